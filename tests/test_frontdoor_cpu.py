"""CPU: the request front door, pinned.  PromptFreePipeline.generate and PromptFreeServer.submit / _generate over the stand-ins
of tests/frontdoor_standin.py: for every named request -- through `generate`, through `submit` alone and through `submit`
coalesced with a second request, with and without mixed_batches -- the ordered calls of the net and the device ops, what the
sampler was handed (types, dtypes, shapes, devices, a sha256 of the bytes, the repr of numbers), what came back, every
request's key() and shareable() and the batches run -- held in the fixture as a sha256 over all those lines and a readable digest; for every per-sample argument the same at rank 0 and 1 of world size 2;
for every bad-argument set of the feature tests, from both doors, the exception and that nothing was called or queued before
it, line for line.  All of it against tests/golden/frontdoor_calls.txt: a change of the front door that is meant to change
nothing changes no line."""
import pytest

import frontdoor_standin as F


@pytest.fixture(scope="module")
def pinned():
    return F.read_fixture()


def _same(got, want, name, full=None):
    assert want is not None, f"{name}: not in the fixture"
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, (f"{name}, line {i}:\n  now:    {g}\n  pinned: {w}" +
                        ("" if full is None else "\nthe full record now (python tests/frontdoor_standin.py --show gives the one "
                         "of another commit):\n" + "\n".join(full)))
    assert len(got) == len(want), f"{name}: {len(got)} lines now, {len(want)} pinned"


def test_fixture_holds_exactly_the_sections_of_the_tables(pinned):
    want = [f"{c} / {w}" for c in F.CASE_IDS for w in ("generate", "submit", "coalesced", "coalesced mixed_batches")]
    want += [f"ranked {c} / rank {r} of 2" for c in F.RANKED_IDS for r in range(2)]
    want += [f"refusal {r}" for r in F.REFUSAL_IDS] + [f"refusal submit_only[{i}]" for i in range(len(F.SUBMIT_ONLY))]
    assert list(pinned) == want and len(set(want)) == len(want)


@pytest.mark.parametrize("cid", F.CASE_IDS)
def test_named_request_through_both_doors(cid, pinned, monkeypatch):
    for way, lines in F.run_case(F.CASES[F.CASE_IDS.index(cid)], monkeypatch).items():
        _same(F.pin(lines), pinned.get(f"{cid} / {way}"), f"{cid} / {way}", lines)


@pytest.mark.parametrize("cid", F.RANKED_IDS)
def test_per_sample_arguments_and_seeded_starts_rank_by_rank(cid, pinned, monkeypatch):
    for way, lines in F.run_ranked(F.RANKED[F.RANKED_IDS.index(cid)], monkeypatch).items():
        _same(F.pin(lines), pinned.get(f"ranked {cid} / {way}"), f"ranked {cid} / {way}", lines)


@pytest.mark.parametrize("rid", F.REFUSAL_IDS)
def test_refusal_from_both_doors(rid, pinned, monkeypatch):
    _same(F.pin_refusal(F.run_refusal(dict(F.REFUSALS)[rid], monkeypatch)), pinned.get(f"refusal {rid}"), f"refusal {rid}")


@pytest.mark.parametrize("i", range(len(F.SUBMIT_ONLY)))
def test_what_submit_alone_refuses(i, pinned, monkeypatch):
    _same(F.run_submit_only(F.SUBMIT_ONLY[i], monkeypatch), pinned.get(f"refusal submit_only[{i}]"), f"refusal submit_only[{i}]")
    assert "raises" in pinned[f"refusal submit_only[{i}]"][0] and pinned[f"refusal submit_only[{i}]"][0].endswith("raise: 0")


def test_a_request_that_starts_from_a_picture_draws_no_xT(pinned):
    """every x_T draw of either door is a line of the record: none for an img2img or a masked request, one per request else"""
    for name, rec in pinned.items():
        if " / " not in name or "raises" in rec[2] and "returns" not in rec[2]:
            continue
        draws = rec[0].count("host.shard_xT")
        if name.startswith(("init_", "mask_", "composite", "ranked init", "ranked mask")):
            assert draws == 0 and "ops.latent_start" in rec[0], name
        else:
            assert draws == (2 if " / coalesced" in name else 1), name


def test_the_record_tells_what_the_issue_asks_it_to_tell(pinned, monkeypatch):
    """'solver' is absent for 'ddim' and present otherwise; a Python float scale is told from a vector; the digest moves with
    any line of the record; a refusal that a door makes touched nothing and queued nothing"""
    run = lambda cid: F.run_case(F.CASES[F.CASE_IDS.index(cid)], monkeypatch)      # noqa: E731
    plain, dpm, ps = run("plain"), run("dpmpp_2m"), run("scale_per_sample")
    assert not any("how['solver']" in ln for ln in plain["generate"] + plain["coalesced"])
    assert "  how['solver'] = str 'dpmpp_2m'" in dpm["generate"] and "  how['solver'] = str 'dpmpp_2m'" in dpm["submit"]
    assert "how.solver=str 'dpmpp_2m'" in pinned["dpmpp_2m / submit"][1] and "how." not in pinned["plain / submit"][1]
    assert "  c_info['unconditional_guidance_scale'] = float 2.0" in plain["generate"]
    assert any(ln.startswith("  c_info['unconditional_guidance_scale'] = Tensor float32[2] cpu") for ln in ps["generate"])
    assert pinned["plain / generate"][1].endswith("c.unconditional_guidance_scale=float 2.0")
    assert "c.unconditional_guidance_scale=float32[2]:" in pinned["scale_per_sample / generate"][1]
    assert "c.unconditional_guidance_scale=float32[3]:" in pinned["scale_per_sample / coalesced mixed_batches"][1]
    moved = [ln.replace("float 2.0", "float 2.5") for ln in plain["generate"]]
    assert F.pin(moved)[0][:39] != F.pin(plain["generate"])[0][:39] == pinned["plain / generate"][0][:39]
    for rid in F.REFUSAL_IDS:
        for ln in pinned[f"refusal {rid}"]:
            if ("raises" in ln or "the same" in ln) and rid != "x":
                assert "calls before the raise: 0" in ln, (rid, ln)
            if ln.startswith(("submit: raises", "submit: the same")):
                assert ln.endswith("queued: 0 | on the caller's thread: True"), (rid, ln)
