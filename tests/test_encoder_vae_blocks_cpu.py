"""Block-level tests of the SeeCoder and AutoKL host layers (lib/model_zoo/swin.py, seecoder.py, autokl_modules.py, autokl.py,
layers.MultiheadAttention) without a GPU: the real `.hip` methods run over tests/ops_standin.py and are compared with the plain fp64
formulas of tests/encoder_vae_refs.py.  Floor f, tolerance T = 4 f and separation are those of tests/test_blocks_cpu.py (its
docstring derives the margin); the cases are the smallest shapes at which each branch of this host code can go wrong.
"""
import os

import pytest
import torch

import block_refs as BR
import encoder_vae_refs as EV
import kernel_refs as KR
import ops_standin as SI
import pfd_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "encoder_vae_block_paths.txt")
IDS = [c["id"] for c in EV.CASES]
f32 = torch.float32


def _rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


def _sd32(cid, name):
    return {k: v.float() for k, v in BR.built(cid).mods[name].state_dict().items()}


def _r(shape, seed, scale=1.0, shift=0.0):
    return BR.rand16(shape, seed, scale, shift).float()


# ------------------------------------------------------------------------------------------------
# the formulas, in fp32, against the oracle (which tests/test_oracle_golden.py pins to the reference itself)
# ------------------------------------------------------------------------------------------------
def test_swin_formulas_pinned_to_oracle():
    cid = "swin-blk-64-13x18-s6-b2"
    sd = _sd32(cid, "blk")
    x = BR.built(cid).inputs["x"].float().view(2, 13 * 18, 64)
    for shift in (0, 6):
        assert _rel(EV.swin_block(BR.P(sd, dtype=f32), x, 13, 18, 2, shift), O.swin_block(O.SD(sd), x, 13, 18, 2, 12, shift)) <= 1e-5
    sd = _sd32("swin-blk-128-5x7-s6", "blk")                       # a frame below one window
    x = BR.built("swin-blk-128-5x7-s6").inputs["x"].float().view(1, 35, 128)
    assert _rel(EV.swin_block(BR.P(sd, dtype=f32), x, 5, 7, 4, 6), O.swin_block(O.SD(sd), x, 5, 7, 4, 12, 6)) <= 1e-5
    # the walk: the oracle has four stages; the Swin of see-encode-mini is one at small widths (patch embedding with padding,
    # odd merges, every stage's output norm)
    sd = {k[len("imencoder."):]: v for k, v in _sd32("see-encode-mini", "net").items() if k.startswith("imencoder.")}
    img = _r((2, 3, 50, 70), 5, 0.3, 0.5)
    mine = EV.swin_stage_walk(BR.P(sd, dtype=f32), img, 64, [2, 2, 2, 2], [2, 4, 8, 16], (0, 1, 2, 3))
    theirs = O.swin_forward(sd, "", img, embed_dim=64, depths=(2, 2, 2, 2), heads=(2, 4, 8, 16), ws=12)
    assert sorted(mine) == sorted(theirs) == ["res2", "res3", "res4", "res5"]
    for k in theirs:
        assert mine[k].shape == theirs[k].shape and _rel(mine[k], theirs[k]) <= 1e-5, k


def test_seecoder_formulas_pinned_to_oracle():
    sd = _sd32("see-mha-13q-33k", "mha")
    q, k, v = _r((13, 2, 192), 1), _r((33, 2, 192), 2), _r((33, 2, 192), 3)          # seq-first, a batch of 2
    assert _rel(EV.mha(BR.P(sd, dtype=f32), q, k, v, 2), O.mha(O.SD(sd), q, k, v, 2)) <= 1e-5
    # the decoder: the oracle has six layers; B 2, so that the attention over the batch axis is not the identity
    dec = EV._decoder(EV.DEC_LEVELS, 6, 71)
    sd = {k: v.float() for k, v in dec.state_dict().items()}
    feats = {t: _r((2, c, h, w), 10 + n, 1.0, 0.2) for n, (t, (h, w, c)) in enumerate(sorted(EV.DEC_LEVELS.items()))}
    mine = EV.seecoder_decoder(BR.P(sd, dtype=f32), feats, 8, 6)
    theirs = O.seecoder_decoder(sd, "", feats, heads=8)
    for t in theirs:
        assert _rel(mine[t], theirs[t]) <= 1e-5, t
    for cid, (h, w) in (("see-ppe-5x7", (5, 7)), ("see-ppe-6x6", (6, 6))):
        sd = _sd32(cid, "pe")
        theirs = O.ppe_mlp(O.SD(sd), h, w)[0].flatten(1).t()
        assert _rel(EV.ppe_mlp(BR.P(sd, dtype=f32), h, w), theirs) <= 1e-5
    for cid in ("see-qt-4layer", "see-qt-4layer-pa"):
        sd = _sd32(cid, "qt")
        feats = [_r((2, 192, h, w), 20 + n, 1.0, 0.2) for n, (h, w, _) in enumerate(EV.DEC_LEVELS[t] for t in sorted(EV.DEC_LEVELS))]
        mine = EV.query_transformer(BR.P(sd, dtype=f32), feats, 2, 3, 4)
        assert _rel(mine, O.seecoder_qtransformer(sd, "", feats, heads=2, num_gq=3, layers=4)) <= 1e-5, cid


def test_vae_formulas_pinned_to_oracle():
    for cid in ("vae-rb-128", "vae-rb-128-256-nin", "vae-rb-128-smallvar"):
        sd = _sd32(cid, "rb")
        x = BR.nchw(BR.built(cid).inputs["x"].float())
        assert _rel(EV.vae_resnet(BR.P(sd, dtype=f32), x), O.vae_resnet(O.SD(sd), x)) <= 1e-5, cid
    for cid in ("vae-attn-512-8x16-b2", "vae-attn-256-gemm"):
        sd = _sd32(cid, "attn")
        x = BR.nchw(BR.built(cid).inputs["x"].float())
        assert _rel(EV.vae_attn(BR.P(sd, dtype=f32), x), O.vae_attn(O.SD(sd), x)) <= 1e-5, cid
    sd = _sd32("vae-dec-mini", "vae")
    z = BR.built("vae-dec-mini").inputs["z"].float()
    assert _rel(EV.autokl_decode(BR.P(sd, dtype=f32), z, EV.IN_SCALE),
                O.vae_decode(sd, "", z, scale_factor=0.18215, num_resolutions=2, num_res_blocks=1)) <= 1e-5
    x = BR.built("vae-enc-mini").inputs["x"].float()
    sd = _sd32("vae-enc-mini", "vae")
    assert _rel(EV.autokl_encode_moments(BR.P(sd, dtype=f32), x), O.vae_encode_moments(sd, "", x, num_resolutions=2, num_res_blocks=1)) <= 1e-5


# ------------------------------------------------------------------------------------------------
# floor, tolerance, separation
# ------------------------------------------------------------------------------------------------
# A variant no test can see, and why.  dec_levels_fine_first (the levels concatenated fine first, every level keeping its own
# embedding and the split following the same order): every step between the concatenation and the split is row-local -- the
# attention of a DecoderLayer runs over the batch axis, the FFN and the LayerNorms over one token -- so the order of the rows is
# not observable in the result.  The test below demands that it stays exactly invisible: a decoder whose layers start to mix
# tokens makes it a variant like the others.
INVISIBLE = ("dec_levels_fine_first",)


def test_every_wrong_variant_is_separated():
    """every variant, in fp64, is >= 4 T from the formula on some case of every class it applies to"""
    best = {}
    for c in EV.CASES:
        if not c["sep"]:
            continue
        b = BR.built(c["id"])
        T = 4 * SI.floor(c)
        for w in b.applies:
            assert w in EV.WRONG, w
            e = BR.err_units(b.ref(wrong=w), b.ref64, b.B) / T
            if e > best.get((w, c["cls"]), ("", -1.0))[1]:
                best[(w, c["cls"])] = (c["id"], e)
    print("\nvariant                            class    best case                         err / T")
    for (w, cls), (cid, e) in sorted(best.items()):
        print(f"{w:34s} {cls:8s} {cid:32s} {e:9.1f}")
    assert {w for w, _ in best} == set(EV.WRONG), set(EV.WRONG) - {w for w, _ in best}
    weak = {k: v for k, v in best.items() if v[1] < 4.0 and k[0] not in INVISIBLE}
    assert not weak, f"variants no case separates at 4 T: {weak}"
    for w in INVISIBLE:
        assert all(v[1] < 1e-9 for k, v in best.items() if k[0] == w), f"{w} has become visible: take it off INVISIBLE"
    # eps 1e-6 against 1e-5 is visible only where the group variances are small: that case must be the one that tells them apart
    c = BR.CASE["vae-rb-128-smallvar"]
    b = BR.built(c["id"])
    assert BR.err_units(b.ref(wrong="vae_eps_1e5"), b.ref64, b.B) >= 16 * SI.floor(c)


@pytest.mark.parametrize("mode", ["serve", "decline"])
@pytest.mark.parametrize("cid", IDS)
def test_host_path_over_standin(cid, mode):
    """the real .hip methods over the stand-in, every optional form served / declined: within T of the fp64 formula, nothing
    reaches the real library"""
    c = BR.CASE[cid]
    b = BR.built(cid)
    f = SI.floor(c)
    assert 0 < f < 16, f"floor {f}: the stand-in path itself is far from the formula"
    y, _, pol = SI.run_standin(c, mode)
    e = BR.err_units(y, b.ref64, b.B)
    print(f"{cid} {mode}: f {f:.3f} T {4 * f:.3f} err {e:.3f} asked {pol.asked}")
    assert y.shape == b.ref64.shape and e <= 4 * f
    if mode == "decline":
        assert not any(served for _, served in pol.asked)
    assert not SI.FELL_THROUGH


@pytest.mark.parametrize("cid", [c["id"] for c in EV.CASES if c["forward"]])
def test_forward_over_standin(cid):
    c = BR.CASE[cid]
    b = BR.built(cid)
    f = SI.floor(c, fwd=True)
    y = SI.run_standin(c, fwd=True)[0]
    assert BR.err_units(y, BR.ref_of(b, True), b.B) <= 4 * f


@pytest.mark.parametrize("cid", IDS)
def test_census_equals_golden(cid):
    """the calls the host layer makes on the CPU, with the stand-in declining what the recorded device run says the library
    declined, are the recorded ones; the branch the case is written for is among them; two runs give equal bits (run_standin)"""
    c = BR.CASE[cid]
    gold = BR.read_golden_paths(GOLDEN)
    assert set(gold) == set(IDS)
    _, cen, _ = SI.run_standin(c, BR.golden_decisions(gold[cid]), census=True)
    assert cen.log == gold[cid]
    assert c["branch"] in " ".join(cen.log), (c["branch"], cen.log)
    assert cen.again == cen.remembered()


def test_the_unet_cases_are_untouched():
    """this file's cases are registered beside the UNet's, not among them"""
    assert len(BR.CASES) == 54 and not set(IDS) & {c["id"] for c in BR.CASES}
    assert all(BR.CASE[i] is c for i, c in zip(IDS, EV.CASES))


# ------------------------------------------------------------------------------------------------
# the host layer's argument errors: raised before anything is launched
# ------------------------------------------------------------------------------------------------
def test_argument_errors_before_any_launch(monkeypatch):
    SI.install(monkeypatch)
    calls = EV.refusals("cpu")
    cen = BR.Census().install(monkeypatch)
    for what, exc, call in calls:
        with pytest.raises(exc):
            call()
        assert cen.log == [], f"{what}: {cen.log} ran before the refusal"
    assert not SI.FELL_THROUGH


# ------------------------------------------------------------------------------------------------
# the stand-in itself
# ------------------------------------------------------------------------------------------------
def test_standin_refusals_are_the_librarys(monkeypatch):
    from lib.hip import ops
    SI.install(monkeypatch)
    p = KR.swin_problem((1, 12, 12, 1, 6))
    a = (p["qkv"], p["qkv_bias"], p["rpb"], 1, 12, 12, 32, 1)
    y = ops.swin_window_attention(*a, 12, 6, p["scale"])
    assert y.dtype == torch.float16 and float((y.double() - p["ref"]).abs().max()) <= 2.0 ** -11 * p["vmax"]
    for ws, C, shift in ((7, 32, 0), (12, 64, 0), (12, 32, 12), (12, 32, -1)):          # pfd_swin_window_attention_f16
        with pytest.raises(ValueError):
            ops.swin_window_attention(p["qkv"], p["qkv_bias"], p["rpb"], 1, 12, 12, C, 1, ws, shift, p["scale"])
    q = BR.rand16((64, 512), 1)
    vt = BR.rand16((512, 64), 2)
    kw = dict(ldq=512, ldk=512, ldvt=64, q_bs=0, k_bs=0, vt_bs=0)
    assert ops.attention(q, q, vt, 1, 1, 64, 64, 512, 512 ** -0.5, **kw).shape == (64, 512)
    with pytest.raises(ValueError):                                                      # D = 512: H == 1
        ops.attention(q, q, vt, 1, 2, 64, 64, 512, 1.0, **kw)
    with pytest.raises(ValueError):                                                      # D = 512: Nk % 32 == 0
        ops.attention(q, q, vt, 1, 1, 64, 48, 512, 1.0, **kw)
    s = BR.rand16((5, 24), 3, 4.0)
    want = KR.softmax_rows_ref(s, 0.3).half()
    buf = s.clone()
    assert ops.softmax_rows(buf, 0.3, out=buf) is buf and torch.equal(buf, want)          # out may be x
    assert torch.equal(ops.softmax_rows(s, 0.3), want)
    x = BR.rand16((2, 5, 7, 16), 4)
    g, be = BR.rand16((64,), 5, 0.2, 1.0), BR.rand16((64,), 6, 0.1)
    assert torch.equal(ops.layernorm_patch_merge(x, g, be), KR.layernorm_patch_merge_ref(x, g, be).half())
    assert not SI.FELL_THROUGH


def test_ppe_feature_cache(monkeypatch):
    SI.install(monkeypatch)
    pe = BR._dev(BR.built("see-ppe-5x7"), "cpu")[0]["pe"]
    a, b = EV.ppe_cache_check(pe, torch.device("cpu"))
    ref = EV.ppe_mlp(BR.P(BR._sd(BR.built("see-ppe-5x7"), "pe")), 5, 7)
    assert BR.err_units(a, ref, 1) <= 4 * SI.floor(BR.CASE["see-ppe-5x7"])
    # the host table is the fp16 rounding of the fp32 features the formula states
    f = pe.features(5, 7, torch.device("cpu"))
    assert f.shape == (35, 80) and f.dtype == torch.float16 and torch.equal(f, pe._features_host(5, 7).half())


def test_attn_forms_agree_over_standin():
    """the fused launch and the chunked GEMM form of AttnBlock on the same input: each within its T, within 2 T of each other"""
    base = BR.CASE["vae-attn-512-gemm-12x16-rows128"]
    b = BR.built(base["id"])
    ys, Ts = [], []
    for sw in ({}, dict(base["switches"]), {"PFD_VAE_ATTN": "gemm"}):
        c = dict(base, switches=sw)
        T = 4 * SI.floor(c)
        y, cen, _ = SI.run_standin(c, census=True)
        assert ("softmax_rows[out]" in cen.log) == bool(sw) and ("attention" in cen.log) == (not sw)
        assert cen.log.count("softmax_rows[out]") == {0: 0, 1: 2, 2: 4}[len(sw)]          # ROWS 4096: one chunk per sample
        assert BR.err_units(y, b.ref64, b.B) <= T
        ys.append(y)
        Ts.append(T)
    for y in ys[1:]:
        assert max(BR.err_units(ys[0], y.double(), b.B), BR.err_units(y, ys[0].double(), b.B)) <= 2 * max(Ts)
