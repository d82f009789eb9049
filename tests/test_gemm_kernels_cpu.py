"""CPU: the fp64 GEMM / convolution reference of tests/kernel_refs.py (gemm_ref), its per-element bound (gemm_allowance) and the
case table (GEMM_CASES) that tests/test_gemm_kernels_gpu.py holds the kernels behind pfd_gemm_f16 to -- the reference pinned to
torch's own F.linear / F.conv2d / F.interpolate / F.layer_norm / F.group_norm compositions, shown to index the strided, poisoned
operands like dense ones, to stay far inside the bound in fp32, to tell every wrong variant of GEMM_MUTANTS from the right one
in every kernel class it applies to, and the table checked against the wide-tile dispatcher itself (tools/cpu_emu, a dry run)."""
import functools
import os
import re
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

import kernel_refs as KR

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get("EMU_CXX", "/opt/rocm/lib/llvm/bin/clang++")
FIXTURE = os.path.join(REPO, "tests", "golden", "gemm_kernel_cases.txt")
ALL = KR.GEMM_CASES
ids = [c["id"] for c in ALL]


def _bound(p, key="out"):
    c = p["case"]
    a = KR.gemm_allowance(p, c["splits"], KR.gemm_case_is_wide(c))
    r = KR.gemm_ref(p)
    return r, {k: KR.round_once_bound(r[k], a[k]) for k in a}


# ------------------------------------------------------------------------------------------------
# the reference is torch's
# ------------------------------------------------------------------------------------------------
def _torch_composition(p):
    """the same operation out of torch's own layers, fp64"""
    c = p["case"]
    M, N, K, act = c["M"], c["N"], c["K"], c["act"]
    W = p["W"].double()
    if c["kind"] == "conv":
        ks, stride, pad, ups, Ho, Wo = c["geom"]
        x = (p["A"] if p["A2"] is None else torch.cat([p["A"], p["A2"]], -1)).double().permute(0, 3, 1, 2)
        if c["gn_pro"] is not None:
            t = p["gn_table"].double()
            x = x * t[:, 0, :, None, None] + t[:, 1, :, None, None]
            x = (F.silu(x) if c["gn_pro"][1] else x).half().double()
        if ups:
            x = F.interpolate(x, scale_factor=2, mode="nearest")
        Hin, Win = x.shape[2:]
        x = F.pad(x, (pad, max(0, (Wo - 1) * stride + ks - Win - pad), pad, max(0, (Ho - 1) * stride + ks - Hin - pad)))
        y = F.conv2d(x, W.view(N, ks, ks, -1).permute(0, 3, 1, 2), stride=stride)[:, :, :Ho, :Wo]
        acc = y.permute(0, 2, 3, 1).reshape(M, N)
    else:
        x = p["A"].double() if p["A2"] is None else torch.cat([p["A"], p["A2"]], 1).double()
        if c["ln"] is not None:
            x = F.layer_norm(x, (K,), None, None, c["ln_eps"])
        x = torch.cat([x.new_zeros((c["zero_rows"], K)), x])
        acc = F.linear(x, W)
    pre = acc
    if p["bias"] is not None:
        pre = pre + (p["bias"].double()[:, None] if c["bias_per_row"] else p["bias"].double())
    if p["rowvec"] is not None:
        pre = pre + p["rowvec"].double().repeat_interleave(c["rows_per_rv"], 0)[:M]
    out = pre[:, :N // 2] * F.gelu(pre[:, N // 2:]) if act == KR.ACT_GEGLU else (pre, F.gelu(pre), F.relu(pre), F.silu(pre))[act]
    if p["R"] is not None:
        r = p["R"].double()
        out = out + (torch.cat([r, r])[:M] if c["res_rows"] else r)
    res = {"out": out}
    if c["n_split"]:
        res = {"out": out[:, :c["n_split"]], "out_t": (acc + p["bias"].double())[:, c["n_split"]:].t()}
    return res


@pytest.mark.parametrize("cid", ids)
def test_reference_is_torchs_composition(cid):
    p = KR.gemm_problem(cid)
    got, want = KR.gemm_ref(p), _torch_composition(p)
    assert set(got) == set(want)
    for k in got:
        assert got[k].dtype == torch.float64 and got[k].shape == want[k].shape
        e = float((got[k] - want[k]).abs().max())
        assert e <= 1e-12, (k, e)


def test_side_output_references_are_torchs():
    g = torch.Generator().manual_seed(3)
    y = torch.randn((256, 640), generator=g).half()
    gamma, beta = torch.randn(640, generator=g).half(), torch.randn(640, generator=g).half()
    want = F.group_norm(y.double().view(2, 128, 640).permute(0, 2, 1), 32, gamma.double(), beta.double(), 1e-5).permute(0, 2, 1)
    assert float((KR.groupnorm32_ref(y, 128, gamma, beta, 1e-5, False) - want.reshape(256, 640)).abs().max()) <= 1e-12
    assert float((KR.groupnorm32_ref(y, 128, gamma, beta, 1e-5, True) - F.silu(want).reshape(256, 640)).abs().max()) <= 1e-12
    ln = KR.ln_out_ref(y)
    assert ln.shape == (256, 4, 2) and float((ln[:, 1, 0] - y.double()[:, 160:320].sum(1)).abs().max()) <= 1e-12
    gn = KR.gn_out_ref(y)                                                  # 20 channels per group, 8 groups per 160-column tile
    assert gn.shape == (4, 4, 16, 2) and bool(torch.isnan(gn[:, :, 8:]).all())
    blk = y.double()[64:128, 160 + 40:160 + 60]
    assert float((gn[1, 1, 2] - torch.stack([blk.sum(), (blk * blk).sum()])).abs().max()) <= 1e-10


@pytest.mark.parametrize("cid", ids)
def test_strided_poisoned_operands_equal_dense_ones(cid):
    """the views a launch is handed (column slices of NaN-filled buffers, packed weights) give the reference's bits back: the
    packing of the test is the inverse of the header's element maps, and no poisoned element is read"""
    p = KR.gemm_problem(cid)
    c = p["case"]
    o = KR.gemm_operands(p)
    N = c["N"]
    W = KR.gemm_view(*o["W"])
    assert bool(torch.isnan(o["A"][0]).any())
    bias = o["bias"]
    if c["w_tiled"]:                    # read the tiled pack back through the header's element map
        T, K = 160 if N % 160 == 0 else 128, c["K"]
        n, k = torch.arange(N)[:, None], torch.arange(K)[None]
        W = W.reshape(-1)[(((n // T) * (K // 64) + k // 64) * T + n % T) * 64 + k % 64]
    if c["act"] == KR.ACT_GEGLU:
        g = 2 if N % 160 == 0 else 32
        W = torch.cat(KR.geglu_unpack(W, g))
        bias = torch.cat(KR.geglu_unpack(bias[:, None], g)).reshape(-1)
    p2 = dict(p, A=KR.gemm_view(*o["A"]), A2=None if p["A2"] is None else KR.gemm_view(*o["A2"]), W=W, bias=bias)
    assert p2["A"].stride(-2) > p2["A"].shape[-1]
    a, b = KR.gemm_ref(p), KR.gemm_ref(p2)
    for k in a:
        assert torch.equal(a[k], b[k]), k


# ------------------------------------------------------------------------------------------------
# the bound: fp32 far inside, every mutant far outside
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ids)
def test_fp32_formula_stays_within_an_eighth_of_the_bound(cid):
    p = KR.gemm_problem(cid)
    r, b = _bound(p)
    r32 = KR.gemm_ref(p, dtype=torch.float32)
    for k in b:
        ratio = float(((r32[k].double() - r[k]).abs() / b[k]).max())
        assert ratio <= 0.125, (k, ratio)


@functools.lru_cache(maxsize=None)
def _bound_of(cid):
    return _bound(KR.gemm_problem(cid))


def _excess(cid, mutant):
    p = KR.gemm_problem(cid)
    r, b = _bound_of(cid)
    m = KR.gemm_ref(p, mutant=mutant)
    c = p["case"]
    if c["gnf"] is False:
        # the raw result is not stored: the GPU file sees only its GroupNorm, held to the allowance that carries the raw bound
        rows, gn = c["geom"][4] * c["geom"][5], (p["gnf_gamma"], p["gnf_beta"], 1e-5, True)
        y, ym = KR.groupnorm32_ref(r["out"], rows, *gn), KR.groupnorm32_ref(m["out"], rows, *gn)
        ay = KR.groupnorm32_allowance(r["out"], rows, *gn, float(b["out"].max()))
        return float(((ym - y).abs() / KR.round_once_bound(y, ay)).max())
    return max(float(((m[k] - r[k]).abs() / b[k]).max()) for k in b)


@pytest.mark.parametrize("mutant", KR.GEMM_MUTANTS)
def test_operands_separate_the_mutant_in_every_class(mutant):
    """a wrong kernel of this kind exceeds the bound at least 4 times on some element of some case of EVERY kernel class the
    mutant applies to (a class without such a case means a case is missing from the table)"""
    by = {}
    for c in ALL:
        if KR.gemm_mutant_applies(mutant, c):
            by.setdefault(c["cls"], []).append(c["id"])
    assert by, mutant
    for cls, cids in sorted(by.items()):
        ex = {cid: _excess(cid, mutant) for cid in cids}
        best = max(ex, key=ex.get)
        print(f"[gemm-kernels] mutant {mutant} / {cls}: {sum(v >= 4 for v in ex.values())} of {len(ex)} cases separate it, "
              f"worst excess {ex[best]:.1f} x bound ({best})")
        assert ex[best] >= 4.0, (mutant, cls, ex)


KINDED = [c for c in ALL if c["operands"] != "unit"]


def test_every_operand_kind_separates_the_mutants():
    """the same on the operand kinds one by one: on `act` and on `cancel` operands every mutant still exceeds the bound at least
    4 times in every class that has cases of the kind it applies to; on `exact` operands, where the GPU file asserts bits, it
    changes bits of the rounded reference"""
    for fam in ("act", "cancel"):
        by = {}
        for c in KINDED:
            if KR.gemm_operand_kind(c)[0] == fam:
                for m in KR.GEMM_MUTANTS:
                    if KR.gemm_mutant_applies(m, c):
                        by.setdefault((m, c["cls"]), set()).add(KR.gemm_problem_key(c["id"]))
        assert by
        memo = {}
        for (m, cls), keys in sorted(by.items()):
            # (one case per problem, the one with the fewest slabs: the formula mutants do not depend on the variant)
            cids = [min((c["id"] for c in KINDED if KR.gemm_problem_key(c["id"]) == k), key=lambda i: KR.GEMM_CASE[i]["splits"]) for k in keys]
            ex = {cid: memo.setdefault((cid, m), _excess(cid, m)) for cid in cids}
            best = max(ex, key=ex.get)
            print(f"[gemm-kernels] {fam}: mutant {m} / {cls}: worst excess {ex[best]:.1f} x bound ({best})")
            assert ex[best] >= 4.0, (fam, m, cls, ex)
    n = 0
    for c in KINDED:
        if KR.gemm_operand_kind(c)[0] == "exact" and c["splits"] == 1:
            p = KR.gemm_problem(c["id"])
            for m in KR.GEMM_MUTANTS:
                if KR.gemm_mutant_applies(m, c):
                    assert not torch.equal(KR.gemm_ref(p, mutant=m)["out"].half(), KR.gemm_ref(p)["out"].half()), (c["id"], m)
                    n += 1
    assert n >= 3


def _slab_counts(c):
    """every slab count the table uses on the case's problem (1 = unsplit)"""
    return sorted({d["splits"] for d in ALL if KR.gemm_problem_key(d["id"]) == KR.gemm_problem_key(c["id"])})


@pytest.mark.parametrize("cid", [c["id"] for c in KINDED])
def test_operand_kinds_meet_their_conditions(cid):
    """from the fp64 reference alone.  act: max |ref| <= 3e4 and every slab partial of every split count of the table <= 3e4.
    cancelS: max |partial| <= 3e4 and, at split count S, the median over the elements of max_s |P_s| / |ref| >= 20.  exactS: every
    slab partial of every split count and the unsplit sum are integers that f16 holds exactly, the unsplit sum below 2^24, the
    result exact in f16.  All: max |ref| <= 3e4 (the sentinel of the GPU file, -61440, is outside every result)."""
    c = KR.GEMM_CASE[cid]
    fam, S = KR.gemm_operand_kind(c)
    p = KR.gemm_problem(cid)
    ref = KR.gemm_ref(p)
    assert all(bool(torch.isfinite(v).all()) for v in ref.values())
    pmax = 0.0
    for s in _slab_counts(c):
        for P, _ in KR.gemm_slab_partials(p, s):
            pmax = max(pmax, float(P.abs().max()))
            if fam == "exact":
                assert torch.equal(P.half().double(), P), (cid, s)
    rmax = float(ref["out"].abs().max())
    msg = f"[gemm-kernels] {cid}: max |ref| {rmax:.4g}, max |partial| over the slab counts {_slab_counts(c)} {pmax:.4g}"
    assert pmax <= 3e4 and rmax <= 3e4, (cid, pmax, rmax)
    if fam == "cancel":
        if c["splits"] > 1:             # (the second figure is recorded only: behind SiLU / GELU half of the results are next to 0)
            big = torch.stack([P.abs() for P, _ in KR.gemm_slab_partials(p, c["splits"])]).amax(0)
            med = [float((big / v.abs()).median()) for v in (ref["out"], KR.gemm_ref(p, parts=True)["acc"])]
            msg += f", median max_s |P_s| / |ref| {med[0]:.4g} (/ |sum over K|, in front of the epilogue: {med[1]:.4g})"
            assert med[0] >= 20.0, (cid, med)
    elif fam == "exact":
        assert c["act"] in (KR.ACT_NONE, KR.ACT_RELU)
        acc = KR.gemm_ref(p, parts=True)["acc"]
        assert float(acc.abs().max()) < 2.0 ** 24 and torch.equal(ref["out"].half().double(), ref["out"])
    print(msg)


SPLIT_UNIT = ["lin160-v41-split2-300x320x320-plain", "lin160-v44-split4-300x320x320-silu-rv-res", "patch-v96-c192-2x16x16-split2",
              "conv-v22-c128-s1p1-9x7", "abi-ln640-split2"]


@pytest.mark.parametrize("cid", [c["id"] for c in KINDED] + SPLIT_UNIT)
def test_documented_arithmetic_in_fp32_meets_the_bound(cid):
    """kernel_refs.gemm_kernel_model -- per-range fp32 contractions, each rounded to f16, summed in fp32 in slab order, the fp32
    epilogue, the staged value, one final rounding: what include/pfd_hip.h says a launch computes -- is inside the bound the GPU
    file holds the kernels to.  (Not inside an eighth of it, as the unrounded fp32 formula is: the slab roundings are what the
    slab term of the allowance is there for, and a cancelling case uses most of it.)  An `exact` case gives the bits of the
    fp64 reference rounded once."""
    p = KR.gemm_problem(cid)
    c = p["case"]
    wide = KR.gemm_case_is_wide(c)
    ref, a = KR.gemm_ref(p), KR.gemm_allowance(p, c["splits"], wide)
    got = KR.gemm_kernel_model(p, c["splits"], wide)
    for k in a:
        ratio, used = KR.bound_ratio(got[k], ref[k], a[k])
        print(f"[gemm-kernels] {cid} documented arithmetic, fp32: {k} err / bound {ratio:.3f}, allowance used {used:.3f}")
        assert ratio <= 1.0, (cid, k, ratio)
        if KR.gemm_operand_kind(c)[0] == "exact":
            assert torch.equal(got[k], ref[k].half())


def test_mutants_apply_where_they_should():
    ap = {m: {c["cls"] for c in ALL if KR.gemm_mutant_applies(m, c)} for m in KR.GEMM_MUTANTS}
    assert ap["last_k_dropped"] == set(KR.GEMM_CLASSES)
    assert ap["pad_tap_reads_edge"] == {"conv", "patch", "narrow"} and ap["tap_crosses_sample"] == {"conv", "patch", "narrow"}
    assert ap["pad_before_normalise"] == {"patch"} and ap["ups_gather_ceil"] == {"conv"}
    assert ap["rowvec_row_by_tile"] >= {"lin160", "lin128", "reg", "conv", "abi"}
    assert ap["bias_after_act"] >= {"lin160", "lin128", "geglu", "reg", "conv", "patch", "abi"}
    assert ap["geglu_halves_swapped"] == {"geglu", "abi"}
    for m in ("residual_no_wrap", "residual_wrap_off_by_one", "zero_rows_rounded_to_tile", "k_split_second_source_offset",
              "ln_mean_of_first_part", "tail_transposed_without_bias"):
        assert ap[m] == {"abi"}, m


# ------------------------------------------------------------------------------------------------
# the cases reach what they are listed for
# ------------------------------------------------------------------------------------------------
TABLES = ALL + KR.GEMM_RANGE_CASES      # (the cases beyond the f16 range are launches like any other to the dispatcher)


def _records():
    seen, out = set(), []
    for c in TABLES:
        r = KR.gemm_case_record(c)
        if r not in seen:
            seen.add(r)
            out.append(r)
    return out


def test_fixture_holds_the_records_of_the_table():
    """tests/golden/gemm_kernel_cases.txt is the table's records in the 24-integer TRACE_FIELDS form (PFD_GEMM_CASES_WRITE=1
    rewrites it)"""
    text = "".join(" ".join(str(v) for v in r) + "\n" for r in _records())
    if os.environ.get("PFD_GEMM_CASES_WRITE") == "1":
        open(FIXTURE, "w").write(text)
    assert open(FIXTURE).read() == text
    from lib.hip import ops
    assert len(ops.TRACE_FIELDS) == 24 and all(len(r) == 24 for r in _records())


@pytest.fixture(scope="module")
def sweep(tmp_path_factory):
    if not os.path.exists(CXX):
        pytest.skip("clang++ of the ROCm toolchain not available")
    out = str(tmp_path_factory.mktemp("pfd_cpu_emu_gemm_cases"))
    subprocess.run([sys.executable, os.path.join(REPO, "tools", "cpu_emu", "build.py"), out], check=True, stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(out, "emu_gemm"), "--dispatch", "--sweep", FIXTURE], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    return KR.parse_dispatch_sweep(r.stdout)


def _fallthrough_kernel(c):
    """what pfd_gemm_f16_ex launches behind the wide-tile dispatcher (csrc/gemm_conv.hip, its last lines, restated)"""
    M, N = c["M"], c["N"]
    if c["tile"] == 0 and c["kind"] == "conv" and N <= 16:
        return "conv3x3_narrow_kernel"
    if c["act"] == KR.ACT_GEGLU:
        return "gemm_conv_kernel<2, 2, false>"
    if c["tile"]:
        return f"gemm_conv_kernel<{c['tile'] // 10}, {c['tile'] % 10}, false>"
    blocks = lambda bm, bn: -(-M // bm) * -(-N // bn)
    waste = -(-N // 128) * 128 / N
    if blocks(128, 128) >= 512 and waste <= 1.13:
        return "gemm_conv_kernel<2, 2, false>"
    if blocks(128, 64) >= 384 and M >= 128:
        return "gemm_conv_kernel<2, 1, false>"
    if N > 64 and blocks(64, 128) >= 384 and waste <= 1.13:
        return "gemm_conv_kernel<1, 2, false>"
    return "gemm_conv_kernel<1, 1, false>"


def test_cases_are_served_as_the_table_says(sweep):
    """every wide-tile case: `emu_gemm --dispatch --sweep` serves its record (its base record where the record cannot express the
    case) under the case's variant and split code with the instantiation, the slab count and the K tiles per slab that the table
    and kernel_refs.gemm_slab_ranges say, and the reduction kernel behind a split"""
    n = 0
    for c in TABLES:
        if not KR.gemm_case_is_wide(c):
            # csrc/gemm_conv.hip: a register-staged tile code goes there directly (pfd_gemm_f16_ex), the heuristic only when the
            # wide-tile dispatcher declines the record (return value 1) -- then the narrow kernel or the register-staged tile
            # the rules at the end of pfd_gemm_f16_ex pick, restated in _register_tile
            assert c["tile"] < 1000 and c["kernel"] == _fallthrough_kernel(c), (c["id"], c["kernel"])
            if c["tile"] == 0:
                rc = sweep[(KR.gemm_case_record(c), 0, 0)]
                assert rc[0] == 1 and rc[1] is None, (c["id"], rc)
            continue
        enc = c["tile"] - 1000 if c["tile"] else 0
        v, s = enc // 100, enc % 100
        assert (v, s) != (0, 0) or c["tile"] == 0
        rc, kern, splits, kt, red = sweep[(KR.gemm_case_record(c), v, s)]
        assert rc == 0, (c["id"], rc)
        assert kern == (c["base_kernel"] or c["kernel"]), (c["id"], kern)
        nk = c["K"] // 64 if c["cls"] != "patch" else c["K"] // 9 // 64
        rng = KR.gemm_slab_ranges(nk, splits)
        assert splits == c["splits"] == len(rng) and kt == rng[0][1] - rng[0][0] and rng[-1][1] == nk, (c["id"], splits, kt, rng)
        if s > 1:
            assert kt == -(-nk // s) and splits == -(-nk // kt)
        assert red == c["reduce"] and (red is not None) == (splits > 1), (c["id"], red)
        n += 1
    assert n > 200


def test_cases_cover_every_kernel_instantiation():
    """every instantiation the pinned dispatch table (tests/golden/gemm_dispatch.txt) names, except the phase forms of
    gemm160ws_kernel (PH = true: tests/test_upsample_phase_gpu.py), is the kernel of at least one case; so are the four
    register-staged tiles, the narrow convolution and the three split-K reductions"""
    named = set()
    for line in open(os.path.join(REPO, "tests", "golden", "gemm_dispatch.txt")):
        named.update(m.group(1) for m in re.finditer(r" \| ([A-Za-z0-9_]+(?:<[^>]*>)?) grid", line))
    named = {k for k in named if not re.fullmatch(r"gemm160ws_kernel<.*, true>", k)}
    assert len(named) >= 38
    have = {c["kernel"] for c in ALL} | {c["reduce"] for c in ALL}
    assert not named - have, sorted(named - have)
    for tm in (1, 2):
        for tn in (1, 2):
            assert f"gemm_conv_kernel<{tm}, {tn}, false>" in have
    assert {"conv3x3_narrow_kernel", "splitk_reduce_kernel", "splitk_reduce_gn_kernel", "splitk_reduce_gnorm_kernel"} <= have
    # every forced variant of the header, rings with fewer K tiles than stages, split counts that do not divide the K tiles
    variants = {(c["tile"] - 1000) // 100 for c in ALL if c["tile"] >= 1000}
    assert variants >= {22, 23, 24, 25, 41, 43, 44, 47, 48, 82, 83, 84, 96, 98, 99}
    assert any(c["K"] == 64 and "gemm160_kernel<2, 2, false, 4, 5>" == c["kernel"] for c in ALL)
    assert {c["splits"] for c in ALL if c["K"] == 320 and c["tile"] % 100 in (2, 4, 8)} == {2, 3, 5}
    assert {c["zero_rows"] for c in ALL} >= {100, 256} and all(c["M"] <= 1024 for c in ALL)
