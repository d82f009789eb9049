"""CPU: the cases of kernel_refs.GEMM_RANGE_CASES -- split-K partial sums and staged values beyond the f16 range -- that
tests/test_gemm_range_gpu.py holds the kernels behind pfd_gemm_f16 to, qualified from the fp64 reference alone: the reference
is torch's, the element classes (finite / nonfinite / band) have the shares the GPU test needs, the expected patterns are the
IEEE evaluation of the two header sentences (PfdGemmDesc.ws and epi(v) of include/pfd_hip.h; kernel_refs.gemm_kernel_model), the
three wrong arithmetics of GEMM_ARITH_MUTANTS are told from the right one, the library's own split-K paths run the contract on the
host (tools/cpu_emu), and the documented arithmetic is compared with the fp16 pipeline of the model this library ports
(kernel_refs.half_pipeline; recorded in profiles/gemm_kernel_tests.md, "Operand kinds")."""
import functools
import os
import subprocess
import sys

import pytest
import torch

import kernel_refs as KR
import test_gemm_kernels_cpu as base

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get("EMU_CXX", "/opt/rocm/lib/llvm/bin/clang++")
RANGE = KR.GEMM_RANGE_CASES
rids = [c["id"] for c in RANGE]
KINDED = [c for c in KR.GEMM_CASES if c["operands"] != "unit"]


@functools.lru_cache(maxsize=None)
def _model(cid, mutant=None):
    p = KR.gemm_problem(cid)
    c = p["case"]
    return KR.gemm_kernel_model(p, c["splits"], KR.gemm_case_is_wide(c), mutant)["out"]


@functools.lru_cache(maxsize=None)
def _classes(cid):
    p = KR.gemm_problem(cid)
    c = p["case"]
    return KR.gemm_range_classes(p, c["splits"], KR.gemm_case_is_wide(c))


def _pattern(t):
    """0 finite, 1 NaN, 2 +inf, 3 -inf"""
    return torch.isnan(t) * 1 + torch.isposinf(t) * 2 + torch.isneginf(t) * 3


@pytest.mark.parametrize("cid", rids)
def test_reference_and_operands_as_for_the_main_table(cid):
    base.test_reference_is_torchs_composition(cid)
    base.test_strided_poisoned_operands_equal_dense_ones(cid)
    base.test_fp32_formula_stays_within_an_eighth_of_the_bound(cid)


@pytest.mark.parametrize("cid", rids)
def test_range_cases_meet_their_conditions(cid):
    """band elements (left out on the GPU) are at most 0.5 % of the output; a launch that the header says overflows has between
    0.5 % and 10 % nonfinite elements, its unsplit / register-staged / split counterpart none at all; max |ref| <= 3e4 on the
    finite elements; on the nonfinite ones the documented arithmetic is not finite except behind RELU, elsewhere it is
    finite and inside the bound"""
    p = KR.gemm_problem(cid)
    c = p["case"]
    fam, _ = KR.gemm_operand_kind(c)
    wide = KR.gemm_case_is_wide(c)
    cls, ref, exp = _classes(cid), KR.gemm_ref(p)["out"], _model(cid)
    share = [float((cls == k).float().mean()) for k in range(3)]
    pmax = max(float(P.abs().max()) for P, _ in KR.gemm_slab_partials(p, c["splits"])) if c["splits"] > 1 else 0.0
    pat = _pattern(exp)[cls == 1]
    print(f"[gemm-range] {cid}: finite / nonfinite / band shares {share[0]:.4f} / {share[1]:.4f} / {share[2]:.4f}, max |partial| {pmax:.4g}, "
          f"max |ref| on finite elements {float(ref[cls == 0].abs().max()):.4g}; expected on the nonfinite elements: "
          f"{int((pat == 0).sum())} finite, {int((pat == 1).sum())} NaN, {int((pat == 2).sum())} +inf, {int((pat == 3).sum())} -inf")
    overflows = (fam == "overflow" and c["splits"] > 1) or (fam == "staged" and wide and c["splits"] == 1)
    assert share[2] <= 0.005
    assert 0.005 <= share[1] <= 0.10 if overflows else share[1] == 0.0 and share[2] == 0.0, share
    assert float(ref[cls == 0].abs().max()) <= 3e4 or not overflows
    assert bool(torch.isfinite(ref).all())
    fin = cls == 0
    assert bool(torch.isfinite(exp[fin]).all())
    a = KR.gemm_allowance(p, c["splits"], wide)["out"]
    assert float(((exp.double() - ref).abs() / KR.round_once_bound(ref, a))[fin].max()) <= 1.0
    if overflows:
        if c["act"] == KR.ACT_RELU:
            assert bool(((pat == 0) | (pat == 2)).all()) and bool((exp[cls == 1][pat == 0] == 0).all()) and int((pat == 0).sum()) > 0
        else:
            assert bool((pat != 0).all())
        assert int((pat == 2).sum()) > 0 and (fam == "staged" or c["act"] == KR.ACT_RELU or int((pat == 1).sum()) > 0)
        if fam == "staged":
            assert int((pat == 3).sum()) > 0 and float(ref[cls == 1].abs().max()) < 5e4      # (the fp64 result is an ordinary f16 value)


def _pairs():
    """(overflowing launch, its finite counterpart on the same operands)"""
    by = {}
    for c in RANGE:
        by.setdefault(KR.gemm_problem_key(c["id"]), []).append(c)
    out = []
    for cs in by.values():
        hot = [c for c in cs if float((_classes(c["id"]) == 1).float().mean()) > 0]
        out += [(h["id"], q["id"]) for h in hot for q in cs if q not in hot]
    return out


def test_every_overflowing_launch_has_a_finite_counterpart():
    pairs = _pairs()
    hot = {h for h, _ in pairs}
    assert hot == {c["id"] for c in RANGE if float((_classes(c["id"]) == 1).float().mean()) > 0} and len(hot) >= 10
    for h, q in pairs:
        ph, pq = KR.gemm_problem(h), KR.gemm_problem(q)
        assert all(torch.equal(ph[k], pq[k]) for k in ("A", "W")) and bool(torch.isfinite(_model(q)).all()), (h, q)


# ------------------------------------------------------------------------------------------------
# three wrong arithmetics
# ------------------------------------------------------------------------------------------------
def test_slab_saturates_changes_every_overflow_pattern():
    """slabs that clamp to +-65504 instead of giving inf: no NaN, no inf from a slab -- the class pattern of every overflowing
    split launch changes"""
    n = 0
    for c in RANGE:
        if KR.gemm_operand_kind(c)[0] == "overflow" and c["splits"] > 1:
            hot = _classes(c["id"]) == 1
            right, wrong = _pattern(_model(c["id"]))[hot], _pattern(_model(c["id"], "slab_saturates"))[hot]
            differ = float((right != wrong).float().mean())
            print(f"[gemm-range] slab_saturates / {c['id']}: pattern differs on {differ:.3f} of the nonfinite elements")
            # (behind RELU the right pattern is finite wherever the sum is -inf or NaN: only the +inf elements tell)
            assert differ > (0.0 if c["act"] == KR.ACT_RELU else 0.5), (c["id"], differ)
            n += 1
    assert n == 6


def test_residual_added_before_staging_changes_every_staged_pattern():
    """act(...) + R rounded once (what the register-staged kernel and the reductions do) on a launch the header says stages
    act(...) as f16 first: finite where inf is due"""
    n = 0
    for c in RANGE:
        if KR.gemm_operand_kind(c)[0] == "staged" and c["splits"] == 1 and KR.gemm_case_is_wide(c):
            hot = _classes(c["id"]) == 1
            wrong = _model(c["id"], "residual_added_before_staging")[hot]
            assert bool(torch.isinf(_model(c["id"])[hot]).all()) and bool(torch.isfinite(wrong).all()), c["id"]
            n += 1
    assert n == 4


TRUNC = {"lin160-v41-split2-300x320x320-plain-kact": True, "lin160-v41-split2-300x320x320-plain": True,
         "lin160-v41-split2-300x320x320-plain-kcancel2": False}


@pytest.mark.parametrize("cid", sorted(TRUNC))
def test_slab_round_toward_zero(cid):
    """slabs rounded toward zero instead of to nearest: outside the bound on trained magnitudes and on unit operands; NOT on the
    symmetric cancel2 recipe, where the truncation errors of the two slabs have opposite signs and cancel like the slabs do
    (recorded, and asserted to be so: if this changes, the recipe did)"""
    p = KR.gemm_problem(cid)
    c = p["case"]
    ref, a = KR.gemm_ref(p)["out"], KR.gemm_allowance(p, c["splits"], True)["out"]
    right, _ = KR.bound_ratio(_model(cid), ref, a)
    wrong, _ = KR.bound_ratio(_model(cid, "slab_round_toward_zero"), ref, a)
    print(f"[gemm-range] slab_round_toward_zero / {cid}: err / bound {wrong:.3f} (rounded to nearest: {right:.3f})")
    assert right <= 1.0 and (wrong > 1.0) == TRUNC[cid], (cid, right, wrong)


# ------------------------------------------------------------------------------------------------
# against the fp16 pipeline of the reference model
# ------------------------------------------------------------------------------------------------
def test_documented_arithmetic_against_the_half_pipeline():
    """recorded: the quantiles over the elements of |documented arithmetic - ref| / |half_pipeline - ref| per operand kind, split
    launches and unsplit ones apart (profiles/gemm_kernel_tests.md).  Asserted: wherever half_pipeline is finite the documented
    arithmetic is finite, except on the elements the two header sentences name (class nonfinite, or band), and there it is not
    finite (or 0 behind RELU)."""
    rows, seen = {}, set()
    for c in KINDED + RANGE:
        p = KR.gemm_problem(c["id"])
        wide = KR.gemm_case_is_wide(c)
        arith = (KR.gemm_problem_key(c["id"]), c["splits"], wide)           # (the variants of one problem share the arithmetic)
        if arith in seen:
            continue
        seen.add(arith)
        hp, got, ref = KR.half_pipeline(p)["out"], _model(c["id"]), KR.gemm_ref(p)["out"]
        cls = KR.gemm_range_classes(p, c["splits"], wide) if c in RANGE else torch.zeros(ref.shape, dtype=torch.int64)
        if c["act"] == KR.ACT_GEGLU:
            cls = cls[:, :ref.shape[1]]
        assert bool(torch.isfinite(hp).all()) or c in RANGE, c["id"]
        lost = torch.isfinite(hp) & ~torch.isfinite(got)
        assert not bool((lost & (cls == 0)).any()), c["id"]
        ok = torch.isfinite(hp) & torch.isfinite(got) & (cls == 0)
        e_k, e_h = (got.double() - ref).abs()[ok], (hp.double() - ref).abs()[ok]
        key = (KR.gemm_operand_kind(c)[0], "split" if c["splits"] > 1 else "unsplit")
        rows.setdefault(key, []).append((e_k, e_h, int(lost.sum()), lost.numel()))
    for key, v in sorted(rows.items()):
        e_k, e_h = torch.cat([r[0] for r in v]), torch.cat([r[1] for r in v])
        both = (e_k > 0) | (e_h > 0)
        if not bool(both.any()):
            print(f"[gemm-range] {key[0]} {key[1]} ({len(v)} problems): both exact on every element")
            continue
        ratio = (e_k[both] / e_h[both].clamp_min(1e-300)).clamp_max(1e6)
        q = torch.quantile(ratio, torch.tensor([0.5, 0.9, 0.99], dtype=torch.float64)).tolist()
        print(f"[gemm-range] {key[0]} {key[1]} ({len(v)} problems): |model - ref| / |half_pipeline - ref| median {q[0]:.3g}, 90 % {q[1]:.3g}, 99 % {q[2]:.3g}; "
              f"sum of errors model / half_pipeline {float(e_k.sum() / e_h.sum()):.3f}; both exact on {1 - float(both.float().mean()):.3f}; "
              f"half_pipeline finite and model not on {sum(r[2] for r in v)} of {sum(r[3] for r in v)} elements")


# ------------------------------------------------------------------------------------------------
# the library's own split-K paths on the host
# ------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(CXX), reason="clang++ of the ROCm toolchain not available")
def test_the_contract_on_the_emulated_kernels(tmp_path):
    """tools/cpu_emu/emu_gemm, its three `slab contract` cases: exact cancelling partials through splitk_reduce_kernel and
    through the statistics-emitting reduction are bit-equal to the double-precision sum; one partial beyond the range gives
    the IEEE pattern"""
    subprocess.run([sys.executable, os.path.join(REPO, "tools", "cpu_emu", "build.py"), str(tmp_path)], check=True, stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(str(tmp_path), "emu_gemm"), "slab contract"], capture_output=True, text=True, timeout=900)
    lines = [l for l in r.stdout.splitlines() if l.startswith(("ok", "FAIL"))]
    assert r.returncode == 0 and len(lines) == 3 and all(l.startswith("ok") for l in lines), r.stdout[-3000:] + r.stderr[-1000:]
    assert sum("bit-equal" in l for l in lines) == 2 and sum("pattern" in l for l in lines) == 1, "\n".join(lines)
