"""GPU (-m gpu): the kernels behind pfd_gemm_f16 where a quantity that include/pfd_hip.h says passes through f16 leaves the f16
range (kernel_refs.GEMM_RANGE_CASES; tests/test_gemm_range_cpu.py qualifies the cases).  Two sentences of the header are held:

  PfdGemmDesc.ws   "the K-range partial sums are stored rounded to f16 and summed in fp32, in slab order ... a partial sum
                   beyond +-65504 becomes +-inf exactly as an f16 result of that magnitude would, and the sum goes on in IEEE
                   arithmetic ... with a slab count that is no multiple of four an element whose last slab is +-inf is NaN"
                   (the second half is what this test found: on 119 elements of the first case the reduction gave NaN where
                   IEEE on the slabs gives -inf; profiles/gemm_kernel_tests.md, "Operand kinds", finding 1)
  epi(v)           the unsplit wide-tile kernels stage act(...) as f16 in front of the residual: it overflows like an f16 result
                   before R is added; the register-staged kernel and the split-K reductions add R in fp32

What this means for a caller: the SAME operands give NaN / inf on some elements of a split launch and an ordinary finite
result on the unsplit one (and the other way round for the staged value) -- and whether a problem is split is the library's
choice.  Every case here runs beside its counterpart on the same operands.

Per element the expected class comes from the fp64 reference alone (kernel_refs.gemm_range_classes): `finite` elements are
finite and inside kernel_refs.gemm_allowance like everywhere else; `nonfinite` elements show exactly the NaN / +inf / -inf pattern
of the IEEE evaluation of the header's words (kernel_refs.gemm_kernel_model: torch, fp32, CPU) and, where that evaluation is
finite (0 behind RELU), that value; `band` elements (a quantity within its accumulation allowance of 65520) are left out."""
import pytest
import torch

import kernel_refs as KR
from test_gemm_kernels_gpu import SENTINEL, _device_operands, _launch, _outputs

pytestmark = pytest.mark.gpu

rids = [c["id"] for c in KR.GEMM_RANGE_CASES]


def _bits(t):
    return t.contiguous().view(torch.int16)


def _pattern(t):
    """0 finite, 1 NaN, 2 +inf, 3 -inf"""
    return torch.isnan(t) * 1 + torch.isposinf(t) * 2 + torch.isneginf(t) * 3


def _run(cid):
    """the guards of the main table's runner without its finiteness assertion: nothing outside the slice is written, every element
    is, three launches give the same bits, the pad values change nothing"""
    p = KR.gemm_problem(cid)
    c = p["case"]
    M = c["M"]
    d = _device_operands(p)
    buf, out, _, n_out = _outputs(c)
    r = _launch(p, d, out)
    torch.cuda.synchronize()
    assert r["out"].data_ptr() == out.data_ptr()
    assert bool((buf[M:] == SENTINEL).all()), "rows behind the last row were written"
    assert bool((buf[:M, :8] == SENTINEL).all()) and bool((buf[:M, 8 + n_out:] == SENTINEL).all()), "columns outside the slice were written"
    got = buf[:M, 8:8 + n_out].contiguous()
    assert not bool((got == SENTINEL).any()), "an element was not written"
    for _ in range(2):
        assert torch.equal(_bits(_launch(p, d)["out"].reshape(got.shape)), _bits(got)), "two launches, different bits"
    assert torch.equal(_bits(_launch(p, _device_operands(p, poison=False))["out"].reshape(got.shape)), _bits(got)), "the pad values changed the result"
    return p, got.cpu()


@pytest.mark.parametrize("cid", rids)
def test_gemm_beyond_the_f16_range(cid):
    p, got = _run(cid)
    c = p["case"]
    wide = KR.gemm_case_is_wide(c)
    ref = KR.gemm_ref(p)["out"]
    cls = KR.gemm_range_classes(p, c["splits"], wide)
    exp = KR.gemm_kernel_model(p, c["splits"], wide)["out"]
    hp = KR.half_pipeline(p)["out"]
    fin, hot = cls == 0, cls == 1
    gp, ep = _pattern(got), _pattern(exp)
    lost = torch.isfinite(hp) & ~torch.isfinite(got)
    counts = lambda t: "/".join(str(int((t[hot] == k).sum())) for k in range(4))
    nonfin = int((gp[fin] != 0).sum())
    g0 = torch.where(fin & (gp == 0), got, torch.zeros_like(got))             # (bound_ratio wants finite input)
    r0 = torch.where(fin & (gp == 0), ref, torch.zeros_like(ref))
    ratio, used = KR.bound_ratio(g0, r0, KR.gemm_allowance(p, c["splits"], wide)["out"])
    print(f"[gemm-range] {c['cls']} {cid} ({c['kernel']}{' + ' + c['reduce'] if c['reduce'] else ''}): {int(fin.sum())} finite-class elements, "
          f"{nonfin} of them not finite, err / bound {ratio:.3f}, allowance used {used:.3f}; {int(hot.sum())} nonfinite-class elements, "
          f"finite/NaN/+inf/-inf got {counts(gp)} expected {counts(ep)}; {int((cls == 2).sum())} band elements left out; "
          f"half_pipeline finite and the kernel not: {int(lost.sum())} elements, {int((lost & fin).sum())} outside the two header sentences")
    assert nonfin == 0, "an element whose slabs / staged value are inside the range is not finite"
    assert ratio <= 1.0, (cid, ratio)
    assert torch.equal(gp[hot], ep[hot]), "not the IEEE pattern of the header's arithmetic"
    both = hot & (ep == 0)
    assert torch.equal(got[both], exp[both]), "the finite values among the nonfinite-class elements"
    assert not bool((lost & fin).any())
