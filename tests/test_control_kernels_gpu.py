"""GPU (-m gpu): pfd_add_scaled_rows_f16 (csrc/control.hip) through ops.add_scaled_rows on the shape grid of the emulation test
(tests/control_refs.py: B 1 and 3; 8, 328 and 40960 elements per sample; scale strides 1 and 13; out of place, in place on x and
on r) plus B 8 at 64 x 64 x 320 once: within the bound of control_refs against fp64, bit-equal to ops.add at scale 1, x's bits
at scale 0 (NaN in r), a strided table column as the scale, and bad arguments as error codes."""
import numpy as np
import pytest
import torch

import control_refs as R
from lib.hip import binding, ops

pytestmark = pytest.mark.gpu

T = torch.from_numpy


def _run(x, r, s, stride, alias):
    xd, rd = T(x).cuda(), T(r).cuda()
    tab = T(R.strided_scale(s, stride)).cuda()
    col = tab[:, 0]
    assert col.shape[0] == 1 or col.stride(0) == stride
    out = (None, xd, rd)[alias]
    y = ops.add_scaled_rows(xd, rd, col, out=out)
    if alias:
        assert y is out
    else:      # out of place: the operands are untouched
        assert np.array_equal(xd.cpu().numpy().view(np.uint16), x.view(np.uint16))
        assert np.array_equal(rd.cpu().numpy().view(np.uint16), r.view(np.uint16))
    return y.cpu().numpy()


@pytest.mark.parametrize("c", R.kernel_cases(), ids=[R.case_id(c) for c in R.kernel_cases()])
def test_kernel_against_fp64(c):
    x, r, s = R.operands(c['B'], c['n'], c['kind'], c['seed'])
    y = _run(x, r, s, c['stride'], c['alias'])
    e = R.judge(y, x, r, s)
    print(f"[control] {R.case_id(c)}: error / bound {e:.3f}")
    assert e <= 1.0
    if c['kind'] == 'ones':
        add = ops.add(T(x).cuda(), T(r).cuda()).cpu().numpy()
        assert np.array_equal(y.view(np.uint16), add.view(np.uint16))
    if c['kind'] == 'zeros':
        assert np.array_equal(y.view(np.uint16), x.view(np.uint16))


def test_kernel_at_the_size_of_the_first_unet_level():
    """B 8, 64 x 64 x 320: more blocks than the grid holds per sample (the grid-stride loop), every sample its own scale, one of
    them 0 and one 1; the result against fp64, the scale-1 sample against ops.add, in place on r as the UNet calls it"""
    B, n = R.BIG
    x, r, s = R.operands(B, n, 'act', 77)
    s[2], s[5] = 0.0, 1.0
    r[2, ::7] = np.nan
    xd, rd = T(x).cuda().reshape(B, 64, 64, 320), T(r).cuda().reshape(B, 64, 64, 320)
    tab = T(R.strided_scale(s, 13)).cuda()
    add5 = ops.add(xd[5:6].contiguous(), rd[5:6].contiguous()).cpu().numpy().reshape(-1)
    y = ops.add_scaled_rows(xd, rd, tab[:, 0], out=rd)
    assert y is rd and tuple(y.shape) == (B, 64, 64, 320)
    y = y.cpu().numpy().reshape(B, n)
    e = R.judge(y, x, r, s)
    print(f"[control] B 8 x 64 x 64 x 320 in place on r: error / bound {e:.3f}")
    assert e <= 1.0
    assert np.array_equal(y[5].view(np.uint16), add5.view(np.uint16))
    assert np.array_equal(xd.cpu().numpy().reshape(B, n).view(np.uint16), x.view(np.uint16))


def test_bad_arguments_come_back_as_error_codes():
    lib = binding.load()
    x = torch.zeros(2, 24, dtype=torch.float16, device='cuda')
    s = torch.ones(2, device='cuda')
    st = torch.cuda.current_stream().cuda_stream
    call = lambda xp, rp, sp, stride, yp, B, n: lib.pfd_add_scaled_rows_f16(xp, rp, sp, stride, yp, B, n, st)      # noqa: E731
    p, q = x.data_ptr(), s.data_ptr()
    assert call(p, p, q, 1, p, 2, 24) == 0
    assert call(p, p, q, 1, p, 2, 12) == binding.PFD_ESHAPE                  # n % 8 != 0
    assert call(p + 2, p, q, 1, p, 1, 8) == binding.PFD_ESHAPE               # a pointer off its 16 bytes
    assert call(p, p + 8, q, 1, p, 1, 8) == binding.PFD_ESHAPE
    assert call(p, p, q, 1, p + 4, 1, 8) == binding.PFD_ESHAPE
    for bad in ((None, p, q, 1, p, 2, 24), (p, None, q, 1, p, 2, 24), (p, p, None, 1, p, 2, 24), (p, p, q, 1, None, 2, 24),
                (p, p, q, 1, p, 0, 24), (p, p, q, 0, p, 2, 24), (p, p, q, 1, p, 2, 0)):
        assert call(*bad) == binding.PFD_EINVAL, bad
    torch.cuda.synchronize()
    assert float(x.float().abs().max()) == 0.0
    # the wrapper: dtype, density, sizes, the scale
    h = torch.zeros(2, 4, 8, dtype=torch.float16, device='cuda')
    for xa, ra, sa in ((h.float(), h, s), (h, h[:, :2], s), (h[:, ::2], h[:, ::2], s), (h, h, s.double()), (h, h, s.cpu()),
                       (h, h, torch.ones(3, device='cuda')), (h, h, 1.0)):
        with pytest.raises((ValueError, TypeError, RuntimeError)):
            ops.add_scaled_rows(xa, ra, sa)
    with pytest.raises(binding.PfdError, match="PFD_ESHAPE"):
        ops.add_scaled_rows(h[:, :, :4].contiguous().reshape(2, 16)[:, :12].contiguous(), torch.zeros(2, 12, dtype=torch.float16, device='cuda'), s)
