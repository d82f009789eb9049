"""GPU (-m gpu): the upsample convolution as four 2x2-tap phase convolutions over the low-res image (PfdGemmDesc.ups = 2,
gemm160ws_kernel's phase form) against fp64 `conv2d(interpolate(x, 2, 'nearest'), w) + bias`, next to the 9-tap gather
(ups = 1) on the same inputs."""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SHAPES = [(2, 16, 16, 64, 160), (3, 16, 16, 64, 160), (1, 8, 32, 128, 320), (1, 16, 16, 64, 128)]


def scaled_err(a, ref):
    """the `close` metric of tests/test_hip_kernels.py"""
    return float((a.double().cpu() - ref).abs().max() / max(1.0, float(ref.abs().max())))


@functools.lru_cache(maxsize=None)
def problem(B, H, W, Cin, N):
    """seeded operands and the fp64 reference, computed once per shape"""
    from lib.hip import layers as L
    g = torch.Generator().manual_seed(B * 1000 + H * 100 + W + Cin + N)
    x = torch.randn((B, H, W, Cin), generator=g).half()
    w4 = (torch.randn((N, Cin, 3, 3), generator=g) * (9 * Cin) ** -0.5).half()
    b = (torch.randn((N,), generator=g) * 0.5).half()
    xr = F.interpolate(x.double().permute(0, 3, 1, 2), scale_factor=2, mode="nearest")
    ref = (F.conv2d(xr, w4.double(), padding=1) + b.double()[None, :, None, None]).permute(0, 2, 3, 1).contiguous()
    w4c = w4.cuda()
    return dict(x=x.cuda(), b=b.cuda(), w9=L.pack_conv_weight(w4c), wf=L.pack_conv_weight_ups(w4c), ref=ref, w4=w4c)


@pytest.mark.parametrize("shape", SHAPES)
def test_phase_form_error_and_determinism(shape):
    from lib.hip import ops
    p = problem(*shape)
    y2 = ops.conv(p["x"], p["wf"], 3, ups=2, bias=p["b"])
    assert y2 is not None, "the library declined a shape it documents as served"
    y1 = ops.conv(p["x"], p["w9"], 3, ups=True, bias=p["b"])
    e2, e1 = scaled_err(y2, p["ref"]), scaled_err(y1, p["ref"])
    print(f"[ups-fold] {shape}: scaled max-abs ups=2 {e2:.3e}, ups=1 {e1:.3e}")
    assert e2 <= 4e-3, e2
    assert e2 <= e1 + 5e-4, (e2, e1)
    assert torch.equal(ops.conv(p["x"], p["wf"], 3, ups=2, bias=p["b"]), y2)     # two launches: the same bits
    for variant in (47, 48):                                                  # both forms of the loader-wave kernel
        yv = ops.conv(p["x"], p["wf"], 3, ups=2, bias=p["b"], tile=1000 + 100 * variant)
        assert scaled_err(yv, p["ref"]) <= 4e-3


def test_phase_form_statistics():
    """gn_out: the per-(sample, group) sums the launch emits are the sums of the f16 values it stored, and GroupNorm from them
    is GroupNorm of the stored tensor"""
    from lib.hip import ops
    B, H, W, Cin, N = shape = (1, 8, 32, 128, 320)
    p = problem(*shape)
    y = ops.conv(p["x"], p["wf"], 3, ups=2, bias=p["b"], gn_out=True)
    st = ops.get_gn_stats(y)
    assert y is not None and st is not None, "no statistics on a shape whose GroupNorm takes them"
    HW, cpg, tn = 4 * H * W, N // 32, N // 160
    assert tuple(st.shape) == (B * HW // 64, tn, 16, 2)
    got = st.view(B, HW // 64, tn, 16, 2).sum(1)[:, :, :160 // cpg].reshape(B, 32, 2).double().cpu()
    v = y.float().view(B, HW, 32, cpg)
    s32, q32 = v.sum((1, 3)).double().cpu(), (v * v).sum((1, 3)).double().cpu()
    # relative to the mass that was summed: sum |x| for the sums (a sum may cancel to ~0), the sum itself for the squares
    e_s = float(((got[..., 0] - s32).abs() / v.abs().sum((1, 3)).double().cpu()).max())
    e_q = float(((got[..., 1] - q32).abs() / q32).max())
    print(f"[ups-fold] statistics {shape}: sums {e_s:.2e}, sums of squares {e_q:.2e} (relative)")
    assert e_s <= 1e-5 and e_q <= 1e-5, (e_s, e_q)
    g = torch.Generator().manual_seed(9)
    gamma, beta = (1 + 0.3 * torch.randn(N, generator=g)).half().cuda(), (0.3 * torch.randn(N, generator=g)).half().cuda()
    yn = ops.groupnorm(y, gamma, beta, 32, 1e-5, silu=True)
    ref = F.silu(F.group_norm(y.float().permute(0, 3, 1, 2), 32, gamma.float(), beta.float(), 1e-5)).permute(0, 2, 3, 1)
    e = scaled_err(yn, ref.double().cpu())
    print(f"[ups-fold] GroupNorm from the phase form's statistics: {e:.2e}")
    assert e <= 5e-3, e


def _layer(Cin, N, seed):
    from lib.hip import layers as L
    torch.manual_seed(seed)
    return L.Conv2d(Cin, N, 3, padding=1).half().cuda()


def test_layer_takes_the_fold_and_falls_back():
    from lib.hip import ops
    m = _layer(64, 160, 3)
    g = torch.Generator().manual_seed(4)
    # served shape: the layer's result is the direct ups = 2 call's
    x = torch.randn((2, 16, 16, 64), generator=g).half().cuda()
    wf, b = m._pk_ups()
    assert torch.equal(m.hip(x, ups=True), ops.conv(x, wf, 3, ups=2, bias=b))
    # 5x6: H * W % 256 != 0 -> declined, the 9-tap call bit for bit, and the decline is remembered
    x = torch.randn((2, 5, 6, 64), generator=g).half().cuda()
    w9, b = m._pk()
    assert torch.equal(m.hip(x, ups=True), ops.conv(x, w9, 3, ups=True, bias=b))
    assert ops.ups_fold_declined(ops.ups_fold_key(x, 160, ops.ACT_NONE, b, None, False))
    assert torch.equal(m.hip(x, ups=True), ops.conv(x, w9, 3, ups=True, bias=b))


def test_declined_request_returns_eshape_and_writes_nothing():
    from lib.hip import binding as _b, ops
    lib = _b.load()
    B, H, W, Cin, N = 1, 8, 8, 64, 160                       # H * W = 64: a 256-row tile would straddle the phases
    g = torch.Generator().manual_seed(6)
    x = torch.randn((B, H, W, Cin), generator=g).half().cuda()
    wf = torch.randn((4, N, 4 * Cin), generator=g).half().cuda()
    out = torch.full((B, 2 * H, 2 * W, N), -7.0, dtype=torch.float16, device="cuda")
    d = _b.PfdGemmDesc()
    d.A, d.W, d.C = x.data_ptr(), wf.data_ptr(), out.data_ptr()
    d.lda, d.ldw, d.ldc = Cin, 4 * Cin, N
    d.M, d.N, d.K = B * 4 * H * W, N, 4 * Cin
    d.rows_per_rv, d.act = 4 * H * W, ops.ACT_NONE
    d.ksize, d.stride, d.pad, d.ups = 3, 1, 1, 2
    d.B, d.H, d.Wd, d.Cin, d.Ho, d.Wo = B, H, W, Cin, 2 * H, 2 * W
    rc = lib.pfd_gemm_f16(ctypes.byref(d), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert rc == _b.PFD_ESHAPE, rc
    assert bool((out == -7.0).all()), "a declined request wrote to its output"
    assert ops.conv(x, wf, 3, ups=2, out=out) is None and bool((out == -7.0).all())
    # a residual is not served by the phase form either (a shape that is served without one)
    x = torch.randn((1, 16, 16, Cin), generator=g).half().cuda()
    out = torch.full((1, 32, 32, N), -7.0, dtype=torch.float16, device="cuda")
    assert ops.conv(x, wf, 3, ups=2, res=torch.zeros_like(out), out=out) is None and bool((out == -7.0).all())


def test_weight_hot_swap_refolds_the_pack():
    from lib.hip import layers as L
    m = _layer(64, 160, 7)
    x = torch.randn((1, 16, 16, 64), generator=torch.Generator().manual_seed(8)).half().cuda()
    wf1 = m._pk_ups()[0].clone()
    y1 = m.hip(x, ups=True).clone()
    assert m._pk_ups()[0].data_ptr() == m._pk_ups()[0].data_ptr()      # cached between calls
    with torch.no_grad():
        m.weight.mul_(-0.5)
    wf2 = m._pk_ups()[0]
    assert not torch.equal(wf1, wf2) and torch.equal(wf2, L.pack_conv_weight_ups(m.weight))
    assert not torch.equal(m.hip(x, ups=True), y1)
