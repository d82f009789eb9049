"""GPU (-m gpu): the boundary kernels of csrc/elementwise.hip on every fp16 input, past the grid cap and in place, against the
oracles and bounds of tests/boundary_refs.py (qualified on the CPU by tests/test_boundary_kernels_cpu.py): pfd_image_u8_f16 bit
for bit on all 63 490 non-NaN inputs, at every size class and through its refusals; pfd_act_f16 on all 63 488 finite inputs
inside per-element bounds derived from the number formats and the source's own claim; the layout kernels and the row-vector
add with their grid-stride loop wrapped; every aliasing include/pfd_hip.h allows.  The measured figures are in
profiles/boundary_kernel_tests.md."""
import pytest
import torch
import torch.nn.functional as F

import boundary_refs as BR
import kernel_refs as KR

pytestmark = pytest.mark.gpu

GUARD = 0xA5                # the byte behind / in place of an output that must not be written
SENTINEL = 1234.0           # exact in fp16, far outside every result below


def _lib():
    from lib.hip import binding
    return binding.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _same_bits(a, b):
    a, b = a.cpu().contiguous(), b.cpu().contiguous()
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, tuple(a.shape), tuple(b.shape))
    view = {torch.float16: torch.int16, torch.float32: torch.int32, torch.uint8: torch.uint8}[a.dtype]
    return int((a.view(view) != b.view(view)).sum())


def _check(name, shape, got, ref64, ref32):
    """got within kernel_refs.round_once_bound of the fp64 reference element by element; the fp32 allowance comes from the same
    torch formula in fp32 on the CPU against fp64, never from the kernel (as test_encoder_kernels_gpu.py does it)"""
    a = KR.fp32_allowance(ref64, ref32)
    r, used = KR.bound_ratio(got, ref64, a)
    print(f"[boundary gpu] {name} {shape}: worst error / bound {r:.3f} (fp32 allowance {a:.2e}, {100 * used:.0f} % of it used)")
    assert r <= 1.0, (name, shape, r)


# ------------------------------------------------------------------------------------------------
# 1. pfd_image_u8_f16
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f16_image", [True, False], ids=["f16", "f32"])
@pytest.mark.parametrize("mul,add", BR.IMAGE_MUL_ADD)
def test_image_u8_on_every_input(mul, add, f16_image):
    """all 63 490 non-NaN fp16 inputs as a (1, 7, 907, 10) picture, ragged against the 64 x 64 transpose tile in both
    directions: the bytes of the CPU oracle bit for bit; at (0.5, 0.5) also the bytes of the device's own float picture
    `to_nchw(...).mul(255).byte()` (what pipeline.generate(as_uint8=True) promises), whose float values are themselves the
    fp32 formula's bit for bit"""
    from lib.hip import ops
    x = BR.all_f16("non_nan").view(1, 7, 907, 10)
    xd = x.cuda()
    got = ops.image_u8(xd, mul, add, f16_image)
    assert got.dtype == torch.uint8 and tuple(got.shape) == tuple(x.shape)
    ref = BR.image_u8_ref(x, mul, add, f16_image)
    diff = got.cpu() != ref
    print(f"[boundary gpu] image_u8 ({mul}, {add}) {'f16' if f16_image else 'f32'} image: {int(diff.sum())} of {x.numel()} bytes differ")
    assert int(diff.sum()) == 0, (x[diff][:8].tolist(), got.cpu()[diff][:8].tolist(), ref[diff][:8].tolist())
    assert torch.equal(ops.image_u8(xd, mul, add, f16_image), got), "two launches, different bytes"
    if (mul, add) == (0.5, 0.5):
        dtype = torch.float16 if f16_image else torch.float32
        pic = ops.to_nchw(xd, dtype, 0.5, 0.5, 0.0, 1.0)
        assert pic.dtype == dtype and tuple(pic.shape) == (1, 10, 7, 907)
        want = (x.float() * 0.5 + 0.5).clamp(0, 1).to(dtype).permute(0, 3, 1, 2).contiguous()
        assert _same_bits(pic, want) == 0, "to_nchw's float picture"
        assert torch.equal(pic.mul(255).byte().permute(0, 2, 3, 1), got), "the bytes are not those of the device's float picture"


@pytest.mark.parametrize("f16_image", [True, False], ids=["f16", "f32"])
@pytest.mark.parametrize("n", BR.IMAGE_U8_SIZES)
def test_image_u8_sizes(n, f16_image):
    """scalar tail only, no tail, a tail behind vectors, and the grid-stride loop past the 4096-block cap (+ a tail): the
    library called directly on a prefix of a guard-filled byte buffer -- the oracle's bytes, nothing behind n written"""
    x = BR.image_u8_operand(n)
    ref = BR.image_u8_ref(x, 0.5, 0.5, f16_image)
    xd = x.cuda()
    bufs = []
    for _ in range(2):
        buf = torch.full((n + 64,), GUARD, dtype=torch.uint8, device="cuda")
        rc = _lib().pfd_image_u8_f16(xd.data_ptr(), buf.data_ptr(), n, 0.5, 0.5, int(f16_image), _stream())
        assert rc == 0
        bufs.append(buf)
    got = bufs[0].cpu()
    assert bool((got[n:] == GUARD).all()), "bytes behind n were written"
    diff = got[:n] != ref
    assert int(diff.sum()) == 0, (n, int(diff.sum()), int(((got[:n] == GUARD) & diff).sum()), "of them left unwritten")
    assert torch.equal(bufs[0], bufs[1]), "two launches, different bytes"


def test_image_u8_of_nan_inputs_returns_and_is_deterministic():
    """NaN inputs are outside the bit-for-bit promise (`.byte()` of a NaN is undefined in the reference): the launch on the
    2046 NaN patterns completes and two launches agree"""
    from lib.hip import ops
    x = BR.all_f16("nan").view(1, 1, 682, 3).cuda()
    for f16_image in (True, False):
        a, b = ops.image_u8(x, 0.5, 0.5, f16_image), ops.image_u8(x, 0.5, 0.5, f16_image)
        torch.cuda.synchronize()
        assert torch.equal(a, b)
        print(f"[boundary gpu] image_u8 of the 2046 NaN patterns ({'f16' if f16_image else 'f32'} image): bytes {sorted(set(a.cpu().reshape(-1).tolist()))}")


def test_bad_arguments_are_refused_with_nothing_written():
    """a pointer 2 or 8 bytes off its alignment, n <= 0, NULL (and an activation outside the four, C % 8, C % 160): the return
    code of include/pfd_hip.h, the output untouched"""
    lib, s, E = _lib(), _stream(), BR.PFD_EINVAL
    n = 800
    xs = torch.zeros(n + 16, dtype=torch.float16, device="cuda")
    x, x2, x8 = xs[:n], xs[1:n + 1], xs[4:n + 4]
    v = torch.zeros(160, dtype=torch.float16, device="cuda")
    yb = torch.full((2 * n + 64,), GUARD, dtype=torch.uint8, device="cuda")
    st = torch.full((5 * 2,), float("nan"), dtype=torch.float32, device="cuda")
    p, y = x.data_ptr(), yb.data_ptr()
    assert p % 16 == 0 and y % 16 == 0 and x2.data_ptr() % 16 == 2 and x8.data_ptr() % 16 == 8
    calls = []
    for xp, yp, nn in ((x2.data_ptr(), y, n), (x8.data_ptr(), y, n), (p, y + 2, n), (p, y + 4, n), (p, y, 0), (p, y, -1), (0, y, n), (p, 0, n)):
        calls.append(("image_u8", lib.pfd_image_u8_f16(xp, yp, nn, 0.5, 0.5, 1, s), E))
    for xp, yp, nn, act in ((x2.data_ptr(), y, n, 3), (x8.data_ptr(), y, n, 3), (p, y + 2, n, 3), (p, y + 8, n, 3), (p, y, 0, 3),
                            (0, y, n, 3), (p, 0, n, 3), (p, y, n, 4), (p, y, n, -1)):
        calls.append(("act", lib.pfd_act_f16(xp, yp, nn, act, s), E))
    for ap, bp, yp, nn in ((x2.data_ptr(), p, y, n), (p, x8.data_ptr(), y, n), (p, p, y + 2, n), (p, p, y + 8, n), (p, p, y, 0),
                           (0, p, y, n), (p, p, 0, n)):
        calls.append(("add", lib.pfd_add_f16(ap, bp, yp, nn, s), E))
        calls.append(("axpby", lib.pfd_axpby_f16(ap, 0.75, bp, -1.25, yp, nn, s), E))
    vp = v.data_ptr()
    for xp, vv, yp, R, C in ((x2.data_ptr(), vp, y, 5, 160), (x8.data_ptr(), vp, y, 5, 160), (p, vp + 2, y, 5, 160), (p, vp, y + 2, 5, 160),
                             (p, vp, y + 8, 5, 160), (p, vp, y, 0, 160), (0, vp, y, 5, 160), (p, 0, y, 5, 160), (p, vp, 0, 5, 160)):
        calls.append(("add_rowvec", lib.pfd_add_rowvec_f16(xp, C, vv, yp, C, R, C, s), E))
        calls.append(("add_rowvec_lnstats", lib.pfd_add_rowvec_lnstats_f16(xp, C, vv, yp, C, R, C, st.data_ptr(), s), E))
    calls.append(("add_rowvec C % 8", lib.pfd_add_rowvec_f16(p, 12, vp, y, 12, 5, 12, s), E))
    calls.append(("add_rowvec_lnstats C % 160", lib.pfd_add_rowvec_lnstats_f16(p, 168, vp, y, 168, 4, 168, st.data_ptr(), s), BR.PFD_ESHAPE))
    calls.append(("add_rowvec_lnstats stats NULL", lib.pfd_add_rowvec_lnstats_f16(p, 160, vp, y, 160, 5, 160, 0, s), E))
    torch.cuda.synchronize()
    wrong = [(name, rc, want) for name, rc, want in calls if rc != want]
    assert not wrong, wrong
    assert bool((yb == GUARD).all()) and bool(torch.isnan(st).all()), "a refused call wrote"


def test_wrappers_refuse_bad_operands_on_the_device():
    """what tests/test_boundary_kernels_cpu.py checks on stand-in tensors, on real device tensors: a float32 or CPU or strided
    or short `out`, `b` of axpby, `v` of add_rowvec -- refused, and the operands keep their contents"""
    from lib.hip import ops
    a = torch.ones((4, 16), dtype=torch.float16, device="cuda")
    v = torch.ones(16, dtype=torch.float16, device="cuda")
    wide = torch.full((4, 32), SENTINEL, dtype=torch.float16, device="cuda")
    f32 = torch.full((4, 16), SENTINEL, dtype=torch.float32, device="cuda")
    for fn in (lambda out: ops.add(a, a, out=out), lambda out: ops.axpby(a, 1.0, a, 1.0, out=out), lambda out: ops.activation(a, 3, out=out),
               lambda out: ops.add_rowvec(a, v, out=out)):
        with pytest.raises(TypeError):
            fn(f32)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(torch.zeros((4, 16), dtype=torch.float16))
        with pytest.raises(ValueError):
            fn(wide[:, ::2])
        with pytest.raises(ValueError):
            fn(wide[:2, :16])
    window = wide[:, :16]                                        # unit inner stride, rows apart: only add_rowvec takes it
    for fn in (lambda: ops.add(a, a, out=window), lambda: ops.axpby(a, 1.0, out=window), lambda: ops.activation(a, 3, out=window)):
        with pytest.raises(ValueError):
            fn()
    for bad_b, exc in ((f32, TypeError), (torch.zeros((4, 16), dtype=torch.float16), RuntimeError), (wide[:, :16], ValueError),
                       (a[:2], ValueError)):
        with pytest.raises(exc):
            ops.axpby(a, 1.0, bad_b, 1.0)
    for bad_v, exc in ((v.float(), TypeError), (v.cpu(), RuntimeError), (v[:8], ValueError), (wide[0, ::2], ValueError), (a, ValueError)):
        with pytest.raises(exc):
            ops.add_rowvec(a, bad_v)
    torch.cuda.synchronize()
    assert bool((wide == SENTINEL).all()) and bool((f32 == SENTINEL).all()) and bool((a == 1).all())
    assert torch.equal(ops.add_rowvec(a, v, out=wide[:, 16:]), torch.full_like(a, 2.0)) and bool((wide[:, :16] == SENTINEL).all())


# ------------------------------------------------------------------------------------------------
# 2. pfd_act_f16
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", [0, 1, 2, 3], ids=BR.ACT_NAMES)
def test_activation_on_every_finite_input(act):
    """all 63 488 finite fp16 inputs in one launch, per element inside boundary_refs.act_bound: the input's bits (none), the
    input's bits or a zero (ReLU), half an fp16 ulp + 2^-20 |ref| (SiLU), half an fp16 ulp + 5e-7 (GELU, the claim of
    csrc/pfd_common.h)"""
    from lib.hip import ops
    x = BR.all_f16("finite")
    y = ops.activation(x.cuda(), act).cpu()
    bad, ratio = BR.act_violations(y, x, act)
    if ratio is not None:
        at = int(ratio.argmax())
        ref = KR.activation_ref(x, act)
        e = (y.double() - ref).abs() - BR.half_ulp_f16(ref)                    # what the fp32 evaluation needs beyond the rounding
        print(f"[boundary gpu] act {BR.ACT_NAMES[act]}: worst error / bound {float(ratio.max()):.4f} at x = {float(x[at]):.6g} "
              f"(got {float(y[at]):.6g}, fp64 {float(ref[at]):.9g}); most needed beyond half an ulp {float(e.max()):.3e} at "
              f"x = {float(x[int(e.argmax())]):.6g}")
    print(f"[boundary gpu] act {BR.ACT_NAMES[act]}: {int(bad.sum())} of {x.numel()} inputs outside the bound")
    assert int(bad.sum()) == 0, (x[bad][:8].tolist(), y[bad][:8].tolist())


def test_activation_of_the_infinities():
    """+-inf against torch's F.gelu / F.silu / relu on the CPU, NaN-or-equal: where torch gives a number the kernel gives that
    number; where torch gives NaN (inf * 0: gelu and silu of -inf -- and torch's own gelu of +inf, whose limit is +inf) the
    kernel gives NaN or the limit, never a finite value"""
    from lib.hip import ops
    x = torch.tensor([float("inf"), float("-inf")] * 4 + [1.0], dtype=torch.float16)         # 9 values: a vector and a tail
    for act, fn in ((0, lambda v: v), (1, F.gelu), (2, torch.relu), (3, F.silu)):
        y = ops.activation(x.cuda(), act).cpu()
        want = fn(x.float()).half()
        print(f"[boundary gpu] act {BR.ACT_NAMES[act]} of +inf, -inf: {y[0].item()}, {y[1].item()} (torch {want[0].item()}, {want[1].item()})")
        free = torch.isnan(want)
        assert torch.equal(y[~free], want[~free]) and not bool(torch.isfinite(y[free]).any()), (act, y, want)

# ------------------------------------------------------------------------------------------------
# 3. past the grid: more elements than grid_for's 4096 x 256 threads
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rep", [1, 2])
@pytest.mark.parametrize("src", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_to_nhwc_past_the_grid(src, rep):
    from lib.hip import ops
    shape = BR.TO_NHWC_PAST_GRID
    x = torch.randn(shape, generator=torch.Generator().manual_seed(592)).to(src)
    y = ops.to_nhwc(x.cuda(), mul=1.0, add=0.0, rep=rep)
    assert tuple(y.shape) == (rep, shape[2], shape[3], shape[1]) and y.dtype == torch.float16 and y.numel() == rep * 1051392
    if src == torch.float16:
        assert _same_bits(y, KR.to_nhwc_ref(x, 1.0, 0.0, rep).half()) == 0          # a copy
    else:
        _check("to_nhwc(f32)", (shape, rep), y, KR.to_nhwc_ref(x, 1.0, 0.0, rep), KR.to_nhwc_ref(x, 1.0, 0.0, rep, dtype=torch.float32))


def test_im2col_past_the_grid():
    from lib.hip import ops
    c = BR.IM2COL_PAST_GRID
    x = torch.randn(c["shape"], generator=torch.Generator().manual_seed(130)).half()
    col, Ho, Wo = ops.im2col(x.cuda(), c["ks"], c["stride"], c["pad"], c["kpad"])
    assert (Ho, Wo) == (130, 130) and tuple(col.shape) == (130 * 130, 64) and col.numel() == 1081600
    ref = KR.im2col_ref(x, c["ks"], c["stride"], c["pad"], c["kpad"])
    assert _same_bits(col, ref) == 0
    assert float(col[:, 27:].abs().max()) == 0.0


def test_add_rowvec_past_the_grid_and_in_place():
    from lib.hip import ops
    R, C = BR.ADD_ROWVEC_PAST_GRID
    g = torch.Generator().manual_seed(R + C)
    x, v = torch.randn((R, C), generator=g).half(), torch.randn((C,), generator=g).half()
    xd, vd = x.cuda(), v.cuda()
    y = ops.add_rowvec(xd, vd)
    _check("add_rowvec", (R, C), y, x.double() + v.double()[None], x.float() + v.float()[None])
    z = ops.add_rowvec(xd, vd, out=xd)
    assert z.data_ptr() == xd.data_ptr() and torch.equal(xd, y), "in place"


# ------------------------------------------------------------------------------------------------
# 4. in place: every aliasing include/pfd_hip.h allows gives the bits of the out-of-place launch
# ------------------------------------------------------------------------------------------------
def _vec(n, seed):
    return torch.randn(n, generator=torch.Generator().manual_seed(seed)).half().cuda()


@pytest.mark.parametrize("n", [9, 2048, 2049, 8 * 256 * 4096 + 13])
def test_flat_kernels_in_place(n):
    """without a tail, with one, and past the grid cap: add and axpby with y = a and y = b, the activations with y = x"""
    from lib.hip import ops
    a, b = _vec(n, n), _vec(n, n + 1)
    for name, fn in (("add", lambda p, q, out=None: ops.add(p, q, out=out)),
                     ("axpby", lambda p, q, out=None: ops.axpby(p, 0.75, q, -1.25, out=out))):
        want = fn(a, b)
        assert want.data_ptr() not in (a.data_ptr(), b.data_ptr())
        a2, b2 = a.clone(), b.clone()
        assert fn(a2, b2, out=a2).data_ptr() == a2.data_ptr() and torch.equal(a2, want), (name, "y = a")
        assert torch.equal(b2, b)
        a2 = a.clone()
        assert fn(a2, b2, out=b2).data_ptr() == b2.data_ptr() and torch.equal(b2, want), (name, "y = b")
        assert torch.equal(a2, a)
    want = ops.axpby(a, -0.3)
    a2 = a.clone()
    ops.axpby(a2, -0.3, out=a2)
    assert torch.equal(a2, want), "axpby without b, y = a"
    for act in (0, 1, 2, 3):
        want = ops.activation(a, act)
        a2 = a.clone()
        assert ops.activation(a2, act, out=a2).data_ptr() == a2.data_ptr() and torch.equal(a2, want), (act, "y = x")


@pytest.mark.parametrize("R,C", [(5, 160), (3, 320), (300, 320), (37, 1280)])
def test_add_rowvec_in_place(R, C):
    """y = x for the plain form and the statistics form (dense and as a column window of a wider matrix): the bits, and the
    row statistics, of the out-of-place launch"""
    from lib.hip import ops
    g = torch.Generator().manual_seed(R * C)
    x, v = (torch.randn((R, C), generator=g) + 0.3).half().cuda(), torch.randn((C,), generator=g).half().cuda()
    st = torch.full((R, C // 160, 2), float("nan"), dtype=torch.float32, device="cuda")
    want = ops.add_rowvec(x, v)
    assert torch.equal(ops.add_rowvec(x, v, ln_out=st), want)
    x2 = x.clone()
    assert ops.add_rowvec(x2, v, out=x2).data_ptr() == x2.data_ptr() and torch.equal(x2, want)
    x2, st2 = x.clone(), torch.full_like(st, float("nan"))
    ops.add_rowvec(x2, v, out=x2, ln_out=st2)
    assert torch.equal(x2, want) and torch.equal(st2, st)
    wide = torch.full((R, C + 24), SENTINEL, dtype=torch.float16, device="cuda")
    wide[:, 16:16 + C] = x
    win = wide[:, 16:16 + C]
    ops.add_rowvec(win, v, out=win)
    assert torch.equal(win, want) and bool((wide[:, :16] == SENTINEL).all()) and bool((wide[:, 16 + C:] == SENTINEL).all())
