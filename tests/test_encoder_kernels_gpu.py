"""GPU (-m gpu): the kernels of the SeeCoder side one launch at a time against the plain fp64 references of
tests/kernel_refs.py -- Swin window attention (pfd_swin_window_attention_f16), LayerNorm in all its forms
(pfd_layernorm_f16: one row per wave at every register count, four rows per wave, strided, the PatchMerging gather), the
row softmax at both of its forms, and the element-wise / layout entry points -- with per-element bounds derived from the
number formats (kernel_refs.SWIN_TOL, kernel_refs.round_once_bound), not the global-max metric of test_hip_kernels.py.
The measured ratios are in profiles/encoder_kernel_tests.md."""
import pytest
import torch

import kernel_refs as KR
import pfd_oracle as O

pytestmark = pytest.mark.gpu

SENTINEL = 1234.0           # exact in fp16, far outside every result below


def _id(s):
    return "x".join(map(str, s)) if isinstance(s, tuple) else str(s)


def _check(name, shape, got, ref64, ref32, ref=None):
    """got within round_once_bound of `ref` (default: the fp64 reference) element by element; the fp32 allowance comes from
    the same torch formula in fp32 on the CPU against fp64, never from the kernel"""
    a = KR.fp32_allowance(ref64, ref32)
    r, used = KR.bound_ratio(got, ref64 if ref is None else ref, a)
    print(f"[enc-kernels] {name} {shape}: worst error / bound {r:.3f} (fp32 allowance {a:.2e}, {100 * used:.0f} % of it used)")
    assert r <= 1.0, (name, shape, r)
    return r


# ------------------------------------------------------------------------------------------------
# 1. Swin window attention
# ------------------------------------------------------------------------------------------------
def _swin_launch(p, shape, out=None):
    from lib.hip import ops
    B, H, W, nH, shift = shape
    return ops.swin_window_attention(p["qkv"].cuda(), p["qkv_bias"].cuda(), p["rpb"].cuda(), B, H, W, nH * KR.HD, nH, KR.WS,
                                     shift, p["scale"], out=out)


def _swin_compare(p, shape, what=""):
    B, H, W, nH, shift = shape
    M, C = B * H * W, nH * KR.HD
    y1 = _swin_launch(p, shape)
    buf = torch.full((M + 16, C), SENTINEL, dtype=torch.float16, device="cuda")
    y2 = _swin_launch(p, shape, out=buf[:M])
    assert y2.data_ptr() == buf.data_ptr()
    assert bool((buf[M:] == SENTINEL).all()), "rows behind the last token were written"
    assert bool(torch.isfinite(buf[:M]).all()) and not bool((buf[:M] == SENTINEL).any()), "a token's row was not written"
    assert torch.equal(y1, buf[:M]), "two launches, different bits"
    err = (y1.double().cpu() - p["ref"]).abs() / p["vmax"]
    print(f"[enc-kernels] swin_window_attention {shape}{what}: max |err| / vmax {float(err.max()):.3e} "
          f"(bound {KR.SWIN_TOL:.3e}, vmax {p['vmax']:.2f})")
    assert bool((err <= KR.SWIN_TOL).all()), (shape, float(err.max()), int((err > KR.SWIN_TOL).sum()))


@pytest.mark.parametrize("shape", KR.SWIN_SHAPES, ids=_id)
def test_swin_window_attention_vs_fp64(shape):
    _swin_compare(KR.swin_problem(shape), shape)


def test_swin_window_attention_peaked_rows():
    """a bias table four times as large: rows dominated by a few keys, the max subtraction at work"""
    shape = (1, 14, 17, 2, 6)
    _swin_compare(KR.swin_problem(shape, rpb_mul=4.0), shape, " rpb x 4")


def test_swin_window_attention_argument_checks():
    from lib.hip import binding as _b, ops
    p = KR.swin_problem((1, 12, 12, 1, 0))
    q, b, r = p["qkv"].cuda(), p["qkv_bias"].cuda(), p["rpb"].cuda()
    with pytest.raises(_b.PfdError, match="PFD_ESHAPE"):
        ops.swin_window_attention(q, b, r, 1, 12, 12, 32, 1, 7, 0, p["scale"])          # ws != 12
    with pytest.raises(_b.PfdError, match="PFD_ESHAPE"):
        ops.swin_window_attention(q, b, r, 1, 12, 12, 64, 1, 12, 0, p["scale"])         # C != 32 nH
    with pytest.raises(_b.PfdError, match="PFD_EINVAL"):
        ops.swin_window_attention(q, b, r, 1, 12, 12, 32, 1, 12, 12, p["scale"])        # shift = 12


# ------------------------------------------------------------------------------------------------
# 2. LayerNorm
# ------------------------------------------------------------------------------------------------
def _ln_case(name, M, C, strided=False):
    from lib.hip import ops
    x, gamma, beta = KR.ln_operands(M, C, 31 * M + C)
    ref64, ref32 = KR.layernorm_ref(x, gamma, beta), KR.layernorm_ref(x, gamma, beta, dtype=torch.float32)
    if not strided:
        y = ops.layernorm(x.cuda(), gamma.cuda(), beta.cuda())
    else:   # x a column slice of a wider matrix, out a column slice of a sentinel-filled wider matrix
        wide = torch.full((M, C + 24), 3.0, dtype=torch.float16)
        wide[:, 8:8 + C] = x
        obuf = torch.full((M, C + 16), SENTINEL, dtype=torch.float16, device="cuda")
        y = ops.layernorm(wide.cuda()[:, 8:8 + C], gamma.cuda(), beta.cuda(), out=obuf[:, 8:8 + C])
        assert bool((obuf[:, :8] == SENTINEL).all()) and bool((obuf[:, 8 + C:] == SENTINEL).all()), \
            "columns outside the slice were written"
    assert tuple(y.shape) == (M, C)
    return _check(name, (M, C), y, ref64, ref32)


@pytest.mark.parametrize("C", [8, 192, 520, 1536, 2048, 2056, 3072, 3080, 4096])
@pytest.mark.parametrize("M", [1, 5])
def test_layernorm_one_row_per_wave(M, C):
    """one vector per lane with 63 idle lanes, one lane in the second slot, each of NV = 1, 2, 3, 4, 6, 8 (3080 -> 7 vectors,
    2056 -> 5: the two rounded-up instantiations)"""
    _ln_case("layernorm", M, C)


def test_layernorm_rejects_rows_wider_than_eight_vectors():
    from lib.hip import binding as _b, ops
    x, gamma, beta = KR.ln_operands(2, 4104, 1)
    with pytest.raises(_b.PfdError, match="PFD_ESHAPE"):
        ops.layernorm(x.cuda(), gamma.cuda(), beta.cuda())


@pytest.mark.parametrize("M,C", [(8192, 640), (8195, 320), (8193, 1536), (8192, 1544)])
def test_layernorm_four_rows_per_wave(M, C):
    """M >= 8192 and C <= 1536: layernorm_rows_kernel (8195: a ragged last wave; 1536: its widest row); 1544 is one step wider
    and takes the per-row kernel at the same M -- the same bound for both"""
    _ln_case("layernorm(rows)", M, C)


@pytest.mark.parametrize("M,C", [(5, 520), (8195, 320)])
def test_layernorm_strided_in_and_out(M, C):
    _ln_case("layernorm(strided)", M, C, strided=True)


@pytest.mark.parametrize("shape", [(1, 1, 1, 8), (2, 5, 7, 48), (1, 4, 6, 192), (1, 3, 3, 384), (1, 7, 2, 96)], ids=_id)
def test_layernorm_patch_merge_gather(shape):
    """out-of-image taps on odd H / W read as zero and still count in the mean over 4C ((1,1,1,8): three of the four parts)"""
    from lib.hip import ops
    B, H, W, Cq = shape
    g = torch.Generator().manual_seed(sum(shape))
    x = (torch.randn(shape, generator=g) + 0.5).half()
    gamma, beta = (1 + 0.2 * torch.randn(4 * Cq, generator=g)).half(), (0.1 * torch.randn(4 * Cq, generator=g)).half()
    y = ops.layernorm_patch_merge(x.cuda(), gamma.cuda(), beta.cuda())
    assert tuple(y.shape) == (B * ((H + 1) // 2) * ((W + 1) // 2), 4 * Cq)
    _check("layernorm_patch_merge", shape, y, KR.layernorm_patch_merge_ref(x, gamma, beta),
           KR.layernorm_patch_merge_ref(x, gamma, beta, dtype=torch.float32))


# ------------------------------------------------------------------------------------------------
# 3. row softmax
# ------------------------------------------------------------------------------------------------
def _softmax_x(R, N, seed):
    g = torch.Generator().manual_seed(seed)
    x = 3 * torch.randn((R, N), generator=g)
    x[torch.arange(R), torch.randint(0, N, (R,), generator=g)] += 20.0
    return x.half()


def _softmax_check(name, x, y, scale):
    R, N = x.shape
    ref64, ref32 = KR.softmax_rows_ref(x, scale), KR.softmax_rows_ref(x, scale, dtype=torch.float32)
    _check(name, (R, N, scale), y, ref64, ref32)
    s = y.double().cpu().sum(-1)
    print(f"[enc-kernels] {name} {(R, N, scale)}: row sums off 1 by {float((s - 1).abs().max()):.2e} (bound {N * 2.0 ** -12:.2e})")
    assert bool(((s - 1).abs() <= N * 2.0 ** -12).all()), s


@pytest.mark.parametrize("scale", [0.044, 1.0])
@pytest.mark.parametrize("N", [8, 504, 2056, 16384, 16392])
def test_softmax_rows(N, scale):
    """one vector, 63 vectors, one thread in the second slot, the largest register-resident row, the first streaming row"""
    from lib.hip import ops
    x = _softmax_x(3, N, N)
    _softmax_check("softmax_rows", x, ops.softmax_rows(x.cuda(), scale), scale)


@pytest.mark.parametrize("N", [2056, 16392])
def test_softmax_rows_strided(N):
    from lib.hip import ops
    x = _softmax_x(3, N, N + 1)
    wide = torch.full((3, N + 24), 50.0, dtype=torch.float16)       # neighbours that would dominate the row if they were read
    wide[:, 16:16 + N] = x
    obuf = torch.full((3, N + 16), SENTINEL, dtype=torch.float16, device="cuda")
    y = ops.softmax_rows(wide.cuda()[:, 16:16 + N], 1.0, out=obuf[:, 8:8 + N])
    assert bool((obuf[:, :8] == SENTINEL).all()) and bool((obuf[:, 8 + N:] == SENTINEL).all())
    _softmax_check("softmax_rows(strided)", x, y, 1.0)


# ------------------------------------------------------------------------------------------------
# 4. element-wise and layout kernels
# ------------------------------------------------------------------------------------------------
# scalar tail only, no tail, a tail after vectors, and the grid-stride loop past the 4096-block cap (+ a tail)
SIZES = [1, 7, 8, 9, 2049, 8 * 256 * 4096 + 13]


def _vec(n, seed, mul=1.0):
    return (mul * torch.randn(n, generator=torch.Generator().manual_seed(seed))).half()


@pytest.mark.parametrize("n", SIZES)
def test_add(n):
    from lib.hip import ops
    a, b = _vec(n, n), _vec(n, n + 1)
    y = ops.add(a.cuda(), b.cuda())
    _check("add", n, y, a.double() + b.double(), a.float() + b.float())


@pytest.mark.parametrize("n", SIZES)
def test_axpby(n):
    from lib.hip import ops
    a, b = _vec(n, n + 2), _vec(n, n + 3)
    y = ops.axpby(a.cuda(), 0.75, b.cuda(), -1.25)
    _check("axpby", n, y, KR.axpby_ref(a, 0.75, b, -1.25), KR.axpby_ref(a, 0.75, b, -1.25, dtype=torch.float32))
    y = ops.axpby(a.cuda(), -0.3)
    _check("axpby(no b)", n, y, KR.axpby_ref(a, -0.3), KR.axpby_ref(a, -0.3, dtype=torch.float32))


@pytest.mark.parametrize("act", [0, 1, 2, 3], ids=["none", "gelu", "relu", "silu"])
@pytest.mark.parametrize("n", SIZES)
def test_activation(n, act):
    from lib.hip import binding as _b, ops
    assert (_b.ACT_NONE, _b.ACT_GELU, _b.ACT_RELU, _b.ACT_SILU) == (0, 1, 2, 3)
    x = _vec(n, n + 4, mul=2.0)
    y = ops.activation(x.cuda(), act)
    _check(f"activation({('none', 'gelu', 'relu', 'silu')[act]})", n, y, KR.activation_ref(x, act),
           KR.activation_ref(x, act, dtype=torch.float32))


@pytest.mark.parametrize("R,C,strided", [(5, 8, False), (37, 1280, False), (37, 1280, True)])
def test_add_rowvec(R, C, strided):
    from lib.hip import ops
    g = torch.Generator().manual_seed(R + C)
    x, v = torch.randn((R, C), generator=g).half(), torch.randn((C,), generator=g).half()
    if not strided:
        y = ops.add_rowvec(x.cuda(), v.cuda())
    else:
        wide = torch.full((R, C + 24), 3.0, dtype=torch.float16)
        wide[:, 16:16 + C] = x
        obuf = torch.full((R, C + 16), SENTINEL, dtype=torch.float16, device="cuda")
        y = ops.add_rowvec(wide.cuda()[:, 16:16 + C], v.cuda(), out=obuf[:, 8:8 + C])
        assert bool((obuf[:, :8] == SENTINEL).all()) and bool((obuf[:, 8 + C:] == SENTINEL).all())
    _check("add_rowvec" + ("(strided)" if strided else ""), (R, C), y, x.double() + v.double()[None], x.float() + v.float()[None])


@pytest.mark.parametrize("R,C", [(5, 160), (300, 320), (64, 1280)])
def test_add_rowvec_with_row_statistics(R, C):
    """ln_out=: the output is the plain form's bit for bit, the emitted sums are ln_rowstats of that output bit for bit (the
    source promises one summation order), and both are the fp64 row sums within 1e-5 of the mass summed (the bar of
    test_upsample_phase_gpu.py::test_phase_form_statistics)"""
    from lib.hip import ops
    g = torch.Generator().manual_seed(R + C)
    x, v = (torch.randn((R, C), generator=g) + 0.3).half().cuda(), torch.randn((C,), generator=g).half().cuda()
    st = torch.full((R, C // 160, 2), float("nan"), dtype=torch.float32, device="cuda")
    y = ops.add_rowvec(x, v, ln_out=st)
    assert torch.equal(y, ops.add_rowvec(x, v))
    _check("add_rowvec(ln_out)", (R, C), y, x.double().cpu() + v.double().cpu()[None], x.float().cpu() + v.float().cpu()[None])
    st2 = ops.ln_rowstats(y)
    assert torch.equal(st, st2), "the two producers of row statistics disagree"
    yd = y.double().cpu().view(R, C // 160, 160)
    s64, q64, mass = yd.sum(-1), (yd * yd).sum(-1), yd.abs().sum(-1)
    e_s = float(((st[..., 0].double().cpu() - s64).abs() / mass).max())
    e_q = float(((st[..., 1].double().cpu() - q64).abs() / q64).max())
    print(f"[enc-kernels] add_rowvec(ln_out) {(R, C)}: sums {e_s:.2e}, sums of squares {e_q:.2e} (relative, bound 1e-5)")
    assert e_s <= 1e-5 and e_q <= 1e-5, (e_s, e_q)


@pytest.mark.parametrize("src", [torch.float32, torch.float16], ids=["f32", "f16"])
def test_to_nhwc(src):
    from lib.hip import ops
    shape = (2, 3, 5, 7)
    x = torch.randn(shape, generator=torch.Generator().manual_seed(11)).to(src)
    y = ops.to_nhwc(x.cuda(), mul=2.0, add=-1.0, rep=2)
    assert tuple(y.shape) == (4, 5, 7, 3) and y.dtype == torch.float16
    _check(f"to_nhwc({'f32' if src == torch.float32 else 'f16'})", shape, y, KR.to_nhwc_ref(x, 2.0, -1.0, 2),
           KR.to_nhwc_ref(x, 2.0, -1.0, 2, dtype=torch.float32))


@pytest.mark.parametrize("dst", [torch.float32, torch.float16], ids=["f32", "f16"])
@pytest.mark.parametrize("shape", [(2, 9, 13, 4), (1, 8, 9, 130)], ids=_id)
def test_to_nchw(shape, dst):
    """HW and C both ragged against the 64x64 tile (117 x 4, 72 x 130: three channel tiles); unit-Gaussian inputs through
    clamp(0.5 x + 0.5, 0, 1) clamp on both sides"""
    from lib.hip import ops
    x = torch.randn(shape, generator=torch.Generator().manual_seed(sum(shape))).half()
    ref64 = KR.to_nchw_ref(x, 0.5, 0.5, 0.0, 1.0)
    assert bool((ref64 == 0).any()) and bool((ref64 == 1).any())
    y = ops.to_nchw(x.cuda(), dst, mul=0.5, add=0.5, lo=0.0, hi=1.0)
    assert y.dtype == dst and tuple(y.shape) == (shape[0], shape[3], shape[1], shape[2])
    _check(f"to_nchw({'f32' if dst == torch.float32 else 'f16'})", shape, y, ref64,
           KR.to_nchw_ref(x, 0.5, 0.5, 0.0, 1.0, dtype=torch.float32))


@pytest.mark.parametrize("cin", [3, 4])
@pytest.mark.parametrize("ks,stride,pad,extra", [(3, 1, 1, 0), (3, 2, 1, 0), (3, 2, 0, 1), (1, 1, 0, 0)])
def test_im2col_bit_for_bit(cin, ks, stride, pad, extra):
    """values are copied: equal bits.  x is a channel slice of a wider tensor (ldx > Cin), kpad = 64 > 9 Cin with a zero tail,
    ho / wo given explicitly as the stride-2 callers do (extra = 1: one more row / column of bottom / right padding)"""
    from lib.hip import ops
    B, H, W, kpad = 2, 6, 9, 64
    g = torch.Generator().manual_seed(cin + ks + stride + pad)
    wide = torch.randn((B, H, W, cin + 5), generator=g).half()
    x = wide[..., 2:2 + cin]
    ho, wo = (H + 2 * pad - ks) // stride + 1 + extra, (W + 2 * pad - ks) // stride + 1 + extra
    col, Ho, Wo = ops.im2col(wide.cuda()[..., 2:2 + cin], ks, stride, pad, kpad, ho, wo)
    assert (Ho, Wo) == (ho, wo) and tuple(col.shape) == (B * ho * wo, kpad)
    ref = KR.im2col_ref(x, ks, stride, pad, kpad, ho, wo)
    assert torch.equal(col.cpu(), ref), int((col.cpu() != ref).sum())
    assert float(col[:, ks * ks * cin:].abs().max()) == 0.0
    if not extra:       # the default extent is the symmetric-padding one
        col2, Ho2, Wo2 = ops.im2col(wide.cuda()[..., 2:2 + cin], ks, stride, pad, kpad)
        assert (Ho2, Wo2) == (ho, wo) and torch.equal(col2, col)


@pytest.mark.parametrize("dim", [320, 321])
def test_timestep_embedding(dim):
    """against the reference project's own fp32 formula (its frequencies are defined in fp32); the allowance is that formula's
    distance from its all-fp64 evaluation.  The odd dim leaves a zero last column."""
    from lib.hip import ops
    t = torch.tensor([0, 1, 500, 999])
    y = ops.timestep_embedding(t.cuda(), dim)
    ref32 = O.timestep_embedding(t, dim)
    assert tuple(y.shape) == (4, dim)
    _check("timestep_embedding", (4, dim), y, KR.timestep_embedding_ref64(t, dim), ref32, ref=ref32)
    if dim % 2:
        assert float(y[:, -1].abs().max()) == 0.0
