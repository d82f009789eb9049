"""Plain fp64 references of single kernels of the SeeCoder side of the library, and the seeded operands the kernel-level
tests run them on (tests/test_encoder_kernels_cpu.py pins the references to the oracle, tests/test_encoder_kernels_gpu.py
compares the HIP kernels with them).  Everything here is torch on whatever device the operands live on; nothing imports the
native library.  A plain module, not a conftest: the two test files import it by name."""
import functools

import torch
import torch.nn.functional as F

import pfd_oracle as O

WS, HD = 12, 32                     # pfd_swin_window_attention_f16: window 12, head_dim 32

# (B, H, W, nH, shift): the smallest shapes that reach each edge of the window-attention index arithmetic
SWIN_SHAPES = [
    (1, 12, 12, 1, 0), (1, 12, 12, 1, 6),         # one window, no padding
    (1, 14, 17, 2, 0), (1, 14, 17, 2, 6),         # padding in both directions, 2x2 windows, not square
    (2, 24, 24, 1, 6), (3, 13, 12, 2, 6),         # B > 1
    (1, 8, 8, 3, 6),                              # extent below the window: the roll wraps the padding into the middle
    (2, 5, 30, 2, 6),                             # H below the shift
    (1, 25, 13, 6, 6),                            # the stage-0 head count, 11 rows / columns of padding
    (1, 36, 12, 1, 0), (1, 7, 19, 2, 0),          # further padded, unshifted cases
    (1, 4, 5, 48, 6), (1, 4, 5, 48, 0),           # stage 3 of the 128x160 fixture image: grid.y = 48, rows of 4608
    (1, 16, 16, 48, 6),                           # stage 3 of a 512 px picture
]
# the GPU tolerance: per element, relative to the largest |v| the launch can read.  The output is a convex combination of v
# values; the kernel rounds the normalised probabilities to fp16 once (<= 2^-11 vmax over the sum) and the result to fp16 once
# (another 2^-11 vmax); fp32 MFMA accumulation and __expf add about 1e-6; the third 2^-11 is the margin.
SWIN_TOL = 3 * 2.0 ** -11
# wrong variants of the reference (test B of the CPU file: the operands must tell each of them from the right one)
SWIN_MUTANTS = ("pad_reads_zero", "roll_reversed", "bias_transposed", "regions_from_unpadded", "mask_at_shift0")


def _regions(Hp, Wp, eh, ew, shift):
    """region ids [Hp, Wp] of the shift mask with the boundaries counted from the extents (eh, ew), as index arithmetic"""
    ys, xs = torch.arange(Hp), torch.arange(Wp)
    rh = (ys >= eh - WS).long() + (ys >= eh - shift).long()
    rw = (xs >= ew - WS).long() + (xs >= ew - shift).long()
    return (rh[:, None] * 3 + rw[None, :]).double()


def swin_window_attention_ref(qkv, qkv_bias, rpb, B, H, W, nH, shift, scale, mutant=None):
    """fp64, literally in the order of swin.py / pfd_oracle.swin_block: pad (a padded token's q|k|v is the qkv bias), roll,
    window partition, q k^T * scale + bias table gather, the -100 mask from the nine slices of the padded frame, softmax,
    @ v, window reverse, roll back, crop.  qkv [B*H*W, 3C], qkv_bias [3C], rpb [529, nH] -> [B*H*W, C] float64.
    mutant: one of SWIN_MUTANTS -- a deliberately wrong variant."""
    assert mutant is None or mutant in SWIN_MUTANTS
    C = nH * HD
    dev = qkv.device
    Hp, Wp = -(-H // WS) * WS, -(-W // WS) * WS
    nWy, nWx = Hp // WS, Wp // WS
    fill = torch.zeros_like(qkv_bias) if mutant == "pad_reads_zero" else qkv_bias
    frame = fill.double().expand(B, Hp, Wp, 3 * C).clone()
    frame[:, :H, :W] = qkv.double().view(B, H, W, 3 * C)
    sgn = 1 if mutant == "roll_reversed" else -1
    if shift > 0:
        frame = torch.roll(frame, shifts=(sgn * shift, sgn * shift), dims=(1, 2))
    win = frame.view(B, nWy, WS, nWx, WS, 3, nH, HD).permute(5, 0, 1, 3, 6, 2, 4, 7).reshape(3, B * nWy * nWx, nH, WS * WS, HD)
    q, k, v = win[0], win[1], win[2]
    idx = O.swin_rel_index(WS)
    if mutant == "bias_transposed":
        idx = idx.t()
    bias = rpb.double()[idx.reshape(-1).to(dev)].view(WS * WS, WS * WS, nH).permute(2, 0, 1)
    attn = q @ k.transpose(-2, -1) * scale + bias[None]
    mshift = WS // 2 if mutant == "mask_at_shift0" else shift      # (the mask of the shifted blocks on an unshifted one)
    if mshift > 0:
        if mutant == "regions_from_unpadded":
            img = _regions(Hp, Wp, H, W, mshift)
        else:
            img = torch.zeros((Hp, Wp), dtype=torch.float64)
            cnt = 0
            for hs in (slice(0, -WS), slice(-WS, -mshift), slice(-mshift, None)):
                for ws_ in (slice(0, -WS), slice(-WS, -mshift), slice(-mshift, None)):
                    img[hs, ws_] = cnt
                    cnt += 1
        mw = img.view(nWy, WS, nWx, WS).permute(0, 2, 1, 3).reshape(nWy * nWx, WS * WS)
        mask = torch.where(mw[:, None, :] != mw[:, :, None], -100.0, 0.0).to(dev)           # [nW, 144, 144]
        attn = (attn.view(B, nWy * nWx, nH, WS * WS, WS * WS) + mask[None, :, None]).view(-1, nH, WS * WS, WS * WS)
    o = (attn.softmax(dim=-1) @ v).transpose(1, 2).reshape(B, nWy, nWx, WS, WS, C)
    o = o.permute(0, 1, 3, 2, 4, 5).reshape(B, Hp, Wp, C)
    if shift > 0:
        o = torch.roll(o, shifts=(-sgn * shift, -sgn * shift), dims=(1, 2))
    return o[:, :H, :W].reshape(B * H * W, C)


@functools.lru_cache(maxsize=None)
def swin_problem(shape, rpb_mul=1.0):
    """the fp16 operands of one window-attention case (CPU; csrc/selftest.cpp's distributions, so the bias and the mask matter
    to the result) with the fp64 reference and vmax, the largest |v| the launch can read.  Computed once; do not modify."""
    B, H, W, nH, shift = shape
    C = nH * HD
    g = torch.Generator().manual_seed(1000003 * B + 10007 * H + 101 * W + 7 * nH + shift)
    qkv = (1.5 * torch.randn((B * H * W, 3 * C), generator=g)).half()
    qkv_bias = (0.5 * torch.randn((3 * C,), generator=g)).half()
    rpb = (rpb_mul * torch.randn(((2 * WS - 1) ** 2, nH), generator=g)).half()
    scale = HD ** -0.5
    ref = swin_window_attention_ref(qkv, qkv_bias, rpb, B, H, W, nH, shift, scale)
    vmax = max(float(qkv[:, 2 * C:].abs().max()), float(qkv_bias[2 * C:].abs().max()))
    return dict(qkv=qkv, qkv_bias=qkv_bias, rpb=rpb, scale=scale, ref=ref, vmax=vmax)


# ------------------------------------------------------------------------------------------------
# row-wise kernels
# ------------------------------------------------------------------------------------------------
def layernorm_ref(x, gamma, beta, eps=1e-5, dtype=torch.float64):
    """F.layer_norm over the last dimension in `dtype` on the given operands"""
    return F.layer_norm(x.to(dtype), (x.shape[-1],), gamma.to(dtype), beta.to(dtype), eps)


def patch_merge_gather(x):
    """[B, H, W, C] -> [B, ceil(H/2) * ceil(W/2), 4C]: the PatchMerging lines of swin.py / pfd_oracle.swin_forward, restated"""
    B, H, W, C = x.shape
    g = F.pad(x, (0, 0, 0, W % 2, 0, H % 2))
    g = torch.cat([g[:, 0::2, 0::2], g[:, 1::2, 0::2], g[:, 0::2, 1::2], g[:, 1::2, 1::2]], -1)
    return g.reshape(B, -1, 4 * C)


def layernorm_patch_merge_ref(x, gamma, beta, eps=1e-5, dtype=torch.float64):
    """x [B, H, W, Cq] -> LayerNorm(4 Cq) of the gather, [B * Ho * Wo, 4 Cq]: taps outside the image are zeros that count
    in the statistics"""
    g = patch_merge_gather(x.to(dtype))
    return layernorm_ref(g.reshape(-1, g.shape[-1]), gamma, beta, eps, dtype)


def softmax_rows_ref(x, scale, dtype=torch.float64):
    return torch.softmax(x.to(dtype) * scale, dim=-1)


def ln_operands(M, C, seed):
    """x = randn + 0.5 (a mean to subtract), gamma = 1 + 0.2 randn, beta = 0.1 randn; fp16, CPU"""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn((M, C), generator=g) + 0.5).half()
    return x, (1 + 0.2 * torch.randn(C, generator=g)).half(), (0.1 * torch.randn(C, generator=g)).half()


# ------------------------------------------------------------------------------------------------
# element-wise and layout kernels
# ------------------------------------------------------------------------------------------------
def activation_ref(x, act, dtype=torch.float64):
    """act: 0 none | 1 GELU (erf) | 2 ReLU | 3 SiLU -- binding.ACT_*"""
    x = x.to(dtype)
    return (x, F.gelu(x), torch.relu(x), F.silu(x))[act]


def axpby_ref(a, alpha, b=None, beta=0.0, dtype=torch.float64):
    y = alpha * a.to(dtype)
    return y if b is None else y + beta * b.to(dtype)


def to_nhwc_ref(x, mul, add, rep, dtype=torch.float64):
    """NCHW -> NHWC, x * mul + add, the batch repeated `rep` times"""
    y = (x.to(dtype) * mul + add).permute(0, 2, 3, 1)
    return torch.cat([y] * rep).contiguous()


def to_nchw_ref(x, mul, add, lo, hi, dtype=torch.float64):
    return (x.to(dtype) * mul + add).clamp(lo, hi).permute(0, 3, 1, 2).contiguous()


def im2col_ref(x, ks, stride, pad, kpad, ho=None, wo=None):
    """x [B, H, W, Cin] fp16 -> [B * Ho * Wo, kpad] fp16: F.unfold rearranged to (tap, channel) order, zero tail.  ho / wo
    beyond the symmetric-padding extent read zeros below / right of the image (the stride-2 callers' bottom / right pad)."""
    B, H, W, Cin = x.shape
    Ho = (H + 2 * pad - ks) // stride + 1 if ho is None else ho
    Wo = (W + 2 * pad - ks) // stride + 1 if wo is None else wo
    need_h, need_w = (Ho - 1) * stride + ks, (Wo - 1) * stride + ks
    xp = F.pad(x.double().permute(0, 3, 1, 2), (pad, max(pad, need_w - W - pad), pad, max(pad, need_h - H - pad)))
    Hn, Wn = (xp.shape[2] - ks) // stride + 1, (xp.shape[3] - ks) // stride + 1
    u = F.unfold(xp, ks, stride=stride).view(B, Cin, ks * ks, Hn, Wn)[:, :, :, :Ho, :Wo]       # [B, Cin, tap, Ho, Wo]
    col = torch.zeros((B * Ho * Wo, kpad), dtype=torch.float64)
    col[:, :ks * ks * Cin] = u.permute(0, 3, 4, 2, 1).reshape(B * Ho * Wo, ks * ks * Cin)
    return col.half()                                                                           # (copies: exact)


def timestep_embedding_ref64(t, dim, max_period=10000):
    """O.timestep_embedding's formula with every step in fp64 (the reference project defines the frequencies in fp32: this is
    only the yardstick of the fp32 formula's own arithmetic)"""
    import math
    half = dim // 2
    freqs = torch.exp(-math.log(max_period) * torch.arange(0, half, dtype=torch.float64) / half)
    args = t[:, None].double() * freqs[None]
    emb = torch.cat([torch.cos(args), torch.sin(args)], dim=-1)
    if dim % 2:
        emb = torch.cat([emb, torch.zeros_like(emb[:, :1])], dim=-1)
    return emb


# ------------------------------------------------------------------------------------------------
# the per-element bound of the kernels that evaluate a shallow formula in fp32 and round once to fp16
# ------------------------------------------------------------------------------------------------
def fp32_allowance(ref64, ref32):
    """a = max(8 e32, 16 * 2^-24 max|ref|): e32 is the largest difference between the same torch formula evaluated in fp32 on
    the CPU and the fp64 reference (the reference's own arithmetic, never the kernel's); 8 is the margin for device
    expf / erff / rsqrtf, a few ulp looser than the host's; the 16-ulp floor covers formulas that are exact in fp32 on the host"""
    e32 = float((ref32.double().cpu() - ref64.double().cpu()).abs().max())
    return max(8 * e32, 16 * 2.0 ** -24 * float(ref64.abs().max()))


def round_once_bound(ref, a):
    """|got - ref| <= 2^-11 (|ref| + a) + a: half an fp16 ulp of the value (2^-25 where it is subnormal) plus the allowance"""
    return torch.clamp(2.0 ** -11 * (ref.double().abs() + a), min=2.0 ** -25) + a


def bound_ratio(got, ref, a):
    """(the worst |got - ref| / bound over the elements (<= 1 passes), the largest share of the allowance `a` that an element
    needs beyond its half ulp).  A correctly rounded result reaches 1.0 of the half-ulp term on some element of any large
    tensor, so the first figure sits just below 1 for a right kernel; the second says how much of `a` its fp32 arithmetic used."""
    ref = ref.double().cpu()
    got = got.double().cpu()
    assert got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
    assert bool(torch.isfinite(got).all()), "non-finite output"
    err = (got - ref).abs()
    used = float(((err - round_once_bound(ref, a) + a) / a).clamp_min(0).max())
    return float((err / round_once_bound(ref, a)).max()), used
