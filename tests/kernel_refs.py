"""Plain fp64 references of single kernels of the library, and the seeded operands the kernel-level tests run them on: the
SeeCoder side (tests/test_encoder_kernels_cpu.py pins the references to the oracle, tests/test_encoder_kernels_gpu.py
compares the HIP kernels with them), the fused attention family (tests/test_attention_kernels_{cpu,gpu}.py), the GEMM /
convolution kernels (tests/test_gemm_kernels_{cpu,gpu}.py, tests/test_gemm_range_{cpu,gpu}.py) and the stand-alone GroupNorm kernels
(tests/test_norm_kernels_{cpu,gpu}.py, the last section).  Everything here is torch on whatever device the operands live on; nothing imports the
native library.  A plain module, not a conftest: the two test files import it by name."""
import functools
import math
import re
import zlib

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


# ------------------------------------------------------------------------------------------------
# fused attention (pfd_attention_f16): references, the dispatcher restated, cases and operands
# (tests/test_attention_kernels_cpu.py pins and qualifies them, tests/test_attention_kernels_gpu.py uses them)
# ------------------------------------------------------------------------------------------------
LOG2E = 1.4426950408889634
ATTN_MUTANTS = ("last_key_dropped", "masked_keys_score_zero", "vt_batch0", "k_batch0", "v_pad_column_read")
ATTN_CLASSES = ("w4", "w8", "a3", "d80", "d96", "d160", "d512_2", "d512_4")
ATTN_FOLDED = ("w8", "a3")          # Q' = fp16(q * scale * log2 e), softmax as exp2 of the raw products


# the class of every kernel `emu_attn --dispatch` can record (tests/golden/attention_dispatch.txt)
ATTN_KERNEL_CLASS = {"attention3_kernel": "a3", "attention512_kernel<2>": "d512_2", "attention512_kernel<4>": "d512_4"}
for _k in ("attention2_kernel", "attention_kbias_kernel", "attention_rbias_kernel"):
    ATTN_KERNEL_CLASS.update({f"{_k}<40, 4, false, false>": "w4", f"{_k}<40, 8, true, true>": "w8", f"{_k}<80, 4, false, false>": "d80",
                              f"{_k}<96, 4, false, false>": "d96", f"{_k}<160, 4, false, false>": "d160"})


def attention_kernel_class(B, H, Nq, Nk, D, slices=2, operand=None):
    """which kernel pfd_attention_f16 (operand None), pfd_attention_kbias_f16 ("kbias") or pfd_attention_rbias_f16 ("rbias")
    launches: attn_plan() of csrc/attention_params.h restated without the process-static test hooks, and held to it line by
    line of the pinned dry run (tests/test_attention_kernels_cpu.py).  None: PFD_ESHAPE."""
    if D == 512:
        return f"d512_{4 if slices == 4 else 2}" if not operand and H == 1 and Nk % 32 == 0 else None
    if D not in (40, 80, 160) and (D != 96 or operand):
        return None
    if D != 40:
        return f"d{D}"
    blocks = B * H * ((Nq + 255) // 256)
    if not operand and Nk % 64 == 0 and Nk >= 128 and Nq >= 256 and blocks >= 256:
        return "a3"
    return "w8" if operand != "rbias" and Nq >= 1024 and blocks >= 512 else "w4"


# (B, H, Nq, Nk, D, layout, spike); layouts: dense | fused_qk | vt_offset | shared_kv (attention_problem)
ATTN_CASES = [
    # w4: attention2_kernel<40, 4, false>
    (2, 2, 77, 64, 40, "fused_qk", 0),          # exactly one full tile
    (1, 2, 300, 148, 40, "dense", 0),
    (1, 1, 33, 1, 40, "dense", 0),              # one key
    (1, 1, 1, 7, 40, "dense", 0),               # one query, Nk below 8: v_last = 0
    (1, 1, 256, 65, 40, "dense", 0),            # one key in the peeled tile
    (1, 2, 130, 127, 40, "dense", 0),
    (1, 2, 130, 129, 40, "vt_offset", 0),
    (3, 2, 64, 148, 40, "shared_kv", 0),
    (1, 2, 300, 148, 40, "dense", 140),         # spike inside the peeled tile
    # w8: attention2_kernel<40, 8, true, true>
    (16, 8, 1024, 148, 40, "vt_offset", 0),
    (13, 8, 1030, 77, 40, "dense", 0),          # ragged last query block, 520 blocks
    (16, 8, 1024, 64, 40, "dense", 0),          # one full tile (a3 declines below 128 keys)
    (16, 8, 1024, 8, 40, "dense", 0),
    (16, 8, 1024, 200, 40, "dense", 0),
    (16, 8, 1024, 200, 40, "dense", 130),
    (16, 8, 1024, 148, 40, "vt_offset", 140),
    # a3: attention3_kernel; 2, 3, 4, 5, 9 key tiles around the ring depths (5 / 4) and the pair parity
    (32, 8, 256, 128, 40, "dense", 0),
    (32, 8, 256, 192, 40, "fused_qk", 0),
    (32, 8, 256, 256, 40, "dense", 0),
    (32, 8, 256, 320, 40, "fused_qk", 0),
    (32, 8, 256, 576, 40, "dense", 0),
    (16, 8, 300, 192, 40, "dense", 0),          # second block: 44 valid queries, whole sub-blocks and waves past Nq
    (8, 8, 1024, 1024, 40, "fused_qk", 0),
    (32, 8, 256, 320, 40, "fused_qk", 200),
    (32, 8, 256, 256, 40, "dense", 100),
    (8, 8, 1024, 1024, 40, "fused_qk", 700),
    # d80 / d96 / d160: attention2_kernel<D, 4, false>
    (2, 2, 64, 64, 80, "dense", 0), (1, 2, 150, 148, 80, "dense", 0), (1, 1, 40, 1, 80, "dense", 0),
    (1, 2, 150, 148, 80, "dense", 100),
    (1, 8, 144, 256, 96, "dense", 0), (1, 3, 148, 148, 96, "dense", 0), (1, 2, 144, 200, 96, "dense", 0),
    (2, 2, 64, 148, 160, "dense", 0), (1, 1, 256, 320, 160, "fused_qk", 0), (1, 2, 70, 8, 160, "dense", 0),
    # d512: attention512_kernel<2 / 4> (the GPU file runs each with PFD_ATTN512_SLICES = 2 and 4)
    (1, 1, 128, 32, 512, "dense", 0),           # one key tile
    (1, 1, 200, 96, 512, "dense", 0),           # ragged query tile
    (2, 1, 128, 512, 512, "fused_qk", 0),
    (1, 1, 128, 512, 512, "dense", 300),
]
# operand variants on top of a case (attention_problem(case, variant))
ATTN_STAIRCASE = [(16, 8, 1024, 200, 40, "dense", 0), (32, 8, 256, 320, 40, "fused_qk", 0)]       # w8, a3
ATTN_PEAKED = [(1, 2, 300, 148, 40, "dense", 0), (16, 8, 1024, 200, 40, "dense", 0), (32, 8, 256, 320, 40, "fused_qk", 0),
               (1, 2, 150, 148, 80, "dense", 0), (1, 3, 148, 148, 96, "dense", 0), (2, 2, 64, 148, 160, "dense", 0),
               (1, 1, 200, 96, 512, "dense", 0)]                                                    # one per class


def attn_case_id(case):
    B, H, Nq, Nk, D, layout, spike = case
    return f"B{B}H{H}q{Nq}k{Nk}d{D}-{layout}" + (f"-spike{spike}" if spike else "")


def _attn_views(q, k, vt, B, H, Nq, Nk, D, ldq, ldk, ldvt, q_bs, k_bs, vt_bs, q_off, k_off, vt_off):
    """[B, H, N, D] views of the three flat buffers by the address formulas of include/pfd_hip.h (PfdAttnDesc)"""
    Q = q.as_strided((B, H, Nq, D), (q_bs, D, ldq, 1), q.storage_offset() + q_off)
    K = k.as_strided((B, H, Nk, D), (k_bs, D, ldk, 1), k.storage_offset() + k_off)
    V = vt.as_strided((B, H, Nk, D), (vt_bs, D * ldvt, 1, ldvt), vt.storage_offset() + vt_off)
    return Q, K, V


def _attention(q, k, vt, B, H, Nq, Nk, D, scale, ldq, ldk, ldvt, q_bs, k_bs, vt_bs, q_off, k_off, vt_off, mutant, folded,
               dtype=torch.float64):
    assert mutant is None or mutant in ATTN_MUTANTS
    if mutant == "vt_batch0":
        vt_bs = 0
    if mutant == "k_batch0":
        k_bs = 0
    nk = Nk - 1 if mutant == "last_key_dropped" and Nk > 1 else Nk
    Nkp = (Nk + 7) // 8 * 8
    if mutant == "v_pad_column_read":        # key j reads the column of key j + (Nkp - Nk): the last ones read the pad
        Q, K, V = _attn_views(q, k, vt, B, H, Nq, Nk, D, ldq, ldk, ldvt, q_bs, k_bs, vt_bs, q_off, k_off, vt_off + Nkp - Nk)
    else:
        Q, K, V = _attn_views(q, k, vt, B, H, Nq, nk, D, ldq, ldk, ldvt, q_bs, k_bs, vt_bs, q_off, k_off, vt_off)
    npad = (-Nk) % 64 if mutant == "masked_keys_score_zero" else 0
    # the kernels' factor: the fp32 product of fp32(scale) and fp32(log2 e) (pfd_attention_f16: d->scale * 1.4426950408889634f)
    c32 = float(torch.tensor(scale, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32))
    out = torch.empty((B, Nq, H * D), dtype=dtype, device=q.device)
    hc = max(1, min(H, (256 << 20) // (8 * Nq * (Nk + npad))))            # heads per chunk: scores below about 256 MB
    for b in range(B):
        for h0 in range(0, H, hc):
            qc, kc, vc = Q[b, h0:h0 + hc], K[b, h0:h0 + hc].to(dtype), V[b, h0:h0 + hc].to(dtype)
            if folded:      # the kernels' operand: fp16(fp32(q) * fp32(scale * log2 e)); scores in log2 units
                qc = (qc.float() * c32).half().to(dtype)
                s = qc @ kc.transpose(-1, -2)
            else:
                s = (qc.to(dtype) @ kc.transpose(-1, -2)) * scale
            if npad:
                s = torch.cat([s, s.new_zeros(s.shape[:-1] + (npad,))], -1)
                vc = torch.cat([vc, vc.new_zeros(vc.shape[:-2] + (npad, D))], -2)
            if folded:
                p = torch.exp2(s - s.amax(-1, keepdim=True))
                p = p / p.sum(-1, keepdim=True)
            else:
                p = s.softmax(-1)
            out[b, :, h0 * D:(h0 + len(qc)) * D] = (p @ vc).transpose(0, 1).reshape(Nq, -1)
    return out


def attention_ref(q, k, vt, B, H, Nq, Nk, D, scale, *, ldq, ldk, ldvt, q_bs, k_bs, vt_bs, q_off=0, k_off=0, vt_off=0,
                  mutant=None, dtype=torch.float64):
    """softmax_j(scale <Q[b,i,h], K[b,j,h]>) . V[b,j,h] in fp64 -> [B, Nq, H * D].  q / k / vt are the flat fp16 buffers (or
    views into them; *_off are further element offsets), indexed by the address formulas of include/pfd_hip.h with
    as_strided -- the strides are part of what is under test.  mutant: one of ATTN_MUTANTS, a deliberately wrong variant."""
    return _attention(q, k, vt, B, H, Nq, Nk, D, scale, ldq, ldk, ldvt, q_bs, k_bs, vt_bs, q_off, k_off, vt_off, mutant, False,
                      dtype)


def attention_ref_folded(q, k, vt, B, H, Nq, Nk, D, scale, *, ldq, ldk, ldvt, q_bs, k_bs, vt_bs, q_off=0, k_off=0, vt_off=0,
                         mutant=None):
    """the same with the operand quantisation of the folded-maximum kernels (csrc/attention.hip, the FOLD comment and the
    query fragment load): Q' = fp16(fp32(q) * fp32(scale * log2 e)), p = exp2(<Q', K> - max); every other step in fp64"""
    return _attention(q, k, vt, B, H, Nq, Nk, D, scale, ldq, ldk, ldvt, q_bs, k_bs, vt_bs, q_off, k_off, vt_off, mutant, True)


def attention_fold_amplitude(q, k, B, H, Nq, Nk, D, scale, *, ldq, ldk, q_bs, k_bs, q_off=0, k_off=0, **_):
    """A = max over the launch of sum_e |q'_e k_e|, q' = q * scale * log2 e, in fp64: the worst case of rounding Q' to fp16 is
    a score error of 2^-11 A (log2 units)"""
    Q = q.as_strided((B, H, Nq, D), (q_bs, D, ldq, 1), q.storage_offset() + q_off)
    K = k.as_strided((B, H, Nk, D), (k_bs, D, ldk, 1), k.storage_offset() + k_off)
    a = 0.0
    for b in range(B):
        a = max(a, float((Q[b].double().abs() @ K[b].double().abs().transpose(-1, -2)).max()))
    return a * scale * LOG2E


# The GPU bound, per element, relative to vmax = the largest |V| among the valid keys of the launch (the output is a convex
# combination of V values):
#   2^-11   P = exp2(s - m) is rounded to fp16 once; every p_j is off by at most 2^-11 relative, so the numerator
#           sum_j p_j v_j moves by at most 2^-11 vmax sum_j p_j
#   2^-11   the row sum carries the same rounding (the ones row sums the rounded P; the register sum the unrounded one)
#   2^-11   the result is rounded to fp16 once (half an ulp of a value <= vmax)
#   Nk 2^-25  a P value below 2^-14 is subnormal in fp16 and loses up to 2^-25 absolutely, against a row sum >= 1
#   2^-16   fp32 score accumulation, the fma in front of v_exp_f32 and v_exp_f32 itself (1 ulp)
# The folded kernels round Q' = q scale log2(e) to fp16: a score moves by at most 2^-11 sum_e |q'_e k_e| <= 2^-11 A (log2
# units), a probability by the factor 2^(+-2^-11 A), numerator against denominator by twice that: 2 ln2 2^-11 A vmax.
def attention_bound(Nk, vmax, A=0.0):
    return (3 * 2.0 ** -11 + Nk * 2.0 ** -25 + 2.0 ** -16 + 2 * 0.6931471805599453 * 2.0 ** -11 * A) * vmax


_POISON = torch.tensor([0x7E00, -0x0200, 0x7C01, 0x7FFF], dtype=torch.int16)     # fp16 NaNs: quiet, negative, signalling, all ones


def _poisoned(n):
    return _POISON.repeat(-(-n // 4))[:n].clone().view(torch.float16)


@functools.lru_cache(maxsize=None)
def attention_problem(case, variant=None):
    """the fp16 operands of one case (CPU; seeded from the case; Q, K = 1.5 randn, V = randn: csrc/selftest.cpp's
    distributions) as flat buffers `q`, `k`, `vt` plus `desc`, the keyword arguments of ops.attention / attention_ref.
    Every element a launch may read but must not use is an fp16 NaN: V^T columns Nk .. Nkp, K pad rows, the rows of a fused
    [B N, 2C] matrix beyond Nq (Q half) / Nk (K half), the skipped leading sample; `*_valid` are the masks of the rest.
    variant: None | "peaked" (four query rows x 6) | "staircase" (the tile maximum rises by 5 log2 units per 64-key tile).
    Do not modify the result."""
    B, H, Nq, Nk, D, layout, spike = case
    C, Nkp, scale = H * D, (Nk + 7) // 8 * 8, D ** -0.5
    g = torch.Generator().manual_seed(((((B * 131 + H) * 131 + Nq) * 131 + Nk) * 131 + D) * 7 + spike + 1000003 * len(layout))
    Q = 1.5 * torch.randn((B, Nq, C), generator=g)
    Bk = 1 if layout == "shared_kv" else B
    K = 1.5 * torch.randn((Bk, Nk, C), generator=g)
    V = torch.randn((Bk, Nk, C), generator=g)
    if variant == "peaked":
        Q[:, sorted({0, min(17, Nq - 1), Nq // 2, Nq - 1})] *= 6.0
    if variant == "staircase":
        # every query and key of a head along one sign vector u (|u|^2 = D): s' = beta_i alpha_j D c, c = scale log2 e.
        # alpha_j puts key j of tile t at 5 t - (0 .. 3) log2 units for beta = 1; beta within 2 % of 1, so an odd tile tops
        # out at +5.1 above the folded maximum (no rescale, P up to 2^5.1) and an even tile at +10.2 (rescale)
        u = torch.sign(torch.randn((1, 1, C), generator=g))
        beta = 1 + 0.02 * (2 * torch.rand((B, Nq, 1), generator=g) - 1)
        j = torch.arange(Nk)
        target = 5.0 * (j // 64) - 3.0 * torch.rand((Bk, Nk), generator=g)
        target[:, j % 64 == 0] = 5.0 * (j // 64)[j % 64 == 0]                # the first key of a tile is its top
        Q, K = beta * u, (target / (D * scale * LOG2E))[:, :, None] * u
    Q, K, V = Q.half(), K.half(), V.half()
    if spike:
        assert Bk == B
        K[:, spike] = (4.0 * Q[:, spike % Nq].float()).half()
    vmax = float(V.abs().max())
    desc = dict(ldq=C, ldk=C, ldvt=Bk * Nkp, q_bs=Nq * C, k_bs=Nk * C, vt_bs=Nkp, q_off=0, k_off=0, vt_off=0)
    z = 1 if layout == "vt_offset" else 0                                   # skipped leading samples of K and V^T
    vt = _poisoned(C * (Bk + z) * Nkp).view(C, Bk + z, Nkp)
    vt_valid = torch.zeros(vt.shape, dtype=torch.bool)
    vt[:, z:, :Nk] = V.permute(2, 0, 1)
    vt_valid[:, z:, :Nk] = True
    if layout == "fused_qk":
        N = max(Nq, Nk)
        qk = _poisoned(B * N * 2 * C).view(B, N, 2 * C)
        qk_valid = torch.zeros(qk.shape, dtype=torch.bool)
        qk[:, :Nq, :C], qk[:, :Nk, C:] = Q, K
        qk_valid[:, :Nq, :C] = True
        qk_valid[:, :Nk, C:] = True
        q = k = qk.reshape(-1)
        q_valid = k_valid = qk_valid.reshape(-1)
        desc.update(ldq=2 * C, ldk=2 * C, q_bs=N * 2 * C, k_bs=N * 2 * C, k_off=C)
    else:
        q, q_valid = Q.reshape(-1).clone(), torch.ones(B * Nq * C, dtype=torch.bool)
        if layout == "vt_offset":
            kb = _poisoned((B + 1) * Nkp * C).view(B + 1, Nkp, C)
            kv = torch.zeros(kb.shape, dtype=torch.bool)
            kb[1:, :Nk] = K
            kv[1:, :Nk] = True
            k, k_valid = kb.reshape(-1), kv.reshape(-1)
            desc.update(k_bs=Nkp * C, k_off=Nkp * C, ldvt=(B + 1) * Nkp, vt_off=Nkp)
        else:
            k, k_valid = K.reshape(-1).clone(), torch.ones(Bk * Nk * C, dtype=torch.bool)
            if layout == "shared_kv":
                assert B > 1
                desc.update(k_bs=0, vt_bs=0)
            else:
                assert layout == "dense", layout
    return dict(q=q, k=k, vt=vt.reshape(-1), q_valid=q_valid, k_valid=k_valid, vt_valid=vt_valid.reshape(-1), desc=desc,
                scale=scale, vmax=vmax, dims=(B, H, Nq, Nk, D))


def attention_densified(p):
    """the same problem as contiguous [B, Nq, C] / [B, Nk, C] / [C, B, Nk8] operands with the dense descriptor (copies taken
    element by element through the address formulas)"""
    B, H, Nq, Nk, D = p["dims"]
    d = p["desc"]
    C, Nkp = H * D, (Nk + 7) // 8 * 8
    Q, K, V = _attn_views(p["q"], p["k"], p["vt"], B, H, Nq, Nk, D, d["ldq"], d["ldk"], d["ldvt"], d["q_bs"], d["k_bs"], d["vt_bs"],
                          d["q_off"], d["k_off"], d["vt_off"])
    q = Q.permute(0, 2, 1, 3).reshape(-1)
    k = K.permute(0, 2, 1, 3).reshape(-1)
    vt = torch.zeros((C, B, Nkp), dtype=torch.float16)
    vt[:, :, :Nk] = V.permute(1, 3, 0, 2).reshape(C, B, Nk)
    return q, k, vt.reshape(-1), dict(ldq=C, ldk=C, ldvt=B * Nkp, q_bs=Nq * C, k_bs=Nk * C, vt_bs=Nkp)


# ------------------------------------------------------------------------------------------------
# GEMM / convolution (pfd_gemm_f16: csrc/gemm_glds.hip, csrc/gemm_conv.hip): reference, bound, mutants, cases and operands
# (tests/test_gemm_kernels_cpu.py pins and qualifies them, tests/test_gemm_kernels_gpu.py uses them)
# ------------------------------------------------------------------------------------------------
ACT_NONE, ACT_GELU, ACT_RELU, ACT_SILU, ACT_GEGLU = 0, 1, 2, 3, 4          # PFD_ACT_* of include/pfd_hip.h
GEMM_MUTANTS = ("last_k_dropped", "pad_tap_reads_edge", "pad_before_normalise", "tap_crosses_sample", "rowvec_row_by_tile",
                "residual_no_wrap", "residual_wrap_off_by_one", "zero_rows_rounded_to_tile", "bias_after_act",
                "geglu_halves_swapped", "ups_gather_ceil", "k_split_second_source_offset", "ln_mean_of_first_part",
                "tail_transposed_without_bias")
# wrong variants of the documented ARITHMETIC (not of the formula): they act on gemm_ref(..., slabs=, staged=), the model of what
# include/pfd_hip.h says a launch computes, and are qualified by tests/test_gemm_range_cpu.py
GEMM_ARITH_MUTANTS = ("slab_round_toward_zero", "slab_saturates", "residual_added_before_staging")
GEMM_CLASSES = ("lin160", "lin128", "geglu", "reg", "abi", "conv", "patch", "narrow")
# the Lipschitz constants of the activations: max |gelu'| = 1.1290 (at x = 1.4142...), max |silu'| = 1.0998 (at x = 2.3994)
_ACT_LIP = {ACT_NONE: 1.0, ACT_GELU: 1.13, ACT_RELU: 1.0, ACT_SILU: 1.10, ACT_GEGLU: 1.13}


def gemm_conv_operand(img, geom, mutant=None, pad_value=None):
    """the operand matrix of the implicit convolution, from the header text: img [B, H, W, Cin] -> [B Ho Wo, ks ks Cin] with
    m = (b, oy, ox), k = (ky, kx, ci) (tap-major, channel-minor), iy = oy * stride + ky - pad, out-of-range taps read 0 (or
    pad_value [B, Cin]: the pad_before_normalise mutant), ups = 1 gathers iy >> 1 from the image upsampled 2x.
    geom = (ks, stride, pad, ups, Ho, Wo)."""
    ks, stride, pad, ups, Ho, Wo = geom
    B, H, W, C = img.shape
    Hin, Win = (2 * H, 2 * W) if ups else (H, W)
    k = torch.arange(ks)
    iy = torch.arange(Ho)[:, None] * stride + k[None] - pad              # [Ho, ks], coordinates of the (upsampled) image
    ix = torch.arange(Wo)[:, None] * stride + k[None] - pad
    vy, vx = (iy >= 0) & (iy < Hin), (ix >= 0) & (ix < Win)
    if mutant == "pad_tap_reads_edge":
        iy, ix = iy.clamp(0, Hin - 1), ix.clamp(0, Win - 1)
        vy, vx = torch.ones_like(vy), torch.ones_like(vx)
    if ups:
        iy, ix = ((iy + 1) >> 1, (ix + 1) >> 1) if mutant == "ups_gather_ceil" else (iy >> 1, ix >> 1)
    rows = torch.arange(B)[:, None, None] * H + iy[None]                  # [B, Ho, ks]: row of the stacked image [B H, W, C]
    vrow = vy[None].expand(B, Ho, ks)
    if mutant == "tap_crosses_sample" and not ups:
        vrow = (rows >= 0) & (rows < B * H)                               # the row above sample b's first is b - 1's last
    else:
        rows = torch.arange(B)[:, None, None] * H + iy.clamp(0, H - 1)[None]
    g = img.reshape(B * H, W, C)[rows.clamp(0, B * H - 1)]                # [B, Ho, ks, W, C]
    g = g[:, :, :, ix.clamp(0, W - 1)]                                    # [B, Ho, ks, Wo, ks, C]
    ok = (vrow[:, :, :, None, None] & vx[None, None, None]).unsqueeze(-1)
    fill = torch.zeros((), dtype=img.dtype) if pad_value is None else pad_value.to(img.dtype)[:, None, None, None, None, :]
    g = torch.where(ok.to(img.device), g, fill.to(img.device))
    return g.permute(0, 1, 3, 2, 4, 5).reshape(B * Ho * Wo, ks * ks * C)


def geglu_pack(wx, wg, g):
    """rows [x (g rows) | gate (g rows)] per group of g outputs (pfd_gemm_geglu_group: g = 2 wide-tile, g = 32 register-staged);
    works for the [N/2, K] weight halves and, with a trailing dimension of 1 squeezed by the caller, for the bias"""
    n2 = wx.shape[0]
    return torch.cat([wx.reshape(n2 // g, g, -1), wg.reshape(n2 // g, g, -1)], 1).reshape(2 * n2, -1)


def geglu_unpack(w, g):
    n = w.shape[0]
    v = w.reshape(n // (2 * g), 2, g, -1)
    return v[:, 0].reshape(n // 2, -1), v[:, 1].reshape(n // 2, -1)


def w_tiled_pack(w, T):
    """PfdGemmDesc.w_tiled: element (n, k) at (((n / T) * (K / 64) + k / 64) * T + n % T) * 64 + k % 64"""
    N, K = w.shape
    return w.reshape(N // T, T, K // 64, 64).permute(0, 2, 1, 3).contiguous().reshape(N, K)


def gemm_slab_ranges(nk, splits):
    """the K-tile (patch kernels: 64-channel block) ranges of the split-K slabs: slab s covers [s kt, min(nk, (s + 1) kt)),
    kt = ceil(nk / splits); slabs that would start at or beyond nk do not exist (real_splits < splits)"""
    kt = -(-nk // splits)
    return [(s * kt, min(nk, (s + 1) * kt)) for s in range(-(-nk // kt))]


def gemm_slab_columns(c, splits):
    """the K indices of every slab of a launch with `splits` slabs requested: K-tile ranges (gemm_slab_ranges), for the patch
    kernels the 64-channel blocks over all nine taps"""
    if c["cls"] == "patch":
        Cin = c["K"] // 9
        return [torch.cat([torch.arange(t * Cin + lo * 64, t * Cin + hi * 64) for t in range(9)])
                for lo, hi in gemm_slab_ranges(Cin // 64, splits)]
    return [torch.arange(lo * 64, hi * 64) for lo, hi in gemm_slab_ranges(c["K"] // 64, splits)]


F16_MAX, F16_OVERFLOW = 65504.0, 65520.0       # the largest f16; the smallest magnitude that rounds to inf (half an ulp above it)


def _slab_sum(X, W, slabs, mutant):
    """include/pfd_hip.h, PfdGemmDesc.ws: "the K-range partial sums are stored rounded to f16 and summed in fp32, in slab
    order ... a partial sum beyond +-65504 becomes +-inf" -- sum_s f16(P_s) in X's dtype"""
    tot = None
    for i in slabs:
        P = X[:, i] @ W[:, i].t()
        h = P.half()
        if mutant == "slab_round_toward_zero":
            h = torch.where(h.to(P.dtype).abs() > P.abs(), torch.nextafter(h, torch.zeros_like(h)), h)
        elif mutant == "slab_saturates":
            h = P.clamp(-F16_MAX, F16_MAX).half()
        tot = h.to(X.dtype) if tot is None else tot + h.to(X.dtype)
    if len(slabs) % 4:                  # the reductions read four slabs at a time; a last group is filled up with copies of the
        tot = tot + h.to(X.dtype) * 0.0     # LAST slab weighted by 0: nothing, unless that slab is +-inf (inf * 0 = NaN)
    return tot


def ln_out_ref(stored):
    """PfdGemmDesc.ln_out: [M, N / 160, 2] = (sum, sum of squares) over the 160-column slices of the f16 values stored"""
    M, N = stored.shape
    v = stored.double().reshape(M, N // 160, 160)
    return torch.stack([v.sum(-1), (v * v).sum(-1)], -1)


def gn_out_ref(stored):
    """PfdGemmDesc.gn_out: [M / 64, N / 160, 16, 2], slot (n % 160) / (N / 32) of tile n / 160 = (sum, sum of squares) over the
    64 rows of the slab and the N / 32 channels of the group; the slots past 160 / (N / 32) are not written (returned as nan)"""
    M, N = stored.shape
    cpg = N // 32
    v = stored.double().reshape(M // 64, 64, N // 160, 160 // cpg, cpg)
    s = torch.stack([v.sum((1, 4)), (v * v).sum((1, 4))], -1)             # [slab, tile, group, 2]
    out = torch.full((M // 64, N // 160, 16, 2), float("nan"), dtype=torch.float64, device=stored.device)
    out[:, :, :160 // cpg] = s
    return out


def groupnorm32_ref(x, rows, gamma, beta, eps, silu):
    """GroupNorm(32) (+ SiLU) of a token-major [B rows, N] tensor, fp64: statistics per (sample, group of N / 32 channels)"""
    M, N = x.shape
    v = x.double().reshape(M // rows, rows, 32, N // 32)
    mean = v.mean((1, 3), keepdim=True)
    var = (v * v).mean((1, 3), keepdim=True) - mean * mean
    y = ((v - mean) / torch.sqrt(var + eps)).reshape(M, N) * gamma.double() + beta.double()
    return F.silu(y) if silu else y


def _gemm_operand(p, mutant, dtype, want_abs=False):
    """the [M, K] operand of the contraction in `dtype` (rows below zero_rows are zeros) and, for the GroupNorm prologue,
    E [M, K]: how far an operand element can move when the fp32 evaluation of the prologue rounds to the other fp16 neighbour"""
    c = p["case"]
    E = None
    if c["kind"] == "conv":
        x = p["A"]
        if c["gn_pro"] is not None:
            x = torch.cat([p["A"], p["A2"]], -1) if p["A2"] is not None else p["A"]
            tab = p["gn_table"].to(dtype)                                # [B, 2, Cin]
            v = activation_ref(x.to(dtype) * tab[:, None, None, 0] + tab[:, None, None, 1], ACT_SILU if c["gn_pro"][1] else ACT_NONE, dtype)
            padv = None
            if mutant == "pad_before_normalise":
                padv = activation_ref(tab[:, 1], ACT_SILU if c["gn_pro"][1] else ACT_NONE, dtype).half().to(dtype)
            if want_abs:
                d = p["pro_delta"]
                E = gemm_conv_operand(((v + d).half().double() - (v - d).half().double()).abs(), c["geom"])
            X = gemm_conv_operand(v.half().to(dtype), c["geom"], mutant, padv)
        else:
            X = gemm_conv_operand(x.to(dtype), c["geom"], mutant)
    else:
        X = p["A"].to(dtype)
        if p["A2"] is not None:
            a2 = p["A2"].to(dtype)
            if mutant == "k_split_second_source_offset":                   # A2 indexed by k instead of k - k_split
                a2 = a2[:, (torch.arange(a2.shape[1]) + c["k_split"]) % a2.shape[1]]
            X = torch.cat([X, a2], 1)
        zr = c["zero_rows"]
        if zr:
            if mutant == "zero_rows_rounded_to_tile":
                X = X.clone()
                X[:min(-(-zr // 64) * 64, c["M"]) - zr] = 0
            X = torch.cat([X.new_zeros((zr, X.shape[1])), X], 0)
    if mutant == "last_k_dropped":
        X = X.clone()
        X[:, -1] = 0
    return X, E


def gemm_ref(p, mutant=None, dtype=torch.float64, parts=False, slabs=None, staged=False, maxnum_relu=False):
    """one formula, from the header text of PfdGemmDesc, on the fp16 operands of gemm_problem(case), on their device:
        C[m, n] = act(sum_k X[m, k] W[n, k] + bias[n or m] + rowvec[m / rows_per_rv, n]) + R[m (- res_rows), n]
    X the linear operand ([A | A2] with k_split, zero rows in front with zero_rows), the implicit-convolution gather or the
    GroupNorm-prologue image; GEGLU x * gelu(gate) of the two logical halves; the LayerNorm fold as ((x - mean) rstd) W'^T + b'
    with the statistics of x in `dtype`; columns >= n_split transposed (+ bias only).  Returns dict(out=[M, N_out]) plus out_t
    ([N - n_split, M]) with a transposed tail; parts=True adds what gemm_allowance needs.  mutant: one of GEMM_MUTANTS.
    slabs / staged turn the formula into the ARITHMETIC the header documents (gemm_kernel_model): slabs = the K index sets whose
    partial sums pass through f16 (of the raw x W'^T under the LayerNorm fold), staged = act(...) rounded to f16 in front of R;
    mutant may then be one of GEMM_ARITH_MUTANTS."""
    assert mutant is None or mutant in GEMM_MUTANTS or ((slabs is not None or staged) and mutant in GEMM_ARITH_MUTANTS)
    c = p["case"]
    M, N, act = c["M"], c["N"], c["act"]
    X, _ = _gemm_operand(p, mutant, dtype)
    W = p["W"].to(dtype)
    if c["ln"] is not None:
        xs = X[:, :160] if mutant == "ln_mean_of_first_part" else X
        mean = xs.mean(1, keepdim=True)
        rstd = 1.0 / torch.sqrt((xs * xs).mean(1, keepdim=True) - mean * mean + c["ln_eps"])
        if slabs is None:
            X = (X - mean) * rstd
            acc = X @ W.t()
        else:
            acc = rstd * (_slab_sum(X, W, slabs, mutant) - mean * W.sum(1)[None])
    else:
        acc = X @ W.t() if slabs is None else _slab_sum(X, W, slabs, mutant)
    m = torch.arange(M, device=acc.device)
    bias = None if p["bias"] is None else (p["bias"].to(dtype)[:, None] if c["bias_per_row"] else p["bias"].to(dtype)[None, :])
    rv = None
    if p["rowvec"] is not None:
        mi = (m // 64 * 64 if mutant == "rowvec_row_by_tile" else m) // c["rows_per_rv"]
        rv = p["rowvec"].to(dtype)[mi]
    pre = acc
    if bias is not None and mutant != "bias_after_act":
        pre = pre + bias
    if rv is not None:
        pre = pre + rv
    if act == ACT_GEGLU:
        px, pg = pre[:, :N // 2], pre[:, N // 2:]                          # W / bias of the problem are the logical [x | gate]
        if mutant == "geglu_halves_swapped":
            px, pg = pg, px
        post = px * F.gelu(pg)
    else:
        post = activation_ref(pre, act, dtype)
        if maxnum_relu and act == ACT_RELU:                                # fmaxf(v, 0): a NaN gives 0 (torch.relu keeps it)
            post = torch.fmax(pre, torch.zeros_like(pre))
    if bias is not None and mutant == "bias_after_act":
        post = post + (bias[:, :N // 2] if act == ACT_GEGLU else bias)
    out = post
    if p["R"] is not None:
        if staged and mutant != "residual_added_before_staging":
            post = post.half().to(dtype)
        r = p["R"].to(dtype)
        rr = c["res_rows"]
        if rr and rr != M:
            if mutant == "residual_no_wrap":
                r = torch.cat([r, r.new_zeros((M - rr, r.shape[1]))], 0)
            elif mutant == "residual_wrap_off_by_one":
                r = r[torch.where(m >= rr, (m - rr + 1).clamp(max=rr - 1), m)]
            else:
                r = r[torch.where(m >= rr, m - rr, m)]
        out = post + r
    res = {}
    ns = c["n_split"]
    if ns:
        tail = acc[:, ns:] + (bias[:, ns:] if bias is not None and mutant != "tail_transposed_without_bias" else 0)
        res["out_t"] = tail.t().contiguous()
        out = out[:, :ns]
    res["out"] = out
    if parts:
        res.update(X=X, pre=pre, post=post, acc=acc)
    return res


# The GPU bound, per element: |got - ref| <= round_once_bound(ref, a) = 2^-11 (|ref| + a) + a with the allowance a[m, n] =
#   accumulation   c K 2^-24 S,  S = sum_k |x_k| |w_k| + |bias| + |rowvec| (an fp64 abs-GEMM).  The products of two fp16 values are
#                  exact in fp32; a sum of K terms in ANY order is off by at most (K - 1) u sum |terms| (u = 2^-24, first order:
#                  Higham, Accuracy and Stability, 4.2), bias and row vector add two more roundings; c = 2 doubles that because
#                  the order and the rounding inside one MFMA are not documented (nobody has measured that factor: the GPU file
#                  prints the share of `a` each case needs)
#   activation     L times the above (L = the activation's Lipschitz constant, _ACT_LIP) plus the fp32 evaluation error of the
#                  activation itself, fp32_allowance of the reference formula on the pre-activation values; GEGLU x * gelu(g):
#                  the product rule, |gelu(g)| a_x + |x| L a_g (+ the fp32 allowance of the product)
#   split-K        slabs are stored as fp16: sum_s 2^-11 |P_s| in front of the activation, P_s the fp64 partial sum over the
#                  slab's K range (gemm_slab_ranges; the patch kernels split the 64-channel blocks, all nine taps each)
#   staged value   FINDING of this section: the unsplit wide-tile kernels (epilogue_stage / epilogue_store of gemm_glds.hip) round
#                  act(v + bias + rowvec) to fp16 into the LDS image of the tile BEFORE the store pass adds the residual in fp32
#                  and rounds again -- 2^-11 |act(...)| where a residual is present (include/pfd_hip.h says so now).  The
#                  register-staged kernel and the split-K reductions add the residual in fp32 and round once: no such term
#   prologue       the GroupNorm prologue is evaluated in fp32 and rounded to fp16: where the fp64 value lies within the fp32
#                  allowance of a rounding boundary the operand may be the other fp16 neighbour: sum_k E_k |w_k|
#   LayerNorm fold the kernel forms rstd (x W'^T) - rstd mean s_n + b'_n: the two large terms cancel, so their errors count in
#                  full: rstd c K u (sum |x| |W'| + |mean| |s_n|); mean and rstd come in fp32 from the partial sums as
#                  sum / K and rsqrt(sq / K - mean^2 + eps): (P + 3) u relative on mean, the variance off by
#                  (P + 4) u (sq / K + 2 mean^2), rstd by half of that over (var + eps) plus 4 u for rsqrtf; these multiply
#                  |mean| |s_n| rstd and |ref - b'|
#   final          round_once_bound: 2^-11 |ref| (one rounding of the result)
_U = 2.0 ** -24
ACC_C = 2.0


def gemm_allowance(p, splits=1, wide=True):
    """the per-element allowance tensor(s) of one case: dict(out=a [M, N_out], out_t=...) for round_once_bound / bound_ratio.
    splits: the slab count of the launch (1 = unsplit); wide: a wide-tile kernel (the staged-value term applies)."""
    c = p["case"]
    M, N, K, act = c["M"], c["N"], c["K"], c["act"]
    r = gemm_ref(p, parts=True)
    Xraw, E = _gemm_operand(p, None, torch.float64, want_abs=True)
    W = p["W"].double()
    S = Xraw.abs() @ W.abs().t()
    extra = torch.zeros_like(S)
    if E is not None:
        extra = extra + E @ W.abs().t()
    if c["ln"] is not None:
        P, ns_ = K // 160, (160 if c["ln"] == "rowstats" else 0)          # ns_: values summed in fp32 per partial sum
        mean = Xraw.mean(1, keepdim=True)
        mabs = Xraw.abs().mean(1, keepdim=True)
        msq = (Xraw * Xraw).mean(1, keepdim=True)
        var = msq - mean * mean
        rstd = 1.0 / torch.sqrt(var + c["ln_eps"])
        s_n = W.sum(1)[None]
        d_mean = (P + 3) * _U * mean.abs() + ns_ * _U * mabs
        d_var = (P + 4) * _U * (msq + 2 * mean * mean) + ns_ * _U * (msq + 2 * mean.abs() * mabs)
        d_rstd_rel = 0.5 * d_var / (var + c["ln_eps"]) + 4 * _U
        # ref - b' = rstd (x W'^T - mean s_n) = r["acc"]: rstd is one factor of it (d_rstd_rel relative), the accumulation and
        # the product mean s_n count in full, mean's error is scaled by rstd |s_n| (s_n itself is fp32: one more u)
        a_acc = rstd * ACC_C * K * _U * (S + mean.abs() * s_n.abs()) + rstd * s_n.abs() * (d_mean + _U * mean.abs()) \
            + d_rstd_rel * r["acc"].abs()
    else:
        rstd = 1.0
        a_acc = ACC_C * K * _U * S
    S_b = torch.zeros_like(S)
    if p["bias"] is not None:
        b = p["bias"].double().abs()
        S_b = S_b + (b[:, None] if c["bias_per_row"] else b[None, :])
    if p["rowvec"] is not None:
        S_b = S_b + p["rowvec"].double().abs()[torch.arange(M) // c["rows_per_rv"]]
    a_pre = a_acc + ACC_C * K * _U * S_b + extra
    if splits > 1:
        rng = gemm_slab_columns(c, splits)
        # (the slabs hold partial sums of x W'^T: the LayerNorm fold is applied behind the reduction, which scales them by rstd)
        a_pre = a_pre + sum(2.0 ** -11 * (Xraw[:, i] @ W[:, i].t()).abs() for i in rng) * rstd
    res = {}
    ns = c["n_split"]
    if ns:
        res["out_t"] = a_pre[:, ns:].t().contiguous()
    pre = r["pre"]
    if act == ACT_GEGLU:
        px, pg = pre[:, :N // 2], pre[:, N // 2:]
        ax, ag = a_pre[:, :N // 2], a_pre[:, N // 2:]
        e_act = fp32_allowance(F.gelu(pg), F.gelu(pg.float()))
        a = F.gelu(pg).abs() * ax + px.abs() * (_ACT_LIP[act] * ag + e_act) + ax * (_ACT_LIP[act] * ag + e_act) \
            + 4 * _U * r["post"].abs()
    elif act == ACT_NONE:
        a = a_pre
    else:
        a = _ACT_LIP[act] * a_pre + fp32_allowance(r["post"], activation_ref(pre.float(), act, torch.float32))
    if wide and splits == 1 and p["R"] is not None:
        a = a + 2.0 ** -11 * (r["post"].abs() + a)                        # the staged value (see above)
    res["out"] = a[:, :ns] if ns else a
    return res


def gemm_kernel_model(p, splits=1, wide=True, mutant=None, dtype=torch.float32):
    """the ARITHMETIC include/pfd_hip.h documents for a launch with `splits` slabs, evaluated by torch in fp32 on the CPU and
    rounded to f16: epi(sum_s f16(P_s)) with per-range fp32 contractions, the slabs summed in order, the epilogue in fp32, act(...)
    staged as f16 in front of a residual on the unsplit wide-tile kernels.  IEEE all the way: a slab beyond +-65504 is +-inf,
    inf - inf NaN, silu / gelu of -inf NaN, and a last slab of +-inf gives NaN whenever the slab count is no multiple of four (the
    zero-weighted copies of _slab_sum; FINDING of the range tests, stated in the header now).  RELU is fmaxf(v, 0) -- IEEE maxNum, the instruction the kernels use: relu(-inf) = 0
    and relu(NaN) = 0, where torch.relu keeps the NaN.  mutant: one of GEMM_ARITH_MUTANTS."""
    c = p["case"]
    r = gemm_ref(p, mutant=mutant, dtype=dtype, slabs=gemm_slab_columns(c, splits) if splits > 1 else None,
                 staged=wide and splits == 1, maxnum_relu=True)
    return {k: r[k].half() for k in ("out", "out_t") if k in r}


def gemm_slab_partials(p, splits):
    """[(P_s, d_s)] in fp64 for every slab of a launch with `splits` slabs (one entry, the whole K, unsplit): the partial sum
    of the raw operand and its own accumulation allowance ACC_C K_s u sum_k |x_k| |w_k| over the slab"""
    c = p["case"]
    X, _ = _gemm_operand(p, None, torch.float64)
    W = p["W"].double()
    cols = gemm_slab_columns(c, splits) if splits > 1 else [torch.arange(c["K"])]
    return [(X[:, i] @ W[:, i].t(), ACC_C * len(i) * _U * (X[:, i].abs() @ W[:, i].abs().t())) for i in cols]


def gemm_range_classes(p, splits, wide):
    """per element of the main output, from the fp64 reference alone: 0 `finite` -- every quantity the header says passes
    through f16 (the slab partials; act(...) on an unsplit wide-tile launch with a residual) lies below 65520 - d, d its own
    accumulation allowance; 1 `nonfinite` -- some quantity lies beyond 65520 + d and none in between; 2 `band` -- otherwise (which
    way such a quantity rounds is not determined by the reference: left out)"""
    c = p["case"]
    q = gemm_slab_partials(p, splits) if splits > 1 else []
    if wide and splits == 1 and p["R"] is not None:
        a = gemm_allowance(p, 1, False)["out"]
        q.append((gemm_ref(p, parts=True)["post"], a))
    cls = torch.zeros((c["M"], c["N"]), dtype=torch.int64)
    for P, d in q:
        cls = torch.maximum(cls, torch.where(P.abs() > F16_OVERFLOW + d, 1, torch.where(P.abs() < F16_OVERFLOW - d, 0, 2)))
    n_out = c["n_split"] or (c["N"] // 2 if c["act"] == ACT_GEGLU else c["N"])
    assert n_out == c["N"]
    return cls


def half_pipeline(p):
    """the same operation the way the model this library ports computes it in fp16 (torch modules on f16 tensors): each GEMM
    accumulates the WHOLE K in fp32 and rounds its result (+ bias) to f16 once, and every op around it -- LayerNorm / GroupNorm
    in front, the row-vector add, the activation, the GEGLU product, the residual add -- is a separate op that reads f16 and
    rounds to f16.  Not a bound on anything: the yardstick the f16-slab loss is recorded against."""
    c = p["case"]
    M, N, act = c["M"], c["N"], c["act"]
    h = lambda t: t.half().float()
    X, _ = _gemm_operand(p, None, torch.float32)
    if c["ln"] is not None:
        X = h(F.layer_norm(X, (c["K"],), None, None, c["ln_eps"]))
    y = X @ p["W"].float().t()
    if p["bias"] is not None:
        y = y + (p["bias"].float()[:, None] if c["bias_per_row"] else p["bias"].float()[None])
    y = h(y)
    res = {}
    if c["n_split"]:
        res["out_t"] = y[:, c["n_split"]:].t().contiguous().half()
    if p["rowvec"] is not None:
        y = h(y + p["rowvec"].float()[torch.arange(M) // c["rows_per_rv"]])
    if act == ACT_GEGLU:
        y = h(y[:, :N // 2] * h(F.gelu(y[:, N // 2:])))
    else:
        y = h(activation_ref(y, act, torch.float32))
    if p["R"] is not None:
        r, rr = p["R"].float(), c["res_rows"]
        m = torch.arange(M)
        y = h(y + (r[torch.where(m >= rr, m - rr, m)] if rr and rr != M else r))
    res["out"] = (y[:, :c["n_split"]] if c["n_split"] else y).half()
    return res


def _embed(data, rows_before, rows_after, c0, width, poison):
    """`data` [rows, cols] as rows [rows_before, +rows) and columns [c0, +cols) of a buffer that holds the fp16 NaN patterns
    of _POISON (or zeros) everywhere else; returns the buffer"""
    rows, cols = data.shape
    n = (rows_before + rows + rows_after) * width
    buf = (_poisoned(n) if poison else torch.zeros(n, dtype=torch.float16)).view(-1, width)
    buf[rows_before:rows_before + rows, c0:c0 + cols] = data
    return buf


# ---- cases: one table; every entry names the forced tile code (0 = the heuristic) and the kernel instantiation it is meant to
# reach, in the spelling of `emu_gemm --dispatch` (tests/test_gemm_kernels_cpu.py checks both against the dispatcher) ----
def wide_tile(v, s=0):
    """tile code of pfd_gemm_f16_ex: wide-tile variant v with split-K factor s (0 = heuristic for either)"""
    return 1000 + 100 * v + s


def wide_kernel_name(v, conv, nt):
    """the instantiation behind a forced wide-tile variant (the variant switches at the end of pfd_gemm160_try, restated)"""
    b = "true" if conv else "false"
    g160 = {22: (2, 2, 2), 23: (2, 2, 4), 24: (2, 4, 2), 25: (2, 4, 3), 41: (4, 1, 2), 43: (4, 1, 4), 82: (4, 2, 2), 83: (4, 2, 3),
            44: (4, 4, 2)}
    if v in g160:
        wm, wmb, nbuf = g160[v]
        return f"gemm160_kernel<{wm}, {wmb}, {b}, {nbuf}, {nt}>"
    if v == 84:
        return "gemm160_kernel<4, 4, false, 2, 10>"
    if v in (47, 48):
        return f"gemm160ws_kernel<{b}, {nt}, {3 if v == 47 else 2}, false>"
    return {96: "conv3x3_patch_ws_kernel<0, 3>", 98: "conv3x3_patch_ws_kernel<0, 2>", 99: "conv3x3_patch_kernel"}[v]


_GEMM_DEFAULTS = dict(kind="lin", act=ACT_NONE, bias=False, rowvec=False, rows_per_rv=1, res=False, bias_per_row=False, geom=None,
                      image=None, k_split=0, zero_rows=0, res_rows=0, n_split=0, ln=None, ln_eps=1e-5, ln_out=False, gn_out=False,
                      w_tiled=False, gn_pro=None, gnf=None, splits=1, reduce=None, tile=0, base_kernel=None, ldc_pad=16,
                      operands="unit")
EPI_NONE = dict()
EPI_FULL = dict(bias=True, act=ACT_SILU, rowvec=True, rows_per_rv=100, res=True)
EPI_GELU = dict(bias=True, act=ACT_GELU)
EPI_RELU = dict(act=ACT_RELU)
EPI_RES = dict(res=True)
EPI_RV_RES = dict(bias=True, rowvec=True, rows_per_rv=100, res=True)
_EPI_NAMES = ((EPI_NONE, "plain"), (EPI_FULL, "silu-rv-res"), (EPI_GELU, "gelu"), (EPI_RELU, "relu"), (EPI_RES, "res"), (EPI_RV_RES, "rv-res"))


def _epi_name(e):
    return next(n for d, n in _EPI_NAMES if d is e)


def _mk(cid, cls, kernel, M, N, K, **kw):
    c = dict(_GEMM_DEFAULTS, id=cid, cls=cls, kernel=kernel, M=M, N=N, K=K)
    assert not set(kw) - set(c), set(kw) - set(c)
    c.update(kw)
    return c


def _wide(cid, cls, v, s, M, N, K, conv=False, **kw):
    """a case under the forced wide-tile variant v (0: heuristic; `kernel=` then names what the heuristic takes) and split s"""
    nt = 5 if N % 160 == 0 else 4
    kernel = kw.pop("kernel", None) or wide_kernel_name(v, conv, nt)
    nk = K // 64 if cls != "patch" else K // 9 // 64
    s_eff = s or kw.get("hsplit", 0)            # hsplit: the split count the heuristic takes where the case forces none
    kw.pop("hsplit", None)
    splits = len(gemm_slab_ranges(nk, s_eff)) if s_eff > 1 else 1
    if splits > 1 and "reduce" not in kw:
        kw["reduce"] = "splitk_reduce_gn_kernel" if kw.get("gn_out") else "splitk_reduce_gnorm_kernel" if kw.get("gnf") is not None \
            else "splitk_reduce_kernel"
    return _mk(cid, cls, kernel, M, N, K, tile=wide_tile(v, s) if (v or s) else 0, splits=splits, **kw)


def _conv_geom(B, H, W, Cin, ks=3, stride=1, pad=1, ups=0, out_hw=None):
    Hin, Win = (2 * H, 2 * W) if ups else (H, W)
    Ho, Wo = out_hw or ((Hin + 2 * pad - ks) // stride + 1, (Win + 2 * pad - ks) // stride + 1)
    return dict(kind="conv", image=(B, H, W, Cin), geom=(ks, stride, pad, ups, Ho, Wo)), B * Ho * Wo, ks * ks * Cin, Ho * Wo


def _build_gemm_cases():
    cs = []
    # what the heuristic takes below: 64-row tiles on eight waves (four at 128 columns), the 4-stage ring from 8 K tiles on
    H41, H43, H22 = "gemm160_kernel<4, 1, false, 2, 5>", "gemm160_kernel<4, 1, false, 4, 5>", "gemm160_kernel<2, 2, false, 2, 4>"
    # linear, 160-wide: M = 300 leaves a ragged last tile for every tile height, K = 64 / 128 fewer K tiles than ring stages
    for v in (22, 23, 24, 25, 41, 43, 44, 82, 83, 48, 47, 0):
        for (M, N, K) in ((1, 160, 64), (77, 160, 128), (300, 320, 320)):
            for e in ((EPI_FULL,) if M != 300 else (EPI_NONE, EPI_FULL, EPI_GELU, EPI_RELU)):
                cs.append(_wide(f"lin160-v{v}-{M}x{N}x{K}-{_epi_name(e)}", "lin160", v, 0, M, N, K, kernel=H41 if v == 0 else None, **e))
    for s in (2, 4, 8):                                  # five K tiles: 3 + 2, 2 + 2 + 1, 1 x 5 (real_splits < splits)
        for v, e in ((44, EPI_FULL), (41, EPI_NONE), (25, EPI_FULL), (0, EPI_GELU)):
            cs.append(_wide(f"lin160-v{v}-split{s}-300x320x320-{_epi_name(e)}", "lin160", v, s, 300, 320, 320,
                            kernel=H41 if v == 0 else None, **e))
    # GEGLU: pairs (g = 2) on the wide-tile kernels, groups of 32 on the register-staged one
    for v in (84, 44, 24, 22, 0):
        cs.append(_wide(f"geglu-v{v}-300x640x320", "geglu", v, 0, 300, 640, 320, act=ACT_GEGLU, bias=True, kernel=H41 if v == 0 else None))
    cs.append(_mk("geglu-reg-300x256x320", "geglu", "gemm_conv_kernel<2, 2, false>", 300, 256, 320, act=ACT_GEGLU, bias=True))
    # 128-wide
    for v in (44, 24, 22, 48, 47):
        for (N, K) in ((256, 128), (384, 512)):
            cs.append(_wide(f"lin128-v{v}-300x{N}x{K}-silu-rv-res", "lin128", v, 0, 300, N, K, **EPI_FULL))
    cs.append(_wide("lin128-v0-300x384x128-plain", "lin128", 0, 0, 300, 384, 128, kernel=H22))
    cs.append(_wide("lin128-v22-split2-300x256x512-gelu", "lin128", 22, 2, 300, 256, 512, **EPI_GELU))
    # register-staged: ragged M and N, bias per row, all four activations
    for t, (tm, tn) in ((22, (2, 2)), (21, (2, 1)), (12, (1, 2)), (11, (1, 1))):
        k = f"gemm_conv_kernel<{tm}, {tn}, false>"
        for e, extra in ((EPI_FULL, {}), ({22: EPI_NONE, 21: EPI_GELU, 12: EPI_RELU, 11: EPI_NONE}[t], dict(bias=True, bias_per_row=True))):
            cs.append(_mk(f"reg-t{t}-301x200x192-{_epi_name(e)}{'-bias-per-row' if extra else ''}", "reg", k, 301, 200, 192, tile=t,
                          **{**e, **extra}))
    # ldc = N + 12 is no multiple of 8: the scalar store path of the register-staged kernel (every other case takes the 16-byte one)
    cs.append(_mk("reg-t11-301x200x192-silu-rv-res-ldc212", "reg", "gemm_conv_kernel<1, 1, false>", 301, 200, 192, tile=11, ldc_pad=12,
                  **EPI_FULL))
    cs.append(_mk("reg-t0-301x200x192-silu-rv-res", "reg", "gemm_conv_kernel<1, 1, false>", 301, 200, 192, **EPI_FULL))
    # ABI fields (linear)
    for v in (0, 44, 22):
        kn = dict(kernel=H41) if v == 0 else {}
        cs.append(_wide(f"abi-ksplit64+64-v{v}", "abi", v, 0, 300, 320, 128, k_split=64, bias=True, **kn))
        cs.append(_wide(f"abi-ksplit64+256-v{v}", "abi", v, 0, 300, 320, 320, k_split=64, **EPI_FULL, **kn))
        cs.append(_wide(f"abi-zero100-v{v}", "abi", v, 0, 300, 320, 320, zero_rows=100, **EPI_FULL, **kn))
        cs.append(_wide(f"abi-zero256-v{v}", "abi", v, 0, 300, 320, 320, zero_rows=256, **EPI_FULL, **kn))
        cs.append(_wide(f"abi-res150-v{v}", "abi", v, 0, 300, 320, 320, res_rows=150, **EPI_FULL, **kn))
        cs.append(_wide(f"abi-tail480-v{v}", "abi", v, 0, 200, 480, 128, n_split=320, bias=True, **kn))
        cs.append(_wide(f"abi-tail384-v{v}", "abi", v, 0, 200, 384, 128, n_split=256, bias=True, **(dict(kernel=H22) if v == 0 else {})))
    cs.append(_wide("abi-res150-zero150-split2", "abi", 24, 2, 300, 320, 320, res_rows=150, zero_rows=150, **EPI_FULL))
    cs.append(_wide("abi-zero100-split2", "abi", 41, 2, 300, 320, 320, zero_rows=100, **EPI_FULL))
    cs.append(_wide("abi-ksplit64+256-split4", "abi", 22, 4, 300, 320, 320, k_split=64, **EPI_FULL))
    # LayerNorm fold (M = 77): statistics from fp64 sums rounded to fp32 ("f64"), from ops.ln_rowstats ("rowstats"), and with 4
    # added to the row mean of x ("shifted": the two large terms cancel)
    for K in (320, 640):
        for v in (0, 44, 25):
            kn = dict(kernel=H41 if K == 320 else H43) if v == 0 else {}
            cs.append(_wide(f"abi-ln{K}-v{v}-plain", "abi", v, 0, 77, 320, K, ln="f64", bias=True, **kn))
            cs.append(_wide(f"abi-ln{K}-v{v}-geglu", "abi", v, 0, 77, 640, K, ln="f64", bias=True, act=ACT_GEGLU, **kn))
        cs.append(_wide(f"abi-ln{K}-tail", "abi", 0, 0, 77, 480, K, ln="f64", bias=True, n_split=320, kernel=H41 if K == 320 else H43))
        cs.append(_wide(f"abi-ln{K}-ln_out", "abi", 0, 0, 77, 320, K, ln="f64", bias=True, ln_out=True, kernel=H41 if K == 320 else H43))
        cs.append(_wide(f"abi-ln{K}-shifted", "abi", 24, 0, 77, 320, K, ln="shifted", bias=True))
    cs.append(_wide("abi-ln320-rowstats", "abi", 0, 0, 77, 320, 320, ln="rowstats", bias=True, kernel=H41))
    cs.append(_wide("abi-ln640-split2", "abi", 22, 2, 77, 320, 640, ln="f64", bias=True, act=ACT_GELU))
    # side outputs
    for N in (320, 640):
        for s in (0, 2):
            cs.append(_wide(f"abi-ln_out-128x{N}x320-split{s}", "abi", 44 if s else 0, s, 128, N, 320, ln_out=True, bias=True, res=True,
                            kernel=None if s else H41))
            cs.append(_wide(f"abi-gn_out-128x{N}x320-split{s}", "abi", 24 if s else 0, s, 128, N, 320, gn_out=True, bias=True, res=True,
                            kernel=None if s else H41))
    cs.append(_wide("abi-wtiled-300x320x320", "abi", 0, 0, 300, 320, 320, w_tiled=True, kernel=H41, **EPI_FULL))
    cs.append(_wide("abi-wtiled-300x256x128", "abi", 0, 0, 300, 256, 128, w_tiled=True, kernel=H22, **EPI_FULL))
    # implicit convolution (B = 2, N = 160)
    conv_epi = dict(bias=True, act=ACT_SILU, rowvec=True, res=True)
    geoms = (("s2p1-10x8", dict(H=10, W=8, stride=2)), ("s1p1-9x7", dict(H=9, W=7)), ("ups-5x6", dict(H=5, W=6, ups=1)),
             ("s2p0-outhw-10x8", dict(H=10, W=8, stride=2, pad=0, out_hw=(5, 4))))
    for v in (22, 24, 44, 41, 43, 82, 83, 23, 25, 48, 47, 0):
        for Cin in (64, 128):                                # 128: two channel blocks per tap, a K tile is not a whole tap
            for gname, g in geoms:
                geo, M, K, hw = _conv_geom(2, g["H"], g["W"], Cin, 3, g.get("stride", 1), g.get("pad", 1), g.get("ups", 0), g.get("out_hw"))
                # (the heuristic: 4-stage ring at nine K tiles; at 18 every 64-row tile form -- forced or not -- splits four ways,
                #  5 + 5 + 5 + 3, and the heuristic keeps the ring for the stride-2 forms only)
                hk = "gemm160_kernel<4, 1, true, 2, 5>" if Cin == 128 and g.get("stride", 1) == 1 else "gemm160_kernel<4, 1, true, 4, 5>"
                cs.append(_wide(f"conv-v{v}-c{Cin}-{gname}", "conv", v, 0, M, 160, K, conv=True, rows_per_rv=hw, kernel=hk if v == 0 else None,
                                hsplit=4 if Cin == 128 and v in (0, 22, 23, 41, 43) else 0, **conv_epi, **geo))
    for v in (22, 24, 44, 48, 47):                       # the same on 128-wide tiles (the VAE's convolutions)
        for gname, g in geoms[:2]:
            geo, M, K, hw = _conv_geom(2, g["H"], g["W"], 64, 3, g.get("stride", 1))
            cs.append(_wide(f"conv-n128-v{v}-c64-{gname}", "conv", v, 0, M, 128, K, conv=True, rows_per_rv=hw, **conv_epi, **geo))
    # the 3x3 patch kernel: whole-row tiles, pixel tiles (pt_w 32 / 16), the two-block split of Cin = 192
    for v in (99, 98, 96, 0):
        for Cin in (128, 192):
            for (B, H, W) in ((2, 16, 16), (1, 8, 32), (1, 4, 64), (1, 8, 96), (1, 16, 48)):
                geo, M, K, hw = _conv_geom(B, H, W, Cin)
                for s in ((0, 2) if Cin == 192 else (0,)):
                    cs.append(_wide(f"patch-v{v}-c{Cin}-{B}x{H}x{W}" + (f"-split{s}" if s else ""), "patch", v, s, M, 160, K, conv=True,
                                    rows_per_rv=hw, kernel="conv3x3_patch_ws_kernel<0, 3>" if v == 0 else None, **conv_epi, **geo))
    for two in (False, True):
        for silu in (False, True):
            geo, M, K, hw = _conv_geom(1, 8, 32, 128)
            cs.append(_wide(f"patch-prologue-{'64+64' if two else '128'}{'-silu' if silu else ''}", "patch", 0, 0, M, 160, K, conv=True,
                            rows_per_rv=hw, gn_pro=(64 if two else 128, silu), kernel=f"conv3x3_patch_ws_kernel<{2 if silu else 1}, 2>", base_kernel="conv3x3_patch_ws_kernel<0, 3>",
                            **conv_epi, **geo))
    for keep in (True, False):
        geo, M, K, hw = _conv_geom(4, 16, 16, 128)
        cs.append(_wide(f"patch-gnf-{'raw-kept' if keep else 'raw-skipped'}", "patch", 0, 2, M, 640, K, conv=True, rows_per_rv=hw, gnf=keep,
                        bias=True, rowvec=True, res=keep, kernel="conv3x3_patch_ws_kernel<0, 3>", **geo))
    geo, M, K, hw = _conv_geom(2, 16, 16, 128)
    cs.append(_wide("patch-wtiled-c128-2x16x16", "patch", 0, 0, M, 160, K, conv=True, rows_per_rv=hw, w_tiled=True,
                    kernel="conv3x3_patch_ws_kernel<0, 3>", **conv_epi, **geo))
    # narrow convolution (N <= 16): 64-pixel segments of an image row
    for N in (4, 3):
        for (B, H, W) in ((2, 9, 7), (1, 3, 70)):
            geo, M, K, hw = _conv_geom(B, H, W, 64)
            cs.append(_mk(f"narrow-n{N}-{B}x{H}x{W}", "narrow", "conv3x3_narrow_kernel", M, N, K, bias=True, rows_per_rv=hw, **geo))
    assert len({c["id"] for c in cs}) == len(cs)
    return cs + _operand_kind_cases({c["id"]: c for c in cs})


def _kinded(c, kind):
    """the same launch on other operands (field `operands`: the case field `kind` already says linear / convolution): the kind
    is part of the id, hence of gemm_problem_key -- the variants and split counts of one problem still share their operands"""
    return dict(c, id=f"{c['id']}-k{kind}", operands=kind)


def _operand_kind_cases(base):
    """the launches of the table that also run on trained magnitudes (`act`), on partial sums that cancel between the slabs of
    split count S (`cancelS`) and on the same construction from small integers (`exactS`); see gemm_problem for the recipes.
    Shapes, variants and split counts are those of the unit cases (the 24-integer records do not change with the kind)."""
    H41 = "gemm160_kernel<4, 1, false, 2, 5>"
    cs = []
    lin = "300x320x320"
    for s in (0, 2, 4, 8):
        sp = f"-split{s}" if s else ""
        for v, e in ((44, EPI_FULL), (41, EPI_NONE), (25, EPI_FULL), (0, EPI_GELU)):
            b = base[f"lin160-v{v}{sp}-{lin}-{_epi_name(e)}"]
            cs +=[_kinded(b, "act"), _kinded(b, "cancel2")]
        for v, e in ((41, EPI_NONE), (44, EPI_RES), (0, EPI_RELU)):
            b = base.get(f"lin160-v{v}{sp}-{lin}-{_epi_name(e)}") or \
                _wide(f"lin160-v{v}{sp}-{lin}-{_epi_name(e)}", "lin160", v, s, 300, 320, 320, kernel=H41 if v == 0 else None, **e)
            cs.append(_kinded(b, "exact2"))
    for b in (_wide("lin128-v22-300x256x512-gelu", "lin128", 22, 0, 300, 256, 512, **EPI_GELU), base["lin128-v22-split2-300x256x512-gelu"]):
        cs += [_kinded(b, "act"), _kinded(b, "cancel2")]
    act_only = ["geglu-v84-300x640x320", "geglu-v44-300x640x320", "geglu-v0-300x640x320", "geglu-reg-300x256x320",
                "reg-t22-301x200x192-silu-rv-res", "reg-t11-301x200x192-silu-rv-res", "reg-t11-301x200x192-silu-rv-res-ldc212",
                "abi-ln640-v0-plain", "abi-ln640-split2", "abi-ln320-rowstats"]
    act_only += [f"abi-{o}-128x{N}x320-split{s}" for N in (320, 640) for s in (0, 2) for o in ("ln_out", "gn_out")]
    for g in ("s1p1-9x7", "s2p1-10x8"):      # 18 K tiles: v0 and v22 split four ways (5 + 5 + 5 + 3), v44 does not
        for v in (0, 22, 44):
            cs += [_kinded(base[f"conv-v{v}-c128-{g}"], "act"), _kinded(base[f"conv-v{v}-c128-{g}"], "cancel4")]
    for v in (96, 0):
        for img in ("2x16x16", "1x8x32"):
            for sp in ("", "-split2"):
                cs += [_kinded(base[f"patch-v{v}-c192-{img}{sp}"], "act"), _kinded(base[f"patch-v{v}-c192-{img}{sp}"], "cancel2")]
    act_only += [f"patch-prologue-{a}{b}" for a in ("128", "64+64") for b in ("", "-silu")]
    act_only += ["patch-gnf-raw-kept", "patch-gnf-raw-skipped", "narrow-n4-2x9x7"]
    cs += [_kinded(base[i], "act") for i in act_only]
    assert len({c["id"] for c in cs}) == len(cs)
    return cs


def _build_gemm_range_cases():
    """beyond the f16 range (tests/test_gemm_range_cpu.py / _gpu.py; the runner of GEMM_CASES asserts finiteness, so these have
    a table of their own): `overflowS` = the cancelS operands times 2 -- some slab partials leave the range while the result
    stays O(1e3) -- split and, beside it, unsplit; `staged` = a large bias + row vector against a residual of the opposite
    sign -- act(...) leaves the range, the result does not"""
    cs = []
    for e in (EPI_NONE, EPI_FULL, EPI_RELU):
        cs.append(_wide(f"range-lin160-v41-split2-300x320x320-{_epi_name(e)}", "lin160", 41, 2, 300, 320, 320, **e))
        cs.append(_wide(f"range-lin160-v44-300x320x320-{_epi_name(e)}", "lin160", 44, 0, 300, 320, 320, **e))
    cs.append(_wide("range-gn_out-v24-split2-128x320x320", "abi", 24, 2, 128, 320, 320, gn_out=True, bias=True, res=True))
    cs.append(_wide("range-gn_out-v44-128x320x320", "abi", 44, 0, 128, 320, 320, gn_out=True, bias=True, res=True))
    conv_epi = dict(bias=True, act=ACT_SILU, rowvec=True, res=True)
    geo, M, K, hw = _conv_geom(2, 16, 16, 192)
    for v, s in ((96, 2), (96, 0)):
        cs.append(_wide(f"range-patch-v{v}-c192-2x16x16" + (f"-split{s}" if s else ""), "patch", v, s, M, 160, K, conv=True, rows_per_rv=hw,
                        **conv_epi, **geo))
    cs = [_kinded(c, "overflow2") for c in cs]
    geo, M, K, hw = _conv_geom(2, 9, 7, 128)
    cs.append(_kinded(_wide("range-conv-v0-c128-s1p1-9x7", "conv", 0, 0, M, 160, K, conv=True, rows_per_rv=hw, hsplit=4,
                            kernel="gemm160_kernel<4, 1, true, 2, 5>", **conv_epi, **geo), "overflow4"))
    cs.append(_kinded(_wide("range-conv-v44-c128-s1p1-9x7", "conv", 44, 0, M, 160, K, conv=True, rows_per_rv=hw, **conv_epi, **geo), "overflow4"))
    for v in (22, 41, 44, 83):
        cs.append(_kinded(_wide(f"range-lin160-v{v}-300x320x320-rv-res", "lin160", v, 0, 300, 320, 320, **EPI_RV_RES), "staged"))
    cs.append(_kinded(_wide("range-lin160-v41-split2-300x320x320-rv-res", "lin160", 41, 2, 300, 320, 320, **EPI_RV_RES), "staged"))
    cs.append(_kinded(_mk("range-reg-t22-301x200x192-rv-res", "reg", "gemm_conv_kernel<2, 2, false>", 301, 200, 192, tile=22, **EPI_RV_RES), "staged"))
    assert len({c["id"] for c in cs}) == len(cs)
    return cs


GEMM_CASES = _build_gemm_cases()
GEMM_RANGE_CASES = _build_gemm_range_cases()
GEMM_CASE = {c["id"]: c for c in GEMM_CASES + GEMM_RANGE_CASES}


def gemm_case_record(c):
    """the 24 integers of lib.hip.ops.TRACE_FIELDS a launch of the case leaves (what a record cannot express -- LayerNorm fold,
    transposed tail, prologue, tiled weights, ln_out -- is left out: the base record)"""
    B, H, W, Cin = c["image"] or (0, 0, 0, 0)
    ks, stride, pad, ups, Ho, Wo = c["geom"] or (0, 0, 0, 0, 0, 0)
    gnf = 0 if c["gnf"] is None else 1 if c["gnf"] else 2
    return (c["M"], c["N"], c["K"], c["act"], int(c["bias"]), int(c["rowvec"]), int(c["res"]), int(c["bias_per_row"]), ks, stride, pad,
            ups, B, H, W, Cin, Ho, Wo, c["rows_per_rv"], c["k_split"], c["zero_rows"], int(c["gn_out"]), gnf, c["res_rows"])


def _put_input(p, x, rn):
    """the input x (image [B, H, W, Cin] or rows [M - zero_rows, K], fp32) as the fp16 A / A2 of the case; with a GroupNorm
    prologue also its table and how far the fp32 evaluation of the prologue can be off"""
    c = p["case"]
    if c["kind"] == "conv":
        B, H, W, Cin = c["image"]
        c1 = c["gn_pro"][0] if c["gn_pro"] is not None else Cin
        p["A"] = x[..., :c1].half()
        if c1 < Cin:
            p["A2"] = x[..., c1:].half()
        if c["gn_pro"] is not None:      # GroupNorm(32) table of the concat in fp64, rounded to fp32: scale = rstd gamma, shift = beta - mean scale
            xc = x.half().double().reshape(B, H * W, 32, Cin // 32)
            mean = xc.mean((1, 3), keepdim=True)
            rstd = 1.0 / torch.sqrt((xc * xc).mean((1, 3), keepdim=True) - mean * mean + 1e-5)
            gamma, beta = (1 + 0.2 * rn(Cin)).double().reshape(32, -1), (0.1 * rn(Cin)).double().reshape(32, -1)
            scale = (rstd[:, 0] * gamma).reshape(B, Cin)
            shift = (beta - mean[:, 0] * rstd[:, 0] * gamma).reshape(B, Cin)
            p["gn_table"] = torch.stack([scale, shift], 1).float()
            act = ACT_SILU if c["gn_pro"][1] else ACT_NONE
            xx, tab = x.half(), p["gn_table"]
            v64 = activation_ref(xx.double() * tab[:, None, None, 0].double() + tab[:, None, None, 1].double(), act, torch.float64)
            v32 = activation_ref(xx.float() * tab[:, None, None, 0] + tab[:, None, None, 1], act, torch.float32)
            p["pro_delta"] = fp32_allowance(v64, v32)
    else:
        ks_ = c["k_split"] or c["K"]
        p["A"] = x[:, :ks_].half()
        if c["k_split"]:
            p["A2"] = x[:, ks_:].half()


def gemm_operand_kind(c):
    """the case's `operands` as (family, S): ("cancel", 2) for cancel2, ("act", 0), ("unit", 0), ..."""
    m = re.fullmatch(r"([a-z]+?)(\d*)", c["operands"])
    return m.group(1), int(m.group(2) or 0)


def _gemm_problem_of_kind(p, g):
    """the operands of a case whose `operands` is not `unit` (the recipes: gemm_problem)"""
    c = p["case"]
    M, N, K = c["M"], c["N"], c["K"]
    fam, S = gemm_operand_kind(c)
    rn = lambda *s: torch.randn(s, generator=g)
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).float()
    ru = lambda lo, hi, n: torch.exp(torch.empty(n).uniform_(math.log(lo), math.log(hi), generator=g))
    conv, geglu = c["kind"] == "conv", c["act"] == ACT_GEGLU
    Cin = c["image"][3] if conv else K
    shape = tuple(c["image"][:3]) if conv else (M - c["zero_rows"],)
    n_out = N // 2 if geglu else N
    groups = -(-M // c["rows_per_rv"])

    def outliers(n):                    # two of every 64 (of a ragged last block too): its last and a random other one
        idx = []
        for b0 in range(0, n, 64):
            w = min(64, n - b0)
            idx += [b0 + w - 1, b0 + int(torch.randint(0, w - 1, (1,), generator=g))]
        return torch.tensor(idx)

    eb, er = 0.5, 1.0                   # bias / row vector and residual amplitudes
    if fam == "act":
        sk = ru(0.1, 30.0, Cin)
        sk[outliers(Cin)] = 300.0
        x = rn(*shape, Cin) * sk
        if c["ln"] is not None or c["gn_pro"] is not None:
            x = x + 4.0 * sk * torch.sign(rn(Cin))
        gain = ru(0.3, 3.0, N)
        W = rn(N, K) * K ** -0.5 * gain[:, None]
        if geglu:                       # sig: the pre-activation std of a row of gain 1
            sig = float(sk.square().mean().sqrt())
            W[:N // 2] *= 3.0 / sig
            W[N // 2:] *= 70.0 / sig / gain[N // 2:, None]
        eb, er = 5.0, 30.0
    elif fam in ("cancel", "exact", "overflow"):
        cols = gemm_slab_columns(c, S)
        sgn = torch.sign(rn(Cin))
        sgn_k = sgn[torch.arange(K) % Cin]                                  # (tap-major, channel-minor)
        rel = torch.zeros(K)
        if fam == "overflow" and c["cls"] == "conv":
            assert Cin == 128
            rel = 1.0 - 2.0 * (torch.arange(K) // 64 % 2)                  # + on the first 64-channel block of a tap, - on the second
        else:
            h = len(cols) // 2
            n_pos, n_neg = sum(len(i) for i in cols[:h]), sum(len(i) for i in cols[h:])
            rel[torch.cat(cols[:h])] = 1.0
            rel[torch.cat(cols[h:])] = -n_pos / n_neg
        assert abs(float(rel.sum())) < 1e-9
        nominal = max(abs(float(rel[i].sum())) for i in cols)              # the largest |sum of rel| over a slab
        if fam == "exact":
            x = 4.0 * ri(-2, 2, *shape, Cin) + 8.0 * sgn
            W = 8.0 * ri(-1, 1, N, K) + 8.0 * rel * sgn_k
            assert bool((W % 4 == 0).all()) and 64.0 * nominal == 12288.0
        else:
            a = 8.0
            b = 12288.0 / (a * nominal)
            x = rn(*shape, Cin) + a * sgn * (1 + 0.1 * rn(*shape, 1))
            W = rn(N, K) * K ** -0.5 + b * rel * sgn_k * (1 + 0.1 * rn(N, 1))
            if fam == "overflow":           # (patch: a pixel's partial averages the row factor over nine taps -- less spread)
                x, W = 2.0 * x, (2.25 if c["cls"] == "patch" else 2.0) * W
            eb = 100.0                      # (of the size of the results: the bound of these cases is 10 to 20 per element)
    else:
        assert fam == "staged" and c["bias"] and c["rowvec"] and c["res"] and not c["bias_per_row"]
        x, W = rn(*shape, Cin), rn(N, K) * K ** -0.5
    _put_input(p, x, rn)
    p["W"] = W.half()
    if fam == "staged":
        sg = torch.sign(rn(N))
        big_b, big_r = torch.rand(N, generator=g) < 0.1, torch.rand((groups, N), generator=g) < 0.15
        p["bias"] = (0.5 * rn(N) + 4e4 * sg * big_b).half()
        p["rowvec"] = (0.5 * rn(groups, N) + 3.5e4 * sg * big_r).half()
        either = big_b[None] | big_r[torch.arange(M) // c["rows_per_rv"]]
        p["R"] = (rn(M, N) - 3e4 * sg * either).half()
        return p
    if c["bias"]:
        p["bias"] = (eb * rn(M if c["bias_per_row"] else N)).half()
    if c["rowvec"]:
        p["rowvec"] = (eb * rn(groups, N)).half()
    if c["res"]:
        if fam == "exact":
            assert not c["bias"] and not c["rowvec"]
            p["R"] = (16.0 * ri(-8, 8, c["res_rows"] or M, n_out)).half()
        else:
            R = er * rn(c["res_rows"] or M, n_out)
            if fam == "act":
                R[:, outliers(n_out)] *= 10.0
            p["R"] = R.half()
    if c["gnf"] is not None:
        p["gnf_gamma"], p["gnf_beta"] = (1 + 0.2 * rn(N)).half(), (0.1 * rn(N)).half()
    return p


@functools.lru_cache(maxsize=None)
def gemm_problem(cid):
    """the seeded fp16 operands of one case (CPU), logical tensors only (gemm_operands puts them into the poisoned buffers a
    launch sees).  Do not modify the result.  By the case's `operands`:
      unit       unit Gaussians against K^-0.5 weights: partial sums below 4, results below 5
      act        SYNTHETIC trained magnitudes (no checkpoint exists where the suite runs: the figures are those reported for
                 transformer / UNet activations, per-channel scales over two decades and a few massive channels).  Activations
                 randn * s_k, s_k log-uniform in [0.1, 30], two channels of every 64 at 300 (the last of the block -- so that
                 the last K index carries weight -- and a random one); LayerNorm-fold and GroupNorm-prologue cases add a
                 per-channel mean of +-4 s_k; weights randn * K^-0.5 times a per-row gain log-uniform in [0.3, 3]; bias and row
                 vector 5 randn; residual 30 randn, times 10 in two columns of every 64.  GEGLU: the gate rows are scaled to
                 a pre-activation std of 70 (about [-300, 300]) and the x rows to 3 times their gain, so that x * gelu(gate)
                 stays below 3e4
      cancelS    a shared sign pattern s_k (per channel) of amplitude 8 (1 + 0.1 randn per row) on top of unit noise in A; in W
                 the same pattern, + in the first half of the slab list of split count S and - in the second, the two
                 weighted by their K extents so that the sum over K vanishes, scaled so that the largest slab partial is
                 nominally 12288: partials about +-2e4, results O(1e2 .. 1e3).  Bias and row vector 100 randn (of the size of
                 the results, so that an epilogue mistake is not lost in the slab term of the bound), the residual as in `unit`
      exactS     the same from small integers: A = 4 {-2 .. 2} + 8 s_k, W = 8 {-1, 0, 1} +- {8, 8 n0 / n1} s_k (multiples of 4), the
                 residual 16 {-8 .. 8}: every product is a multiple of 16 and nothing rounds
      overflowS  (GEMM_RANGE_CASES) cancelS with A and W times 2 (W of the patch kernel times 2.25): partials about +-8e4.  On the implicit convolution the + and
                 - parts alternate between the 64-channel blocks of every TAP instead (amplitude: one K tile = 12288 * 4):
                 a border pixel then loses balanced pairs, where the half / half layout leaves it a result beyond the range
                 even unsplit
      staged     (GEMM_RANGE_CASES) unit A and W; bias +-4e4 on a tenth of the columns, row vector +-3.5e4 of the same sign on
                 15 % of its entries, residual -+3e4 wherever either is large"""
    c = GEMM_CASE[cid]
    M, N, K = c["M"], c["N"], c["K"]
    # (seeded from the id without its variant / split part: the cases of one problem share their operands, so the GPU file can
    #  hold a forced variant against the heuristic and a split launch against the unsplit one)
    g = torch.Generator().manual_seed(zlib.crc32(gemm_problem_key(cid).encode()))
    rn = lambda *s: torch.randn(s, generator=g)
    p = dict(case=c, A2=None, bias=None, rowvec=None, R=None, gn_table=None)
    if c["operands"] != "unit":
        return _gemm_problem_of_kind(p, g)
    if c["kind"] == "conv":
        B, H, W, Cin = c["image"]
        x = rn(B, H, W, Cin) + (0.5 if c["gn_pro"] is not None else 0.0)
    else:
        x = rn(M - c["zero_rows"], K) + (0.5 if c["ln"] is not None else 0.0) + (4.0 if c["ln"] == "shifted" else 0.0)
    _put_input(p, x, rn)
    p["W"] = (rn(N, K) * K ** -0.5).half()                                # logical rows: [x | gate] halves for GEGLU
    if c["bias"]:
        p["bias"] = (0.5 * rn(M if c["bias_per_row"] else N)).half()
    if c["rowvec"]:
        p["rowvec"] = (0.5 * rn(-(-M // c["rows_per_rv"]), N)).half()
    n_out = N // 2 if c["act"] == ACT_GEGLU else N
    if c["res"]:
        p["R"] = rn(c["res_rows"] or M, n_out).half()
    if c["gnf"] is not None:
        p["gnf_gamma"], p["gnf_beta"] = (1 + 0.2 * rn(N)).half(), (0.1 * rn(N)).half()
    return p


def gemm_problem_key(cid):
    return re.sub(r"-(v\d+|t\d+|split\d+)(?=-|$)", "", cid)


def gemm_ln_args(p):
    """the ln_stats array (f32 [M, K / 160, 2]) of a LayerNorm-fold case from fp64 sums rounded to fp32, so that norm.hip is
    not under test"""
    x = p["A"].double()
    M, K = x.shape
    v = x.reshape(M, K // 160, 160)
    return torch.stack([v.sum(-1), (v * v).sum(-1)], -1).float().contiguous()


def gemm_operands(p, poison=True):
    """what a launch of the case is handed (CPU tensors; the GPU file moves the buffers): dict of name -> (buffer, view spec).
    A / A2 are the leading rows and a column slice of larger buffers; the rows in front, the rows behind and the columns outside
    hold the NaN patterns of _POISON (zeros with poison=False); W has eight such rows behind N where N is no multiple of 64.
    GEGLU weights / bias are packed for the serving kernel, w_tiled weights tiled, here, from the header's description."""
    c = p["case"]
    N, K = c["N"], c["K"]
    o = {}

    def put(name, data, rb=3, ra=5, c0=8, extra=16):
        shp = data.shape
        d2 = data.reshape(-1, shp[-1])
        o[name] = (_embed(d2, rb, ra, c0, shp[-1] + extra, poison), (rb, d2.shape[0], c0, shp[-1], tuple(shp)))

    # rows in front of the view: every virtual row below zero_rows (A / A2 point at row zero_rows: "never read"); for an image
    # the row of pixels above the first one and the one behind the last (where a clamped or unmasked tap would land)
    rb = max(3, c["zero_rows"]) if c["kind"] == "lin" else c["image"][2] + 3
    ra = 5 if c["kind"] == "lin" else c["image"][2] + 5
    put("A", p["A"], rb=rb, ra=ra)
    if p["A2"] is not None:
        put("A2", p["A2"], rb=rb, ra=ra, c0=16, extra=24)                 # lda2 != lda
    W, bias = p["W"], p["bias"]
    if c["act"] == ACT_GEGLU:
        g = 2 if N % 160 == 0 else 32
        W = geglu_pack(W[:N // 2], W[N // 2:], g)
        if bias is not None:
            bias = geglu_pack(bias[:N // 2, None], bias[N // 2:, None], g).reshape(-1)
    if c["w_tiled"]:
        W = w_tiled_pack(W, 160 if N % 160 == 0 else 128)
    put("W", W, rb=0, ra=8 if N % 64 else 0, c0=0, extra=0)
    o["bias"] = bias
    return o


def gemm_view(buf, spec):
    rb, rows, c0, cols, shp = spec
    return buf[rb:rb + rows].view(*shp[:-1], buf.shape[1])[..., c0:c0 + cols]


def parse_dispatch_sweep(text):
    """`emu_gemm --dispatch --sweep` output -> {(record, variant, splits): (return value, kernel, splits, kt_per_split, reduction kernel)}"""
    out = {}
    for line in text.splitlines():
        m = re.match(r"^((?:-?\d+ ){24})v (\d+) s (\d+) -> (-?\d+)(.*)$", line)
        if not m:
            continue
        rec = tuple(int(t) for t in m.group(1).split())
        launches = [l.strip() for l in m.group(5).split(" | ")[1:]]
        kern = sp = kt = red = None
        if launches:
            kern = launches[0].split(" grid ")[0]
            sp, kt = int(re.search(r"splits=(\d+)", launches[0]).group(1)), int(re.search(r"kt_per_split=(\d+)", launches[0]).group(1))
            red = launches[1].split(" grid ")[0] if len(launches) > 1 else None
        out[(rec, int(m.group(2)), int(m.group(3)))] = (int(m.group(4)), kern, sp, kt, red)
    return out


def gemm_case_is_wide(c):
    """served by the wide-tile kernels of csrc/gemm_glds.hip (else: the register-staged / narrow kernels of csrc/gemm_conv.hip)"""
    return not c["kernel"].startswith(("gemm_conv_kernel<", "conv3x3_narrow_kernel"))


def gemm_mutant_applies(mutant, c):
    """does the wrong variant differ from the right one on a case of this kind at all?"""
    conv = c["kind"] == "conv"
    ks, stride, pad, ups, Ho, Wo = c["geom"] or (0, 0, 0, 0, 0, 0)
    return {
        "last_k_dropped": True,
        "pad_tap_reads_edge": conv,
        "pad_before_normalise": c["gn_pro"] is not None,
        "tap_crosses_sample": conv and c["image"][0] > 1 and not ups and pad > 0,
        "rowvec_row_by_tile": c["rowvec"] and c["rows_per_rv"] % 64 != 0 and c["M"] > c["rows_per_rv"],
        "residual_no_wrap": c["res_rows"] > 0, "residual_wrap_off_by_one": c["res_rows"] > 0,
        "zero_rows_rounded_to_tile": c["zero_rows"] % 64 != 0,
        "bias_after_act": c["bias"] and c["act"] != ACT_NONE,
        "geglu_halves_swapped": c["act"] == ACT_GEGLU,
        "ups_gather_ceil": bool(ups),
        "k_split_second_source_offset": c["k_split"] > 0,
        "ln_mean_of_first_part": c["ln"] is not None,
        "tail_transposed_without_bias": c["n_split"] > 0 and c["bias"],
    }[mutant]


def groupnorm32_allowance(x, rows, gamma, beta, eps, silu, dx=0.0):
    """allowance of GroupNorm(32)(+SiLU) formed in fp32 from n = rows * N / 32 values per (sample, group): the sums are fp32 sums
    of n values in a fixed order, n u sum |v| each (u = 2^-24), so mean moves by n u mean|x| and the variance E[x^2] - mean^2 by
    n u (E[x^2] + 2 |mean| mean|x|); y = gamma xhat + beta moves by |gamma| (rstd d_mean + |xhat| d_var / (2 (var + eps))); plus the
    fp32 evaluation (fp32_allowance of the same formula on the CPU).  dx: the input itself is only known to within dx per element
    (the raw result is not stored): mean moves by dx, x - mean by 2 dx, rstd by 2 dx rstd relative -- |gamma| rstd 2 dx (1 + |xhat|)."""
    M, N = x.shape
    n = rows * (N // 32)
    v = x.double().reshape(M // rows, rows, 32, N // 32)
    mean, mabs, msq = v.mean((1, 3), keepdim=True), v.abs().mean((1, 3), keepdim=True), (v * v).mean((1, 3), keepdim=True)
    var = msq - mean * mean
    rstd = 1.0 / torch.sqrt(var + eps)
    xhat = ((v - mean) * rstd).abs()
    d_mean = n * _U * mabs
    d_var = n * _U * (msq + 2 * mean.abs() * mabs)
    a = rstd * d_mean + xhat * 0.5 * d_var / (var + eps) + rstd * 2 * dx * (1 + xhat)
    a = a.reshape(M, N) * gamma.double().abs() * (1.10 if silu else 1.0)
    y64 = groupnorm32_ref(x, rows, gamma, beta, eps, silu)
    y32 = F.group_norm(x.float().reshape(M // rows, rows, N).permute(0, 2, 1), 32, gamma.float(), beta.float(), eps).permute(0, 2, 1)
    y32 = (F.silu(y32) if silu else y32).reshape(M, N)
    return a + fp32_allowance(y64, y32)


# ------------------------------------------------------------------------------------------------
# stand-alone GroupNorm (csrc/norm.hip: pfd_groupnorm_f16, pfd_groupnorm_pstats_f16, pfd_groupnorm_table_f16): reference, the
# host's decisions restated, bound, mutants, cases and operands
# (tests/test_norm_kernels_cpu.py pins and qualifies them, tests/test_norm_kernels_gpu.py uses them)
# ------------------------------------------------------------------------------------------------
GN_ROWS, GN_MAX_CHUNKS, GN_MAX_G, GNS_T, GNS_MAX = 8, 256, 64, 1024, 8       # the constants of csrc/norm.hip
GN_FORMS = ("small", "two", "pstats_par", "pstats_plain")
# the kernels a form launches, in the spelling of `emu_norm --dispatch`
GN_FORM_KERNELS = {"small": ("gn_small_kernel",), "two": ("gn_stats_kernel", "gn_apply_kernel"),
                   "pstats_par": ("gn_apply_pstats_kernel<true>",), "pstats_plain": ("gn_apply_pstats_kernel<false>",),
                   "table": ("gn_stats_kernel", "gn_table_kernel")}
GN_MUTANTS = ("last_row_dropped", "last_row_twice", "chunk_last_row_dropped", "second_slot_skipped", "count_from_c1",
              "group_by_source", "eps_1e-5", "eps_omitted", "var_not_clamped", "silu_before_affine", "slab_without_sample_offset",
              "second_producer_group_dropped")


def gn_chunks(B, C, HW):
    """gn_chunks() of csrc/norm.hip restated: (nchunks, rows_per_chunk) of the two-launch and producer-statistics forms"""
    nvec = C // 8
    RT = 256 // nvec if nvec < 256 else 1
    nchunks = min(-(-512 // B), -(-HW // (RT * 4)), GN_MAX_CHUNKS)
    nchunks = max(nchunks, 1)
    rpc = -(-HW // nchunks)
    return -(-HW // rpc), rpc


def gn_is_small(B, C, HW, G):
    cpg = C // G
    return cpg % 4 == 0 and cpg >= 32 and HW * (cpg // 4) <= GNS_T * GNS_MAX and B * G >= 128


def gn_takes_pstats(B, C1, C2, HW, G):
    """pfd_groupnorm_takes_pstats restated"""
    if B <= 0 or C1 <= 0 or C2 < 0 or HW <= 0 or G <= 0 or G > GN_MAX_G:
        return False
    C = C1 + C2
    if C % G or C > 4096 or HW % 64 or C1 % 160 or C2 % 160 or C1 % 32 or C2 % 32:
        return False
    if gn_is_small(B, C, HW, G):
        return False
    cpg, cpp1 = C // G, C1 // 32
    cpp2 = C2 // 32 if C2 else cpp1
    if cpp1 < 8 or 160 % cpp1 or cpg % cpp1 or C1 % cpg:
        return False
    if C2 and (cpp2 < 8 or 160 % cpp2 or cpg % cpp2):
        return False
    return True


def gn_producer_groups(C1, C2, G):
    """(npg1, npg2): producer groups (C_src / 32 channels each) per group of this norm, per source"""
    cpg, cpp1 = (C1 + C2) // G, C1 // 32
    cpp2 = C2 // 32 if C2 else cpp1
    return cpg // cpp1, cpg // cpp2


def gn_form(B, HW, C1, C2, G, pstats):
    """the form a request takes (pstats: the caller hands over producer statistics), None: PFD_ESHAPE"""
    if pstats:
        if not gn_takes_pstats(B, C1, C2, HW, G):
            return None
        n1, n2 = gn_producer_groups(C1, C2, G)
        return "pstats_par" if n1 <= 2 and n2 <= 2 else "pstats_plain"
    return "small" if gn_is_small(B, C1 + C2, HW, G) else "two"


# D, the largest number of fp32 additions between one input value and the sum of its group, from the loops of csrc/norm.hip
# (an addition of a masked 0.f counts: it is on the chain even where it cannot round); the squares of fp16 values are exact in
# fp32, so the sum of squares has the same chain.  Behind the two sums come three more roundings that the variance sees in full
# (sum / count, sum of squares / count, mean * mean): + 3 in every form.
#   two-launch   gn_stats_kernel: a thread adds GN_ROWS values per sweep of its chunk, sweeps = ceil(rows_per_chunk / (GN_ROWS RT)),
#                RT = 256 / min(C / 8, 256) row threads per channel vector; thread rt = 0 adds the RT partials of a channel; thread g
#                adds the C / G channels of its group.  gn_apply_kernel / gn_table_kernel: thread (part, g) adds chunks part,
#                part + P, ... (ceil(nchunks / P), P = 256 / G), thread g the P partials.
#                D = GN_ROWS sweeps + RT + C / G + ceil(nchunks / P) + P + 3
#   small        gn_small_kernel: a thread adds 4 values of each of its GNS_MAX register slots, wave_sum is 6 xor exchanges, every
#                thread adds the GNS_T / 64 wave sums.  D = 4 GNS_MAX + 6 + GNS_T / 64 + 3
#   pstats       the tests form the producers' sums in fp64 and round them to fp32 once (1); thread (part, g) folds slabs part,
#                part + P, ...: the plain loop ceil(nslab / P) slabs of npg producer groups each, the grouped form whole trips of 8
#                slabs, two additions per slab (the second with weight 0 where npg = 1); thread g adds the P partials.
#                D = 1 + npg ceil(nslab / P)  |  1 + 2 * 8 ceil(ceil(nslab / P) / 8)   + P + 3
def gn_depth(form, B, HW, C1, C2, G):
    C = C1 + C2
    P = 256 // G
    if form == "small":
        return 4 * GNS_MAX + 6 + GNS_T // 64 + 3
    nchunks, rpc = gn_chunks(B, C, HW)
    if form in ("two", "table"):
        RT = 256 // min(C // 8, 256)
        return GN_ROWS * -(-rpc // (GN_ROWS * RT)) + RT + C // G + -(-nchunks // P) + P + 3
    per = -(-(HW // 64) // P)
    if form == "pstats_par":
        return 1 + 2 * 8 * -(-per // 8) + P + 3
    assert form == "pstats_plain", form
    return 1 + max(gn_producer_groups(C1, C2, G)) * per + P + 3


def _gn_cat(x1, x2, B, HW, dtype):
    v = x1.to(dtype).reshape(B, HW, -1)
    return v if x2 is None else torch.cat([v, x2.to(dtype).reshape(B, HW, -1)], -1)


def _gn_stats(x1, x2, B, HW, G, eps, mutant=None, dtype=torch.float64, rpc=None, depth=None):
    """(v [B, HW, C], mean [B, G], var [B, G], eps): the statistics of the virtual concat as sums over count, the way every
    kernel form defines them; the wrong variants of GN_MUTANTS that concern the statistics"""
    assert mutant is None or mutant in GN_MUTANTS, mutant
    v = _gn_cat(x1, x2, B, HW, dtype)
    C, C1 = v.shape[-1], x1.shape[-1]
    cpg = C // G
    wr, wc = torch.ones(HW, dtype=dtype, device=v.device), torch.ones(C, dtype=dtype, device=v.device)
    count = float(HW * cpg)
    if mutant == "last_row_dropped":
        wr[-1] = 0
    if mutant == "last_row_twice":
        wr[-1] = 2
    if mutant == "chunk_last_row_dropped":
        wr[rpc - 1::rpc] = 0
        wr[-1] = 0
    if mutant == "second_slot_skipped":
        wc[2048:] = 0
    if mutant == "count_from_c1":
        count = float(HW * C1) / G
    if mutant == "second_producer_group_dropped":
        n1, n2 = gn_producer_groups(C1, C - C1, G)
        c = torch.arange(C)
        cpp = torch.where(c < C1, C1 // 32, (C - C1) // 32 if C > C1 else C1 // 32)
        npg = torch.where(c < C1, n1, n2)
        wc[((c % cpg) // cpp == 1) & (npg >= 2)] = 0
    S = (torch.einsum("r,brc->bc", wr, v) * wc).reshape(B, G, cpg).sum(-1)
    Q = (torch.einsum("r,brc->bc", wr, v * v) * wc).reshape(B, G, cpg).sum(-1)
    if mutant == "slab_without_sample_offset":
        S, Q = S[:1].expand(B, G), Q[:1].expand(B, G)
    mean = S / count
    var = Q / count - mean * mean
    if mutant == "var_not_clamped":
        # the clamp matters once fp32 rounding has taken the difference below zero: the mutant's variance sits at the low end of
        # what the allowance admits, D u E[x^2] below the exact one
        var = var - depth * _U * Q / count
    else:
        var = var.clamp_min(0)
    if mutant == "eps_1e-5":
        eps = 1e-5
    if mutant == "eps_omitted":
        eps = 0.0
    return v, mean, var, eps


def groupnorm_ref(x1, x2, B, HW, G, gamma, beta, eps, silu, mutant=None, dtype=torch.float64, rpc=None, depth=None):
    """GroupNorm(G) (+ SiLU) over the virtual channel concat [x1 | x2] of token-major [B HW, C1] / [B HW, C2] tensors (x2 may be
    None) -> [B HW, C1 + C2] in `dtype`: per (sample, group of C / G consecutive channels of the concat) mean = sum / n,
    var = max(sum of squares / n - mean^2, 0), y = (x - mean) / sqrt(var + eps) * gamma + beta.  mutant: one of GN_MUTANTS (rpc:
    the rows per chunk for chunk_last_row_dropped, depth: D for var_not_clamped)."""
    v, mean, var, eps = _gn_stats(x1, x2, B, HW, G, eps, mutant, dtype, rpc, depth)
    C, C1 = v.shape[-1], x1.shape[-1]
    cpg = C // G
    gi = torch.arange(C, device=v.device) // cpg
    if mutant == "group_by_source":
        gi[C1:] = torch.arange(C - C1, device=v.device) // cpg
    rstd = 1.0 / torch.sqrt(var + eps)
    xhat = (v - mean[:, gi][:, None]) * rstd[:, gi][:, None]
    if mutant == "silu_before_affine":
        return (F.silu(xhat) * gamma.to(dtype) + beta.to(dtype)).reshape(B * HW, C)
    y = xhat * gamma.to(dtype) + beta.to(dtype)
    return (F.silu(y) if silu else y).reshape(B * HW, C)


def groupnorm_table_ref(x1, x2, B, HW, G, gamma, beta, eps):
    """pfd_groupnorm_table_f16: float64 [B, 2, C], scale = rstd gamma, shift = beta - mean scale"""
    v, mean, var, eps = _gn_stats(x1, x2, B, HW, G, eps)
    gi = torch.arange(v.shape[-1]) // (v.shape[-1] // G)
    scale = (1.0 / torch.sqrt(var + eps))[:, gi] * gamma.double()
    return torch.stack([scale, beta.double() - mean[:, gi] * scale], 1)


def groupnorm_allowance(x1, x2, B, HW, G, gamma, beta, eps, silu, D, parts=False):
    """groupnorm32_allowance with the number of values per group replaced by D (gn_depth): a sum whose every input passes
    through at most D fp32 additions is off by at most D u sum |v| (first order; Higham, Accuracy and Stability, 4.2), so mean
    moves by d_mean = D u mean|x| and the variance E[x^2] - mean^2 by d_var = D u (E[x^2] + 2 |mean| mean|x|); y = gamma xhat +
    beta moves by |gamma| (rstd d_mean + |xhat| d_var / (2 (var + eps))); plus the fp32 evaluation (fp32_allowance of torch's
    F.group_norm (+ F.silu) in fp32 on the CPU against the fp64 reference).  Returns a [B HW, C]; parts=True: (a, a_scale,
    a_shift), the last two [B, C]: the statistics part for the table -- scale = rstd gamma moves by |scale| d_var / (2 (var + eps)),
    shift = beta - mean scale by |scale| d_mean + |mean| d_scale, each plus 8 u of its terms (rsqrtf, the quotients and products)."""
    v, mean, var, _ = _gn_stats(x1, x2, B, HW, G, eps)
    C = v.shape[-1]
    cpg = C // G
    vg = v.reshape(B, HW, G, cpg)
    mabs, msq = vg.abs().mean((1, 3)), (vg * vg).mean((1, 3))
    rstd = 1.0 / torch.sqrt(var + eps)
    d_mean = D * _U * mabs
    d_rstd_rel = 0.5 * D * _U * (msq + 2 * mean.abs() * mabs) / (var + eps)
    gi = torch.arange(C) // cpg
    xhat = ((v - mean[:, gi][:, None]) * rstd[:, gi][:, None]).abs()
    a = (rstd * d_mean)[:, gi][:, None] + xhat * d_rstd_rel[:, gi][:, None]
    a = (a * gamma.double().abs() * (1.10 if silu else 1.0)).reshape(B * HW, C)
    y64 = groupnorm_ref(x1, x2, B, HW, G, gamma, beta, eps, silu)
    y32 = F.group_norm(v.float().permute(0, 2, 1), G, gamma.float(), beta.float(), eps).permute(0, 2, 1)
    y32 = (F.silu(y32) if silu else y32).reshape(B * HW, C)
    a = a + fp32_allowance(y64, y32)
    if not parts:
        return a
    scale = rstd[:, gi] * gamma.double()
    a_scale = scale.abs() * d_rstd_rel[:, gi] + 8 * _U * scale.abs()
    ms = (mean[:, gi] * scale).abs()
    a_shift = scale.abs() * d_mean[:, gi] + mean[:, gi].abs() * a_scale + 8 * _U * (beta.double().abs() + ms)
    return a, a_scale, a_shift


def _gnc(cid, form, B, HW, C1, C2=0, G=32, eps=1e-5, silu=True, strides=None, kind="unit", shares=None, table=False):
    return dict(id=cid, form=form, B=B, HW=HW, C1=C1, C2=C2, G=G, eps=eps, silu=silu, strides=strides, kind=kind, shares=shares,
                table=table or form == "two")


# (id, expected form, B, HW, C1, C2, G, eps, silu, strides = the pad columns of x / x2 / y, input kind); `shares`: the case takes
# the leading samples of that case's operands; `table`: pfd_groupnorm_table_f16 runs on the case's operands too (every
# two-launch case and two small-form shapes)
GN_CASES = [
    _gnc("small-B4-HW64-C1280", "small", 4, 64, 1280, table=True),                     # B G exactly 128
    _gnc("small-B4-HW64-C1280+640", "small", 4, 64, 1280, 640, kind="offset6"),          # cpg 60: a group straddles the sources
    _gnc("small-B4-HW819-C1280", "small", 4, 819, 1280, silu=False),                    # 8190 of 8192 chunks, all eight slots
    _gnc("small-B4-HW100-C1408", "small", 4, 100, 1408, kind="tiny", table=True),       # cpr 11
    _gnc("small-B2-HW16-C2048-G64", "small", 2, 16, 2048, G=64, kind="const"),
    _gnc("small-B4-HW9-C1024+256-strided", "small", 4, 9, 1024, 256, strides=(8, 16, 24)),
    _gnc("two-B4-HW820-C1280", "two", 4, 820, 1280),                                    # one row past the small form
    _gnc("two-B3-HW64-C1280", "two", 3, 64, 1280, shares="small-B4-HW64-C1280"),        # B G = 96
    _gnc("two-B2-HW30-C320+640", "two", 2, 30, 320, 640, kind="offset6"),               # cpg 30, 16 idle threads
    _gnc("two-B1-HW64-C1280+1280", "two", 1, 64, 1280, 1280, silu=False),               # second vector slot
    _gnc("two-B1-HW5-C4096", "two", 1, 5, 4096),                                        # both slots full, chunks of 3 and 2 rows
    _gnc("two-B1-HW1089-C128-eps1e-6", "two", 1, 1089, 128, eps=1e-6, kind="tiny"),     # the VAE's cpg 4 at 33 x 33, ragged last chunk
    _gnc("two-B1-HW4096-C320", "two", 1, 4096, 320, kind="offset6", silu=False),
    _gnc("two-B3-HW37-C256", "two", 3, 37, 256, kind="const"),
    _gnc("two-B2-HW1-C64-G8", "two", 2, 1, 64, G=8),
    _gnc("two-B2-HW50-C192-G24", "two", 2, 50, 192, G=24),                              # P = 10
    _gnc("two-B2-HW33-C64-G1", "two", 2, 33, 64, G=1, kind="offset6"),
    _gnc("two-B1-HW1100-C2048", "two", 1, 1100, 2048, silu=False),                      # the GN_MAX_CHUNKS cap
    _gnc("two-B2-HW45-C320+192-strided", "two", 2, 45, 320, 192, strides=(8, 16, 24)),
    _gnc("pstats-B1-HW4096-C320", "pstats_par", 1, 4096, 320),
    _gnc("pstats-B2-HW1024-C320+320", "pstats_par", 2, 1024, 320, 320, kind="offset6"),
    _gnc("pstats-B2-HW256-C640", "pstats_par", 2, 256, 640, silu=False),                # clamped slab slots
    _gnc("pstats-B1-HW4608-C320", "pstats_par", 1, 4608, 320, kind="tiny"),             # second trip of the fold
    _gnc("pstats-B2-HW128-C1280+1280", "pstats_par", 2, 128, 1280, 1280),
    _gnc("pstats-B2-HW256-C320-G8", "pstats_plain", 2, 256, 320, G=8),
    _gnc("pstats-B2-HW256-C640+640-G16", "pstats_plain", 2, 256, 640, 640, G=16, kind="offset6", silu=False),
    _gnc("pstats-B2-HW128-C1280+640-G24", "pstats_plain", 2, 128, 1280, 640, G=24),     # producer groups of 40 | 20 channels
]
GN_CASE = {c["id"]: c for c in GN_CASES}
assert len(GN_CASE) == len(GN_CASES)
GN_EDGE_GAIN = 4.0


def gn_edge_rows(c):
    """the rows a wrong row count would lose or count twice: the first and last of a sample, both sides of every chunk
    boundary (gn_chunks) and, where producer statistics are folded, of every 64-row slab"""
    nchunks, rpc = gn_chunks(c["B"], c["C1"] + c["C2"], c["HW"])
    rows = {0, c["HW"] - 1}
    step = [rpc] + ([64] if c["form"].startswith("pstats") else [])
    for s in step:
        for k in range(s, c["HW"], s):
            rows.update((k - 1, k))
    return sorted(rows)


def gn_depth_of(c, table=False):
    return gn_depth("table" if table else c["form"], c["B"], c["HW"], c["C1"], c["C2"], c["G"])


@functools.lru_cache(maxsize=None)
def gn_problem(cid):
    """the seeded fp16 operands of one case (CPU): x1 [B HW, C1], x2 [B HW, C2] | None, gamma = 1 + 0.2 randn, beta = 0.1 randn.
    kinds: unit (randn + 0.5) | offset6 (6 + 0.5 randn) | tiny (zero mean, std 1e-3 .. 3e-3 per channel) | const (unit, with group
    0 constant at 3.0 -- every sum exact -- and group 1 at fp16(2.7), whose sums round).  The deviation from the offset is
    GN_EDGE_GAIN times larger on gn_edge_rows.  Do not modify the result."""
    c = GN_CASE[cid]
    if c["shares"]:
        q = gn_problem(c["shares"])
        n = c["B"] * c["HW"]
        assert q["case"]["HW"] == c["HW"] and q["case"]["C1"] == c["C1"] and q["x2"] is None and c["C2"] == 0
        assert gn_edge_rows(c) == gn_edge_rows(q["case"])
        return dict(q, case=c, x1=q["x1"][:n])
    B, HW, C1, C2, G = c["B"], c["HW"], c["C1"], c["C2"], c["G"]
    C = C1 + C2
    g = torch.Generator().manual_seed(zlib.crc32(cid.encode()))
    dev = torch.randn((B, HW, C), generator=g)
    dev[:, gn_edge_rows(c)] *= GN_EDGE_GAIN
    if c["kind"] == "offset6":
        x = 6.0 + 0.5 * dev
    elif c["kind"] == "tiny":
        x = dev * (1e-3 + 2e-3 * torch.rand(C, generator=g))
    else:
        x = dev + 0.5
    if c["kind"] == "const":
        cpg = C // G
        x[..., :cpg] = 3.0
        x[..., cpg:2 * cpg] = 2.7
    x = x.half().reshape(B * HW, C)
    gamma, beta = (1 + 0.2 * torch.randn(C, generator=g)).half(), (0.1 * torch.randn(C, generator=g)).half()
    return dict(case=c, x1=x[:, :C1].contiguous(), x2=x[:, C1:].contiguous() if C2 else None, gamma=gamma, beta=beta)


def gn_args(p):
    """the positional arguments of groupnorm_ref / groupnorm_allowance up to silu"""
    c = p["case"]
    return (p["x1"], p["x2"], c["B"], c["HW"], c["G"], p["gamma"], p["beta"], c["eps"], c["silu"])


def gn_operands(p, poison=True):
    """what a launch is handed (CPU): x1 / x2 as [B, HW, C] views; with strides, column slices (offset 8) of wider buffers that
    hold fp16 NaNs (zeros with poison=False) in the pad columns and in two rows in front and three behind"""
    c = p["case"]
    out = {}
    for k, pad in (("x1", 0), ("x2", 1)):
        t = p[k]
        if t is None:
            out[k] = None
        elif c["strides"] is None:
            out[k] = t.view(c["B"], c["HW"], -1)
        else:
            buf = _embed(t, 2, 3, 8, t.shape[1] + 8 + c["strides"][pad], poison)
            out[k] = (buf, (2, t.shape[0], 8, t.shape[1], (c["B"], c["HW"], t.shape[1])))
    return out


def gn_pstats(x):
    """the producer statistics of one source, float32 [B HW / 64, C / 160, 16, 2]: gn_out_ref of the f16 values (fp64 sums)
    rounded to fp32 once; the slots no producer writes stay NaN"""
    return gn_out_ref(x).float().contiguous()


def gn_mutant_applies(mutant, c):
    """does the wrong variant differ from the right one on this case, by more than an fp32 rounding?"""
    C = c["C1"] + c["C2"]
    ps = c["form"].startswith("pstats")
    return {
        "last_row_dropped": not ps, "last_row_twice": not ps,
        "chunk_last_row_dropped": c["form"] == "two" and gn_chunks(c["B"], C, c["HW"])[0] > 1,
        "second_slot_skipped": c["form"] == "two" and C > 2048,
        "count_from_c1": c["C2"] > 0, "group_by_source": c["C2"] > 0,
        "eps_1e-5": c["eps"] != 1e-5,
        "eps_omitted": c["kind"] in ("tiny", "const"),
        "var_not_clamped": c["kind"] == "const",
        "silu_before_affine": c["silu"],
        "slab_without_sample_offset": ps and c["B"] > 1,
        "second_producer_group_dropped": ps and max(gn_producer_groups(c["C1"], c["C2"], c["G"])) >= 2,
    }[mutant]
