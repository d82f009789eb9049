"""Plain fp64 references of single kernels of the library, and the seeded operands the kernel-level tests run them on: the
SeeCoder side (tests/test_encoder_kernels_cpu.py pins the references to the oracle, tests/test_encoder_kernels_gpu.py
compares the HIP kernels with them) and the fused attention family (tests/test_attention_kernels_{cpu,gpu}.py, the last
section).  Everything here is torch on whatever device the operands live on; nothing imports the
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


# ------------------------------------------------------------------------------------------------
# fused attention (pfd_attention_f16): references, the dispatcher restated, cases and operands
# (tests/test_attention_kernels_cpu.py pins and qualifies them, tests/test_attention_kernels_gpu.py uses them)
# ------------------------------------------------------------------------------------------------
LOG2E = 1.4426950408889634
ATTN_MUTANTS = ("last_key_dropped", "masked_keys_score_zero", "vt_batch0", "k_batch0", "v_pad_column_read")
ATTN_CLASSES = ("w4", "w8", "a3", "d80", "d96", "d160", "d512_2", "d512_4")
ATTN_FOLDED = ("w8", "a3")          # Q' = fp16(q * scale * log2 e), softmax as exp2 of the raw products


def attention_kernel_class(B, H, Nq, Nk, D, slices=2):
    """which kernel pfd_attention_f16 launches: csrc/attention.hip launch<D>() (the `big` / `w8` lines), launch512() and the
    switch of pfd_attention_f16, and pfd_attention3_takes() at the end of csrc/attention3_kernel.h, restated without the
    process-static test hooks.  None: PFD_ESHAPE."""
    if D == 512:
        return f"d512_{4 if slices == 4 else 2}" if H == 1 and Nk % 32 == 0 else None
    if D in (80, 96, 160):
        return f"d{D}"
    if D != 40:
        return None
    blocks = B * H * ((Nq + 255) // 256)
    if Nk % 64 == 0 and Nk >= 128 and Nq >= 256 and blocks >= 256:
        return "a3"
    if Nq >= 1024 and blocks >= 512:
        return "w8"
    return "w4"


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
