"""TEST INFRASTRUCTURE: a torch stand-in of `lib.hip.ops` for machines without a GPU.

Every function below has the signature of the function of the same name in lib/hip/ops.py and computes what that function's
docstring and include/pfd_hip.h say the launch computes, with the fp64 references of tests/kernel_refs.py (gemm_ref,
attention_ref, groupnorm_ref, layernorm_ref, ln_out_ref, gn_out_ref, ...): arithmetic in fp64, every tensor the library stores as
fp16 rounded to fp16 ONCE, statistics as fp32 in the documented layouts.  What the host layer hands from one launch to the next is
USED, not recomputed: the LayerNorm fold normalises with the partial row sums and the column sums it was given, a GroupNorm that
finds producer statistics on its input normalises with those, the phase-folded upsample contracts the folded weight.  A host layer
that hands over the wrong slice therefore computes the wrong thing here as it would on the device.

Carried state (set_gn_stats / get_gn_stats / set_normed / get_normed / _written / cat_pair), the decline memory (_DECLINED,
ups_fold_key, ups_fold_declined) and the shape predicates (ln_fold_ok, wide_tile_ok, conv_gn_fusable, gn_stats_wanted) are the real
functions of lib.hip.ops: they are code under test.  gn_stats_wanted and the GEGLU group size ask the real library's host-side
functions (nothing is launched).

The optional forms -- conv(ups=2), conv(gn_fuse=...) -- are answered "served" or "declined" by a Policy the test chooses.
`install(monkeypatch, policy)` patches the attributes of lib.hip.ops (the product modules look `ops.*` up at call time) and the one
device guard of the host layer.
"""
import torch
import torch.nn.functional as F

import kernel_refs as KR
from lib.hip import binding, layers, ops
from lib.hip.binding import ACT_GEGLU, ACT_NONE, ACT_SILU


class Policy:
    """answers for the optional forms.  mode: 'serve' (wherever the header's contract allows the form), 'decline' (never) or a
    list of booleans consumed in request order (a recorded run).  .asked: [(form, served)] of this run."""

    def __init__(self, mode="serve"):
        self.mode = mode if isinstance(mode, str) else list(mode)
        self.asked = []

    def answer(self, form, allowed):
        if isinstance(self.mode, list):
            if not self.mode:
                raise AssertionError(f"recorded run has no answer left for this {form} request: the requests do not line up")
            served = bool(self.mode.pop(0))
            if served and not allowed:
                raise AssertionError(f"recorded run has {form} served where the header's contract does not allow it")
        else:
            served = allowed and self.mode == "serve"
        self.asked.append((form, served))
        return served


_POLICY = [Policy()]
FELL_THROUGH = []


def _lib():
    return binding.load()


def _h(v):
    return v.to(torch.float16)


def _put(out, val, shape):
    """the fp16 result in a new tensor or written THROUGH the caller's `out` (views included)"""
    v = _h(val).reshape(shape)
    if out is None:
        return v.contiguous()
    out.copy_(v.reshape(out.shape))
    return out


def _gn_stats_of(stored2d):
    s = KR.gn_out_ref(stored2d)
    return torch.nan_to_num(s, nan=0.0).float().contiguous()


def _case(**kw):
    c = dict(kind="lin", gn_pro=None, geom=None, zero_rows=0, k_split=0, act=ACT_NONE, ln=None, ln_eps=1e-5, bias_per_row=False,
             rows_per_rv=1, res_rows=0, n_split=0)
    c.update(kw)
    return c


# ----------------------------------------------------------------------------------------------
# GEMM / convolution
# ----------------------------------------------------------------------------------------------
def gemm(a, w, *, bias=None, rowvec=None, rows_per_rv=1, res=None, act=ACT_NONE, out=None, bias_per_row=False, n=None, k=None,
         tile=0, out_t=None, n_split=None, ln=None, ln_out=None, a2=None, zero_rows=0, gn_out=False, res_rows=None, w_tiled=False):
    assert a.dtype == torch.float16 and w.dtype == torch.float16 and not w_tiled and tile == 0
    M, Ka, _ = ops._rows(a)
    Nw, Kw, _ = ops._rows(w)
    N = Nw if n is None else n
    K = min(Ka, Kw) if k is None else k
    A = a.reshape(M, Ka)
    A2 = None
    if a2 is not None:
        M2, Ka2, _ = ops._rows(a2)
        if M2 != M:
            raise ValueError(f"gemm: a2 {tuple(a2.shape)} does not pair with a {tuple(a.shape)}")
        if k is None:
            K = Ka + Ka2
        if Ka % 64 or Ka >= K or K - Ka > Ka2:
            raise ValueError(f"gemm: a2 needs a first source of a multiple of 64 columns below K (Ka {Ka}, K {K})")
        if not ops.wide_tile_ok(N, K):
            raise ValueError("gemm: a2 is a wide-tile form (PFD_ESHAPE)")
        A2 = a2.reshape(M, Ka2)[:, :K - Ka].double()
        X = A.double()
    else:
        X = A[:, :K].double()
    if K % 64 or ops._rows(a)[2] % 8 or ops._rows(w)[2] % 8:
        raise ValueError(f"gemm: K {K} % 64 != 0 or a leading dimension % 8 != 0 (PFD_ESHAPE: include/pfd_hip.h, Requirements)")
    if zero_rows:
        if zero_rows < 0 or ln is not None:
            raise ValueError("gemm: zero_rows must be >= 0 and cannot be combined with ln=")
        if not ops.wide_tile_ok(N, K):
            raise ValueError("gemm: zero_rows is a wide-tile form (PFD_ESHAPE)")
        M += zero_rows
    n_out = N // 2 if act == ACT_GEGLU else N
    if out_t is not None:
        n_out = n_split
        if out_t.shape[0] != N - n_split or out_t.shape[1] < M or out_t.stride(1) != 1:
            raise ValueError(f"gemm: out_t {tuple(out_t.shape)} cannot hold [{N - n_split}, {M}]")
    if out is not None and (out.shape[-1] != n_out or out.numel() != M * n_out or out.dtype != torch.float16):
        raise ValueError(f"gemm: out {tuple(out.shape)} cannot hold [{M}, {n_out}]")
    R = None
    if res_rows is not None:
        if res is None or M != 2 * res_rows or ops._rows(res)[0] != res_rows:
            raise ValueError(f"gemm: res_rows {res_rows} needs a residual of exactly that many rows and M == 2 * res_rows (M {M})")
        if not ops.wide_tile_ok(N, K):
            raise ValueError("gemm: res_rows is a wide-tile form (PFD_ESHAPE)")
    elif res is not None and ops._rows(res)[0] != M:
        raise ValueError(f"gemm: residual of {ops._rows(res)[0]} rows for {M} output rows (res_rows= names a shared one)")
    if res is not None:
        R = res.reshape(-1, res.shape[-1])
    W = w.reshape(Nw, Kw)[:N, :K].double()
    b = None if bias is None else bias.double()
    if ln is not None:
        # PfdGemmDesc.ln_stats: rstd (x W'^T - mean s) + b' with mean / rstd from the PARTIAL sums handed over and the column sums
        # handed over, written as one contraction over [rstd x | -rstd mean] and [W' | s]
        st, cs, eps = ln
        if st.dtype != torch.float32 or st.dim() != 3 or st.shape[0] != M or st.shape[1] * 160 != K or st.shape[2] != 2:
            raise ValueError(f"gemm: ln stats {tuple(st.shape)} {st.dtype} do not describe a [{M}, {K}] operand")
        if cs.dtype != torch.float32 or cs.numel() != N:
            raise ValueError("gemm: ln column sums must be a contiguous float32 [N]")
        mean = st[..., 0].double().sum(1) / K
        rstd = 1.0 / torch.sqrt(st[..., 1].double().sum(1) / K - mean * mean + eps)
        X = torch.cat([X * rstd[:, None], (-rstd * mean)[:, None]], 1)
        W = torch.cat([W, cs.double().reshape(N, 1)], 1)
    if act == ACT_GEGLU:      # the packed weight interleaves x / gate rows in groups the library names: back to the logical halves
        g = int(_lib().pfd_gemm_geglu_group(N))
        W = torch.cat(KR.geglu_unpack(W, g), 0)
        if b is not None:
            b = torch.cat(KR.geglu_unpack(b.reshape(N, 1), g), 0).reshape(N)
    c = _case(M=M, N=N, K=K, act=act, bias_per_row=bool(bias_per_row), rows_per_rv=rows_per_rv, zero_rows=zero_rows,
              res_rows=res_rows or 0, n_split=n_split if out_t is not None else 0, k_split=Ka if a2 is not None else 0)
    p = dict(case=c, A=X, A2=A2, W=W, bias=b, rowvec=None if rowvec is None else rowvec.reshape(-1, rowvec.shape[-1]), R=R)
    r = KR.gemm_ref(p)
    out = _put(out, r["out"], (M, n_out))
    if out_t is not None:
        out_t[:, :M].copy_(_h(r["out_t"]))
    stats = None
    ln_out = ops.ln_out_arg(ln_out)
    if ln_out is not None:
        if N % 160 or act == ACT_GEGLU or out_t is not None:
            raise ValueError("gemm: ln_out needs N % 160 == 0, no GEGLU, no transposed tail (PFD_ESHAPE)")
        stats = ops._row_stats("gemm: ln_out", "M, N/160, 2", M, N, a.device, ln_out)
        stats.copy_(KR.ln_out_ref(out.reshape(M, N)).float().reshape(stats.shape))
    gst = _gn_stats_of(out.reshape(M, N)) if gn_out else None
    ops._written(out, gst)
    return out if stats is None else (out, stats)


def _phase_conv(x, w, bias, act):
    """PfdGemmDesc.ups = 2 from the header text: output pixel (2y+py, 2x+px) reads the low-res pixels (y+py-1+ty, x+px-1+tx)"""
    B, H, W_, Cin = x.shape
    N = w.shape[1]
    xp = F.pad(x.double(), (0, 0, 1, 1, 1, 1))
    y = torch.empty((B, 2 * H, 2 * W_, N), dtype=torch.float64)
    for py in range(2):
        for px in range(2):
            acc = 0
            for ty in range(2):
                for tx in range(2):
                    t = ty * 2 + tx
                    acc = acc + xp[:, py + ty:py + ty + H, px + tx:px + tx + W_] @ w[py * 2 + px][:, t * Cin:(t + 1) * Cin].double().t()
            y[:, py::2, px::2] = acc
    if bias is not None:
        y = y + bias.double()
    return KR.activation_ref(y, act)


def conv(x, w, ksize, *, stride=1, pad=None, ups=False, bias=None, rowvec=None, res=None, act=ACT_NONE, out=None, tile=0,
         out_hw=None, rows_per_rv=None, gn=None, gn_out=False, gn_fuse=None, w_tiled=False):
    assert x.dtype == torch.float16 and w.dtype == torch.float16 and not w_tiled and tile == 0
    B, H, W_, Cin = x.shape
    x2 = table = None
    C1 = Cin
    if gn is not None:
        table, x2, gn_silu = gn
        if x2 is not None:
            if x2.shape[:3] != x.shape[:3]:
                raise ValueError(f"conv: x2 {tuple(x2.shape)} does not match x {tuple(x.shape)}")
            Cin = C1 + x2.shape[-1]
        if table.dtype != torch.float32 or tuple(table.shape) != (B, 2, Cin):
            raise ValueError(f"conv: gn table {tuple(table.shape)} {table.dtype} is not a float32 [{B}, 2, {Cin}]")
    if pad is None:
        pad = ksize // 2
    Hin, Win = (2 * H, 2 * W_) if ups else (H, W_)
    Ho = (Hin + 2 * pad - ksize) // stride + 1
    Wo = (Win + 2 * pad - ksize) // stride + 1
    if out_hw is not None:
        Ho, Wo = out_hw
    phase = ups == 2
    pol = _POLICY[0]
    if phase:
        if gn is not None or gn_fuse is not None:
            raise ValueError("conv: ups=2 cannot be combined with gn= / gn_fuse=")
        if ksize != 3 or w.dim() != 3 or tuple(w.shape[::2]) != (4, 4 * Cin):
            raise ValueError(f"conv: ups=2 takes the folded weight [4, N, {4 * Cin}] of a 3x3 convolution, got {tuple(w.shape)}")
        N = w.shape[1]
        fold_key = ops.ups_fold_key(x, N, act, bias, out, gn_out)
        if fold_key in ops._DECLINED:
            return None
        allowed = (stride, pad) == (1, 1) and Cin % 64 == 0 and (H * W_) % 256 == 0 and (N % 160 == 0 or N % 128 == 0) and \
            act != ACT_GEGLU and rowvec is None and res is None
        if not pol.answer("ups2", allowed):
            ops._DECLINED.add(fold_key)
            return None
        y = _phase_conv(x, w, bias, act)
    else:
        N, K, _ = ops._rows(w)
        if K != ksize * ksize * Cin:
            raise ValueError(f"conv: packed weight K {K} != {ksize}*{ksize}*{Cin}")
    M = B * Ho * Wo
    if out is not None and (out.shape[-1] != N or out.numel() != M * N):
        raise ValueError(f"conv: out {tuple(out.shape)} cannot hold [{B},{Ho},{Wo},{N}]")
    rpv = Ho * Wo if rows_per_rv is None else rows_per_rv
    key = None
    if gn_fuse is not None:
        if gn is not None or gn_out:
            raise ValueError("conv: gn_fuse cannot be combined with gn= / gn_out=")
        g_gamma, g_beta, g_eps, g_silu, g_keep = gn_fuse
        ldr = 0 if res is None else ops._rows(res)[2]
        key = (B, H, W_, Cin, N, ksize, stride, pad, bool(ups), Ho, Wo, act, rowvec is not None, None if rowvec is None else rpv,
               res is not None, int(x.stride(2)), N if out is None else int(ops._rows(out)[2]), int(ldr), str(x.device))
        if key in ops._DECLINED:
            return None
        if g_gamma.numel() != N or g_beta.numel() != N:
            raise ValueError(f"conv: gn_fuse gamma / beta must have {N} entries")
        # the header's conditions; "where the library splits K (it decides; M small)": at most 2048 rows here
        rows = Ho * Wo
        allowed = N % 160 == 0 and (N // 32) % 4 == 0 and 20 <= N // 32 <= 256 and rows * (N // 128) <= 8192 and \
            (M // rows) * 32 >= 128 and (rowvec is None or rpv % rows == 0 or rpv >= M) and act != ACT_GEGLU and M <= 2048
        if not pol.answer("gn_fuse", allowed):
            ops._DECLINED.add(key)
            return None
    if not phase:
        c = _case(kind="conv", M=M, N=N, K=ksize * ksize * Cin, act=act, rows_per_rv=rpv,
                  geom=(ksize, stride, pad, 1 if ups else 0, Ho, Wo), gn_pro=None if gn is None else (None, bool(gn_silu)))
        p = dict(case=c, A=x, A2=x2, W=w.reshape(N, -1), bias=bias, gn_table=table,
                 rowvec=None if rowvec is None else rowvec.reshape(-1, rowvec.shape[-1]),
                 R=None if res is None else res.reshape(-1, res.shape[-1]))
        y = KR.gemm_ref(p)["out"]
    if gn_fuse is not None:
        raw = _h(y).reshape(M, N)
        yn = KR.groupnorm_ref(raw, None, B, Ho * Wo, 32, g_gamma, g_beta, g_eps, g_silu)
        kept = ops._written(_put(out, raw, (B, Ho, Wo, N))) if g_keep else None
        return kept, _h(yn).reshape(B, Ho, Wo, N).contiguous()
    out = _put(out, y, (B, Ho, Wo, N))
    gst = None
    if gn_out and gn is None and ops.gn_stats_wanted(B, Ho * Wo, N) and Cin % 64 == 0:
        gst = _gn_stats_of(out.reshape(M, N))
    return ops._written(out, gst)


def conv_narrow(x, w, ksize, *, stride=1, pad=None, bias=None, rowvec=None, res=None, act=ACT_NONE, ho=None, wo=None, out=None,
                gn_out=False):
    if pad is None:
        pad = ksize // 2
    B = x.shape[0]
    col = KR.im2col_ref(x, ksize, stride, pad, w.shape[1], ho, wo)
    H, W_ = x.shape[1:3]
    Ho = (H + 2 * pad - ksize) // stride + 1 if ho is None else ho
    Wo = (W_ + 2 * pad - ksize) // stride + 1 if wo is None else wo
    N = w.shape[0]
    o2 = None if out is None else out.view(-1, out.shape[-1])
    gn_out = bool(gn_out) and ops.gn_stats_wanted(B, Ho * Wo, N) and ops.wide_tile_ok(N, w.shape[1])
    y = gemm(col, w, bias=bias, rowvec=rowvec, rows_per_rv=Ho * Wo, res=res, act=act, out=o2, gn_out=gn_out)
    r = y.view(B, Ho, Wo, N) if out is None else out
    return ops._written(r, ops.get_gn_stats(y) if gn_out else None)


# ----------------------------------------------------------------------------------------------
# attention, normalisation
# ----------------------------------------------------------------------------------------------
def attention(q, k, vt, B, H, Nq, Nk, D, scale, *, ldq, ldk, ldvt, q_bs, k_bs, vt_bs, out=None):
    if D not in (40, 80, 96, 160, 512) or ldq % 8 or ldk % 8 or ldvt % 8 or vt_bs % 8:
        raise ValueError(f"attention: D {D} / leading dimensions outside the contract of pfd_attention_f16")
    if D == 512 and (H != 1 or Nk % 32):
        raise ValueError(f"attention: D 512 needs H == 1 and Nk % 32 == 0 (H {H}, Nk {Nk}; PFD_ESHAPE: include/pfd_hip.h)")
    y = KR.attention_ref(q, k, vt, B, H, Nq, Nk, D, scale, ldq=ldq, ldk=ldk, ldvt=ldvt, q_bs=q_bs, k_bs=k_bs, vt_bs=vt_bs)
    y = _h(y).reshape(B * Nq, H * D)
    if out is None:
        return y.contiguous()
    out[:B * Nq, :H * D].copy_(y)
    return out


def swin_window_attention(qkv, qkv_bias, rpb, B, H, W_, Cdim, nH, ws, shift, scale, out=None):
    """pfd_swin_window_attention_f16: window 12, head width 32, with the refusals of the library.  The result is rounded once;
    the kernel's fp16 store of the normalised probabilities (profiles/encoder_kernel_tests.md: at most 2^-11 vmax) is not
    restated here -- profiles/encoder_vae_block_tests.md says what that costs against T"""
    assert qkv.dtype == torch.float16
    if ws != KR.WS or Cdim != KR.HD * nH:
        raise ValueError(f"swin_window_attention: window {ws} / C {Cdim} with {nH} heads (built for window 12, C == 32 nH: PFD_ESHAPE)")
    if not 0 <= shift < KR.WS:
        raise ValueError(f"swin_window_attention: shift {shift} outside [0, 12) (PFD_EINVAL)")
    if tuple(qkv.shape) != (B * H * W_, 3 * Cdim) or not qkv.is_contiguous():
        raise ValueError(f"swin_window_attention: qkv {tuple(qkv.shape)} is not a dense [{B * H * W_}, {3 * Cdim}]")
    if out is not None and (tuple(out.shape) != (B * H * W_, Cdim) or not out.is_contiguous()):
        raise ValueError(f"swin_window_attention: out {tuple(out.shape)} is not a dense [{B * H * W_}, {Cdim}]")
    y = KR.swin_window_attention_ref(qkv, qkv_bias, rpb, B, H, W_, nH, shift, scale)
    return ops._written(_put(out, y, (B * H * W_, Cdim)))


def _from_pstats(x, x2, st1, st2, B, HW, gamma, beta, eps, silu):
    """pfd_groupnorm_pstats_f16: GroupNorm(32) of [x | x2] from the producers' gn_out arrays (sum, sum of squares per 64-row slab
    and producer group of C_src / 32 channels)"""
    C1 = x.shape[-1]
    C2 = 0 if x2 is None else x2.shape[-1]
    C = C1 + C2
    cpg = C // 32

    def sums(st, Cs):
        cpp = Cs // 32
        pg = torch.arange(32)
        v = st.double().reshape(B, HW // 64, Cs // 160, 16, 2).sum(1)              # [B, tile, slot, 2]
        v = v[:, (pg * cpp) // 160, ((pg * cpp) % 160) // cpp]                     # [B, 32 producer groups, 2]
        return v.reshape(B, Cs // cpg, cpg // cpp, 2).sum(2)                       # per group of THIS norm
    s = sums(st1, C1)
    if x2 is not None:
        s = torch.cat([s, sums(st2, C2)], 1)
    n = float(HW * cpg)
    mean = s[..., 0] / n
    var = (s[..., 1] / n - mean * mean).clamp_min(0)
    v = KR._gn_cat(x.reshape(B * HW, C1), None if x2 is None else x2.reshape(B * HW, C2), B, HW, torch.float64)
    gi = torch.arange(C) // cpg
    y = (v - mean[:, gi][:, None]) / torch.sqrt(var + eps)[:, gi][:, None] * gamma.double() + beta.double()
    return (F.silu(y) if silu else y).reshape(B * HW, C)


def groupnorm(x, gamma, beta, groups, eps, *, x2=None, silu=False, out=None):
    assert x.dtype == torch.float16
    B, C1 = x.shape[0], x.shape[-1]
    HW = x.numel() // (B * C1)
    C2 = 0 if x2 is None else x2.shape[-1]
    st1 = ops.get_gn_stats(x) if ops.GN_PSTATS else None
    st2 = ops.get_gn_stats(x2) if (ops.GN_PSTATS and x2 is not None) else None
    x1m = x.reshape(B * HW, C1)
    x2m = None if x2 is None else x2.reshape(B * HW, C2)
    if st1 is not None and (x2 is None or st2 is not None) and groups == 32 and _lib().pfd_groupnorm_takes_pstats(B, C1, C2, HW, groups):
        y = _from_pstats(x, x2, st1, st2, B, HW, gamma, beta, eps, silu)
    else:
        y = KR.groupnorm_ref(x1m, x2m, B, HW, groups, gamma, beta, eps, silu)
    return ops._written(_put(out, y, tuple(x.shape[:-1]) + (C1 + C2,)))


def groupnorm_table(x, gamma, beta, groups, eps, *, x2=None):
    B, C1 = x.shape[0], x.shape[-1]
    HW = x.numel() // (B * C1)
    x2m = None if x2 is None else x2.reshape(B * HW, -1)
    return KR.groupnorm_table_ref(x.reshape(B * HW, C1), x2m, B, HW, groups, gamma, beta, eps).float().contiguous()


def layernorm(x, gamma, beta, eps=1e-5, out=None):
    assert x.dtype == torch.float16
    return ops._written(_put(out, KR.layernorm_ref(x, gamma, beta, eps), x.shape))


def layernorm_patch_merge(x, gamma, beta, eps=1e-5):
    assert x.dtype == torch.float16
    return _h(KR.layernorm_patch_merge_ref(x, gamma, beta, eps)).contiguous()


def softmax_rows(x, scale, out=None):
    """pfd_softmax_rows_f16; out may be x itself (the row is read whole before it is written)"""
    assert x.dtype == torch.float16
    R, N, _ = ops._rows(x)
    return _put(out, KR.softmax_rows_ref(x.reshape(R, N), scale), (R, N))


def ln_rowstats(x, out=None):
    M, Cc, _ = ops._rows(x)
    out = ops._row_stats("ln_rowstats: out", "M, C/160, 2", M, Cc, x.device, out)
    out.copy_(KR.ln_out_ref(x.reshape(M, Cc)).float())
    return out


# ----------------------------------------------------------------------------------------------
# boundary / elementwise
# ----------------------------------------------------------------------------------------------
def to_nhwc(x, mul=1.0, add=0.0, rep=1):
    if x.dtype not in (torch.float32, torch.float16):
        x = x.float()
    return _h(KR.to_nhwc_ref(x, mul, add, rep))


def to_nchw(x, dtype=torch.float16, mul=1.0, add=0.0, lo=-65504.0, hi=65504.0):
    if not x.is_contiguous():
        raise ValueError("to_nchw: dense NHWC expected")
    y = KR.to_nchw_ref(x, mul, add, lo, hi)
    return y.float() if dtype == torch.float32 else _h(y).to(dtype)


def timestep_embedding(t, dim, max_period=10000.0):
    return _h(KR.timestep_embedding_ref64(t.to(torch.int64), dim, max_period))


def add(a, b, out=None):
    if not (a.is_contiguous() and b.is_contiguous()):
        raise ValueError("add: dense tensors expected")
    if a.numel() != b.numel() or (out is not None and out.numel() != a.numel()):
        raise ValueError(f"add: operand sizes differ ({tuple(a.shape)} vs {tuple(b.shape)}); no broadcasting")
    return ops._written(_put(out, a.double() + b.double().reshape(a.shape), a.shape))


def axpby(a, alpha, b=None, beta=0.0, out=None):
    if (b is not None and b.numel() != a.numel()) or (out is not None and out.numel() != a.numel()):
        raise ValueError("axpby: operand sizes differ; no broadcasting")
    return ops._written(_put(out, KR.axpby_ref(a, float(alpha), b, float(beta)), a.shape))


def add_rowvec(x, v, out=None, ln_out=None):
    R, Cc, _ = ops._rows(x)
    out = _put(out, x.double() + v.double(), x.shape)
    if ln_out is not None:
        ln_out = ops._row_stats("add_rowvec: ln_out", "R, C/160, 2", R, Cc, x.device, ln_out)
        ln_out.copy_(KR.ln_out_ref(out.reshape(R, Cc)).float().reshape(ln_out.shape))
    return ops._written(out)


def activation(x, act, out=None):
    if not x.is_contiguous():
        raise ValueError("activation: dense tensor expected")
    return ops._written(_put(out, KR.activation_ref(x, act), x.shape))


def _fell_through(*a, **k):
    FELL_THROUGH.append("a launch reached the real library")
    raise AssertionError("host layer on the stand-in: a call fell through to the real library")


STANDIN = ("gemm", "conv", "conv_narrow", "attention", "swin_window_attention", "groupnorm", "groupnorm_table", "layernorm",
           "layernorm_patch_merge", "softmax_rows", "ln_rowstats", "to_nhwc", "to_nchw", "timestep_embedding", "add", "axpby",
           "add_rowvec", "activation")


def install(monkeypatch, policy=None):
    """patch lib.hip.ops for this test: the functions above, the one device guard, and a trap on the launch helpers of the real
    wrappers.  The decline memory is emptied and restored with the patches."""
    _POLICY[0] = policy or Policy()
    del FELL_THROUGH[:]
    g = globals()
    for name in STANDIN:
        monkeypatch.setattr(ops, name, g[name])
    monkeypatch.setattr(ops, "_stream", _fell_through)
    monkeypatch.setattr(ops, "_launch", _fell_through)
    monkeypatch.setattr(ops, "_workspace", _fell_through)
    monkeypatch.setattr(ops, "_DECLINED", set())
    monkeypatch.setattr(layers, "_require_gpu", lambda t, message: None)
    return _POLICY[0]


def set_policy(policy):
    _POLICY[0] = policy
    return policy


# ----------------------------------------------------------------------------------------------
# running a case of tests/block_refs.py over the stand-in
# ----------------------------------------------------------------------------------------------
_FLOOR = {}


def run_standin(case, mode="serve", census=False, fwd=False):
    """the case through the real .hip methods over the stand-in, in a patch context of its own -> (output, census | None, policy).
    With census=True the case runs twice (the first run builds the weight packs) and the second run is recorded from an empty
    decline memory."""
    import pytest
    import block_refs as BR
    b = BR.built(case["id"])
    with pytest.MonkeyPatch.context() as mp:
        pol = install(mp, Policy(mode))
        BR.apply_switches(mp, case["switches"])
        mods, inputs = BR._dev(b, "cpu")
        run = b.fwd if fwd else b.run
        b.ln_carried = b.gn_carried = None          # (what the tests read afterwards belongs to THIS run)
        y = run(mods, inputs).detach().clone()
        cen = None
        if census:
            ops._DECLINED.clear()
            pol = set_policy(Policy(mode))
            cen = BR.Census().install(mp)
            y2 = run(mods, inputs)
            assert torch.equal(y, y2), "second run over the stand-in differs"
            assert isinstance(pol.mode, str) or not pol.mode, f"recorded answers left over: {pol.mode}"
            # (the further run asks again only what was served: the declines are in the memory)
            set_policy(Policy(mode if isinstance(mode, str) else [d for d in mode if d]))
            cen.rerun(lambda: run(mods, inputs))
        assert not FELL_THROUGH, FELL_THROUGH
    return y, cen, pol


def floor(case, fwd=False):
    """f: the error of the stand-in run (every optional form served) against the fp64 formula, in units of 2^-11 -- what rounding
    at the documented stores alone costs.  The tolerance of the case is T = 4 f.  (case: a row of block_refs.CASES, or a copy with
    other switches; fwd: the .forward calling convention)"""
    import block_refs as BR
    key = (case["id"], tuple(sorted(case["switches"].items())), fwd)
    if key not in _FLOOR:
        b = BR.built(case["id"])
        f = BR.err_units(run_standin(case, fwd=fwd)[0], BR.ref_of(b, fwd), b.B)
        # a floor is a handful of fp16 roundings; one far above that means the host path itself is wrong under these switches,
        # and a tolerance derived from it would admit the same error on the device
        assert 0 < f < 16, f"floor {f} of {key}: the stand-in run of the host path is far from the fp64 formula"
        _FLOOR[key] = f
    return _FLOOR[key]
