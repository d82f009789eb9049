"""Tensor-level wrappers over the C ABI (binding.py): torch is used here for device memory and
the current HIP stream only -- every arithmetic op below is a hand-written gfx950 kernel.

Layout convention of the whole product path: activations are fp16, token-major / NHWC
(`[B, H, W, C]` or `[M, C]`, channel stride 1, row stride `ld`).  NCHW exists only at the
reference API boundary (ops.to_nhwc / ops.to_nchw).
"""
import ctypes as C
import functools
import os
import threading

import torch

from . import binding as _b
from .binding import ACT_GEGLU, ACT_GELU, ACT_NONE, ACT_RELU, ACT_SILU  # noqa: F401

_byref = C.byref


def _lib():
    return _b.load()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _ptr(t):
    return t.data_ptr() if t is not None else None


# The reference's models are called from Gradio worker threads on ONE shared global model with no lock
# (app.py:277, 405-410).  Everything here runs on the current stream and shares per-device scratch (the
# split-K slabs below, the per-layer packed-weight caches, captured hipGraphs with static input buffers),
# so every public entry point of the product path (composite model methods, DDIMSampler, the pipeline)
# holds this re-entrant lock for the duration of its launch sequence: concurrent requests serialise
# instead of interleaving a GEMM and its split-K reduce with another thread's GEMM.
DEVICE_LOCK = threading.RLock()


def serialised(fn):
    @functools.wraps(fn)
    def wrapper(*a, **k):
        with DEVICE_LOCK:
            return fn(*a, **k)
    return wrapper


_WS = {}
_WS_BYTES = 96 << 20


def _workspace(device):
    """per-device scratch for split-K GEMMs (the library keeps f16 partial sums in it since round 6; sized at 4 bytes per element as ABI 9 requires) (stable address for hipGraphs; launch sequences are serialised by
    DEVICE_LOCK and run on one stream, so one slab per device suffices)"""
    ws = _WS.get(device)
    if ws is None:
        ws = _WS[device] = torch.empty(_WS_BYTES, dtype=torch.uint8, device=device)
    return ws


_TRACE = os.environ.get("PFD_TRACE_GEMM")
_TRACE_GN = os.environ.get("PFD_TRACE_GN")
# False: every LayerNorm is its own launch again (tests flip it per call; the round-3 A/B: -52 ms per batch for the fold)
LN_FOLD = True


# One record per GEMM / conv launch: THE field list of profiles/unet_c2_gemm_shapes.txt.  The writer below, the readers in
# tests/test_hip_kernels_fullsize.py (parse_launch_records) and csrc/selftest_replay.cpp (--replay: 19, 22 or 24 integers per line) follow
# it; tests/test_host.py parses the tracked file with it on CPU, so a regenerated file cannot break a GPU-only test unseen.
TRACE_FIELDS = ("M", "N", "K", "act", "has_bias", "has_rowvec", "has_res", "bias_per_row",
                "ksize", "stride", "pad", "ups", "B", "H", "W", "Cin", "Ho", "Wo", "rows_per_rv",
                "k_split", "zero_rows", "gn_out", "gnf", "res_rows")
TRACE_FIELDS_ABI7 = 19      # rounds 1-3 wrote the first 19 (k_split = zero_rows = gn_out = 0)
TRACE_FIELDS_ABI8 = 22      # rounds 4-5 the first 22 (ABI 9's gnf = 0 | 1 keeps the raw result | 2 skips it, res_rows = 0: ADVICE r05)


def trace_record(d):
    """the TRACE_FIELDS of a PfdGemmDesc, as ints"""
    return tuple(int(v) for v in (
        d.M, d.N, d.K, d.act, d.bias is not None, d.rowvec is not None, d.R is not None, d.bias_per_row,
        d.ksize, d.stride, d.pad, d.ups, d.B, d.H, d.Wd, d.Cin, d.Ho, d.Wo, d.rows_per_rv,
        d.k_split, d.zero_rows, bool(d.gn_out), (2 if d.gnf_skip_raw else 1) if d.gnf_y else 0, d.res_rows))


def parse_launch_records(path, distinct=True):
    """[LaunchRecord] of a PFD_TRACE_GEMM file (19-field lines of older rounds are padded with zeros)"""
    import collections
    Rec = collections.namedtuple("LaunchRecord", TRACE_FIELDS)
    seen, out = set(), []
    for ln, line in enumerate(open(path), 1):
        v = tuple(int(t) for t in line.split())
        if not v:
            continue
        if len(v) in (TRACE_FIELDS_ABI7, TRACE_FIELDS_ABI8):
            v = v + (0,) * (len(TRACE_FIELDS) - len(v))
        if len(v) != len(TRACE_FIELDS):
            raise ValueError(f"{path}:{ln}: {len(v)} fields, expected {len(TRACE_FIELDS)} ({' '.join(TRACE_FIELDS)})")
        if distinct and v in seen:
            continue
        seen.add(v)
        out.append(Rec(*v))
    return out


def _trace(d):
    """PFD_TRACE_GEMM=<file>: append one line per GEMM/conv launch (shape replay for tools/selftest --replay,
    used to measure HBM traffic with rocprofv3 --pmc on a torch-free process)"""
    with open(_TRACE, "a") as f:
        f.write(" ".join(str(v) for v in trace_record(d)) + "\n")


# Requests the library declined once under its heuristic (it decides whether a problem splits K, which upsample shapes the
# phase form serves): not asked again.  Keys: everything the decision depends on (conv(gn_fuse=...): built there; conv(ups=2):
# ups_fold_key).
_DECLINED = set()


def _launch(d, tile, label, decline_key=None):
    """the one GEMM / conv launch: pfd_gemm_f16 (tile 0: the library's heuristic) or pfd_gemm_f16_ex.  True when it launched (and
    left its PFD_TRACE_GEMM record).  decline_key: the caller has another way to run the request -- PFD_ESHAPE (nothing was
    launched, nothing written: include/pfd_hip.h) then returns False and, for a heuristic call, remembers the key (a decline
    under a forced tile says nothing about the heuristic's choice)."""
    lib = _lib()
    rc = lib.pfd_gemm_f16_ex(_byref(d), tile, _stream()) if tile else lib.pfd_gemm_f16(_byref(d), _stream())
    if decline_key is not None and rc == _b.PFD_ESHAPE:
        if tile == 0:
            _DECLINED.add(decline_key)
        return False
    _b.check(rc, label)
    if _TRACE:
        _trace(d)
    return True


def _gemm_desc(a, w, out, M, N, K, lda, ldw, bias, rowvec, res):
    """PfdGemmDesc with the fields gemm() and conv() share: operands, epilogue vectors, leading dimensions, sizes, workspace"""
    d = _b.PfdGemmDesc()
    d.A, d.W, d.C = a.data_ptr(), w.data_ptr(), out.data_ptr()
    d.bias, d.rowvec, d.R = _ptr(bias), _ptr(rowvec), _ptr(res)
    d.lda, d.ldw, d.ldc = lda, ldw, _rows(out)[2]
    d.ldr = _rows(res)[2] if res is not None else 0
    d.ldrv = _rows(rowvec)[2] if rowvec is not None else 0
    d.M, d.N, d.K = M, N, K
    d.ws, d.ws_bytes = _workspace(a.device).data_ptr(), _WS_BYTES
    return d


def _chk16(t, what):
    if t.dtype != torch.float16:
        raise TypeError(f"{what}: expected float16, got {t.dtype}")
    if not t.is_cuda:
        raise RuntimeError(f"{what}: tensor is on {t.device}; the HIP path has no CPU fallback")
    if t.stride(-1) != 1:
        raise ValueError(f"{what}: innermost stride must be 1")


def _rows(t):
    """(rows, cols, ld) of a tensor viewed as a row-major matrix with unit column stride."""
    cols = t.shape[-1]
    if t.dim() == 1:
        return 1, cols, cols
    ld = t.stride(-2)
    rows = t.numel() // cols
    # all leading dims must be collapsible onto the row stride
    exp = ld
    for d in range(t.dim() - 2, -1, -1):
        if t.shape[d] != 1 and t.stride(d) != exp:
            raise ValueError(f"tensor of shape {tuple(t.shape)} strides {t.stride()} is not a strided matrix")
        exp *= t.shape[d]
    return rows, cols, ld


# ----------------------------------------------------------------------------------------------
# GEMM / convolution
# ----------------------------------------------------------------------------------------------
def ln_fold_ok(C):
    """widths whose LayerNorm can be folded into the consumer GEMM (PfdGemmDesc.ln_stats: 160-column slices, <= 8; the
    contraction must not need K padding -- pack_matrix pads K to 64 and the fold's gamma has C entries)"""
    return LN_FOLD and C % 160 == 0 and C // 160 <= 8 and C % 64 == 0


def ln_out_arg(ln_out):
    """the ln_out keyword of gemm / Conv2d.hip / Linear.hip -- None | False (no statistics), True (allocate) or a float32
    tensor -- with "none" spelled one way: None"""
    return None if ln_out is False else ln_out


def _row_stats(what, dims, rows, cols, device, given=None):
    """the float32 [rows, cols / 160, 2] partial row sums (the layout gemm(ln=...) takes): `given` checked, or a new tensor"""
    if given is None or given is True:
        return torch.empty((rows, cols // 160, 2), dtype=torch.float32, device=device)
    if given.dtype != torch.float32 or not given.is_contiguous() or given.numel() != rows * (cols // 160) * 2:
        raise ValueError(f"{what} must be a contiguous float32 [{dims}]")
    return given


def ln_rowstats(x, out=None):
    """partial row sums [M, C/160, 2] (fp32) of a token matrix, in the layout gemm(ln=...) takes -- for tensors that
    were not written by a gemm(ln_out=...) launch"""
    _chk16(x, "ln_rowstats x")
    M, Cc, ld = _rows(x)
    out = _row_stats("ln_rowstats: out", "M, C/160, 2", M, Cc, x.device, out)
    _b.check(_lib().pfd_ln_rowstats_f16(x.data_ptr(), ld, M, Cc, out.data_ptr(), _stream()), "pfd_ln_rowstats_f16")
    return out


# GroupNorm statistics from the producers (PfdGemmDesc.gn_out / pfd_groupnorm_pstats_f16); PFD_GN_PSTATS=0: every
# two-launch GroupNorm reads its input for statistics again (A/B runs)
GN_PSTATS = True


def gn_stats_wanted(B, HW, N, M=None):
    """should the launch that writes a [B, HW, N] tensor also emit GroupNorm(32) statistics of it?  Yes where a GroupNorm
    over these channels (alone or as one source of a skip concat) takes the two-launch form and the wide-tile kernels
    can form them (N = 320 | 640 | 1280, whole 64-row slabs per sample)."""
    if not GN_PSTATS or N not in (320, 640, 1280) or HW % 64 or (M is not None and M != B * HW):
        return False
    return bool(_lib().pfd_groupnorm_takes_pstats(B, N, 0, HW, 32))


def _new_gn_stats(M, N, device):
    return torch.empty((M // 64, N // 160, 16, 2), dtype=torch.float32, device=device)


def set_gn_stats(t, stats):
    """attach the producer's statistics to the tensor OBJECT that holds its output (views / copies do not inherit them)"""
    t._pfd_gn = (stats, t.data_ptr(), tuple(t.shape), t._version)
    return t


def get_gn_stats(t):
    """the statistics the producer of `t` emitted, or None (also when the object was re-pointed since)"""
    ent = getattr(t, "_pfd_gn", None)
    if ent is None or ent[1] != t.data_ptr() or ent[2] != tuple(t.shape) or ent[3] != t._version:
        return None       # (the version counter also moves on torch in-place ops and writes through a view of this tensor)
    return ent[0]


def _written(out, stats=None):
    """every op that writes into a caller-provided `out` goes through here: the tensor object carries the statistics of
    THIS write or none (stale producer statistics would be normalised with silently).  A write through a VIEW of a
    statistics-carrying tensor invalidates them through the shared version counter (get_gn_stats / get_normed compare it)."""
    if out is not None:
        # the library wrote through a raw pointer: tell torch (the version counter is shared by every view of the storage), so
        # that statistics / normalised copies riding on ANOTHER object over these bytes -- ControlNet's `add(h[b:b+1], g,
        # out=h[b:b+1])` writes through a view of h -- stop matching
        torch._C._increment_version((out,))     # (an iterable of tensors: a bare tensor is iterated row by row)
    if stats is not None:
        set_gn_stats(out, stats)
    elif out is not None and getattr(out, "_pfd_gn", None) is not None:
        out._pfd_gn = None
    if out is not None and getattr(out, "_pfd_normed", None) is not None:
        out._pfd_normed = None
    return out


def set_normed(t, key, y):
    """attach the GroupNorm of `t` that its producer already computed (conv(gn_fuse=...)): key = (id of the norm module's
    gamma storage, eps, silu).  Rides on the tensor OBJECT like the statistics; any rewrite of the object drops it."""
    t._pfd_normed = (key, t.data_ptr(), tuple(t.shape), y, t._version)
    return t


def get_normed(t, key):
    ent = getattr(t, "_pfd_normed", None)
    if ent is None or ent[0] != key or ent[1] != t.data_ptr() or ent[2] != tuple(t.shape) or ent[4] != t._version:
        return None       # (a torch in-place op or a write through a view bumps the version -> recompute)
    return ent[3]


def cat_pair(t):
    """torch.cat([t, t]) of a CFG pair, statistics included (per-sample slabs: the copy's are the original's)"""
    out = torch.cat([t, t])
    st = get_gn_stats(t)
    if st is not None:
        set_gn_stats(out, torch.cat([st, st]))
    return out


# ABI 8 forms (PfdGemmDesc.k_split / zero_rows); PFD_GEMM_FUSE=0 keeps the two-launch forms (A/B runs)
GEMM_FUSE = True


def wide_tile_ok(N, K):
    """shapes the wide-tile linear kernels take (they alone serve gemm(a2=...) / gemm(zero_rows=...))"""
    return GEMM_FUSE and (N % 160 == 0 or N % 128 == 0) and K % 64 == 0


def gemm(a, w, *, bias=None, rowvec=None, rows_per_rv=1, res=None, act=ACT_NONE, out=None,
         bias_per_row=False, n=None, k=None, tile=0, out_t=None, n_split=None, ln=None, ln_out=None,
         a2=None, zero_rows=0, gn_out=False, res_rows=None, w_tiled=False):
    """out[M, N] = epi(a[M, K] @ w[N, K]^T); see pfd_gemm_f16 in include/pfd_hip.h.
    a2: second source of the contraction -- the operand is the virtual column concat [a | a2] (K = Ka + Ka2; the
    1x1 skip convolution over a skip concat).  zero_rows: that many all-zero operand rows come in front of a's rows
    (M = zero_rows + rows of a); their result is epi(0).  Both: wide-tile kernels only (wide_tile_ok).
    gn_out: the launch also emits the GroupNorm statistics of its output (PfdGemmDesc.gn_out); they ride on the returned
    tensor (get_gn_stats).
    res_rows: `res` holds that many rows and is the residual of BOTH halves of a doubled batch (M == 2 * res_rows; the CFG
    pair [x | x] stored once, PfdGemmDesc.res_rows).  Wide-tile kernels only.
    out_t / n_split: columns >= n_split go, transposed, to out_t[N - n_split, M] (wide-tile path only).
    ln = (stats, colsum, eps): LayerNorm of `a` folded into the contraction (w is the gamma-scaled weight, bias is b';
    PfdGemmDesc.ln_stats).  ln_out: True (allocate) or a float32 [M, N/160, 2] tensor -> the partial row sums of the
    OUTPUT are written there and (out, stats) is returned.
    w_tiled: `w` holds the K-tile-contiguous pack of the [N, K] weight (PfdGemmDesc.w_tiled; the caller packs it) -- a contiguous
    [N, K] tensor whose memory is [N / T][K / 64][T][64], T = 160 if N % 160 == 0 else 128.  Wide-tile kernels only."""
    _chk16(a, "gemm A")
    _chk16(w, "gemm W")
    M, Ka, lda = _rows(a)
    Nw, Kw, ldw = _rows(w)
    N = Nw if n is None else n
    K = min(Ka, Kw) if k is None else k
    if a2 is not None:
        _chk16(a2, "gemm A2")
        M2, Ka2, lda2 = _rows(a2)
        if M2 != M or a2.device != a.device:
            raise ValueError(f"gemm: a2 {tuple(a2.shape)} does not pair with a {tuple(a.shape)}")
        if k is None:
            K = Ka + Ka2
        if Ka % 64 or Ka >= K or K - Ka > Ka2:
            raise ValueError(f"gemm: a2 needs a first source of a multiple of 64 columns below K (Ka {Ka}, K {K})")
    if zero_rows:
        if zero_rows < 0 or ln is not None:
            raise ValueError("gemm: zero_rows must be >= 0 and cannot be combined with ln=")
        M += zero_rows
    n_out = N // 2 if act == ACT_GEGLU else N
    if out_t is not None:
        n_out = n_split
    if out is None:
        out = torch.empty((M, n_out), dtype=torch.float16, device=a.device)
    else:
        _chk16(out, "gemm out")
        if out.device != a.device or out.shape[-1] != n_out or out.numel() != M * n_out:
            raise ValueError(f"gemm: out {tuple(out.shape)} on {out.device} cannot hold [{M}, {n_out}] on {a.device}")
    d = _gemm_desc(a, w, out, M, N, K, lda, ldw, bias, rowvec, res)
    if out_t is not None:
        _chk16(out_t, "gemm out_t")
        if out_t.shape[0] != N - n_split or out_t.shape[1] < M or out_t.stride(1) != 1:
            raise ValueError(f"gemm: out_t {tuple(out_t.shape)} cannot hold [{N - n_split}, {M}]")
        d.Ct, d.ldct, d.n_split = out_t.data_ptr(), out_t.stride(0), n_split
    d.rows_per_rv, d.act, d.bias_per_row = rows_per_rv, act, 1 if bias_per_row else 0
    d.ksize = 0
    if w_tiled:
        if not w.is_contiguous() or (N % 160 and N % 128) or K % 64 or (Nw, Kw) != (N, K):
            raise ValueError(f"gemm: w_tiled takes the contiguous pack of a whole [N, K] weight, N % 160 == 0 or N % 128 == 0 (w {tuple(w.shape)})")
        d.w_tiled = 1
    if a2 is not None:
        d.A2, d.lda2, d.k_split = a2.data_ptr(), lda2, Ka
    d.zero_rows = zero_rows
    if res_rows is not None:
        if res is None or M != 2 * res_rows or _rows(res)[0] != res_rows:
            raise ValueError(f"gemm: res_rows {res_rows} needs a residual of exactly that many rows and M == 2 * res_rows (M {M})")
        d.res_rows = res_rows
    elif res is not None and _rows(res)[0] != M:
        raise ValueError(f"gemm: residual of {_rows(res)[0]} rows for {M} output rows (res_rows= names a shared one)")
    if ln is not None:
        st, cs, eps = ln
        if st.dtype != torch.float32 or not st.is_contiguous() or st.dim() != 3 or st.shape[0] != M or \
                st.shape[1] * 160 != K or st.shape[2] != 2 or st.device != a.device:
            raise ValueError(f"gemm: ln stats {tuple(st.shape)} {st.dtype} do not describe a [{M}, {K}] operand")
        if cs.dtype != torch.float32 or cs.numel() != N or not cs.is_contiguous() or cs.device != a.device:
            raise ValueError("gemm: ln column sums must be a contiguous float32 [N]")
        d.ln_stats, d.ln_colsum, d.ln_parts, d.ln_eps = st.data_ptr(), cs.data_ptr(), st.shape[1], float(eps)
    stats = None
    ln_out = ln_out_arg(ln_out)
    if ln_out is not None:
        stats = _row_stats("gemm: ln_out", "M, N/160, 2", M, N, a.device, ln_out)
        d.ln_out = stats.data_ptr()
    gst = None
    if gn_out:
        gst = _new_gn_stats(M, N, a.device)
        d.gn_out = gst.data_ptr()
    _launch(d, tile, f"pfd_gemm_f16 M{M} N{N} K{K}")
    _written(out, gst)
    return out if stats is None else (out, stats)


def conv_gn_fusable(B, H, W_, C1, C2, N, ksize=3, stride=1, pad=1):
    """True when conv(..., gn=...) is served (PfdGemmDesc.gn_table: the 3x3 patch kernel) AND pays: at 16-wide
    images GroupNorm is the single-launch small-slab kernel, cheaper than statistics + table."""
    return (ksize == 3 and stride == 1 and pad == 1 and W_ in (32, 64) and H % (256 // W_) == 0 and
            (B * H * W_) % 256 == 0 and N % 160 == 0 and C1 % 64 == 0 and C2 % 64 == 0)


# Upsample convolutions as four 2x2-tap phase convolutions (PfdGemmDesc.ups = 2) where the library serves the shape;
# PFD_UPS_FOLD=0: every upsample convolution runs the 9-tap gather of ups = 1 (A/B runs)
UPS_FOLD = os.environ.get("PFD_UPS_FOLD", "1") != "0"


def ups_fold_key(x, N, act, bias, out, gn_out):
    """everything the library's decision about conv(ups=2) can depend on (heuristic calls only)"""
    return (tuple(x.shape), int(N), int(act), bias is not None, bool(gn_out), int(x.stride(2)),
            int(N) if out is None else int(_rows(out)[2]), str(x.device))


def ups_fold_declined(key):
    return key in _DECLINED


def conv(x, w, ksize, *, stride=1, pad=None, ups=False, bias=None, rowvec=None, res=None, act=ACT_NONE,
         out=None, tile=0, out_hw=None, rows_per_rv=None, gn=None, gn_out=False, gn_fuse=None, w_tiled=False):
    """Implicit-GEMM convolution of an NHWC image x[B,H,W,Cin] (Cin % 64 == 0) with packed
    weights w[N, ksize*ksize*Cin]; returns [B,Ho,Wo,N].  rowvec: [B, N] per-sample vector.
    ups: False | True (nearest-2x upsample fused into the gather of the 9-tap weight, PfdGemmDesc.ups = 1) | 2 (the same
    convolution as four 2x2-tap phase convolutions over the low-res image, PfdGemmDesc.ups = 2: w is the folded pack
    [4, N, 4*Cin] of layers.pack_conv_weight_ups; returns None with NOTHING launched where the library does not serve the
    shape -- the caller runs ups=True with the 9-tap pack).
    gn = (table, x2, silu): GroupNorm(+SiLU) of the virtual concat [x | x2] applied while the input is staged
    (table from groupnorm_table; see PfdGemmDesc.gn_table) -- x is then the UN-normalised tensor.
    gn_fuse = (gamma, beta, eps, silu, keep_raw): GroupNorm(32)(+SiLU) of the OUTPUT inside the launch's split-K reduction
    (PfdGemmDesc.gnf_y, ABI 9).  Returns (raw | None, normalised) when the library serves it, else None with NOTHING launched
    (a problem it does not split, a width the fused reduction is not built for): the caller runs conv + groupnorm.
    w_tiled: `w` holds the K-tile-contiguous pack of the weight (PfdGemmDesc.w_tiled, as for gemm); not with ups=2."""
    _chk16(x, "conv x")
    _chk16(w, "conv W")
    B, H, W_, Cin = x.shape
    x2 = None
    if gn is not None:
        table, x2, gn_silu = gn
        C1 = Cin
        if x2 is not None:
            _chk16(x2, "conv x2")
            if x2.shape[:3] != x.shape[:3] or x2.device != x.device:
                raise ValueError(f"conv: x2 {tuple(x2.shape)} does not match x {tuple(x.shape)}")
            ld2 = x2.stride(2)
            if x2.stride(1) != ld2 * W_ or (B > 1 and x2.stride(0) != ld2 * W_ * H):
                raise ValueError("conv: x2 must be dense over (B, H, W)")
            Cin = C1 + x2.shape[-1]
        if table.dtype != torch.float32 or table.device != x.device or tuple(table.shape) != (B, 2, Cin) or \
                not table.is_contiguous():
            raise ValueError(f"conv: gn table {tuple(table.shape)} {table.dtype} is not a float32 [{B}, 2, {Cin}]")
    if x.stride(2) < x.shape[-1]:
        raise ValueError("conv: bad pixel stride")
    lda = x.stride(2)
    if x.stride(1) != lda * W_ or (B > 1 and x.stride(0) != lda * W_ * H):
        raise ValueError("conv: image must be dense over (B, H, W)")
    if pad is None:
        pad = ksize // 2
    Hin, Win = (2 * H, 2 * W_) if ups else (H, W_)
    Ho = (Hin + 2 * pad - ksize) // stride + 1
    Wo = (Win + 2 * pad - ksize) // stride + 1
    if out_hw is not None:  # asymmetric (bottom/right) zero padding: taps past the image read 0
        Ho, Wo = out_hw
    phase = ups == 2
    if phase:
        if gn is not None or gn_fuse is not None:
            raise ValueError("conv: ups=2 cannot be combined with gn= / gn_fuse=")
        if ksize != 3 or w.dim() != 3 or tuple(w.shape[::2]) != (4, 4 * Cin) or not w.is_contiguous():
            raise ValueError(f"conv: ups=2 takes the folded weight [4, N, {4 * Cin}] of a 3x3 convolution, got {tuple(w.shape)}")
        N, K, ldw = w.shape[1], w.shape[2], w.shape[2]
        fold_key = ups_fold_key(x, N, act, bias, out, gn_out)
        if tile == 0 and fold_key in _DECLINED:
            return None
    else:
        N, K, ldw = _rows(w)
        if K != ksize * ksize * Cin:
            raise ValueError(f"conv: packed weight K {K} != {ksize}*{ksize}*{Cin}")
    M = B * Ho * Wo
    if out is None:
        out = torch.empty((B, Ho, Wo, N), dtype=torch.float16, device=x.device)
    else:
        _chk16(out, "conv out")
        if out.device != x.device or out.shape[-1] != N or out.numel() != M * N:
            raise ValueError(f"conv: out {tuple(out.shape)} on {out.device} cannot hold [{B},{Ho},{Wo},{N}]")
    d = _gemm_desc(x, w, out, M, N, K, lda, ldw, bias, rowvec, res)
    d.rows_per_rv, d.act, d.bias_per_row = (Ho * Wo if rows_per_rv is None else rows_per_rv), act, 0
    d.ksize, d.stride, d.pad, d.ups = ksize, stride, pad, 2 if phase else 1 if ups else 0
    d.B, d.H, d.Wd, d.Cin, d.Ho, d.Wo = B, H, W_, Cin, Ho, Wo
    if w_tiled:
        if phase or not w.is_contiguous() or (N % 160 and N % 128):
            raise ValueError(f"conv: w_tiled takes the contiguous pack of a 9-tap weight, N % 160 == 0 or N % 128 == 0 (w {tuple(w.shape)})")
        d.w_tiled = 1
    if gn is not None:
        d.gn_table, d.gn_c1, d.gn_act = table.data_ptr(), C1, ACT_SILU if gn_silu else ACT_NONE
        if x2 is not None:
            d.A2, d.lda2 = x2.data_ptr(), x2.stride(2)
    gst = None
    if gn_fuse is not None:
        if gn is not None or gn_out:
            raise ValueError("conv: gn_fuse cannot be combined with gn= / gn_out=")
        g_gamma, g_beta, g_eps, g_silu, g_keep = gn_fuse
        # (everything the library's decision can depend on -- residual present, leading dimensions, device --
        #  and only for heuristic calls: a decline under a forced tile says nothing about the heuristic's choice)
        key = (B, H, W_, Cin, N, ksize, stride, pad, bool(ups), Ho, Wo, act, rowvec is not None,
               None if rowvec is None else d.rows_per_rv, res is not None, int(d.lda), int(d.ldc), int(d.ldr), str(x.device))
        if tile == 0 and key in _DECLINED:
            return None
        _chk16(g_gamma, "conv gn_fuse gamma")
        _chk16(g_beta, "conv gn_fuse beta")
        if g_gamma.numel() != N or g_beta.numel() != N:
            raise ValueError(f"conv: gn_fuse gamma / beta must have {N} entries")
        y = torch.empty((B, Ho, Wo, N), dtype=torch.float16, device=x.device)
        d.gnf_gamma, d.gnf_beta, d.gnf_y, d.gnf_ldy = g_gamma.data_ptr(), g_beta.data_ptr(), y.data_ptr(), N
        d.gnf_eps, d.gnf_act, d.gnf_rows, d.gnf_skip_raw = float(g_eps), ACT_SILU if g_silu else ACT_NONE, Ho * Wo, 0 if g_keep else 1
        if not _launch(d, tile, f"pfd_gemm_f16(conv, fused GroupNorm) M{M} N{N} K{K}", key):
            return None
        return (_written(out) if g_keep else None), y
    if gn_out and gn is None and gn_stats_wanted(B, Ho * Wo, N) and Cin % 64 == 0:   # (True = "where a GroupNorm will use them")
        gst = _new_gn_stats(M, N, x.device)
        d.gn_out = gst.data_ptr()
    form = ", phase-folded upsample" if phase else ""
    if not _launch(d, tile, f"pfd_gemm_f16(conv{form}) M{M} N{N} K{K}" + (" with GroupNorm prologue" if gn is not None else ""),
                   fold_key if phase else None):
        return None
    return _written(out, gst)


def im2col(x, ksize, stride, pad, kpad, ho=None, wo=None):
    """[B,H,W,Cin] -> [B*Ho*Wo, kpad] patch matrix (zero padded) for narrow-channel convs."""
    _chk16(x, "im2col x")
    B, H, W_, Cin = x.shape
    Ho = (H + 2 * pad - ksize) // stride + 1 if ho is None else ho
    Wo = (W_ + 2 * pad - ksize) // stride + 1 if wo is None else wo
    col = torch.empty((B * Ho * Wo, kpad), dtype=torch.float16, device=x.device)
    rc = _lib().pfd_im2col_f16(x.data_ptr(), x.stride(2), col.data_ptr(), B, H, W_, Cin, ksize, stride, pad,
                               Ho, Wo, kpad, _stream())
    _b.check(rc, "pfd_im2col_f16")
    return col, Ho, Wo


def conv_narrow(x, w, ksize, *, stride=1, pad=None, bias=None, rowvec=None, res=None, act=ACT_NONE,
                ho=None, wo=None, out=None, gn_out=False):
    """Convolution whose Cin is not a multiple of 64: im2col + GEMM.  w: [N, kpad] packed."""
    if pad is None:
        pad = ksize // 2
    B = x.shape[0]
    col, Ho, Wo = im2col(x, ksize, stride, pad, w.shape[1], ho, wo)
    N = w.shape[0]
    o2 = None if out is None else out.view(-1, out.shape[-1])
    gn_out = bool(gn_out) and gn_stats_wanted(B, Ho * Wo, N) and wide_tile_ok(N, w.shape[1])
    y = gemm(col, w, bias=bias, rowvec=rowvec, rows_per_rv=Ho * Wo, res=res, act=act, out=o2, gn_out=gn_out)
    r = y.view(B, Ho, Wo, N) if out is None else out
    return _written(r, get_gn_stats(y) if gn_out else None)


# ----------------------------------------------------------------------------------------------
# attention
# ----------------------------------------------------------------------------------------------
def _chk_kbias(kbias, kb_bs, B, Nk, device):
    """the key-logit operand of pfd_attention_kbias_f16: fp32 on `device`, dense, 16-byte aligned, rows of kb_bs % 4 == 0
    elements of which the first Nk are read.  -> kb_bs"""
    if not isinstance(kbias, torch.Tensor) or kbias.dtype != torch.float32:
        raise TypeError(f"attention kbias: expected a float32 tensor, got {getattr(kbias, 'dtype', type(kbias).__name__)}")
    if not kbias.is_cuda:
        raise RuntimeError("attention kbias: tensor on the CPU (no CPU fallback)")
    if kbias.device != device:
        raise ValueError(f"attention kbias: on {kbias.device}, the operands are on {device}")
    if not kbias.is_contiguous():
        raise ValueError("attention kbias: must be contiguous")
    if kb_bs is None:
        if kbias.dim() != 2:
            raise ValueError("attention kbias: kb_bs is needed unless kbias is a [B, kb_bs] matrix")
        kb_bs = kbias.shape[1]
    kb_bs = int(kb_bs)
    if kb_bs % 4 or kb_bs < Nk:
        raise ValueError(f"attention kbias: kb_bs {kb_bs} must be a multiple of 4 and at least Nk = {Nk}")
    if kbias.numel() < (B - 1) * kb_bs + Nk:
        raise ValueError(f"attention kbias: {kbias.numel()} elements, {B} rows of stride {kb_bs} with {Nk} keys need "
                         f"{(B - 1) * kb_bs + Nk}")
    if kbias.data_ptr() % 16:
        raise ValueError("attention kbias: must start on a 16-byte boundary")
    return kb_bs


MAX_REGIONS = 8


def _chk_rbias(rbias, qregion, B, Nq, Nk, device):
    """the operands of pfd_attention_rbias_f16.  rbias: fp32 [B, NR, rb_rs] (or [1, NR, rb_rs]: one table for the batch) on
    `device`, contiguous, 16-byte aligned, rb_rs % 4 == 0 and >= Nk, 1 <= NR <= 8.  qregion: uint8 [B, >= Nq] (a column slice
    of a wider matrix is fine) or [>= Nq] (one map for the batch) on `device`; its values must be < NR, which the caller checks on the host where the map is
    made (lib/regions.region_grid): nothing is read back here.  -> (rb_rs, rb_bs, NR, qr_bs)"""
    if rbias is None or qregion is None:
        raise ValueError("attention: rbias and qregion come together")
    if not isinstance(rbias, torch.Tensor) or rbias.dtype != torch.float32:
        raise TypeError(f"attention rbias: expected a float32 tensor, got {getattr(rbias, 'dtype', type(rbias).__name__)}")
    if not isinstance(qregion, torch.Tensor) or qregion.dtype != torch.uint8:
        raise TypeError(f"attention qregion: expected a uint8 tensor, got {getattr(qregion, 'dtype', type(qregion).__name__)}")
    if not rbias.is_cuda or not qregion.is_cuda:
        raise RuntimeError("attention rbias / qregion: tensor on the CPU (no CPU fallback)")
    if rbias.device != device or qregion.device != device:
        raise ValueError(f"attention rbias / qregion: on {rbias.device} / {qregion.device}, the operands are on {device}")
    if not rbias.is_contiguous() or qregion.stride(-1) != 1 or (qregion.dim() == 1 and not qregion.is_contiguous()):
        raise ValueError("attention rbias / qregion: rbias must be contiguous, the bytes of a map consecutive")
    if rbias.dim() != 3 or rbias.shape[0] not in (1, B):
        raise ValueError(f"attention rbias: expected [{B}, NR, rb_rs] or [1, NR, rb_rs], got {tuple(rbias.shape)}")
    NR, rb_rs = int(rbias.shape[1]), int(rbias.shape[2])
    if not 1 <= NR <= MAX_REGIONS:
        raise ValueError(f"attention rbias: between 1 and {MAX_REGIONS} regions, got {NR}")
    if rb_rs % 4 or rb_rs < Nk:
        raise ValueError(f"attention rbias: row length {rb_rs} must be a multiple of 4 and at least Nk = {Nk}")
    if rbias.data_ptr() % 16:
        raise ValueError("attention rbias: must start on a 16-byte boundary")
    if qregion.dim() not in (1, 2) or qregion.shape[-1] < Nq or (qregion.dim() == 2 and qregion.shape[0] not in (1, B)):
        raise ValueError(f"attention qregion: expected [{B}, >= {Nq}] or [>= {Nq}], got {tuple(qregion.shape)}")
    rb_bs = NR * rb_rs if rbias.shape[0] == B and B > 1 else 0
    qr_bs = int(qregion.stride(0)) if qregion.dim() == 2 and qregion.shape[0] == B and B > 1 else 0   # (rows of a wider matrix are fine)
    if qr_bs and qr_bs < Nq:
        raise ValueError(f"attention qregion: rows {qr_bs} bytes apart hold no {Nq} queries")
    return rb_rs, rb_bs, NR, qr_bs


def attention(q, k, vt, B, H, Nq, Nk, D, scale, *, ldq, ldk, ldvt, q_bs, k_bs, vt_bs, out=None, kbias=None, kb_bs=None,
              rbias=None, qregion=None):
    """Fused attention; see pfd_attention_f16.  q/k/vt may be views into wider buffers; out (optional): [>= B*Nq, >= H*D]
    rows of stride % 8 == 0 (a column slice of a wider matrix is fine), the first B*Nq rows and H*D columns are written.
    kbias (optional): fp32 per-key logits in log2 units, element (b, j) at kbias.view(-1)[b * kb_bs + j] (kb_bs defaults to the
    row length of a [B, kb_bs] matrix); see pfd_attention_kbias_f16.  None is the plain entry point, exactly.
    rbias, qregion (optional, together, not with kbias): fp32 [B, NR, rb_rs] logits per region and key and the uint8 region of every
    query, [B, >= Nq] or [>= Nq]; see pfd_attention_rbias_f16 and _chk_rbias."""
    _chk16(q, "attention q")
    _chk16(k, "attention k")
    _chk16(vt, "attention vt")
    if kbias is not None:
        kb_bs = _chk_kbias(kbias, kb_bs, B, Nk, q.device)
    elif kb_bs is not None:
        raise ValueError("attention: kb_bs without kbias")
    rb = None
    if rbias is not None or qregion is not None:
        if kbias is not None:
            raise ValueError("attention: kbias and rbias exclude each other (one region IS the per-key operand)")
        rb = _chk_rbias(rbias, qregion, B, Nq, Nk, q.device)
    if out is None:
        out = torch.empty((B * Nq, H * D), dtype=torch.float16, device=q.device)
    else:
        _chk16(out, "attention out")
        if out.device != q.device or out.dim() != 2 or out.shape[0] < B * Nq or out.shape[1] < H * D or out.stride(-2) % 8:
            raise ValueError(f"attention: out {tuple(out.shape)} strides {out.stride()} on {out.device} is not a matrix of at "
                             f"least [{B * Nq}, {H * D}] with a row stride that is a multiple of 8 on {q.device}")
    d = _b.PfdAttnDesc()
    d.Q, d.K, d.Vt, d.O = q.data_ptr(), k.data_ptr(), vt.data_ptr(), out.data_ptr()
    d.ldq, d.ldk, d.ldvt, d.ldo = ldq, ldk, ldvt, out.stride(-2)
    d.q_bs, d.k_bs, d.vt_bs, d.o_bs = q_bs, k_bs, vt_bs, Nq * out.stride(-2)
    d.B, d.H, d.Nq, d.Nk, d.D = B, H, Nq, Nk, D
    d.scale = scale
    if kbias is not None:
        _b.check(_lib().pfd_attention_kbias_f16(_byref(d), kbias.data_ptr(), kb_bs, _stream()),
                 f"pfd_attention_kbias_f16 B{B} H{H} Nq{Nq} Nk{Nk} D{D}")
        return out
    if rb is not None:
        rb_rs, rb_bs, NR, qr_bs = rb
        _b.check(_lib().pfd_attention_rbias_f16(_byref(d), rbias.data_ptr(), rb_rs, rb_bs, NR, qregion.data_ptr(), qr_bs, _stream()),
                 f"pfd_attention_rbias_f16 B{B} H{H} Nq{Nq} Nk{Nk} D{D} NR{NR}")
        return out
    _b.check(_lib().pfd_attention_f16(_byref(d), _stream()), f"pfd_attention_f16 B{B} H{H} Nq{Nq} Nk{Nk} D{D}")
    return out


def swin_window_attention(qkv, qkv_bias, rpb, B, H, W_, Cdim, nH, ws, shift, scale, out=None):
    """qkv [B*H*W, 3C] token-major (dense), qkv_bias [3C], rpb [(2 ws - 1)^2, nH] -> out [B*H*W, C] (dense); see
    pfd_swin_window_attention_f16"""
    _chk16(qkv, "swin qkv")
    if out is None:
        out = torch.empty((B * H * W_, Cdim), dtype=torch.float16, device=qkv.device)
    else:
        _chk16(out, "swin out")
        if out.device != qkv.device or tuple(out.shape) != (B * H * W_, Cdim) or not out.is_contiguous():
            raise ValueError(f"swin_window_attention: out {tuple(out.shape)} on {out.device} is not a dense "
                             f"[{B * H * W_}, {Cdim}] on {qkv.device}")
    d = _b.PfdSwinAttnDesc()
    d.qkv, d.qkv_bias, d.rpb, d.out = qkv.data_ptr(), qkv_bias.data_ptr(), rpb.data_ptr(), out.data_ptr()
    d.B, d.H, d.W, d.C, d.nH, d.ws, d.shift = B, H, W_, Cdim, nH, ws, shift
    d.scale = scale
    _b.check(_lib().pfd_swin_window_attention_f16(_byref(d), _stream()), "pfd_swin_window_attention_f16")
    return _written(out)


# ----------------------------------------------------------------------------------------------
# normalisation
# ----------------------------------------------------------------------------------------------
def groupnorm(x, gamma, beta, groups, eps, *, x2=None, silu=False, out=None):
    """GroupNorm(+SiLU) of NHWC x[B,H,W,C1] (optionally virtually concatenated with x2[B,H,W,C2]).  When the launches
    that wrote x (and x2) emitted their statistics (gemm / conv gn_out=True) and the shape qualifies, the normalisation is
    ONE launch from those sums (pfd_groupnorm_pstats_f16); otherwise statistics + apply (or the small-slab kernel)."""
    _chk16(x, "groupnorm x")
    B = x.shape[0]
    C1 = x.shape[-1]
    HW = x.numel() // (B * C1)
    C2 = 0 if x2 is None else x2.shape[-1]
    if out is None:
        out = torch.empty(tuple(x.shape[:-1]) + (C1 + C2,), dtype=torch.float16, device=x.device)
    lib = _lib()
    st1 = get_gn_stats(x) if GN_PSTATS else None
    st2 = get_gn_stats(x2) if (GN_PSTATS and x2 is not None) else None
    if _TRACE_GN:   # PFD_TRACE_GN=<file>: which norms find their producers' statistics (tools/gn_paths.py)
        with open(_TRACE_GN, "a") as f:
            f.write(f"{B} {HW} {C1} {C2} {int(st1 is not None)} {int(x2 is None or st2 is not None)} "
                    f"{int(bool(lib.pfd_groupnorm_takes_pstats(B, C1, C2, HW, groups)))}\n")
    if st1 is not None and (x2 is None or st2 is not None) and groups == 32 and \
            lib.pfd_groupnorm_takes_pstats(B, C1, C2, HW, groups):
        rc = lib.pfd_groupnorm_pstats_f16(x.data_ptr(), C1, x.stride(-2), st1.data_ptr(), _ptr(x2), C2,
                                          0 if x2 is None else x2.stride(-2), _ptr(st2), gamma.data_ptr(), beta.data_ptr(),
                                          out.data_ptr(), out.stride(-2), B, HW, groups, eps,
                                          ACT_SILU if silu else ACT_NONE, _stream())
        _b.check(rc, f"pfd_groupnorm_pstats_f16 B{B} HW{HW} C{C1}+{C2}")
        return _written(out)
    wsb = lib.pfd_groupnorm_ws_bytes(B, C1 + C2, HW)
    ws = torch.empty(wsb, dtype=torch.uint8, device=x.device)
    rc = lib.pfd_groupnorm_f16(x.data_ptr(), C1, x.stride(-2), _ptr(x2), C2, 0 if x2 is None else x2.stride(-2),
                               gamma.data_ptr(), beta.data_ptr(), out.data_ptr(), out.stride(-2), B, HW, groups,
                               eps, ACT_SILU if silu else ACT_NONE, ws.data_ptr(), wsb, _stream())
    _b.check(rc, f"pfd_groupnorm_f16 B{B} HW{HW} C{C1}+{C2}")
    return _written(out)


def groupnorm_table(x, gamma, beta, groups, eps, *, x2=None):
    """GroupNorm statistics of NHWC x[B,H,W,C1] (| x2) as the per-(sample, channel) affine map the convolution's
    GroupNorm prologue applies: float32 [B, 2, C1+C2] = (rstd * gamma | beta - mean * rstd * gamma)."""
    _chk16(x, "groupnorm_table x")
    B = x.shape[0]
    C1 = x.shape[-1]
    HW = x.numel() // (B * C1)
    C2 = 0 if x2 is None else x2.shape[-1]
    if x2 is not None:
        _chk16(x2, "groupnorm_table x2")
    table = torch.empty((B, 2, C1 + C2), dtype=torch.float32, device=x.device)
    lib = _lib()
    wsb = lib.pfd_groupnorm_ws_bytes(B, C1 + C2, HW)
    ws = torch.empty(wsb, dtype=torch.uint8, device=x.device)
    rc = lib.pfd_groupnorm_table_f16(x.data_ptr(), C1, x.stride(-2), _ptr(x2), C2, 0 if x2 is None else x2.stride(-2),
                                     gamma.data_ptr(), beta.data_ptr(), table.data_ptr(), B, HW, groups, eps,
                                     ws.data_ptr(), wsb, _stream())
    _b.check(rc, f"pfd_groupnorm_table_f16 B{B} HW{HW} C{C1}+{C2}")
    return table


def layernorm(x, gamma, beta, eps=1e-5, out=None):
    _chk16(x, "layernorm x")
    M, Cdim, ldx = _rows(x)
    if out is None:
        out = torch.empty(x.shape, dtype=torch.float16, device=x.device)
    rc = _lib().pfd_layernorm_f16(x.data_ptr(), ldx, gamma.data_ptr(), beta.data_ptr(), out.data_ptr(),
                                  _rows(out)[2], M, Cdim, eps, 0, 0, 0, 0, _stream())
    _b.check(rc, f"pfd_layernorm_f16 M{M} C{Cdim}")
    return _written(out)


def layernorm_patch_merge(x, gamma, beta, eps=1e-5):
    """PatchMerging gather + LayerNorm(4C): x[B,H,W,C] -> [B*ceil(H/2)*ceil(W/2), 4C]."""
    _chk16(x, "layernorm_patch_merge x")
    B, H, W_, Cq = x.shape
    Ho, Wo = (H + 1) // 2, (W_ + 1) // 2
    out = torch.empty((B * Ho * Wo, 4 * Cq), dtype=torch.float16, device=x.device)
    rc = _lib().pfd_layernorm_f16(x.data_ptr(), x.stride(2), gamma.data_ptr(), beta.data_ptr(), out.data_ptr(),
                                  4 * Cq, B * Ho * Wo, 4 * Cq, eps, 1, B, H, W_, _stream())
    _b.check(rc, "pfd_layernorm_f16(gather4)")
    return out


def softmax_rows(x, scale, out=None):
    _chk16(x, "softmax x")
    R, N, ldx = _rows(x)
    if out is None:
        out = torch.empty((R, N), dtype=torch.float16, device=x.device)
    _b.check(_lib().pfd_softmax_rows_f16(x.data_ptr(), ldx, out.data_ptr(), _rows(out)[2], R, N, scale, _stream()),
             "pfd_softmax_rows_f16")
    return out


# ----------------------------------------------------------------------------------------------
# boundary / elementwise
# ----------------------------------------------------------------------------------------------
def to_nhwc(x, mul=1.0, add=0.0, rep=1):
    """NCHW fp32|fp16 -> NHWC fp16 (x*mul+add), batch repeated `rep` times."""
    if not x.is_cuda:
        raise RuntimeError("to_nhwc: input must live on the GPU; the HIP path has no CPU fallback")
    if x.dtype not in (torch.float32, torch.float16):
        x = x.float()
    x = x.contiguous()
    B, Cc, H, W_ = x.shape
    out = torch.empty((rep * B, H, W_, Cc), dtype=torch.float16, device=x.device)
    rc = _lib().pfd_nchw_to_nhwc_f16(x.data_ptr(), 1 if x.dtype == torch.float32 else 0, out.data_ptr(), B, Cc, H,
                                     W_, mul, add, rep, _stream())
    _b.check(rc, "pfd_nchw_to_nhwc_f16")
    return out


def to_nchw(x, dtype=torch.float16, mul=1.0, add=0.0, lo=-65504.0, hi=65504.0):
    """NHWC fp16 (dense) -> NCHW fp32|fp16, y = clamp(x*mul+add, lo, hi)."""
    _chk16(x, "to_nchw x")
    B, H, W_, Cc = x.shape
    if not x.is_contiguous():
        raise ValueError("to_nchw: dense NHWC expected")
    out = torch.empty((B, Cc, H, W_), dtype=torch.float32 if dtype == torch.float32 else torch.float16,
                      device=x.device)
    rc = _lib().pfd_nhwc_to_nchw(x.data_ptr(), out.data_ptr(), 1 if dtype == torch.float32 else 0, B, Cc, H, W_,
                                 mul, add, lo, hi, _stream())
    _b.check(rc, "pfd_nhwc_to_nchw")
    return out if out.dtype == dtype else out.to(dtype)


def image_u8(x, mul=1.0, add=0.0, f16_image=True):
    """NHWC fp16 [B,H,W,C] -> uint8 [B,H,W,C]: uint8(clamp(x*mul+add, 0, 1) * 255), the reference's ToPILImage
    arithmetic (app.py:273-275) on the device; f16_image: the image the reference would hold is fp16 (both the
    image and the product are rounded to f16 before the truncation), else fp32"""
    _chk16(x, "image_u8 x")
    if not x.is_contiguous():
        raise ValueError("image_u8: dense NHWC expected")
    out = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    _b.check(_lib().pfd_image_u8_f16(x.data_ptr(), out.data_ptr(), x.numel(), float(mul), float(add),
                                     1 if f16_image else 0, _stream()),
             "pfd_image_u8_f16")
    return out


_TAPS = {}
_IMG_KIND = {('nchw', torch.float16): _b.IMG_NCHW_F16, ('nchw', torch.float32): _b.IMG_NCHW_F32,
             ('nhwc', torch.float16): _b.IMG_NHWC_F16, ('u8', torch.uint8): _b.IMG_U8}


def _resample_taps(in_size, out_size, device):
    """device copy of Pillow's tap tables for one axis (lib/image_io.py): (kk, xmin, klen, ktaps).  They depend on
    (in, out) only: built once on the host and kept in a small bounded cache, like PPE_MLP.features -- so a hipGraph
    capture never sees a pageable host->device copy, and a table for a new size requested during capture raises"""
    key = (int(in_size), int(out_size), str(device))
    hit = _TAPS.get(key)
    if hit is None:
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError(f"image_from_u8: tap table for a new size {key[0]} -> {key[1]} requested during stream capture")
        from ..image_io import pillow_bicubic_taps
        xmin, klen, kk = pillow_bicubic_taps(*key[:2])
        if len(_TAPS) >= 32:
            _TAPS.clear()
        i32 = functools.partial(torch.tensor, dtype=torch.int32)
        hit = _TAPS[key] = (i32(kk).to(device), i32(xmin).to(device), i32(klen).to(device), len(kk[0]))
    return hit


def image_from_u8(img, size=None, dtype=torch.float16, layout='nchw'):
    """uint8 picture(s) [H,W,C] | [B,H,W,C] (C in {1, 3}) on the device -> the model's input [B,C,H',W'] in [0, 1]:
    Pillow's 8-bit bicubic `resize` to size = (H', W') (app.py:232; None: no resize) and torchvision's ToTensor + the
    cast to `dtype` (fp16 | fp32; app.py:234,244), byte for byte / bit for bit.  layout='nhwc' gives the fp16
    [B,H',W',C] of the product path, layout='u8' the resized uint8 [B,H',W',C] (Image.resize alone)."""
    if not (torch.is_tensor(img) and img.dtype == torch.uint8 and img.dim() in (3, 4)):
        raise ValueError("image_from_u8: a uint8 tensor [H, W, C] or [B, H, W, C] expected")
    if not img.is_cuda:
        raise RuntimeError("image_from_u8: input must live on the GPU; the HIP path has no CPU fallback")
    if layout == 'u8':
        dtype = torch.uint8
    kind = _IMG_KIND.get((layout, dtype))
    if kind is None:
        raise ValueError(f"image_from_u8: no output {layout!r} / {dtype} (nchw fp16 | fp32, nhwc fp16, u8)")
    x = (img[None] if img.dim() == 3 else img).contiguous()
    B, H, W_, Cc = x.shape
    Ho, Wo = (H, W_) if size is None else (int(size[0]), int(size[1]))
    lib = _lib()
    _b.check(lib.pfd_image_resample_check(B, H, W_, Ho, Wo, Cc), "pfd_image_resample_check")
    if Wo != W_:                                    # horizontal pass first, into a rounded uint8 picture (as Pillow)
        kk, xmin, klen, ktaps = _resample_taps(W_, Wo, x.device)
        mid = torch.empty((B, H, Wo, Cc), dtype=torch.uint8, device=x.device)
        _b.check(lib.pfd_image_resample_h_u8(x.data_ptr(), mid.data_ptr(), B, H, W_, Wo, Cc, kk.data_ptr(),
                                             xmin.data_ptr(), klen.data_ptr(), ktaps, _stream()),
                 "pfd_image_resample_h_u8")
        if Ho == H and kind == _b.IMG_U8:
            return mid
        x = mid
    shape = {_b.IMG_U8: (B, Ho, Wo, Cc), _b.IMG_NHWC_F16: (B, Ho, Wo, Cc)}.get(kind, (B, Cc, Ho, Wo))
    out = torch.empty(shape, dtype=dtype, device=x.device)
    kk, ymin, klen, ktaps = _resample_taps(H, Ho, x.device) if Ho != H else (None, None, None, 0)
    _b.check(lib.pfd_image_resample_v_u8(x.data_ptr(), out.data_ptr(), kind, B, H, Ho, Wo, Cc, _ptr(kk), _ptr(ymin),
                                         _ptr(klen), ktaps, _stream()),
             "pfd_image_resample_v_u8")
    return out


def canny_thresholds(low, high):
    """(low, high) as the detector takes them (lib/canny.py step 1): two finite numbers, floored, in order; clamped to
    [-1, 2041], which changes nothing (a magnitude lies in [0, 2040]) and keeps them int32.  ValueError otherwise."""
    import math
    try:
        low, high = float(low), float(high)
    except (TypeError, ValueError):
        raise ValueError(f"canny: thresholds must be two finite numbers, got {low!r}, {high!r}") from None
    if not (math.isfinite(low) and math.isfinite(high)):
        raise ValueError(f"canny: thresholds must be two finite numbers, got {low!r}, {high!r}")
    low, high = (max(-1, min(2041, int(math.floor(v)))) for v in (low, high))
    return (high, low) if low > high else (low, high)


@serialised
def canny_u8(img, low=100, high=200, out='u8', dtype=torch.float16, return_states=False):
    """uint8 picture(s) [H,W,C] | [B,H,W,C] (C in {1, 3}) on the device -> the Canny edge map of lib/canny.py, byte for
    byte (the reference's `cv2.Canny(img, low, high)`, controlnet_annotator/canny/__init__.py:5; equality with OpenCV
    itself is unverified).  out='u8': uint8 [B,H,W], 255 on an edge; out='hint': [B,3,H,W] in `dtype` (fp16 | fp32) with
    1 on an edge, three equal planes (`ToTensor` + `repeat(1, 3, 1, 1)`, controlnet.py:357-359).  Four launches on the
    current stream whatever the picture holds, no host synchronisation: capturable.  return_states: (result, the uint8
    [B,H,W] states after non-maximum suppression: 0 | 1 weak | 2 strong)."""
    if not (torch.is_tensor(img) and img.dtype == torch.uint8 and img.dim() in (3, 4)):
        raise ValueError("canny_u8: a uint8 tensor [H, W, C] or [B, H, W, C] expected")
    if out not in ('u8', 'hint'):
        raise ValueError(f"canny_u8: out must be 'u8' or 'hint', got {out!r}")
    kind = _b.IMG_U8 if out == 'u8' else _IMG_KIND.get(('nchw', dtype))
    if kind is None:
        raise ValueError(f"canny_u8: the hint is fp16 or fp32, not {dtype}")
    low, high = canny_thresholds(low, high)
    if not img.is_cuda:
        raise RuntimeError("canny_u8: input must live on the GPU; the HIP path has no CPU fallback")
    x = (img[None] if img.dim() == 3 else img).contiguous()
    B, H, W_, Cc = x.shape
    lib = _lib()
    _b.check(lib.pfd_canny_check(B, H, W_, Cc), "pfd_canny_check")
    states = torch.empty((B, H, W_), dtype=torch.uint8, device=x.device)
    parent = torch.empty((B, H, W_), dtype=torch.int32, device=x.device)
    strong = torch.empty((B, H, W_), dtype=torch.uint8, device=x.device)
    res = torch.empty((B, H, W_) if out == 'u8' else (B, 3, H, W_), dtype=torch.uint8 if out == 'u8' else dtype,
                      device=x.device)
    _b.check(lib.pfd_canny_u8(x.data_ptr(), B, H, W_, Cc, low, high, states.data_ptr(), parent.data_ptr(),
                              strong.data_ptr(), res.data_ptr(), kind, _stream()), "pfd_canny_u8")
    return (res, states) if return_states else res


def timestep_embedding(t, dim, max_period=10000.0):
    t = t.to(torch.int64).contiguous()
    out = torch.empty((t.shape[0], dim), dtype=torch.float16, device=t.device)
    _b.check(_lib().pfd_timestep_embedding_f16(t.data_ptr(), out.data_ptr(), t.shape[0], dim, max_period, _stream()),
             "pfd_timestep_embedding_f16")
    return out


def noise_key_rows(key, B, device):
    """int64 [B, 2] {seed, sample_id} rows on `device` (a CPU tensor is copied: not during a stream capture)"""
    if not (torch.is_tensor(key) and key.dtype == torch.int64 and tuple(key.shape) == (B, 2)):
        raise ValueError(f"noise_key must be an int64 tensor [{B}, 2] of (seed, sample_id) rows")
    return key.to(device).contiguous()


def philox_normal(key, step, n_per_sample):
    """fp32 [B, n_per_sample] standard normals: row b is the noise of sample key[b] = (seed, sample_id) at DDIM step
    `step` (Philox4x32-10 + Box-Muller; lib/noise.py is the same function on the host)."""
    if not (torch.is_tensor(key) and key.is_cuda):
        raise RuntimeError("philox_normal: key must live on the GPU; the HIP path has no CPU fallback")
    B = key.shape[0]
    key = noise_key_rows(key, B, key.device)
    out = torch.empty((B, int(n_per_sample)), dtype=torch.float32, device=key.device)
    _b.check(_lib().pfd_philox_normal_f32(key.data_ptr(), int(step), out.data_ptr(), B, int(n_per_sample), _stream()),
             "pfd_philox_normal_f32")
    return out


def latent_start(moments_nhwc, key, scale_factor, a_t, B=None, posterior='sample', want_x0=False):
    """The seeded start of an img2img request in one launch (pfd_latent_start; lib/img2img.py is the same function on the
    host).  moments_nhwc: f16 NHWC [Bm, h, w, 2C], what `quant_conv.hip(...)` returns, Bm = 1 (one picture for all
    samples) or B; key: int64 [B, 2] rows (seed, sample_id), B = key.shape[0] unless given; a_t: the cumulative alpha of
    the first timestep the run evaluates.  -> x_t fp32 NCHW [B, C, h, w], or (x0, x_t) with want_x0."""
    from ..img2img import check_posterior, kernel_scalars
    check_posterior(posterior)
    if not (torch.is_tensor(moments_nhwc) and moments_nhwc.dtype == torch.float16 and moments_nhwc.dim() == 4 and
            moments_nhwc.shape[3] % 2 == 0):
        raise ValueError("latent_start: moments must be an f16 NHWC tensor [Bm, h, w, 2C]")
    if not torch.is_tensor(key) or key.dim() != 2:
        raise ValueError("latent_start: key must be an int64 tensor [B, 2] of (seed, sample_id) rows")
    B = int(key.shape[0]) if B is None else int(B)
    Bm, h, w, C2 = moments_nhwc.shape
    if Bm not in (1, B):
        raise ValueError(f"latent_start: {Bm} pictures for {B} samples (one shared picture, or one per sample)")
    sf, sq_at, sq_1mat = (float(v) for v in kernel_scalars(scale_factor, a_t))
    if not moments_nhwc.is_cuda:
        raise RuntimeError("latent_start: moments must live on the GPU; the HIP path has no CPU fallback")
    if not moments_nhwc.is_contiguous():
        raise ValueError("latent_start: dense NHWC moments expected")
    key = noise_key_rows(key, B, moments_nhwc.device)
    xt = torch.empty((B, C2 // 2, h, w), dtype=torch.float32, device=moments_nhwc.device)
    x0 = torch.empty_like(xt) if want_x0 else None
    rc = _lib().pfd_latent_start(moments_nhwc.data_ptr(), Bm, key.data_ptr(), sf, sq_at, sq_1mat,
                                 1.0 if posterior == 'sample' else 0.0, _ptr(x0), xt.data_ptr(), B, C2 // 2, h, w, _stream())
    _b.check(rc, "pfd_latent_start")
    return (x0, xt) if want_x0 else xt


def guidance_scale_rows(scale, B, device):
    """the per-sample guidance scales of cfg_ddim_step, checked: a contiguous float32 tensor [B] on the GPU (the step
    runs inside a captured loop, so nothing is converted or copied here: DDIMSampler moves the vector once per request)"""
    if not (torch.is_tensor(scale) and scale.dtype == torch.float32 and tuple(scale.shape) == (B,) and
            scale.is_contiguous()):
        raise ValueError(f"a per-sample guidance scale must be a contiguous float32 tensor [{B}]")
    if not scale.is_cuda or scale.device != torch.device(device):
        raise ValueError(f"a per-sample guidance scale must live on {device}, next to x")
    return scale


def guidance_phi_rows(phi, B, device):
    """the per-sample guidance-rescale factors phi, checked like guidance_scale_rows: a contiguous float32 [B] next to x.
    Their range, [0, 1], is the sampler's to check (DDIMSampler moves the vector once per request)"""
    if not (torch.is_tensor(phi) and phi.dtype == torch.float32 and tuple(phi.shape) == (B,) and phi.is_contiguous()):
        raise ValueError(f"the guidance-rescale factors must be a contiguous float32 tensor [{B}]")
    if not phi.is_cuda or phi.device != torch.device(device):
        raise ValueError(f"the guidance-rescale factors must live on {device}, next to eps")
    return phi


def guidance_rescale(eps, scale_or_rows, phi_rows):
    """The per-sample factor of guidance rescale (pfd_guidance_rescale_f32; lib/guidance.py is the same function in fp64):
    mul[b] = phi[b] * std(ec_b) / std(g_b) + (1 - phi[b]), g the guided eps as the step kernel rounds it.  eps: f16 NHWC
    [2B, h, w, C], unconditional half first; scale_or_rows: a float32 tensor [B] (per-sample scales) or a float32 tensor
    of one element on the device (one scale for all, e.g. coef[index][4] -- a view, nothing is copied); phi_rows: float32
    [B] on the device.  Returns mul, float32 [B], for the eps_mul= of the step ops.  One launch; reads nothing back."""
    if not (torch.is_tensor(eps) and eps.dtype == torch.float16 and eps.dim() == 4 and eps.shape[0] % 2 == 0 and
            eps.shape[0] > 0 and eps.is_contiguous()):
        raise ValueError("guidance_rescale: eps must be a contiguous f16 NHWC tensor [2B, h, w, C], unconditional half first")
    if not eps.is_cuda:
        raise RuntimeError("guidance_rescale: eps must live on the GPU; the HIP path has no CPU fallback")
    B = int(eps.shape[0]) // 2
    n = eps[0].numel()
    phi_rows = guidance_phi_rows(phi_rows, B, eps.device)
    sc = scale_or_rows
    if not (torch.is_tensor(sc) and sc.dtype == torch.float32 and sc.is_cuda and sc.device == eps.device):
        raise ValueError("guidance_rescale: the scale must be a float32 tensor next to eps (one element, or one per sample)")
    if sc.numel() == 1:
        s_stride = 0
    elif tuple(sc.shape) == (B,) and sc.stride(0) >= 0:
        s_stride = int(sc.stride(0))
    else:
        raise ValueError(f"guidance_rescale: the scale must have one element or the shape [{B}], got {tuple(sc.shape)}")
    mul = torch.empty((B,), dtype=torch.float32, device=eps.device)
    rc = _lib().pfd_guidance_rescale_f32(eps.data_ptr(), sc.data_ptr(), s_stride, phi_rows.data_ptr(), 1, mul.data_ptr(), B,
                                         n, _stream())
    _b.check(rc, "pfd_guidance_rescale_f32")
    return mul


def _step_mul(eps, nb, x, solver, coef, eps_mul, outs, *, noise=None, x0_prev=None, key=None, step=None, noise_mul=1.0,
              scale=None, x0_keep=None, mask=None, ksq=0.0, ks=0.0):
    """the step ops with eps_mul=: pfd_cfg_step_mul, the entry point the op would have called plus the factor per sample"""
    B = x.shape[0]
    if nb != 2:
        raise ValueError("eps_mul (guidance rescale) needs the unconditional half: nb must be 2")
    if not (torch.is_tensor(eps_mul) and eps_mul.dtype == torch.float32 and tuple(eps_mul.shape) == (B,) and
            eps_mul.is_contiguous() and eps_mul.device == x.device):
        raise ValueError(f"eps_mul must be a contiguous float32 tensor [{B}] next to x (ops.guidance_rescale)")
    rc = _lib().pfd_cfg_step_mul(eps.data_ptr(), nb, x.data_ptr(), solver, _ptr(noise), _ptr(x0_prev), _ptr(key),
                                 0 if step is None else int(step), float(noise_mul), coef.data_ptr(), _ptr(scale),
                                 eps_mul.data_ptr(), _ptr(x0_keep), _ptr(mask), 0 if mask is None else int(mask.shape[0]),
                                 float(ksq), float(ks), *outs)
    _b.check(rc, "pfd_cfg_step_mul")


def _step_outputs(x, rep, want_next):
    """(x_prev | x_next, pred_x0) fp32 like x, and the next UNet input f16 NHWC [rep*B, h, w, C] or None"""
    B, Cc, h, w = x.shape
    xin = torch.empty((rep * B, h, w, Cc), dtype=torch.float16, device=x.device) if want_next else None
    return torch.empty_like(x), torch.empty_like(x), xin


def cfg_ddim_step(eps, nb, x, coef, *, noise=None, want_next=True, rep=None, noise_key=None, step=None, noise_mul=1.0,
                  scale=None, eps_mul=None):
    """Fused CFG combine + DDIM update.  eps NHWC f16 [nb*B,h,w,C]; x NCHW fp32 [B,C,h,w];
    coef fp32[5] device.  Returns (x_prev fp32 NCHW, pred_x0 fp32 NCHW, xin_next f16 NHWC|None);
    xin_next holds `rep` copies of the batch (default nb: the CFG-doubled UNet input).
    noise: fp32 NCHW tensor added as sigma * noise, or -- noise_key int64 [B,2] (seed, sample_id), step, noise_mul --
    the seeded noise sigma * noise_mul * z(key[b], step, element) evaluated inside the kernel (philox_normal).
    scale: fp32 [B] tensor, the guidance scale of sample b in place of coef[4] (pfd_cfg_ddim_step_ps; with noise,
    noise_key or neither).  None: coef[4] for the whole batch.
    eps_mul: fp32 [B] tensor (guidance_rescale), the guided eps of sample b times eps_mul[b] (pfd_cfg_step_mul: the same
    kernel; ones give the bits of the call without it).  None: the call is what it was."""
    B, Cc, h, w = x.shape
    rep = nb if rep is None else rep
    if noise_key is not None:
        if noise is not None:
            raise ValueError("cfg_ddim_step: give either noise or noise_key, not both")
        if step is None:
            raise ValueError("cfg_ddim_step: noise_key needs the DDIM step index (step=)")
        noise_key = noise_key_rows(noise_key, B, x.device)
    if scale is not None:
        scale = guidance_scale_rows(scale, B, x.device)
    x_prev, pred_x0, xin = _step_outputs(x, rep, want_next)
    outs = (x_prev.data_ptr(), pred_x0.data_ptr(), _ptr(xin), rep, B, Cc, h, w, _stream())
    if eps_mul is not None:
        _step_mul(eps, nb, x, 0, coef, eps_mul, outs, noise=noise, key=noise_key, step=step, noise_mul=noise_mul, scale=scale)
        return x_prev, pred_x0, xin
    if scale is not None:
        name = "pfd_cfg_ddim_step_ps"
        args = (_ptr(noise), _ptr(noise_key), 0 if step is None else int(step), float(noise_mul), coef.data_ptr(),
                scale.data_ptr())
    elif noise_key is not None:
        name, args = "pfd_cfg_ddim_step_rng", (noise_key.data_ptr(), int(step), float(noise_mul), coef.data_ptr())
    else:
        name, args = "pfd_cfg_ddim_step", (_ptr(noise), coef.data_ptr())
    _b.check(getattr(_lib(), name)(eps.data_ptr(), nb, x.data_ptr(), *args, *outs), name)
    return x_prev, pred_x0, xin


def cfg_dpmpp_step(eps, nb, x, coef, x0_prev=None, want_next=False, rep=None, scale=None, eps_mul=None):
    """Fused CFG combine + one DPM-Solver++(2M) step (pfd_cfg_dpmpp_step).  eps NHWC f16 [nb*B,h,w,C]; x NCHW fp32
    [B,C,h,w]; coef fp32[8] device, one row of lib/solver.py::dpmpp_2m_table.  x0_prev: the pred_x0 of the step before
    (fp32 NCHW, like x), or None for a first-order step (= DDIM at eta 0; the weights of the row are not read).
    scale: fp32 [B] tensor, the guidance scale of sample b in place of coef[6]; None: coef[6] for the whole batch.
    eps_mul: as in cfg_ddim_step.
    Returns (x_next fp32 NCHW, pred_x0 fp32 NCHW, xin_next f16 NHWC|None) like cfg_ddim_step."""
    B, Cc, h, w = x.shape
    rep = nb if rep is None else rep
    if tuple(coef.shape) != (8,) or coef.dtype != torch.float32:
        raise ValueError(f"cfg_dpmpp_step: coef must be a float32 row of 8 numbers: got {tuple(coef.shape)} {coef.dtype}")
    if x0_prev is not None and not (x0_prev.shape == x.shape and x0_prev.dtype == torch.float32 and
                                    x0_prev.device == x.device and x0_prev.is_contiguous()):
        raise ValueError("cfg_dpmpp_step: x0_prev must be a contiguous float32 tensor of x's shape, next to x")
    if scale is not None:
        scale = guidance_scale_rows(scale, B, x.device)
    x_next, pred_x0, xin = _step_outputs(x, rep, want_next)
    if eps_mul is not None:
        _step_mul(eps, nb, x, 1, coef, eps_mul, (x_next.data_ptr(), pred_x0.data_ptr(), _ptr(xin), rep, B, Cc, h, w, _stream()),
                  x0_prev=x0_prev, scale=scale)
        return x_next, pred_x0, xin
    rc = _lib().pfd_cfg_dpmpp_step(eps.data_ptr(), nb, x.data_ptr(), _ptr(x0_prev), coef.data_ptr(), _ptr(scale),
                                   x_next.data_ptr(), pred_x0.data_ptr(), _ptr(xin), rep, B, Cc, h, w, _stream())
    _b.check(rc, "pfd_cfg_dpmpp_step")
    return x_next, pred_x0, xin


MASKED_SOLVERS = {'ddim': 0, 'dpmpp': 1}


def mask_rows(mask, B, h, w):
    """the mask of cfg_step_masked, checked: float32 [1 | B, h, w] or [1 | B, 1, h, w] -> the contiguous [1 | B, h, w] view"""
    if not (torch.is_tensor(mask) and mask.dtype == torch.float32 and mask.dim() in (3, 4)):
        raise ValueError(f"mask must be a float32 tensor [1 | {B}, {h}, {w}] or [1 | {B}, 1, {h}, {w}]")
    if mask.dim() == 4:
        if mask.shape[1] != 1:
            raise ValueError(f"mask must have one channel (it is shared by the latent's channels), got {tuple(mask.shape)}")
        mask = mask[:, 0]
    if mask.shape[0] not in (1, B) or tuple(mask.shape[1:]) != (h, w):
        raise ValueError(f"mask must be [1 | {B}, {h}, {w}], got {tuple(mask.shape)}")
    return mask


def cfg_step_masked(eps, nb, x, coef, *, solver='ddim', x0_prev=None, keep_key=None, step=None, x0_keep=None, mask=None,
                    ksq=None, ks=None, noise_mul=1.0, scale=None, want_next=True, rep=None, eps_mul=None):
    """The masked (inpainting) form of cfg_ddim_step (solver='ddim') / cfg_dpmpp_step (solver='dpmpp') in one launch
    (pfd_cfg_step_masked; lib/inpaint.py is the same function on the host): x_out = m * xp + (1 - m) * known with xp the
    unmasked update and known = ksq * x0_keep + ks * z_keep, z_keep the stream-3 normal of (keep_key[b], step, element).
    keep_key: int64 [B, 2] rows (seed, sample_id), required: a DDIM row with sigma != 0 draws its step noise from the same
    rows (stream 0, times noise_mul) -- there is no form with a noise tensor.  x0_keep: fp32 NCHW like x, the clean latent
    of the init picture (latent_start(..., want_x0=True)); mask: fp32 [1 | B, h, w] in [0, 1], 1 = regenerate; ksq, ks:
    lib/inpaint.py::step_constants of the row stepped to.  coef, x0_prev, scale, eps_mul, want_next, rep: as in the unmasked ops.
    The mask's values are the caller's (reading them back would synchronise a loop that is captured): outside [0, 1] the
    blend extrapolates, nothing is read or written out of bounds.
    Returns (x_out fp32 NCHW, pred_x0 fp32 NCHW -- the unmasked one --, xin_next f16 NHWC | None)."""
    if solver not in MASKED_SOLVERS:
        raise ValueError(f"cfg_step_masked: solver must be 'ddim' or 'dpmpp', got {solver!r}")
    if not (torch.is_tensor(x) and x.dtype == torch.float32 and x.dim() == 4):
        raise ValueError("cfg_step_masked: x must be a float32 NCHW tensor")
    B, Cc, h, w = x.shape
    if nb not in (1, 2):
        raise ValueError(f"cfg_step_masked: nb must be 1 or 2, got {nb!r}")
    rep = nb if rep is None else rep
    if rep not in (1, 2):
        raise ValueError(f"cfg_step_masked: rep must be 1 or 2, got {rep!r}")
    if not (torch.is_tensor(eps) and eps.dtype == torch.float16 and tuple(eps.shape) == (nb * B, h, w, Cc) and
            eps.device == x.device and eps.is_contiguous()):
        raise ValueError(f"cfg_step_masked: eps must be a contiguous f16 NHWC tensor [{nb * B}, {h}, {w}, {Cc}] next to x")
    if keep_key is None or step is None or x0_keep is None or mask is None or ksq is None or ks is None:
        raise ValueError("cfg_step_masked: keep_key, step, x0_keep, mask, ksq and ks are all required")
    if int(step) != step or int(step) < 0:
        raise ValueError(f"cfg_step_masked: step must be a non-negative integer, got {step!r}")
    import math
    if not all(math.isfinite(float(v)) for v in (ksq, ks, noise_mul)):
        raise ValueError(f"cfg_step_masked: ksq, ks and noise_mul must be finite, got {ksq!r}, {ks!r}, {noise_mul!r}")
    ncoef = 5 if solver == 'ddim' else 8
    if not (torch.is_tensor(coef) and tuple(coef.shape) == (ncoef,) and coef.dtype == torch.float32):
        raise ValueError(f"cfg_step_masked: coef must be a float32 row of {ncoef} numbers for solver {solver!r}")
    if x0_prev is not None and solver != 'dpmpp':
        raise ValueError("cfg_step_masked: x0_prev goes with solver='dpmpp'")
    for t, what in ((x0_keep, 'x0_keep'), (x0_prev, 'x0_prev')):
        if t is not None and not (torch.is_tensor(t) and t.shape == x.shape and t.dtype == torch.float32 and
                                  t.device == x.device and t.is_contiguous()):
            raise ValueError(f"cfg_step_masked: {what} must be a contiguous float32 tensor of x's shape, next to x")
    mask = mask_rows(mask, B, h, w)
    if mask.device != x.device or not mask.is_contiguous():
        raise ValueError("cfg_step_masked: mask must be contiguous and live next to x")
    if not (torch.is_tensor(keep_key) and keep_key.dtype == torch.int64 and tuple(keep_key.shape) == (B, 2)):
        raise ValueError(f"cfg_step_masked: keep_key must be an int64 tensor [{B}, 2] of (seed, sample_id) rows")
    if not x.is_cuda:
        raise RuntimeError("cfg_step_masked: x must live on the GPU; the HIP path has no CPU fallback")
    if keep_key.device != x.device or not keep_key.is_contiguous() or not x.is_contiguous():
        raise ValueError("cfg_step_masked: keep_key must be contiguous and live next to x, x contiguous")
    if scale is not None:
        scale = guidance_scale_rows(scale, B, x.device)
    x_out, pred_x0, xin = _step_outputs(x, rep, want_next)
    if eps_mul is not None:
        _step_mul(eps, nb, x, MASKED_SOLVERS[solver], coef, eps_mul,
                  (x_out.data_ptr(), pred_x0.data_ptr(), _ptr(xin), rep, B, Cc, h, w, _stream()), x0_prev=x0_prev, key=keep_key,
                  step=step, noise_mul=noise_mul, scale=scale, x0_keep=x0_keep, mask=mask, ksq=ksq, ks=ks)
        return x_out, pred_x0, xin
    rc = _lib().pfd_cfg_step_masked(eps.data_ptr(), nb, x.data_ptr(), MASKED_SOLVERS[solver], _ptr(x0_prev),
                                    keep_key.data_ptr(), int(step), float(noise_mul), coef.data_ptr(), _ptr(scale),
                                    x0_keep.data_ptr(), mask.data_ptr(), int(mask.shape[0]), float(ksq), float(ks),
                                    x_out.data_ptr(), pred_x0.data_ptr(), _ptr(xin), rep, B, Cc, h, w, _stream())
    _b.check(rc, "pfd_cfg_step_masked")
    return x_out, pred_x0, xin


def mask_grid_u8(mask, gh, gw, dtype=torch.float32):
    """uint8 mask(s) [Hm, Wm] | [Bm, Hm, Wm] on the device (>= 128: regenerate) -> the binary grid [Bm, gh, gw] in `dtype`
    (float32 for the latent grid of cfg_step_masked, uint8 for the pixel grid of composite_u8): a cell is set if any pixel
    of its footprint is (pfd_mask_grid_u8, lib/inpaint.py::mask_grid) -- the rule dilates and never erodes."""
    if not (torch.is_tensor(mask) and mask.dtype == torch.uint8 and mask.dim() in (2, 3)):
        raise ValueError("mask_grid_u8: a uint8 tensor [Hm, Wm] or [Bm, Hm, Wm] expected")
    if dtype not in (torch.float32, torch.uint8):
        raise ValueError(f"mask_grid_u8: the grid is float32 or uint8, not {dtype}")
    gh, gw = int(gh), int(gw)
    m = mask[None] if mask.dim() == 2 else mask
    Bm, Hm, Wm = m.shape
    from ..image_io import MAX_SIDE
    if min(Bm, Hm, Wm, gh, gw) < 1 or max(Hm, Wm, gh, gw) > MAX_SIDE:
        raise ValueError(f"mask_grid_u8: sides must be in [1, {MAX_SIDE}], got {Hm} x {Wm} -> {gh} x {gw}")
    if not mask.is_cuda:
        raise RuntimeError("mask_grid_u8: the mask must live on the GPU; the HIP path has no CPU fallback")
    m = m.contiguous()
    out = torch.empty((Bm, gh, gw), dtype=dtype, device=m.device)
    _b.check(_lib().pfd_mask_grid_u8(m.data_ptr(), Bm, Hm, Wm, out.data_ptr(), 1 if dtype == torch.float32 else 0, gh, gw,
                                     _stream()), "pfd_mask_grid_u8")
    return out


def composite_u8(decoded, init, sel):
    """out[i, y, x, :] = sel[i or 0, y, x] ? decoded[i, y, x, :] : init[i or 0, y, x, :] (pfd_composite_u8): decoded uint8
    [n, H, W, C], init uint8 [1 | n, H, W, C] (the init picture at the output size), sel uint8 [1 | n, H, W]
    (mask_grid_u8 at the pixel grid) -> uint8 [n, H, W, C]"""
    for t, what, nd in ((decoded, 'decoded', 4), (init, 'init', 4), (sel, 'sel', 3)):
        if not (torch.is_tensor(t) and t.dtype == torch.uint8 and t.dim() == nd):
            raise ValueError(f"composite_u8: {what} must be a uint8 tensor of {nd} dimensions")
    n, H, W_, Cc = decoded.shape
    if init.shape[0] not in (1, n) or tuple(init.shape[1:]) != (H, W_, Cc):
        raise ValueError(f"composite_u8: init must be [1 | {n}, {H}, {W_}, {Cc}], got {tuple(init.shape)}")
    if sel.shape[0] not in (1, n) or tuple(sel.shape[1:]) != (H, W_):
        raise ValueError(f"composite_u8: sel must be [1 | {n}, {H}, {W_}], got {tuple(sel.shape)}")
    if n < 1 or Cc > 4:
        raise ValueError("composite_u8: at least one picture of at most 4 channels expected")
    if not decoded.is_cuda:
        raise RuntimeError("composite_u8: the pictures must live on the GPU; the HIP path has no CPU fallback")
    if init.device != decoded.device or sel.device != decoded.device:
        raise ValueError("composite_u8: init and sel must live next to decoded")
    decoded, init, sel = decoded.contiguous(), init.contiguous(), sel.contiguous()
    out = torch.empty_like(decoded)
    _b.check(_lib().pfd_composite_u8(decoded.data_ptr(), init.data_ptr(), int(init.shape[0]), sel.data_ptr(),
                                     int(sel.shape[0]), out.data_ptr(), n, H, W_, Cc, _stream()), "pfd_composite_u8")
    return out


def _chk_dense_out(out, n, what):
    """a caller's `out` of a dense element-wise launch: float16, on the device, dense, n elements (it may be an input)"""
    _chk16(out, what)
    if not out.is_contiguous():
        raise ValueError(f"{what}: dense tensor expected")
    if out.numel() != n:
        raise ValueError(f"{what}: {out.numel()} elements for a result of {n}")


def add(a, b, out=None):
    """out = a + b; out may be a or b"""
    _chk16(a, "add a")
    _chk16(b, "add b")
    if not (a.is_contiguous() and b.is_contiguous()):
        raise ValueError("add: dense tensors expected")
    if a.numel() != b.numel():
        raise ValueError(f"add: operand sizes differ ({tuple(a.shape)} vs {tuple(b.shape)}); no broadcasting")
    if out is None:
        out = torch.empty_like(a)
    else:
        _chk_dense_out(out, a.numel(), "add out")
    _b.check(_lib().pfd_add_f16(a.data_ptr(), b.data_ptr(), out.data_ptr(), a.numel(), _stream()), "pfd_add_f16")
    return _written(out)


def add_scaled_rows(x, r, scale, out=None):
    """out[b] = x[b] + scale[b] * r[b] (fp32 fma, one f16 rounding): the add of a ControlNet residual with one strength per
    sample (lib/control.py).  x, r: dense f16 [B, ...] of equal sizes; scale: an fp32 [B] view on the device, any stride
    -- a column of the request's [B, 13] table; out: x, r or another dense f16 tensor of that size.  A sample of scale 0
    receives x's bits and r is not read for it; at scale 1 the result is add(x, r) bit for bit.  Reads nothing back."""
    _chk16(x, "add_scaled_rows x")
    _chk16(r, "add_scaled_rows r")
    if not (x.is_contiguous() and r.is_contiguous()) or (out is not None and not out.is_contiguous()):
        raise ValueError("add_scaled_rows: dense tensors expected")
    if x.dim() < 2 or x.numel() != r.numel() or x.shape[0] != r.shape[0] or (out is not None and out.numel() != x.numel()):
        raise ValueError(f"add_scaled_rows: operand sizes differ ({tuple(x.shape)} vs {tuple(r.shape)}); no broadcasting")
    B = int(x.shape[0])
    if not torch.is_tensor(scale) or scale.dtype != torch.float32 or not scale.is_cuda or tuple(scale.shape) != (B,):
        raise ValueError(f"add_scaled_rows: scale must be a float32 [{B}] tensor on the device (a column of the strength table)")
    stride = int(scale.stride(0)) if B > 1 else 1
    if stride < 1:
        raise ValueError("add_scaled_rows: scale must have a positive stride")
    if out is None:
        out = torch.empty_like(x)
    else:
        _chk16(out, "add_scaled_rows out")
    _b.check(_lib().pfd_add_scaled_rows_f16(x.data_ptr(), r.data_ptr(), scale.data_ptr(), stride, out.data_ptr(), B,
                                            x.numel() // B, _stream()), "pfd_add_scaled_rows_f16")
    return _written(out)


def axpby(a, alpha, b=None, beta=0.0, out=None):
    """out = alpha*a + beta*b (b optional); out may be a or b"""
    _chk16(a, "axpby a")
    if b is not None:
        _chk16(b, "axpby b")
    if not a.is_contiguous() or (b is not None and not b.is_contiguous()):
        raise ValueError("axpby: dense tensors expected")
    if b is not None and b.numel() != a.numel():
        raise ValueError("axpby: operand sizes differ; no broadcasting")
    if out is None:
        out = torch.empty_like(a)
    else:
        _chk_dense_out(out, a.numel(), "axpby out")
    _b.check(_lib().pfd_axpby_f16(a.data_ptr(), float(alpha), _ptr(b), float(beta), out.data_ptr(), a.numel(),
                                  _stream()), "pfd_axpby_f16")
    return _written(out)


def add_rowvec(x, v, out=None, ln_out=None):
    """out = x + v[None, :]; ln_out: a float32 [R, C/160, 2] tensor that receives the partial row sums of `out` in the
    same launch (the layout gemm(ln=...) takes).  x and out: strided [R, C] matrices (out may be x); v: dense [C]"""
    _chk16(x, "add_rowvec x")
    R, Cc, ldx = _rows(x)
    _chk16(v, "add_rowvec v")
    if v.numel() != Cc or not v.is_contiguous():
        raise ValueError(f"add_rowvec: v of shape {tuple(v.shape)} strides {v.stride()} is not a dense vector of {Cc} elements")
    if out is None:
        out = torch.empty(x.shape, dtype=torch.float16, device=x.device)
    else:
        _chk16(out, "add_rowvec out")
        if _rows(out)[:2] != (R, Cc):
            raise ValueError(f"add_rowvec: out of shape {tuple(out.shape)} for a [{R}, {Cc}] result")
    if ln_out is not None:
        ln_out = _row_stats("add_rowvec: ln_out", "R, C/160, 2", R, Cc, x.device, ln_out)
        _b.check(_lib().pfd_add_rowvec_lnstats_f16(x.data_ptr(), ldx, v.data_ptr(), out.data_ptr(), _rows(out)[2], R, Cc,
                                                   ln_out.data_ptr(), _stream()), "pfd_add_rowvec_lnstats_f16")
        return _written(out)
    _b.check(_lib().pfd_add_rowvec_f16(x.data_ptr(), ldx, v.data_ptr(), out.data_ptr(), _rows(out)[2], R, Cc,
                                       _stream()), "pfd_add_rowvec_f16")
    return _written(out)


def activation(x, act, out=None):
    """out = act(x); out may be x"""
    _chk16(x, "activation x")
    if not x.is_contiguous():
        raise ValueError("activation: dense tensor expected")
    if out is None:
        out = torch.empty_like(x)
    else:
        _chk_dense_out(out, x.numel(), "activation out")
    _b.check(_lib().pfd_act_f16(x.data_ptr(), out.data_ptr(), x.numel(), act, _stream()), "pfd_act_f16")
    return _written(out)
