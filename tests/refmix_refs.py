"""Helpers of the reference-mixing tests (tests/test_refmix_*.py): the cases and key-logit patterns of the kernel tests, the fp64
weighted attention on torch tensors in the layouts the kernels take (pinned to lib/refmix.weighted_attention, the numpy
specification, by tests/test_refmix_cpu.py) and the per-element bound.
Imports kernel_refs; changes nothing in it."""
import functools
import math

import numpy as np
import torch

import kernel_refs as KR

from lib import refmix

KBIAS_CLASSES = ("w4", "w8", "d80", "d160")
# (B, H, Nq, Nk, D): the smallest shapes that reach each path
KBIAS_CASES = {
    "w4": [(1, 2, 300, 148, 40), (1, 1, 33, 1, 40), (1, 2, 130, 129, 40), (3, 2, 64, 296, 40), (1, 2, 300, 444, 40)],
    "w8": [(16, 8, 1024, 296, 40), (13, 8, 1030, 148, 40)],
    "d80": [(1, 2, 150, 296, 80)],
    "d160": [(2, 2, 64, 296, 160), (2, 2, 64, 444, 160)],
}
PATTERNS = ("zero", "two", "three", "random", "ragged", "holes")
ALL_CASES = [(cls, c) for cls in KBIAS_CLASSES for c in KBIAS_CASES[cls]]


def case_id(c):
    return "B%dH%dq%dk%dd%d" % tuple(c[:5])


def kbias_kernel_class(B, H, Nq, Nk, D):
    """which kernel pfd_attention_kbias_f16 launches.  None: PFD_ESHAPE."""
    return KR.attention_kernel_class(B, H, Nq, Nk, D, operand="kbias")


def kb_stride(Nk):
    return (Nk + 3) // 4 * 4 + 4          # a multiple of 4, > Nk


def _mix_row(weights, Nk):
    R = max(1, min(len(weights), Nk))
    return torch.from_numpy(refmix.key_bias(list(weights)[:R], Nk // R, Nk))


@functools.lru_cache(maxsize=None)
def bias_rows(case, pattern):
    """fp32 [B, kb_stride(Nk)] (CPU): the logits of keys 0 .. Nk - 1, NaN behind them; rows differ per sample.  Key 0 is finite.
      zero    all 0
      two     two references 0.7 / 0.3 (sample b: the weights rotated by b), Nk // 2 tokens each, a rest of Nk % 2 keys -inf
      three   three references 0.5 / 0.3 / 0.2, rotated by b
      random  uniform in [-12, 0] per key
      ragged  R = 3 references (2 below 444 keys) of Nk // R tokens at weight 1; sample b keeps 1 + b % R of them, the rest is
              -inf: whole trailing 64-key tiles are masked
      holes   -inf on keys 64 .. 127 and on every fifth key, key 0 finite; random in [-12, 0] elsewhere
    Do not modify the result."""
    B, H, Nq, Nk, D = case[:5]
    g = torch.Generator().manual_seed(Nk * 7919 + B * 31 + D + 1000 * PATTERNS.index(pattern))
    out = torch.full((B, kb_stride(Nk)), float("nan"), dtype=torch.float32)
    for b in range(B):
        if pattern == "zero":
            row = torch.zeros(Nk)
        elif pattern in ("two", "three"):
            w = (0.7, 0.3) if pattern == "two" else (0.5, 0.3, 0.2)
            row = _mix_row(w[b % len(w):] + w[:b % len(w)], Nk)
        elif pattern == "random":
            row = -12.0 * torch.rand(Nk, generator=g)
        elif pattern == "ragged":
            R = max(1, min(3 if Nk >= 444 else 2, Nk))
            row = _mix_row((1.0,) * R, Nk)
            row[(1 + b % R) * (Nk // R):] = float("-inf")
        else:
            assert pattern == "holes", pattern
            row = -12.0 * torch.rand(Nk, generator=g)
            j = torch.arange(Nk)
            row[((j >= 64) & (j < 128)) | ((j % 5 == 0) & (j > 0))] = float("-inf")
        assert math.isfinite(float(row[0]))
        out[b, :Nk] = row
    return out


def problem(case):
    """kernel_refs.attention_problem of the dense case: NaN in every V^T pad column; K and V of every key inside Nk are finite
    (the contract of a -inf key)"""
    return KR.attention_problem(tuple(case[:5]) + ("dense", 0))


def weighted_ref(q, k, vt, bias, B, H, Nq, Nk, D, scale, *, ldq, ldk, ldvt, q_bs, k_bs, vt_bs, q_off=0, k_off=0, vt_off=0,
                 folded=False, wrong=None):
    """lib/refmix.weighted_attention on the flat fp16 operands of a launch (any device), in fp64 torch: bias [B, >= Nk] in log2
    units.  -> ([B, Nq, H * D], T) with T = the largest |biased score| (log2 units) among the live keys.
    folded: with the operand quantisation of the folded-maximum kernel, Q' = fp16(fp32(q) * fp32(scale log2 e)).
    wrong: 'bias_ignored' | 'bias_of_sample0' | 'masked_keys_score_zero' (the refmix mutants that are a one-line change here)."""
    Q, K, V = KR._attn_views(q, k, vt, B, H, Nq, Nk, D, ldq, ldk, ldvt, q_bs, k_bs, vt_bs, q_off, k_off, vt_off)
    c32 = float(torch.tensor(scale, dtype=torch.float32) * torch.tensor(KR.LOG2E, dtype=torch.float32))
    out = torch.empty((B, Nq, H * D), dtype=torch.float64, device=q.device)
    T = 0.0
    for b in range(B):
        bb = bias[0 if wrong == "bias_of_sample0" else b, :Nk].to(device=q.device, dtype=torch.float64)
        live = torch.isfinite(bb)
        if folded:
            t = (Q[b].float() * c32).half().double() @ K[b].double().transpose(-1, -2)
        else:
            t = (Q[b].double() @ K[b].double().transpose(-1, -2)) * (scale * KR.LOG2E)
        if wrong == "bias_ignored":
            tb, vb = t, V[b].double()
        elif wrong == "masked_keys_score_zero":
            tb, vb = torch.where(live, t + torch.where(live, bb, 0.0), 0.0), V[b].double()
        else:
            tb = torch.where(live, t + torch.where(live, bb, 0.0), float("-inf"))
            vb = torch.where(live[:, None], V[b].double(), 0.0)
            T = max(T, float(tb[..., live].abs().max()))
        p = torch.exp2(tb - tb.amax(-1, keepdim=True))
        out[b] = ((p @ vb) / p.sum(-1, keepdim=True)).transpose(0, 1).reshape(Nq, H * D)
    return out, T


# The bound of kernel_refs.attention_bound plus what the logit adds.  The kernels start the fp32 QK^T accumulator at the
# logit in the units of the score -- kbias itself where the score is in log2 units (w8), fl(kbias / c) with c = scale log2 e
# where it is raw (one more rounding, 2^-24 |kbias|) -- so each of the D / 16 (rounded up) MFMAs that accumulate a score now
# rounds a value of magnitude up to |kbias| + |t| instead of |t| (t: the biased score, log2 units; A_t: its largest
# magnitude over the live keys of the launch).  That is at most (ceil(D / 16) + 1) roundings of 2^-24 (|kbias| + |t|) each:
#     d_t <= (ceil(D / 16) + 1) 2^-24 (Bmax + T)        (log2 units; Bmax = the largest finite |kbias|, T = max |t|)
# A score error d_t moves a probability by the factor 2^(+-d_t), numerator against denominator by twice that:
#     2 ln2 d_t vmax
# (attention_bound's own 2^-16 covers the accumulation of the unbiased score, the fma and v_exp_f32, as before.)
def kbias_extra(D, T, Bmax, vmax):
    return 2 * 0.6931471805599453 * (-(-D // 16) + 1) * 2.0 ** -24 * (Bmax + T) * vmax


def kbias_bound(Nk, D, vmax, T, Bmax, A=0.0):
    return KR.attention_bound(Nk, vmax, A) + kbias_extra(D, T, Bmax, vmax)


def bias_max(bias, Nk):
    b = bias[:, :Nk]
    return float(b[torch.isfinite(b)].abs().max())


def to_spec(q, k, vt, B, H, Nq, Nk, D, desc):
    """the operands as the numpy arrays lib/refmix.weighted_attention takes: q [B, H, Nq, D], k / v [B, H, Nk, D] (fp64)"""
    Q, K, V = KR._attn_views(q, k, vt, B, H, Nq, Nk, D, desc["ldq"], desc["ldk"], desc["ldvt"], desc["q_bs"], desc["k_bs"],
                             desc["vt_bs"], desc.get("q_off", 0), desc.get("k_off", 0), desc.get("vt_off", 0))
    return tuple(np.nan_to_num(a.double().cpu().numpy()) if a is V else a.double().cpu().numpy() for a in (Q, K, V))


# ------------------------------------------------------------------------------------------------
# operands that tell every mutant of lib/refmix.py from the specification (shared by the CPU and the GPU kernel tests)
# ------------------------------------------------------------------------------------------------
# B, H, Nq, Nk, D per kernel class: two references of 74 tokens.  Every head and every query of a problem holds the same numbers,
# so the problem of a class with one head and 32 queries (`reduced`, what the CPU tests evaluate) has the same outputs.
DISC_DIMS = {"w4": (2, 1, 32, 148, 40), "w8": (2, 64, 1024, 148, 40), "d80": (2, 1, 32, 148, 80), "d160": (2, 1, 32, 148, 160)}


@functools.lru_cache(maxsize=None)
def discriminating(mutant, cls="w4", reduced=False):
    """one problem per mutant on which the specification gives about +1 where the mutant gives about -1 (or NaN): every query and
    key along one sign vector u, so that the score of key j is a chosen number t_j of log2 units; V = +-1 in every column; keys
    0 .. 73 are reference 0 (group A), 74 .. 147 reference 1 (group B).
    -> dict(q, k, vt flat fp16; desc; scale; bias fp32 [B, Nk] (the specification's); wrong_bias (for the key_bias mutants))
      bias_ignored             B masked, scores + 12 above A, V_B = -1
      bias_of_sample0          the same in sample 1; sample 0 has no masked key
      masked_keys_score_zero   every score at -12, B masked, V_B = -1: a masked key scored 0 dominates by 2^12
      bias_after_max           B masked and + 40 above A: exp2(t_A - max) is below the smallest fp16 number
      natural_log              weights (1, 2^-40), B + 34 above A: - 6 in log2 units, + 6.3 with the natural log taken for it
      last_ref_shifted         weights (1, 2^-40); key 74 at + 30 with V = -1: suppressed in its own reference, dominant in A's"""
    assert mutant in refmix.MUTANTS
    B, H, Nq, Nk, D = DISC_DIMS[cls]
    if reduced:
        H, Nq = 1, 32
    assert reduced or kbias_kernel_class(B, H, Nq, Nk, D) == cls
    t_ref = Nk // 2
    scale = D ** -0.5
    c = scale * KR.LOG2E
    g = torch.Generator().manual_seed(refmix.MUTANTS.index(mutant) + 11)
    u = torch.sign(torch.randn(D, generator=g))
    inB = torch.arange(Nk) >= t_ref
    tA, tB = {"bias_ignored": (0., 12.), "bias_of_sample0": (0., 12.), "masked_keys_score_zero": (-12., -12.),
              "bias_after_max": (0., 40.), "natural_log": (0., 34.), "last_ref_shifted": (0., 0.)}[mutant]
    t = torch.where(inB, torch.tensor(tB), torch.tensor(tA))
    v = torch.where(inB, -1.0, 1.0)
    wrong_bias = None
    if mutant in refmix.BIAS_MUTANTS:
        w = (1.0, 2.0 ** -40)
        if mutant == "last_ref_shifted":
            t[t_ref], v = 30.0, torch.ones(Nk)
            v[t_ref] = -1.0
        row = torch.from_numpy(refmix.key_bias(w, t_ref, Nk))
        bias = row[None].repeat(B, 1)
        wrong_bias = torch.from_numpy(refmix.key_bias(w, t_ref, Nk, wrong=mutant))[None].repeat(B, 1)
    else:
        bias = torch.zeros((B, Nk))
        bias[:, inB] = float("-inf")
        if mutant == "bias_of_sample0":
            bias[0] = 0.0
    C = H * D
    uh = u.repeat(H)                                                       # the same direction in every head
    Q = uh[None, None].expand(B, Nq, C).half()
    K = ((t / (D * c))[None, :, None] * uh).expand(B, Nk, C).half()
    Nkp = (Nk + 7) // 8 * 8
    vt = KR._poisoned(C * B * Nkp).view(C, B, Nkp)
    vt[:, :, :Nk] = v.half()[None, None].expand(C, B, Nk)
    desc = dict(ldq=C, ldk=C, ldvt=B * Nkp, q_bs=Nq * C, k_bs=Nk * C, vt_bs=Nkp)
    return dict(q=Q.reshape(-1).contiguous(), k=K.reshape(-1).contiguous(), vt=vt.reshape(-1), desc=desc, scale=scale,
                bias=bias.float(), wrong_bias=wrong_bias, vmax=1.0, dims=(B, H, Nq, Nk, D))


def mutant_output(p, mutant):
    """what `mutant` computes on problem p, through lib/refmix.py (numpy, fp64) -> [B, H, Nq, D]"""
    B, H, Nq, Nk, D = p["dims"]
    Q, K, V = KR._attn_views(p["q"], p["k"], p["vt"], B, H, Nq, Nk, D, p["desc"]["ldq"], p["desc"]["ldk"], p["desc"]["ldvt"],
                             p["desc"]["q_bs"], p["desc"]["k_bs"], p["desc"]["vt_bs"], 0, 0, 0)
    q, k, v = (a.double().numpy() for a in (Q, K, V))
    if mutant in refmix.BIAS_MUTANTS:
        return refmix.weighted_attention(q, k, v, p["wrong_bias"].double().numpy(), p["scale"])
    return refmix.weighted_attention(q, k, v, p["bias"].double().numpy(), p["scale"], wrong=mutant)


# ------------------------------------------------------------------------------------------------
# block_refs extended by the weighted attention (block_refs.py itself is not touched)
# ------------------------------------------------------------------------------------------------
import contextlib


@contextlib.contextmanager
def weighted_cross_attention(bias):
    """inside the block: block_refs.cross_attention with the per-key logits `bias` [B, Nk] (log2 units, -inf = no such key)
    wherever a context is given -- softmax over scale q k^T + ln 2 * bias; self-attention is what it was.  The block formulas
    (attention_branch, basic_transformer_block, spatial_transformer, unet) are block_refs' own, unchanged."""
    import block_refs as BR
    orig = BR.cross_attention

    def cross_attention(p, x, context, heads, wrong=None):
        if context is None:
            return orig(p, x, context, heads, wrong)
        q, k, v = BR.linear(p.sub("to_q."), x), BR.linear(p.sub("to_k."), context), BR.linear(p.sub("to_v."), context)
        B, N, Cd = q.shape
        d = Cd // heads
        sp = lambda t: t.reshape(B, -1, heads, d).permute(0, 2, 1, 3)  # noqa: E731
        q, k, v = sp(q), sp(k), sp(v)
        s = (q @ k.transpose(-1, -2)) * d ** -0.5 + (bias.to(q.dtype) * math.log(2.0))[:, None, None, :]
        return BR.linear(p.sub("to_out.0."), (s.softmax(dim=-1) @ v).permute(0, 2, 1, 3).reshape(B, N, Cd))
    BR.cross_attention = cross_attention
    try:
        yield
    finally:
        BR.cross_attention = orig
