"""Several reference pictures mixed in ONE UNet pass: per-key weights in every cross-attention -- numpy only, fp64.

In this project the reference picture is the prompt.  A request that carries R references attends, in every cross-attention,
over the UNION of their tokens, and every key carries the weight of its reference:

    O[b,i,h,:] = sum_j w[b,j] exp(s_ij) V[b,j,h,:] / sum_j w[b,j] exp(s_ij),      s_ij = scale * <Q[b,i,h,:], K[b,j,h,:]>

which is softmax attention with the additive per-key logit log w[b,j].  Weights (1, 0) give the first reference alone, the
same reference twice at (1/2, 1/2) gives the single reference, and the order of the references does not matter.  The same
logit at -inf removes a key: that is how contexts of different lengths share a batch.

This is NOT the reference's `context_mixing` (pfd.py:366-386; lib.model_zoo.attention.ContextMix), which runs every context
layer once per context and adds the transformer outputs; the two are different functions of the same inputs and are not
compared numerically anywhere.

What the device is handed (pfd_attention_kbias_f16, include/pfd_hip.h) is `key_bias`: fp32, in log2 units, relative to
the largest weight -- so the largest weight is exactly 0.0, a single reference is an all-zero row, and every live logit is
<= 0.  `weighted_attention` is the specification of what it computes with them.
"""
import numpy as np

MAX_REFS = 8
# named ways to get it wrong (the tests show that their tolerance tells the specification from each of them)
BIAS_MUTANTS = ('natural_log', 'last_ref_shifted')                       # of key_bias
ATTN_MUTANTS = ('bias_ignored', 'bias_of_sample0', 'bias_after_max', 'masked_keys_score_zero')   # of weighted_attention
MUTANTS = BIAS_MUTANTS + ATTN_MUTANTS
F16_MIN_SUBNORMAL_LOG2 = -25.0            # a P value below 2^-25 rounds to 0 in fp16 (the 'bias_after_max' mutant)


def check_weights(weights):
    """-> float64 [R]; ValueError unless 1 <= R <= MAX_REFS and every weight is finite and > 0.
    A reference with weight 0 is DROPPED by the caller before anything is encoded -- it is never masked -- so a zero here is
    a caller that forgot to (`drop_zero_weights` does it)."""
    w = np.asarray(weights, dtype=np.float64).reshape(-1)
    if w.size < 1 or w.size > MAX_REFS:
        raise ValueError(f"between 1 and {MAX_REFS} references can be mixed, got {w.size}")
    if not np.all(np.isfinite(w)) or np.any(w < 0):
        raise ValueError(f"image_weights must be finite and >= 0, got {w.tolist()}")
    if np.any(w == 0):
        raise ValueError("a reference with weight 0 is dropped before it is encoded (drop_zero_weights), not masked")
    return w


def drop_zero_weights(weights):
    """-> (indices of the references kept, their weights as float64).  ValueError for weights that are not finite, negative,
    all zero, or more than MAX_REFS of them (counted before dropping: the request is what is checked)."""
    w = np.asarray(weights, dtype=np.float64).reshape(-1)
    if w.size < 1 or w.size > MAX_REFS:
        raise ValueError(f"between 1 and {MAX_REFS} references can be mixed, got {w.size}")
    if not np.all(np.isfinite(w)) or np.any(w < 0):
        raise ValueError(f"image_weights must be finite and >= 0, got {w.tolist()}")
    keep = [i for i in range(w.size) if w[i] > 0]
    if not keep:
        raise ValueError("at least one image weight must be > 0")
    return keep, w[keep]


def key_bias(weights, tokens_per_ref, nkp, wrong=None):
    """fp32 [nkp]: log2(w_r / max(w)) on the tokens_per_ref tokens of reference r, -inf behind the last reference's tokens.
    wrong: None or one of BIAS_MUTANTS."""
    if wrong is not None and wrong not in BIAS_MUTANTS:
        raise ValueError(f"unknown mutant {wrong!r}")
    w = check_weights(weights)
    t, nkp = int(tokens_per_ref), int(nkp)
    if t < 1 or w.size * t > nkp:
        raise ValueError(f"{w.size} references of {t} tokens do not fit {nkp} keys")
    rel = w / w.max()
    lg = np.log(rel) if wrong == 'natural_log' else np.log2(rel)
    lg[rel == 1.0] = 0.0
    out = np.full(nkp, -np.inf, dtype=np.float64)
    out[:w.size * t] = np.repeat(lg, t)
    if wrong == 'last_ref_shifted' and w.size > 1:
        s = (w.size - 1) * t
        out[s] = lg[-2]                                  # the run of the last reference starts (and ends) one key late
        out[s + 1:min(s + t + 1, nkp)] = lg[-1]
    return out.astype(np.float32)


def weighted_attention(q, k, v, bias, scale, wrong=None):
    """q [B, H, Nq, D], k / v [B, H, Nk, D], bias [B, Nk] (log2 units, finite or -inf; at least one finite per row)
    -> float64 [B, H, Nq, D]: the formula of the module text with w = 2**bias.  A key with bias -inf contributes exactly
    nothing, whatever its K and V hold.  wrong: None or one of ATTN_MUTANTS."""
    if wrong is not None and wrong not in ATTN_MUTANTS:
        raise ValueError(f"unknown mutant {wrong!r}")
    q, k, v = (np.asarray(a, dtype=np.float64) for a in (q, k, v))
    bias = np.asarray(bias, dtype=np.float64)
    B, H, Nq, D = q.shape
    Nk = k.shape[2]
    if bias.shape != (B, Nk):
        raise ValueError(f"bias must be [{B}, {Nk}], got {bias.shape}")
    if np.any(np.isnan(bias)) or np.any(bias == np.inf) or not np.all(np.isfinite(bias).any(axis=1)):
        raise ValueError("bias values are finite or -inf, with at least one finite value per row")
    if wrong == 'bias_of_sample0':
        bias = np.broadcast_to(bias[:1], bias.shape)
    live = np.isfinite(bias)[:, None, None, :]                                     # [B, 1, 1, Nk]
    t = np.einsum('bhid,bhjd->bhij', q, k) * (float(scale) * np.log2(np.e))         # log2 units
    b4 = np.where(live, bias[:, None, None, :], 0.0)
    if wrong == 'bias_ignored':
        p = np.exp2(t - t.max(-1, keepdims=True))
    elif wrong == 'masked_keys_score_zero':
        tb = np.where(live, t + b4, 0.0)
        p = np.exp2(tb - tb.max(-1, keepdims=True))
    elif wrong == 'bias_after_max':
        # the maximum of the UNbiased scores (masked keys included), the weight applied to P afterwards: the same number
        # until P = exp2(t - m) leaves the range of the fp16 it is kept in
        e = t - t.max(-1, keepdims=True)
        if not np.any(live & (e < F16_MIN_SUBNORMAL_LOG2)):
            return weighted_attention(q, k, v, bias, scale)
        p = np.where(live & (e >= F16_MIN_SUBNORMAL_LOG2), np.exp2(e + b4), 0.0)
    else:
        tb = np.where(live, t + b4, -np.inf)
        p = np.where(live, np.exp2(tb - tb.max(-1, keepdims=True)), 0.0)
    vz = np.where(np.isfinite(bias)[:, None, :, None] | (wrong in ('bias_ignored', 'masked_keys_score_zero')), v, 0.0)
    den = p.sum(-1, keepdims=True)
    num = np.einsum('bhij,bhjd->bhid', p, vz)
    if wrong == 'bias_after_max':          # a row whose every P was flushed is 0 / 0, as it would be in a kernel
        with np.errstate(invalid='ignore', divide='ignore'):
            return num / den
    return num / den
