"""Guidance rescale -- numpy only, fp64, no torch, no device.

This module is the specification of generate(guidance_rescale=) and of the kernels behind it (csrc/guidance.hip,
pfd_guidance_rescale_f32, and the eps_mul operand of the step kernel, pfd_cfg_step_mul).  It is Lin et al.
2023, "Common Diffusion Noise Schedules and Sample Steps are Flawed", section 3.4, and diffusers' `guidance_rescale`:
classifier-free guidance multiplies the spread of the guided eps by roughly the scale; the guided eps is brought back to the
standard deviation of the conditional eps, per sample, and blended by phi.

For sample b, with eu / ec its unconditional / conditional eps (f16 values, all n = C*h*w elements), guidance scale s_b and
phi_b in [0, 1]:

    g    = fl32(fma(s_b, fl32(ec - eu), eu))      the guided eps exactly as `guided_eps` in csrc/step.hip rounds it
    f_b  = phi_b * std(ec) / std(g) + (1 - phi_b) std over all n elements of the sample, mean removed
    e    = fl32(f_b * g)                          what the step then uses in place of g, for pred_x0 and the update alike

std(g) == 0, or phi_b == 0, gives f_b = 1 exactly.  The correction of the std (n or n - 1) is the same factor in the
numerator and the denominator and cancels: the ratio is sqrt(sum (ec - mean ec)^2 / sum (g - mean g)^2).  Only nb = 2 is
defined: there is no rescale without an unconditional half.

The kernel's order of summation (chain_length) is stated here because the tests' error bound is derived from it.

MUTANTS are named ways to get it wrong, for the tests to show that they tell the specification from its neighbours.
"""
import math

import numpy as np

MUTANTS = ('std_of_uncond', 'rms_not_std', 'phi_swapped', 'ratio_inverted', 'stats_over_batch', 'rescale_after_pred_x0')

# csrc/guidance.hip: one block of THREADS threads per sample; thread t owns the groups t, t + THREADS, ... of GROUP
# consecutive elements and adds their elements serially; six butterfly levels in the wave, four tree levels over the 16 waves
THREADS = 1024
GROUP = 8
WAVE = 64


def _check_wrong(wrong):
    if wrong is not None and wrong not in MUTANTS:
        raise ValueError(f"unknown mutant {wrong!r}")
    return wrong


def chain_length(n):
    """the longest chain of fp32 additions an element's value passes through in the kernel's sums over n elements: the
    serial part of the thread that owns the most elements (thread 0: ceil(groups / THREADS) groups of GROUP), then
    log2(WAVE) levels in the wave and log2(THREADS / WAVE) over the waves"""
    n = int(n)
    if n < 1:
        raise ValueError(f"n must be positive, got {n}")
    groups = -(-n // GROUP)
    serial = min(n, -(-groups // THREADS) * GROUP)
    return serial + int(math.log2(WAVE)) + int(math.log2(THREADS // WAVE))


def error_bound(n):
    """the bound on |mul - f| / f of the fp32 kernel against this module: (L + 8) * 2^-24.  Each of the four sums carries a
    relative error of at most L half-ulps (its terms have one sign in the sums of squares; in the means the error enters
    the result in second order only); the + 8 covers the division by n (twice), q_c / q_g, the square root, 1 - phi and
    the final fma, and the second-order effect of the means' error"""
    return (chain_length(n) + 8) * 2.0 ** -24


def check_phi(phi, n):
    """one number or n numbers, each finite and in [0, 1] -> float64 [n]"""
    n = int(n)
    try:
        v = np.asarray(phi, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"guidance_rescale must be one number or {n} numbers, got {phi!r}") from None
    if v.ndim == 0:
        v = np.full(n, float(v))
    if v.shape != (n,):
        raise ValueError(f"guidance_rescale must be one number or {n} numbers, one per sample: got shape {v.shape}")
    if not np.all(np.isfinite(v)) or np.any(v < 0) or np.any(v > 1):
        raise ValueError("guidance_rescale must be finite and in [0, 1]")
    return v


def normalise(phi, n, nb=2):
    """what a request's guidance_rescale comes to for its n samples: None -- the plain request -- when it is absent, all
    zero or there is no unconditional half (nb == 1); else the float32 [n] vector.  Checked whatever the outcome."""
    if phi is None:
        return None
    v = check_phi(phi, n)
    if int(nb) != 2 or not np.any(v):
        return None
    return v.astype(np.float32)


def _halves(eps):
    e = np.asarray(eps)
    if e.ndim < 2 or e.shape[0] % 2 or e.shape[0] == 0:
        raise ValueError(f"eps must be [2B, ...], the unconditional half first: got {e.shape}")
    B = e.shape[0] // 2
    e = e.astype(np.float16).astype(np.float32).reshape(2 * B, -1)     # f16 values, exact in fp32
    return e[:B], e[B:], B


def guided(eu, ec, s):
    """fl32(fma(s, fl32(ec - eu), eu)) for fp32 arrays of f16 values and an fp32 s: the difference of two f16 values and
    the product of two fp32 values are exact in fp64; the sum is exact in fp64 too whenever it spans at most 53 bits -- f16
    values are multiples of 2^-24 below 2^16, the product of a scale like 7.5 and such a difference is a multiple of 2^-26 --
    so the one rounding to fp32 is the fma's.  (A scale with all 24 bits in use on data near 65504 could round twice.)"""
    d = (ec.astype(np.float32) - eu.astype(np.float32)).astype(np.float32)
    return (np.float64(np.float32(s)) * d.astype(np.float64) + eu.astype(np.float64)).astype(np.float32)


def _std(v):
    v = np.asarray(v, dtype=np.float64)
    return math.sqrt(float(np.mean((v - v.mean()) ** 2)))


def _rms(v):
    v = np.asarray(v, dtype=np.float64)
    return math.sqrt(float(np.mean(v ** 2)))


def factor(eps, scale, phi, wrong=None):
    """-> float64 [B]: f_b of the module's head.  eps [2B, ...] (any layout behind the batch: the statistics are over all
    elements), scale one number or B, phi one number or B in [0, 1]"""
    _check_wrong(wrong)
    eu, ec, B = _halves(eps)
    s = np.asarray(scale, dtype=np.float64)
    s = np.full(B, float(s)) if s.ndim == 0 else s
    if s.shape != (B,):
        raise ValueError(f"scale must be one number or {B} numbers, got shape {s.shape}")
    ph = check_phi(phi, B)
    g = np.stack([guided(eu[b], ec[b], np.float32(s[b])) for b in range(B)])
    spread = _rms if wrong == 'rms_not_std' else _std
    num_of = eu if wrong == 'std_of_uncond' else ec
    out = np.ones(B, dtype=np.float64)
    for b in range(B):
        if wrong == 'stats_over_batch':
            num, den = spread(num_of), spread(g)
        else:
            num, den = spread(num_of[b]), spread(g[b])
        if ph[b] == 0.0 or den == 0.0:
            continue
        ratio = den / num if wrong == 'ratio_inverted' else num / den
        out[b] = (1.0 - ph[b]) * ratio + ph[b] if wrong == 'phi_swapped' else ph[b] * ratio + (1.0 - ph[b])
    return out


def rescaled_eps(eps, scale, mul):
    """-> (g, e) float32 [B, n]: the guided eps and e = fl32(mul_b * g), mul rounded to fp32 first (the kernel's operand)"""
    eu, ec, B = _halves(eps)
    s = np.asarray(scale, dtype=np.float64)
    s = np.full(B, float(s)) if s.ndim == 0 else s
    m = np.asarray(mul, dtype=np.float64).astype(np.float32).reshape(B)
    g = np.stack([guided(eu[b], ec[b], np.float32(s[b])) for b in range(B)])
    e = (m.astype(np.float64)[:, None] * g.astype(np.float64)).astype(np.float32)
    return g, e


def ddim_step(eps, x, a_t, a_prev, scale, mul, wrong=None):
    """the deterministic DDIM step (sigma = 0) on the rescaled eps in fp64 -> (x_prev, pred_x0) float64 [B, n]; eps and x
    [.., n] in ONE element order.  pred_x0 and the direction term both take e; the mutant 'rescale_after_pred_x0' takes
    pred_x0 from the un-rescaled g"""
    _check_wrong(wrong)
    g, e = rescaled_eps(eps, scale, mul)
    B = g.shape[0]
    x = np.asarray(x, dtype=np.float64).reshape(B, -1)
    e64, g64 = e.astype(np.float64), g.astype(np.float64)
    s1mat = math.sqrt(1.0 - a_t)
    pred = (x - s1mat * (g64 if wrong == 'rescale_after_pred_x0' else e64)) / math.sqrt(a_t)
    return math.sqrt(a_prev) * pred + math.sqrt(1.0 - a_prev) * e64, pred
