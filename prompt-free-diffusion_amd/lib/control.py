"""How strongly, in which layers and on which steps a ControlNet hint binds -- numpy only, fp64, no torch, no device.

This module is the specification of generate(control_scale=, control_layer_scales=, control_window=, control_cond_only=)
and of the kernel behind it (csrc/control.hip, pfd_add_scaled_rows_f16).  The reference adds the 13
ControlNet residuals as they are (pfd.py:515-521; its `control_scales` list is never applied, pfd.py:463); here

    h      = h + T[b, 12] * control[12]                 behind the middle block        (`h = h + control.pop()`)
    skip_j = skip_j + T[b, i] * control[i]              i = 11 .. 0, in the order the output blocks pop their skips

with a table T fp32 [nb * n, 13], row b of the CFG batch [uncond | cond], T[b of sample j, i] = scale[j] * layers[i]
(one fp32 rounding of the fp64 product), and only on the steps of a window of the schedule; on every other step the
UNet runs without the ControlNet, which is then not evaluated at all.

Index i is the position in the list ControlNet.hip returns: 0 the residual of the stem, 11 of the last input block, 12
`middle_block_out`, which the UNet pops first.

Steps are counted on the FULL schedule: a run that evaluates k of `total` steps (img2img, a mask: k < total) evaluates
its step i (i = 0 first, at the highest noise) at position p = total - k + i, and a window (start, end) controls the
positions ceil(start * total) <= p < floor(end * total) (each with a guard of 1e-9 against a product like 0.3 * 10
landing a hair beside its integer).  A window therefore names the same noise levels whatever `strength` is.

MUTANTS are named ways to get it wrong, for the tests to show that they tell the specification from its neighbours.
"""
import math

import numpy as np

N_RESIDUALS = 13
SOFT_BASE = 0.825          # 'soft' layer weights: 0.825 ** (12 - i), the deep layers bind, the shallow ones give way
_EPS = 1e-9
MUTANTS = ('window_lo_off_by_one', 'window_hi_off_by_one', 'window_of_run', 'layers_reversed', 'uncond_not_zeroed',
           'scale_on_x')


def _check_wrong(wrong):
    if wrong is not None and wrong not in MUTANTS:
        raise ValueError(f"unknown mutant {wrong!r}")
    return wrong


def check_window(window):
    """-> (start, end) as floats; ValueError unless 0 <= start <= end <= 1"""
    try:
        start, end = (float(v) for v in window)
    except (TypeError, ValueError):
        raise ValueError(f"control_window must be a pair (start, end), got {window!r}") from None
    if not (math.isfinite(start) and math.isfinite(end) and 0.0 <= start <= end <= 1.0):
        raise ValueError(f"control_window must satisfy 0 <= start <= end <= 1, got {window!r}")
    return start, end


def window_steps(total, k, window, wrong=None):
    """-> (lo, hi): the steps lo <= i < hi of a run of k of `total` steps are controlled; lo == hi: none is"""
    _check_wrong(wrong)
    total, k = int(total), int(k)
    if total < 1 or not 1 <= k <= total:
        raise ValueError(f"a run evaluates 1 <= k <= total steps, got k = {k}, total = {total}")
    start, end = check_window(window)
    span, first = (k, 0) if wrong == 'window_of_run' else (total, total - k)
    p_lo = math.ceil(start * span - _EPS) + (1 if wrong == 'window_lo_off_by_one' else 0)
    p_hi = math.floor(end * span + _EPS) + (1 if wrong == 'window_hi_off_by_one' else 0)
    lo, hi = min(max(p_lo - first, 0), k), min(max(p_hi - first, 0), k)
    return (lo, hi) if lo < hi else (0, 0)


def layer_scales(spec, wrong=None):
    """None -> ones; 'soft' -> 0.825 ** (12 - i); 13 finite numbers >= 0 -> themselves.  float64 [13]"""
    _check_wrong(wrong)
    if spec is None:
        v = np.ones(N_RESIDUALS, dtype=np.float64)
    elif isinstance(spec, str):
        if spec != 'soft':
            raise ValueError(f"control_layer_scales must be None, 'soft' or {N_RESIDUALS} numbers, got {spec!r}")
        v = SOFT_BASE ** (12.0 - np.arange(N_RESIDUALS, dtype=np.float64))
    else:
        try:
            v = np.array([float(x) for x in spec], dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError(f"control_layer_scales must be None, 'soft' or {N_RESIDUALS} numbers, got {spec!r}") from None
        if v.shape != (N_RESIDUALS,) or not np.all(np.isfinite(v)) or np.any(v < 0):
            raise ValueError(f"control_layer_scales must be {N_RESIDUALS} finite numbers >= 0, one per ControlNet residual")
    return v[::-1].copy() if wrong == 'layers_reversed' else v


def sample_scales(scale, n):
    """one number or n numbers, each finite and >= 0 -> float64 [n]"""
    n = int(n)
    try:
        v = np.asarray(scale, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"control_scale must be one number or {n} numbers, got {scale!r}") from None
    if v.ndim == 0:
        v = np.full(n, float(v))
    if v.shape != (n,):
        raise ValueError(f"control_scale must be one number or {n} numbers, one per sample: got shape {v.shape}")
    if not np.all(np.isfinite(v)) or np.any(v < 0):
        raise ValueError("control_scale must be finite and >= 0")
    return v


def scale_table(scale, layers, n, nb, cond_only=False, wrong=None):
    """-> float32 [nb * n, 13], rows in the order of the CFG batch [uncond | cond]: scale[j] * layers[i], the fp64 product
    rounded once; cond_only with nb == 2: the unconditional rows are exactly 0"""
    _check_wrong(wrong)
    nb = int(nb)
    if nb not in (1, 2):
        raise ValueError(f"nb is 1 (no CFG) or 2, got {nb}")
    s = sample_scales(scale, n)
    lay = layer_scales(layers, wrong if wrong == 'layers_reversed' else None)
    rows = (s[:, None] * lay[None, :]).astype(np.float32)
    tab = np.concatenate([rows] * nb, axis=0)
    if cond_only and nb == 2 and wrong != 'uncond_not_zeroed':
        tab[:int(n)] = 0.0
    return np.ascontiguousarray(tab)


def add_scaled(x, r, s, wrong=None):
    """the kernel's formula in fp64: x [B, ...] + s[b] * r [B, ...] per sample row; a row whose s[b] == 0 is x itself,
    whatever r holds there (NaN included)"""
    _check_wrong(wrong)
    x, r = np.asarray(x, dtype=np.float64), np.asarray(r, dtype=np.float64)
    s = np.asarray(s, dtype=np.float64).reshape(-1)
    if x.shape != r.shape or x.shape[0] != s.shape[0]:
        raise ValueError(f"x {x.shape} and r {r.shape} must agree, with one scale per row (got {s.shape[0]})")
    out = x.copy()
    for b in range(x.shape[0]):
        if s[b] != 0.0:
            out[b] = s[b] * x[b] + r[b] if wrong == 'scale_on_x' else x[b] + s[b] * r[b]
    return out


def normalise(scale, layers, window, cond_only, n, total, k, nb=2):
    """what a request's four control arguments come to, for its n samples and its run of k of `total` steps (nb: 1 without
    CFG, where cond_only means nothing):
      None                 the plain control request: every entry of the table is 1 and every step of the run is controlled
                           (all arguments at their defaults, however they are spelled)
      'off'                nothing is left of the control: an all-zero table or no controlled step
      (table, (lo, hi))    scale_table(...) and window_steps(...)
    Every argument is checked, whatever the outcome."""
    tab = scale_table(scale, layers, n, nb, cond_only)
    lo, hi = window_steps(total, k, window)
    if lo == hi or not np.any(tab):
        return 'off'
    if (lo, hi) == (0, int(k)) and np.all(tab == np.float32(1.0)):
        return None
    return tab, (lo, hi)
