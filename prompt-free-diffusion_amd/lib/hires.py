"""The start of the second pass of a two-pass ("hires fix") request, on the host -- numpy only.

This module is the specification in fp64 and the way to compute a request's second start on the host.  The device
launch that evaluates it and generate(hires=...) / submit(hires=...) above it are NOT part of the library yet (DESIGN.md
3.19 says why); what is fixed here is what they will have to compute, bit rule by bit rule.

A picture is composed at the size the model was trained for; its clean latent x [C, h, w] is enlarged to [C, h2, w2] and
noised part of the way, and the last k2 = hires_steps(steps2, strength2) steps run at the large size from

    r   = resample(x, h2, w2, mode)
    x_t = sqrt(a_t) * r + sqrt(1 - a_t) * z                  (pfd.py:204-207)
    a_t = alphas_cumprod[ddim_timesteps[k2 - 1]]             (the first timestep evaluated, as lib/img2img.py)

where, for element e2 = (c*h2 + y)*w2 + x of the OUTPUT of sample (seed, sample_id),
z = noise.normal(seed, sample_id, 0, ., stream=4)[e2]: nothing is drawn from a generator, so a sample's start depends on
its key and its first-pass latent alone -- not on its batch, not on the world size.

The resample is separable; rows and columns each use the one-dimensional taps below, defined by exact integer arithmetic
so that fp32 and fp64 pick the same source index everywhere (d: output index, n_in -> n_out, n_out >= n_in):

  'nearest'   i = min((d * n_in) // n_out, n_in - 1)
  'bilinear', 'bicubic' (half-pixel centres, align_corners=False):
              num = (2d + 1) * n_in - n_out;  i0 = floor(num / (2 n_out));  t = (num - i0 * 2 n_out) / (2 n_out)
  'bilinear'  num < 0: i0 = 0, t = 0.  Taps (i0, min(i0 + 1, n_in - 1)), weights (1 - t, t)
  'bicubic'   taps i0 - 1 .. i0 + 2, each index clamped to [0, n_in - 1]; weights the Keys cubic with A = -0.75 written
              as torch writes it: ((A + 2) u - (A + 3)) u^2 + 1 for the inner two taps (u = t, 1 - t) and
              ((A u - 5A) u + 8A) u - 4A for the outer two (u = t + 1, 2 - t)

In fp64 'bilinear' and 'bicubic' agree with torch.nn.functional.interpolate(..., align_corners=False) on float64 input to
a few 1e-14.  The integer 'nearest' rule is the specification, NOT torch's: torch computes floor(d * scale) with an fp32
scale and picks another index at 372 of the 19 344 size pairs with n_in <= 129, n_out <= 4 n_in (the first is 14 -> 46 at
d = 23); compare with torch only at sizes where the two agree (TORCH_NEAREST_AGREES).

Only h2 >= h and w2 >= w are legal: there is no antialiased reduction, and reducing a latent is not what this is for.

What a kernel is handed as fp32 numbers -- sqrt(a_t), sqrt(1 - a_t) -- is rounded to fp32 here too, before the fp64
arithmetic (as lib/img2img.py does).
"""
import numpy as np

from . import noise
from .img2img import level, start_steps  # noqa: F401  (level: the same rule as an img2img start)

MODES = ('nearest', 'bilinear', 'bicubic')
MODE_ID = {'nearest': 0, 'bilinear': 1, 'bicubic': 2}          # the number a device entry point will take as `mode`
STREAM_HIRES = noise.STREAM_HIRES
CUBIC_A = -0.75
MUTANTS = ('align_corners', 'catmull_rom', 'edge_zero', 'axes_swapped', 'nearest_round', 'stream_q', 'level_of_k',
           'element_index_of_input')
# (n_in, n_out) at which torch's fp32 nearest rule picks the indices of the integer rule
TORCH_NEAREST_AGREES = ((8, 12), (5, 9), (7, 16), (8, 16), (12, 24), (6, 6), (3, 11), (4, 5), (64, 96), (64, 128), (64, 80))


def check_mode(mode):
    if mode not in MODES:
        raise ValueError(f"hires_resample must be 'nearest', 'bilinear' or 'bicubic', got {mode!r}")
    return mode


def hires_steps(steps, strength):
    """k2 = min(steps, int(steps * strength)): the number of steps the second pass runs, over ddim_timesteps[:k2] --
    img2img.start_steps.  ValueError unless 0 < strength <= 1 and k2 >= 1."""
    return start_steps(steps, strength)


def kernel_scalars(a_t):
    """(sqrt(a_t), sqrt(1 - a_t)) as the fp32 numbers a kernel is handed"""
    a_t = float(a_t)
    if not 0.0 <= a_t <= 1.0:
        raise ValueError(f"a_t must be in [0, 1], got {a_t!r}")
    return np.float32(np.sqrt(a_t)), np.float32(np.sqrt(1.0 - a_t))


def cubic_weights(t, A=CUBIC_A):
    """the four weights of taps i0 - 1 .. i0 + 2 at fraction t, [..., 4]"""
    t = np.asarray(t, dtype=np.float64)

    def inner(u):
        return ((A + 2.0) * u - (A + 3.0)) * u * u + 1.0

    def outer(u):
        return ((A * u - 5.0 * A) * u + 8.0 * A) * u - 4.0 * A
    return np.stack([outer(t + 1.0), inner(t), inner(1.0 - t), outer(2.0 - t)], axis=-1)


def taps(n_in, n_out, mode, wrong=None, ratio=None):
    """-> (index int64 [n_out, T], weight float64 [n_out, T]), T = 1 / 2 / 4 for nearest / bilinear / bicubic.
    ratio: (r_in, r_out) the coordinates are computed with (the 'axes_swapped' mutant); indices stay inside n_in."""
    check_mode(mode)
    n_in, n_out = int(n_in), int(n_out)
    if n_in < 1 or n_out < n_in:
        raise ValueError(f"cannot resample {n_in} to {n_out}: only enlarging (n_out >= n_in >= 1) is defined")
    r_in, r_out = (n_in, n_out) if ratio is None else (int(ratio[0]), int(ratio[1]))
    d = np.arange(n_out, dtype=np.int64)
    if mode == 'nearest':
        i = (d * r_in) // r_out
        if wrong == 'nearest_round':
            i = (2 * d * r_in + r_out) // (2 * r_out)
        return np.minimum(i, n_in - 1)[:, None], np.ones((n_out, 1))
    if wrong == 'align_corners':
        src = d.astype(np.float64) * ((r_in - 1) / (r_out - 1) if r_out > 1 else 0.0)
        i0 = np.floor(src).astype(np.int64)
        t = src - i0
    else:
        num = (2 * d + 1) * r_in - r_out
        i0 = num // (2 * r_out)                                   # floor division, also of negative num
        t = (num - i0 * 2 * r_out).astype(np.float64) / (2 * r_out)
        if mode == 'bilinear' and wrong != 'edge_zero':
            i0, t = np.where(num < 0, 0, i0), np.where(num < 0, 0.0, t)
    if mode == 'bilinear':
        idx, wt = np.stack([i0, i0 + 1], axis=-1), np.stack([1.0 - t, t], axis=-1)
    else:
        idx = i0[:, None] + np.arange(-1, 3, dtype=np.int64)[None, :]
        wt = cubic_weights(t, -0.5 if wrong == 'catmull_rom' else CUBIC_A)
    if wrong == 'edge_zero':
        wt = np.where((idx < 0) | (idx > n_in - 1), 0.0, wt)
    return np.clip(idx, 0, n_in - 1), wt


def resample(x, h2, w2, mode='bicubic', wrong=None):
    """x [..., h, w] -> float64 [..., h2, w2]"""
    x = np.asarray(x, dtype=np.float64)
    h, w = x.shape[-2:]
    tap_wrong = wrong if wrong in ('align_corners', 'catmull_rom', 'edge_zero', 'nearest_round') else None
    swap = wrong == 'axes_swapped'
    iy, wy = taps(h, h2, mode, tap_wrong, ratio=(w, w2) if swap else None)
    ix, wx = taps(w, w2, mode, tap_wrong, ratio=(h, h2) if swap else None)
    cols = sum(x[..., ix[:, j]] * wx[:, j] for j in range(ix.shape[1]))                       # [..., h, w2]
    return sum(cols[..., iy[:, j], :] * wy[:, j][:, None] for j in range(iy.shape[1]))       # [..., h2, w2]


def hires_start(x, seed, sample_id, a_t, size, mode='bicubic', wrong=None, a_next=None):
    """x [C, h, w], the clean latent of the first pass -> (r, x_t), float32 [C, h2, w2] each; size = (h2, w2).
    wrong: None, or one of MUTANTS -- a named way to get it wrong, for the tests to show that their tolerance tells the
    specification from its neighbours ('level_of_k' needs a_next, the level of ddim_timesteps[k2])."""
    check_mode(mode)
    if wrong is not None and wrong not in MUTANTS:
        raise ValueError(f"unknown mutant {wrong!r}")
    x = np.asarray(x, dtype=np.float64)
    if x.ndim != 3:
        raise ValueError(f"x must be [C, h, w], got {x.shape}")
    C, h, w = x.shape
    h2, w2 = int(size[0]), int(size[1])
    if h2 < h or w2 < w:
        raise ValueError(f"cannot resample {h} x {w} to {h2} x {w2}: only enlarging is defined")
    r = resample(x, h2, w2, mode, wrong)
    stream = noise.STREAM_Q if wrong == 'stream_q' else STREAM_HIRES
    if wrong == 'element_index_of_input':      # the noise of the input grid, carried along to the output
        zi = noise.normal64(seed, sample_id, 0, C * h * w, stream=stream).reshape(C, h, w)
        z = zi[:, taps(h, h2, 'nearest')[0][:, 0]][:, :, taps(w, w2, 'nearest')[0][:, 0]]
    else:
        z = noise.normal64(seed, sample_id, 0, C * h2 * w2, stream=stream).reshape(C, h2, w2)
    if wrong == 'level_of_k':
        if a_next is None:
            raise ValueError("'level_of_k' needs a_next")
        a_t = a_next
    sq_at, sq_1mat = (float(v) for v in kernel_scalars(a_t))
    x_t = sq_at * r + sq_1mat * z
    return r.astype(np.float32), x_t.astype(np.float32)


def hires_start_batch(x, keys, a_t, size, mode='bicubic', **kw):
    """x [B, C, h, w], keys [B, 2] rows (seed, sample_id) -> (r, x_t), float32 [B, C, h2, w2] each"""
    x = np.asarray(x)
    keys = np.asarray(keys, dtype=np.int64).reshape(-1, 2)
    if x.ndim != 4 or x.shape[0] != keys.shape[0]:
        raise ValueError(f"x must be [{keys.shape[0]}, C, h, w], got {x.shape}")
    outs = [hires_start(x[b], int(keys[b, 0]), int(keys[b, 1]), a_t, size, mode, **kw) for b in range(keys.shape[0])]
    return np.stack([o[0] for o in outs]), np.stack([o[1] for o in outs])
