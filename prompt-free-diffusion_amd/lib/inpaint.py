"""Masked regeneration (inpainting) on the host -- numpy only.

The device evaluates the same functions in csrc/step.hip (pfd_cfg_step_masked) and csrc/inpaint.hip (pfd_mask_grid_u8, pfd_composite_u8);
this module is the specification restated in fp64, the oracle of the tests, and the way to reproduce a masked request
without a GPU.  The reference has no masked path (its ddim.py has none): the specification is this file.

Mask grid.  A uint8 mask [Hm, Wm] of any size, value >= 128 meaning "regenerate", becomes a binary grid [gh, gw]: cell y
covers mask rows lo = (y*Hm)//gh up to hi = max(lo + 1, ceil((y+1)*Hm/gh)) in integer arithmetic, columns alike, and is
1 if any pixel of its footprint is >= 128.  Footprints are never empty and together cover the mask, so a marked pixel
always lies in a regenerated cell: the rule dilates and never erodes.  The same rule serves the latent grid (H/8, W/8)
as float32 and the pixel grid (H, W) as uint8 0/1 for the composite.

Masked step.  For element e = (c*h + y)*w + x of sample (seed, sample_id) at step index `index`, with the constants
(ksq, ks) = (sqrt(a_prev), sqrt(1 - a_prev)) of the row being stepped to, rounded to fp32 by the host
(img2img.kernel_scalars(1, a_prev)[1:]), and (1, 0) exactly at the last step (index == 0):

    xp    = the unmasked update of the solver (DDIM with or without seeded step noise, DPM-Solver++ order 1 or 2)
    known = ksq * x0[e] + ks * z_keep,   z_keep = noise.normal(seed, sample_id, index, ., stream=3)[e]
    x_out = m * xp + (1 - m) * known     (in exactly this form: m = 1 gives xp's bits, m = 0 gives known's)

pred_x0 is the unmasked one, the next UNet input is half(x_out), and m = mask[b or 0, y, x] is the same for every channel;
soft values in [0, 1] are legal.  The kept region therefore follows the init picture's own forward trajectory, drawn from
the sample's key, and ends as x0 itself.

Composite.  out[n, y, x, :] = sel[y, x] ? decoded[n, y, x, :] : init_u8_resized[y, x, :].
"""
import numpy as np

from . import noise
from .img2img import kernel_scalars

SOLVERS = ('ddim', 'dpmpp')
MUTANTS = ('mask_inverted', 'stream0', 'no_keep_noise', 'level_of_t', 'last_step_noised', 'mask_channel_major',
           'blend_pred_x0')


def footprint(i, n_in, n_out):
    """[lo, hi) of cell i of n_out over an axis of n_in pixels"""
    lo = (i * n_in) // n_out
    return lo, max(lo + 1, -((-(i + 1) * n_in) // n_out))


def mask_grid(mask, gh, gw, dtype=np.float32):
    """uint8 [Hm, Wm] | [Hm, Wm, 1] -> [gh, gw] of 0 / 1 in `dtype` (stacked masks: mask_grid_batch)"""
    m = np.asarray(mask)
    if m.ndim == 3 and m.shape[2] == 1:
        m = m[:, :, 0]
    if m.ndim != 2 or m.dtype != np.uint8:
        raise ValueError(f"mask must be uint8 [Hm, Wm] or [Hm, Wm, 1], got {m.dtype} {m.shape}")
    gh, gw = int(gh), int(gw)
    if gh < 1 or gw < 1 or m.shape[0] < 1 or m.shape[1] < 1:
        raise ValueError("mask and grid sides must be positive")
    on = m >= 128
    out = np.zeros((gh, gw), dtype=dtype)
    rows = [footprint(y, m.shape[0], gh) for y in range(gh)]
    cols = [footprint(x, m.shape[1], gw) for x in range(gw)]
    for y, (y0, y1) in enumerate(rows):
        band = on[y0:y1].any(axis=0)
        for x, (x0, x1) in enumerate(cols):
            out[y, x] = 1 if band[x0:x1].any() else 0
    return out


def mask_grid_batch(masks, gh, gw, dtype=np.float32):
    """uint8 [Bm, Hm, Wm] -> [Bm, gh, gw]"""
    return np.stack([mask_grid(m, gh, gw, dtype) for m in np.asarray(masks)])


def composite(decoded, init, sel):
    """decoded uint8 [n, H, W, C], init uint8 [1 | n, H, W, C], sel [1 | n, H, W] (nonzero: keep decoded) -> uint8 [n, H, W, C]"""
    d, i, s = np.asarray(decoded), np.asarray(init), np.asarray(sel)
    if d.ndim != 4 or i.ndim != 4 or s.ndim != 3 or i.shape[0] not in (1, d.shape[0]) or s.shape[0] not in (1, d.shape[0]) \
            or i.shape[1:] != d.shape[1:] or s.shape[1:] != d.shape[1:3]:
        raise ValueError(f"composite: decoded {d.shape}, init {i.shape}, sel {s.shape} do not go together")
    return np.where((s != 0)[..., None], d, np.broadcast_to(i, d.shape)).astype(np.uint8)


def step_constants(a_prev, index):
    """(ksq, ks) of the step with index `index` that steps to the level a_prev, as the fp32 numbers the kernel is handed:
    (sqrt(a_prev), sqrt(1 - a_prev)), and (1, 0) exactly at the last step"""
    if int(index) == 0:
        return np.float32(1.0), np.float32(0.0)
    return kernel_scalars(1.0, a_prev)[1:]


def masked_step(eps, nb, x, coef, keys, index, x0, mask, ksq, ks, solver='ddim', x0_prev=None, noise_mul=1.0,
                scale=None, wrong=None, a_prev=None):
    """One masked step.  eps: f16 NHWC [nb*B, h, w, C] (unconditional batch first); x, x0, x0_prev: [B, C, h, w]; coef:
    the fp32 row of the solver (DDIM {a_t, a_prev, sigma, sqrt(1-a_t), scale}; DPM-Solver++ {a_t, sqrt(1-a_t), c_x, c_d,
    w_cur, w_prev, scale, 0}, x0_prev None for a first-order step); keys: int64 [B, 2]; mask: [1 | B, h, w] in [0, 1];
    scale: None or [B].  -> (x_out f32 [B,C,h,w], pred_x0 f32 [B,C,h,w], xin_next f16 NHWC [B,h,w,C]).
    wrong: None or one of MUTANTS, a named way to get it wrong ('last_step_noised' needs a_prev, the level of the last row)."""
    if solver not in SOLVERS:
        raise ValueError(f"solver must be one of {SOLVERS}, got {solver!r}")
    if wrong is not None and wrong not in MUTANTS:
        raise ValueError(f"unknown mutant {wrong!r}")
    x = np.asarray(x, dtype=np.float64)
    B, C, h, w = x.shape
    e_all = np.asarray(eps, dtype=np.float64).reshape(nb, B, h, w, C).transpose(0, 1, 4, 2, 3)     # -> [nb, B, C, h, w]
    coef = [float(np.float32(v)) for v in np.asarray(coef).reshape(-1)]
    keys = np.asarray(keys, dtype=np.int64).reshape(B, 2)
    x0 = np.asarray(x0, dtype=np.float64)
    m_all = np.asarray(mask, dtype=np.float64)
    if m_all.ndim != 3 or m_all.shape[0] not in (1, B) or m_all.shape[1:] != (h, w) or x0.shape != x.shape:
        raise ValueError(f"mask must be [1 | {B}, {h}, {w}] and x0 like x, got {m_all.shape}, {x0.shape}")
    s_all = coef[4 if solver == 'ddim' else 6]
    sc = np.full(B, s_all) if scale is None else np.asarray(scale, dtype=np.float32).astype(np.float64).reshape(B)
    sc = sc[:, None, None, None]
    e = e_all[0] + sc * (e_all[1] - e_all[0]) if nb == 2 else e_all[0] * sc
    ns = C * h * w
    ksq, ks = float(np.float32(ksq)), float(np.float32(ks))
    if solver == 'ddim':
        a_t, a_p, sigma, s1mat = coef[:4]
        p0 = (x - s1mat * e) * (1.0 / np.sqrt(a_t))
        xp = np.sqrt(a_p) * p0 + np.sqrt(max(1.0 - a_p - sigma * sigma, 0.0)) * e
        if sigma != 0.0:
            z = np.stack([noise.normal64(int(k[0]), int(k[1]), index, ns, stream=noise.STREAM_STEP) for k in keys])
            xp = xp + sigma * (float(np.float32(noise_mul)) * z.reshape(x.shape))
    else:
        a_t, s1mat, c_x, c_d, w_cur, w_prev = coef[:6]
        p0 = (x - s1mat * e) * (1.0 / np.sqrt(a_t))
        d = p0 if x0_prev is None else w_cur * p0 + w_prev * np.asarray(x0_prev, dtype=np.float64)
        xp = c_x * x + c_d * d
    if wrong == 'level_of_t':
        ksq, ks = (float(v) for v in kernel_scalars(1.0, min(max(coef[0], 0.0), 1.0))[1:])
    if wrong == 'last_step_noised' and (ksq, ks) == (1.0, 0.0):
        if a_prev is None:
            raise ValueError("'last_step_noised' needs a_prev")
        ksq, ks = (float(v) for v in kernel_scalars(1.0, a_prev)[1:])
    known = ksq * x0
    if ks != 0.0 and wrong != 'no_keep_noise':
        stream = noise.STREAM_STEP if wrong == 'stream0' else noise.STREAM_KEEP
        zk = np.stack([noise.normal64(int(k[0]), int(k[1]), index, ns, stream=stream) for k in keys])
        known = known + ks * zk.reshape(x.shape)
    m = np.broadcast_to(m_all[:, None], (m_all.shape[0], C, h, w))
    if wrong == 'mask_channel_major':      # the mask read as if it were [h, w, C]
        c_i, y_i, x_i = np.meshgrid(np.arange(C), np.arange(h), np.arange(w), indexing='ij')
        idx = ((y_i * w + x_i) * C + c_i) % (h * w)
        m = m_all.reshape(m_all.shape[0], h * w)[:, idx]
    if wrong == 'mask_inverted':
        m = 1.0 - m
    x_out = m * xp + (1.0 - m) * known
    pred = m * p0 + (1.0 - m) * x0 if wrong == 'blend_pred_x0' else p0
    x_out = x_out.astype(np.float32)
    return x_out, pred.astype(np.float32), np.ascontiguousarray(x_out.transpose(0, 2, 3, 1)).astype(np.float16)
