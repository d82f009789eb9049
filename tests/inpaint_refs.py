"""TEST INFRASTRUCTURE: the inputs, cases and tolerance that tests/test_inpaint_cpu.py and tests/test_inpaint_gpu.py
share, so that what the CPU file proves about the tolerance (every mutant of lib/inpaint.py leaves it) is proved on the
very inputs the GPU file judges the kernels on.  numpy only; the reference itself is lib/inpaint.py.
"""
import functools

import numpy as np

import img2img_refs as I

TOL = I.TOL                                      # 1e-5 scaled max-abs: the same generator followed by the same kind of fp32 chain
keys = I.keys
scaled_err = I.scaled_err

# (B, C, h, w): w % 4 != 0 forces the scalar path; (2, 3, 3, 5) has an odd sample length; the last is one quad past the
# 4096 x 256 threads of the largest grid (csrc/pfd_common.h grid_for), B = 1 only
SHAPES = [(2, 4, 8, 8), (1, 4, 3, 5), (3, 4, 1, 1), (2, 3, 3, 5)]
PAST_THE_GRID = (1, 4, 1, (1 << 20) + 1)

FORMS = ('ddim', 'ddim_seeded', 'ddim_ps', 'dpm1', 'dpm2')
MASKS = ('binary', 'soft', 'ones', 'zeros')

# a three-row schedule; row 1 is stepped in the middle of a run (index 1), row 0 is the last step (index 0)
ALPHAS = np.array([0.9, 0.4375, 0.2])
ALPHAS_PREV = np.array([0.99, 0.9, 0.4375])
SCALE = 2.0
SIGMA = 0.3
NOISE_MUL = 0.75


def mask(kind, shape, Bm):
    """float32 [Bm, h, w] by formula; row b of a per-sample mask is the formula shifted by b (row 0 is the formula itself)"""
    B, C, h, w = shape
    b, y, x = np.meshgrid(np.arange(Bm), np.arange(h), np.arange(w), indexing='ij')
    if kind == 'binary':
        m = ((x + 2 * y + b) % 3 != 0)
    elif kind == 'soft':
        m = ((x + y + b) % 5) / 4.0
    elif kind == 'ones':
        m = np.ones((Bm, h, w))
    elif kind == 'zeros':
        m = np.zeros((Bm, h, w))
    else:
        raise ValueError(kind)
    return np.ascontiguousarray(m, dtype=np.float32)


def coef_row(form, index):
    """the fp32 coefficient row of `form` at step index 1 (mid-run) or 0 (the last step)"""
    from lib import solver
    if form.startswith('ddim'):
        a, ap = ALPHAS[index], ALPHAS_PREV[index]
        sg = SIGMA if form == 'ddim_seeded' else 0.0
        return np.array([a, ap, sg, np.sqrt(1.0 - a), SCALE], dtype=np.float32)
    return solver.dpmpp_2m_table(ALPHAS, ALPHAS_PREV, SCALE, 2 if form == 'dpm2' else 1)[index].astype(np.float32)


@functools.lru_cache(maxsize=None)
def tensors(shape, nb):
    """(eps f16 NHWC [nb*B,h,w,C], x, x0_prev, x0 fp32 NCHW): unit-scale latents, a history and a clean latent of a few units"""
    B, C, h, w = shape
    g = np.random.default_rng(B * 1000 + C * 100 + h * 10 + (w % 1000) + 7 * nb)
    eps = g.standard_normal((nb * B, h, w, C)).astype(np.float16)
    x = g.standard_normal(shape).astype(np.float32)
    hist = (1.5 * g.standard_normal(shape)).astype(np.float32)
    x0 = (2.0 * g.standard_normal(shape)).astype(np.float32)
    return eps, x, hist, x0


def case(form, shape, Bm=1, mask_kind='binary', nb=2, rep=1, last=False):
    """everything one launch takes, as a dict of host arrays and numbers"""
    from lib import inpaint
    B = shape[0]
    index = 0 if last else 1
    eps, x, hist, x0 = tensors(tuple(shape), nb)
    ksq, ks = inpaint.step_constants(ALPHAS_PREV[index], index)
    return dict(form=form, shape=tuple(shape), Bm=Bm, nb=nb, rep=rep, index=index, eps=eps, x=x, x0=x0,
                x0_prev=hist if form == 'dpm2' and not last else None, coef=coef_row(form, index), keys=keys(B),
                mask=mask(mask_kind, shape, Bm), mask_kind=mask_kind, ksq=ksq, ks=ks,
                solver='ddim' if form.startswith('ddim') else 'dpmpp', noise_mul=NOISE_MUL if form == 'ddim_seeded' else 1.0,
                scale=np.linspace(1.0, 3.0, B).astype(np.float32) if form == 'ddim_ps' else None,
                a_prev=float(ALPHAS_PREV[index]))


def reference(c, wrong=None):
    """(x_out, pred_x0, xin_next [B,h,w,C] f16) of lib/inpaint.py on a case"""
    from lib import inpaint
    return inpaint.masked_step(c['eps'], c['nb'], c['x'], c['coef'], c['keys'], c['index'], c['x0'], c['mask'], c['ksq'],
                               c['ks'], solver=c['solver'], x0_prev=c['x0_prev'], noise_mul=c['noise_mul'], scale=c['scale'],
                               wrong=wrong, a_prev=c['a_prev'])


def xin_err(xin, ref_x_out):
    """the next UNet input against the specification's x_out, [B,h,w,C] against [B,C,h,w]: the largest excess of
    |float(xin) - x_out| over the half ulp that rounding ANY fp32 number to f16 may cost (2^-11 relative; 2^-25 below the
    normal range), scaled like scaled_err.  xin is half(x_out) of the DEVICE's x_out (asserted bit for bit on its own), and
    that x_out is within TOL of the specification's, so this figure is bounded by TOL -- while half(device x_out) and
    half(specification x_out) themselves may differ by a whole f16 ulp where the two straddle a rounding boundary."""
    ref = np.transpose(np.asarray(ref_x_out, dtype=np.float64), (0, 2, 3, 1))
    got = np.asarray(xin, dtype=np.float64)
    half_ulp = np.maximum(np.abs(got) * 2.0 ** -11, 2.0 ** -25)
    return float(np.maximum(np.abs(got - ref) - half_ulp, 0.0).max() / max(1.0, float(np.abs(ref).max())))


def cases():
    """the cases both files judge on (the past-the-grid shape apart): every shape x form, Bm in {1, B}, the four masks, both
    rep and nb, and the last step's constants -- spread so that every value of every axis meets every form"""
    out = []
    for si, shape in enumerate(SHAPES):
        for fi, form in enumerate(FORMS):
            for Bm in sorted({1, shape[0]}):
                kind = MASKS[(si + fi + Bm) % 2]                     # binary / soft in turn
                out.append(case(form, shape, Bm, kind, nb=2 - (si + fi) % 2, rep=1 + (si + fi + Bm) % 2))
            out.append(case(form, shape, 1, 'binary', last=True, rep=2))
    for form in FORMS:
        for kind in ('ones', 'zeros'):
            out.append(case(form, SHAPES[0], 1, kind))
    return out


def name(c):
    return f"{c['form']} {c['shape']} Bm={c['Bm']} {c['mask_kind']} nb={c['nb']} rep={c['rep']} index={c['index']}"


# ---- masks and pictures for the ingest and the composite ---------------------------------------------------------------
GRIDS = [((96, 72), (8, 8)), ((5, 7), (8, 8)), ((64, 64), (64, 64)), ((100, 80), (64, 64))]


def mask_u8(Hm, Wm, seed=0):
    """uint8 [Hm, Wm]: blobs of both kinds with values on both sides of 128, 127 and 128 included"""
    y, x = np.meshgrid(np.arange(Hm), np.arange(Wm), indexing='ij')
    v = (37 * x + 91 * y + 13 * seed + ((x * y) % 7) * 29) % 256
    blob = (((7 * x) // Wm + (5 * y) // Hm + seed) % 4 == 0)      # 7 x 5 bands whatever the size: a quarter of them marked
    return np.where(blob, np.where(v % 2 == 0, 128, v), np.where(v % 3 == 0, 127, v // 2)).astype(np.uint8)


def worked_masks():
    """the two worked masks of the specification: 96 x 72 -> 8 x 8 (cells of 12 x 9 pixels) and the cells they give"""
    a = np.zeros((96, 72), dtype=np.uint8)
    a[24:72, 18:54] = 255
    b = np.zeros((96, 72), dtype=np.uint8)
    b[30:41, 20:31] = 200
    wa = np.zeros((8, 8), dtype=np.float32)
    wa[2:6, 2:6] = 1
    wb = np.zeros((8, 8), dtype=np.float32)
    wb[2:4, 2:4] = 1
    return (a, wa), (b, wb)
