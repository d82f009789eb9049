"""TEST INFRASTRUCTURE: the inputs, cases and tolerance that tests/test_img2img_cpu.py and tests/test_img2img_gpu.py
share, so that what the CPU file proves about the tolerance (every mutant of lib/img2img.py leaves it) is proved on the
very inputs the GPU file judges the kernel on.  numpy only; the reference itself is lib/img2img.py.

tools/make_img2img_golden.py takes `picture_u8` from here: the fixture's picture is a formula, not a file.
"""
import numpy as np

SEEDS = (0, -1, (1 << 40) + 12345)               # tests/test_device_noise_gpu.py::SEEDS
SAMPLE_IDS = (3, 1, 0x1_0000_0002)
SCALE_FACTOR = 0.18215                           # pfd.yaml latent_scale_factor
A_T, A_NEXT = 0.4375, 0.3125                     # the level of ddim_timesteps[k - 1], and of [k] (the 'level_of_k' mutant)
TOL = 1e-5                                       # tests/test_device_noise_gpu.py::close: the same generator, the same kind of fp32 chain

# (B, C, h, w): the three of the issue; C = 3 makes the sample length odd (the scalar stores; C = 4 never does); the last is
# one quad past the 1024 x 256 threads of the largest grid (csrc/latent.hip kMaxBlocks), B = Bm = 1 only
SHAPES = [(2, 4, 8, 8), (1, 4, 3, 5), (3, 4, 1, 1), (2, 3, 3, 5)]
PAST_THE_GRID = (1, 4, 1, (1 << 18) + 1)


def keys(B):
    """int64 [B, 2]: rows (seed, sample_id)"""
    return np.array([(SEEDS[i % 3], SAMPLE_IDS[i % 3] + i // 3) for i in range(B)], dtype=np.int64)


def moments(shape, Bm, kind='ordinary'):
    """f16 NHWC [Bm, h, w, 2C] as quant_conv writes them: means of a few units, logvars in [-8, 2] ('ordinary'), or
    logvars of -40 and +25 in turn ('clamp': both ends of the clamp)"""
    B, C, h, w = shape
    g = np.random.default_rng(B * 1000 + C * 100 + h * 10 + w + 7 * Bm)
    mean = 3.0 * g.standard_normal((Bm, h, w, C))
    if kind == 'clamp':
        logvar = np.where(np.arange(Bm * h * w * C).reshape(Bm, h, w, C) % 2 == 0, -40.0, 25.0)
    else:
        logvar = g.uniform(-8.0, 2.0, (Bm, h, w, C))
    return np.concatenate([mean, logvar], axis=-1).astype(np.float16)


def nchw(m):
    """NHWC moments -> [Bm, 2C, h, w] float64, the layout of lib/img2img.py"""
    return np.ascontiguousarray(np.transpose(np.asarray(m, dtype=np.float64), (0, 3, 1, 2)))


def reference(m_nhwc, key_rows, posterior='sample', **kw):
    """(x0, x_t) float32 [B, C, h, w] of lib/img2img.py at the shared scalars"""
    from lib import img2img
    return img2img.latent_start_batch(nchw(m_nhwc), key_rows, SCALE_FACTOR, A_T, posterior, a_next=A_NEXT, **kw)


def scaled_err(a, ref):
    """the figure tests/test_device_noise_gpu.py::close bounds: max|a - ref| / max(1, max|ref|)"""
    a, ref = np.asarray(a, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.abs(a - ref).max() / max(1.0, float(np.abs(ref).max())))


def _isin(p):
    """integer sinusoid: period 512, range [-256, 256] (a parabola per half period)"""
    q = p % 256
    v = (q * (256 - q)) >> 6
    return np.where((p // 256) % 2 == 0, v, -v)


def picture_u8(h, w, seed=0):
    """uint8 [h, w, 3]: smooth colour waves under three bits of hashed dither -- a closed integer formula, no RNG stream"""
    i = np.arange(h * w * 3, dtype=np.int64)
    y, x, ch = np.unravel_index(i, (h, w, 3))
    mix = (i * 2654435761 + (seed + 1) * 40503) & 0xFFFFFFFF
    v = 128 + ((_isin(7 * x + 85 * ch + 31 * seed) * _isin(5 * y + 128 + 17 * ch)) >> 9)
    v = np.clip(v, 0, 255) ^ ((mix >> 29) & 7)
    return np.clip(v, 0, 255).astype(np.uint8).reshape(h, w, 3)


def picture_f32(h, w, seed=0):
    """the picture as ToTensor gives it: float32 [1, 3, h, w] in [0, 1]"""
    return np.ascontiguousarray(np.transpose(picture_u8(h, w, seed).astype(np.float32) / 255.0, (2, 0, 1))[None])
