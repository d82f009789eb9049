"""TEST INFRASTRUCTURE: the inputs, cases and tolerance of the second-pass start of a two-pass request, shared by
tests/test_hires_cpu.py today and meant for the GPU test of a device implementation later: what the CPU file proves about the
tolerance (every mutant of lib/hires.py leaves it) is proved on the very inputs such a kernel will be judged on.  numpy only;
the reference itself is lib/hires.py."""
import functools

import numpy as np

from img2img_refs import A_NEXT, A_T, SAMPLE_IDS, SEEDS, TOL, keys, picture_u8, scaled_err  # noqa: F401  (shared with img2img)

MODES = ('nearest', 'bilinear', 'bicubic')

# (B, C, h, w, h2, w2): integer ratio with vector stores; ratios 3/2 and 4/3; an odd sample length (scalar stores and a dropped
# tail; C = 4 never gives one); every tap clamped; the identity; one axis unchanged
CASES = [(2, 4, 8, 8, 16, 16), (1, 4, 8, 12, 12, 16), (2, 3, 3, 5, 5, 7), (3, 4, 1, 1, 4, 4), (1, 4, 6, 6, 6, 6), (2, 4, 5, 7, 5, 16)]
IDENTITY = CASES[4]
# one quad past 1024 x 256 threads (the largest grid of csrc/latent.hip, one thread per four elements), B = 1
PAST_THE_GRID = (1, 4, 1, 65536, 1, 262145)
ALL_CASES = CASES + [PAST_THE_GRID]


def latent(case):
    """fp32 [B, C, h, w]: Gaussian at latent magnitudes (std about 5)"""
    B, C, h, w, h2, w2 = case
    g = np.random.default_rng(B * 100000 + C * 10000 + h * 1000 + w * 100 + h2 * 10 + w2)
    return (5.0 * g.standard_normal((B, C, h, w))).astype(np.float32)


@functools.lru_cache(maxsize=None)
def reference(case, mode):
    """(r, x_t) float32 [B, C, h2, w2] of lib/hires.py at the shared scalars: computed once, shared, never modified"""
    from lib import hires
    r, xt = hires.hires_start_batch(latent(case), keys(case[0]), A_T, case[4:], mode)
    r.setflags(write=False)
    xt.setflags(write=False)
    return r, xt


def mutant(case, mode, wrong):
    from lib import hires
    return hires.hires_start_batch(latent(case), keys(case[0]), A_T, case[4:], mode, wrong=wrong, a_next=A_NEXT)
