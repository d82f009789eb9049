"""TEST INFRASTRUCTURE: the shapes, the data and the bound of the guidance-rescale tests (lib/guidance.py, csrc/guidance.hip),
shared by tests/test_guidance_cpu.py (the kernel on the CPU emulation), tests/test_guidance_kernels_gpu.py and
tests/test_guidance_gpu.py (on the card).  numpy only.

The bound on |mul - f| / f against the fp64 specification is DERIVED (lib/guidance.py::error_bound): (L + 8) * 2^-24, L the
longest chain of fp32 additions an element passes through under the kernel's ownership rule (thread t owns the 8-element
groups t, t + 1024, ...; six levels in the wave, four over the waves): each of the sums of squares, whose terms have one
sign, carries at most L half-ulps of relative error, the ratio of two of them 2 L, its square root L; the + 8 covers the
two divisions by n, q_c / q_g, the square root, 1 - phi, the final fma and the second-order effect of the means' error.
"""
import os

import numpy as np

from lib import guidance as G

# (C, h, w): 120 elements -- fewer elements than threads (120 IS a multiple of 8: the scalar path is taken there only from an
# unaligned base); 75 -- n % 8 != 0, a short last group, samples that start off 16 bytes: the scalar path; 256 -- a group for
# some threads, none for the others; the flagship latent; 96 x 96 -- 4608 groups, the trip count does not divide evenly
# (4.5 per thread); 192 x 192 -- the 1536-pixel limit, the longest chain (run once, B = 1)
SHAPES = [(4, 6, 5), (3, 5, 5), (4, 8, 8), (4, 64, 64), (4, 96, 96)]
LONGEST = (4, 192, 192)
BATCHES = (1, 3)
SCALES = (2.0, 7.5, 12.0)
PHIS = (0.7, 0.25, 1.0)
MUTANT_MARGIN = 1e3


def bound(shape):
    return G.error_bound(int(np.prod(shape)))


def make_eps(B, shape, seed=0):
    """f16 NHWC [2B, h, w, C], unconditional half first: correlated halves with a non-zero mean that differs per sample
    and per half -- base + 0.15 noise +/- 0.04 -- so that every mutant of lib/guidance.py is visible (the mean: rms_not_std;
    the differing spread of the samples: stats_over_batch; eu narrower than ec: std_of_uncond)"""
    C, h, w = shape
    g = np.random.default_rng(1000 * seed + 100 * B + C * h * w)
    out = np.empty((2 * B, h, w, C), dtype=np.float16)
    for b in range(B):
        base = (0.6 + 0.35 * b) * g.standard_normal((h, w, C))
        out[b] = (0.9 * base + 0.15 * g.standard_normal((h, w, C)) - 0.04 + 0.5 + 0.3 * b).astype(np.float16)
        out[B + b] = (base + 0.15 * g.standard_normal((h, w, C)) + 0.04 + 0.5 + 0.3 * b).astype(np.float16)
    return out


def rows(values, B):
    """the first B of a tuple of per-sample numbers, as float32"""
    return np.array([values[b % len(values)] for b in range(B)], dtype=np.float32)


def rel_err(mul, f):
    mul, f = np.asarray(mul, dtype=np.float64), np.asarray(f, dtype=np.float64)
    return float(np.max(np.abs(mul - f) / np.abs(f)))


def strided(v, stride):
    """float32 [(B-1)*stride + 1] holding v at the given stride (stride 0: v must be constant), NaN elsewhere"""
    v = np.asarray(v, dtype=np.float32)
    if stride == 0:
        assert np.all(v == v[0])
        return v[:1].copy()
    out = np.full((v.size - 1) * stride + 1, np.nan, dtype=np.float32)
    out[::stride] = v
    return out


def emu_stats_case(path, eps, scale, phi, sstride=1, pstride=1, offset=0, null=0, rc=0, B=None, n=None):
    """write the input file of tools/cpu_emu/emu_guidance.cpp for a statistics case -> the case argument"""
    eps = np.ascontiguousarray(eps, dtype=np.float16)
    B = eps.shape[0] // 2 if B is None else B
    n = int(np.prod(eps.shape[1:])) if n is None else n
    with open(path, "wb") as f:
        f.write(eps.tobytes() + strided(scale, max(sstride, 0)).tobytes() + strided(phi, max(pstride, 0)).tobytes())
    return f"stats,{B},{n},{sstride},{pstride},{offset},{null},{rc},{path}"


def read_mul(path, B):
    return np.fromfile(path + ".mul", dtype=np.float32, count=B)
