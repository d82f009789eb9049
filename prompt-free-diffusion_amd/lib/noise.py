"""Seeded counter-based noise of the stochastic DDIM step (eta > 0), on the host -- numpy only.

The device evaluates the same function inside the step kernel (csrc/philox.h, pfd_cfg_ddim_step_rng); this module
is the specification restated, the oracle of the tests, and the way to reproduce a request's noise without a GPU.

The noise of element e (NCHW order inside the sample, e = (c*h + y)*w + x) of sample (seed, sample_id) at DDIM
step index `step` is output word e & 3 -> normal of

    Philox4x32-10(counter = (e >> 2, step, sample_id & 0xffffffff, stream),
                  key     = (seed & 0xffffffff, (seed >> 32) & 0xffffffff))

`stream` is 0 for the step noise (the word was always 0: those draws are what they were), 1 for the forward-noising
noise and 2 for the posterior noise of an img2img start (lib/img2img.py, csrc/latent.hip), both at step 0, and 3 for the
noise the kept region of a masked step is re-noised with (lib/inpaint.py, csrc/step.hip), at that step's index, and 4
for the noise the enlarged latent of a two-pass request is re-noised with (lib/hires.py; host only so far), at step 0 and
indexed by the element of the enlarged latent;

with words (r0, r1) -> (z0, z1) and (r2, r3) -> (z2, z3) by Box-Muller:

    u = ((ra >> 8) + 1) * 2^-24  in (0, 1],   v = (rb >> 8) * 2^-24  in [0, 1)
    rad = sqrt(-2 ln u),   z_even = rad * cos(2 pi v),   z_odd = rad * sin(2 pi v)

so |z| <= sqrt(-2 ln 2^-24) = 5.7681...  The device computes in fp32 (accurate logf / sinpif / cospif); `normal`
computes in fp64 and rounds once.
"""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
_MASK = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """counter [..., 4], key [..., 2] (anything numpy turns into uint32 words; broadcast against each other) ->
    uint32 [..., 4]"""
    c = np.asarray(counter, dtype=np.uint64) & np.uint64(_MASK)
    k = np.asarray(key, dtype=np.uint64) & np.uint64(_MASK)
    c0, c1, c2, c3 = (c[..., i] for i in range(4))
    k0, k1 = k[..., 0], k[..., 1]
    mask, s32 = np.uint64(_MASK), np.uint64(32)
    for _ in range(10):
        p0 = np.uint64(M0) * c0      # < 2^64: both factors are 32-bit
        p1 = np.uint64(M1) * c2
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & mask, (p0 >> s32) ^ c3 ^ k1, p0 & mask
        k0 = (k0 + np.uint64(W0)) & mask
        k1 = (k1 + np.uint64(W1)) & mask
    return np.stack(np.broadcast_arrays(c0, c1, c2, c3), axis=-1).astype(np.uint32)


def key_words(seed):
    """the two 32-bit key words of an int64 seed (two's complement: negative seeds are fine)"""
    seed = int(seed)
    return seed & _MASK, (seed >> 32) & _MASK


STREAM_STEP, STREAM_Q, STREAM_POSTERIOR = 0, 1, 2
STREAM_KEEP = 3
STREAM_HIRES = 4


def normal(seed, sample_id, step, n, stream=0):
    """float32 [n]: the noise of the first n elements of sample (seed, sample_id) at DDIM step `step` in `stream`"""
    return normal64(seed, sample_id, step, n, stream).astype(np.float32)


def normal64(seed, sample_id, step, n, stream=0):
    """`normal` before its one rounding: float64 [n]"""
    n = int(n)
    nq = (n + 3) // 4
    ctr = np.zeros((nq, 4), dtype=np.uint64)
    ctr[:, 0] = np.arange(nq, dtype=np.uint64)
    ctr[:, 1] = int(step) & _MASK
    ctr[:, 2] = int(sample_id) & _MASK
    ctr[:, 3] = int(stream) & _MASK
    r = philox4x32_10(ctr, np.array(key_words(seed), dtype=np.uint64)).astype(np.uint64)
    ra, rb = r[:, 0::2], r[:, 1::2]                                   # [nq, 2] each: (r0, r2), (r1, r3)
    u = ((ra >> np.uint64(8)) + np.uint64(1)).astype(np.float64) * 2.0 ** -24
    v = (rb >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
    rad = np.sqrt(-2.0 * np.log(u))
    ang = 2.0 * np.pi * v
    z = np.stack([rad * np.cos(ang), rad * np.sin(ang)], axis=-1)     # [nq, 2, 2] -> z0 z1 z2 z3
    return z.reshape(-1)[:n]


def sample_keys(seed, first, count):
    """int64 [count, 2] key rows {seed, sample_id} of samples first .. first + count - 1 of a request / global batch"""
    k = np.empty((int(count), 2), dtype=np.int64)
    k[:, 0] = int(seed)
    k[:, 1] = np.arange(int(first), int(first) + int(count), dtype=np.int64)
    return k
