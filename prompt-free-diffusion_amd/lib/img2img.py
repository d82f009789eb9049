"""The seeded latent start of an image-to-image request, on the host -- numpy only.

The device evaluates the same function in one kernel (csrc/latent.hip, pfd_latent_start); this module is the
specification restated in fp64, the oracle of the tests, and the way to reproduce a request's start without a GPU.

An img2img request of `steps` DDIM steps at `strength` runs the k = start_steps(steps, strength) steps
ddim_timesteps[:k] (reversed) from

    std = exp(0.5 * clamp(logvar, -30, 20))                  (distributions.py:24-62)
    x0  = scale_factor * (mean + std * z_p)                  ('mode': scale_factor * mean)
    x_t = sqrt(a_t) * x0 + sqrt(1 - a_t) * z_q               (pfd.py:204-207)
    a_t = alphas_cumprod[ddim_timesteps[k - 1]]

where mean / logvar are the two halves of the VAE encoder's moments and, for element e = (c*h + y)*w + x of sample
(seed, sample_id), z_q = noise.normal(seed, sample_id, 0, ., stream=1)[e] and z_p = (... stream=2)[e]: nothing is drawn
from a generator, so a sample's start depends on its key alone -- not on its batch, not on the world size.

a_t is the level of the FIRST timestep the loop evaluates (ddim_timesteps[k - 1]): the UNet is asked for the noise of
x_t at the level x_t was noised to.  The reference's x_info['x0'] branch (ddim.py:213-219) noises to timesteps[k] and
evaluates the first step at timesteps[k - 1]; that branch keeps its convention (DDIMSampler._start_latent).

What the kernel is handed as fp32 numbers -- scale_factor, sqrt(a_t), sqrt(1 - a_t) -- is rounded to fp32 here too,
before the fp64 arithmetic: 'mode' x0 is then ONE fp32 rounding of an exact product on both sides.
"""
import numpy as np

from . import noise

POSTERIORS = ('sample', 'mode')
MUTANTS = ('streams_swapped', 'stream0', 'no_clamp', 'logvar_as_std', 'level_of_k', 'unscaled')


def check_strength(strength):
    """0 < strength <= 1 as a float; ValueError otherwise (NaN included)"""
    try:
        s = float(strength)
    except (TypeError, ValueError):
        raise ValueError(f"strength must be a number in (0, 1], got {strength!r}") from None
    if not (0.0 < s <= 1.0):
        raise ValueError(f"strength must be in (0, 1], got {strength!r}")
    return s


def start_steps(steps, strength):
    """k = min(steps, int(steps * strength)): the number of steps an img2img request runs, over ddim_timesteps[:k].
    ValueError unless 0 < strength <= 1 and k >= 1."""
    s = check_strength(strength)
    steps = int(steps)
    k = min(steps, int(steps * s))
    if k < 1:
        raise ValueError(f"strength {strength!r} leaves no step of {steps} to run (steps * strength < 1)")
    return k


def check_posterior(posterior):
    if posterior not in POSTERIORS:
        raise ValueError(f"posterior must be 'sample' or 'mode', got {posterior!r}")
    return posterior


def level(alphas_cumprod, ddim_timesteps, k):
    """a_t of a start that runs ddim_timesteps[:k]: the level of the first timestep evaluated"""
    k = int(k)
    if not 1 <= k <= len(ddim_timesteps):
        raise ValueError(f"k must be in [1, {len(ddim_timesteps)}], got {k}")
    return float(np.asarray(alphas_cumprod, dtype=np.float64)[int(ddim_timesteps[k - 1])])


def kernel_scalars(scale_factor, a_t):
    """(scale_factor, sqrt(a_t), sqrt(1 - a_t)) as the fp32 numbers the kernel is handed"""
    a_t = float(a_t)
    if not 0.0 <= a_t <= 1.0:
        raise ValueError(f"a_t must be in [0, 1], got {a_t!r}")
    return np.float32(scale_factor), np.float32(np.sqrt(a_t)), np.float32(np.sqrt(1.0 - a_t))


def latent_start(moments, seed, sample_id, scale_factor, a_t, posterior='sample', wrong=None, a_next=None):
    """moments [2C, h, w] (mean channels first, then logvar) -> (x0, x_t), float32 [C, h, w] each.
    wrong: None, or one of MUTANTS -- a named way to get it wrong, for the tests to show that their tolerance tells the
    specification from its neighbours ('level_of_k' needs a_next, the level of ddim_timesteps[k])."""
    check_posterior(posterior)
    if wrong is not None and wrong not in MUTANTS:
        raise ValueError(f"unknown mutant {wrong!r}")
    m = np.asarray(moments, dtype=np.float64)
    if m.ndim != 3 or m.shape[0] % 2:
        raise ValueError(f"moments must be [2C, h, w], got {m.shape}")
    C = m.shape[0] // 2
    mean, logvar = m[:C], m[C:]
    n = mean.size
    sq, sp = noise.STREAM_Q, noise.STREAM_POSTERIOR
    if wrong == 'streams_swapped':
        sq, sp = sp, sq
    elif wrong == 'stream0':
        sq = sp = noise.STREAM_STEP
    z_q = noise.normal64(seed, sample_id, 0, n, stream=sq).reshape(mean.shape)
    z_p = noise.normal64(seed, sample_id, 0, n, stream=sp).reshape(mean.shape)
    if wrong == 'level_of_k':
        if a_next is None:
            raise ValueError("'level_of_k' needs a_next")
        a_t = a_next
    sf, sq_at, sq_1mat = (float(v) for v in kernel_scalars(1.0 if wrong == 'unscaled' else scale_factor, a_t))
    lv = logvar if wrong == 'no_clamp' else np.clip(logvar, -30.0, 20.0)
    with np.errstate(over='ignore'):
        std = lv if wrong == 'logvar_as_std' else np.exp(0.5 * lv)
    x0 = sf * mean if posterior == 'mode' else sf * (mean + std * z_p)
    x_t = sq_at * x0 + sq_1mat * z_q
    return x0.astype(np.float32), x_t.astype(np.float32)


def latent_start_batch(moments, keys, scale_factor, a_t, posterior='sample', **kw):
    """moments [Bm, 2C, h, w] with Bm in {1, B} (1: one picture shared by the B samples), keys [B, 2] rows
    (seed, sample_id) -> (x0, x_t), float32 [B, C, h, w] each"""
    m = np.asarray(moments)
    keys = np.asarray(keys, dtype=np.int64).reshape(-1, 2)
    B = keys.shape[0]
    if m.ndim != 4 or m.shape[0] not in (1, B):
        raise ValueError(f"moments must be [1 | {B}, 2C, h, w], got {m.shape}")
    outs = [latent_start(m[b if m.shape[0] > 1 else 0], int(keys[b, 0]), int(keys[b, 1]), scale_factor, a_t, posterior, **kw)
            for b in range(B)]
    return np.stack([o[0] for o in outs]), np.stack([o[1] for o in outs])
