"""TEST INFRASTRUCTURE: the request front door -- PromptFreePipeline.generate (lib/pipeline.py) and PromptFreeServer.submit /
_generate (lib/serving.py) -- on a machine without a GPU, with the net, the sampler and the device ops all stubbed.

  * `Net`: tests/stubs.py::StubNet with the VAE encoder of tests/test_img2img_cpu.py; ctx_encode, vae_encode_moments and
    vae_decode are cheap deterministic functions of their input and append one line to `LOG` per call;
  * the device ops the front door calls (ops.image_from_u8, latent_start, mask_grid_u8, composite_u8, canny_u8): the stand-ins
    of test_img2img_cpu.py, test_inpaint_cpu.py and test_canny_cpu.py, a nearest-neighbour resize and lib/inpaint.composite,
    each behind one log line;
  * `Sampler`: records what it was handed -- steps, shape, eta, every extra keyword and every key of x_info / c_info in sorted
    order: the Python type; dtype, shape and device of a tensor; a sha256 of the bytes of a tensor or an array; the repr of a
    number or a tuple.  A key that is absent has no line: `solver` for 'ddim', say;
  * `CASES`, `RANKED`, `REFUSALS` and the functions that run them through both doors: every case through `generate` at world
    size 1, through `submit` alone, and through `submit` next to a second request behind a held queue, under mixed_batches
    False and True.  Whatever a door raises is a line of the record like any other.

Everything is pinned in tests/golden/frontdoor_calls.txt (tests/test_frontdoor_cpu.py): a refusal line for line, the record of
a run by a sha256 over all its lines next to a readable digest of them (`pin`); `--show 'SECTION'` prints the full record of a
section as the code gives it now, so the record of a parent commit can be laid next to it.  The fixture is regenerated with

    python tests/frontdoor_standin.py --write

Regenerate it only for a change that is MEANT to change what a door hands on or refuses, and read the diff: it is the change.
"""
import hashlib
import os
import re
import sys
import threading

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, os.path.join(REPO, "prompt-free-diffusion_amd"))

import img2img_refs as I                                                    # noqa: E402
import test_canny_cpu as TC                                                 # noqa: E402
import test_control_cpu as TS                                               # noqa: E402
import test_image_ingest_cpu as TG                                          # noqa: E402
import test_img2img_cpu as TI                                               # noqa: E402
import test_inpaint_cpu as TP                                               # noqa: E402
from lib.hip import ops                                                     # noqa: E402

FIXTURE = os.path.join(REPO, "tests", "golden", "frontdoor_calls.txt")
LOG = []
DRAWS = []             # the x_T draws, apart from LOG: a draw on the host is no step in the order of the device calls
SEED = 1234            # the global generator at the start of every run


# ----------------------------------------------------------------------------------------------------------------------
# the record
# ----------------------------------------------------------------------------------------------------------------------
def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


def desc(v):
    """one value as the fixture shows it"""
    if torch.is_tensor(v):
        return f"Tensor {str(v.dtype).replace('torch.', '')}{list(v.shape)} {v.device} {_sha(v.detach().cpu().contiguous().numpy())}"
    if isinstance(v, np.ndarray):
        return f"ndarray {v.dtype}{list(v.shape)} {_sha(v)}"
    if isinstance(v, list):
        return "list[" + "; ".join(desc(x) for x in v) + "]"
    return f"{type(v).__name__} {v!r}"


def log(name, *vals, **kw):
    LOG.append(" ".join([name] + [desc(v) for v in vals] + [f"{k}={v!r}" for k, v in kw.items()]))


# ----------------------------------------------------------------------------------------------------------------------
# the net, the ops, the sampler
# ----------------------------------------------------------------------------------------------------------------------
class Net(type(TI._net())):
    def __init__(self):
        from lib.model_zoo.controlnet import ControlNet
        self.ctl = ControlNet.__new__(ControlNet)        # preprocess reads no weights

    def ctx_encode(self, image, which):
        log("net.ctx_encode", image, which=which)
        assert which == 'image' and image.shape[0] == 1
        return image.double().mean().float().reshape(1, 1, 1).expand(1, 148, 768).clone()

    def vae_encode_moments(self, x, which):
        log("net.vae_encode_moments", x, which=which)
        if x.shape[-1] == 3 and x.shape[1] != 3:         # the f16 NHWC picture of a uint8 init
            x = x.permute(0, 3, 1, 2)
        return super().vae_encode_moments(x, which)

    def vae_decode(self, z, which, out_uint8=False):
        log("net.vae_decode", z, which=which, out_uint8=out_uint8)
        return super().vae_decode(z, which, out_uint8=out_uint8)


def image_from_u8(img, size=None, dtype=torch.float16, layout='nchw'):
    """ops.image_from_u8 with a nearest-neighbour resize: the layouts and dtypes of the real one"""
    log("ops.image_from_u8", img, size=None if size is None else tuple(int(s) for s in size), dtype=dtype, layout=layout)
    x = img[None] if img.dim() == 3 else img
    if size is not None:
        ys = (torch.arange(int(size[0])) * x.shape[1]) // int(size[0])
        xs = (torch.arange(int(size[1])) * x.shape[2]) // int(size[1])
        x = x[:, ys][:, :, xs]
    if layout == 'u8':
        return x.contiguous()
    if layout == 'nhwc':
        return (x.float() / 255).to(torch.float16).contiguous()
    return (x.float() / 255).permute(0, 3, 1, 2).to(dtype).contiguous()


def latent_start(moments_nhwc, key, scale_factor, a_t, B=None, posterior='sample', want_x0=False):
    log("ops.latent_start", moments_nhwc, key, float(scale_factor), float(a_t), posterior=posterior, want_x0=want_x0)
    return TI._standin_latent_start(moments_nhwc, key, scale_factor, a_t, B, posterior, want_x0)


def mask_grid_u8(mask, gh, gw, dtype=torch.float32):
    log("ops.mask_grid_u8", mask, gh=int(gh), gw=int(gw), dtype=dtype)
    return TP._standin_mask_grid_u8(mask, gh, gw, dtype)


def composite_u8(decoded, init, sel):
    from lib import inpaint
    log("ops.composite_u8", decoded, init, sel)
    return torch.from_numpy(inpaint.composite(decoded.numpy(), init.numpy(), sel.numpy()))


def canny_u8(img, low=100, high=200, out='u8', dtype=torch.float16, return_states=False):
    log("ops.canny_u8", img, low=low, high=high, out=out, dtype=dtype)
    return TC.canny_u8_standin(img, low, high, out, dtype, return_states)


def install(monkeypatch):
    """the op stand-ins, and a logging wrapper around the x_T draw of each door (the `shard_xT` of lib.pipeline and the one
    lib.serving names): a request that starts from a picture shows no `host.shard_xT` line"""
    from lib import pipeline, serving
    del LOG[:], DRAWS[:]
    for name in ("image_from_u8", "latent_start", "mask_grid_u8", "composite_u8", "canny_u8"):
        monkeypatch.setattr(ops, name, globals()[name])
    draw = pipeline.shard_xT

    def shard_xT(n, height, width, seed, rank, world_size):
        DRAWS.append(f"host.shard_xT n={n!r} height={height!r} width={width!r} seed={seed!r}")
        return draw(n, height, width, seed, rank, world_size)
    monkeypatch.setattr(pipeline, "shard_xT", shard_xT)
    monkeypatch.setattr(serving, "shard_xT", shard_xT)


class Sampler:
    """records the call; the result is a cheap per-sample function of the start and the context"""

    def enable_graph(self, on=True):
        pass

    def sample(self, steps, shape, x_info, c_info, eta=0., verbose=True, **how):
        LOG.append(f"sampler.sample steps={desc(steps)} shape={desc(shape)} eta={desc(eta)} verbose={verbose!r}")
        LOG.extend(f"  how[{k!r}] = {desc(how[k])}" for k in sorted(how))
        LOG.extend(f"  x_info[{k!r}] = {desc(x_info[k])}" for k in sorted(x_info))
        LOG.extend(f"  c_info[{k!r}] = {desc(c_info[k])}" for k in sorted(c_info))
        x = x_info['xt']
        assert list(x.shape) == list(shape)
        return x.float() * 0.5 + c_info['conditioning'][:, :1, :1].reshape(-1, 1, 1, 1).float(), {}


# ----------------------------------------------------------------------------------------------------------------------
# the named requests
# ----------------------------------------------------------------------------------------------------------------------
def _f32(seed, h=64, w=64):
    return torch.from_numpy(I.picture_f32(h, w, seed))


IMG, IMG_U8 = _f32(1), I.picture_u8(48, 40, 2)
A, B, C, B_U8 = _f32(3), _f32(4, 32, 48), _f32(5), I.picture_u8(40, 56, 6)
CTL, CTL_U8 = _f32(7), I.picture_u8(50, 70, 8)
INIT, INIT_U8 = _f32(9), I.picture_u8(100, 80, 10)
MASK_U8, MASK_F = TP._mask_u8(), (torch.arange(64, dtype=torch.float32).reshape(8, 8) / 63)
UNCOND, UNCOND2 = torch.full((1, 148, 768), 0.5), torch.full((1, 296, 768), 0.25)
MAP = np.zeros((10, 6), dtype=np.uint8)
MAP[:, 3:] = 1
MAP2 = np.ones((5, 9), dtype=np.uint8)
MAP2[:, :4] = 0
I2I = dict(steps=8, strength=0.75)


def _case(cid, kw=None, gen=None, other=None):
    """kw: the request, through both doors; gen: what `generate` alone is given on top; other: how the second request of the
    coalesced run differs from the first (besides its seed and n = 1)"""
    return dict(id=cid, kw=dict(kw or {}), gen=dict(gen or {}), other=dict(other or {}))


CASES = [
    _case("plain"),
    _case("scale_per_sample", gen=dict(scale=[1.5, 3.0]), other=dict(scale=3.0)),
    _case("scale_per_sample_submitted", dict(scale=[1.5, 3.0])),
    _case("scale_1", dict(scale=1.0)),
    _case("eta", dict(eta=0.5)),
    _case("eta_device_noise", dict(eta=0.5, device_noise=True)),
    _case("dpmpp_2m", dict(solver='dpmpp_2m')),
    _case("dpmpp_1", dict(solver='dpmpp_1')),
    _case("reference_u8", dict(image=IMG_U8)),
    _case("control_u8", dict(control=CTL_U8)),
    _case("control_float", dict(control=CTL), other=dict(control=CTL_U8)),
    _case("canny_u8", dict(control=CTL_U8, control_preprocess='canny')),
    _case("canny_float", dict(control=CTL, control_preprocess='canny', control_thresholds=(50, 120))),
    _case("uncond", dict(uncond=UNCOND)),
    _case("init_u8", dict(I2I, init=INIT_U8)),
    _case("init_float", dict(I2I, init=INIT), other=dict(init=INIT_U8, strength=0.8)),
    _case("init_mode", dict(I2I, init=INIT), gen=dict(init_posterior='mode')),
    _case("mask_u8", dict(I2I, init=INIT_U8, mask=MASK_U8), other=dict(mask=TP._mask_u8(1), init=INIT)),
    _case("mask_float", dict(I2I, init=INIT, mask=MASK_F)),
    _case("composite", dict(I2I, init=INIT_U8, mask=MASK_U8, composite=True, as_uint8=True)),
    _case("image_weights", dict(image=[A, B_U8], image_weights=[0.7, 0.3])),
    _case("image_weights_zero_weight", dict(image=[A, B, C], image_weights=[0.5, 0.0, 0.25])),
    _case("image_weights_one_left", dict(image=[A, B], image_weights=[1.0, 0.0])),
    _case("regions", dict(image=[A, B, C], regions=MAP, region_weights=[[1.0, 0.0, 0.0], [0.5, 0.0, 1.0]])),
    _case("regions_one_region", dict(image=[A, B], regions=MAP[:, :3], region_weights=[[0.7, 0.3]])),
    _case("regions_one_left", dict(image=[A, B], regions=MAP, region_weights=[[0.0, 1.0], [0.0, 2.0]])),
    _case("control_scale", dict(control=CTL, control_scale=0.5), other=dict(control_scale=0.25)),
    _case("control_scale_per_sample", dict(control=CTL, control_scale=[1.0, 0.4]), other=dict(control_scale=[0.3])),
    _case("control_layer_scales", dict(control=CTL, control_layer_scales='soft')),
    _case("control_window", dict(control=CTL, control_window=(0, 0.5))),
    _case("control_cond_only", dict(control=CTL, control_cond_only=True)),
    _case("control_scale_0_is_off", dict(control=CTL, control_scale=0), other=dict(control=None, control_scale=1.0)),
    _case("control_empty_window_is_off", dict(control=CTL_U8, control_window=(0.5, 0.5))),
    _case("guidance_rescale", dict(guidance_rescale=0.7), other=dict(guidance_rescale=0.25)),
    _case("guidance_rescale_per_sample", dict(guidance_rescale=[0.0, 0.25]), other=dict(guidance_rescale=[0.5])),
    _case("guidance_rescale_scale_1", dict(guidance_rescale=0.7, scale=1.0)),
    # the pairs that interact in the code
    _case("image_weights_uncond_shorter", dict(image=[A, B], image_weights=[0.7, 0.3], uncond=UNCOND)),
    _case("image_weights_uncond_equal", dict(image=[A, B], image_weights=[0.7, 0.3]), gen=dict(uncond=UNCOND2)),
    _case("image_weights_uncond_equal_submitted", dict(image=[A, B], image_weights=[0.7, 0.3], uncond=UNCOND2)),
    _case("image_weights_uncond_longer", dict(image=[A, B], image_weights=[0.7, 0.3], uncond=torch.zeros(1, 300, 768))),
    _case("regions_uncond", dict(image=[A, B], regions=MAP, region_weights=[[1, 0], [0, 1]]), gen=dict(uncond=UNCOND)),
    _case("regions_uncond_submitted", dict(image=[A, B], regions=MAP, region_weights=[[1, 0], [0, 1]], uncond=UNCOND)),
    _case("init_control_window", dict(steps=4, init=INIT, strength=0.5, control=CTL, control_window=(0, 0.75))),
    _case("init_control_window_ends_before_the_run", dict(steps=4, init=INIT, strength=0.5, control=CTL, control_window=(0, 0.5))),
    _case("mask_device_noise", dict(I2I, init=INIT, mask=MASK_U8, eta=0.5, device_noise=True)),
    _case("control_cond_only_scale_1", dict(control=CTL, control_cond_only=True, scale=1.0)),
    _case("guidance_rescale_per_sample_scale", dict(guidance_rescale=[0.0, 0.25], scale=7.5), gen=dict(scale=[1.0, 7.5]),
          other=dict(scale=3.0, guidance_rescale=0.2)),
    _case("image_weights_different_numbers_of_references", dict(image=[A, B], image_weights=[0.7, 0.3]),
          other=dict(image=[A, B_U8, C], image_weights=[0.5, 0.3, 0.2])),
    _case("image_weights_one_with_uncond", dict(image=[A, B, C], image_weights=[0.5, 0.3, 0.2]),
          other=dict(image=[A, B], image_weights=[0.7, 0.3], uncond=UNCOND)),
    _case("regions_maps_of_different_sizes", dict(image=[A, B], regions=MAP, region_weights=[[1, 0], [0, 1]]),
          other=dict(image=[B, C], regions=MAP2, region_weights=[[1, 1], [0.2, 1]])),
]
CASE_IDS = [c['id'] for c in CASES]

# every per-sample argument, and the seeded starts, at rank 0 and rank 1 of world size 2 (n_global = 4)
PER_SAMPLE_CTL = torch.cat([_f32(11), _f32(12)])
PER_SAMPLE_REF = torch.cat([_f32(13), _f32(14)])
RANKED = [
    _case("scale", dict(scale=[1.5, 2.0, 3.0, 7.25])),
    _case("control_scale", dict(control=CTL, control_scale=[1.0, 0.4, 0.0, 0.7], control_layer_scales='soft')),
    _case("control_scale_0_on_rank_1", dict(control=CTL, control_scale=[1.0, 0.4, 0.0, 0.0])),
    _case("guidance_rescale", dict(guidance_rescale=[0.7, 0.25, 0.0, 1.0])),
    _case("guidance_rescale_0_on_rank_1", dict(guidance_rescale=[0.7, 0.25, 0.0, 0.0])),
    _case("hint_per_local_sample", dict(control=PER_SAMPLE_CTL)),
    _case("reference_per_local_sample", dict(image=PER_SAMPLE_REF)),
    _case("init", dict(I2I, init=INIT_U8)),
    _case("mask", dict(I2I, init=INIT, mask=MASK_U8, eta=0.5, device_noise=True)),
    _case("mask_per_local_sample", dict(I2I, init=INIT, mask=torch.stack([MASK_F, 1 - MASK_F]))),
    _case("image_weights", dict(image=[A, B], image_weights=[0.7, 0.3], uncond=UNCOND)),
    _case("regions", dict(image=[A, B], regions=MAP, region_weights=[[1, 0], [0, 1]], uncond=UNCOND)),
]
RANKED_IDS = [c['id'] for c in RANKED]


def _refusals():
    """the bad-argument sets of the feature tests (BAD and its kin), as keyword sets over a plain two-sample request"""
    out = []

    def add(group, sets, **base):
        for i, kw in enumerate(sets):
            out.append((f"{group}[{i}]", dict(base, **kw)))

    u8, fl = np.zeros((40, 50, 3), np.uint8), CTL
    add("control_strength", TS.BAD, control=CTL)
    add("control_strength_without_control", [dict(control_scale=0.5), dict(control_layer_scales='soft'), dict(control_window=(0, 0.5)),
                                             dict(control_cond_only=True), dict(control_scale=0.0)])
    add("control_scale_per_sample", [dict(control_scale=[1.0, 0.4, 0.0, -0.7]), dict(control_scale=[1.0])], control=CTL)
    add("preprocess_u8", TC.BAD_PREPROCESS, control=u8)
    add("preprocess_float", TC.BAD_PREPROCESS, control=fl)
    add("preprocess", [dict(control_preprocess='canny'), dict(control=np.zeros((2000, 64, 3), np.uint8), control_preprocess='canny')])
    bad_pics = list(TG._bad_pictures().values())
    add("reference_picture", [dict(image=p) for p in bad_pics] +
        [dict(image=torch.zeros(31, 64, 3, dtype=torch.uint8)), dict(image=np.zeros((64, 16, 3), np.uint8)),
         dict(image=torch.zeros(1, 3, 64, 64, dtype=torch.int32)), dict(image=torch.zeros(64, 20, 3, dtype=torch.uint8))])
    add("control_picture", [dict(control=p) for p in bad_pics] +
        [dict(control=torch.zeros(2000, 64, 3, dtype=torch.uint8)), dict(control=np.zeros((64, 1100, 3), np.uint8)),
         dict(control=torch.rand(3, 3, 64, 64, generator=torch.Generator().manual_seed(1)))], image=IMG_U8)
    add("scale", [dict(scale=[1.5, 2.0, 3.0])])
    add("solver", [dict(solver='euler'), dict(solver='dpmpp_2m', eta=0.5), dict(solver='dpmpp_2m', device_noise=True),
                   dict(solver='dpmpp_1', eta=0.5, device_noise=True)])
    add("guidance_rescale", [dict(guidance_rescale=v) for v in (-0.5, 1.5, float('nan'), [0.5, 0.5, 0.5], [0.5], 'x', 1.01)])
    add("img2img", [dict(strength=0), dict(strength=1.01), dict(strength=1.5), dict(strength=0.01), dict(init=_f32(9, 32, 64)),
                    dict(init=_f32(9, 64, 32)), dict(init=_f32(9)[0]), dict(init=torch.zeros(1, 3, 64, 64, dtype=torch.int32)),
                    dict(init=np.zeros((64, 64, 4), dtype=np.uint8)), dict(init=np.zeros((64, 64), dtype=np.uint8)),
                    dict(init=np.zeros((2000, 64, 3), dtype=np.uint8)), dict(init=np.zeros((64 * 17, 64, 3), dtype=np.uint8))],
        **dict(I2I, init=INIT))
    add("mask", [dict(init=None), dict(mask=np.zeros((96, 72), dtype=np.float32)), dict(mask=np.zeros((96, 72), dtype=np.int32)),
                 dict(mask=np.zeros((96, 72, 3), dtype=np.uint8)), dict(mask=np.zeros((96, 72, 2), dtype=np.uint8)),
                 dict(mask=np.zeros((0, 72), dtype=np.uint8)), dict(mask=np.zeros((64 * 17, 64), dtype=np.uint8)),
                 dict(mask=torch.zeros(16, 16)), dict(mask=torch.zeros(4, 4)), dict(mask=torch.zeros(3, 8, 8)),
                 dict(mask=torch.zeros(1, 2, 8, 8)), dict(mask=torch.zeros(4, 8, 8)), dict(mask=torch.zeros(3, 1, 8, 8)),
                 dict(mask=torch.zeros(8, 8, dtype=torch.int32)), dict(eta=0.5), dict(composite=True, as_uint8=False),
                 dict(composite=True, init=INIT), dict(composite=True, mask=torch.zeros(8, 8)), dict(composite=True, mask=None)],
        **dict(I2I, init=INIT_U8, mask=MASK_U8, as_uint8=True))
    add("image_weights", [dict(image=[A, B], image_weights=None), dict(image=A, image_weights=[1.0]), dict(image=[A, B], image_weights=[1.0]),
                          dict(image=[A, B], image_weights=[1.0, -1.0]), dict(image=[A, B], image_weights=[0.0, 0.0]),
                          dict(image=[A, B], image_weights=[1.0, float('nan')]), dict(image=[A] * 9, image_weights=[1.0] * 9),
                          dict(image=[A, torch.zeros(2, 3, 64, 64)], image_weights=[1.0, 1.0]),
                          dict(image=[A, np.zeros((8, 8, 3), dtype=np.uint8)], image_weights=[1.0, 1.0]),
                          dict(image=[A, _f32(3, 16, 16)], image_weights=[1.0, 1.0])])
    add("regions", [dict(regions=MAP), dict(regions=MAP, region_weights=[[1, 0], [0, 1]], image_weights=[1, 1]),
                    dict(regions=MAP2, region_weights=[[1, 0]]), dict(regions=MAP, region_weights=[[1, 0], [0, 0]]),
                    dict(regions=MAP, region_weights=[[1, 0, 0], [0, 1, 0]]), dict(regions=MAP.astype(np.int32), region_weights=[[1, 0], [0, 1]]),
                    dict(regions=MAP[0], region_weights=[[1, 0], [0, 1]])], image=[A, B])
    return out


REFUSALS = _refusals()
# what submit alone refuses, one defect each (which of two defects is reported is pinned only where the feature tests have the pair)
SUBMIT_ONLY = [dict(height=96), dict(width=32), dict(n=0), dict(n=9), dict(steps=0), dict(closed=True)]
REFUSAL_IDS = [r[0] for r in REFUSALS]


# ----------------------------------------------------------------------------------------------------------------------
# running them
# ----------------------------------------------------------------------------------------------------------------------
def _returns(out):
    if isinstance(out, tuple):
        return "returns (" + ", ".join(desc(o) for o in out) + ")"
    return "returns " + desc(out)


def _caught(e):
    return f"raises {type(e).__name__}: {e}"


def run_generate(kw, rank=0, world=1, n=2):
    """the request through PromptFreePipeline.generate -> fixture lines"""
    from lib.pipeline import PromptFreePipeline
    del LOG[:], DRAWS[:]
    kw = dict(kw)
    kw.setdefault('steps', 4)
    image = kw.pop('image', IMG)
    pipe = PromptFreePipeline(Net(), rank=rank, world_size=world, sampler=Sampler())
    torch.manual_seed(SEED)
    try:
        tail = _returns(pipe.generate(image, n, 64, 64, **kw))
    except Exception as e:      # noqa: BLE001 -- what a door raises is part of its record
        tail = _caught(e)
    return list(LOG) + list(DRAWS) + [tail, "generator %.5f" % float(torch.randn(1))]


def run_submit(requests, mixed=False, held=True):
    """the requests through one PromptFreeServer, queued behind a held gate -> fixture lines: the call log, what every future
    gave, every request's key() and shareable(), the composition of the batches run"""
    from lib.serving import PromptFreeServer
    del LOG[:], DRAWS[:]
    srv = PromptFreeServer(Net(), use_graph=False, max_batch=8, mixed_batches=mixed)
    srv.pipe.sampler = Sampler()
    ran, inner = [], srv._generate

    def spy(batch):
        ran.append(list(batch))
        LOG.append(f"_generate of {len(batch)} request(s)")
        return inner(batch)
    srv._generate = spy
    tails, futs = [], []
    torch.manual_seed(SEED)
    try:
        gate = threading.Event()
        if held:
            srv.call(lambda net: gate.wait(30))
        for kw in requests:
            kw = dict(kw)
            kw.setdefault('steps', 4)
            image, n = kw.pop('image', IMG), kw.pop('n', 2)
            try:
                futs.append(srv.submit(image, n, 64, 64, **kw))
            except Exception as e:      # noqa: BLE001
                futs.append(e)
        gate.set()
        for i, f in enumerate(futs):
            if isinstance(f, Exception):
                tails.append(f"request {i}: submit {_caught(f)}")
                continue
            try:
                tails.append(f"request {i}: {_returns(f.result(60))}")
            except Exception as e:      # noqa: BLE001
                tails.append(f"request {i}: future {_caught(e)}")
    finally:
        srv.close()
    seen = []
    for batch in ran:
        for r in batch:
            if not any(r is s for s in seen):
                seen.append(r)
    lines = list(LOG) + list(DRAWS) + tails
    lines += [f"request seed={r.seed}: key={r.key()!r} shareable={r.shareable()!r}" for r in seen]
    lines.append(f"batches run: {[[(r.seed, r.n) for r in b] for b in ran]} srv.batches={srv.batches}")
    return lines


def run_case(case, monkeypatch):
    """{way: lines} of one named request"""
    install(monkeypatch)
    first = dict(case['kw'], seed=20)
    second = dict(first, seed=21, n=1)
    if isinstance(second.get('control_scale'), list):
        second['control_scale'] = second['control_scale'][:1]
    if isinstance(second.get('guidance_rescale'), list):
        second['guidance_rescale'] = second['guidance_rescale'][:1]
    if isinstance(second.get('scale'), list):
        second['scale'] = second['scale'][:1]
    second.update(case['other'])
    return {"generate": run_generate(dict(first, **case['gen'])),
            "submit": run_submit([first], held=False),
            "coalesced": run_submit([first, second]),
            "coalesced mixed_batches": run_submit([first, second], mixed=True)}


def run_ranked(case, monkeypatch):
    install(monkeypatch)
    return {f"rank {r} of 2": run_generate(dict(case['kw'], seed=20, decode=False), rank=r, world=2, n=4) for r in range(2)}


def run_refusal(kw, monkeypatch):
    """one bad-argument set through both doors -> two lines: the exception, whether the net and the ops were left alone, and
    from submit that nothing was queued (the raise reaches this, the caller's, thread by construction)"""
    from lib.pipeline import PromptFreePipeline
    from lib.serving import PromptFreeServer
    install(monkeypatch)
    kw = dict(kw)
    kw.setdefault('steps', 4)
    image = kw.pop('image', IMG)
    lines = []
    try:
        PromptFreePipeline(Net(), sampler=Sampler()).generate(image, 2, 64, 64, **kw)
        lines.append("generate: accepted")
    except Exception as e:      # noqa: BLE001
        lines.append(f"generate: {_caught(e)} | calls before the raise: {len(LOG)}")
    del LOG[:], DRAWS[:]
    srv = PromptFreeServer(Net(), use_graph=False, max_batch=8)
    srv.pipe.sampler = Sampler()
    try:
        gate, entered = threading.Event(), threading.Event()
        srv.call(lambda net: (entered.set(), gate.wait(30)))
        entered.wait(30)                    # the worker has taken the gate and waits in it: the queue is empty
        here = threading.current_thread()
        try:
            srv.submit(image, 2, 64, 64, **kw)
            lines.append(f"submit: accepted | queued: {srv._q.qsize()}")
        except Exception as e:      # noqa: BLE001
            lines.append(f"submit: {_caught(e)} | calls before the raise: {len(LOG)} | queued: {srv._q.qsize()} | "
                         f"on the caller's thread: {threading.current_thread() is here}")
        gate.set()
    finally:
        srv.close()
    return lines


# ----------------------------------------------------------------------------------------------------------------------
# the fixture
# ----------------------------------------------------------------------------------------------------------------------
def sections(monkeypatch_context, only=None):
    """every (section name, full record) in the fixture's order; only: the one section of that name"""
    for case in CASES:
        if only is None or only.startswith(case['id'] + " / "):
            with monkeypatch_context() as mp:
                for way, lines in run_case(case, mp).items():
                    yield f"{case['id']} / {way}", lines
    for case in RANKED:
        if only is None or only.startswith(f"ranked {case['id']} / "):
            with monkeypatch_context() as mp:
                for way, lines in run_ranked(case, mp).items():
                    yield f"ranked {case['id']} / {way}", lines
    for rid, kw in REFUSALS:
        if only is None or only == f"refusal {rid}":
            with monkeypatch_context() as mp:
                yield f"refusal {rid}", run_refusal(kw, mp)
    for i, kw in enumerate(SUBMIT_ONLY):
        if only is None or only == f"refusal submit_only[{i}]":
            with monkeypatch_context() as mp:
                yield f"refusal submit_only[{i}]", run_submit_only(kw, mp)


def _short(ln):
    """one line of the sampler record, shortened: "  c_info['key_bias'] = Tensor float32[2, 296] cpu 0123456789abcdef" ->
    "c.key_bias=float32[2,296]:01234567" (the device is named where it is not the CPU)"""
    k, v = ln.strip().split(" = ", 1)
    k = k.replace("_info['", ".").replace("how['", "how.").replace("']", "")
    v = re.sub(r"\b(Tensor|ndarray) ", "", v).replace(", ", ",").replace(" cpu ", ":")
    return k + "=" + re.sub(r"([: ])([0-9a-f]{8})[0-9a-f]{8}\b", r"\1\2", v)


def pin(lines):
    """the full record of a run -> what the fixture holds of it: a sha256 over every line; the calls in order; the sampler
    record, every key with type, dtype, shape and the head of its sha256 (a changed value shows as a changed entry); what
    came back, the keys and the batches"""
    calls = [ln.split(" ", 1)[0] for ln in lines if ln.startswith(("net.", "ops.", "host.", "sampler.", "_generate"))]
    head = [ln[len("sampler.sample "):] for ln in lines if ln.startswith("sampler.sample ")]
    back = [re.sub(r"( cpu) [0-9a-f]{16}\b", r"\1", ln) for ln in lines
            if not ln.startswith(("net.", "ops.", "host.", "sampler.", "_generate", "  ", "generator"))]
    return ["sha256 " + hashlib.sha256("\n".join(lines).encode()).hexdigest()[:32] + " | calls: " + " ".join(calls),
            "handed: " + "; ".join(head) + " | " + " ".join(_short(ln) for ln in lines if ln.startswith("  ")),
            "back: " + " | ".join(back)]


def run_submit_only(kw, monkeypatch):
    """one of SUBMIT_ONLY -> the one line of what submit raises"""
    from lib.serving import PromptFreeServer
    install(monkeypatch)
    kw = dict(dict(steps=4, height=64, width=64, n=2, image=IMG), **kw)
    srv = PromptFreeServer(Net(), use_graph=False, max_batch=8)
    try:
        if kw.pop('closed', False):
            srv.close()
        try:
            srv.submit(kw.pop('image'), kw.pop('n'), kw.pop('height'), kw.pop('width'), **kw)
            return [f"submit: accepted | queued: {srv._q.qsize()}"]
        except Exception as e:      # noqa: BLE001
            return [f"submit: {_caught(e)} | calls before the raise: {len(LOG)}"]
    finally:
        srv.close()


def pin_refusal(lines):
    """the two lines of a refusal, the words of submit's exception left out where they are generate's"""
    gen, sub = lines
    what = gen[len("generate: "):].split(" | ")[0]
    return [gen, sub.replace("submit: " + what + " |", "submit: the same |") if what.startswith("raises") else sub]


def show(name):
    """the full record of one section, as the runs give it now"""
    import pytest
    for got, lines in sections(pytest.MonkeyPatch.context, only=name):
        if got == name:
            return lines
    raise KeyError(name)


def read_fixture():
    """{section name: [lines]}"""
    out, cur = {}, None
    for line in open(FIXTURE).read().splitlines():
        if line.startswith("== "):
            cur = out.setdefault(line[3:], [])
        elif line and not line.startswith("#"):
            cur.append(line)
    return out


def write_fixture():
    import pytest
    text = ["# both request doors over tests/frontdoor_standin.py.  Per run of a named request: a sha256 over its full record (every call",
            "# with its arguments, everything the sampler was handed, what came back, the server's keys and batches) and, readable, the",
            "# calls, the sampler record with the head of every value's sha256, what came back.  Per bad-argument set: what each door raises.",
            "# The full record of a section: `python tests/frontdoor_standin.py --show 'NAME'`.",
            "# Written by `python tests/frontdoor_standin.py --write`; pinned by tests/test_frontdoor_cpu.py."]
    n = 0
    for name, lines in sections(pytest.MonkeyPatch.context):
        text += ["== " + name] + (pin(lines) if " / " in name else pin_refusal(lines) if len(lines) == 2 else lines)
        n += 1
    with open(FIXTURE, "w") as f:
        f.write("\n".join(text) + "\n")
    print(f"{FIXTURE}: {n} sections, {len(text)} lines, {os.path.getsize(FIXTURE)} bytes")


if __name__ == "__main__":
    if sys.argv[1:] == ["--write"]:
        write_fixture()
    elif len(sys.argv) == 3 and sys.argv[1] == "--show":
        print("\n".join(show(sys.argv[2])))
    else:
        sys.exit(__doc__)
