"""Request front-end of the hot path: reference image -> SeeCoder context -> DDIM/CFG loop ->
VAE decode, for one rank's shard of a (possibly multi-GPU) batch.

Restates the arithmetic-free glue of the reference's `prompt_free_diffusion.action_inference`
(app.py:229-274): ctx = ctx_encode(image).repeat(n); uncond = zeros_like(ctx) (or a padded fixed
tensor for SeeCoder-Anime, app.py:236-241); x_T ~ N(0, 1) of shape [n, 4, H/8, W/8];
DDIMSampler.sample(steps, eta, CFG scale, optional control); vae_decode.  The Gradio UI itself
is out of scope.

Multi-GPU (new, the reference is single-device): samples are independent, so rank r of P takes
samples [r*n/P, (r+1)*n/P) of the global batch.  x_T is drawn ONCE for the global shape from a
CPU generator and sliced, so results do not depend on P.  The only collective is one RCCL
all-gather of the decoded images after the loop (`gather=True`).

Both request doors -- `PromptFreePipeline.generate` here, `PromptFreeServer.submit` / `_generate` in lib/serving.py -- go through
`check_request` (arguments -> `Request`, on the host) and `PromptFreePipeline.assemble` (slices of requests -> one sampler call):
generate hands over one slice, its rank's samples of one request; a server one slice per request of its batch.
"""
import os

import numpy as np
import torch

from . import image_io
from . import refmix
from . import regions as region_lib
from .hip import ops
from .hip.ops import serialised


def build_model(name='pfd_seecoder', device='cuda', fp16=True, randomize_zero_init=True, seed=0, verbose=False):
    """Construct a composite from the config bank with synthetic weights (no checkpoints exist in
    the build/bench environment): default initialisation, plus re-randomised zero-initialised
    tensors so that no branch of the network is multiplied by zero."""
    from .cfg_helper import model_cfg_bank
    from .model_zoo import get_model
    cfg = model_cfg_bank()(name)
    cfg.args.vae_cfg_list[0][1].pth = None  # checkpoint not available: synthetic weights
    torch.manual_seed(seed)
    if device != 'cpu' and torch.cuda.is_available():
        with torch.device(device):
            net = get_model()(cfg, verbose=verbose)
    else:
        net = get_model()(cfg, verbose=verbose)
    if randomize_zero_init:
        g = torch.Generator(device='cpu').manual_seed(seed + 1)
        with torch.no_grad():
            for p in net.parameters():
                if p.is_floating_point() and p.numel() > 0 and float(p.detach().abs().max()) == 0.0:
                    fan_in = max(1, p.numel() // p.shape[0]) if p.dim() > 1 else 1
                    std = fan_in ** -0.5 if p.dim() > 1 else 0.02
                    p.copy_((torch.randn(p.shape, generator=g) * std).to(p.device, p.dtype))
    if fp16:
        net.half()
    net.to(device)
    net.eval()
    return net


def shard_xT(n_global, height, width, seed, rank, world_size):
    """rank's slice of the x_T drawn once for the GLOBAL batch (CPU generator => independent of P)"""
    assert n_global % world_size == 0, "global batch must divide over the ranks"
    n = n_global // world_size
    g = torch.Generator(device='cpu').manual_seed(seed)
    return torch.randn([n_global, 4, height // 8, width // 8], generator=g)[rank * n:(rank + 1) * n]


def shard_noise_keys(n_global, seed, rank, world_size):
    """rank's rows of the seeded-noise keys of the GLOBAL batch: sample j gets (seed, j) whatever P is (lib/noise.py),
    int64 [n_local, 2] on the CPU"""
    assert n_global % world_size == 0, "global batch must divide over the ranks"
    from .noise import sample_keys
    n = n_global // world_size
    return torch.from_numpy(sample_keys(seed, rank * n, n))


def shard_scales(scales, rank, world_size):
    """rank's entries of the per-sample guidance scales of the GLOBAL batch (the contiguous split of shard_xT and
    shard_noise_keys: sample j keeps its scale whatever P is), fp32 [n_local] on the CPU"""
    v = torch.as_tensor(scales).detach().to(device='cpu', dtype=torch.float32).reshape(-1)
    n_global = v.shape[0]
    if n_global % world_size:
        raise ValueError(f"{n_global} guidance scales do not divide over {world_size} ranks")
    n = n_global // world_size
    return v[rank * n:(rank + 1) * n].clone()


def shard_rescale(guidance_rescale, n_global, rank, world_size):
    """generate's guidance_rescale for this rank: checked for the GLOBAL batch (one number or n_global numbers in [0, 1],
    lib/guidance.check_phi), cut like shard_scales -- sample j keeps its phi whatever P is.  -> None when nothing of it is
    left on this rank's samples (all zero: the plain request), else float32 [n_local] on the CPU"""
    from . import guidance as guidance_lib
    if torch.is_tensor(guidance_rescale):
        guidance_rescale = guidance_rescale.detach().cpu().numpy()
    v = guidance_lib.check_phi(guidance_rescale, n_global)
    if n_global % world_size:
        raise ValueError(f"{n_global} guidance-rescale factors do not divide over {world_size} ranks")
    n = n_global // world_size
    local = guidance_lib.normalise(v[rank * n:(rank + 1) * n], n)
    return None if local is None else torch.from_numpy(local)


def force_collective():
    """PFD_FORCE_COLLECTIVE=1 with an initialised process group: the collectives run even at world size 1 -- the
    one-GPU RCCL smoke (tests/test_hip_parity.py::test_rccl_one_rank_collectives, `bench.py --gpus 1` under that
    environment): communicator creation, all_gather and all_reduce on an MI355X without a multi-GPU node"""
    if os.environ.get("PFD_FORCE_COLLECTIVE") != "1":
        return False
    import torch.distributed as dist
    return dist.is_available() and dist.is_initialized()


def all_gather_batch(local, world_size):
    """the one collective of the path: concatenate every rank's shard in rank order"""
    if world_size == 1 and not force_collective():
        return local
    import torch.distributed as dist
    out = [torch.empty_like(local) for _ in range(world_size)]
    dist.all_gather(out, local.contiguous())  # RCCL over xGMI on the GPU box; gloo in the CPU tests
    return torch.cat(out, 0)


class _GraphedStage:
    """One stage (context encode, VAE decode) replayed as a hipGraph: ~920 / ~105 kernel launches per call at C2
    (426 / 75 of them the library's, tools/stage_launches.py) whose issue cost is otherwise paid by the host every
    batch (SeeCoder: 5.8 ms of device time in launches of 4-16 us).  One
    graph per (input shape, dtype, weights identity+version of the sub-model); static input buffer owned here;
    the same kernels as the eager path.  A capture that fails RAISES (like DDIMSampler._capture): a stage
    that silently fell back to eager launches would hide exactly the kind of capture-illegal call (host sync,
    pageable H2D copy) that corrupts a replay."""

    def __init__(self, net, method, which, module):
        # (net, method name) instead of a closure over the pipeline: no reference cycle, so the graphs and
        # their private memory pools are released by refcount when the pipeline is dropped, not at some
        # later cyclic-GC pass (possibly in the middle of another stream capture)
        self.net, self.method, self.which, self.module = net, method, which, module
        self.graphs = {}

    def fn(self, x):
        return getattr(self.net, self.method)(x, self.which)

    def _signature(self):
        from .hip.layers import generation
        return hash((generation(),) + tuple((p.data_ptr(), p._version) for p in self.module.parameters()))

    @serialised
    def __call__(self, x):
        if not x.is_cuda:
            raise RuntimeError("HIP path: stage input must be on the GPU (no CPU fallback)")
        key = (tuple(x.shape), x.dtype, self._signature())
        ent = self.graphs.get(key)
        if ent is None:
            from .hip import binding
            binding.prof_enable(False)
            sx = x.clone()
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):     # warm-up outside capture: packs weights, sizes the allocator
                self.fn(sx)
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                out = self.fn(sx)
            if len(self.graphs) >= 4:
                torch.cuda.synchronize()      # never drop a graph whose replay may still be in flight
                self.graphs.clear()
            ent = self.graphs[key] = (g, sx, out)
        g, sx, out = ent
        sx.copy_(x)
        g.replay()
        return out.clone()


class _Marks:
    """stage boundaries of one request: HIP events on a GPU model, wall clock otherwise (CPU tests)"""

    def __init__(self, on_gpu):
        self.on_gpu, self.t = on_gpu, []

    def mark(self):
        if self.on_gpu:
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            self.t.append(e)
        else:
            import time
            self.t.append(time.perf_counter())

    def ms(self, i, j):
        if self.on_gpu:
            return self.t[i].elapsed_time(self.t[j])
        return (self.t[j] - self.t[i]) * 1e3


def max_over_ranks(seconds, world_size, device='cpu'):
    """the timing reduction of bench.py: a step is as slow as its slowest rank"""
    if world_size == 1 and not force_collective():
        return float(seconds)
    import torch.distributed as dist
    t = torch.tensor([float(seconds)], device=device, dtype=torch.float64)
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return float(t.item())


def check_references(image, image_weights):
    """the reference argument(s) of a request, checked on the host.  -> None for a plain request (one picture, no weights),
    else (references kept, their weights): references of weight 0 are dropped here, before anything is encoded.  One
    reference left = the plain request of that picture (the caller passes no bias then).
    image: a list / tuple of references, each a uint8 HWC picture of any size (at least 32 a side) or a float [1, 3, h, w]
    tensor; image_weights: one finite number >= 0 per reference, not all 0; at most refmix.MAX_REFS references."""
    listed = isinstance(image, (list, tuple))
    if image_weights is None and not listed:
        return None
    if image_weights is None or not listed:
        raise ValueError("several references are given as image=[ref0, ref1, ...] together with image_weights=[w0, w1, ...]")
    if len(image) != len(image_weights):
        raise ValueError(f"{len(image)} reference pictures but {len(image_weights)} image_weights")
    keep, w = refmix.drop_zero_weights(image_weights)
    for i, ref in enumerate(image):
        if image_io.wants_ingest(ref):
            image_io.check_u8_picture(ref, f'image[{i}]', min_side=32)
        elif not (ref.dim() == 4 and ref.shape[0] == 1 and ref.shape[1] == 3 and ref.is_floating_point()):
            raise ValueError(f"image[{i}] must be a float tensor [1, 3, h, w] in [0, 1] or a uint8 picture [h, w, 3]")
    return [image[i] for i in keep], w


def check_regions(image, regions, region_weights, image_weights):
    """the regional arguments of a request, checked on the host before anything touches the device.
    -> (image, image_weights, None) where the request is no regional one after all -- none given; one region, which IS the
    image_weights request of its row; one reference left after the all-zero columns are dropped, which IS the plain request
    of that picture -- else (references kept, None, (uint8 map [Hm, Wm] as numpy, float64 weights [NR, R]))."""
    if regions is None and region_weights is None:
        return image, image_weights, None
    if regions is None or region_weights is None:
        raise ValueError("a regional request gives regions=<uint8 map [Hm, Wm]> together with region_weights=[[w00, w01, ...], ...]")
    if image_weights is not None:
        raise ValueError("region_weights and image_weights exclude each other: one region is the image_weights request")
    if not isinstance(image, (list, tuple)):
        raise ValueError("a regional request gives its references as image=[ref0, ref1, ...]")
    w = region_lib.check_region_weights(region_weights)
    if w.shape[1] != len(image):
        raise ValueError(f"{len(image)} reference pictures but rows of {w.shape[1]} region_weights")
    m = regions.detach().cpu().numpy() if torch.is_tensor(regions) else np.asarray(regions)
    if m.ndim != 2:
        raise ValueError(f"regions must be a uint8 map [Hm, Wm], got shape {m.shape}")
    region_lib.region_grid(m, 1, 1, nr=w.shape[0])          # dtype, shape and ids, on the host
    if w.shape[0] == 1:
        return image, [float(x) for x in w[0]], None
    keep, w = region_lib.drop_zero_columns(w)
    if len(keep) == 1:
        return image[keep[0]], None, None
    check_references([image[i] for i in keep], [1.0] * len(keep))      # the pictures themselves
    return [image[i] for i in keep], None, (np.ascontiguousarray(m), w)


def schedule_length(steps, num_timesteps):
    """how many timesteps the sampler's schedule has for a request of `steps` steps (len(ddim_timesteps))"""
    from .model_zoo.diffusion_utils import make_ddim_timesteps
    return int(len(make_ddim_timesteps("uniform", int(steps), int(num_timesteps), verbose=False)))


def check_control_strength(control, control_scale, control_layer_scales, control_window, control_cond_only, n, nb, total_k,
                           first=0, n_local=None):
    """the four strength arguments of a control request (lib/control.py), checked on the host before anything touches the
    device.  n: the samples control_scale speaks of (the global batch; a request's own on the server), of which this caller
    runs n_local from `first` on; nb: 2 with CFG, else 1; total_k: a callable -> (schedule length, steps the run evaluates),
    asked only when an argument is off its default.
    -> None: the plain request (with or without control); 'off': drop the control, the request is the uncontrolled one;
    else (table float32 [nb * n_local, 13], (lo, hi)) for c_info['control_scale'] / ['control_steps']."""
    from . import control as control_lib
    plain = (control_layer_scales is None and not control_cond_only and isinstance(control_scale, (int, float)) and
             not isinstance(control_scale, bool) and control_scale == 1 and isinstance(control_window, (tuple, list)) and
             tuple(control_window) == (0.0, 1.0))
    if plain:
        return None
    scales = control_lib.sample_scales(control_scale.detach().cpu().numpy() if torch.is_tensor(control_scale) else control_scale, n)
    n_local = int(n) if n_local is None else int(n_local)
    total, k = total_k()
    out = control_lib.normalise(scales[first:first + n_local], control_layer_scales, control_window, bool(control_cond_only),
                                n_local, total, k, nb)
    if control is None and out is not None:
        raise ValueError("control_scale / control_layer_scales / control_window / control_cond_only need a control picture")
    return out


class Request:
    """one checked request (`check_request`): what both doors -- PromptFreePipeline.generate and PromptFreeServer.submit --
    turn their arguments into before anything touches the device, and what `PromptFreePipeline.assemble` reads.  A field
    that was not given is None."""
    __slots__ = ("image", "n", "height", "width", "steps", "scale", "eta", "seed", "control", "uncond", "as_uint8",
                 "device_noise", "future", "mixed", "solver", "control_preprocess", "control_thresholds", "init", "strength",
                 "init_k", "mask", "composite", "weights", "regional", "ctl", "rescale")

    def __init__(self, **kw):
        for k in self.__slots__:
            setattr(self, k, kw.get(k))

    def key(self):
        """requests with equal keys can share one DDIM batch (mixed: any two scales other than 1 can)"""
        how = () if self.solver in (None, 'ddim') else (self.solver,)     # a batch runs ONE solver; the DDIM keys are unchanged
        if self.init is not None:     # img2img: a batch runs ONE number of steps; every other key is unchanged
            how = how + (('init', int(self.init_k)),)
        if self.mask is not None:     # inpainting: masked requests share batches with each other only; every other key is unchanged
            how = how + (('mask', bool(self.composite)),)
        if self.regional is not None:  # regional mixing: with regional requests of the same number of regions and references only
            how = how + (('regions',) + tuple(self.regional[1].shape),)
        elif self.weights is not None:  # several references: with each other only, whatever their number; every other key is unchanged
            how = how + ('refmix',)
        if self.ctl is not None:      # a scaled / windowed control: equal layers, steps and cond_only; the strengths may differ
            how = how + (('control',) + tuple(self.ctl[1:]),)
        if self.rescale is not None:  # guidance rescale: with each other only, whatever their phi; every other key is unchanged
            how = how + ('rescale',)
        if self.mixed:
            return (self.height, self.width, self.steps, float(self.scale) == 1.0, float(self.eta),
                    self.control is None, self.uncond is None, bool(self.as_uint8), bool(self.device_noise)) + how
        return (self.height, self.width, self.steps, float(self.scale), float(self.eta), self.control is None,
                self.uncond is None, bool(self.as_uint8), bool(self.device_noise)) + how

    def shareable(self):
        """eta > 0 WITHOUT device_noise draws its noise from the global RNG inside the loop (ddim.py:166): batched with
        other requests the draw -- and so the result for a given seed -- would depend on the company; such requests run
        alone, seeded.  With device_noise the noise of sample j is a function of (request seed, j, step, element)
        (lib/noise.py), whatever it is batched with: shareable at any eta.  ControlNet requests always run alone, unless
        the server mixes batches: then they share with each other (`control is None` is part of the key)."""
        return (float(self.eta) == 0.0 or bool(self.device_noise)) and (self.control is None or bool(self.mixed))


def check_request(*, image, n, height, width, steps, scale, eta, seed, control, uncond, as_uint8, device_noise, solver,
                  control_preprocess, control_thresholds, init, strength, mask, composite, image_weights, regions,
                  region_weights, control_scale, control_layer_scales, control_window, control_cond_only, guidance_rescale,
                  num_timesteps, init_posterior='sample', first=0, n_local=None):
    """the arguments of a request of n samples (`PromptFreePipeline.generate` describes them), checked on the host before
    anything touches the device -> Request.  The one place where a feature's arguments are checked, for both doors.
    The caller runs the n_local samples from `first` on (generate: its rank's; default: all n): a per-sample argument is
    checked for all n, and what comes to nothing ON THOSE samples -- a control of strength 0, a phi of 0 -- is dropped from
    the record, which otherwise speaks of the whole request.  image, control and mask are kept as given, so a picture per
    sample is one per sample of the caller.  num_timesteps: a callable, asked only when a strength argument is off its
    default."""
    from . import control as control_lib
    from . import guidance as guidance_lib
    from .model_zoo.ddim import is_per_sample
    from .solver import solver_order
    n_local = int(n) if n_local is None else int(n_local)
    if solver_order(solver) is not None and (float(eta) != 0.0 or device_noise):     # an unknown name raises here too
        raise ValueError(f"solver {solver!r} is deterministic: eta must be 0 and device_noise off")
    image, image_weights, regional = check_regions(image, regions, region_weights, image_weights)
    refs = check_references(image, image_weights if regional is None else [1.0] * len(image))
    weights = None
    if refs is not None:      # one reference left: the plain request of that picture
        image, weights = (refs[0][0], None) if len(refs[0]) == 1 else (list(refs[0]), [float(w) for w in refs[1]])
    if is_per_sample(scale) and tuple(torch.as_tensor(scale).shape) != (n,):
        raise ValueError(f"scale must be one number or {n} numbers, one per sample of the global batch")
    cfg = is_per_sample(scale) or float(scale) != 1.0          # scale 1: no unconditional half
    if torch.is_tensor(guidance_rescale):
        guidance_rescale = guidance_rescale.detach().cpu().numpy()
    phi = guidance_lib.check_phi(guidance_rescale, n)
    rescale = guidance_lib.normalise(phi[first:first + n_local], n_local, 2 if cfg else 1)      # None: nothing of it on those samples
    if rescale is not None:
        rescale = phi.astype(np.float32)
    if torch.is_tensor(control) and control.dim() == 4 and control.shape[0] not in (1, n_local):
        raise ValueError(f"control must be [1, 3, H, W] (shared) or [{n_local}, 3, H, W] (one hint per local "
                         f"sample): got {control.shape[0]} hints")
    if weights is None and image_io.wants_ingest(image):
        image_io.check_u8_picture(image, 'image', min_side=32)
    if control is not None and image_io.wants_ingest(control):
        image_io.check_resize(image_io.check_u8_picture(control, 'control')[:2], (int(height), int(width)), 'control')
    thresholds = image_io.check_control_preprocess(control, control_preprocess, control_thresholds)
    init_k = None if init is None else image_io.check_img2img(init, int(height), int(width), int(steps), strength, init_posterior)
    image_io.check_mask(mask, init, int(height), int(width), composite, as_uint8, n=n_local)
    if mask is not None and float(eta) != 0.0 and not device_noise:
        raise ValueError("a masked request with eta > 0 needs device_noise=True: the masked step draws nothing from "
                         "the global generator")

    def total_k():      # (schedule length, steps the run evaluates)
        total = schedule_length(steps, num_timesteps())
        return total, total if init_k is None else int(init_k)
    ctl = check_control_strength(control, control_scale, control_layer_scales, control_window, control_cond_only, n,
                                 2 if cfg else 1, total_k, first=first, n_local=n_local)
    if ctl == 'off':
        control, ctl = None, None        # nothing left of the control: the uncontrolled request, before a hint is made
    elif ctl is not None:        # (strengths float64 [n], layer weights, controlled steps, cond_only); a server's key: all but the first
        ctl = (control_lib.sample_scales(control_scale.tolist() if torch.is_tensor(control_scale) else control_scale, n),
               tuple(float(v) for v in control_lib.layer_scales(control_layer_scales)), ctl[1], bool(control_cond_only) and cfg)
    return Request(image=image, weights=weights, regional=regional, ctl=ctl, rescale=rescale, n=int(n), height=int(height),
                   width=int(width), steps=int(steps), scale=scale, eta=eta, seed=int(seed), control=control, uncond=uncond,
                   as_uint8=as_uint8, device_noise=bool(device_noise), solver=solver, control_preprocess=control_preprocess,
                   control_thresholds=thresholds, init=init, strength=strength, init_k=init_k, mask=mask,
                   composite=bool(composite) if mask is not None else None)


class PromptFreePipeline:
    """One rank's view of a (possibly multi-GPU) request: shard -> encode -> DDIM loop -> decode -> gather.
    `sampler` is injectable (the gloo CPU tests drive this very code with a stand-in for the GPU compute)."""

    def __init__(self, net, rank=0, world_size=1, sampler=None):
        self.net = net
        if sampler is None:
            from .model_zoo.ddim import DDIMSampler
            sampler = DDIMSampler(net)
        self.sampler = sampler
        self.rank, self.world_size = rank, world_size
        self._ctx_stage = self._vae_stage = self._enc_stage = self._stages = None
        self._acp_host = None

    def enable_graph(self, on=True):
        """hipGraph replay for every stage: the DDIM loop (DDIMSampler.enable_graph) and, here, the context encode, the
        VAE decode and the VAE encode of an img2img start"""
        self.sampler.enable_graph(on)
        if on and self._stages is None:
            self._stages = (_GraphedStage(self.net, 'ctx_encode', 'image', self.net.ctx['image']),
                            _GraphedStage(self.net, 'vae_decode', 'image', self.net.vae['image']),
                            _GraphedStage(self.net, 'vae_encode_moments', 'image', self.net.vae['image']))
        self._ctx_stage, self._vae_stage, self._enc_stage = self._stages if on else (None, None, None)

    @serialised
    @torch.no_grad()
    def encode_reference(self, image, n):
        """image: [1,3,H,W] in [0,1] -> (cond [n,148,768], uncond zeros), app.py:234-236"""
        c = self._ctx_stage(image) if self._ctx_stage is not None else self.net.ctx_encode(image, 'image')
        cond = c.repeat(n, 1, 1)
        return cond, torch.zeros_like(cond)

    @serialised
    @torch.no_grad()
    def encode_reference_tokens(self, images, n):
        """the tokens of several references side by side: images, a list of uint8 HWC pictures / float [1,3,H,W] tensors
        -> (cond [n, R*Nk, C], zeros like it, Nk = tokens per reference).  SeeCoder runs once per reference (through the
        graphed stage when graphs are on)."""
        dev = self.net.device
        toks = []
        for ref in images:
            img = self.ingest(ref) if image_io.wants_ingest(ref) else ref.to(dev)
            toks.append(self._ctx_stage(img) if self._ctx_stage is not None else self.net.ctx_encode(img, 'image'))
        cond = torch.cat(toks, 1).repeat(n, 1, 1)
        return cond, torch.zeros_like(cond), int(toks[0].shape[1])

    @serialised
    @torch.no_grad()
    def encode_regions(self, images, region_weights, n):
        """regional mixing (lib/regions.py): the references' tokens and a row of logits per region
        -> (cond [n, R*Nk, C], zeros like it, table fp32 [n, NR, R*Nk])"""
        cond, zeros, nk = self.encode_reference_tokens(images, n)
        tab = torch.from_numpy(region_lib.region_bias(region_weights, nk, int(cond.shape[1])))
        return cond, zeros, tab.to(self.net.device)[None].repeat(n, 1, 1)

    @serialised
    @torch.no_grad()
    def encode_references(self, images, weights, n):
        """several references mixed in one UNet pass (lib/refmix.py): images, a list of uint8 HWC pictures / float [1,3,H,W]
        tensors, with one weight > 0 each -> (cond [n, R*Nk, C], zeros like it, bias fp32 [n, R*Nk]).  SeeCoder runs once
        per reference (through the graphed stage when graphs are on), the tokens are concatenated and every token carries
        log2(w_r / max w) (refmix.key_bias).  Not the reference's context_mixing."""
        w = refmix.check_weights(weights)
        if len(images) != w.size:
            raise ValueError(f"{len(images)} references but {w.size} weights")
        cond, zeros, nk = self.encode_reference_tokens(images, n)
        bias = torch.from_numpy(refmix.key_bias(w, nk, int(cond.shape[1]))).to(self.net.device)[None].repeat(n, 1)
        return cond, zeros, bias

    @staticmethod
    def pad_context(ctx, bias, nk):
        """a context [n, Nc, C] and its logits [n, Nc] padded to nk tokens: zero tokens at -inf"""
        nc = int(ctx.shape[1])
        if nc == nk:
            return ctx, bias
        pad = torch.zeros((ctx.shape[0], nk - nc, ctx.shape[2]), dtype=ctx.dtype, device=ctx.device)
        pb = torch.full((bias.shape[0], nk - nc), float('-inf'), dtype=bias.dtype, device=bias.device)
        return torch.cat([ctx, pad], 1), torch.cat([bias, pb], 1)

    @staticmethod
    def pad_uncond(uncond, bias_like):
        """an unconditional context [*, Nu, C] with fewer tokens than the mix [*, Nk]: zero tokens behind it and the logits
        of its rows, 0 on its own tokens and -inf on the padding -> (uncond [*, Nk, C], fp32 [*, Nk])"""
        nu, nk = int(uncond.shape[1]), int(bias_like.shape[1])
        if nu > nk:
            raise ValueError(f"uncond has {nu} tokens, the mixed context {nk}: an unconditional context longer than the mix "
                             "is not served")
        pad = torch.zeros((uncond.shape[0], nk - nu, uncond.shape[2]), dtype=uncond.dtype, device=uncond.device)
        ub = torch.zeros((uncond.shape[0], nk), dtype=torch.float32, device=uncond.device)
        ub[:, nu:] = float('-inf')
        return torch.cat([uncond, pad], 1), ub

    def _dtypes(self):
        """(the model dtype, the dtype the picture kernels write for it: fp16 and fp32 themselves, fp32 for any other)"""
        dtype = self.net.get_dtype() if hasattr(self.net, 'get_dtype') else torch.float32
        return dtype, (dtype if dtype in (torch.float16, torch.float32) else torch.float32)

    @serialised
    @torch.no_grad()
    def ingest(self, picture, size=None, what='image'):
        """uint8 HWC picture (torch or numpy, any size) -> [1,3,H,W] in [0,1] in the model dtype, on the device:
        `ToTensor()(im)[None].to(device).to(dtype)` (app.py:234), behind `im.resize([W, H], BICUBIC)` when size = (H, W)
        is given (app.py:232,244) -- both as HIP kernels (ops.image_from_u8); one byte per channel crosses PCIe"""
        u8 = image_io.to_device_u8(picture, self.net.device, what)
        dtype, kdtype = self._dtypes()
        x = ops.image_from_u8(u8, size, dtype=kdtype)
        return x if kdtype == dtype else x.to(dtype)

    @serialised
    @torch.no_grad()
    def control_hint(self, control, height, width, preprocess=None, thresholds=(100, 200)):
        """the hint the ControlNet is given for `control`, [1|n,3,height,width] in the model dtype on the device -- what
        app.py:244-249 calls `cc` and shows next to the results (app.py:272).  preprocess None: the picture itself (a
        uint8 picture resized to (height, width), `ingest`; a float tensor as it is).  'canny': its Canny edges
        (ControlNet.preprocess(type='canny'), app.py:246) at `thresholds` = (low, high): a uint8 picture is resized on
        the device AS uint8 and handed to the detector, which writes the hint in the model dtype (ops.canny_u8) -- no
        float picture, no byte round trip; a float tensor goes through net.ctl.preprocess, which makes the bytes."""
        low, high = image_io.check_control_preprocess(control, preprocess, thresholds)
        dev = self.net.device
        if preprocess is None:
            return self.ingest(control, (height, width), 'control') if image_io.wants_ingest(control) else control.to(dev)
        dtype, kdtype = self._dtypes()
        if image_io.wants_ingest(control):
            image_io.check_resize(image_io.check_u8_picture(control, 'control')[:2], (height, width), 'control')
            u8 = ops.image_from_u8(image_io.to_device_u8(control, dev, 'control'), (height, width), layout='u8')
            hint = ops.canny_u8(u8, low, high, out='hint', dtype=kdtype)
            return hint if kdtype == dtype else hint.to(dtype)
        return self.net.ctl.preprocess(control.to(dev), type=preprocess, low_threshold=low, high_threshold=high,
                                       size=[height, width]).to(dtype)

    def _level(self, steps, k):
        """a_t of an img2img start that runs k of `steps` steps: alphas_cumprod at ddim_timesteps[k - 1], the first
        timestep the loop evaluates (lib/img2img.py) -- the number DDIMSampler.make_schedule puts in ddim_alphas[k - 1]"""
        from .img2img import level
        from .model_zoo.diffusion_utils import make_ddim_timesteps
        acp = self.net.alphas_cumprod
        if self._acp_host is None or self._acp_host[0] is not acp:
            self._acp_host = (acp, acp.detach().float().cpu().numpy())     # one copy per schedule tensor, not per request
        ts = make_ddim_timesteps("uniform", steps, self.net.num_timesteps, verbose=False)
        return level(self._acp_host[1], ts, k)

    @serialised
    @torch.no_grad()
    def init_latent(self, init, height, width, steps, strength, keys, posterior='sample', want_x0=False):
        """the seeded start of an img2img request -> (x_t fp32 [n, 4, height/8, width/8] on the device, k): the latent of
        `init` -- a uint8 HWC picture of any size, resized to (height, width) on the device straight into the f16 NHWC
        the encoder reads, or a float tensor [1, 3, height, width] in [0, 1] -- sampled from the VAE posterior (or its
        mode), scaled and noised to the level of the first of the k = start_steps(steps, strength) steps the request
        runs, in one launch behind the encoder (ops.latent_start).  keys: int64 [n, 2] rows (seed, sample_id): sample i's
        start is a function of the picture and keys[i] alone (lib/img2img.py); the picture is encoded once.
        want_x0: -> (x_t, k, x0), x0 the clean latent of the same draw, what a masked request keeps outside its mask."""
        k = image_io.check_img2img(init, height, width, steps, strength, posterior)
        dev = self.net.device
        if image_io.wants_ingest(init):
            pic = ops.image_from_u8(image_io.to_device_u8(init, dev, 'init'), (int(height), int(width)), layout='nhwc')
        else:
            pic = init.to(dev)
        moments = self._enc_stage(pic) if self._enc_stage is not None else self.net.vae_encode_moments(pic, 'image')
        sf = (getattr(self.net, 'latent_scale_factor', None) or {}).get('image', None)
        out = ops.latent_start(moments, keys.to(dev), 1.0 if sf is None else sf, self._level(steps, k), posterior=posterior,
                               want_x0=want_x0)
        return (out[1], k, out[0]) if want_x0 else (out, k)

    @serialised
    @torch.no_grad()
    def mask_grid(self, mask, height, width, n=None):
        """the mask of an inpainting request at latent resolution -> fp32 [1 | n, height/8, width/8] on the device, 1 =
        regenerate: a uint8 mask [Hm, Wm] of any size (>= 128: regenerate) is reduced on the device by the dilating rule of
        lib/inpaint.py (ops.mask_grid_u8: a marked pixel always lies in a regenerated cell); a float tensor already at
        latent resolution passes through after the shape check (soft values in [0, 1] are legal; a leading axis of n gives
        each of the n samples its own mask)."""
        kind = image_io.check_mask(mask, True, height, width, n=n)
        dev = self.net.device
        gh, gw = int(height) // 8, int(width) // 8
        if kind == 'u8':
            return ops.mask_grid_u8(self._mask_u8(mask), gh, gw, torch.float32)
        return mask.to(device=dev, dtype=torch.float32).reshape(-1, gh, gw).contiguous()

    def _mask_u8(self, mask):
        """a checked uint8 mask -> contiguous uint8 [Hm, Wm] on the device"""
        m = mask if torch.is_tensor(mask) else torch.from_numpy(mask)
        return m.reshape(int(m.shape[0]), int(m.shape[1])).contiguous().to(self.net.device)

    @serialised
    @torch.no_grad()
    def composite(self, images_u8, init, mask, height, width):
        """decoded uint8 images [n, H, W, 3] with everything outside the mask replaced by the bytes of the init picture
        (resized to the output size as the request's start was): the selection is the mask reduced to the PIXEL grid by
        the same dilating rule (ops.mask_grid_u8), so it covers every marked pixel; one launch (ops.composite_u8)"""
        dev = self.net.device
        H, W = int(height), int(width)
        init_u8 = ops.image_from_u8(image_io.to_device_u8(init, dev, 'init'), (H, W), layout='u8')
        sel = ops.mask_grid_u8(self._mask_u8(mask), H, W, torch.uint8)
        return ops.composite_u8(images_u8, init_u8, sel)

    @serialised
    @torch.no_grad()
    def generate(self, image, n_global, height, width, steps=50, scale=2.0, eta=0.0, seed=20, control=None,
                 uncond=None, decode=True, gather=False, verbose=False, timings=None, as_uint8=False,
                 device_noise=False, solver='ddim', control_preprocess=None, control_thresholds=(100, 200), init=None,
                 strength=0.75, init_posterior='sample', mask=None, composite=False, image_weights=None, regions=None,
                 region_weights=None, control_scale=1.0, control_layer_scales=None, control_window=(0.0, 1.0),
                 control_cond_only=False, guidance_rescale=0.0):
        """returns (images, latents [n_local,4,h,w]); images = [n_local | n_global (gather), 3, H, W] in [0,1]
        in the model dtype, or -- as_uint8 -- packed uint8 [n, H, W, 3] (the bytes ToPILImage would produce,
        app.py:273-275; 4x fewer bytes through the all-gather); decode=False returns the latents twice.
        `image` and `control` may each be a uint8 HWC picture of any size instead of a float tensor (`ingest`): the
        reference picture is converted as it is and shared by all samples, the control picture is resized to
        (height, width) first.
        device_noise: the per-step noise of eta > 0 is the seeded counter-based noise of lib/noise.py, sample j of the
        GLOBAL batch keyed (seed, j), evaluated inside the DDIM step kernel: the result does not depend on the world
        size (like x_T) and the loop replays as a hipGraph.  False: the reference's draw from the global generator.
        scale: one number, or a sequence / tensor of n_global numbers: sample j of the GLOBAL batch is guided with
        scale[j] (pfd_cfg_ddim_step_ps; CFG is then on for every sample, also one whose scale is 1).
        control: [1,3,H,W] is one hint shared by all samples; [n_local,3,H,W] is one hint PER SAMPLE of this rank.
        solver: 'ddim', or 'dpmpp_2m' -- DPM-Solver++(2M), second order, on the same `steps` timesteps (lib/solver.py;
        typically 20 to 25 steps in place of 50) -- or 'dpmpp_1', its first-order form (DDIM at eta 0).  The last two are
        deterministic: eta = 0, no device_noise.
        control_preprocess: None -- the control picture is the hint -- or 'canny': the hint is the picture's Canny edges at
        control_thresholds = (low, high), computed on the device (`control_hint`; app.py:246 with do_preprocess=True).
        init: image-to-image -- a uint8 HWC picture of any size or a float [1,3,height,width] tensor in [0,1] shared by all
        samples.  The trajectory starts from the picture's latent noised to the level of the first of the
        k = min(steps, int(steps * strength)) steps it runs (`init_latent`) instead of from x_T: no x_T is drawn, sample j
        of the GLOBAL batch draws its posterior and forward noise keyed (seed, j), so the result does not depend on the
        world size.  strength in (0, 1]: 1 runs every step (the picture only shades the start), small values stay close
        to the picture.  init_posterior: 'sample' or 'mode' (the posterior mean).  timings gains init_encode_ms.
        mask: inpainting (needs init) -- a uint8 mask [Hm, Wm] of any size, >= 128 marking what to regenerate, or a float
        tensor at latent resolution (`mask_grid`).  Every step of the loop then keeps the latent outside the mask on the init
        picture's own noised trajectory (pfd_cfg_step_masked, lib/inpaint.py), keyed (seed, j) per sample of the GLOBAL batch
        like the start: no generator, the result does not depend on the world size, the loop replays as a hipGraph.  The
        final latent outside the mask is the picture's clean latent itself.  eta > 0 needs device_noise.  composite (needs
        as_uint8, a uint8 init and a uint8 mask): the pixels outside the mask are the init picture's bytes (`composite`),
        before the gather.
        image_weights: several references mixed in ONE UNet pass -- image=[ref0, ref1, ...] (each a uint8 HWC picture of any
        size or a float [1,3,H,W] tensor, shared by all samples) with one number >= 0 per reference: every cross-attention
        attends over the union of the references' tokens, each key weighted by its reference's weight (lib/refmix.py,
        `encode_references`; pfd_attention_kbias_f16).  Only the ratios matter.  A reference of weight 0 is dropped before it
        is encoded; with one reference left the request IS the plain request of that picture.  An `uncond` with fewer tokens
        than the mix is padded with zero tokens that carry weight 0.  Works with every other argument; draws nothing, so the
        result does not depend on the world size.  Not the reference's context_mixing (sample_multicontext).
        regions, region_weights (instead of image_weights): regional mixing, lib/regions.py -- regions is a uint8 map [Hm, Wm]
        of any size whose pixel value is a region id, region_weights[g][r] >= 0 the weight of reference r in region g (up to
        8 regions; every row with a weight > 0).  A query of a cross-attention listens to the references at the weights of the
        region under the centre of its cell (regions.region_grid, every UNet level from the map itself;
        pfd_attention_rbias_f16).  One region IS the image_weights request of its row, a reference no region uses is dropped,
        one reference left IS the plain request.  Works with every other argument; draws nothing.
        control_scale, control_layer_scales, control_window, control_cond_only (with control; lib/control.py): how strongly,
        in which layers and on which steps the hint binds.  control_scale: one number >= 0 or one per sample of the GLOBAL
        batch.  control_layer_scales: None, 'soft' (0.825 ** (12 - i): the deep layers bind, the shallow ones give way to the
        reference picture) or 13 numbers >= 0, one per ControlNet residual.  control_window = (start, end) in [0, 1]: the
        part of the FULL schedule that is controlled, 0 the first (noisiest) step -- the same noise levels whatever
        `strength` is; a step outside it is the uncontrolled step and does not run the ControlNet.  control_cond_only: the
        unconditional half of the CFG batch gets no control.  All at their defaults: the plain control request, its path,
        graph and bits.  Nothing left of the control (scale 0, an empty window): the request without `control`, bit for bit.
        Works with every other argument; draws nothing.
        guidance_rescale: phi in [0, 1], one number or one per sample of the GLOBAL batch (lib/guidance.py; Lin et al. 2023,
        section 3.4; diffusers' `guidance_rescale`): the guided eps of every step is brought back to the standard deviation
        of the sample's conditional eps and blended by phi, which keeps pictures from burning out at the scales used with a
        reference (0.7 is the paper's value).  One small launch in front of the step kernel (pfd_guidance_rescale_f32); a
        sample's result does not depend on its company nor on the world size.  0 (or all zero, or scale 1): the plain
        request, its path, graph and bits.  Works with every other argument; draws nothing."""
        P, r = self.world_size, self.rank
        if n_global % P:
            raise ValueError("global batch must divide over the ranks")
        n = n_global // P
        req = check_request(
            image=image, n=n_global, height=height, width=width, steps=steps, scale=scale, eta=eta, seed=seed, control=control,
            uncond=uncond, as_uint8=as_uint8, device_noise=device_noise, solver=solver, control_preprocess=control_preprocess,
            control_thresholds=control_thresholds, init=init, strength=strength, mask=mask, composite=composite,
            image_weights=image_weights, regions=regions, region_weights=region_weights, control_scale=control_scale,
            control_layer_scales=control_layer_scales, control_window=control_window, control_cond_only=control_cond_only,
            guidance_rescale=guidance_rescale, num_timesteps=lambda: self.net.num_timesteps, init_posterior=init_posterior,
            first=r * n, n_local=n)
        if composite and not decode:
            raise ValueError("composite=True needs decode=True")
        mk = _Marks(torch.device(self.net.device).type == 'cuda') if timings is not None else None
        if mk:
            mk.mark()
        x_info, c_info, shape = self.assemble([(req, r * n, n)], posterior=init_posterior, mark=mk.mark if mk else None)
        how = {} if solver == 'ddim' else {'solver': solver}     # the default call is what it was
        x, _ = self.sampler.sample(steps=steps, shape=shape, x_info=x_info, c_info=c_info, eta=eta,
                                   verbose=verbose, **how)
        if mk:
            mk.mark()
        if not decode:
            return x, x
        if as_uint8:
            img = self.net.vae_decode(x, 'image', out_uint8=True)
            if composite:
                img = self.composite(img, init, mask, height, width)
        else:       # (float images go through the graphed VAE stage here; a server decodes them directly)
            img = self._vae_stage(x) if self._vae_stage is not None else self.net.vae_decode(x, 'image')
        if mk:
            mk.mark()
            if mk.on_gpu:
                torch.cuda.synchronize()
            o = 0 if init is None else 1      # the mark behind the init encode
            timings.update(ctx_encode_ms=mk.ms(0, 1), ddim_loop_ms=mk.ms(1 + o, 2 + o), vae_decode_ms=mk.ms(2 + o, 3 + o))
            if init is not None:
                timings.update(init_encode_ms=mk.ms(1, 2))
        if gather:
            img = all_gather_batch(img, P)
        return img, x

    @serialised
    @torch.no_grad()
    def assemble(self, slices, coalesced=False, posterior='sample', mark=None, draw_xT=None):
        """slices of checked requests -> (x_info, c_info, shape) of ONE sampler call: the one place where a feature's entries
        of x_info / c_info are built, for both doors.  slices: [(Request, first sample, n), ...] -- samples [first, first + n)
        of each request, side by side in that order.  generate hands over one slice, its rank's; a server one per request of
        the batch, from 0 on.  What is equal over a batch (a server's key says so) is read from the first request.
        coalesced -- the slices are a server's batch, several requests side by side: every context is expanded to its samples
        and mixed contexts are padded to the longest of the batch, the logits of the unconditional rows are there when any
        request gave an uncond, every sample has its own mask and its own region map.  False, generate's one request: an
        uncond is handed on as given and padded (`pad_uncond`) only where it is shorter than a mix, a mask stays [1 | n, h, w],
        the region map is the one map.
        posterior: the init_posterior of generate.  mark: called behind the context encode and behind the init encode of a
        slice (generate's timings).  draw_xT: the caller's `shard_xT` -- a server hands over the one of ITS module, so that
        whoever replaces `serving.shard_xT` (a test that proves that no x_T is drawn) replaces what runs; None: this module's."""
        from . import control as control_lib
        from .model_zoo.ddim import is_per_sample
        from .noise import sample_keys
        dev = self.net.device
        r0 = slices[0][0]
        mixing = r0.weights is not None or r0.regional is not None
        conds, unconds, xts, keys, masks, x0s, biases, tables, rmaps = ([] for _ in range(9))
        for r, first, n in slices:
            if r.regional is not None:          # the references' tokens side by side; ITS table and ITS map (of its own size)
                c, z, tab = self.encode_regions(r.image, r.regional[1], n)
                tables.append(tab)
                rmaps.extend([r.regional[0]] * n)
            elif r.weights is not None:         # several references: ITS tokens and ITS row of logits
                c, z, kb = self.encode_references(r.image, r.weights, n)
                biases.append(kb)
            elif not image_io.wants_ingest(r.image) and r.image.shape[0] > 1:
                # one reference image PER SAMPLE (the "+737 GFLOP/img" variant): SeeCoder is run once per image
                # (its decoder MHA attends across the batch axis, seecoder.py:70,83 -- a batch of images would mix them)
                if r.image.shape[0] != n:
                    raise ValueError(f"{r.image.shape[0]} reference images for {n} local samples")
                pairs = [self.encode_reference(r.image[i:i + 1].to(dev), 1) for i in range(n)]
                c, z = torch.cat([c for c, _ in pairs]), torch.cat([z for _, z in pairs])
            else:
                c, z = self.encode_reference(self.ingest(r.image) if image_io.wants_ingest(r.image) else r.image.to(dev), n)
            conds.append(c)
            if r.uncond is None:
                unconds.append(z)
            else:
                unconds.append(r.uncond.to(dev).to(c.dtype).expand(n, -1, -1) if coalesced else r.uncond)
            if mark:
                mark()
            key = torch.from_numpy(sample_keys(r.seed, first, n))      # sample j of the request is keyed (seed, j), int64 [n, 2]
            keys.append(key)
            if r.init is None:                  # ITS x_T stream, drawn once for the whole request (CPU generator)
                xts.append((draw_xT or shard_xT)(r.n, r.height, r.width, r.seed, 0, 1)[first:first + n])
                continue
            start = self.init_latent(r.init, r.height, r.width, r.steps, r.strength, key, posterior, want_x0=r.mask is not None)
            xts.append(start[0])                # ... or ITS picture, noised under ITS keys
            if r.mask is not None:              # ... and ITS mask over ITS clean latent
                x0s.append(start[2])
                m = self.mask_grid(r.mask, r.height, r.width, n=None if coalesced else n)
                masks.append(m[:1].expand(n, -1, -1) if coalesced else m)
            if mark:
                mark()
        ubias = None
        if coalesced and mixing and r0.regional is None:
            # contexts of different lengths: padded to the longest of the batch with zero tokens at -inf
            nk = max(int(t.shape[1]) for t in conds + unconds)      # (an uncond longer than every mix is padded to as well)
            ubiases = []
            for i, (c, u, kb) in enumerate(zip(conds, unconds, biases)):
                conds[i], biases[i] = self.pad_context(c, kb, nk)
                ub = torch.zeros((u.shape[0], u.shape[1]), dtype=torch.float32, device=u.device)
                unconds[i], ub = self.pad_context(u, ub, nk)
                ubiases.append(ub)
            if any(r.uncond is not None for r, _, _ in slices):
                ubias = torch.cat(ubiases)
        elif not coalesced and mixing and r0.uncond is not None and r0.uncond.shape[1] != conds[0].shape[1]:
            n = slices[0][2]
            unconds[0], ubias = self.pad_uncond(r0.uncond.to(dev).to(conds[0].dtype), conds[0][:, :, 0])
            if unconds[0].shape[0] == 1 and n > 1:
                unconds[0], ubias = unconds[0].expand(n, -1, -1), ubias.expand(n, -1)
        xT = torch.cat(xts).to(dev)
        x_info = {'type': 'image', 'xt': xT}
        if r0.init is not None:
            x_info['xt_steps'] = r0.init_k       # equal over a batch: part of the key
        if r0.device_noise:
            x_info['noise_key'] = torch.cat(keys).to(dev)
        if r0.mask is not None:
            x_info.update(mask=torch.cat(masks).contiguous(), x0_keep=torch.cat(x0s), keep_key=torch.cat(keys).to(dev))
        # a scale per sample: a vector given to generate, or a mixed server's batch (its scale-1 key keeps the batch without
        # CFG); else one scale stays the Python number it was given as
        per_sample = is_per_sample(r0.scale) or (bool(r0.mixed) and float(r0.scale) != 1.0)
        scale = r0.scale
        if per_sample:                          # fp32 [N]: each sample its request's scale, or its own entry of it
            rows = [torch.as_tensor(r.scale).detach().to(device='cpu', dtype=torch.float32).reshape(-1) for r, _, _ in slices]
            scale = torch.cat([v.expand(r.n)[f:f + n] for v, (r, f, n) in zip(rows, slices)])
        c_info = {'type': 'image', 'conditioning': torch.cat(conds), 'unconditional_conditioning': torch.cat(unconds),
                  'unconditional_guidance_scale': scale}
        if r0.regional is not None:             # (equal numbers of references over a batch: the key says so, nothing to pad)
            c_info['region_bias'], c_info['region_map'] = torch.cat(tables), (rmaps if coalesced else r0.regional[0])
            if ubias is not None:
                c_info['unconditional_region_bias'] = ubias[:, None].expand(-1, c_info['region_bias'].shape[1], -1)
        elif r0.weights is not None:
            c_info['key_bias'] = torch.cat(biases)
            if ubias is not None:
                c_info['unconditional_key_bias'] = ubias
        if r0.control is not None:
            # a mixed server's batch: one hint per sample [N,3,H,W], every request's picture ingested on its own (uint8
            # pictures may differ in source size) and repeated over the request's samples; else the one hint (or hints) given
            def hint(r):
                return self.control_hint(r.control, r.height, r.width, r.control_preprocess, r.control_thresholds or (100, 200))
            c_info['control'] = torch.cat([hint(r).expand(n, -1, -1, -1) for r, _, n in slices]) if r0.mixed else hint(r0)
        if r0.ctl is not None:      # each sample its own rows of the table (layers, steps, cond_only are equal over a batch)
            strengths = [float(v) for r, f, n in slices for v in r.ctl[0][f:f + n]]
            tab = control_lib.scale_table(strengths, r0.ctl[1], len(strengths), 2 if per_sample or float(r0.scale) != 1.0 else 1,
                                          r0.ctl[3])
            c_info['control_scale'], c_info['control_steps'] = torch.from_numpy(tab).to(dev), r0.ctl[2]
        if r0.rescale is not None:  # each sample its own phi
            c_info['guidance_rescale'] = torch.from_numpy(np.concatenate([r.rescale[f:f + n] for r, f, n in slices]))
        return x_info, c_info, list(xT.shape)
