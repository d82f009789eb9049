"""Queued, batched serving in front of ONE shared model -- the request front-end of SURVEY 8(f)-3.

The reference serves requests by letting Gradio's worker threads call `action_inference` on a global
model with no lock and one request = one `sampler.sample` of `n_sample_image` samples (app.py:229-277,
405-410).  Here every request goes through a FIFO; one worker thread owns the device and

  * coalesces compatible queued requests (same output size, step count, solver, guidance scale, eta, noise kind, control /
    unconditional-context kind) into ONE DDIM batch (eta > 0 only with `device_noise=True`, see `shareable`): samples are independent on this path, every sample
    carries its own SeeCoder context in the cross-attention K / V^T cache, so four single-image requests
    cost one batch-4 loop instead of four batch-1 loops (the UNet at batch 2 fills 1/4 of the chip);
  * applies weight hot swaps (`load`, the per-request tag switches of app.py:217-222) strictly in queue
    order between batches -- the packed-weight caches and captured hipGraphs are keyed on the parameter
    versions, so the next batch re-packs / re-captures;
  * returns packed uint8 HWC images (`ToPILImage`'s arithmetic on the device, pfd_image_u8_f16) or the
    float images, through `concurrent.futures.Future`s.

`mixed_batches=True` (opt-in) takes two entries out of that list.  The guidance scale becomes per-sample
(pfd_cfg_ddim_step_ps): the key keeps only "scale == 1" (those requests keep the cheaper half-size batch without CFG
among themselves), every other batch runs with a scale vector and one captured graph per shape whatever the scales
are.  ControlNet requests share a batch with other ControlNet requests, each sample with its own hint.  Still per
batch: output size, steps, eta, noise kind, output kind, with / without control, unconditional-context kind.

ControlNet strength (submit(control_scale=, control_layer_scales=, control_window=, control_cond_only=), lib/control.py): a
request whose arguments are off their defaults shares a batch only with requests that have them too, with equal layer
weights, equal controlled steps and equal cond_only; the strengths may differ, each sample has its own rows of the table.
A request with nothing left of its control (scale 0, an empty window) IS the uncontrolled request and batches as one.

Guidance rescale (submit(guidance_rescale=), lib/guidance.py): the key gains "has rescale", not the values -- requests with
it share a batch whatever their phi, each sample with its own (the vector is a static input of one captured graph); a
request without it (0, or scale 1) never shares a batch with one that has it, so it keeps its graph and its bits.
"""
import queue
import threading
from concurrent.futures import Future

import torch

from . import image_io
from .pipeline import (PromptFreePipeline, check_control_strength, check_references, check_regions, schedule_length,
                       shard_noise_keys, shard_xT)
from .solver import solver_order


class _Request:
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


class PromptFreeServer:
    def __init__(self, net, use_graph=True, max_batch=8, max_wait_s=0.0, mixed_batches=False):
        """mixed_batches: requests that differ in guidance scale (other than scale 1) or in control picture share a
        batch; see the module docstring.  False: one scale per batch, ControlNet requests alone."""
        self.net = net
        self.mixed_batches = bool(mixed_batches)
        self.pipe = PromptFreePipeline(net)
        self.pipe.enable_graph(use_graph)
        self.max_batch, self.max_wait_s = int(max_batch), float(max_wait_s)
        self._q = queue.Queue()
        self._stop = False
        self.batches = []                  # sizes of the DDIM batches run so far (observability / tests)
        self._worker = threading.Thread(target=self._run, name="pfd-server", daemon=True)
        self._worker.start()

    # ---- client side (any thread) -------------------------------------------------------------------
    def submit(self, image, n_samples=1, height=512, width=512, steps=50, scale=2.0, eta=0.0, seed=20,
               control=None, uncond=None, as_uint8=True, device_noise=False, solver='ddim', control_preprocess=None,
               control_thresholds=(100, 200), init=None, strength=0.75, mask=None, composite=False, image_weights=None,
               regions=None, region_weights=None, control_scale=1.0, control_layer_scales=None, control_window=(0.0, 1.0),
               control_cond_only=False, guidance_rescale=0.0):
        """image [1,3,h,w] in [0,1] (any size); control [1,3,H,W] or None; uncond [1,148,768] or None (zeros).
        image and control may each be a uint8 HWC picture [h,w,3] (torch or numpy, any size; the reference picture
        at least 32 a side) instead: the request carries the bytes and the worker converts them on the device
        (PromptFreePipeline.ingest), the control picture resized to (height, width) as app.py:232 does.
        device_noise: with eta > 0, sample j of the request draws the seeded noise keyed (seed, j) inside the step kernel
        (lib/noise.py) instead of the global generator: its images do not depend on what it was batched with, so such
        requests are coalesced like eta = 0 ones.
        solver: 'ddim', 'dpmpp_2m' (DPM-Solver++(2M), lib/solver.py) or 'dpmpp_1'; the last two need eta = 0 and no
        device_noise, and share batches only with requests of the same solver.
        control_preprocess: None, or 'canny': the worker turns the control picture into its Canny edge hint at
        control_thresholds = (low, high) on the device (PromptFreePipeline.control_hint).  A preprocessed control is a
        control: the batch key does not change.
        init: image-to-image (PromptFreePipeline.init_latent) -- a uint8 HWC picture of any size or a float
        [1,3,height,width] tensor: the request starts from that picture's latent, noised for the
        k = min(steps, int(steps * strength)) steps it runs, sample j keyed (seed, j).  Such requests share a batch with
        each other when k (and the rest of the key) is equal, each with its own picture and keys.
        mask: inpainting (needs init; PromptFreePipeline.generate) -- a uint8 mask [Hm, Wm] of any size, >= 128 marking what
        to regenerate, or a float tensor [height/8, width/8]: outside the mask the result stays the init picture.  Masked
        requests of equal k share a batch with each other, each with its own picture, mask and keys; never with unmasked
        ones.  eta > 0 needs device_noise.  composite (needs as_uint8, a uint8 init and a uint8 mask): the pixels outside
        the mask are the init picture's bytes.
        image_weights: several references mixed in one UNet pass (PromptFreePipeline.generate, lib/refmix.py) --
        image=[ref0, ref1, ...] with one number >= 0 per reference.  Such requests share a batch with each other (equal in
        the other key fields) whatever their numbers of references: contexts are padded to the longest of the batch with
        zero tokens of weight 0, each sample with its own row of logits.  A request without image_weights never shares a
        batch with one that has them.  One reference left after dropping zero weights is the plain request.
        regions, region_weights: regional mixing (PromptFreePipeline.generate, lib/regions.py) -- a uint8 map [Hm, Wm] of region
        ids and a row of weights per region, instead of image_weights.  Regional requests share a batch only with regional
        requests of the same output size, number of regions and number of references (equal in the other key fields), each
        sample with its own map (of its own size) and table; never with plain or image_weights requests.  One region is the
        image_weights request, one reference left the plain request.  An uncond is not taken with regions here.
        control_scale, control_layer_scales, control_window, control_cond_only (with control; PromptFreePipeline.generate,
        lib/control.py): control_scale is one number or n_samples numbers.  Off their defaults, the request shares a batch
        only with requests that have them too and agree in layer weights, controlled steps and cond_only -- the strengths
        may differ.  Nothing left of the control: the request is served as the one without `control`.
        guidance_rescale: phi in [0, 1], one number or n_samples numbers (PromptFreePipeline.generate, lib/guidance.py).
        Requests with it share a batch whatever their phi, never with requests without it; 0, or scale 1, is the request
        without it.
        -> Future of uint8 [n,H,W,3] (as_uint8) or float [n,3,H,W] images"""
        if self._stop:
            raise RuntimeError("server is closed")
        if height % 64 or width % 64:
            raise ValueError("output size must be a multiple of 64 (app.py:226-227)")
        # everything a coalesced batch would first touch inside _generate is checked HERE, on the caller's thread: a
        # malformed tensor must fail its own request, not the batch it was merged into
        if n_samples < 1 or n_samples > self.max_batch:
            raise ValueError(f"n_samples must be in [1, {self.max_batch}]")
        if steps < 1:
            raise ValueError("steps must be >= 1")
        if solver_order(solver) is not None and (float(eta) != 0.0 or device_noise):     # an unknown name raises here too
            raise ValueError(f"solver {solver!r} is deterministic: eta must be 0 and device_noise off")
        image, image_weights, regional = check_regions(image, regions, region_weights, image_weights)
        if regional is not None and uncond is not None:
            raise ValueError("a regional request takes no uncond on the server (PromptFreePipeline.generate does)")
        refs = check_references(image, image_weights if regional is None else [1.0] * len(image))
        weights = None
        if refs is not None:
            for ref in refs[0]:
                if torch.is_tensor(ref) and ref.is_floating_point() and min(ref.shape[2:]) < 32:
                    raise ValueError("a reference picture must be at least 32 a side")
            image, weights = (refs[0][0], None) if len(refs[0]) == 1 else (list(refs[0]), [float(w) for w in refs[1]])
        if weights is not None:
            pass                                    # every reference was checked by check_references
        elif image_io.wants_ingest(image):          # a uint8 picture (anything that is not a torch tensor is checked as one)
            image_io.check_u8_picture(image, "image", min_side=32)
        elif not (image.dim() == 4 and image.shape[0] == 1 and image.shape[1] == 3 and image.is_floating_point() and
                  min(image.shape[2:]) >= 32):
            raise ValueError("image must be a float tensor [1, 3, h, w] in [0, 1] or a uint8 picture [h, w, 3]")
        if uncond is not None and not (torch.is_tensor(uncond) and uncond.is_floating_point() and
                                       tuple(uncond.shape) == (1, 148, 768)):
            raise ValueError("uncond must be a float tensor [1, 148, 768]")
        if control is not None and image_io.wants_ingest(control):
            image_io.check_resize(image_io.check_u8_picture(control, "control")[:2], (int(height), int(width)), "control")
        elif control is not None and not (control.is_floating_point() and
                                          tuple(control.shape) == (1, 3, int(height), int(width))):
            raise ValueError(f"control must be a float tensor [1, 3, {height}, {width}] or a uint8 picture [h, w, 3]")
        thresholds = image_io.check_control_preprocess(control, control_preprocess, control_thresholds)
        init_k = None if init is None else image_io.check_img2img(init, int(height), int(width), int(steps), strength)
        image_io.check_mask(mask, init, int(height), int(width), composite, as_uint8, n=1)
        if mask is not None and float(eta) != 0.0 and not device_noise:
            raise ValueError("a masked request with eta > 0 needs device_noise=True")
        from . import control as control_lib
        ctl = check_control_strength(
            control, control_scale, control_layer_scales, control_window, control_cond_only, int(n_samples),
            1 if float(scale) == 1.0 else 2,
            lambda: (schedule_length(steps, getattr(self.net, 'num_timesteps', 1000)),) * 2 if init_k is None else
            (schedule_length(steps, getattr(self.net, 'num_timesteps', 1000)), int(init_k)))
        if ctl == 'off':
            control, ctl = None, None
        elif ctl is not None:        # (strengths float64 [n], layer weights, controlled steps, cond_only): the last three are the key
            ctl = (control_lib.sample_scales(control_scale.tolist() if torch.is_tensor(control_scale) else control_scale, n_samples),
                   tuple(float(v) for v in control_lib.layer_scales(control_layer_scales)), ctl[1],
                   bool(control_cond_only) and float(scale) != 1.0)
        from . import guidance as guidance_lib
        rescale = guidance_lib.normalise(guidance_rescale.tolist() if torch.is_tensor(guidance_rescale) else guidance_rescale,
                                         int(n_samples), 1 if float(scale) == 1.0 else 2)
        r = _Request(image=image, ctl=ctl, rescale=rescale, n=int(n_samples), height=int(height), width=int(width), steps=int(steps), init=init,
                     strength=strength, init_k=init_k, mask=mask, composite=bool(composite) if mask is not None else None,
                     scale=scale, eta=eta, seed=int(seed), control=control, uncond=uncond, as_uint8=as_uint8,
                     device_noise=bool(device_noise), future=Future(), mixed=self.mixed_batches or None, solver=solver,
                     control_preprocess=control_preprocess, control_thresholds=thresholds, weights=weights, regional=regional)
        self._q.put(r)
        return r.future

    def load(self, kind, path):
        """queue a weight hot swap ('ctx' | 'diffuser' | 'ctl', app.py:139-161); applied in order"""
        f = Future()
        self._q.put(("load", kind, path, f))
        return f

    def call(self, fn):
        """queue an arbitrary action on the model (e.g. attaching a PPE_MLP, app.py:166-177); applied in order"""
        f = Future()
        self._q.put(("call", fn, None, f))
        return f

    def close(self):
        self._stop = True
        self._q.put(None)
        self._worker.join()
        while True:      # a submit() that raced past the _stop check sits behind the sentinel: fail it, never leave it pending
            try:
                item = self._q.get_nowait()
            except queue.Empty:
                break
            f = item.future if isinstance(item, _Request) else (item[3] if isinstance(item, tuple) else None)
            if f is not None and not f.done():
                f.set_exception(RuntimeError("server is closed"))

    # ---- worker -------------------------------------------------------------------------------------
    def _run(self):
        pending = None
        while True:
            item = pending if pending is not None else self._q.get()
            pending = None
            if item is None:
                break
            if isinstance(item, tuple):
                self._control(item)
                continue
            batch, total = [item], item.n
            while total < self.max_batch and item.shareable():   # coalesce what is already queued (or arrives within max_wait_s)
                try:
                    nxt = self._q.get(timeout=self.max_wait_s) if self.max_wait_s > 0 else self._q.get_nowait()
                except queue.Empty:
                    break
                if nxt is None or isinstance(nxt, tuple) or nxt.key() != item.key() or \
                        total + nxt.n > self.max_batch or (nxt.control is not None and not self.mixed_batches):
                    pending = nxt                   # order is preserved: it starts the next round
                    if nxt is None:
                        pending = None
                        self._q.put(None)
                    break
                batch.append(nxt)
                total += nxt.n
            try:
                outs = self._generate(batch)
                for r, o in zip(batch, outs):
                    r.future.set_result(o)
            except BaseException as e:   # noqa: BLE001 -- delivered to the callers, the worker keeps serving
                if len(batch) == 1:
                    if not batch[0].future.done():
                        batch[0].future.set_exception(e)
                    continue
                # a coalesced batch failed: run its requests one by one so that only the one that causes the error
                # receives it (the others would otherwise fail with somebody else's exception)
                for r in batch:
                    if r.future.done():
                        continue
                    try:
                        r.future.set_result(self._generate([r])[0])
                    except BaseException as e1:   # noqa: BLE001
                        r.future.set_exception(e1)

    def _control(self, item):
        op, a, b, f = item
        try:
            if op == "load":
                from . import weights_io
                fn = {"ctx": weights_io.load_ctx, "diffuser": weights_io.load_diffuser, "ctl": weights_io.load_ctl}[a]
                f.set_result(fn(self.net, b))
            else:
                f.set_result(a(self.net))
        except BaseException as e:   # noqa: BLE001
            f.set_exception(e)

    def _hint(self, r):
        """the hint of one request: its control picture as given, or (control_preprocess) its Canny edges"""
        return self.pipe.control_hint(r.control, r.height, r.width, r.control_preprocess, r.control_thresholds or (100, 200))

    @torch.no_grad()
    def _generate(self, batch):
        """one DDIM batch for a list of compatible requests; returns one image tensor per request"""
        from .hip.ops import DEVICE_LOCK
        r0 = batch[0]
        dev = self.net.device
        with DEVICE_LOCK:
            if float(r0.eta) != 0.0 and not r0.device_noise:   # runs alone (shareable()): its noise stream is a function
                torch.manual_seed(r0.seed)                      # of ITS seed only
            conds, xts, unconds, keys, masks, x0s, biases, ubiases, tables, rmaps = [], [], [], [], [], [], [], [], [], []
            for r in batch:
                if r.regional is not None:          # regional: ITS tokens, ITS table and ITS map (of its own size) per sample
                    c, z, tab = self.pipe.encode_regions(r.image, r.regional[1], r.n)
                    tables.append(tab)
                    rmaps.extend([r.regional[0]] * r.n)
                elif r.weights is not None:           # several references: ITS tokens and ITS row of logits
                    c, z, kb = self.pipe.encode_references(r.image, r.weights, r.n)
                    biases.append(kb)
                else:
                    img = self.pipe.ingest(r.image) if image_io.wants_ingest(r.image) else r.image.to(dev)
                    c, z = self.pipe.encode_reference(img, r.n)
                conds.append(c)
                unconds.append(z if r.uncond is None else r.uncond.to(dev).to(c.dtype).expand(r.n, -1, -1))
                keys.append(shard_noise_keys(r.n, r.seed, 0, 1))                # each request keeps ITS noise keys (seed, j)
                if r.init is None:
                    xts.append(shard_xT(r.n, r.height, r.width, r.seed, 0, 1))  # ... and ITS x_T stream
                elif r.mask is None:                                            # ... or ITS picture, noised under ITS keys
                    xts.append(self.pipe.init_latent(r.init, r.height, r.width, r.steps, r.strength, keys[-1])[0])
                else:                                                           # ... and ITS mask over ITS clean latent
                    x_t, _, x0 = self.pipe.init_latent(r.init, r.height, r.width, r.steps, r.strength, keys[-1], want_x0=True)
                    xts.append(x_t)
                    x0s.append(x0)
                    masks.append(self.pipe.mask_grid(r.mask, r.height, r.width)[:1].expand(r.n, -1, -1))
            if r0.weights is not None and r0.regional is None:
                # contexts of different lengths: padded to the longest of the batch with zero tokens at -inf
                nk = max(int(t.shape[1]) for t in conds + unconds)      # (an uncond longer than every mix is padded to as well)
                for i, (c, u, kb) in enumerate(zip(conds, unconds, biases)):
                    conds[i], biases[i] = self.pipe.pad_context(c, kb, nk)
                    ub = torch.zeros((u.shape[0], u.shape[1]), dtype=torch.float32, device=u.device)
                    unconds[i], ub = self.pipe.pad_context(u, ub, nk)
                    ubiases.append(ub)
            cond, uncond, xT = torch.cat(conds), torch.cat(unconds), torch.cat(xts).to(dev)
            c_info = {'type': 'image', 'conditioning': cond, 'unconditional_conditioning': uncond,
                      'unconditional_guidance_scale': r0.scale}
            if r0.regional is not None:             # (equal numbers of references: the key says so, nothing to pad)
                c_info['region_bias'], c_info['region_map'] = torch.cat(tables), rmaps
            elif r0.weights is not None:
                c_info['key_bias'] = torch.cat(biases)
                if any(r.uncond is not None for r in batch):
                    c_info['unconditional_key_bias'] = torch.cat(ubiases)
            per_sample = bool(r0.mixed) and float(r0.scale) != 1.0    # the scale-1 key keeps the batch without CFG
            if per_sample:                                            # fp32 [N]: r.scale for each of r's samples, batch order
                c_info['unconditional_guidance_scale'] = torch.tensor(
                    [float(r.scale) for r in batch for _ in range(r.n)], dtype=torch.float32)
            if r0.control is not None and r0.mixed:
                # one hint per sample [N,3,H,W]: every request's picture is ingested on its own (uint8 pictures may
                # differ in source size) and repeated over the request's samples
                hints = [self._hint(r).expand(r.n, -1, -1, -1) for r in batch]
                c_info['control'] = torch.cat(hints)
            elif r0.control is not None:
                c_info['control'] = self._hint(r0)
            if r0.ctl is not None:      # each sample its own rows of the table, batch order (layers, steps, cond_only: the key)
                from . import control as control_lib
                strengths = [float(v) for r in batch for v in r.ctl[0]]
                tab = control_lib.scale_table(strengths, r0.ctl[1], len(strengths), 2 if per_sample or float(r0.scale) != 1.0 else 1,
                                              r0.ctl[3])
                c_info['control_scale'], c_info['control_steps'] = torch.from_numpy(tab).to(dev), r0.ctl[2]
            if r0.rescale is not None:  # each sample its own phi, batch order ("has rescale" is the key)
                import numpy as np
                c_info['guidance_rescale'] = torch.from_numpy(np.concatenate([r.rescale for r in batch]))
            x_info = {'type': 'image', 'xt': xT}
            if r0.init is not None:
                x_info['xt_steps'] = r0.init_k       # equal over the batch: part of the key
            if r0.device_noise:
                x_info['noise_key'] = torch.cat(keys).to(dev)
            if r0.mask is not None:                  # masks stacked to [B, h, w]: one per sample
                x_info.update(mask=torch.cat(masks).contiguous(), x0_keep=torch.cat(x0s), keep_key=torch.cat(keys).to(dev))
            how = {} if r0.solver in (None, 'ddim') else {'solver': r0.solver}
            x, _ = self.pipe.sampler.sample(steps=r0.steps, shape=list(xT.shape), x_info=x_info, c_info=c_info,
                                            eta=r0.eta, verbose=False, **how)
            img = self.net.vae_decode(x, 'image', out_uint8=True) if r0.as_uint8 else self.net.vae_decode(x, 'image')
            self.batches.append(int(xT.shape[0]))
        outs, off = [], 0
        for r in batch:
            o = img[off:off + r.n]
            if r.composite:                          # each request with its own picture and mask
                o = self.pipe.composite(o.contiguous(), r.init, r.mask, r.height, r.width)
            outs.append(o)
            off += r.n
        return outs
