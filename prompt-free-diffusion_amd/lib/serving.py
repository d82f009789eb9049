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
from .pipeline import PromptFreePipeline, check_request
from .pipeline import Request as _Request
from .pipeline import shard_xT      # handed to `assemble` by `_generate`: replacing serving.shard_xT replaces the server's x_T draw


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
        """The arguments are those of PromptFreePipeline.generate, one request of n_samples samples; its docstring describes
        them.  Here only what differs on the server:
        height, width: multiples of 64 (app.py:226-227); n_samples in [1, max_batch]; steps >= 1; scale: one number.
        image: [1,3,h,w] in [0,1] or a uint8 picture, at least 32 a side either way; no picture per sample.  The request
        carries the bytes of a uint8 picture and the worker converts them on the device.
        control: a float [1,3,height,width] or a uint8 picture of any size; uncond: a float [1,148,768]; mask: one per request.
        There is no init_posterior ('sample'), timings or decode=False; as_uint8 is the default.
        Which requests share a batch (the module docstring): equal output size, steps, solver, eta, noise kind, output kind,
        control / uncond kind; img2img and masked requests of equal k (masked ones with masked ones, equal in composite) --
        each with its own picture, mask and keys; image_weights requests with each other whatever their numbers of references
        (contexts padded to the longest of the batch); regional requests of equal numbers of regions and references, each
        with its own map -- an uncond is not taken with regions here; strength arguments off their defaults with equal layer
        weights, controlled steps and cond_only; guidance_rescale with guidance_rescale, whatever the phi.  A request that
        comes to the plain one (one reference left, nothing left of the control, phi 0 or scale 1) is served as the plain one.
        -> Future of uint8 [n,H,W,3] (as_uint8) or float [n,3,H,W] images"""
        if self._stop:
            raise RuntimeError("server is closed")
        # everything a coalesced batch would first touch inside _generate is checked HERE, on the caller's thread: a
        # malformed tensor must fail its own request, not the batch it was merged into.  First what the server is stricter
        # in than generate, then the checks of every request, then what is stricter in the references left.
        if height % 64 or width % 64:
            raise ValueError("output size must be a multiple of 64 (app.py:226-227)")
        if n_samples < 1 or n_samples > self.max_batch:
            raise ValueError(f"n_samples must be in [1, {self.max_batch}]")
        if steps < 1:
            raise ValueError("steps must be >= 1")
        float(scale)                                # one number per request (a vector is generate's): TypeError
        if uncond is not None and not (torch.is_tensor(uncond) and uncond.is_floating_point() and
                                       tuple(uncond.shape) == (1, 148, 768)):
            raise ValueError("uncond must be a float tensor [1, 148, 768]")
        if control is not None and not image_io.wants_ingest(control) and not (
                control.is_floating_point() and tuple(control.shape) == (1, 3, int(height), int(width))):
            raise ValueError(f"control must be a float tensor [1, 3, {height}, {width}] or a uint8 picture [h, w, 3]")
        if mask is not None:                        # one mask per request (generate takes one per sample too)
            image_io.check_mask(mask, init, int(height), int(width), composite, as_uint8, n=1)
            if float(eta) != 0.0 and not device_noise:      # (the server's own, shorter, words for check_request's refusal)
                raise ValueError("a masked request with eta > 0 needs device_noise=True")
        r = check_request(
            image=image, n=n_samples, height=height, width=width, steps=steps, scale=scale, eta=eta, seed=seed, control=control,
            uncond=uncond, as_uint8=as_uint8, device_noise=device_noise, solver=solver, control_preprocess=control_preprocess,
            control_thresholds=control_thresholds, init=init, strength=strength, mask=mask, composite=composite,
            image_weights=image_weights, regions=regions, region_weights=region_weights, control_scale=control_scale,
            control_layer_scales=control_layer_scales, control_window=control_window, control_cond_only=control_cond_only,
            guidance_rescale=guidance_rescale, num_timesteps=lambda: getattr(self.net, 'num_timesteps', 1000))
        if r.regional is not None and uncond is not None:
            raise ValueError("a regional request takes no uncond on the server (PromptFreePipeline.generate does)")
        for ref in r.image if r.weights is not None else [r.image]:
            if not torch.is_tensor(ref) or ref.dtype == torch.uint8:
                continue                            # a uint8 picture: checked, at least 32 a side
            if r.weights is not None and min(ref.shape[2:]) < 32:
                raise ValueError("a reference picture must be at least 32 a side")
            if not (ref.dim() == 4 and ref.shape[0] == 1 and ref.shape[1] == 3 and ref.is_floating_point() and
                    min(ref.shape[2:]) >= 32):
                raise ValueError("image must be a float tensor [1, 3, h, w] in [0, 1] or a uint8 picture [h, w, 3]")
        r.future, r.mixed = Future(), self.mixed_batches or None
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

    @torch.no_grad()
    def _generate(self, batch):
        """one DDIM batch for a list of compatible requests; returns one image tensor per request"""
        from .hip.ops import DEVICE_LOCK
        r0 = batch[0]
        with DEVICE_LOCK:
            if float(r0.eta) != 0.0 and not r0.device_noise:   # runs alone (shareable()): its noise stream is a function
                torch.manual_seed(r0.seed)                      # of ITS seed only
            x_info, c_info, shape = self.pipe.assemble([(r, 0, r.n) for r in batch], coalesced=True, draw_xT=shard_xT)
            how = {} if r0.solver in (None, 'ddim') else {'solver': r0.solver}
            x, _ = self.pipe.sampler.sample(steps=r0.steps, shape=shape, x_info=x_info, c_info=c_info, eta=r0.eta,
                                            verbose=False, **how)
            img = self.net.vae_decode(x, 'image', out_uint8=True) if r0.as_uint8 else self.net.vae_decode(x, 'image')
            self.batches.append(int(shape[0]))
        outs, off = [], 0
        for r in batch:
            o = img[off:off + r.n]
            if r.composite:                          # each request with its own picture and mask
                o = self.pipe.composite(o.contiguous(), r.init, r.mask, r.height, r.width)
            outs.append(o)
            off += r.n
        return outs
