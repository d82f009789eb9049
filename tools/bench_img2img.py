#!/usr/bin/env python
"""Time the img2img start and the requests behind it at one output size (default 512x512).  Synthetic weights, like
bench.py; device events around work on one stream, every shape warmed up first, the compared paths alternated.

    python tools/bench_img2img.py [--batch 2 --height 512 --width 512 --ddim-steps 50 --steps 4 --warmup 1 --reps 50]

  encode     the VAE encoder stage (picture -> f16 NHWC moments), eager and as a replayed hipGraph, next to the VAE
             decode stage of the same size (graphed);
  start      pfd_latent_start (one launch from the NHWC moments) against the torch composition it replaces -- to_nchw,
             chunk, clamp, exp, two randn, the multiply-adds -- on the same moments, `reps` calls each, alternated;
  requests   a `ddim-steps`-step request at strengths 0.3 / 0.5 / 0.75 / 1.0 against generate without init, all graphed,
             with the stage timings generate reports.
Prints one JSON line.  A run without a GPU fails: nothing here is a CPU number."""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "prompt-free-diffusion_amd"))
os.environ.setdefault("PFD_QUIET", "1")


def _stats(ms):
    ms = sorted(ms)
    return {"min_ms": round(ms[0], 4), "median_ms": round(ms[len(ms) // 2], 4), "max_ms": round(ms[-1], 4), "n": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=2)
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--ddim-steps", type=int, default=50)
    ap.add_argument("--steps", type=int, default=4, help="timed requests per path")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=50, help="timed calls of the stage / kernel measurements")
    ap.add_argument("--skip-requests", action="store_true")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_img2img.py measures on the GPU only"
    from lib import img2img
    from lib.hip import ops
    from lib.pipeline import PromptFreePipeline, build_model
    torch.cuda.set_device(0)
    net = build_model('pfd_seecoder', device='cuda', fp16=True)
    H, W, B = args.height, args.width, args.batch
    g = torch.Generator().manual_seed(0)
    image = torch.rand((1, 3, H, W), generator=g)
    init_u8 = (torch.rand((H + 88, W + 56, 3), generator=g) * 255).to(torch.uint8)       # another size: the resize is part of the start
    out = {"shape": [B, H, W, args.ddim_steps]}

    def events(fn, n):
        """device time of n calls of fn, one event pair each"""
        ms = []
        for _ in range(n):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        return ms

    # ---- the encode stage -------------------------------------------------------------------------------------------
    pipe = PromptFreePipeline(net)
    pipe.enable_graph(True)
    pic = ops.image_from_u8(init_u8.cuda()[None], (H, W), layout='nhwc')
    z = torch.randn((1, 4, H // 8, W // 8), generator=g).cuda()
    eager_enc = lambda: net.vae_encode_moments(pic, 'image')       # noqa: E731
    graph_enc = lambda: pipe._enc_stage(pic)                       # noqa: E731
    graph_dec = lambda: pipe._vae_stage(z)                         # noqa: E731
    for fn in (eager_enc, graph_enc, graph_dec):
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    t = {"encode_eager": [], "encode_graphed": [], "decode_graphed": []}
    for _ in range(max(1, args.reps // 5)):                         # alternated
        t["encode_eager"] += events(eager_enc, 1)
        t["encode_graphed"] += events(graph_enc, 1)
        t["decode_graphed"] += events(graph_dec, 1)
    out["encode"] = {k: _stats(v) for k, v in t.items()}
    out["encode"]["resize_u8_to_nhwc"] = _stats(events(
        lambda: ops.image_from_u8(init_u8.cuda()[None], (H, W), layout='nhwc'), max(1, args.reps // 5)))

    # which kernels the encoder's launches take at this size, next to the decoder's: the library's per-bucket event
    # timing (eager launches only; buckets 0-7 are the narrow gemm_conv_kernel family, behind the wide-tile dispatcher)
    from lib.hip import binding

    def buckets(fn):
        binding.prof_enable(True)
        fn()
        torch.cuda.synchronize()
        rows = [dict(name=r["name"], launches=r["launches"], ms=round(r["ms"], 4)) for r in binding.prof_read()]
        binding.prof_enable(False)
        return rows

    out["buckets"] = {"encode": buckets(eager_enc), "decode": buckets(lambda: net.vae_decode(z, 'image'))}

    # ---- the start kernel against the torch composition ----------------------------------------------------------------
    moments = eager_enc()
    key = torch.tensor([[20, j] for j in range(B)], dtype=torch.int64, device='cuda')
    sf, a_t = 0.18215, 0.4375
    sq_at, sq_1mat = a_t ** 0.5, (1 - a_t) ** 0.5

    def fused():
        return ops.latent_start(moments, key, sf, a_t)

    def composed():
        m = ops.to_nchw(moments, torch.float32)
        mean, logvar = torch.chunk(m, 2, dim=1)
        std = torch.exp(0.5 * torch.clamp(logvar, -30.0, 20.0))
        x0 = sf * (mean + std * torch.randn((B,) + tuple(mean.shape[1:]), device='cuda'))
        return sq_at * x0 + sq_1mat * torch.randn_like(x0)

    for _ in range(3):
        fused(), composed()
    torch.cuda.synchronize()
    t = {"pfd_latent_start": [], "torch_composition": []}
    for _ in range(args.reps):
        t["pfd_latent_start"] += events(fused, 1)
        t["torch_composition"] += events(composed, 1)
    out["start"] = {k: _stats(v) for k, v in t.items()}
    # one event pair around `reps` back-to-back calls: the per-call figure without the event's own cost
    for name, fn in (("pfd_latent_start", fused), ("torch_composition", composed)):
        out["start"][name]["back_to_back_ms_per_call"] = round(events(lambda: [fn() for _ in range(args.reps)], 1)[0] / args.reps, 5)

    # ---- whole requests --------------------------------------------------------------------------------------------------
    if not args.skip_requests:
        def request(**kw):
            ms, stages = [], []
            for i in range(args.warmup + args.steps):
                tm = {}
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                pipe.generate(image, B, H, W, steps=args.ddim_steps, scale=2.0, seed=20 + i, timings=tm, **kw)
                torch.cuda.synchronize()
                ms.append((time.perf_counter() - t0) * 1e3)
                stages.append(tm)
            ms, stages = ms[args.warmup:], stages[args.warmup:]
            res = _stats(ms)
            for k in stages[0]:
                res[k] = round(sorted(s[k] for s in stages)[len(stages) // 2], 3)
            return res

        out["requests"] = {"no_init": request()}
        for s in (0.3, 0.5, 0.75, 1.0):
            out["requests"][f"strength_{s}"] = dict(request(init=init_u8, strength=s), k=img2img.start_steps(args.ddim_steps, s))
        out["requests"]["no_init_again"] = request()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
