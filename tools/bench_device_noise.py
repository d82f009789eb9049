#!/usr/bin/env python
"""Time one request shape through PromptFreePipeline at eta > 0 on its three paths -- the global-generator noise
(eager: it cannot be captured), the seeded on-device noise eager, and the seeded on-device noise replayed as a
hipGraph -- next to the eta = 0 graphed request the last one is expected to match.  Synthetic weights, like bench.py.

    python tools/bench_device_noise.py [--batch 4 --height 512 --width 512 --ddim-steps 50 --steps 4 --warmup 1]

--kernels: instead, launch the step kernels alone at [batch, 4, height/8, width/8] (a profiler reads the times):
pfd_cfg_ddim_step_rng against torch.randn + pfd_cfg_ddim_step.  Prints one JSON line."""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "prompt-free-diffusion_amd"))
os.environ.setdefault("PFD_QUIET", "1")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--ddim-steps", type=int, default=50)
    ap.add_argument("--eta", type=float, default=0.5)
    ap.add_argument("--steps", type=int, default=4, help="timed requests per path")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--kernels", action="store_true")
    args = ap.parse_args()
    import torch
    from lib.hip import ops
    torch.cuda.set_device(0)

    if args.kernels:
        B, h, w = args.batch, args.height // 8, args.width // 8
        g = torch.Generator().manual_seed(0)
        eps = torch.randn((2 * B, h, w, 4), generator=g).half().cuda()
        x = torch.randn((B, 4, h, w), generator=g).cuda()
        coef = torch.tensor([0.4, 0.6, 0.1, 0.6 ** 0.5, 2.0], device='cuda')
        key = torch.tensor([[20, j] for j in range(B)], dtype=torch.int64, device='cuda')
        for i in range(args.warmup + args.steps):
            ops.cfg_ddim_step(eps, 2, x, coef, noise_key=key, step=i, noise_mul=1.0, rep=1)
            ops.cfg_ddim_step(eps, 2, x, coef, noise=torch.randn_like(x), rep=1)
            ops.philox_normal(key, i, 4 * h * w)
        torch.cuda.synchronize()
        print(json.dumps({"kernels": "launched", "shape": [B, 4, h, w], "launches_each": args.warmup + args.steps}))
        return

    from lib.pipeline import PromptFreePipeline, build_model
    net = build_model('pfd_seecoder', device='cuda', fp16=True)
    image = torch.rand((1, 3, args.height, args.width), generator=torch.Generator().manual_seed(0))

    def timed(graph, eta, device_noise):
        pipe = PromptFreePipeline(net)
        pipe.enable_graph(True)                  # context encode and VAE decode replay as graphs on every path
        pipe.sampler.enable_graph(graph)         # the DDIM loop: a graph only where asked (and capturable)
        ms = []
        for i in range(args.warmup + args.steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pipe.generate(image, args.batch, args.height, args.width, steps=args.ddim_steps, scale=2.0, eta=eta,
                          seed=20 + i, device_noise=device_noise)
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        ms = ms[args.warmup:]
        return {"min_ms": round(min(ms), 2), "median_ms": round(sorted(ms)[len(ms) // 2], 2), "all_ms": [round(v, 2) for v in ms]}

    out = {"shape": [args.batch, args.height, args.width, args.ddim_steps], "eta": args.eta}
    out["eta0_graphed"] = timed(True, 0.0, False)
    out["global_generator_eager"] = timed(True, args.eta, False)       # graph requested: the sampler declines it
    out["device_noise_eager"] = timed(False, args.eta, True)
    out["device_noise_graphed"] = timed(True, args.eta, True)
    out["eta0_graphed_again"] = timed(True, 0.0, False)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
