#!/usr/bin/env python
"""Time guidance rescale (lib/guidance.py) -- synthetic weights, like bench.py.

  --what kernel    the statistics launch pfd_guidance_rescale_f32 alone at B 8, 64 x 64 x 4 and at B 2, 96 x 96 x 4, next to
                   pfd_cfg_ddim_step and pfd_cfg_step_mul on the same tensors, alternated: median time of each launch and the
                   spread of the medians over the rounds.
  --what request   whole requests (512 x 512, batch 4, 50 steps, scale 7.5, graphed) through PromptFreePipeline.generate,
                   alternated round by round in one process:
                     plain             the request without guidance_rescale (kernels and graph of the parent commit)
                     rescale_0.7       guidance_rescale=0.7: one statistics launch in front of every step
                   One line: median / min / max per variant, the spread of the plain request's own rounds and the extra cost
                   per step (the difference of the medians over the step count).
  --what all       both, each in a fresh child process under its own time limit; stops at the first that fails.

    python tools/bench_guidance.py --what kernel|request|all [--rounds 5] [--iters 200] [--height 512 --width 512 --batch 4 --ddim-steps 50]"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "prompt-free-diffusion_amd"))
LIMITS = {"kernel": 120, "request": 420}     # seconds per child of --what all


def bench_requests(a):
    os.environ.setdefault("PFD_QUIET", "1")
    from lib.pipeline import PromptFreePipeline, build_model
    net = build_model('pfd_seecoder', device='cuda', fp16=True)
    H, W, n = a.height, a.width, a.batch
    g = torch.Generator().manual_seed(0)
    image = torch.rand((1, 3, H, W), generator=g)
    pipe = PromptFreePipeline(net)
    pipe.enable_graph(True)
    gen = lambda **kw: pipe.generate(image, n, H, W, steps=a.ddim_steps, scale=7.5, seed=20, **kw)[0]      # noqa: E731
    variants = [("plain", lambda: gen()), ("rescale_0.7", lambda: gen(guidance_rescale=0.7))]
    times = {name: [] for name, _ in variants}
    for name, fn in variants:          # captures and packs
        fn()
    torch.cuda.synchronize()
    for _ in range(a.rounds):
        for name, fn in variants:      # alternated: every variant sees every phase of the clocks
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3)
    res = {name: {"median_ms": round(statistics.median(v), 1), "min_ms": round(min(v), 1), "max_ms": round(max(v), 1),
                  "images_per_s": round(n / statistics.median(v) * 1e3, 3)} for name, v in times.items()}
    res["plain_spread_ms"] = round(res["plain"]["max_ms"] - res["plain"]["min_ms"], 1)
    extra = res["rescale_0.7"]["median_ms"] - res["plain"]["median_ms"]
    res["rescale_minus_plain_ms"] = round(extra, 1)
    res["extra_us_per_step"] = round(extra * 1e3 / a.ddim_steps, 1)
    print(json.dumps({"what": "request", "shape": [H, W, n, a.ddim_steps], "graphs": len(pipe.sampler._graphs), "result": res}),
          flush=True)


def bench_kernel(a):
    from lib.hip import ops
    out = []
    for B, h in ((8, 64), (2, 96)):
        g = torch.Generator().manual_seed(0)
        eps = torch.randn((2 * B, h, h, 4), generator=g).half().cuda()
        x = torch.randn((B, 4, h, h), generator=g).cuda()
        coef = torch.tensor([0.5, 0.55, 0.0, 0.5 ** 0.5, 7.5], device="cuda")
        phi = torch.full((B,), 0.7, device="cuda")
        mul = ops.guidance_rescale(eps, coef[4:5], phi)
        runs = {"pfd_guidance_rescale_f32": lambda: ops.guidance_rescale(eps, coef[4:5], phi),
                "pfd_cfg_ddim_step": lambda: ops.cfg_ddim_step(eps, 2, x, coef, want_next=True, rep=1),
                "pfd_cfg_step_mul": lambda: ops.cfg_ddim_step(eps, 2, x, coef, want_next=True, rep=1, eps_mul=mul)}
        med = {n: [] for n in runs}
        for _ in range(a.rounds):
            for n, f in runs.items():
                for _ in range(10):
                    f()
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(a.iters + 1)]
                ev[0].record()
                for i in range(a.iters):
                    f()
                    ev[i + 1].record()
                torch.cuda.synchronize()
                med[n].append(statistics.median(ev[i].elapsed_time(ev[i + 1]) * 1e3 for i in range(a.iters)))
        res = {n: dict(us=round(statistics.median(v), 2), spread_us=round(max(v) - min(v), 2)) for n, v in med.items()}
        out.append(dict(B=B, shape=[h, h, 4], kbytes_read=round(2 * eps.numel() * 2 / 1e3, 1), **res))
    print(json.dumps(dict(what="kernel", note="event pairs around eager launches: each figure includes the launch itself",
                          cases=out)), flush=True)


def run_all(a, argv):
    """each measurement in a child of its own, under its own time limit; a child that fails or runs out of time ends the run"""
    for what in ("kernel", "request"):
        cmd = [sys.executable, os.path.abspath(__file__), "--what", what] + argv
        try:
            rc = subprocess.run(cmd, timeout=LIMITS[what]).returncode
        except subprocess.TimeoutExpired:
            print(f"bench_guidance: --what {what} exceeded {LIMITS[what]} s; stopping", file=sys.stderr)
            return 124
        if rc != 0:
            print(f"bench_guidance: --what {what} ended with {rc}; stopping", file=sys.stderr)
            return rc
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=("kernel", "request", "all"), default="kernel")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--ddim-steps", type=int, default=50)
    a = ap.parse_args()
    if a.what == "all":
        argv = ["--rounds", str(a.rounds), "--iters", str(a.iters), "--height", str(a.height), "--width", str(a.width),
                "--batch", str(a.batch), "--ddim-steps", str(a.ddim_steps)]
        sys.exit(run_all(a, argv))
    torch.cuda.set_device(0)
    return bench_requests(a) if a.what == "request" else bench_kernel(a)


if __name__ == "__main__":
    main()
