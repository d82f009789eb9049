#!/usr/bin/env python
"""Time ControlNet strength (lib/control.py) -- synthetic weights, like bench.py.

  --what request   whole requests (512 x 512, batch 4, 50 steps, graphed) through PromptFreePipeline.generate on the composite
                   with a ControlNet, alternated round by round in one process:
                     control           the plain control request (kernels and graph of the parent commit)
                     control_0.7       control_scale=0.7 over the full window: 13 scaled adds in place of 13 plain ones
                     window_0.5        control_window=(0, 0.5): the ControlNet on the first half of the steps
                     window_0.25       control_window=(0, 0.25)
                     uncontrolled      the same request without `control`
                   One line: median / min / max per variant, the spread of the plain request's own rounds, and for each
                   window the share of the gap (control - uncontrolled) it recovers next to the share of steps it releases.
  --what kernel    pfd_add_scaled_rows_f16 next to pfd_add_f16 on the same tensors, B 8 at 64 x 64 x 320, alternated: median
                   time of each launch, the spread of the medians over the rounds, and the scaled launch with the
                   unconditional half at scale 0 (control_cond_only).

    python tools/bench_control.py --what request|kernel [--rounds 5] [--iters 200] [--height 512 --width 512 --batch 4 --ddim-steps 50]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "prompt-free-diffusion_amd"))


def bench_requests(a):
    os.environ.setdefault("PFD_QUIET", "1")
    from lib.pipeline import PromptFreePipeline, build_model
    net = build_model('pfd_seecoder_with_controlnet', device='cuda', fp16=True)
    H, W, n = a.height, a.width, a.batch
    g = torch.Generator().manual_seed(0)
    image = torch.rand((1, 3, H, W), generator=g)
    control = torch.rand((1, 3, H, W), generator=g)
    pipe = PromptFreePipeline(net)
    pipe.enable_graph(True)
    gen = lambda **kw: pipe.generate(image, n, H, W, steps=a.ddim_steps, scale=2.0, seed=20, **kw)[0]      # noqa: E731
    variants = [("control", lambda: gen(control=control)),
                ("control_0.7", lambda: gen(control=control, control_scale=0.7)),
                ("window_0.5", lambda: gen(control=control, control_window=(0.0, 0.5))),
                ("window_0.25", lambda: gen(control=control, control_window=(0.0, 0.25))),
                ("uncontrolled", lambda: gen())]
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
    full, none = res["control"]["median_ms"], res["uncontrolled"]["median_ms"]
    res["control_spread_ms"] = round(res["control"]["max_ms"] - res["control"]["min_ms"], 1)
    res["scaled_minus_plain_ms"] = round(res["control_0.7"]["median_ms"] - full, 1)
    for name, released in (("window_0.5", 0.5), ("window_0.25", 0.75)):
        res[name]["gap_recovered"] = round((full - res[name]["median_ms"]) / (full - none), 4) if full != none else None
        res[name]["steps_released"] = released
    print(json.dumps({"what": "request", "shape": [H, W, n, a.ddim_steps], "graphs": len(pipe.sampler._graphs), "result": res}),
          flush=True)


def bench_kernel(a):
    from lib.hip import ops
    B, shape = 8, (8, 64, 64, 320)
    g = torch.Generator().manual_seed(0)
    x = torch.randn(shape, generator=g).half().cuda()
    r = torch.randn(shape, generator=g).half().cuda()
    out = torch.empty_like(x)
    tab = torch.full((B, 13), 0.7, dtype=torch.float32, device="cuda")
    half = tab.clone()
    half[:B // 2] = 0.0
    runs = {"pfd_add_f16": lambda: ops.add(x, r, out=out),
            "pfd_add_scaled_rows_f16": lambda: ops.add_scaled_rows(x, r, tab[:, 3], out=out),
            "pfd_add_scaled_rows_f16, half the samples at 0": lambda: ops.add_scaled_rows(x, r, half[:, 3], out=out)}
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
    mb = 3 * x.numel() * 2 / 1e6
    res = {n: dict(us=round(statistics.median(v), 2), spread_us=round(max(v) - min(v), 2)) for n, v in med.items()}
    res["ratio"] = round(res["pfd_add_scaled_rows_f16"]["us"] / res["pfd_add_f16"]["us"], 4)
    print(json.dumps(dict(what="kernel", shape=list(shape), mbytes_moved=round(mb, 1), **res)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=("kernel", "request"), default="kernel")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--ddim-steps", type=int, default=50)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    return bench_requests(a) if a.what == "request" else bench_kernel(a)


if __name__ == "__main__":
    main()
