#!/usr/bin/env python
"""Time regional reference mixing (lib/regions.py) -- synthetic weights, like bench.py.

  --what kernel    pfd_attention_rbias_f16 against pfd_attention_kbias_f16, alternated in one process, at the cross-attention
                   shapes of a 512 x 512 request with two references (batch 4: B = 4, Nk = 296): one line per shape with the
                   median time of each entry and the spread of the medians over the rounds.  The regional launch uses 2
                   regions, left / right, region 1 masking the first reference (the first key tiles in full).  The row with
                   B = 3 at the 64 x 64 level is a shape at which BOTH entries launch their 4-wave d = 40 build: it shows the
                   cost of the per-lane rows alone, the B = 4 row that cost plus the folded 8-wave build's absence.
  --what request   a whole request (512 x 512, batch 4, 50 steps, graphed) through PromptFreePipeline.generate: two references
                   with image_weights=[0.7, 0.3] against the same two with a left / right map and region_weights
                   [[1, 0], [0, 1]], alternated round by round.  (The image_weights request launches kernels whose code is
                   the parent commit's, tools/isa_diff.py.)

    python tools/bench_regions.py --what kernel|request [--rounds 5] [--iters 200] [--height 512 --width 512 --batch 4 --ddim-steps 50]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "prompt-free-diffusion_amd"))

# (class, B, H, Nq, Nk, D): the 64^2, 32^2, 16^2 and 8^2 levels of the UNet at 512 x 512; w8 is the per-key entry's class at 64^2
SHAPES = [("w8/w4", 4, 8, 4096, 296, 40), ("w4/w4", 3, 8, 4096, 296, 40), ("d80", 4, 8, 1024, 296, 80), ("d160", 4, 8, 256, 296, 160), ("d160", 4, 8, 64, 296, 160)]


def bench_requests(a):
    import numpy as np
    os.environ.setdefault("PFD_QUIET", "1")
    from lib.pipeline import PromptFreePipeline, build_model
    net = build_model('pfd_seecoder', device='cuda', fp16=True)
    H, W, n = a.height, a.width, a.batch
    g = torch.Generator().manual_seed(0)
    pics = [torch.rand((1, 3, H, W), generator=g) for _ in range(2)]
    m = np.zeros((H, W), dtype=np.uint8)
    m[:, W // 2:] = 1
    pipe = PromptFreePipeline(net)
    pipe.enable_graph(True)
    variants = [("image_weights_2", lambda: pipe.generate(pics, n, H, W, steps=a.ddim_steps, scale=2.0, seed=20, image_weights=[0.7, 0.3])[0]),
                ("regions_2x2", lambda: pipe.generate(pics, n, H, W, steps=a.ddim_steps, scale=2.0, seed=20, regions=m,
                                                      region_weights=[[1.0, 0.0], [0.0, 1.0]])[0])]
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
    res = {name: {"median_ms": round(statistics.median(v), 1), "min_ms": round(min(v), 1), "max_ms": round(max(v), 1)}
           for name, v in times.items()}
    res["ratio"] = round(res["regions_2x2"]["median_ms"] / res["image_weights_2"]["median_ms"], 4)
    print(json.dumps({"what": "request", "shape": [H, W, n, a.ddim_steps], "result": res}), flush=True)


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
    if a.what == "request":
        return bench_requests(a)
    from lib.hip import ops
    g = torch.Generator().manual_seed(0)
    for cls, B, H, Nq, Nk, D in SHAPES:
        C, Nkp = H * D, (Nk + 7) // 8 * 8
        q = torch.randn(B * Nq * C, generator=g).half().cuda()
        k = torch.randn(B * Nkp * C, generator=g).half().cuda()
        vt = torch.randn(C * B * Nkp, generator=g).half().cuda()
        kw = dict(ldq=C, ldk=C, ldvt=B * Nkp, q_bs=Nq * C, k_bs=Nkp * C, vt_bs=Nkp)
        kb = torch.zeros((B, Nkp), dtype=torch.float32, device="cuda")
        kb[:, Nk // 2:] = -1.2
        rb = torch.zeros((B, 2, Nkp), dtype=torch.float32, device="cuda")
        rb[:, 0, Nk // 2:] = float("-inf")
        rb[:, 1, :Nk // 2] = float("-inf")
        side = int(Nq ** 0.5)
        qr = (torch.arange(Nq) % side >= side // 2).to(torch.uint8).cuda()[None].repeat(B, 1)
        out = torch.empty((B * Nq, C), dtype=torch.float16, device="cuda")
        runs = {"kbias": lambda: ops.attention(q, k, vt, B, H, Nq, Nk, D, D ** -0.5, out=out, kbias=kb, **kw),
                "rbias": lambda: ops.attention(q, k, vt, B, H, Nq, Nk, D, D ** -0.5, out=out, rbias=rb, qregion=qr, **kw)}
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
        res["ratio"] = round(res["rbias"]["us"] / res["kbias"]["us"], 4)
        print(json.dumps(dict(cls=cls, B=B, H=H, Nq=Nq, Nk=Nk, D=D, **res)), flush=True)


if __name__ == "__main__":
    main()
