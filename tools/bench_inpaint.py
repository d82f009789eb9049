#!/usr/bin/env python
"""Time masked regeneration (inpainting) next to what it is added to.  Synthetic weights, like bench.py; device events
around work on one stream, every shape warmed up first, the compared paths alternated.

    python tools/bench_inpaint.py [--batch 4 --height 512 --width 512 --ddim-steps 50 --steps 4 --warmup 1 --reps 50]

  step       pfd_cfg_step_masked against the unmasked step it stands in for (DDIM at sigma 0, seeded DDIM, DPM-Solver++
             with history) at `batch` latents of (height/8) x (width/8), `reps` calls each, alternated, and back to back;
  mask       pfd_mask_grid_u8 of a height x width uint8 mask to the latent grid and to the pixel grid;
  composite  pfd_composite_u8 of `batch` height x width pictures;
  requests   a `ddim-steps`-step masked request against the same img2img request, both graphed, alternated, with the
             stage timings generate reports.  --img2img-only times that img2img request alone and touches nothing this
             file's other sections need: it runs on a tree without the masked path (the commit before it), for the
             comparison across trees.
Prints one JSON line.  A run without a GPU fails: nothing here is a CPU number."""
import argparse
import json
import os
import sys
import time

REPO = os.environ.get("PFD_BENCH_TREE") or os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "prompt-free-diffusion_amd"))
os.environ.setdefault("PFD_QUIET", "1")


def _stats(ms):
    ms = sorted(ms)
    return {"min_ms": round(ms[0], 4), "median_ms": round(ms[len(ms) // 2], 4), "max_ms": round(ms[-1], 4), "n": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--ddim-steps", type=int, default=50)
    ap.add_argument("--strength", type=float, default=0.75)
    ap.add_argument("--steps", type=int, default=4, help="timed requests per path")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--reps", type=int, default=50, help="timed calls of the kernel measurements")
    ap.add_argument("--skip-requests", action="store_true")
    ap.add_argument("--img2img-only", action="store_true")
    args = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "bench_inpaint.py measures on the GPU only"
    from lib.hip import ops
    from lib.pipeline import PromptFreePipeline, build_model
    torch.cuda.set_device(0)
    H, W, B = args.height, args.width, args.batch
    h, w = H // 8, W // 8
    g = torch.Generator().manual_seed(0)
    out = {"shape": [B, H, W, args.ddim_steps], "tree": REPO}

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

    def compare(paths):
        """{name: fn}: warmed up, `reps` calls each with an event pair, alternated; then `reps` calls back to back"""
        for fn in paths.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        t = {k: [] for k in paths}
        for _ in range(args.reps):
            for k, fn in paths.items():
                t[k] += events(fn, 1)
        res = {k: _stats(v) for k, v in t.items()}
        for k, fn in paths.items():
            res[k]["back_to_back_ms_per_call"] = round(events(lambda: [fn() for _ in range(args.reps)], 1)[0] / args.reps, 5)
        return res

    mask_u8 = torch.zeros((H, W), dtype=torch.uint8)
    mask_u8[H // 4:3 * H // 4, W // 4:3 * W // 4] = 255
    if not args.img2img_only:
        from lib import inpaint, solver
        # ---- the step ------------------------------------------------------------------------------------------------
        eps = torch.randn((2 * B, h, w, 4), generator=g).half().cuda()
        x, x0, hist = (torch.randn((B, 4, h, w), generator=g).cuda() for _ in range(3))
        key = torch.tensor([[20, j] for j in range(B)], dtype=torch.int64, device='cuda')
        m = ops.mask_grid_u8(mask_u8.cuda(), h, w)
        a_t, a_p = 0.4375, 0.5625
        ksq, ks = (float(v) for v in inpaint.step_constants(a_p, 1))
        row = lambda sg: torch.tensor([a_t, a_p, sg, (1 - a_t) ** 0.5, 2.0], dtype=torch.float32, device='cuda')   # noqa: E731
        d0, d1 = row(0.0), row(0.3)
        dp = torch.tensor(solver.dpmpp_2m_table([0.9, a_t, 0.2], [0.99, 0.9, a_t], 2.0, 2)[1], dtype=torch.float32, device='cuda')
        common = dict(keep_key=key, step=1, x0_keep=x0, mask=m, ksq=ksq, ks=ks, want_next=True, rep=1)
        out["step"] = compare({
            "ddim_plain": lambda: ops.cfg_ddim_step(eps, 2, x, d0, want_next=True, rep=1),
            "ddim_masked": lambda: ops.cfg_step_masked(eps, 2, x, d0, solver='ddim', **common),
            "ddim_seeded_plain": lambda: ops.cfg_ddim_step(eps, 2, x, d1, want_next=True, rep=1, noise_key=key, step=1),
            "ddim_seeded_masked": lambda: ops.cfg_step_masked(eps, 2, x, d1, solver='ddim', **common),
            "dpmpp_2m_plain": lambda: ops.cfg_dpmpp_step(eps, 2, x, dp, hist, want_next=True, rep=1),
            "dpmpp_2m_masked": lambda: ops.cfg_step_masked(eps, 2, x, dp, solver='dpmpp', x0_prev=hist, **common),
        })
        n = B * 4 * h * w
        out["step"]["bytes_masked"] = 2 * n * 2 + 4 * n * 4 + n * 2 + h * w * 4      # eps pair, x / x0 in, x_out / pred out, xin, mask
        # ---- the mask ingest and the composite -----------------------------------------------------------------------------
        md = mask_u8.cuda()
        out["mask"] = compare({"to_latent_grid_f32": lambda: ops.mask_grid_u8(md, h, w),
                               "to_pixel_grid_u8": lambda: ops.mask_grid_u8(md, H, W, torch.uint8)})
        dec = (torch.rand((B, H, W, 3), generator=g) * 255).to(torch.uint8).cuda()
        ini = (torch.rand((1, H, W, 3), generator=g) * 255).to(torch.uint8).cuda()
        sel = ops.mask_grid_u8(md, H, W, torch.uint8)
        out["composite"] = compare({"composite_u8": lambda: ops.composite_u8(dec, ini, sel)})

    # ---- whole requests ----------------------------------------------------------------------------------------------------
    if not args.skip_requests:
        net = build_model('pfd_seecoder', device='cuda', fp16=True)
        pipe = PromptFreePipeline(net)
        pipe.enable_graph(True)
        image = torch.rand((1, 3, H, W), generator=g)
        init_u8 = (torch.rand((H + 88, W + 56, 3), generator=g) * 255).to(torch.uint8)
        paths = {"img2img": dict(init=init_u8, strength=args.strength)}
        if not args.img2img_only:
            paths["masked"] = dict(init=init_u8, strength=args.strength, mask=mask_u8.numpy())
            paths["masked_composite_u8"] = dict(init=init_u8.numpy(), strength=args.strength, mask=mask_u8.numpy(),
                                                composite=True, as_uint8=True)
        ms, stages = {k: [] for k in paths}, {k: [] for k in paths}
        for i in range(args.warmup + args.steps):          # alternated: every path once per round
            for k, kw in paths.items():
                tm = {}
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                pipe.generate(image, B, H, W, steps=args.ddim_steps, scale=2.0, seed=20 + i, timings=tm, **kw)
                torch.cuda.synchronize()
                if i >= args.warmup:
                    ms[k].append((time.perf_counter() - t0) * 1e3)
                    stages[k].append(tm)
        out["requests"] = {}
        for k in paths:
            res = _stats(ms[k])
            for name in stages[k][0]:
                res[name] = round(sorted(s[name] for s in stages[k])[len(stages[k]) // 2], 3)
            out["requests"][k] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
