#!/usr/bin/env python
"""Time one request shape through PromptFreePipeline with the DDIM sampler and with DPM-Solver++(2M) at fewer steps,
loop graphed: `ddim` at 50 steps next to `dpmpp_2m` at 20, 25 and 50, the configurations alternating inside one process.
Synthetic weights, like bench.py.  Prints one JSON line.

    python tools/bench_sampler.py [--batch 4 --height 512 --width 512 --rounds 4 --warmup 1]

--kernels: instead, time the step kernels alone at [batch, 4, height/8, width/8] with device events around runs of
back-to-back launches, alternating: pfd_cfg_dpmpp_step (with and without history) against pfd_cfg_ddim_step.  Eager
launches measure the launch rate more than the kernel; for kernel times run it under `rocprofv3 --kernel-trace --stats`,
once per `--arm` (the two forms of the new kernel are one kernel name), and read tools/rocpd_stats.py.

--convergence: instead, at 64 x 64 (8 x 8 latents) on the same random-weight net, the distance of the final latents of
`ddim` and `dpmpp_2m` at 10, 20 and 50 steps to a 250-step DDIM run from the same x_T (fp32 latents, eager)."""
import argparse
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "prompt-free-diffusion_amd"))
os.environ.setdefault("PFD_QUIET", "1")

CONFIGS = [("ddim", 50), ("dpmpp_2m", 20), ("dpmpp_2m", 25), ("dpmpp_2m", 50)]


def _stats(ms):
    return {"min_ms": round(min(ms), 3), "median_ms": round(sorted(ms)[len(ms) // 2], 3), "all_ms": [round(v, 3) for v in ms]}


def kernels(args, torch):
    from lib import solver
    from lib.hip import ops
    B, h, w = args.batch, args.height // 8, args.width // 8
    g = torch.Generator().manual_seed(0)
    eps = torch.randn((2 * B, h, w, 4), generator=g).half().cuda()
    x = torch.randn((B, 4, h, w), generator=g).cuda()
    hist = torch.randn((B, 4, h, w), generator=g).cuda()
    ddim = torch.tensor([0.4, 0.6, 0.0, 0.6 ** 0.5, 2.0], device='cuda')
    row = torch.tensor(solver.dpmpp_2m_table([0.2, 0.4, 0.6], [0.1, 0.2, 0.4], 2.0)[1], dtype=torch.float32, device='cuda')
    arms = {"cfg_ddim_step": lambda: ops.cfg_ddim_step(eps, 2, x, ddim, rep=1),
            "cfg_dpmpp_step_first_order": lambda: ops.cfg_dpmpp_step(eps, 2, x, row, None, want_next=True, rep=1),
            "cfg_dpmpp_step_history": lambda: ops.cfg_dpmpp_step(eps, 2, x, row, hist, want_next=True, rep=1)}
    if args.arm:                     # under a profiler the two forms of the new kernel share a name: one run each
        arms = {k: v for k, v in arms.items() if k in ("cfg_ddim_step", args.arm)}
    us = {k: [] for k in arms}
    for r in range(args.warmup + args.rounds):
        for name, fn in arms.items():
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t0.record()
            for _ in range(args.launches):
                fn()
            t1.record()
            torch.cuda.synchronize()
            if r >= args.warmup:
                us[name].append(t0.elapsed_time(t1) * 1e3 / args.launches)
    return {"kernels_us_per_launch": {k: {"min": round(min(v), 3), "median": round(sorted(v)[len(v) // 2], 3)}
                                      for k, v in us.items()},
            "shape": [B, 4, h, w], "launches_per_round": args.launches, "rounds": args.rounds,
            "note": "back-to-back eager launches between two device events: launch rate and kernel time together"}


def convergence(args, torch, net):
    from lib.model_zoo.ddim import DDIMSampler
    n = 3
    xT = torch.randn([n, 4, 8, 8], generator=torch.Generator().manual_seed(1)).cuda()
    c = torch.randn([n, 148, 768], generator=torch.Generator().manual_seed(2)).cuda().half().float()   # fp32: fp32 latents out
    s = DDIMSampler(net)

    def run(solver, steps):
        c_info = {'type': 'image', 'conditioning': c, 'unconditional_conditioning': torch.zeros_like(c),
                  'unconditional_guidance_scale': 2.0}
        how = {} if solver == 'ddim' else {'solver': solver}
        x = s.sample(steps=steps, shape=[n, 4, 8, 8], x_info={'type': 'image', 'xt': xT.clone()}, c_info=c_info,
                     verbose=False, **how)[0].double().cpu()
        assert len(s.ddim_timesteps) == steps
        return x

    ref = run('ddim', 250)
    out = {"reference": "ddim, 250 steps", "latents": [n, 4, 8, 8], "ref_max_abs": round(float(ref.abs().max()), 4), "rows": []}
    for steps in (10, 20, 50):
        for solver in ('ddim', 'dpmpp_2m'):
            x = run(solver, steps)
            out["rows"].append({"solver": solver, "steps": steps,
                                "scaled_max_abs": float((x - ref).abs().max() / max(1.0, float(ref.abs().max()))),
                                "rel_l2": float((x - ref).norm() / ref.norm())})
    return out


def loops(args, torch, net):
    from lib.pipeline import PromptFreePipeline
    image = torch.rand((1, 3, args.height, args.width), generator=torch.Generator().manual_seed(0))
    pipe = PromptFreePipeline(net)
    pipe.enable_graph(True)          # context encode, the sampler's loop and VAE decode all replay as graphs
    total = {c: [] for c in CONFIGS}
    loop = {c: [] for c in CONFIGS}
    for r in range(args.warmup + args.rounds):
        for cfg in CONFIGS:          # alternating: one round visits every configuration
            solver, steps = cfg
            tm = {}
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pipe.generate(image, args.batch, args.height, args.width, steps=steps, scale=2.0, seed=20 + r, timings=tm,
                          solver=solver)
            torch.cuda.synchronize()
            if r >= args.warmup:
                total[cfg].append((time.perf_counter() - t0) * 1e3)
                loop[cfg].append(tm["ddim_loop_ms"])
    real = {}
    for solver, steps in CONFIGS:
        pipe.sampler.make_schedule(steps, verbose=False)
        real[(solver, steps)] = len(pipe.sampler.ddim_timesteps)
    base = min(loop[CONFIGS[0]])
    rows = []
    for cfg in CONFIGS:
        rows.append({"solver": cfg[0], "steps": cfg[1], "unet_evaluations": real[cfg], "request": _stats(total[cfg]),
                     "loop": _stats(loop[cfg]), "loop_ms_per_step": round(min(loop[cfg]) / real[cfg], 4),
                     "loop_vs_ddim50": round(min(loop[cfg]) / base, 4),
                     "images_per_s": round(args.batch / (min(total[cfg]) * 1e-3), 3)})
    return {"shape": [args.batch, args.height, args.width], "rounds": args.rounds, "rows": rows}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--rounds", type=int, default=4, help="timed rounds; one round visits every configuration")
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--launches", type=int, default=500, help="--kernels: launches between the two events")
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--arm", choices=["cfg_dpmpp_step_first_order", "cfg_dpmpp_step_history"],
                    help="--kernels: launch only this form of the new kernel next to cfg_ddim_step")
    ap.add_argument("--convergence", action="store_true")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_sampler.py measures on the GPU: none is visible")
    torch.cuda.set_device(0)
    if args.kernels:
        print(json.dumps(kernels(args, torch)))
        return
    from lib.pipeline import build_model
    net = build_model('pfd_seecoder', device='cuda', fp16=True)
    print(json.dumps(convergence(args, torch, net) if args.convergence else loops(args, torch, net)))


if __name__ == "__main__":
    main()
