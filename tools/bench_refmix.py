#!/usr/bin/env python
"""Time several references mixed in one UNet pass (lib/refmix.py) -- synthetic weights, like bench.py.

  --what kernel    pfd_attention_kbias_f16 against pfd_attention_f16 per kernel class (w4, w8, d80, d160) at Nk = 148 / 296 /
                   444 keys (1, 2, 3 references): median microseconds of a launch, with and without the key logits, the two
                   alternated launch by launch inside one loop (they see the same clocks)
  --what request   a whole request at the benchmark shape (512 x 512, batch 4, 50 steps, graphed) through
                   PromptFreePipeline.generate for R = 1, 2, 3 references, and the same two contexts through
                   DDIMSampler.sample_multicontext (the reference's context_mixing: every context layer once per context,
                   eager -- it is not captured); the variants alternated round by round, median of the rounds.  The two
                   kinds of mixing are different functions; only their cost is compared.

    python tools/bench_refmix.py --what kernel|request [--rounds 5] [--height 512 --width 512 --batch 4 --ddim-steps 50]

Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "prompt-free-diffusion_amd"))
os.environ.setdefault("PFD_QUIET", "1")

# (class, B, H, Nq, D): the cross-attention launches of the UNet at the benchmark shape (CFG pair of batch 4 with the
# zero-context shortcut: 4 samples reach the kernel) -- 64^2 level (w8), 16^2 (d160), 32^2 (d80) -- and a small d = 40 launch (w4)
KERNEL_SHAPES = [("w8", 4, 8, 4096, 40), ("d80", 4, 8, 1024, 80), ("d160", 4, 8, 256, 160), ("w4", 1, 8, 256, 40)]


def bench_kernels(args):
    import torch
    from lib.hip import ops
    out = {}
    for cls, B, H, Nq, D in KERNEL_SHAPES:
        C = H * D
        for Nk in (148, 296, 444):
            Nkp = (Nk + 7) // 8 * 8
            g = torch.Generator().manual_seed(Nk)
            q = torch.randn(B * Nq * C, generator=g).half().cuda()
            k = torch.randn(B * Nkp * C, generator=g).half().cuda()
            vt = torch.randn(C * B * Nkp, generator=g).half().cuda()
            kb = (-4.0 * torch.rand((B, Nkp), generator=g)).cuda()
            kw = dict(ldq=C, ldk=C, ldvt=B * Nkp, q_bs=Nq * C, k_bs=Nkp * C, vt_bs=Nkp)
            o = torch.empty((B * Nq, C), dtype=torch.float16, device="cuda")
            ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(args.iters)]
            for _ in range(10):
                ops.attention(q, k, vt, B, H, Nq, Nk, D, D ** -0.5, out=o, **kw)
                ops.attention(q, k, vt, B, H, Nq, Nk, D, D ** -0.5, out=o, kbias=kb, **kw)
            for e in ev:
                e[0].record()
                ops.attention(q, k, vt, B, H, Nq, Nk, D, D ** -0.5, out=o, **kw)
                e[1].record()
                ops.attention(q, k, vt, B, H, Nq, Nk, D, D ** -0.5, out=o, kbias=kb, **kw)
                e[2].record()
            torch.cuda.synchronize()
            plain = statistics.median(e[0].elapsed_time(e[1]) for e in ev) * 1e3
            biased = statistics.median(e[1].elapsed_time(e[2]) for e in ev) * 1e3
            out[f"{cls}_q{Nq}_k{Nk}"] = {"plain_us": round(plain, 2), "kbias_us": round(biased, 2), "ratio": round(biased / plain, 4)}
    return out


def bench_requests(args):
    import torch
    from lib.model_zoo.ddim import DDIMSampler
    from lib.pipeline import PromptFreePipeline, build_model, shard_xT
    net = build_model('pfd_seecoder', device='cuda', fp16=True)
    H, W, n = args.height, args.width, args.batch
    g = torch.Generator().manual_seed(0)
    pics = [torch.rand((1, 3, H, W), generator=g) for _ in range(3)]
    weights = {1: None, 2: [0.7, 0.3], 3: [0.5, 0.3, 0.2]}
    pipe = PromptFreePipeline(net)
    pipe.enable_graph(True)
    eager = DDIMSampler(net)

    def request(R):
        img = pics[0] if R == 1 else pics[:R]
        return pipe.generate(img, n, H, W, steps=args.ddim_steps, scale=2.0, seed=20, image_weights=weights[R])[0]

    def multicontext():
        toks = [net.ctx_encode(p.cuda().half(), 'image').repeat(n, 1, 1) for p in pics[:2]]
        cl = [{'type': 'image', 'conditioning': t, 'unconditional_conditioning': torch.zeros_like(t),
               'unconditional_guidance_scale': 2.0, 'ratio': r} for t, r in zip(toks, (0.7, 0.3))]
        xT = shard_xT(n, H, W, 20, 0, 1).cuda()
        x = eager.sample_multicontext(args.ddim_steps, list(xT.shape), {'type': 'image', 'xt': xT}, cl, verbose=False)[0]
        return net.vae_decode(x, 'image')

    variants = [("R1", lambda: request(1)), ("R2", lambda: request(2)), ("R3", lambda: request(3)),
                ("multicontext_2", multicontext)]
    times = {name: [] for name, _ in variants}
    for name, fn in variants:          # captures and packs
        fn()
    torch.cuda.synchronize()
    for _ in range(args.rounds):
        for name, fn in variants:      # alternated: every variant sees every phase of the clocks
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3)
    return {name: {"median_ms": round(statistics.median(v), 1), "min_ms": round(min(v), 1), "max_ms": round(max(v), 1)}
            for name, v in times.items()}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", choices=("kernel", "request"), required=True)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--ddim-steps", type=int, default=50)
    args = ap.parse_args()
    import torch
    torch.cuda.set_device(0)
    res = bench_kernels(args) if args.what == "kernel" else bench_requests(args)
    print(json.dumps({"what": args.what, "shape": [args.height, args.width, args.batch, args.ddim_steps], "result": res}))


if __name__ == "__main__":
    main()
