#!/usr/bin/env python
"""Time what PromptFreeServer(mixed_batches=True) is for, through the public `submit` API only: four one-picture requests
queued together (the worker is held until all four are in) that differ
  (a) in guidance scale, or
  (b) in ControlNet control picture,
with the flag off (one batch per scale value / per control request) and on (one batch).  Per round: wall time from
releasing the worker to the last result, `srv.batches`, and the number of captured DDIM graphs.  The rounds are: four
scales, the same four again (every graph is there), four other scales (flag off: four more captures).  Synthetic
weights, like bench.py.

    python tools/bench_mixed_batches.py [--height 512 --width 512 --ddim-steps 50 --modes off,on --cases scale,control]

A tree without the flag (an older commit) is measured with `--modes off`.  Prints one JSON line."""
import argparse
import json
import os
import sys
import threading
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "prompt-free-diffusion_amd"))
os.environ.setdefault("PFD_QUIET", "1")

ROUNDS = ([1.5, 2.0, 2.5, 3.0], [1.5, 2.0, 2.5, 3.0], [3.5, 4.0, 4.5, 5.0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--height", type=int, default=512)
    ap.add_argument("--width", type=int, default=512)
    ap.add_argument("--ddim-steps", type=int, default=50)
    ap.add_argument("--modes", default="off,on")
    ap.add_argument("--cases", default="scale,control")
    args = ap.parse_args()
    import torch
    from lib.pipeline import build_model
    from lib.serving import PromptFreeServer
    torch.cuda.set_device(0)
    H, W = args.height, args.width
    net = build_model('pfd_seecoder_with_controlnet', device='cuda', fp16=True)
    g = torch.Generator().manual_seed(0)
    images = [torch.rand((1, 3, H, W), generator=g) for _ in range(4)]
    controls = [torch.rand((1, 3, H, W), generator=g) for _ in range(4)]

    def run(case, mixed):
        srv = PromptFreeServer(net, use_graph=True, max_batch=8, **({"mixed_batches": True} if mixed else {}))
        rounds = []
        try:
            for scales in ROUNDS:
                gate = threading.Event()
                srv.call(lambda n: gate.wait(600))
                futs = []
                for i in range(4):
                    kw = dict(scale=scales[i]) if case == "scale" else dict(scale=2.0, control=controls[i])
                    futs.append(srv.submit(images[i], 1, H, W, steps=args.ddim_steps, seed=20 + i, **kw))
                before = len(srv.batches)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                gate.set()
                for f in futs:
                    f.result(1200)
                torch.cuda.synchronize()
                rounds.append({"wall_ms": round((time.perf_counter() - t0) * 1e3, 1), "batches": srv.batches[before:],
                               "graphs": len(srv.pipe.sampler._graphs)})
        finally:
            srv.close()
        return rounds

    out = {"shape": [H, W, args.ddim_steps], "rounds": "four requests; the same again; four other scales (scale case)"}
    for case in args.cases.split(","):
        for mode in args.modes.split(","):
            out[f"{case}_{mode}"] = run(case, mode == "on")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
