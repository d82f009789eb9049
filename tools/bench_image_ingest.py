#!/usr/bin/env python
"""Time the uint8 picture ingest on the GPU against what a client of the float interface does on the host.

  device column: np.asarray(picture) -> H2D copy of the uint8 bytes -> ops.image_from_u8 (resize + ToTensor, fp16 NCHW),
                 HIP events around copy + kernels; and the kernels alone (picture already on the device) with their
                 achieved GB/s (algorithmic bytes: every pass reads its input and writes its output once)
  host column:   Pillow `resize(BICUBIC)` + ToTensor (`/ 255`) + `.half()` + H2D copy of the float tensor
                 (app.py:232,234,244), wall clock around work that ends in a device synchronise

Warm, median of --reps after --warmup.  Needs a GPU; without Pillow the host column is left out and the file says so.
usage: bench_image_ingest.py [--reps 50] [--out DIR]   -> DIR/image_ingest_run.json, DIR/image_ingest_run.md"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "prompt-free-diffusion_amd"), os.path.join(REPO, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import make_image_golden as G  # noqa: E402

HBM_PEAK_GBS = 8000.0            # the figure bench.py --full uses
CASES = [("app_ctl", (600, 900), (512, 768)), ("full", (1000, 1500), (1536, 1024)), ("totensor_1536", (1536, 1536), (1536, 1536))]


def picture(name, hw):
    if name in G.CASES:
        return G.source(name)
    h, w = hw
    i = np.arange(h * w * 3, dtype=np.int64)
    return (((i * 2654435761) >> 13) & 255).astype(np.uint8).reshape(h, w, 3)


def algorithmic_bytes(hw, out_hw, esz=2, c=3):
    (h, w), (oh, ow) = hw, out_hw
    n = 0
    if w != ow:
        n += h * w * c + h * ow * c
    n += h * ow * c + oh * ow * c * esz
    return n


def events_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts), min(ts), max(ts)


def wall_ms(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_image_ingest needs a GPU (a CPU run gives no time)"
    from lib.hip import ops
    try:
        from PIL import Image
        import PIL
        pillow = PIL.__version__
    except ImportError:
        Image, pillow = None, None
    rows = []
    for name, hw, out_hw in CASES:
        a = picture(name, hw)
        size = None if hw == out_hw else out_hw
        on_dev = torch.from_numpy(a).cuda()

        def device_path():
            return ops.image_from_u8(torch.from_numpy(np.asarray(a)).to('cuda'), size, dtype=torch.float16)

        def kernels_only():
            return ops.image_from_u8(on_dev, size, dtype=torch.float16)

        row = dict(case=name, input=list(hw), output=list(out_hw), bytes=algorithmic_bytes(hw, out_hw))
        row["device_ms"], row["device_min"], row["device_max"] = events_ms(device_path, args.reps, args.warmup)
        row["kernels_ms"], row["kernels_min"], row["kernels_max"] = events_ms(kernels_only, args.reps, args.warmup)
        row["kernels_gbs"] = row["bytes"] / (row["kernels_ms"] * 1e-3) / 1e9
        row["hbm_frac"] = row["kernels_gbs"] / HBM_PEAK_GBS
        if Image is not None:
            im = Image.fromarray(a)

            def host_path():
                r = im if size is None else im.resize((out_hw[1], out_hw[0]), Image.Resampling.BICUBIC)
                t = torch.from_numpy(np.asarray(r)).permute(2, 0, 1)[None].float().div(255)       # ToTensor
                return t.half().to('cuda')

            row["host_ms"], row["host_min"], row["host_max"] = wall_ms(host_path, max(5, args.reps // 5), 2)
            assert torch.equal(host_path(), device_path()), name          # the two columns compute the same tensor
        rows.append(row)
        print(json.dumps(row), flush=True)
    res = dict(device=torch.cuda.get_device_name(0), pillow=pillow, omp_num_threads=os.environ.get("OMP_NUM_THREADS"),
               torch_threads=torch.get_num_threads(), reps=args.reps, rows=rows)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "image_ingest_run.json"), "w") as f:
        json.dump(res, f, indent=1)
    with open(os.path.join(args.out, "image_ingest_run.md"), "w") as f:
        f.write(f"device {res['device']}, Pillow {pillow}, OMP_NUM_THREADS {res['omp_num_threads']}, median of {args.reps} warm runs (min - max)\n\n")
        f.write("| case | in -> out | host: Pillow + /255 + .half() + H2D [ms] | device: H2D u8 + kernels [ms] | kernels alone [us] | GB/s | of 8 TB/s |\n")
        f.write("|---|---|---|---|---|---|---|\n")
        for r in rows:
            host = f"{r['host_ms']:.2f} ({r['host_min']:.2f} - {r['host_max']:.2f})" if "host_ms" in r else "not measured (no Pillow)"
            f.write(f"| {r['case']} | {r['input'][0]}x{r['input'][1]} -> {r['output'][0]}x{r['output'][1]} | {host} | "
                    f"{r['device_ms']:.3f} ({r['device_min']:.3f} - {r['device_max']:.3f}) | {r['kernels_ms'] * 1e3:.1f} "
                    f"({r['kernels_min'] * 1e3:.1f} - {r['kernels_max'] * 1e3:.1f}) | {r['kernels_gbs']:.0f} | {r['hbm_frac'] * 100:.1f} % |\n")
    print(open(os.path.join(args.out, "image_ingest_run.md")).read())


if __name__ == "__main__":
    main()
