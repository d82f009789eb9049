#!/usr/bin/env python
"""Time the Canny edge hint on the GPU (ops.canny_u8, csrc/canny.hip), per picture, three channels:

  canny alone:      the uint8 picture is on the device at the output size -> the fp16 hint [1, 3, H, W]; 4 launches
  resize + canny:   a larger uint8 picture on the device -> Pillow-exact bicubic resize as uint8 (ops.image_from_u8,
                    layout='u8'; 2 launches) -> the hint: what generate(control=<uint8>, control_preprocess='canny') does
  resize + ingest:  the same picture through the existing ops.image_from_u8 to the fp16 tensor (no edge detector), for scale
  host:             the numpy specification (lib/canny.py) on the same resized picture, wall clock -- the statement the
                    kernels are held to, not an optimised host implementation (cv2.Canny would be far faster than it)

HIP events around the calls, warm, median of --reps after --warmup; the device result is compared with the specification
once per case.  Needs a GPU.
usage: bench_canny.py [--reps 50] [--out DIR]   -> DIR/canny_run.json, DIR/canny_run.md"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "prompt-free-diffusion_amd"), os.path.join(REPO, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

import make_canny_golden as G  # noqa: E402
from bench_image_ingest import events_ms  # noqa: E402

# (output H, W), (source H, W) of the resize
CASES = [((512, 512), (600, 600)), ((1024, 768), (1200, 900))]


def picture(h, w, kind):
    """'contours': grey curved contours in levels 48 apart; after the resize about one pixel in five is an edge (the photograph
    crop of the fixture has one in eight).  'dense': another contour set per channel plus three bits of dither per byte, after
    which two pixels in five are edges -- more union-find work than a picture gives"""
    if kind == "contours":
        return np.ascontiguousarray(np.repeat(G.blobs(h, w, 1, 9), 3, 2))
    i = np.arange(h * w * 3, dtype=np.int64).reshape(h, w, 3)
    return G.blobs(h, w, 3, 9) + ((((i * 2654435761) & 0xFFFFFFFF) >> 29) & 7).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_canny needs a GPU (a CPU run gives no time)"
    from lib import canny as K
    from lib.hip import ops
    rows = []
    for (h, w), (sh, sw), kind in [c + (k,) for c in CASES for k in ("contours", "dense")]:
        big = torch.from_numpy(picture(sh, sw, kind)).cuda()
        small = ops.image_from_u8(big, (h, w), layout='u8')
        host_in = small[0].cpu().numpy()
        t0 = time.perf_counter()
        st = K.canny_states(host_in, 100, 200)
        want = K.hysteresis(st)
        host_ms = (time.perf_counter() - t0) * 1e3
        got = ops.canny_u8(small)[0].cpu().numpy()
        assert np.array_equal(got, want), (h, w, kind)
        row = dict(picture=kind, output=[h, w], source=[sh, sw], strong=int((st == 2).sum()), weak=int((st == 1).sum()),
                   edges=int((want == 255).sum()), host_numpy_spec_ms=host_ms, launches_canny=4, launches_resize=2)
        for key, fn in (("canny_ms", lambda: ops.canny_u8(small, out='hint', dtype=torch.float16)),
                        ("canny_u8_out_ms", lambda: ops.canny_u8(small)),
                        ("resize_canny_ms", lambda: ops.canny_u8(ops.image_from_u8(big, (h, w), layout='u8'), out='hint',
                                                                 dtype=torch.float16)),
                        ("resize_ingest_ms", lambda: ops.image_from_u8(big, (h, w), dtype=torch.float16))):
            row[key], row[key[:-3] + "_min"], row[key[:-3] + "_max"] = events_ms(fn, args.reps, args.warmup)
        rows.append(row)
        print(json.dumps(row), flush=True)
    res = dict(device=torch.cuda.get_device_name(0), reps=args.reps, cv2=G.load()[0]["cv2"], rows=rows)
    os.makedirs(args.out, exist_ok=True)
    with open(os.path.join(args.out, "canny_run.json"), "w") as f:
        json.dump(res, f, indent=1)
    with open(os.path.join(args.out, "canny_run.md"), "w") as f:
        f.write(f"device {res['device']}, median of {args.reps} warm runs (min - max), HIP events; fixture: {res['cv2']}\n\n")
        f.write("| picture | H x W | strong / weak / edges | canny alone, fp16 hint [us] | canny alone, uint8 [us] | resize + canny [us] | "
                "resize + ingest (no detector) [us] | numpy specification on the host [ms] | launches |\n|---|---|---|---|---|---|---|---|---|\n")
        for r in rows:
            us = lambda k: f"{r[k + '_ms'] * 1e3:.1f} ({r[k + '_min'] * 1e3:.1f} - {r[k + '_max'] * 1e3:.1f})"      # noqa: E731
            f.write(f"| {r['picture']} | {r['output'][0]} x {r['output'][1]} (from {r['source'][0]} x {r['source'][1]}) | {r['strong']} / {r['weak']} / "
                    f"{r['edges']} | {us('canny')} | {us('canny_u8_out')} | {us('resize_canny')} | {us('resize_ingest')} | "
                    f"{r['host_numpy_spec_ms']:.0f} | {r['launches_canny']} + {r['launches_resize']} |\n")
    print(open(os.path.join(args.out, "canny_run.md")).read())


if __name__ == "__main__":
    main()
