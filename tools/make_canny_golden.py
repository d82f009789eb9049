#!/usr/bin/env python
"""Write tests/golden/canny.npz: the input pictures of tests/test_canny_*.py and what the numpy specification
(prompt-free-diffusion_amd/lib/canny.py) makes of them -- the state bytes after non-maximum suppression and the edge
bytes after hysteresis, per case (packed into one byte per pixel: the state in bits 0-1, the edge in bit 2) -- plus, per case, the count of strong / weak / edge pixels and the number of sweeps a
dilation formulation of the hysteresis needs.

Where OpenCV can be imported the tool also runs `cv2.Canny(img, low, high)` on every case and stores the OpenCV version and
the number of differing pixels; where it cannot, it stores "cv2 absent": the equality of the specification with
cv2.Canny is then UNVERIFIED, and nothing in the repository may claim it.

The photograph crop comes from a picture file given on the command line (any RGB photograph; needs Pillow to decode);
without one the crop already in the fixture is kept.
usage: make_canny_golden.py [--photo picture.jpg] [out.npz]"""
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "canny.npz")
if os.path.join(REPO, "prompt-free-diffusion_amd") not in sys.path:
    sys.path.insert(0, os.path.join(REPO, "prompt-free-diffusion_amd"))

DEFAULT = (100, 200)
THRESHOLDS = (DEFAULT, (200, 100), (99.9, 200.5), (0, 0), (0, 2000))
# pictures that are run at every threshold pair; every other picture is run at the default pair only
SWEPT = ("smooth2", "p70x150", "chan")


def _hash(shape, seed):
    i = np.arange(int(np.prod(shape)), dtype=np.int64)
    return ((((i * 2654435761 + seed * 40503) & 0xFFFFFFFF) >> 13) & 255).astype(np.uint8).reshape(shape)


def _isin(p):
    """integer sinusoid: period 512, range [-256, 256] (a parabola per half period)"""
    q = p % 256
    v = (q * (256 - q)) >> 6
    return np.where((p // 256) % 2 == 0, v, -v)


def blobs(h, w, c, seed):
    """closed-form curved contours in every direction: a product of two integer sinusoids per channel, in grey levels 48 apart
    (a straight step of 48 is weak at the default thresholds, a diagonal one strong)"""
    y, x, ch = np.meshgrid(np.arange(h), np.arange(w), np.arange(c), indexing="ij")
    f = (_isin(7 * x + 3 * y + 77 * ch + seed) * _isin(3 * x - 5 * y + 131 * ch + 3 * seed)) >> 9         # [-128, 128]
    return (np.clip(128 + f, 0, 255) // 48 * 48).astype(np.uint8)


def step(kind, n=16, height=60):
    y, x = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    on = {"v": x >= 8, "h": y >= 8, "d1": x + y >= n, "d2": x - y >= 0}[kind]
    return (on * height).astype(np.uint8)


def channels_disagree():
    """three channels with different gradients at the same pixels: a vertical step in R, a horizontal one of the same height
    in G (equal magnitudes where they cross: the lowest channel keeps the tie), a larger diagonal one in B"""
    n = 24
    y, x = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    return np.stack([(x >= 8) * 60, (y >= 8) * 60, (x + y >= 30) * 90], -1).astype(np.uint8)


def serpentine(h, w, lit=True):
    """one winding band of weak pixels, three pixels thick, with (lit) a short strong stretch at its start"""
    img = np.zeros((h, w), np.uint8)
    rows = list(range(4, h - 6, 8))
    for r in rows:
        img[r:r + 3, 4:w - 4] = 30
    for k, (r0, r1) in enumerate(zip(rows, rows[1:])):
        if k % 2 == 0:
            img[r0:r1 + 3, w - 7:w - 4] = 30
        else:
            img[r0:r1 + 3, 4:7] = 30
    img[4:7, 4:10] = 60 if lit else 30
    return img


def blurred_noise(h, w, c, sigma, seed):
    """uniform noise blurred with a Gaussian of `sigma` (separable, reflected border), scaled to 0 ... 255"""
    a = np.random.default_rng(seed).random((h, w, c))
    r = int(4 * sigma + 0.5)
    k = np.exp(-0.5 * (np.arange(-r, r + 1) / sigma) ** 2)
    k /= k.sum()
    for axis in (0, 1):
        pad = [(r, r) if ax == axis else (0, 0) for ax in range(3)]
        a = np.apply_along_axis(lambda v: np.convolve(v, k, mode="valid"), axis, np.pad(a, pad, mode="reflect"))
    a = (a - a.min()) / (a.max() - a.min())
    return np.round(a * 255).astype(np.uint8)


def photo_crop(path):
    from PIL import Image
    a = np.asarray(Image.open(path).convert("RGB"))
    y0, x0 = (a.shape[0] - 96) // 2, (a.shape[1] - 128) // 2
    return np.ascontiguousarray(a[y0:y0 + 96, x0:x0 + 128])


def pictures(photo=None):
    p = {
        "t1x1": _hash((1, 1, 3), 1), "t1x17": _hash((1, 17, 3), 2), "t5x3": _hash((5, 3, 1), 3),
        "p64": blobs(64, 64, 3, 5), "p128x256": blobs(128, 256, 1, 6), "p70x150": blobs(70, 150, 3, 7),
        "p133x200": blobs(133, 200, 1, 8),
        "step_v": step("v"), "step_h": step("h"), "step_d1": step("d1"), "step_d2": step("d2"),
        "flat0": np.zeros((9, 13, 3), np.uint8), "flat255": np.full((9, 13, 3), 255, np.uint8),
        "chan": channels_disagree(),
        # four grey levels per channel, drawn per pixel: equal magnitudes in two channels are common, and at some pixels
        # the channel that keeps the tie decides the state and the edge (tests/test_canny_cpu.py swaps R and G)
        "ties": ((_hash((24, 24, 3), 45) >> 6) * 20).astype(np.uint8),
        "smooth2": blurred_noise(96, 130, 3, 2.0, 2), "smooth3": blurred_noise(96, 130, 3, 3.0, 3),
        "serp70": serpentine(70, 150), "serp70_off": serpentine(70, 150, lit=False),
        "serp133": serpentine(133, 200), "serp133_off": serpentine(133, 200, lit=False),
    }
    if photo is not None:
        p["photo"] = photo
    return p


def case_name(pic, thr):
    return pic if tuple(thr) == DEFAULT else f"{pic}@{thr[0]:g},{thr[1]:g}"


def case_list(names):
    """[(case name, picture name, (low, high))]"""
    return [(case_name(p, t), p, t) for p in names for t in (THRESHOLDS if p in SWEPT else (DEFAULT,))]


def load(path=GOLDEN):
    """-> (meta, {picture: uint8 array}, {case: (picture name, (low, high), states, edges)})"""
    g = np.load(path, allow_pickle=False)
    meta = json.loads(str(g["meta"]))
    pics = {k[4:]: g[k] for k in g.files if k.startswith("img.")}
    cases = {}
    for c, m in meta["cases"].items():
        e = g["expect." + c]                 # one byte per pixel: the state in bits 0-1, the edge in bit 2
        cases[c] = (m["picture"], tuple(m["thresholds"]), e & 3, ((e >> 2) * 255).astype(np.uint8))
    return meta, pics, cases


def main():
    from lib import canny as K
    args = sys.argv[1:]
    photo = None
    if "--photo" in args:
        i = args.index("--photo")
        photo = photo_crop(args[i + 1])
        del args[i:i + 2]
    out = args[0] if args else GOLDEN
    if photo is None and os.path.exists(GOLDEN):
        photo = load(GOLDEN)[1].get("photo")
    pics = pictures(photo)
    try:
        import cv2
        cv = cv2.__version__
    except ImportError:
        cv2, cv = None, "cv2 absent"
    arrays = {"img." + k: v for k, v in pics.items()}
    meta = {"script": "tools/make_canny_golden.py", "cv2": cv, "cases": {},
            "cv2_verified": "compared with cv2.Canny, see cv2_differing per case" if cv2 else
            "UNVERIFIED: cv2 absent, the expected bytes are the numpy specification's alone"}
    for name, pic, thr in case_list(pics):
        st = K.canny_states(pics[pic], *thr)
        ed = K.hysteresis(st)
        ed2, sweeps = K.hysteresis_by_dilation(st)
        assert np.array_equal(ed, ed2), name
        m = dict(picture=pic, thresholds=list(thr), shape=list(pics[pic].shape), strong=int((st == 2).sum()),
                 weak=int((st == 1).sum()), edges=int((ed == 255).sum()), sweeps=sweeps)
        m["promoted"] = m["edges"] - m["strong"]
        if cv2 is not None:
            m["cv2_differing"] = int((cv2.Canny(np.ascontiguousarray(pics[pic]), thr[0], thr[1]) != ed).sum())
        meta["cases"][name] = m
        arrays["expect." + name] = st | ((ed == 255).astype(np.uint8) << 2)
        print(f"{name:22s} {str(pics[pic].shape):14s} strong {m['strong']:5d} weak {m['weak']:5d} edges {m['edges']:5d} "
              f"promoted {m['promoted']:5d} sweeps {sweeps:4d}" + (f"  cv2 differs in {m['cv2_differing']}" if cv2 else ""))
    arrays["meta"] = np.array(json.dumps(meta))
    np.savez_compressed(out, **arrays)
    print(f"cv2: {cv} ({meta['cv2_verified']})")
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
