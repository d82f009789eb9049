#!/usr/bin/env python
"""Write tests/golden/image_ingest.npz: what Pillow's `Image.resize(..., BICUBIC)` (app.py:232) returns for the cases of
tests/test_image_ingest_*.py -- the bytes for the small cases, a sha256 for the large ones -- and the Pillow version.

Inputs are NOT stored: `source()` below is a closed integer formula (no RNG stream, no libm), evaluated here and by the
tests.  Needs Pillow; nothing under prompt-free-diffusion_amd/ does.
usage: make_image_golden.py [out.npz]"""
import hashlib
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "image_ingest.npz")

# name: (h, w, c, kind, h', w', stored as bytes?)
CASES = {
    "up":        (97, 131, 3, "hash", 128, 192, True),        # 4 taps per axis
    "down":      (200, 300, 3, "smooth", 64, 128, True),      # 10 / 13 taps
    "h_same":    (130, 70, 3, "hash", 130, 140, True),        # horizontal pass only
    "w_same":    (70, 130, 3, "hash", 140, 130, True),        # vertical pass only
    "identity":  (64, 64, 3, "hash", 64, 64, True),           # no pass: ToTensor only
    "gray":      (50, 77, 1, "hash", 96, 64, True),           # one channel
    "clip":      (33, 35, 3, "checker", 128, 128, True),      # overshoot at every edge: the clamp works at both ends
    "down_big":  (400, 300, 3, "smooth", 64, 64, True),       # 19 / 25 taps
    "app_ctl":   (600, 900, 3, "smooth", 512, 768, False),    # the app's own use
    "max_ratio": (1024, 1024, 3, "hash", 64, 64, False),      # 64 taps, the documented bound
    "full":      (1000, 1500, 3, "smooth", 1536, 1024, False),
}


def _isin(p):
    """integer sinusoid: period 512, range [-256, 256] (a parabola per half period)"""
    q = p % 256
    v = (q * (256 - q)) >> 6
    return np.where((p // 256) % 2 == 0, v, -v)


def source(name):
    """the input picture of a case, uint8 [h, w, c]"""
    h, w, c, kind = CASES[name][:4]
    seed = sum(name.encode())
    i = np.arange(h * w * c, dtype=np.int64)
    y, x, ch = np.unravel_index(i, (h, w, c))
    mix = (i * 2654435761 + seed * 40503) & 0xFFFFFFFF           # multiplicative hash of the flat index, 32 bits
    if kind == "hash":
        v = (mix >> 13) & 255
    elif kind == "checker":
        v = ((y // 3 + x // 2 + ch) % 2) * 255
    elif kind == "smooth":
        v = 128 + ((_isin(7 * x + 85 * ch + seed) * _isin(5 * y + 128)) >> 9)
        v = np.clip(v, 0, 255) ^ ((mix >> 29) & 7)                # three bits of dither
    else:
        raise KeyError(kind)
    return np.clip(v, 0, 255).astype(np.uint8).reshape(h, w, c)


def pillow_resize(a, oh, ow):
    from PIL import Image
    c = a.shape[2]
    im = Image.fromarray(a if c == 3 else a[:, :, 0])
    return np.asarray(im.resize((ow, oh), Image.Resampling.BICUBIC)).reshape(oh, ow, c)


def main():
    import PIL
    out = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    arrays, meta = {}, {"script": "tools/make_image_golden.py", "pillow": PIL.__version__, "cases": {}}
    for name, (h, w, c, kind, oh, ow, stored) in CASES.items():
        ref = pillow_resize(source(name), oh, ow)
        meta["cases"][name] = dict(input=[h, w, c], kind=kind, output=[oh, ow, c], stored=stored,
                                   sha256=hashlib.sha256(ref.tobytes()).hexdigest(),
                                   saturated=[int((ref == 0).sum()), int((ref == 255).sum())])
        if stored:
            arrays[name] = ref
        print(f"{name:10s} {h}x{w}x{c} -> {oh}x{ow}  sat0 {meta['cases'][name]['saturated'][0]:6d} "
              f"sat255 {meta['cases'][name]['saturated'][1]:6d}  {meta['cases'][name]['sha256'][:12]}")
    arrays["meta"] = np.array(json.dumps(meta))
    np.savez_compressed(out, **arrays)
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
