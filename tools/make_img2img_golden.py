#!/usr/bin/env python
"""Write tests/golden/img2img.npz: the oracle's VAE-encoder moments (oracle/pfd_oracle.py::vae_encode_moments, fp32 on
the CPU) of a 256x256 picture under the seeded weights of the test suite -- 65536 rows at the encoder's top level, the
smallest picture whose convolutions take the wide-tile dispatch a 512x512 request takes.

The picture is NOT stored: tests/img2img_refs.py::picture_u8 is a closed integer formula, evaluated here and by the tests.
tests/test_img2img_cpu.py recomputes the fixture from oracle/; tests/test_img2img_gpu.py compares the HIP encoder with it.
usage: make_img2img_golden.py [out.npz]"""
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in ("tests", "oracle"):
    sys.path.insert(0, os.path.join(REPO, p))
GOLDEN = os.path.join(REPO, "tests", "golden", "img2img.npz")
SIDE, PICTURE_SEED, PREFIX = 256, 0, "vae.image."


def oracle_moments(side=SIDE, seed=PICTURE_SEED):
    """float32 [1, 8, side/8, side/8]"""
    import pfd_oracle as O
    from img2img_refs import picture_f32
    from weights import seeded_tensor
    spec = json.load(open(os.path.join(REPO, "tests", "golden", "state_spec.json")))
    sd = {k: seeded_tensor(k, v["shape"], 0) for k, v in spec.items() if v["param"] and k.startswith(PREFIX)}
    with torch.no_grad():
        return O.vae_encode_moments(sd, PREFIX, torch.from_numpy(picture_f32(side, side, seed))).float().numpy()


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    m = oracle_moments()
    meta = dict(script="tools/make_img2img_golden.py", side=SIDE, picture_seed=PICTURE_SEED, prefix=PREFIX,
                mean_absmax=float(np.abs(m[:, :4]).max()), logvar_range=[float(m[:, 4:].min()), float(m[:, 4:].max())])
    np.savez_compressed(out, moments=m, meta=np.array(json.dumps(meta)))
    print(out, os.path.getsize(out), "bytes", meta)


if __name__ == "__main__":
    main()
