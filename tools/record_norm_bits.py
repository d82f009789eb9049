#!/usr/bin/env python
"""Record what the GroupNorm entry points and the split-K reductions produce, bit for bit, on the card: every case of
tests/norm_bits_refs.py::cases through the lib.hip.ops wrappers -> tests/golden/norm_bits.txt with, per case, a SHA-256 of
the operands and a SHA-256 of every output (y | table | out, gn_out, gnf_y, ln_out).

The script calls the wrappers only, so it runs unchanged against any build of the library: the committed fixture was recorded
with the GroupNorm stages typed out per kernel, before csrc/gn_stages.h, and a refactor of those kernels is checked against it
(tests/test_norm_bits_gpu.py).  Re-record only when the arithmetic is changed on purpose.
usage: record_norm_bits.py [out.txt]     (needs the built library and a GPU)"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "prompt-free-diffusion_amd"), os.path.join(REPO, "oracle"), os.path.join(REPO, "tests")):
    sys.path.insert(0, p)


def main():
    import torch
    import norm_bits_refs as N
    assert torch.cuda.is_available(), "record_norm_bits.py needs a GPU"
    out = sys.argv[1] if len(sys.argv) > 1 else N.FIXTURE
    rows = []
    for kind, cid in N.cases():
        got = N.run(kind, cid)
        assert got == N.run(kind, cid), f"{kind} {cid}: two launches disagree"
        rows.append((kind, cid, N.input_hash(kind, cid), got))
    N.save(out, rows, torch.version.hip)
    hip, back = N.load(out)
    assert hip == torch.version.hip and back == rows
    print(f"{out}: {len(rows)} cases ({', '.join(f'{sum(r[0] == k for r in rows)} {k}' for k in ('gn', 'table', 'splitk'))}), "
          f"{os.path.getsize(out)} bytes, HIP {hip}")


if __name__ == "__main__":
    main()
