#!/usr/bin/env python
"""Record what the fused sampler-step entry points produce, bit for bit, on the card: every case of
tests/step_bits_refs.py::settings through the lib.hip.ops wrappers (cfg_ddim_step, cfg_dpmpp_step, cfg_step_masked) ->
tests/golden/step_bits.npz with each case's inputs, its three outputs as raw bytes, and torch.version.hip.

The script calls the wrappers only, so it runs unchanged against any build of the library: the committed fixture was
recorded with the four step kernel templates that csrc/step.hip replaced, and a refactor of the step is checked against it
(tests/test_step_bits_cpu.py on the emulation, tests/test_step_bits_gpu.py on the card).  Re-record only when the step's
arithmetic is changed on purpose.
usage: record_step_bits.py [out.npz]     (needs the built library and a GPU)"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "prompt-free-diffusion_amd"), os.path.join(REPO, "tests")):
    sys.path.insert(0, p)


def main():
    import torch
    import step_bits_refs as S
    from lib.hip import ops
    assert torch.cuda.is_available(), "record_step_bits.py needs a GPU"
    out = sys.argv[1] if len(sys.argv) > 1 else S.FIXTURE
    cases = []
    for c in S.settings():
        c = dict(c, **S.make_inputs(c))
        got = S.run_ops(c, ops, torch)
        again = S.run_ops(c, ops, torch)
        assert all((a == b).all() for a, b in zip(got, again)), f"{c['name']}: two launches disagree"
        c.update({k: v for (k, _), v in zip(S.OUTPUTS, got)})
        cases.append(c)
    S.save(out, cases, torch.version.hip)
    hip, back = S.load(out)
    assert hip == torch.version.hip and len(back) == len(cases)
    print(f"{out}: {len(cases)} cases ({sum(c['generator_free'] for c in cases)} generator-free), "
          f"{os.path.getsize(out)} bytes, HIP {hip}")


if __name__ == "__main__":
    main()
