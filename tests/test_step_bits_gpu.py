"""GPU: every case of tests/golden/step_bits.npz through the lib.hip.ops wrappers equals the recorded bytes -- the bits the
five sampler-step entry points produced before they became one kernel (tools/record_step_bits.py;
tests/test_step_bits_cpu.py holds the emulation to the same file)."""
import numpy as np
import pytest
import torch

import step_bits_refs as S

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fixture():
    return S.load()


def _mismatches(c, got):
    out = []
    for (k, _), g in zip(S.OUTPUTS, got):
        bad = np.flatnonzero(g.reshape(-1) != c[k].reshape(-1))
        if bad.size:
            out.append(f"{k}: {bad.size} of {g.size} elements differ, first {bad[:4].tolist()}")
    return out


def test_generator_free_cases_equal_the_recorded_bytes(fixture):
    """no Philox draw reaches these outputs: correctly rounded operations only, whatever the HIP version"""
    from lib.hip import ops
    _, cases = fixture
    n = 0
    for c in cases:
        if c['generator_free']:
            n += 1
            bad = _mismatches(c, S.run_ops(c, ops, torch))
            assert not bad, (c['name'], bad)
    assert n >= 50


def test_keyed_cases_equal_the_recorded_bytes(fixture):
    from lib.hip import ops
    hip, cases = fixture
    n = 0
    for c in cases:
        if not c['generator_free']:
            n += 1
            bad = _mismatches(c, S.run_ops(c, ops, torch))
            why = "" if hip == torch.version.hip else \
                f" -- KEYED MISMATCH UNDER ANOTHER HIP: recorded with {hip}, running {torch.version.hip} " \
                f"(the device's logf / sinpif / cospif enter these cases)"
            assert not bad, f"{c['name']}: {bad}{why}"
    assert n >= 50
