"""GPU: every case of tests/golden/norm_bits.txt through the lib.hip.ops wrappers hashes to the recorded value -- the bits the
GroupNorm kernels of csrc/norm.hip and the three split-K reductions of csrc/gemm_glds.hip produced before their shared stages
moved to csrc/gn_stages.h (tools/record_norm_bits.py).  A case whose regenerated operands do not hash to the recorded value
fails: nothing is skipped."""
import pytest
import torch

import norm_bits_refs as N

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fixture():
    return N.load()


@pytest.mark.parametrize("kind", ("gn", "table", "splitk"))
def test_cases_equal_the_recorded_bits(fixture, kind):
    hip, rows = fixture
    assert [(k, cid) for k, cid, _, _ in rows] == N.cases(), "the fixture does not hold the case list"
    bad, n = [], 0
    for k, cid, hin, want in rows:
        if k != kind:
            continue
        n += 1
        if N.input_hash(k, cid) != hin:
            bad.append(f"{cid}: the regenerated operands are not the recorded ones")
            continue
        got = N.run(k, cid)
        if got != want:
            bad.append(f"{cid}: {sorted(o for o in set(got) | set(want) if got.get(o) != want.get(o))} differ")
    print(f"[norm-bits] {kind}: {n} cases, {len(bad)} differ (recorded under HIP {hip}, running {torch.version.hip})")
    assert n and not bad, bad
