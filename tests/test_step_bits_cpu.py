"""CPU: the one sampler-step kernel (csrc/step.hip) on the emulation against tests/golden/step_bits.npz, the bits every
entry point produced on the card before the step became one kernel (tools/record_step_bits.py).  A case no Philox draw
can influence depends on IEEE mul / add / fma / sqrt / div and f16 conversion alone, all correctly rounded on the card and
on the host: there the emulation must reproduce the recorded bytes exactly.  The keyed cases also go through the
device's logf / sinpif / cospif and are held to the host specification at the tolerance of the other seeded tests."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import inpaint_refs as R
import step_bits_refs as S

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get("EMU_CXX", "/opt/rocm/lib/llvm/bin/clang++")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
CSRC = os.path.join(REPO, "prompt-free-diffusion_amd", "csrc")


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """every fixture case once through emu_step -> [(case, the driver's line, (x_out, pred_x0, xin_next) as recorded types)]"""
    if not os.path.exists(CXX):
        pytest.skip("clang++ of the ROCm toolchain not available")
    out = str(tmp_path_factory.mktemp("pfd_cpu_emu_step"))
    subprocess.run([sys.executable, os.path.join(REPO, "tools", "cpu_emu", "build.py"), out], check=True,
                   stdout=subprocess.DEVNULL, env=dict(os.environ, EMU_ONLY="emu_step", EMU_OPT="-O1"))
    _, cases = S.load()
    paths = [os.path.join(out, f"case{i}.bin") for i in range(len(cases))]
    args = [S.emu_case(c, p) for c, p in zip(cases, paths)]
    r = subprocess.run([os.path.join(out, "emu_step"), *args], capture_output=True, text=True, timeout=900)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith(("ok", "FAIL"))]
    assert len(lines) == len(cases), r.stdout[-3000:] + r.stderr[-1000:]
    got = [tuple(np.fromfile(p + ext, dtype=dt).reshape(c[k].shape)
                 for (k, dt), ext in zip(S.OUTPUTS, (".xout", ".pred", ".xin"))) for c, p in zip(cases, paths)]
    return list(zip(cases, lines, got))


def test_fixture_holds_the_case_list():
    hip, cases = S.load()
    assert hip and [c['name'] for c in cases] == [c['name'] for c in S.settings()]
    assert os.path.getsize(S.FIXTURE) < 512 * 1024
    for c, s in zip(cases, S.settings()):
        assert all(c[k] == v for k, v in s.items()), c['name']
        assert all(c[k] is not None for k, _ in S.OUTPUTS), c['name']
    assert {c['entry'] for c in cases} == set(S.ENTRY_POINTS)


def test_every_case_returns_0_from_one_launch_with_its_guard_bands_intact(runs):
    for c, line, _ in runs:
        assert line.startswith("ok") and " rc 0 launches 1 " in line and "OUTSIDE" not in line, (c['name'], line)


def test_the_16_byte_form_runs_only_on_aligned_rows_of_a_multiple_of_four(runs):
    seen = set()
    for c, line, _ in runs:
        assert line.endswith("| " + S.kernel_of(c)), (c['name'], line)
        assert ("true>" in S.kernel_of(c)) == (c['shape'] == [2, 4, 8, 8] and c['offset'] == 0)
        seen.add(S.kernel_of(c))
    assert len(seen) == 10, seen      # every instantiation of the library


def test_generator_free_cases_reproduce_the_recorded_bytes(runs):
    n = 0
    for c, line, got in runs:
        if not c['generator_free']:
            continue
        n += 1
        for (k, _), g in zip(S.OUTPUTS, got):
            bad = np.flatnonzero(g.reshape(-1) != c[k].reshape(-1))
            assert bad.size == 0, f"{c['name']}: {k} differs from the recording at {bad.size} of {g.size} elements, first {bad[:4]}"
    assert n == sum(s['generator_free'] for s in S.settings()) and n >= 50


def test_keyed_cases_meet_the_host_specification(runs):
    n = 0
    for c, line, got in runs:
        if c['generator_free']:
            continue
        n += 1
        xout, pred, xin = got[0].view(np.float32), got[1].view(np.float32), got[2].view(np.float16)
        ref = S.specification(c)
        B, C, h, w = c['shape']
        xin = xin.reshape(c['rep'], B, h, w, C)
        e = max(R.scaled_err(xout, ref[0]), R.scaled_err(pred, ref[1]))
        ex = R.xin_err(xin[0], ref[0])
        print(f"[step emu] {c['name']}: err {e:.2e}, xin_next beyond its rounding {ex:.2e}")
        assert e <= R.TOL and ex <= R.TOL, (c['name'], e, ex)
        for r in range(c['rep']):
            assert np.array_equal(xin[r], np.transpose(xout, (0, 2, 3, 1)).astype(np.float16)), c['name']
    assert n > 0


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_the_step_is_one_kernel_of_at_most_16_instantiations(tmp_path):
    """kernel symbol names of the gfx950 assembly: the step kernels live in step.hip alone"""
    def kernels(name):
        asm = str(tmp_path / (name + ".s"))
        subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", f"-I{REPO}/include", f"-I{CSRC}",
                        "-mllvm", "-amdgpu-mfma-vgpr-form", "--cuda-device-only", "-S", os.path.join(CSRC, name + ".hip"),
                        "-o", asm], check=True, stderr=subprocess.DEVNULL)
        return set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", open(asm).read(), flags=re.M))
    step = kernels("step")
    assert step and all("cfg_step_kernel" in k for k in step), step
    print(f"[step isa] {len(step)} instantiations of cfg_step_kernel")
    assert len(step) <= 16
    for name in ("elementwise", "inpaint"):
        assert not [k for k in kernels(name) if "cfg_" in k], name
