"""CPU: the fragment pipeline of the wave-specialised 3x3 patch kernel (conv3x3_patch_ws_kernel).
(a) the kernel on the CPU emulation (tools/cpu_emu): three channel blocks, a split-K slice of one block, the GroupNorm-prologue
form -- against the double-precision reference and bit for bit against the 8-wave kernel, whose loop reads every fragment behind
the barrier; the dispatcher's decisions unchanged.  (b) the generated gfx950 code of the four instantiations: register and LDS
budget, reads and MFMAs per tap, and the distance between every LDS wait of the tap loop and the read it waits for.
What neither can see is a read that is issued before its data has landed: tests/test_patch_pipeline_gpu.py."""
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get("EMU_CXX", "/opt/rocm/lib/llvm/bin/clang++")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
sys.path.insert(0, os.path.join(REPO, "tools"))

DISPATCH_SHAPES = ("unet_c2_gemm_shapes.txt", "ups_phase_fold_shapes.txt", "lin_shapes_ablation.txt", "r06_fixed_cost_probe_shapes.txt")
# LDS bytes of the instantiations before the pipeline: two patches + two (three) weight tiles
LDS_BYTES = {"<2>": 143360, "<1>": 143360, "<0,2>": 143360, "<0,3>": 163840}


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    if not os.path.exists(CXX):
        pytest.skip("clang++ of the ROCm toolchain not available")
    out = str(tmp_path_factory.mktemp("pfd_cpu_emu_patch_pipeline"))
    subprocess.run([sys.executable, os.path.join(REPO, "tools", "cpu_emu", "build.py"), out], check=True, stdout=subprocess.DEVNULL,
                   env=dict(os.environ, EMU_ONLY="emu_gemm"))
    return os.path.join(out, "emu_gemm")


def test_pipelined_patch_kernel_on_the_cpu_emulation(emu):
    r = subprocess.run([emu, "fragment pipeline"], capture_output=True, text=True, timeout=900)
    lines = [l for l in r.stdout.splitlines() if l.startswith(("ok", "FAIL"))]
    assert r.returncode == 0 and len(lines) == 5 and all(l.startswith("ok") for l in lines), r.stdout[-3000:] + r.stderr[-1000:]
    # forms 96 and 98 of one problem each carry the same bits as form 99, so the three are equal to each other
    for what in ("16x16x192", "split-K 3"):
        same = [l for l in lines if what in l and "== variant 99 bitwise" in l]
        assert len(same) == 2, "\n".join(lines)
    assert sum("prologue" in l for l in lines) == 1


def test_dispatch_is_unchanged(emu):
    files = [os.path.join(REPO, "profiles", f) for f in DISPATCH_SHAPES]
    r = subprocess.run([emu, "--dispatch"] + files, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.splitlines() == open(os.path.join(REPO, "tests", "golden", "gemm_dispatch.txt")).read().splitlines()


@pytest.fixture(scope="module")
def reports():
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    import isa_audit
    asm = isa_audit.compile_asm(os.path.join(isa_audit.CSRC, "gemm_glds.hip"))
    return {inst: isa_audit.patch_pipeline_report(asm, part) for inst, part in isa_audit.PATCH_WS.items()}


@pytest.mark.parametrize("inst", sorted(LDS_BYTES))
def test_budget_and_tap_loop_of_the_generated_code(reports, inst):
    r = reports[inst]
    print(f"[patch-pipeline] conv3x3_patch_ws_kernel{inst}: {r}")
    assert r["vgprs"] <= 168 and r["scratch"] == 0 and r["lds"] == LDS_BYTES[inst], r
    # one tap: 2 half steps x (4 A + 5 B fragments), 2 x 4 x 5 MFMAs, one barrier, no other LDS traffic in the consumer loop
    assert (r["reads"], r["mfmas"], r["barriers"], r["other_lds"]) == (18, 40, 1, 0), r


@pytest.mark.parametrize("inst", sorted(LDS_BYTES))
def test_every_lds_wait_but_the_first_after_the_barrier_is_eight_mfmas_behind_its_read(reports, inst):
    """steady: the second of two consecutive passes of the tap loop (taps 1..7); block: one pass of the channel-block loop --
    tap 0's reads behind its barrier, one loop body, tap 8 without a prefetch"""
    r = reports[inst]
    for what in ("steady", "block"):
        waits = r[what]
        print(f"[patch-pipeline] conv3x3_patch_ws_kernel{inst} {what}: " + " ".join(f"lgkmcnt({n}):{d}{'*' if f else ''}" for n, d, f in waits))
        assert len(waits) >= 5 and sum(f for _, _, f in waits) == (1 if what == "steady" else 2), waits
        near = [(n, d) for n, d, first in waits if not first and d is not None and d < 8]
        assert not near, (inst, what, near)
