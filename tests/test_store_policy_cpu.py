"""CPU: the store-policy helper of csrc/pfd_common.h (gst / gst_t).
  * under the emulation (tools/cpu_emu, PFD_CPU_EMU) every policy is a plain store: the drivers build with the helper in every
    epilogue, and the cases that go through the touched store paths still pass;
  * the policy each kernel's global stores carry in the generated gfx950 ISA (tools/isa_audit.py --stores) is the table below --
    a policy must not appear, or disappear, unnoticed;
  * registers and scratch of every kernel whose stores go through the helper are what they were before the helper existed
    (the first two figures of every row were read off the build without it; with the write-through stores of the final store
    passes no kernel's count moved)."""
import os
import shutil
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
CXX = os.environ.get("EMU_CXX", "/opt/rocm/lib/llvm/bin/clang++")
HAVE_HIPCC = shutil.which("hipcc") is not None or os.path.exists("/opt/rocm/bin/hipcc")


@pytest.mark.skipif(not os.path.exists(CXX), reason="clang++ of the ROCm toolchain not available")
def test_emulation_builds_with_the_policy_helper_and_its_cases_pass(tmp_path):
    out = str(tmp_path)
    subprocess.run([sys.executable, os.path.join(REPO, "tools", "cpu_emu", "build.py"), out], check=True, stdout=subprocess.DEVNULL)

    def ok_lines(cmd):
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        lines = [l for l in r.stdout.splitlines() if l.startswith(("ok", "FAIL"))]
        assert r.returncode == 0 and lines and all(l.startswith("ok") for l in lines), r.stdout[-3000:] + r.stderr[-1000:]
        return lines

    # final store pass + slab branch + plain reduction (variant 98 / 99), the statistics-emitting store pass and reduction,
    # the residual read of the store pass and of the reduction
    assert len(ok_lines([os.path.join(out, "emu_gemm"), "variant 98", "variant 99", "statistics", "residual read with one wrap"])) >= 7
    assert len(ok_lines([os.path.join(out, "emu_norm"), "--quick"])) == 5            # gn_small_kernel, gn_apply_pstats_kernel
    assert len(ok_lines([os.path.join(out, "emu_attn"), "--quick", "--w4"])) == 2    # the attention2_kernel epilogue


# kernel (mangled, as in the assembly) -> (VGPRs, scratch bytes, plain / write-through / non-temporal global stores)
SHIPPED = {
    "_ZN12_GLOBAL__N_114gemm160_kernelILi2ELi2ELb0ELi2ELi4EEEvNS_10G160ParamsE": (129, 0, 36, 11, 0),
    "_ZN12_GLOBAL__N_114gemm160_kernelILi2ELi2ELb0ELi2ELi5EEEvNS_10G160ParamsE": (169, 0, 45, 21, 0),
    "_ZN12_GLOBAL__N_114gemm160_kernelILi2ELi2ELb0ELi4ELi5EEEvNS_10G160ParamsE": (257, 0, 45, 21, 0),
    "_ZN12_GLOBAL__N_114gemm160_kernelILi2ELi2ELb1ELi2ELi4EEEvNS_10G160ParamsE": (129, 0, 36, 6, 0),
    "_ZN12_GLOBAL__N_114gemm160_kernelILi2ELi2ELb1ELi2ELi5EEEvNS_10G160ParamsE": (169, 0, 45, 15, 0),
    "_ZN12_GLOBAL__N_114gemm160_kernelILi2ELi2ELb1ELi4ELi5EEEvNS_10G160ParamsE": (257, 0, 45, 15, 0),
    "_ZN12_GLOBAL__N_114gemm160_kernelILi2ELi4ELb0ELi2ELi4EEEvNS_10G160ParamsE": (169, 0, 72, 22, 0),
    "_ZN12_GLOBAL__N_114gemm160_kernelILi2ELi4ELb0ELi2ELi5EEEvNS_10G160ParamsE": (176, 0, 90, 39, 0),
    "_ZN12_GLOBAL__N_114gemm160_kernelILi2ELi4ELb0ELi3ELi5EEEvNS_10G160ParamsE": (257, 0, 90, 39, 0),
    "_ZN12_GLOBAL__N_114gemm160_kernelILi2ELi4ELb1ELi2ELi4EEEvNS_10G160ParamsE": (169, 0, 72, 12, 0),
    "_ZN12_GLOBAL__N_114gemm160_kernelILi2ELi4ELb1ELi2ELi5EEEvNS_10G160ParamsE": (171, 0, 90, 27, 0),
    "_ZN12_GLOBAL__N_114gemm160_kernelILi2ELi4ELb1ELi3ELi5EEEvNS_10G160ParamsE": (257, 0, 90, 27, 0),
    "_ZN12_GLOBAL__N_114gemm160_kernelILi4ELi1ELb0ELi2ELi5EEEvNS_10G160ParamsE": (97, 0, 23, 15, 0),
    "_ZN12_GLOBAL__N_114gemm160_kernelILi4ELi1ELb0ELi4ELi5EEEvNS_10G160ParamsE": (169, 0, 23, 15, 0),
    "_ZN12_GLOBAL__N_114gemm160_kernelILi4ELi1ELb1ELi2ELi5EEEvNS_10G160ParamsE": (97, 0, 23, 9, 0),
    "_ZN12_GLOBAL__N_114gemm160_kernelILi4ELi1ELb1ELi4ELi5EEEvNS_10G160ParamsE": (169, 0, 23, 9, 0),
    "_ZN12_GLOBAL__N_114gemm160_kernelILi4ELi2ELb0ELi2ELi5EEEvNS_10G160ParamsE": (115, 0, 45, 21, 0),
    "_ZN12_GLOBAL__N_114gemm160_kernelILi4ELi2ELb0ELi3ELi5EEEvNS_10G160ParamsE": (169, 0, 45, 21, 0),
    "_ZN12_GLOBAL__N_114gemm160_kernelILi4ELi2ELb1ELi2ELi5EEEvNS_10G160ParamsE": (119, 0, 45, 15, 0),
    "_ZN12_GLOBAL__N_114gemm160_kernelILi4ELi2ELb1ELi3ELi5EEEvNS_10G160ParamsE": (169, 0, 45, 15, 0),
    "_ZN12_GLOBAL__N_114gemm160_kernelILi4ELi4ELb0ELi2ELi10EEEvNS_10G160ParamsE": (230, 0, 0, 10, 0),
    "_ZN12_GLOBAL__N_114gemm160_kernelILi4ELi4ELb0ELi2ELi4EEEvNS_10G160ParamsE": (169, 0, 72, 22, 0),
    "_ZN12_GLOBAL__N_114gemm160_kernelILi4ELi4ELb0ELi2ELi5EEEvNS_10G160ParamsE": (176, 0, 90, 39, 0),
    "_ZN12_GLOBAL__N_114gemm160_kernelILi4ELi4ELb1ELi2ELi10EEEvNS_10G160ParamsE": (254, 0, 0, 10, 0),
    "_ZN12_GLOBAL__N_114gemm160_kernelILi4ELi4ELb1ELi2ELi4EEEvNS_10G160ParamsE": (169, 0, 72, 12, 0),
    "_ZN12_GLOBAL__N_114gemm160_kernelILi4ELi4ELb1ELi2ELi5EEEvNS_10G160ParamsE": (169, 0, 90, 27, 0),
    "_ZN12_GLOBAL__N_116gemm160ws_kernelILb0ELi4ELi2ELb0EEEvNS_10G160ParamsE": (145, 0, 70, 9, 0),
    "_ZN12_GLOBAL__N_116gemm160ws_kernelILb0ELi4ELi3ELb0EEEvNS_10G160ParamsE": (145, 0, 70, 9, 0),
    "_ZN12_GLOBAL__N_116gemm160ws_kernelILb0ELi5ELi2ELb0EEEvNS_10G160ParamsE": (166, 0, 87, 20, 0),
    "_ZN12_GLOBAL__N_116gemm160ws_kernelILb0ELi5ELi3ELb0EEEvNS_10G160ParamsE": (166, 0, 87, 20, 0),
    "_ZN12_GLOBAL__N_116gemm160ws_kernelILb1ELi4ELi2ELb0EEEvNS_10G160ParamsE": (146, 0, 70, 9, 0),
    "_ZN12_GLOBAL__N_116gemm160ws_kernelILb1ELi4ELi2ELb1EEEvNS_10G160ParamsE": (146, 0, 70, 9, 0),
    "_ZN12_GLOBAL__N_116gemm160ws_kernelILb1ELi4ELi3ELb0EEEvNS_10G160ParamsE": (145, 0, 70, 9, 0),
    "_ZN12_GLOBAL__N_116gemm160ws_kernelILb1ELi4ELi3ELb1EEEvNS_10G160ParamsE": (145, 0, 70, 9, 0),
    "_ZN12_GLOBAL__N_116gemm160ws_kernelILb1ELi5ELi2ELb0EEEvNS_10G160ParamsE": (167, 0, 87, 20, 0),
    "_ZN12_GLOBAL__N_116gemm160ws_kernelILb1ELi5ELi2ELb1EEEvNS_10G160ParamsE": (166, 0, 87, 20, 0),
    "_ZN12_GLOBAL__N_116gemm160ws_kernelILb1ELi5ELi3ELb0EEEvNS_10G160ParamsE": (167, 0, 87, 20, 0),
    "_ZN12_GLOBAL__N_116gemm160ws_kernelILb1ELi5ELi3ELb1EEEvNS_10G160ParamsE": (167, 0, 87, 20, 0),
    "_ZN12_GLOBAL__N_120conv3x3_patch_kernelENS_10G160ParamsE": (169, 0, 90, 27, 0),
    "_ZN12_GLOBAL__N_120splitk_reduce_kernelENS_10G160ParamsE": (80, 0, 1, 0, 0),
    "_ZN12_GLOBAL__N_123conv3x3_patch_ws_kernelILi0ELi2EEEvNS_10G160ParamsE": (164, 0, 87, 20, 0),
    "_ZN12_GLOBAL__N_123conv3x3_patch_ws_kernelILi0ELi3EEEvNS_10G160ParamsE": (163, 0, 87, 20, 0),
    "_ZN12_GLOBAL__N_123conv3x3_patch_ws_kernelILi1ELi2EEEvNS_10G160ParamsE": (164, 0, 87, 20, 0),
    "_ZN12_GLOBAL__N_123conv3x3_patch_ws_kernelILi2ELi2EEEvNS_10G160ParamsE": (164, 0, 87, 20, 0),
    "_ZN12_GLOBAL__N_123splitk_reduce_gn_kernelENS_10G160ParamsE": (132, 0, 4, 0, 0),
    "_ZN12_GLOBAL__N_126splitk_reduce_gnorm_kernelENS_10G160ParamsENS_6GnFuseE": (94, 0, 16, 0, 0),
    "_ZN12_GLOBAL__N_115gn_apply_kernelENS_5GnSrcEPKDF16_S2_PKfPDF16_liiiiiff": (97, 0, 4, 0, 0),
    "_ZN12_GLOBAL__N_115gn_small_kernelENS_5GnSrcEPKDF16_S2_PDF16_liiif": (61, 0, 8, 0, 0),
    "_ZN12_GLOBAL__N_116layernorm_kernelILb0ELi1EEEvPKDF16_lS2_S2_PDF16_liifiii": (33, 0, 1, 0, 0),
    "_ZN12_GLOBAL__N_116layernorm_kernelILb0ELi2EEEvPKDF16_lS2_S2_PDF16_liifiii": (52, 0, 2, 0, 0),
    "_ZN12_GLOBAL__N_116layernorm_kernelILb0ELi3EEEvPKDF16_lS2_S2_PDF16_liifiii": (70, 0, 3, 0, 0),
    "_ZN12_GLOBAL__N_116layernorm_kernelILb0ELi4EEEvPKDF16_lS2_S2_PDF16_liifiii": (86, 0, 4, 0, 0),
    "_ZN12_GLOBAL__N_116layernorm_kernelILb0ELi6EEEvPKDF16_lS2_S2_PDF16_liifiii": (122, 0, 6, 0, 0),
    "_ZN12_GLOBAL__N_116layernorm_kernelILb0ELi8EEEvPKDF16_lS2_S2_PDF16_liifiii": (156, 0, 8, 0, 0),
    "_ZN12_GLOBAL__N_116layernorm_kernelILb1ELi1EEEvPKDF16_lS2_S2_PDF16_liifiii": (32, 0, 1, 0, 0),
    "_ZN12_GLOBAL__N_116layernorm_kernelILb1ELi2EEEvPKDF16_lS2_S2_PDF16_liifiii": (52, 0, 2, 0, 0),
    "_ZN12_GLOBAL__N_116layernorm_kernelILb1ELi3EEEvPKDF16_lS2_S2_PDF16_liifiii": (70, 0, 3, 0, 0),
    "_ZN12_GLOBAL__N_116layernorm_kernelILb1ELi4EEEvPKDF16_lS2_S2_PDF16_liifiii": (86, 0, 4, 0, 0),
    "_ZN12_GLOBAL__N_116layernorm_kernelILb1ELi6EEEvPKDF16_lS2_S2_PDF16_liifiii": (124, 0, 6, 0, 0),
    "_ZN12_GLOBAL__N_116layernorm_kernelILb1ELi8EEEvPKDF16_lS2_S2_PDF16_liifiii": (156, 0, 8, 0, 0),
    "_ZN12_GLOBAL__N_121layernorm_rows_kernelILi1ELi4EEEvPKDF16_lS2_S2_PDF16_liif": (54, 0, 4, 0, 0),
    "_ZN12_GLOBAL__N_121layernorm_rows_kernelILi2ELi4EEEvPKDF16_lS2_S2_PDF16_liif": (101, 0, 8, 0, 0),
    "_ZN12_GLOBAL__N_121layernorm_rows_kernelILi3ELi4EEEvPKDF16_lS2_S2_PDF16_liif": (136, 0, 12, 0, 0),
    "_ZN12_GLOBAL__N_122gn_apply_pstats_kernelILb0EEEvNS_5GnSrcENS_8GnPStatsEPKDF16_S4_PDF16_liiiiff": (97, 0, 4, 0, 0),
    "_ZN12_GLOBAL__N_122gn_apply_pstats_kernelILb1EEEvNS_5GnSrcENS_8GnPStatsEPKDF16_S4_PDF16_liiiiff": (97, 0, 8, 0, 0),
    "_ZN12_GLOBAL__N_117attention2_kernelILi160ELi4ELb0ELb0EEEv10AttnParams": (257, 0, 20, 0, 0),
    "_ZN12_GLOBAL__N_117attention2_kernelILi40ELi4ELb0ELb0EEEv10AttnParams": (128, 0, 5, 0, 0),
    "_ZN12_GLOBAL__N_117attention2_kernelILi40ELi8ELb1ELb1EEEv10AttnParams": (123, 0, 6, 0, 0),
    "_ZN12_GLOBAL__N_117attention2_kernelILi80ELi4ELb0ELb0EEEv10AttnParams": (168, 0, 10, 0, 0),
    "_ZN12_GLOBAL__N_117attention2_kernelILi96ELi4ELb0ELb0EEEv10AttnParams": (194, 0, 12, 0, 0),
    "_ZN12_GLOBAL__N_117attention3_kernelE10AttnParams": (249, 0, 12, 0, 0),
}
# a kernel whose stores go through the helper and that is missing from the table fails the test: these name parts select them
TOUCHED = ("gemm160_kernel", "gemm160ws_kernel", "conv3x3_patch_kernel", "conv3x3_patch_ws_kernel", "splitk_reduce_kernel",
           "splitk_reduce_gn_kernel", "splitk_reduce_gnorm_kernel", "attention2_kernel", "attention3_kernel", "gn_apply_kernel",
           "gn_apply_pstats_kernel", "gn_small_kernel", "layernorm_kernel", "layernorm_rows_kernel")


@pytest.mark.skipif(not HAVE_HIPCC, reason="hipcc not available")
def test_shipped_store_policies_registers_and_scratch():
    import isa_audit
    got = {k: (v["vgprs"], v["scratch"], v["plain"], v["wt"], v["nt"]) for _, k, v in isa_audit.store_policy_rows()
           if any(t in k for t in TOUCHED)}
    assert set(got) == set(SHIPPED), (sorted(set(got) - set(SHIPPED)), sorted(set(SHIPPED) - set(got)))
    diff = [f"{k}: table {SHIPPED[k]}, build {got[k]}" for k in sorted(got) if got[k] != SHIPPED[k]]
    assert not diff, "\n".join(diff)
    for part in TOUCHED:
        assert any(part in k for k in got), part
