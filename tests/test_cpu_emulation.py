"""CPU emulation of the wide-tile GEMM / convolution kernels (tools/cpu_emu): the kernel file csrc/gemm_glds.hip is compiled
for the HOST against a shim of the HIP runtime -- one OS thread per GPU thread of a block, MFMA / shuffles / ballot as
rendezvous of a wave's 64 threads, LDS as block-shared statics, real barriers -- and the library's own dispatcher
(pfd_gemm160_try, forced variants, split-K) runs small problems through it.  Checked against a double-precision reference,
and the split-K reduction with the fused GroupNorm (round 5) against the plain reduction + a double-precision GroupNorm.
What the model cannot see: s_waitcnt counts (tests/test_isa_audit.py covers the compiler's), register allocation, timing."""
import os
import subprocess
import sys

import numpy as np
import pytest

import kernel_refs as KR
import refmix_refs as RR
import regions_refs as GR

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get("EMU_CXX", "/opt/rocm/lib/llvm/bin/clang++")

pytestmark = pytest.mark.skipif(not os.path.exists(CXX), reason="clang++ of the ROCm toolchain not available")


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("pfd_cpu_emu"))
    subprocess.run([sys.executable, os.path.join(REPO, "tools", "cpu_emu", "build.py"), out], check=True,
                   stdout=subprocess.DEVNULL)
    return os.path.join(out, "emu_gemm")


def test_groupnorm_kernels_on_the_emulation(emu):
    """csrc/norm.hip on the same emulation: the single-launch small-slab GroupNorm and the apply from producer statistics
    (grouped partial loads, adopted in round 5) against a double-precision GroupNorm"""
    r = subprocess.run([os.path.join(os.path.dirname(emu), "emu_norm"), "--quick"], capture_output=True, text=True, timeout=900)
    lines = [l for l in r.stdout.splitlines() if l.startswith(("ok", "FAIL"))]
    assert r.returncode == 0 and len(lines) == 5, r.stdout[-3000:] + r.stderr[-1000:]
    assert all(l.startswith("ok") for l in lines), "\n".join(lines)


def _run(emu, *filters):
    r = subprocess.run([emu, *filters], capture_output=True, text=True, timeout=900)
    lines = [l for l in r.stdout.splitlines() if l.startswith(("ok", "FAIL"))]
    assert r.returncode == 0 and lines and not any(l.startswith("FAIL") for l in lines), r.stdout[-3000:] + r.stderr[-1000:]
    return lines


def test_emulation_reproduces_the_hardware_validated_kernels(emu):
    lines = _run(emu, "variant 23 (", "variant 83 (", "variant 98", "variant 96", "variant 99")
    assert len(lines) == 6                                               # (96 also with K-tile-contiguous weights)
    assert sum("== variant 98 bitwise" in l for l in lines) == 2      # 3-stage ring and 8-wave forms of the patch kernel


def test_statistics_emitting_splitk_reduce(emu):
    """split-K reduction that also emits the GroupNorm statistics of what it stores (three row sweeps of loads in flight):
    statistics == sums of the stored f16 values"""
    lines = _run(emu, "statistics")
    assert len(lines) == 2 and all("statistics err" in l for l in lines), "\n".join(lines)


def test_residual_stored_once_for_a_doubled_batch(emu):
    """PfdGemmDesc.res_rows (ABI 9): the store pass, the store pass behind zero rows (the cross-attention re-join of a CFG pair)
    and the plain split-K reduction read residual row m - res_rows for the second half"""
    lines = _run(emu, "residual read with one wrap")
    assert len(lines) == 3, "\n".join(lines)


def test_splitk_reduce_with_fused_groupnorm(emu):
    """PfdGemmDesc.gnf_y (ABI 9, round 5): the split-K reduction whose blocks own (sample, group) slabs and normalise them in
    the same launch -- ring kernel, 4-wave ring with residual and raw tensor kept, patch kernel: raw result bit for bit the
    plain reduction's (or not written at all), normalised tensor == GroupNorm(32) + SiLU of it in double precision, and the
    same request on the unsplit problem declined with nothing written"""
    # (one of the three cases of tools/cpu_emu/emu_gemm here -- a minute of emulation each; `emu_gemm "fused GroupNorm"` runs all,
    #  `selftest --r5` runs the real shapes on hardware)
    lines = _run(emu, "fused GroupNorm: split-K 2 conv 4x4x128")
    assert len(lines) == 1 and all("unsplit request declined, nothing written" in l for l in lines), "\n".join(lines)


DISPATCH_SHAPES = ("unet_c2_gemm_shapes.txt", "ups_phase_fold_shapes.txt", "lin_shapes_ablation.txt", "r06_fixed_cost_probe_shapes.txt")


def test_dispatch_table_is_pinned(emu):
    """what pfd_gemm160_try decides -- kernel instantiation, grid, split count, the G160Params it hands over -- for every record of
    the tracked launch lists under the heuristic, for hand-written requests (LayerNorm fold, transposed tail, GroupNorm
    prologue, tiled weights, 128-wide problems, requests that must be declined) and for a dozen records under every forced
    variant: `emu_gemm --dispatch` (a dry run: nothing is emulated) against tests/golden/gemm_dispatch.txt, line for line.
    A change of the heuristic regenerates the fixture and shows up as a reviewed diff of it.
    The kernel names in the text ("gemm160_kernel<4, 4, false, 2, 5>") are the demangled type name of a tag template, cut to size by
    emu::kernel_name (tools/cpu_emu/hip/hip_runtime.h): if EVERY line differs, and only in how those names are spelled, after a
    compiler / C++ runtime update, the demangler's format moved, not the dispatcher."""
    files = [os.path.join(REPO, "profiles", f) for f in DISPATCH_SHAPES]
    r = subprocess.run([emu, "--dispatch"] + files, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    got = r.stdout.splitlines()
    want = open(os.path.join(REPO, "tests", "golden", "gemm_dispatch.txt")).read().splitlines()
    diff = [f"line {i + 1}:\n  fixture: {w}\n  probe:   {g}" for i, (w, g) in enumerate(zip(want, got)) if w != g]
    assert not diff and len(got) == len(want), f"{len(diff)} lines differ, {len(got)} lines against {len(want)} in the fixture\n" + "\n".join(diff[:5])


# the run_attn_* shapes of csrc/selftest.cpp that ATTN_CASES does not have
SELFTEST_ATTN_SHAPES = [(2, 2, 128, 128, 40), (2, 2, 512, 256, 40), (1, 1, 256, 40, 40), (1, 2, 520, 1000, 40), (1, 2, 77, 64, 40), (1, 2, 200, 148, 40),
                        (1, 2, 512, 1024, 40), (1, 1, 700, 640, 40), (2, 1, 256, 256, 512)]
# the dispatch rule's edges, each from both sides
ATTN_EDGE_SHAPES = [(32, 8, 256, 64, 40), (32, 8, 256, 128, 40), (32, 8, 256, 200, 40),            # a3: Nk = 64 | 128, Nk % 64
                    (32, 8, 255, 128, 40), (51, 5, 256, 128, 40),                                  # a3: Nq = 255 | 256, 255 | 256 blocks
                    (16, 8, 1023, 148, 40), (16, 8, 1024, 148, 40), (73, 1, 1792, 148, 40),        # w8: Nq = 1023 | 1024, 511 | 512 blocks
                    (73, 1, 1792, 1024, 40), (16, 8, 1024, 1024, 40),                              # ... where a3 takes the plain operand
                    (1, 2, 128, 64, 512), (1, 1, 128, 64, 512), (1, 1, 128, 40, 512),              # d = 512: H = 2 | 1, Nk = 40 | 64
                    (1, 2, 128, 128, 64)]                                                          # no such head dim
# what the product launches: the UNet levels (8 heads, a CFG pair and a batch of 8; self-attention and the 148 context tokens) at
# every head dim, SeeCoder's d = 96, the VAE mid-block at 64^2 and 96^2
ATTN_PRODUCT_SHAPES = ([(B, 8, N, Nk, D) for D in (40, 80, 160) for N in (4096, 1024, 256, 64) for Nk in (N, 148) for B in (2, 8)]
                       + [(1, 8, 144, 256, 96), (1, 8, 148, 148, 96), (1, 8, 4, 144, 96)]
                       + [(B, 1, N, N, 512) for N in (4096, 9216) for B in (1, 2)])


def attention_dispatch_requests():
    """the request lines of `emu_attn --dispatch`: every shape above and of the test case lists through all three entry points
    (d = 512 on the plain one with PFD_ATTN512_SLICES unset, 2 and 4), then the calls that must be declined, next to one that is
    not"""
    shapes = [c[:5] for c in KR.ATTN_CASES] + [c for _, c in RR.ALL_CASES] + [c for _, c in GR.ALL_CASES] + [GR.W8_SHAPE]
    shapes = list(dict.fromkeys(shapes + SELFTEST_ATTN_SHAPES + ATTN_EDGE_SHAPES + ATTN_PRODUCT_SHAPES))
    lines = []
    for c in shapes:
        dims = "%d %d %d %d %d" % c
        lines += [f"plain {dims}"] + ([f"plain {dims} slices=2", f"plain {dims} slices=4"] if c[4] == 512 else [])
        lines += [f"kbias {dims}", f"rbias {dims}"]
    ok = "1 2 130 148 40"                      # C = 80; kb_bs = rb_rs = 152, nr = 2 where the request does not say
    for api in ("plain", "kbias", "rbias"):    # check_desc
        lines += [f"{api} {ok} null=O", f"{api} {ok} ldk=84", f"{api} {ok} misalign=K", f"{api} 0 2 130 148 40"]
    lines += [f"kbias {ok} null=bias", f"kbias {ok} misalign=bias", f"kbias {ok} kb_bs=150", f"kbias {ok} kb_bs=144", f"kbias {ok} kb_bs=148",
              f"kbias {ok} scale=0", f"rbias {ok} scale=0"]
    lines += [f"rbias {ok} nr=0", f"rbias {ok} nr=1", f"rbias {ok} nr=8", f"rbias {ok} nr=9", f"rbias {ok} misalign=bias", f"rbias {ok} rb_rs=150",
              f"rbias {ok} rb_rs=144", f"rbias {ok} rb_bs=302", f"rbias {ok} rb_bs=300", f"rbias {ok} rb_bs=0", f"rbias {ok} null=qregion",
              f"rbias {ok} qr_bs=129", f"rbias {ok} qr_bs=0"]
    # scale log2(e) = 2^-28 and 2^10 exactly in fp32 (declined), and the neighbouring fp32 scale inside the range
    log2e = np.float32(KR.LOG2E)
    for edge, inside in ((2.0 ** -28, np.inf), (2.0 ** 10, 0.0)):
        s = np.float32(edge) / log2e
        assert float(s * log2e) == edge
        lines += [f"rbias {ok} scale={float(s).hex()}", f"rbias {ok} scale={float(np.nextafter(s, np.float32(inside))).hex()}"]
    return lines


ATTN_DISPATCH_HOOKS = ((), ("PFD_ATTN_FORCE8",), ("PFD_ATTN3_FORCE",), ("PFD_ATTN_FORCE8", "PFD_ATTN3_FORCE"))


def test_attention_dispatch_is_pinned(emu, tmp_path):
    """what pfd_attention_f16 / pfd_attention_kbias_f16 / pfd_attention_rbias_f16 decide -- return value, kernel instantiation,
    grid, block -- for every request of attention_dispatch_requests(): `emu_attn --dispatch` (a dry run: nothing is emulated)
    against tests/golden/attention_dispatch.txt, line for line.  PFD_ATTN_FORCE8 and PFD_ATTN3_FORCE are read once per process:
    one run and one section of the fixture per setting (PFD_ATTN_DISPATCH_WRITE=1 rewrites it).  A change of the rule
    regenerates the fixture and shows up as a reviewed diff of it; for kernel names that all change their spelling see
    test_dispatch_table_is_pinned."""
    req = tmp_path / "attention_requests.txt"
    req.write_text("\n".join(attention_dispatch_requests()) + "\n")
    env = {k: v for k, v in os.environ.items() if not k.startswith("PFD_ATTN")}
    got = []
    for hooks in ATTN_DISPATCH_HOOKS:
        r = subprocess.run([os.path.join(os.path.dirname(emu), "emu_attn"), "--dispatch", str(req)], capture_output=True, text=True, timeout=60,
                           env=dict(env, **{h: "1" for h in hooks}))
        assert r.returncode == 0, r.stderr[-2000:]
        got += ["# hooks: " + (" ".join(h + "=1" for h in hooks) or "none")] + r.stdout.splitlines()
    fixture = os.path.join(REPO, "tests", "golden", "attention_dispatch.txt")
    if os.environ.get("PFD_ATTN_DISPATCH_WRITE") == "1":
        open(fixture, "w").write("\n".join(got) + "\n")
    want = open(fixture).read().splitlines()
    diff = [f"line {i + 1}:\n  fixture: {w}\n  probe:   {g}" for i, (w, g) in enumerate(zip(want, got)) if w != g]
    assert not diff and len(got) == len(want), f"{len(diff)} lines differ, {len(got)} lines against {len(want)} in the fixture\n" + "\n".join(diff[:5])


def test_attention_kernels_on_the_emulation(emu):
    """csrc/attention.hip on the same emulation (v_mfma_f32_32x32x16_f16, v_permlane16_swap, 16-byte clears of the LDS image):
    the 8-wave d = 40 form and the 4-wave forms against a double-precision softmax(Q K^T) V at d = 40 / 80 / 96 / 160 with
    ragged query / key counts"""
    exe = os.path.join(os.path.dirname(emu), "emu_attn")
    # --a3 (round 6): attention3_kernel, the software-pipelined 64-queries-per-wave d = 40 form, incl. two deferred-rescale cases
    for extra, n in (([], 5), (["--quick", "--w4"], 2), (["--a3"], 7)):
        r = subprocess.run([exe] + extra, capture_output=True, text=True, timeout=900)
        lines = [l for l in r.stdout.splitlines() if l.startswith(("ok", "FAIL"))]
        assert r.returncode == 0 and len(lines) == n and all(l.startswith("ok") for l in lines), r.stdout[-2000:] + r.stderr[-1000:]
