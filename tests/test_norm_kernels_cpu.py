"""CPU: the fp64 GroupNorm reference of tests/kernel_refs.py (groupnorm_ref, groupnorm_table_ref), its per-element bound
(groupnorm_allowance with the addition depth D of gn_depth) and the case table (GN_CASES) that tests/test_norm_kernels_gpu.py
holds the stand-alone GroupNorm kernels of csrc/norm.hip to -- the reference pinned to torch's F.group_norm (+ F.silu) of the
materialised concat, the fp32 evaluations shown to stay inside the bound and every wrong variant of GN_MUTANTS outside it on
every case it applies to, the table checked against the host code itself (tools/cpu_emu: `emu_norm --dispatch`, a dry run,
pinned as tests/golden/groupnorm_dispatch.txt), and the kernel forms the suite had never run executed on the emulation
(`emu_norm --forms`)."""
import functools
import os
import re
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

import kernel_refs as KR

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get("EMU_CXX", "/opt/rocm/lib/llvm/bin/clang++")
FIXTURE = os.path.join(REPO, "tests", "golden", "groupnorm_dispatch.txt")
ALL = KR.GN_CASES
ids = [c["id"] for c in ALL]


def _rpc(c):
    return KR.gn_chunks(c["B"], c["C1"] + c["C2"], c["HW"])[1]


@functools.lru_cache(maxsize=4)
def _ref_and_bound(cid):
    p = KR.gn_problem(cid)
    ref = KR.groupnorm_ref(*KR.gn_args(p))
    return ref, KR.round_once_bound(ref, KR.groupnorm_allowance(*KR.gn_args(p), KR.gn_depth_of(p["case"])))


# ------------------------------------------------------------------------------------------------
# the reference is torch's
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ids)
def test_reference_is_torchs_group_norm(cid):
    p = KR.gn_problem(cid)
    c = p["case"]
    B, HW, C = c["B"], c["HW"], c["C1"] + c["C2"]
    x = p["x1"] if p["x2"] is None else torch.cat([p["x1"], p["x2"]], 1)
    want = F.group_norm(x.double().view(B, HW, C).permute(0, 2, 1), c["G"], p["gamma"].double(), p["beta"].double(), c["eps"])
    want = (F.silu(want) if c["silu"] else want).permute(0, 2, 1).reshape(B * HW, C)
    got = KR.groupnorm_ref(*KR.gn_args(p))
    assert got.dtype == torch.float64 and got.shape == want.shape
    # (a constant group: torch's two-pass variance is exactly 0 and so is sum of squares / n - mean^2 of these values)
    e = float((got - want).abs().max())
    assert e <= 1e-12, e
    if c["G"] == 32 and c["C2"] == 0:
        assert float((got - KR.groupnorm32_ref(x, HW, p["gamma"], p["beta"], c["eps"], c["silu"])).abs().max()) <= 1e-12
    if c["table"]:      # x * scale + shift (+ SiLU) of the table is the same function
        t = KR.groupnorm_table_ref(*KR.gn_args(p)[:-1])
        y = (x.double().view(B, HW, C) * t[:, None, 0] + t[:, None, 1]).reshape(B * HW, C)
        assert float(((F.silu(y) if c["silu"] else y) - want).abs().max()) <= 1e-11


def test_operands_are_what_the_table_says():
    for c in ALL:
        p = KR.gn_problem(c["id"])
        x = (p["x1"] if p["x2"] is None else torch.cat([p["x1"], p["x2"]], 1)).double().view(c["B"], c["HW"], -1)
        assert bool(torch.isfinite(x).all())
        cpg = x.shape[-1] // c["G"]
        if c["kind"] == "const":
            assert bool((x[..., :cpg] == 3.0).all()) and len(x[..., cpg:2 * cpg].unique()) == 1
        if c["kind"] == "tiny":                       # eps 1e-5 against 1e-6 is a different function at these variances
            var = x.reshape(c["B"], c["HW"], c["G"], cpg).var((1, 3))
            assert 1e-7 < float(var.min()) and float(var.max()) < 1e-4
        if c["strides"] is not None:
            o = KR.gn_operands(p)
            for k in ("x1", "x2"):
                v = KR.gemm_view(*o[k])
                assert v.stride(-2) > v.shape[-1] and torch.equal(v.reshape(p[k].shape), p[k]) and bool(torch.isnan(o[k][0]).any())
    a, b = KR.gn_problem("small-B4-HW64-C1280"), KR.gn_problem("two-B3-HW64-C1280")
    assert torch.equal(a["x1"][:3 * 64], b["x1"]) and torch.equal(a["gamma"], b["gamma"])


# ------------------------------------------------------------------------------------------------
# the bound: fp32 inside, every mutant outside
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ids)
def test_fp32_inside_and_mutants_outside_the_bound(cid):
    """the torch fp32 evaluations (F.group_norm, and the kernels' own sum / n, sum of squares / n - mean^2 formula) stay within the
    bound; every wrong variant that applies to the case exceeds it on some element"""
    p = KR.gn_problem(cid)
    c = p["case"]
    ref, bnd = _ref_and_bound(cid)
    B, HW, C = c["B"], c["HW"], c["C1"] + c["C2"]
    x = p["x1"] if p["x2"] is None else torch.cat([p["x1"], p["x2"]], 1)
    y32 = F.group_norm(x.float().view(B, HW, C).permute(0, 2, 1), c["G"], p["gamma"].float(), p["beta"].float(), c["eps"]).permute(0, 2, 1)
    y32 = (F.silu(y32) if c["silu"] else y32).reshape(B * HW, C)
    r_torch = float(((y32.double() - ref).abs() / bnd).max())
    r_form = float(((KR.groupnorm_ref(*KR.gn_args(p), dtype=torch.float32).double() - ref).abs() / bnd).max())
    D = KR.gn_depth_of(c)
    worst = {}
    for m in KR.GN_MUTANTS:
        if KR.gn_mutant_applies(m, c):
            y = KR.groupnorm_ref(*KR.gn_args(p), mutant=m, rpc=_rpc(c), depth=D)
            r = ((y - ref).abs() / bnd)
            worst[m] = float(torch.where(torch.isfinite(r), r, torch.full_like(r, float("inf"))).max())
    low = min(worst, key=worst.get) if worst else None
    print(f"[norm-kernels] {cid} ({c['form']}, D {D}): fp32 F.group_norm / bound {r_torch:.3f}, fp32 sums formula / bound {r_form:.3f}, "
          f"{len(worst)} mutants, smallest excess " + (f"{worst[low]:.1f} x bound ({low})" if low else "-"))
    assert r_torch <= 1.0 and r_form <= 1.0, (cid, r_torch, r_form)
    assert all(v > 1.0 for v in worst.values()), (cid, worst)


def test_mutants_apply_where_they_should():
    ap = {m: {c["form"] for c in ALL if KR.gn_mutant_applies(m, c)} for m in KR.GN_MUTANTS}
    assert ap["last_row_dropped"] == ap["last_row_twice"] == {"small", "two"}
    assert ap["chunk_last_row_dropped"] == {"two"} and ap["second_slot_skipped"] == {"two"}
    assert ap["count_from_c1"] == ap["group_by_source"] == set(KR.GN_FORMS)
    assert ap["eps_1e-5"] == {"two"} and ap["eps_omitted"] >= {"small", "two", "pstats_par"}
    assert ap["var_not_clamped"] == {"small", "two"} and ap["silu_before_affine"] == set(KR.GN_FORMS)
    assert ap["slab_without_sample_offset"] == ap["second_producer_group_dropped"] == {"pstats_par", "pstats_plain"}


def test_depth_follows_the_loops():
    """D of a few cases by hand from the loops of csrc/norm.hip"""
    assert KR.gn_depth("small", 4, 64, 1280, 0, 32) == 32 + 6 + 16 + 3
    # 3 x 37 x 256: 32 vectors, RT 8, 2 chunks of 19 rows: one sweep (8), 8 row threads, 8 channels, 1 chunk per part, P = 8
    assert KR.gn_chunks(3, 256, 37) == (2, 19) and KR.gn_depth("two", 3, 37, 256, 0, 32) == 8 + 8 + 8 + 1 + 8 + 3
    # 1 x 4096 x 320: 40 vectors, RT 6, 171 chunks of 24 rows: one sweep, 6, 10 channels, 22 chunks per part, 8
    assert KR.gn_chunks(1, 320, 4096) == (171, 24) and KR.gn_depth("two", 1, 4096, 320, 0, 32) == 8 + 6 + 10 + 22 + 8 + 3
    assert KR.gn_chunks(1, 2048, 1100) == (220, 5) and KR.gn_chunks(1, 128, 1089) == (18, 61) and KR.gn_chunks(1, 4096, 5) == (2, 3)
    # 64 slabs over 8 parts: one trip of 8 slabs, two additions each; 72 slabs: two trips
    assert KR.gn_depth("pstats_par", 1, 4096, 320, 0, 32) == 1 + 16 + 8 + 3 and KR.gn_depth("pstats_par", 1, 4608, 320, 0, 32) == 1 + 32 + 8 + 3
    # G 24: P = 10, 2 slabs: one per part, 4 producer groups of the second source
    assert KR.gn_depth("pstats_plain", 2, 128, 1280, 640, 24) == 1 + 4 + 10 + 3
    # the longest chain of the table: one group of 64 channels on P = 256 parts (n = 2112 values per group there; the UNet's
    # own shapes have n up to 40960 against D <= 75)
    assert max(KR.gn_depth_of(c) for c in ALL) == KR.gn_depth("two", 2, 33, 64, 0, 1) == 8 + 32 + 64 + 1 + 256 + 3


def test_plain_pstats_loop_is_unreachable_at_32_groups():
    """pfd_groupnorm_takes_pstats admits no shape with G = 32 whose group spans more than two producer groups of a source (a
    group of the concat is a whole number of producer groups of BOTH sources only where C2 = 0 or C2 = C1), so
    gn_apply_pstats_kernel<false> is reached through the C ABI alone -- the three plain-loop cases go through `binding`"""
    n = 0
    for C1 in range(160, 4097, 160):
        for C2 in range(0, 4097 - C1, 160):
            for B, HW in ((1, 64), (2, 1024), (8, 4096)):
                if KR.gn_takes_pstats(B, C1, C2, HW, 32):
                    n += 1
                    assert max(KR.gn_producer_groups(C1, C2, 32)) <= 2 and KR.gn_form(B, HW, C1, C2, 32, True) == "pstats_par"
    assert n > 20
    assert {c["G"] for c in ALL if c["form"] == "pstats_plain"} == {8, 16, 24}


# ------------------------------------------------------------------------------------------------
# the cases reach what they are listed for
# ------------------------------------------------------------------------------------------------
def _dispatch_requests():
    """one line per launch the GPU file makes: id, entry point (gn | pstats | table), B HW C1 C2 G"""
    lines = []
    for c in ALL:
        api = "pstats" if c["form"].startswith("pstats") else "gn"
        lines.append(f"{c['id']} {api} {c['B']} {c['HW']} {c['C1']} {c['C2']} {c['G']}")
        if c["table"]:
            lines.append(f"{c['id']}/table table {c['B']} {c['HW']} {c['C1']} {c['C2']} {c['G']}")
    return lines


@pytest.fixture(scope="module")
def emu_norm(tmp_path_factory):
    if not os.path.exists(CXX):
        pytest.skip("clang++ of the ROCm toolchain not available")
    out = str(tmp_path_factory.mktemp("pfd_cpu_emu_norm"))
    subprocess.run([sys.executable, os.path.join(REPO, "tools", "cpu_emu", "build.py"), out], check=True, stdout=subprocess.DEVNULL,
                   env=dict(os.environ, EMU_ONLY="emu_norm"))
    return os.path.join(out, "emu_norm")


@pytest.fixture(scope="module")
def dispatch(emu_norm, tmp_path_factory):
    req = os.path.join(str(tmp_path_factory.mktemp("gn_requests")), "groupnorm_requests.txt")
    open(req, "w").write("\n".join(_dispatch_requests()) + "\n")
    r = subprocess.run([emu_norm, "--dispatch", req], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout


def test_dispatch_is_pinned(dispatch):
    """what pfd_groupnorm_f16 / pfd_groupnorm_pstats_f16 / pfd_groupnorm_table_f16 decide for every request of the table --
    kernel, grid, block, return value -- against tests/golden/groupnorm_dispatch.txt (PFD_GN_DISPATCH_WRITE=1 rewrites it)"""
    if os.environ.get("PFD_GN_DISPATCH_WRITE") == "1":
        open(FIXTURE, "w").write(dispatch)
    want = open(FIXTURE).read().splitlines()
    got = dispatch.splitlines()
    diff = [f"line {i + 1}:\n  fixture: {w}\n  probe:   {g}" for i, (w, g) in enumerate(zip(want, got)) if w != g]
    assert not diff and len(got) == len(want), f"{len(diff)} lines differ, {len(got)} against {len(want)}\n" + "\n".join(diff[:5])


def test_cases_take_the_form_the_table_says():
    """every case against the pinned dry run: return value 0, the kernels of its form in order, the grid that gn_chunks (restated
    in kernel_refs) gives; and every gn_ kernel of csrc/norm.hip is launched by some case"""
    seen, by_id = set(), {}
    for line in open(FIXTURE).read().splitlines():
        m = re.match(r"^(\S+) (gn|pstats|table) (\d+) (\d+) (\d+) (\d+) (\d+) -> (-?\d+)(.*)$", line)
        assert m, line
        launches = [re.match(r"^(\S+) grid (\d+)x(\d+) block (\d+)$", l.strip()) for l in m.group(9).split(" | ")[1:]]
        assert all(launches), line
        by_id[m.group(1)] = (int(m.group(8)), [(l.group(1), int(l.group(2)), int(l.group(3)), int(l.group(4))) for l in launches])
    for c in ALL:
        B, HW, C, G = c["B"], c["HW"], c["C1"] + c["C2"], c["G"]
        assert c["form"] == KR.gn_form(B, HW, c["C1"], c["C2"], G, c["form"].startswith("pstats")), c["id"]
        nchunks, _ = KR.gn_chunks(B, C, HW)
        for key, form in ((c["id"], c["form"]),) + (((c["id"] + "/table", "table"),) if c["table"] else ()):
            rc, ls = by_id[key]
            want = [(k, G, B, KR.GNS_T) if k == "gn_small_kernel" else (k, B, 1, 256) if k == "gn_table_kernel" else (k, nchunks, B, 256)
                    for k in KR.GN_FORM_KERNELS[form]]
            assert rc == 0 and ls == want, (key, rc, ls, want)
            seen.update(k for k, *_ in ls)
    src = open(os.path.join(REPO, "prompt-free-diffusion_amd", "csrc", "norm.hip")).read()
    kernels = set(re.findall(r"__global__[^{;]*?\bvoid (gn_\w+)\(", src))
    assert kernels == {"gn_stats_kernel", "gn_apply_kernel", "gn_apply_pstats_kernel", "gn_table_kernel", "gn_small_kernel"}
    assert {k.split("<")[0] for k in seen} == kernels and {"gn_apply_pstats_kernel<true>", "gn_apply_pstats_kernel<false>"} <= seen
    assert len(by_id) == len(_dispatch_requests())


def test_kernel_forms_on_the_emulation(emu_norm):
    """csrc/norm.hip on the emulation, against its double-precision GroupNorm: a two-launch case with both vector slots, the
    table kernel, the plain-loop apply from producer statistics (G = 8) and a case with constant groups"""
    r = subprocess.run([emu_norm, "--forms"], capture_output=True, text=True, timeout=900)
    lines = [l for l in r.stdout.splitlines() if l.startswith(("ok", "FAIL"))]
    assert r.returncode == 0 and len(lines) == 4, r.stdout[-3000:] + r.stderr[-1000:]
    assert all(l.startswith("ok") for l in lines), "\n".join(lines)
