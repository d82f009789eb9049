"""GPU (-m gpu): every output store that goes through the policy helper of csrc/pfd_common.h (gst / gst_t),
at the smallest shapes that reach each store path, launched as the other kernel files do (ops.gemm / ops.conv through
pfd_gemm_f16_ex, ops.attention, ops.groupnorm, ops.layernorm) and held to the fp64 references and bounds of
tests/kernel_refs.py.

What is particular to this file: every case runs TWICE into the same output buffer (and, for split-K, the same workspace:
lib.hip.ops keeps one), on operands from two different seeds, with a launch that reads the whole first result (a device copy)
queued between the two and no host synchronisation anywhere in the chain; both results are then checked.  A store that is
lost, that lands late (after the consumer's read, or after the second launch's store of the same address) or that is
overtaken shows up as an element of the other seed's result, far outside the bound.

The stores reached: the split-K slab branch and the final store pass of epilogue_store (64 x 160 and 128-wide tiles, row
guard at M = 72), its ln_out, gn_out and GEGLU passes and the transposed tail; the three reduction kernels (plain, gn_out,
fused GroupNorm keeping and skipping the raw result) behind the 3x3 patch kernel; store_o of attention3_kernel and the
attention2_kernel epilogue; gn_apply_pstats_kernel and layernorm_kernel.  The fused GroupNorm reduction serves groups of
20 ... 256 channels (a multiple of four) and at least four samples (128 blocks), so those two cases run at 4 x 16 x 16 and
N = 640 instead of 1 x 16 x 16 and N = 160; statistics (gn_out) are emitted for groups of at least eight channels, so that
case runs at N = 320.  attention3_kernel takes a 128 x 128 problem only under the process-static hook
PFD_ATTN3_FORCE=1: that case runs this file as a child process."""
import os
import subprocess
import sys
import zlib

import pytest
import torch

if __name__ == "__main__":        # the PFD_ATTN3_FORCE child: the paths tests/conftest.py sets up
    _repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for _p in (os.path.join(_repo, "prompt-free-diffusion_amd"), os.path.join(_repo, "oracle"), _repo, os.path.join(_repo, "tests")):
        if _p not in sys.path:
            sys.path.insert(0, _p)
    os.environ.setdefault("PFD_QUIET", "1")

import kernel_refs as KR
import test_gemm_kernels_gpu as G

pytestmark = pytest.mark.gpu

SENTINEL = G.SENTINEL
SEEDS = (1, 2)


# ------------------------------------------------------------------------------------------------
# GEMM / convolution
# ------------------------------------------------------------------------------------------------
def _cases():
    C = {}

    def lin(name, cls, v, s, M, N, K, **kw):
        C[name] = KR._wide(name, cls, v, s, M, N, K, **kw)

    # 64 x 160 tile (forced variant 41: gemm160_kernel<4, 1, false, 2, 5>), K = 128 = two K tiles
    for M in (64, 72):
        for s in (1, 2):
            for res in (False, True):
                lin(f"lin160-{M}x160x128-split{s}{'-res' if res else ''}", "lin160", 41, s, M, 160, 128, bias=True, res=res)
    for s in (1, 2):
        lin(f"lin160-72x160x128-split{s}-ln_out", "abi", 41, s, 72, 160, 128, bias=True, res=True, ln_out=True)
        lin(f"lin160-64x320x128-split{s}-gn_out", "abi", 41, s, 64, 320, 128, bias=True, res=True, gn_out=True)
    lin("lin160-72x320x128-geglu", "geglu", 41, 1, 72, 320, 128, bias=True, act=KR.ACT_GEGLU)
    lin("lin160-72x320x128-tail160", "abi", 41, 1, 72, 320, 128, bias=True, n_split=160)
    # 128-wide tile (forced variant 22: gemm160_kernel<2, 2, false, 2, 4>)
    for s in (1, 2):
        lin(f"lin128-72x128x128-split{s}-res", "lin128", 22, s, 72, 128, 128, bias=True, res=True)
    # 3x3 patch convolution, 1 x 16 x 16, Cin = 128, two slabs of one channel block each, into each reduction kernel
    geo, M, K, hw = KR._conv_geom(1, 16, 16, 128)
    for v in PATCH_FORMS:
        lin(f"patch-n160-split2-v{v}", "patch", v, 2, M, 160, K, conv=True, rows_per_rv=hw, bias=True, rowvec=True, res=True, **geo)
    lin("patch-n320-split2-gn_out", "patch", 0, 2, M, 320, K, conv=True, rows_per_rv=hw, bias=True, res=True, gn_out=True,
        kernel="conv3x3_patch_ws_kernel<0, 3>", **geo)
    geo, M, K, hw = KR._conv_geom(4, 16, 16, 128)
    for keep in (True, False):
        lin(f"patch-4x16x16-n640-split2-gnf-{'raw-kept' if keep else 'raw-skipped'}", "patch", 0, 2, M, 640, K, conv=True, rows_per_rv=hw,
            gnf=keep, bias=True, rowvec=True, res=keep, kernel="conv3x3_patch_ws_kernel<0, 3>", **geo)
    return C


PATCH_FORMS = (96, 98, 99)          # 3-stage / 2-stage loader-wave kernels, the 8-wave kernel: one split count, the same bits
CASES = _cases()


def _problem(c, seed):
    """operands as kernel_refs.gemm_problem draws them (unit Gaussians against K^-0.5 weights), from (case, seed)"""
    M, N, K = c["M"], c["N"], c["K"]
    g = torch.Generator().manual_seed(zlib.crc32(f"{KR.gemm_problem_key(c['id'])}/seed{seed}".encode()))
    rn = lambda *s: torch.randn(s, generator=g)
    p = dict(case=c, A2=None, bias=None, rowvec=None, R=None, gn_table=None)
    p["A"] = (rn(*c["image"]) if c["kind"] == "conv" else rn(M, K)).half()
    p["W"] = (rn(N, K) * K ** -0.5).half()
    if c["bias"]:
        p["bias"] = (0.5 * rn(N)).half()
    if c["rowvec"]:
        p["rowvec"] = (0.5 * rn(-(-M // c["rows_per_rv"]), N)).half()
    if c["res"]:
        p["R"] = rn(M, N // 2 if c["act"] == KR.ACT_GEGLU else N).half()
    if c["gnf"] is not None:
        p["gnf_gamma"], p["gnf_beta"] = (1 + 0.2 * rn(N)).half(), (0.1 * rn(N)).half()
    return p


def _launch(p, d, out, out_t):
    """G._launch; a convolution that emits GroupNorm statistics as tests/test_patch_pipeline_gpu.py launches it"""
    c = p["case"]
    if not (c["kind"] == "conv" and c["gn_out"]):
        return G._launch(p, d, out, out_t)
    from lib.hip import ops
    ks, stride, pad, ups, Ho, Wo = c["geom"]
    r = ops.conv(d["A"], d["W"], ks, stride=stride, pad=pad, bias=d["bias"], rowvec=d["rowvec"], res=d["R"], out=out, tile=c["tile"],
                 out_hw=(Ho, Wo), gn_out=True)
    st = ops.get_gn_stats(r)
    assert st is not None
    return dict(out=r, gn_out=st)


_ran = {}


def _run_twice(name):
    """-> [(problem, outputs on the CPU)] for the two seeds; see the module docstring"""
    if name in _ran:
        return _ran[name]
    c = CASES[name]
    M, N = c["M"], c["N"]
    ps = [_problem(c, s) for s in SEEDS]
    ds = [G._device_operands(p) for p in ps]
    buf, out, tbuf, n_out = G._outputs(c)
    out_t = None if tbuf is None else tbuf[:N - c["n_split"]]
    torch.cuda.synchronize()
    snaps = []
    for p, d in zip(ps, ds):
        r = _launch(p, d, out, out_t)
        snap = dict(buf=buf.clone())                       # the consumer launch: reads everything the producer stored
        if tbuf is not None:
            snap["tbuf"] = tbuf.clone()
        for k in ("ln_out", "gn_out", "gnf_y"):
            if k in r:
                snap[k] = r[k].clone()
        snaps.append(snap)
    torch.cuda.synchronize()
    res = []
    for p, s in zip(ps, snaps):
        b = s["buf"]
        assert bool((b[M:] == SENTINEL).all()), "rows behind the last row were written"
        assert bool((b[:M, :8] == SENTINEL).all()) and bool((b[:M, 8 + n_out:] == SENTINEL).all()), "columns outside the slice were written"
        got = {}
        if c["gnf"] is not None and not c["gnf"]:
            assert bool((b == SENTINEL).all()), "gnf_skip_raw: the raw result was stored"
        else:
            got["out"] = b[:M, 8:8 + n_out].contiguous().cpu()
        if "tbuf" in s:
            t = s["tbuf"]
            assert bool((t[N - c["n_split"]:] == SENTINEL).all()) and bool((t[:, M:] == SENTINEL).all()), "the tail wrote outside [N - n_split, M]"
            got["out_t"] = t[:N - c["n_split"], :M].contiguous().cpu()
        for k in ("ln_out", "gn_out", "gnf_y"):
            if k in s:
                got[k] = s[k].cpu()
        for k in ("out", "out_t", "gnf_y"):
            if k in got:
                assert bool(torch.isfinite(got[k]).all()) and not bool((got[k] == SENTINEL).any()), f"{k}: an element was not written"
        res.append((p, got))
    _ran[name] = res
    return res


def _ratios(p, got):
    """worst error / bound of every output of one launch (the checks of tests/test_gemm_kernels_gpu.py)"""
    c = p["case"]
    M, N = c["M"], c["N"]
    ref = KR.gemm_ref(p)
    a = KR.gemm_allowance(p, c["splits"], True)
    parts = {}
    for k in ("out", "out_t"):
        if k in got:
            parts[k] = KR.bound_ratio(got[k], ref[k], a[k])[0]
    stored = got.get("out")
    if "ln_out" in got:                 # fp32 sums of 160 stored values
        want = KR.ln_out_ref(stored)
        v = stored.double().reshape(M, N // 160, 160)
        bnd = 160 * 2.0 ** -24 * torch.stack([v.abs().sum(-1), (v * v).sum(-1)], -1)
        parts["ln_out"] = float(((got["ln_out"].double().reshape(want.shape) - want).abs() / bnd).max())
    if "gn_out" in got:                 # fp32 sums of 64 N / 32 stored values
        cpg = N // 32
        want = KR.gn_out_ref(stored)[:, :, :160 // cpg]
        v = stored.double().reshape(M // 64, 64, N // 160, 160 // cpg, cpg)
        bnd = 64 * cpg * 2.0 ** -24 * torch.stack([v.abs().sum((1, 4)), (v * v).sum((1, 4))], -1)
        g = got["gn_out"].reshape(M // 64, N // 160, 16, 2)[:, :, :160 // cpg]
        parts["gn_out"] = float(((g.double() - want).abs() / bnd).max())
    if "gnf_y" in got:                  # GroupNorm(32) + SiLU of the stored raw values, or of the reference where they are not stored
        rows = c["geom"][4] * c["geom"][5]
        src, dx = (stored, 0.0) if c["gnf"] else (ref["out"], float(KR.round_once_bound(ref["out"], a["out"]).max()))
        want = KR.groupnorm32_ref(src, rows, p["gnf_gamma"], p["gnf_beta"], 1e-5, True)
        ay = KR.groupnorm32_allowance(src, rows, p["gnf_gamma"], p["gnf_beta"], 1e-5, True, dx)
        parts["gnf_y"] = KR.bound_ratio(got["gnf_y"].reshape(want.shape), want, ay)[0]
    return parts


@pytest.mark.parametrize("name", sorted(CASES))
def test_gemm_twice_into_the_same_buffers(name):
    worst = 0.0
    for seed, (p, got) in zip(SEEDS, _run_twice(name)):
        parts = _ratios(p, got)
        print(f"[store-policy] {name} seed {seed} splits {p['case']['splits']}: " + ", ".join(f"{k} err / bound {v:.3f}" for k, v in parts.items()))
        worst = max([worst] + list(parts.values()))
    assert worst <= 1.0, (name, worst)


def test_patch_forms_of_one_split_count_are_bitwise_equal():
    base = _run_twice(f"patch-n160-split2-v{PATCH_FORMS[-1]}")
    assert len({CASES[f"patch-n160-split2-v{v}"]["splits"] for v in PATCH_FORMS}) == 1
    for v in PATCH_FORMS[:-1]:
        for seed, (_, g), (_, b) in zip(SEEDS, _run_twice(f"patch-n160-split2-v{v}"), base):
            n = int((g["out"] != b["out"]).sum())
            assert n == 0, f"form {v}, seed {seed}: differs from form {PATCH_FORMS[-1]} in {n} elements"


# ------------------------------------------------------------------------------------------------
# attention
# ------------------------------------------------------------------------------------------------
ATTN3_DIMS = (1, 2, 128, 128, 40)       # attention3_kernel under PFD_ATTN3_FORCE=1 (two 64-key tiles, half a query block)
ATTN2_DIMS = (1, 2, 150, 148, 80)       # attention2_kernel<80, 4, false>


def _attn_twice(dims, folded):
    """the two layouts of one shape (their seeds differ) into one output buffer; -> [(layout, err / bound(, / sharp bound))]"""
    import test_attention_kernels_gpu as AT
    B, H, Nq, Nk, D = dims
    C, M = H * D, B * Nq
    ps = [KR.attention_problem(dims + (layout, 0)) for layout in ("dense", "fused_qk")]
    devs = [AT._operands(p) for p in ps]
    buf = torch.full((M + 16, C + 16), SENTINEL, dtype=torch.float16, device="cuda")
    torch.cuda.synchronize()
    snaps = []
    for p, dev in zip(ps, devs):
        AT._launch(p, dev, out=buf[:M, 8:8 + C])
        snaps.append(buf.clone())
    torch.cuda.synchronize()
    res = []
    for p, dev, b in zip(ps, devs, snaps):
        assert bool((b[M:] == SENTINEL).all()) and bool((b[:M, :8] == SENTINEL).all()) and bool((b[:M, 8 + C:] == SENTINEL).all())
        got = b[:M, 8:8 + C].contiguous()
        assert bool(torch.isfinite(got).all()) and not bool((got == SENTINEL).any())
        q, k, vt = dev
        ref = KR.attention_ref(q, k, vt, B, H, Nq, Nk, D, p["scale"], **p["desc"]).view(M, C)
        A = KR.attention_fold_amplitude(q, k, B, H, Nq, Nk, D, p["scale"], **p["desc"]) if folded else 0.0
        r = [AT._ratio(got, ref, KR.attention_bound(Nk, p["vmax"], A))]
        if folded:
            reff = KR.attention_ref_folded(q, k, vt, B, H, Nq, Nk, D, p["scale"], **p["desc"]).view(M, C)
            r.append(AT._ratio(got, reff, KR.attention_bound(Nk, p["vmax"])))
        res.append(r)
    return res


def test_attention2_twice_into_the_same_buffer():
    assert KR.attention_kernel_class(*ATTN2_DIMS) == "d80"
    for layout, r in zip(("dense", "fused_qk"), _attn_twice(ATTN2_DIMS, False)):
        print(f"[store-policy] attention2 {ATTN2_DIMS} {layout}: err / bound {r[0]:.3f}")
        assert max(r) <= 1.0, (layout, r)


def test_attention3_twice_into_the_same_buffer():
    """in a child process: the hook is read once per process, and this one may have launched attention already"""
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "attention3"], env=dict(os.environ, PFD_ATTN3_FORCE="1"),
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-2000:]
    assert r.stdout.count("[store-policy] attention3") == 2


def _attention3_child():
    assert os.environ.get("PFD_ATTN3_FORCE") == "1" and torch.cuda.is_available()
    bad = 0
    for layout, r in zip(("dense", "fused_qk"), _attn_twice(ATTN3_DIMS, True)):
        print(f"[store-policy] attention3 {ATTN3_DIMS} {layout}: err / bound {r[0]:.3f}, against the folded reference / sharp bound {r[1]:.3f}")
        bad += max(r) > 1.0
    return 1 if bad else 0


# ------------------------------------------------------------------------------------------------
# GroupNorm from producer statistics, LayerNorm: one 64-row shape
# ------------------------------------------------------------------------------------------------
def test_gn_apply_pstats_twice_into_the_same_buffer():
    from lib.hip import ops
    B, HW, C, G = 1, 64, 320, 32
    assert KR.gn_form(B, HW, C, 0, G, True) == "pstats_par"
    D = KR.gn_depth("pstats_par", B, HW, C, 0, G)
    ops_ = []
    for seed in SEEDS:
        g = torch.Generator().manual_seed(7000 + seed)
        x = (torch.randn((B * HW, C), generator=g) + 0.5).half()
        gamma, beta = (1 + 0.2 * torch.randn(C, generator=g)).half(), (0.1 * torch.randn(C, generator=g)).half()
        ops_.append((x, gamma, beta, x.view(B, HW, C).cuda(), KR.gn_pstats(x).cuda(), gamma.cuda(), beta.cuda()))
    buf = torch.full((B * HW + 16, C + 16), SENTINEL, dtype=torch.float16, device="cuda")
    out = buf[:B * HW].view(B, HW, C + 16)[..., 8:8 + C]
    torch.cuda.synchronize()
    snaps = []
    for x, gamma, beta, dx, st, dg, db in ops_:
        ops.set_gn_stats(dx, st)
        assert ops.GN_PSTATS and ops._lib().pfd_groupnorm_takes_pstats(B, C, 0, HW, G)
        ops.groupnorm(dx, dg, db, G, 1e-5, silu=True, out=out)
        snaps.append(buf.clone())
    torch.cuda.synchronize()
    for seed, (x, gamma, beta, *_), b in zip(SEEDS, ops_, snaps):
        assert bool((b[B * HW:] == SENTINEL).all()) and bool((b[:, :8] == SENTINEL).all()) and bool((b[:, 8 + C:] == SENTINEL).all())
        args = (x, None, B, HW, G, gamma, beta, 1e-5, True)
        ratio, _ = KR.bound_ratio(b[:B * HW, 8:8 + C].contiguous().cpu(), KR.groupnorm_ref(*args), KR.groupnorm_allowance(*args, D))
        print(f"[store-policy] gn_apply_pstats B{B} HW{HW} C{C} seed {seed}: err / bound {ratio:.3f}")
        assert ratio <= 1.0, (seed, ratio)


def test_layernorm_twice_into_the_same_buffer():
    from lib.hip import ops
    M, C = 64, 320
    ops_ = [KR.ln_operands(M, C, 9000 + seed) for seed in SEEDS]
    dev = [tuple(t.cuda() for t in o) for o in ops_]
    buf = torch.full((M + 16, C + 16), SENTINEL, dtype=torch.float16, device="cuda")
    torch.cuda.synchronize()
    snaps = []
    for x, gamma, beta in dev:
        ops.layernorm(x, gamma, beta, out=buf[:M, 8:8 + C])
        snaps.append(buf.clone())
    torch.cuda.synchronize()
    for seed, (x, gamma, beta), b in zip(SEEDS, ops_, snaps):
        assert bool((b[M:] == SENTINEL).all()) and bool((b[:, :8] == SENTINEL).all()) and bool((b[:, 8 + C:] == SENTINEL).all())
        ref64, ref32 = KR.layernorm_ref(x, gamma, beta), KR.layernorm_ref(x, gamma, beta, dtype=torch.float32)
        ratio, _ = KR.bound_ratio(b[:M, 8:8 + C].contiguous().cpu(), ref64, KR.fp32_allowance(ref64, ref32))
        print(f"[store-policy] layernorm {M}x{C} seed {seed}: err / bound {ratio:.3f}")
        assert ratio <= 1.0, (seed, ratio)


if __name__ == "__main__":
    sys.exit(_attention3_child() if sys.argv[1:] == ["attention3"] else 2)
