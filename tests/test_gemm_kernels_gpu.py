"""GPU (-m gpu): the kernels behind pfd_gemm_f16 (csrc/gemm_glds.hip, csrc/gemm_conv.hip), each reached through ops.gemm / ops.conv
under the forced tile code (or the heuristic) its entry of kernel_refs.GEMM_CASES names, against the plain fp64 reference
kernel_refs.gemm_ref written from the header text of PfdGemmDesc.  Every element is held to the per-element bound that
kernel_refs.gemm_allowance derives from the number formats (accumulation, activation, split-K slabs, the staged value in front of
the residual, LayerNorm fold, one final rounding); the side outputs (ln_out, gn_out, gnf_y) to theirs.  Operands are column
slices of buffers with NaN in every position a launch may read but must not use; outputs go to a column slice of a
sentinel-filled buffer with sentinel rows behind the last one.  tests/test_gemm_kernels_cpu.py qualifies the reference, the bound
and the table; the measured ratios are in profiles/gemm_kernel_tests.md."""
import pytest
import torch

import kernel_refs as KR

pytestmark = pytest.mark.gpu

SENTINEL = -61440.0         # exact in fp16, outside every result below (tests/test_gemm_kernels_cpu.py: max |ref| <= 3e4 on every operand kind)
ALL = KR.GEMM_CASES
ids = [c["id"] for c in ALL]


def _device_operands(p, poison=True):
    """the launch's tensors on the device: A / A2 / W as views of the poisoned (or zero-padded) buffers"""
    c = p["case"]
    o = KR.gemm_operands(p, poison)
    d = {k: KR.gemm_view(o[k][0].cuda(), o[k][1]) for k in ("A", "A2", "W") if k in o}
    d["bias"] = None if o["bias"] is None else o["bias"].cuda()
    for k in ("rowvec", "R", "gn_table", "gnf_gamma", "gnf_beta"):
        d[k] = None if p.get(k) is None else p[k].cuda()
    if c["ln"] is not None:
        from lib.hip import ops
        # s_n of the PACKED row order, of the f16 weight; statistics from fp64 sums rounded to fp32 (norm.hip is not under test),
        # except in the one case that takes them from pfd_ln_rowstats_f16
        d["colsum"] = KR.gemm_view(*o["W"]).double().sum(1).float().cuda()
        d["stats"] = ops.ln_rowstats(d["A"]) if c["ln"] == "rowstats" else KR.gemm_ln_args(p).cuda()
    return d


def _launch(p, d, out=None, out_t=None):
    """one launch of the case through the wrappers; returns dict(out=, out_t=, ln_out=, gn_out=, gnf_y=)"""
    from lib.hip import ops
    c = p["case"]
    M, N = c["M"], c["N"]
    res = {}
    if c["kind"] == "lin":
        if c["n_split"] and out_t is None:
            out_t = torch.empty((N - c["n_split"], (M + 7) // 8 * 8), dtype=torch.float16, device="cuda")
        r = ops.gemm(d["A"], d["W"], bias=d["bias"], rowvec=d["rowvec"], rows_per_rv=c["rows_per_rv"], res=d["R"], act=c["act"], out=out,
                     bias_per_row=c["bias_per_row"], tile=c["tile"], out_t=out_t, n_split=c["n_split"] or None,
                     ln=(d["stats"], d["colsum"], c["ln_eps"]) if c["ln"] is not None else None, ln_out=True if c["ln_out"] else None,
                     a2=d.get("A2"), zero_rows=c["zero_rows"], gn_out=c["gn_out"], res_rows=c["res_rows"] or None, w_tiled=c["w_tiled"])
        if c["ln_out"]:
            r, res["ln_out"] = r
        if c["gn_out"]:
            res["gn_out"] = ops.get_gn_stats(r)
            assert res["gn_out"] is not None
        res["out"] = r
        if c["n_split"]:
            res["out_t"] = out_t
        return res
    ks, stride, pad, ups, Ho, Wo = c["geom"]
    kw = dict(stride=stride, pad=pad, ups=bool(ups), bias=d["bias"], rowvec=d["rowvec"], res=d["R"], act=c["act"], out=out, tile=c["tile"],
              out_hw=(Ho, Wo), w_tiled=c["w_tiled"])
    if c["gn_pro"] is not None:
        kw["gn"] = (d["gn_table"], d.get("A2"), c["gn_pro"][1])
    if c["gnf"] is not None:
        r = ops.conv(d["A"], d["W"], ks, gn_fuse=(d["gnf_gamma"], d["gnf_beta"], 1e-5, True, c["gnf"]), **kw)
        assert r is not None, "the fused GroupNorm reduction declined a case of the table"
        res["out"], res["gnf_y"] = r[0], r[1].view(M, N)
        return res
    res["out"] = ops.conv(d["A"], d["W"], ks, **kw)
    return res


def _outputs(c):
    """sentinel-filled buffers: the output as a column slice with 16 sentinel rows behind it; the transposed tail with pad columns"""
    M, N = c["M"], c["N"]
    n_out = c["n_split"] or (N // 2 if c["act"] == KR.ACT_GEGLU else N)
    buf = torch.full((M + 16, n_out + c["ldc_pad"]), SENTINEL, dtype=torch.float16, device="cuda")
    if c["kind"] == "conv":
        B = c["image"][0]
        out = buf[:M].view(B, c["geom"][4], c["geom"][5], n_out + c["ldc_pad"])[..., 8:8 + n_out]
    else:
        out = buf[:M, 8:8 + n_out]
    tbuf = torch.full((N - c["n_split"] + 4, (M + 7) // 8 * 8 + 8), SENTINEL, dtype=torch.float16, device="cuda") if c["n_split"] else None
    return buf, out, tbuf, n_out


_ran = {}


def _run_case(cid):
    """guards and poison, three launches, zeros for NaNs; returns the outputs on the CPU (cached: the agreement tests reuse them)"""
    if cid in _ran:
        return _ran[cid]
    p = KR.gemm_problem(cid)
    c = p["case"]
    M, N = c["M"], c["N"]
    d = _device_operands(p)
    buf, out, tbuf, n_out = _outputs(c)
    r = _launch(p, d, out, None if tbuf is None else tbuf[:N - c["n_split"]])
    torch.cuda.synchronize()
    assert bool((buf[M:] == SENTINEL).all()), "rows behind the last row were written"
    assert bool((buf[:M, :8] == SENTINEL).all()) and bool((buf[:M, 8 + n_out:] == SENTINEL).all()), "columns outside the slice were written"
    got = {}
    if c["gnf"] is not None and not c["gnf"]:
        assert r["out"] is None and bool((buf == SENTINEL).all()), "gnf_skip_raw: the raw result was stored"
    else:
        assert r["out"].data_ptr() == out.data_ptr()
        got["out"] = buf[:M, 8:8 + n_out].contiguous()
    if tbuf is not None:
        assert bool((tbuf[N - c["n_split"]:] == SENTINEL).all()) and bool((tbuf[:, M:] == SENTINEL).all()), "the tail wrote outside [N - n_split, M]"
        got["out_t"] = tbuf[:N - c["n_split"], :M].contiguous()
    for k in ("ln_out", "gn_out", "gnf_y"):
        if k in r:
            got[k] = r[k].clone()
    for k in ("out", "out_t", "gnf_y"):
        if k in got:
            assert bool(torch.isfinite(got[k]).all()), f"{k}: NaN from a pad position reached the output (or an element is not finite)"
            assert not bool((got[k] == SENTINEL).any()), f"{k}: an element was not written"

    def same(r2, what):
        for k in got:
            g2 = r2[k] if k != "out_t" else r2[k][:, :M]
            g2 = g2.reshape(got[k].shape)
            if k == "gn_out":           # (the slots past 160 / (N / 32) are not written)
                g2, g1 = g2[:, :, :160 // (N // 32)], got[k][:, :, :160 // (N // 32)]
            else:
                g1 = got[k]
            assert torch.equal(g2, g1), f"{k}: {what}"
    for _ in range(2):
        same(_launch(p, d), "two launches, different bits")
    same(_launch(p, _device_operands(p, poison=False)), "the pad values changed the result")
    _ran[cid] = {k: v.cpu() for k, v in got.items()}
    return _ran[cid]


@pytest.mark.parametrize("cid", ids)
def test_gemm_vs_fp64(cid):
    p = KR.gemm_problem(cid)
    c = p["case"]
    M, N = c["M"], c["N"]
    got = _run_case(cid)
    ref = KR.gemm_ref(p)
    a = KR.gemm_allowance(p, c["splits"], KR.gemm_case_is_wide(c))
    parts = []
    worst = 0.0
    for k in ("out", "out_t"):
        if k in got:
            ratio, used = KR.bound_ratio(got[k], ref[k], a[k])
            parts.append(f"{k} err / bound {ratio:.3f}, allowance used {used:.3f}")
            worst = max(worst, ratio)
    stored = got.get("out")
    if "ln_out" in got:                # fp32 sums of 160 stored values: 160 u sum |v| (and sum v^2)
        from lib.hip import ops
        want = KR.ln_out_ref(stored)
        v = stored.double().reshape(M, N // 160, 160)
        bnd = 160 * 2.0 ** -24 * torch.stack([v.abs().sum(-1), (v * v).sum(-1)], -1)
        ratio = float(((got["ln_out"].double() - want).abs() / bnd).max())
        parts.append(f"ln_out err / bound {ratio:.3f}")
        worst = max(worst, ratio)
        # the header: the same summation order as pfd_ln_rowstats_f16 (the store pass and ln_rowstats_kernel: lane k of four takes
        # the 16-byte chunks k, k + 4, ... in order, then two xor shuffles; the split-K form launches that kernel itself)
        assert torch.equal(got["ln_out"], ops.ln_rowstats(stored.cuda()).cpu()), "ln_out is not bitwise pfd_ln_rowstats_f16 of the output"
    if "gn_out" in got:                # fp32 sums of n = 64 N / 32 stored values
        cpg = N // 32
        want = KR.gn_out_ref(stored)[:, :, :160 // cpg]
        v = stored.double().reshape(M // 64, 64, N // 160, 160 // cpg, cpg)
        bnd = 64 * cpg * 2.0 ** -24 * torch.stack([v.abs().sum((1, 4)), (v * v).sum((1, 4))], -1)
        ratio = float(((got["gn_out"][:, :, :160 // cpg].double() - want).abs() / bnd).max())
        parts.append(f"gn_out err / bound {ratio:.3f}")
        worst = max(worst, ratio)
    if "gnf_y" in got:                 # GroupNorm(32) + SiLU of the stored raw values, or of the reference where they are not stored
        rows = c["geom"][4] * c["geom"][5]
        src, dx = (stored, 0.0) if c["gnf"] else (ref["out"], float(KR.round_once_bound(ref["out"], a["out"]).max()))
        want = KR.groupnorm32_ref(src, rows, p["gnf_gamma"], p["gnf_beta"], 1e-5, True)
        ay = KR.groupnorm32_allowance(src, rows, p["gnf_gamma"], p["gnf_beta"], 1e-5, True, dx)
        ratio, used = KR.bound_ratio(got["gnf_y"], want, ay)
        parts.append(f"gnf_y err / bound {ratio:.3f}, allowance used {used:.3f}")
        worst = max(worst, ratio)
    print(f"[gemm-kernels] {c['cls']} {cid} ({c['kernel']}{' + ' + c['reduce'] if c['reduce'] else ''}): " + "; ".join(parts))
    if KR.gemm_operand_kind(c)[0] == "exact":
        # nothing rounds on these operands (tests/test_gemm_kernels_cpu.py): the bits of the fp64 reference rounded once, which
        # any rounding the header does not name, any misplaced slab and any f16 arithmetic other than a store would change
        assert torch.equal(got["out"], ref["out"].half()), (cid, int((got["out"] != ref["out"].half()).sum()), parts)
    else:
        assert worst <= 1.0, (cid, parts)


# ------------------------------------------------------------------------------------------------
# once per problem: the forced variants and the heuristic, split and unsplit
# ------------------------------------------------------------------------------------------------
def _groups():
    by = {}
    for c in ALL:
        by.setdefault(KR.gemm_problem_key(c["id"]), []).append(c["id"])
    return {k: v for k, v in by.items() if len(v) > 1}


@pytest.mark.parametrize("key", sorted(_groups()))
def test_variants_and_splits_of_one_problem_agree(key):
    """the cases that differ only in the forced variant / split count share their operands: every one agrees with the first (the
    heuristic where the table has it) within the sum of both bounds, per element"""
    cids = sorted(_groups()[key], key=lambda i: ("-v0-" not in i and not i.endswith("-v0"), i))
    base = cids[0]
    pb = KR.gemm_problem(base)
    cb = pb["case"]
    rb = KR.gemm_ref(pb)
    ab = KR.gemm_allowance(pb, cb["splits"], KR.gemm_case_is_wide(cb))
    gb = _run_case(base)
    worst = 0.0
    for cid in cids[1:]:
        p = KR.gemm_problem(cid)
        c = p["case"]
        assert all(torch.equal(p[k], pb[k]) for k in ("A", "W")), "the cases of one problem share their operands"
        a = KR.gemm_allowance(p, c["splits"], KR.gemm_case_is_wide(c))
        g = _run_case(cid)
        for k in ("out", "out_t"):
            if k in g and k in gb:
                bnd = KR.round_once_bound(rb[k], ab[k]) + KR.round_once_bound(rb[k], a[k])
                worst = max(worst, float(((g[k].double() - gb[k].double()).abs() / bnd).max()))
    print(f"[gemm-kernels] {cb['cls']} {key}: {len(cids)} variants / split counts, worst difference / (sum of bounds) {worst:.3f}")
    assert worst <= 1.0, (key, worst)


# ------------------------------------------------------------------------------------------------
# arguments: answered before anything is written
# ------------------------------------------------------------------------------------------------
def _plain(M=128, N=320, K=128, slack=8):
    g = torch.Generator().manual_seed(2)
    a = torch.randn((M, K + slack), generator=g).half().cuda()
    w = (torch.randn((N, K + slack), generator=g) * K ** -0.5).half().cuda()
    out = torch.full((M, N), SENTINEL, dtype=torch.float16, device="cuda")
    return a, w, out


def _desc(a, w, out, M, N, K, res=None):
    from lib.hip import ops
    d = ops._gemm_desc(a, w, out, M, N, K, a.stride(0), w.stride(0), None, None, res)
    d.rows_per_rv, d.act, d.ksize = 1, 0, 0
    return d


def test_gemm_rejects_bad_arguments_before_writing():
    from lib.hip import binding as _b, ops
    M, N, K = 128, 320, 128
    a, w, out = _plain(M, N, K)
    bad = (_b.PfdError, ValueError)
    with pytest.raises(_b.PfdError, match="PFD_EINVAL"):                    # lda + 4
        ops.gemm(a.view(-1)[:M * (K + 4)].view(M, K + 4)[:, :K], w[:, :K], out=out)
    with pytest.raises(_b.PfdError, match="PFD_EINVAL"):                    # A four halfs into a 16-byte unit
        ops.gemm(a[:, 4:4 + K], w[:, :K], out=out)
    a100 = torch.randn((M, 104)).half().cuda()
    with pytest.raises(_b.PfdError, match="PFD_ESHAPE"):                    # K = 100
        ops.gemm(a100[:, :100], w[:, :100], out=out)
    with pytest.raises(bad):                                                # k_split = 32 (the wrapper's own check)
        ops.gemm(a[:, :32], w[:, :K], a2=a[:, 32:K], out=out)
    d = _desc(a, w, out, M, N, K)                                           # ... and the library's
    d.k_split, d.A2, d.lda2 = 32, a[:, 32:].data_ptr() + 64, a.stride(0)
    with pytest.raises(_b.PfdError, match="PFD_ESHAPE"):
        ops._launch(d, 0, "k_split 32")
    ot = torch.full((N - 96, M), SENTINEL, dtype=torch.float16, device="cuda")
    with pytest.raises(_b.PfdError, match="PFD_ESHAPE"):                    # n_split no multiple of the tile
        ops.gemm(a[:, :K], w[:, :K], out=out[:, :96], out_t=ot, n_split=96)
    res = torch.randn((M, N // 2)).half().cuda()
    with pytest.raises(_b.PfdError, match="PFD_ESHAPE"):                    # GEGLU with a residual
        ops.gemm(a[:, :K], w[:, :K], act=ops.ACT_GEGLU, res=res, out=out[:, :N // 2])
    a320, w320, _ = _plain(M, N, 320)
    st = torch.zeros((M, 1, 2), dtype=torch.float32, device="cuda")
    cs = torch.zeros(N, dtype=torch.float32, device="cuda")
    with pytest.raises(bad):                                                # ln_parts * 160 != K (wrapper)
        ops.gemm(a320[:, :320], w320[:, :320], ln=(st, cs, 1e-5), out=out)
    d = _desc(a320, w320, out, M, N, 320)
    d.ln_stats, d.ln_colsum, d.ln_parts, d.ln_eps = st.data_ptr(), cs.data_ptr(), 1, 1e-5
    with pytest.raises(_b.PfdError, match="PFD_ESHAPE"):
        ops._launch(d, 0, "ln_parts 1 at K 320")
    with pytest.raises(_b.PfdError, match="PFD_ESHAPE"):                    # gn_out with M % 64 != 0
        ops.gemm(a[:100, :K], w[:, :K], gn_out=True, out=out[:100])
    r40 = torch.randn((40, N)).half().cuda()
    with pytest.raises(bad):                                                # res_rows < M / 2 (wrapper)
        ops.gemm(a[:, :K], w[:, :K], res=r40, res_rows=40, out=out)
    d = _desc(a, w, out, M, N, K, res=r40)
    d.res_rows = 40
    with pytest.raises(_b.PfdError, match="PFD_ESHAPE"):
        ops._launch(d, 0, "res_rows 40 of 128")
    with pytest.raises(_b.PfdError, match="PFD_ESHAPE"):                    # tiled weights where no wide-tile kernel serves the shape
        ops.gemm(a[:, :K], w[:, :K].contiguous(), w_tiled=True, bias_per_row=True, bias=torch.zeros(M, dtype=torch.float16, device="cuda"), out=out)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((ot == SENTINEL).all())
    ops.gemm(a[:, :K], w[:, :K], out=out)                                   # (the same operands are fine when well-formed)
    assert not bool((out == SENTINEL).any())
