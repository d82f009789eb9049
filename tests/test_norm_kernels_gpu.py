"""GPU (-m gpu): the stand-alone GroupNorm kernels of csrc/norm.hip, one launch at a time -- gn_small_kernel, gn_stats_kernel +
gn_apply_kernel, gn_apply_pstats_kernel<true / false>, gn_stats_kernel + gn_table_kernel -- each reached through ops.groupnorm /
ops.groupnorm_table (the plain-loop producer-statistics form, which no G = 32 shape reaches, through `binding`) on the cases of
kernel_refs.GN_CASES, against the plain fp64 reference kernel_refs.groupnorm_ref.  Every element is held to
round_once_bound(ref, groupnorm_allowance), whose statistics term charges D fp32 additions (kernel_refs.gn_depth: the longest
chain of additions of the form the case takes, read off the loops of norm.hip), not the number of values per group.
tests/test_norm_kernels_cpu.py qualifies the reference, the bound and the table and pins the form of every case; the measured
ratios are in profiles/norm_kernel_tests.md."""
import pytest
import torch
import torch.nn.functional as F

import kernel_refs as KR

pytestmark = pytest.mark.gpu

SENTINEL = 1234.0           # exact in fp16, far outside every result below
ALL = KR.GN_CASES
ids = [c["id"] for c in ALL]


def _device_operands(p, poison=True):
    """x1 / x2 as [B, HW, C] device tensors (strided cases: column slices of NaN-filled buffers), gamma, beta and, for the
    producer-statistics forms, the statistics of each source"""
    c = p["case"]
    o = KR.gn_operands(p, poison)
    d = {}
    for k in ("x1", "x2"):
        d[k] = None if o[k] is None else o[k].cuda() if c["strides"] is None else KR.gemm_view(o[k][0].cuda(), o[k][1])
    d["gamma"], d["beta"] = p["gamma"].cuda(), p["beta"].cuda()
    if c["form"].startswith("pstats"):
        d["st1"] = KR.gn_pstats(p["x1"]).cuda()
        d["st2"] = None if p["x2"] is None else KR.gn_pstats(p["x2"]).cuda()
        assert bool(torch.isnan(d["st1"]).any()) == (160 // (c["C1"] // 32) < 16)
    return d


def _pstats_direct(c, d, out):
    """pfd_groupnorm_pstats_f16 through the C ABI; returns the return value"""
    from lib.hip import ops
    x2, st2 = d["x2"], d.get("st2")
    return ops._lib().pfd_groupnorm_pstats_f16(
        d["x1"].data_ptr(), c["C1"], d["x1"].stride(-2), d["st1"].data_ptr(), ops._ptr(x2), c["C2"], 0 if x2 is None else x2.stride(-2),
        ops._ptr(st2), d["gamma"].data_ptr(), d["beta"].data_ptr(), out.data_ptr(), out.stride(-2), c["B"], c["HW"], c["G"], c["eps"],
        ops.ACT_SILU if c["silu"] else ops.ACT_NONE, ops._stream())


def _launch(c, d, out=None):
    from lib.hip import binding as _b, ops
    if out is None:
        out = torch.empty((c["B"], c["HW"], c["C1"] + c["C2"]), dtype=torch.float16, device="cuda")
    if c["form"] == "pstats_plain":
        _b.check(_pstats_direct(c, d, out), c["id"])
        return out
    if c["form"] == "pstats_par":       # the statistics ride on the tensor objects; ops.groupnorm takes them under these two conditions
        ops.set_gn_stats(d["x1"], d["st1"])
        if d["x2"] is not None:
            ops.set_gn_stats(d["x2"], d["st2"])
        assert ops.GN_PSTATS and ops.get_gn_stats(d["x1"]) is not None and ops._lib().pfd_groupnorm_takes_pstats(c["B"], c["C1"], c["C2"], c["HW"], 32)
    r = ops.groupnorm(d["x1"], d["gamma"], d["beta"], c["G"], c["eps"], x2=d["x2"], silu=c["silu"], out=out)
    assert r.data_ptr() == out.data_ptr()
    return out


def _wide_out(c):
    """a sentinel-filled buffer with 16 rows behind the last one; the output is columns [8, 8 + C) of its leading B HW rows"""
    M, C = c["B"] * c["HW"], c["C1"] + c["C2"]
    W = C + 8 + (c["strides"][2] if c["strides"] else 8)
    buf = torch.full((M + 16, W), SENTINEL, dtype=torch.float16, device="cuda")
    return buf, buf[:M].view(c["B"], c["HW"], W)[..., 8:8 + C]


_ran = {}


def _run_case(cid):
    """sentinels and poison, two more launches; returns the output [B HW, C] on the CPU (cached: the table and pair tests reuse it)"""
    if cid in _ran:
        return _ran[cid]
    p = KR.gn_problem(cid)
    c = p["case"]
    M, C = c["B"] * c["HW"], c["C1"] + c["C2"]
    d = _device_operands(p)
    buf, out = _wide_out(c)
    _launch(c, d, out)
    torch.cuda.synchronize()
    assert bool((buf[M:] == SENTINEL).all()), "rows behind the last row were written"
    assert bool((buf[:M, :8] == SENTINEL).all()) and bool((buf[:M, 8 + C:] == SENTINEL).all()), "columns outside the slice were written"
    got = buf[:M, 8:8 + C].contiguous()
    assert bool(torch.isfinite(got).all()), "a NaN (pad column, unwritten statistics slot) reached the output, or an element is not finite"
    assert not bool((got == SENTINEL).any()), "an element was not written"
    assert torch.equal(_launch(c, d).view(M, C), got), "two launches (ldy > C, ldy = C), different bits"
    if c["strides"] is not None:
        assert torch.equal(_launch(c, _device_operands(p, poison=False)).view(M, C), got), "the pad values changed the result"
    if c["form"] == "pstats_par":       # ops.groupnorm took the statistics: the same bits as the direct call
        o2 = torch.empty((c["B"], c["HW"], C), dtype=torch.float16, device="cuda")
        assert _pstats_direct(c, d, o2) == 0 and torch.equal(o2.view(M, C), got), "ops.groupnorm did not take the producer statistics"
    _ran[cid] = got.cpu()
    return _ran[cid]


@pytest.mark.parametrize("cid", ids)
def test_groupnorm_vs_fp64(cid):
    p = KR.gn_problem(cid)
    c = p["case"]
    got = _run_case(cid)
    D = KR.gn_depth_of(c)
    ref = KR.groupnorm_ref(*KR.gn_args(p))
    ratio, used = KR.bound_ratio(got, ref, KR.groupnorm_allowance(*KR.gn_args(p), D))
    print(f"[norm-kernels] {cid} ({' + '.join(KR.GN_FORM_KERNELS[c['form']])}, D {D}): err / bound {ratio:.3f}, allowance used {used:.3f}")
    if c["kind"] == "const":            # the constant groups come out as beta, whatever the clamp had to do
        cpg = (c["C1"] + c["C2"]) // c["G"]
        y = got[:, :2 * cpg].double()
        want = p["beta"][:2 * cpg].double()
        want = F.silu(want) if c["silu"] else want
        print(f"[norm-kernels] {cid}: constant groups, largest |y - beta| {float((y - want).abs().max()):.2e}")
    assert ratio <= 1.0, (cid, ratio, used)


TABLE = [c["id"] for c in ALL if c["table"]]


@pytest.mark.parametrize("cid", TABLE)
def test_groupnorm_table_vs_fp64(cid):
    """pfd_groupnorm_table_f16 on the case's operands: scale and shift within the statistics part of the allowance; for the
    two-launch cases x * scale + shift (+ SiLU) of the device's own table, evaluated in fp64, is the device's GroupNorm within one
    rounding and the 16-ulp fp32 floor (csrc/norm.hip: the same sums in the same order as gn_apply_kernel)"""
    from lib.hip import ops
    p = KR.gn_problem(cid)
    c = p["case"]
    B, HW, C = c["B"], c["HW"], c["C1"] + c["C2"]
    d = _device_operands(p)
    t = ops.groupnorm_table(d["x1"], d["gamma"], d["beta"], c["G"], c["eps"], x2=d["x2"])
    assert t.shape == (B, 2, C) and t.dtype == torch.float32
    assert torch.equal(t, ops.groupnorm_table(d["x1"], d["gamma"], d["beta"], c["G"], c["eps"], x2=d["x2"])), "two launches, different bits"
    t = t.double().cpu()
    assert bool(torch.isfinite(t).all())
    D = KR.gn_depth_of(c, table=True)
    want = KR.groupnorm_table_ref(*KR.gn_args(p)[:-1])
    _, a_scale, a_shift = KR.groupnorm_allowance(*KR.gn_args(p), D, parts=True)
    r_scale, r_shift = float(((t[:, 0] - want[:, 0]).abs() / a_scale).max()), float(((t[:, 1] - want[:, 1]).abs() / a_shift).max())
    msg = f"[norm-kernels] {cid} table (D {D}): scale err / allowance {r_scale:.3f}, shift err / allowance {r_shift:.3f}"
    r_apply = 0.0
    if c["form"] == "two":
        x = (p["x1"] if p["x2"] is None else torch.cat([p["x1"], p["x2"]], 1)).double().view(B, HW, C)
        y = (x * t[:, None, 0] + t[:, None, 1]).reshape(B * HW, C)
        y = F.silu(y) if c["silu"] else y
        r_apply, _ = KR.bound_ratio(_run_case(cid), y, 16 * 2.0 ** -24 * float(y.abs().max()))
        msg += f", groupnorm output against x * scale + shift of this table: err / bound {r_apply:.3f}"
    print(msg)
    assert r_scale <= 1.0 and r_shift <= 1.0 and r_apply <= 1.0, (cid, r_scale, r_shift, r_apply)


def test_small_and_two_launch_forms_on_shared_samples():
    """B G = 128 takes the small form, B G = 96 the two-launch form: on the three samples they share, both are within the bound of
    the one reference"""
    a, b = "small-B4-HW64-C1280", "two-B3-HW64-C1280"
    pa, pb = KR.gn_problem(a), KR.gn_problem(b)
    n = 3 * 64
    ref = KR.groupnorm_ref(*KR.gn_args(pb))
    assert torch.equal(ref, KR.groupnorm_ref(*KR.gn_args(pa))[:n])
    ga, gb = _run_case(a)[:n], _run_case(b)
    ra, _ = KR.bound_ratio(ga, ref, KR.groupnorm_allowance(*KR.gn_args(pa), KR.gn_depth_of(pa["case"]))[:n])
    rb, _ = KR.bound_ratio(gb, ref, KR.groupnorm_allowance(*KR.gn_args(pb), KR.gn_depth_of(pb["case"])))
    print(f"[norm-kernels] {a} | {b}: err / bound {ra:.3f} | {rb:.3f}, {int((ga != gb).sum())} of {ga.numel()} elements differ between the forms")
    assert ra <= 1.0 and rb <= 1.0


# ------------------------------------------------------------------------------------------------
# arguments: answered before anything is written
# ------------------------------------------------------------------------------------------------
def test_groupnorm_rejects_bad_arguments_before_writing():
    from lib.hip import binding as _b, ops
    lib = ops._lib()
    B, HW = 2, 64
    x = torch.randn((B * HW, 4400), generator=torch.Generator().manual_seed(5)).half().cuda()
    gamma, beta = torch.ones(4400, dtype=torch.float16, device="cuda"), torch.zeros(4400, dtype=torch.float16, device="cuda")
    y = torch.full((B * HW, 4400), SENTINEL, dtype=torch.float16, device="cuda")
    wsb = lib.pfd_groupnorm_ws_bytes(B, 4096, HW)
    ws = torch.full((wsb,), 0x5A, dtype=torch.uint8, device="cuda")
    st = torch.zeros((B * HW // 64 + 2, 8, 16, 2), dtype=torch.float32, device="cuda")
    table = torch.full((B * 2 * 4400 + 4,), SENTINEL, dtype=torch.float32, device="cuda")
    ld = x.stride(0)

    def gn(C1, C2=0, G=32, ld1=ld, ld2=ld, ldy=ld, act=ops.ACT_SILU, ws_bytes=wsb):
        return lib.pfd_groupnorm_f16(x.data_ptr(), C1, ld1, x.data_ptr() if C2 else None, C2, ld2 if C2 else 0, gamma.data_ptr(), beta.data_ptr(),
                                     y.data_ptr(), ldy, B, HW, G, 1e-5, act, ws.data_ptr(), ws_bytes, ops._stream())

    def pstats(C1, hw=HW, G=32, ld1=ld, act=ops.ACT_SILU, st_off=0):
        return lib.pfd_groupnorm_pstats_f16(x.data_ptr(), C1, ld1, st.data_ptr() + st_off, None, 0, 0, None, gamma.data_ptr(), beta.data_ptr(),
                                            y.data_ptr(), ld, B, hw, G, 1e-5, act, ops._stream())

    def tab(C1, G=32, ld1=ld, off=0, ws_bytes=wsb):
        return lib.pfd_groupnorm_table_f16(x.data_ptr(), C1, ld1, None, 0, 0, gamma.data_ptr(), beta.data_ptr(), table.data_ptr() + off, B, HW, G,
                                           1e-5, ws.data_ptr(), ws_bytes, ops._stream())

    assert table.data_ptr() % 16 == 0
    shape, inval = _b.PFD_ESHAPE, _b.PFD_EINVAL
    assert gn(320, G=7) == shape and tab(320, G=7) == shape                          # C % G != 0
    assert gn(100, G=25) == shape and gn(320, 100, G=20) == shape and tab(100, G=25) == shape      # C1 (C2) % 8 != 0
    assert gn(4352) == shape and gn(2176, 2176) == shape and tab(4352) == shape      # C > 4096 (a multiple of G and of 8)
    assert pstats(320, hw=100) == shape and pstats(320, hw=32) == shape              # takes_pstats: whole 64-row slabs only
    assert pstats(2560, G=64) == shape and pstats(200, G=25) == shape                # ... no small-form shape, C1 % 160 == 0
    assert gn(320, ld1=324) == inval and gn(320, 320, ld2=324) == inval and gn(320, ldy=324) == inval      # ld % 8 != 0
    assert pstats(320, ld1=324) == inval and tab(320, ld1=324) == inval
    assert gn(1280, G=128) == inval and tab(1280, G=128) == inval                    # G > 64
    assert gn(320, ws_bytes=wsb - 1) == inval and tab(320, ws_bytes=wsb - 1) == inval    # a short workspace
    assert gn(320, act=ops.ACT_GELU) == inval and pstats(320, act=ops.ACT_GELU) == inval
    assert tab(320, off=4) == inval and pstats(320, st_off=4) == inval               # a misaligned table / statistics array
    torch.cuda.synchronize()
    assert bool((y == SENTINEL).all()) and bool((table == SENTINEL).all()) and bool((ws == 0x5A).all())
    assert pstats(320) == 0 and tab(320) == 0 and gn(320) == 0                       # (the same operands are fine when well-formed)
    torch.cuda.synchronize()
    assert not bool((y[:, :320] == SENTINEL).any()) and bool((y[:, 320:] == SENTINEL).all())


def test_ln_rowstats_strided():
    """pfd_ln_rowstats_f16 on a column slice (ldx > C) with M P = 104 groups, no multiple of the 64 a block takes: the fp64 row sums
    within 1e-5 of the mass summed (the bar of test_encoder_kernels_gpu.py::test_add_rowvec_with_row_statistics), nothing
    written behind the last group"""
    from lib.hip import ops
    M, C, P = 13, 1280, 8
    g = torch.Generator().manual_seed(13)
    buf = KR._embed((torch.randn((M, C), generator=g) + 0.3).half(), 2, 3, 8, C + 24, True).cuda()
    x = buf[2:2 + M, 8:8 + C]
    assert x.stride(0) == C + 24 and bool(torch.isnan(buf).any())
    flat = torch.full((M * P * 2 + 64,), SENTINEL, dtype=torch.float32, device="cuda")
    st = ops.ln_rowstats(x, out=flat[:M * P * 2].view(M, P, 2))
    torch.cuda.synchronize()
    assert st.data_ptr() == flat.data_ptr() and bool((flat[M * P * 2:] == SENTINEL).all()), "written behind the last group"
    assert torch.equal(st, ops.ln_rowstats(x.contiguous())), "ldx changed the sums"
    xd = x.double().cpu().view(M, P, 160)
    s64, q64, mass = xd.sum(-1), (xd * xd).sum(-1), xd.abs().sum(-1)
    e_s = float(((st[..., 0].double().cpu() - s64).abs() / mass).max())
    e_q = float(((st[..., 1].double().cpu() - q64).abs() / q64).max())
    print(f"[norm-kernels] ln_rowstats {(M, C)} ldx {C + 24}: sums {e_s:.2e}, sums of squares {e_q:.2e} (relative, bound 1e-5)")
    assert e_s <= 1e-5 and e_q <= 1e-5, (e_s, e_q)
