"""GPU (-m gpu): pfd_attention_rbias_f16 (csrc/attention.hip: attention_rbias_kernel, the text of attention2_kernel compiled with a
logit row per region of the query) -- the kernel under regional reference mixing (lib/regions.py).  Each of its three kernel
classes is reached through ops.attention(rbias=, qregion=) and held, element by element, to lib/regions.regional_attention in
fp64 on the device (regions_refs.regional_ref, pinned to the numpy specification by tests/test_regions_cpu.py) within
refmix_refs.kbias_bound, Bmax and T taken over the table; and, for the regions whose row has key 0 finite, to the BITS of
pfd_attention_kbias_f16 launched with that row.  Tables mask the first key tile in full, a middle tile and the trailing tiles;
maps change region inside a wave's 32 queries, at wave and block boundaries and at a ragged last query, shared and per sample.
The measured ratios are in profiles/regions.md."""
import ctypes

import pytest
import torch

import refmix_refs as RR
import regions_refs as GR

pytestmark = pytest.mark.gpu

SENTINEL = 1234.0
_ids = lambda v: v if isinstance(v, str) else GR.case_id(v) if isinstance(v, tuple) else str(v)     # noqa: E731


def _dev(p):
    return p["q"].cuda(), p["k"].cuda(), p["vt"].cuda()


def _launch(p, dev, out=None, **kw):
    from lib.hip import ops
    B, H, Nq, Nk, D = p["dims"]
    d = p["desc"]
    q, k, vt = dev
    return ops.attention(q, k, vt, B, H, Nq, Nk, D, p["scale"], ldq=d["ldq"], ldk=d["ldk"], ldvt=d["ldvt"], q_bs=d["q_bs"],
                         k_bs=d["k_bs"], vt_bs=d["vt_bs"], out=out, **kw)


def _ratio(got, ref, bound):
    assert got.shape == ref.shape
    return float((got.double() - ref).abs().max()) / bound


@pytest.mark.parametrize("shared", [True, False], ids=["shared_map", "map_per_sample"])
@pytest.mark.parametrize("cls,case", GR.ALL_CASES, ids=_ids)
def test_rbias_attention_vs_fp64_and_vs_the_per_key_entry(cls, case, shared):
    """guards and poison, two launches with the same bits, every element against the bound; then, region by region, the bits of
    pfd_attention_kbias_f16 with that region's row wherever key 0 of the row is finite and both entries launch the same class"""
    assert GR.rbias_kernel_class(*case) == cls
    p = GR.problem(case)
    B, H, Nq, Nk, D = p["dims"]
    C, M = H * D, B * Nq
    dev = _dev(p)
    tab = GR.table(case).cuda()
    qreg = GR.region_map(case, shared).cuda()
    assert tab.shape[2] > Nk and bool(torch.isnan(tab[..., Nk:]).all())
    assert bool(torch.isneginf(tab[:, 0, :64]).all()) and bool(torch.isneginf(tab[:, 2, 64:min(128, Nk)]).all())
    buf = torch.full((M + 16, C + 16), SENTINEL, dtype=torch.float16, device="cuda")
    y = _launch(p, dev, out=buf[:M, 8:8 + C], rbias=tab, qregion=qreg)
    assert y.data_ptr() == buf[:M, 8:8 + C].data_ptr()
    assert bool((buf[M:] == SENTINEL).all()), "rows behind the last query were written"
    assert bool((buf[:M, :8] == SENTINEL).all()) and bool((buf[:M, 8 + C:] == SENTINEL).all()), "columns outside the slice were written"
    got = buf[:M, 8:8 + C].contiguous()
    assert bool(torch.isfinite(got).all()), "NaN from a pad position or a masked leading tile reached the output"
    assert not bool((got == SENTINEL).any()), "an output element was not written"
    assert torch.equal(_launch(p, dev, rbias=tab, qregion=qreg), got), "two launches, different bits"
    ref, T = GR.regional_ref(*dev, tab, qreg, B, H, Nq, Nk, D, p["scale"], **p["desc"])
    bound = GR.bound(Nk, D, p["vmax"], T, GR.table_max(tab, Nk))
    r = _ratio(got, ref.view(M, C), bound)
    print(f"[regions-kernels] {cls} {GR.case_id(case)} {'shared' if shared else 'per-sample'}: err / vmax {r * bound / p['vmax']:.3e}, / bound {r:.3f}")
    assert r <= 1.0, (cls, case, r)
    # the per-key entry, row by row
    same_class = RR.kbias_kernel_class(*case) == cls
    assert same_class
    got3 = got.view(B, Nq, C)
    regs = (qreg[None].expand(B, Nq) if shared else qreg).long()
    compared = 0
    for g in GR.KEY0_ROWS:
        sel = regs == g
        if not bool(sel.any()):
            continue
        assert bool(torch.isfinite(tab[:, g, 0]).all())
        one = _launch(p, dev, kbias=tab[:, g].contiguous()).view(B, Nq, C)
        assert torch.equal(one[sel], got3[sel]), f"region {g}: not the bits of pfd_attention_kbias_f16 with its row"
        compared += 1
    assert compared >= 2, "fewer than two regions with key 0 finite occur in this case"


@pytest.mark.parametrize("cls,case", [(c, GR.RBIAS_CASES[c][0]) for c in GR.RBIAS_CLASSES], ids=_ids)
@pytest.mark.parametrize("g", [3, 5])
def test_the_same_row_in_all_regions_is_the_per_key_entry_bit_for_bit(cls, case, g):
    p = GR.problem(case)
    B, H, Nq, Nk, D = p["dims"]
    dev = _dev(p)
    row = GR.table(case)[:, g].cuda()
    tab = row[:, None].repeat(1, GR.NR, 1).contiguous()
    qreg = GR.region_map(case, False).cuda()
    assert torch.equal(_launch(p, dev, rbias=tab, qregion=qreg), _launch(p, dev, kbias=row.contiguous()))


def test_the_folded_class_shape_is_served_by_the_4_wave_kernel():
    """(16, 8, 1024, 296, 40) is the folded 8-wave build's with per-key logits; there is no such build with regions, the 4-wave
    kernel takes it: against fp64 within the bound"""
    case = GR.W8_SHAPE
    assert RR.kbias_kernel_class(*case) == "w8" and GR.rbias_kernel_class(*case) == "w4"
    p = GR.problem(case)
    B, H, Nq, Nk, D = p["dims"]
    dev = _dev(p)
    tab = GR.table(case).cuda()
    qreg = GR.region_map(case, True).cuda()
    got = _launch(p, dev, rbias=tab, qregion=qreg)
    ref, T = GR.regional_ref(*dev, tab, qreg, B, H, Nq, Nk, D, p["scale"], **p["desc"])
    r = _ratio(got, ref.view(B * Nq, -1), GR.bound(Nk, D, p["vmax"], T, GR.table_max(tab, Nk)))
    print(f"[regions-kernels] w4 on the folded class's shape {GR.case_id(case)}: / bound {r:.3f}")
    assert bool(torch.isfinite(got).all()) and r <= 1.0, r


@pytest.mark.parametrize("cls", GR.RBIAS_CLASSES)
@pytest.mark.parametrize("mutant", GR.regions.MUTANTS)
def test_kernel_is_the_specification_where_the_mutants_are_not(mutant, cls):
    """the operands on which tests/test_regions_cpu.py shows `mutant` a thousand bounds from the specification, in every kernel
    class: the kernel is within one (region 1 masks the whole first key tile on all of them)"""
    p = GR.discriminating(mutant, cls)
    B, H, Nq, Nk, D = p["dims"]
    dev = _dev(p)
    tab = GR.padded_table(p["table"], Nk).cuda()
    qreg = p["qreg"].cuda()
    got = _launch(p, dev, rbias=tab, qregion=qreg)
    ref, T = GR.regional_ref(*dev, tab, qreg, B, H, Nq, Nk, D, p["scale"], **p["desc"])
    r = _ratio(got, ref.view(B * Nq, -1), GR.bound(Nk, D, p["vmax"], T, GR.table_max(tab, Nk)))
    print(f"[regions-kernels] {cls} operands of mutant {mutant}: / bound {r:.3f}")
    assert bool(torch.isfinite(got).all()) and r <= 1.0, (mutant, cls, r)


# ------------------------------------------------------------------------------------------------
# arguments
# ------------------------------------------------------------------------------------------------
def _args(B=2, H=2, Nq=16, Nk=16, D=40):
    C = H * D
    g = torch.Generator().manual_seed(1)
    q = torch.randn(B * Nq * C, generator=g).half().cuda()
    k = torch.randn(B * Nk * C, generator=g).half().cuda()
    vt = torch.randn(C * B * Nk, generator=g).half().cuda()
    kw = dict(ldq=C, ldk=C, ldvt=B * Nk, q_bs=Nq * C, k_bs=Nk * C, vt_bs=Nk)
    out = torch.full((B * Nq, C), SENTINEL, dtype=torch.float16, device="cuda")
    return q, k, vt, (B, H, Nq, Nk, D, D ** -0.5), kw, out


@pytest.mark.parametrize("D,Nk", [(96, 16), (512, 32)])
def test_rbias_rejects_unserved_head_sizes(D, Nk):
    from lib.hip import binding as _b, ops
    H = 1 if D == 512 else 2
    q, k, vt, dims, kw, out = _args(B=1, H=H, Nk=Nk, D=D)
    tab = torch.zeros((1, 2, Nk + 4), dtype=torch.float32, device="cuda")
    qr = torch.zeros(16, dtype=torch.uint8, device="cuda")
    with pytest.raises(_b.PfdError, match="PFD_ESHAPE"):
        ops.attention(q, k, vt, *dims, **kw, out=out, rbias=tab, qregion=qr)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())


def test_rbias_entry_point_and_ops_reject_bad_arguments():
    """the C entry point itself: PFD_EINVAL for rbias == NULL, a pointer 4 bytes into a 16-byte unit, rb_rs % 4 != 0, rb_rs < Nk,
    nr = 0 and 9, qregion == NULL, 0 < qr_bs < Nq; nothing is written.  ops.attention refuses the same before the call."""
    from lib.hip import binding as _b, ops
    q, k, vt, (B, H, Nq, Nk, D, scale), kw, out = _args()
    rs = Nk + 8
    tab = torch.zeros((B, 9, rs), dtype=torch.float32, device="cuda")
    qr = torch.zeros((B, Nq), dtype=torch.uint8, device="cuda")
    d = _b.PfdAttnDesc()
    d.Q, d.K, d.Vt, d.O = q.data_ptr(), k.data_ptr(), vt.data_ptr(), out.data_ptr()
    d.ldq, d.ldk, d.ldvt, d.ldo = kw["ldq"], kw["ldk"], kw["ldvt"], out.stride(0)
    d.q_bs, d.k_bs, d.vt_bs, d.o_bs = kw["q_bs"], kw["k_bs"], kw["vt_bs"], Nq * out.stride(0)
    d.B, d.H, d.Nq, d.Nk, d.D, d.scale = B, H, Nq, Nk, D, scale
    lib, s = _b.load(), torch.cuda.current_stream().cuda_stream
    T, R = tab.data_ptr(), qr.data_ptr()
    good = (T, rs, 9 * rs, 2, R, Nq)
    for bad in ((None, rs, 9 * rs, 2, R, Nq), (T + 4, rs, 9 * rs, 2, R, Nq), (T, Nk + 6, 9 * rs, 2, R, Nq),
                (T, Nk - 4, 9 * rs, 2, R, Nq), (T, rs, 9 * rs, 0, R, Nq), (T, rs, 9 * rs, 9, R, Nq), (T, rs, rs, 2, R, Nq),
                (T, rs, 9 * rs, 2, None, Nq), (T, rs, 9 * rs, 2, R, Nq - 1)):
        assert lib.pfd_attention_rbias_f16(ctypes.byref(d), *bad, s) == _b.PFD_EINVAL, bad
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    call = lambda **a: ops.attention(q, k, vt, B, H, Nq, Nk, D, scale, **kw, out=out, **a)     # noqa: E731
    t2 = tab[:, :2].contiguous()
    with pytest.raises(ValueError, match="come together"):
        call(rbias=t2)
    with pytest.raises(ValueError, match="exclude each other"):
        call(rbias=t2, qregion=qr, kbias=t2[:, 0].contiguous())
    with pytest.raises(ValueError, match="between 1 and 8"):
        call(rbias=tab, qregion=qr)
    with pytest.raises(ValueError, match="multiple of 4"):
        call(rbias=torch.zeros((B, 2, Nk + 2), dtype=torch.float32, device="cuda"), qregion=qr)
    with pytest.raises(ValueError, match="16-byte"):
        call(rbias=tab.view(-1)[1:1 + B * 2 * rs].view(B, 2, rs), qregion=qr)
    with pytest.raises(TypeError, match="float32"):
        call(rbias=t2.half(), qregion=qr)
    with pytest.raises(TypeError, match="uint8"):
        call(rbias=t2, qregion=qr.int())
    with pytest.raises(ValueError, match="qregion: expected"):
        call(rbias=t2, qregion=qr[:, :Nq - 1].contiguous())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        call(rbias=t2.cpu(), qregion=qr)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    for bad_scale in (0.0, -1.0, 2.0 ** -30, 2.0 ** 11, float("nan")):     # scale log2 e outside (2^-28, 2^10): the header's range
        d.scale = bad_scale
        assert lib.pfd_attention_rbias_f16(ctypes.byref(d), *good, s) == _b.PFD_EINVAL, bad_scale
    d.scale = scale
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    assert lib.pfd_attention_rbias_f16(ctypes.byref(d), *good, s) == 0
    torch.cuda.synchronize()
    assert not bool((out == SENTINEL).any())
    ref = out.clone()
    out.fill_(SENTINEL)
    call(rbias=t2, qregion=qr)
    assert torch.equal(out, ref)
