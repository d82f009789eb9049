"""GPU (-m gpu): pfd_attention_kbias_f16 (csrc/attention.hip: attention_kbias_kernel, the text of attention2_kernel compiled with KBIAS) -- attention with an
additive logit per key, the kernel under several reference pictures mixed in one UNet pass (lib/refmix.py).  Each of its four
kernel classes is reached through ops.attention(kbias=...) by the dispatcher's own rule and held, element by element, to
lib/refmix.weighted_attention in fp64 on the device (refmix_refs.weighted_ref, pinned to the numpy specification by
tests/test_refmix_cpu.py) within refmix_refs.kbias_bound; the folded class (w8) also to the sharp bound against the reference
that shares its fp16 Q'.  Operands, NaN poison and the sentinel buffer are those of tests/test_attention_kernels_gpu.py, except
that K and V of a -inf key are finite (the contract).  The measured ratios are in profiles/refmix.md."""
import ctypes

import pytest
import torch

import kernel_refs as KR
import refmix_refs as RR

pytestmark = pytest.mark.gpu

SENTINEL = 1234.0


def _dev(p):
    return p["q"].cuda(), p["k"].cuda(), p["vt"].cuda()


def _launch(p, dev, kbias=None, out=None, Nk=None):
    from lib.hip import ops
    B, H, Nq, Nk0, D = p["dims"]
    d = p["desc"]
    q, k, vt = dev
    return ops.attention(q, k, vt, B, H, Nq, Nk0 if Nk is None else Nk, D, p["scale"], ldq=d["ldq"], ldk=d["ldk"], ldvt=d["ldvt"],
                         q_bs=d["q_bs"], k_bs=d["k_bs"], vt_bs=d["vt_bs"], out=out, kbias=kbias)


def _ratio(got, ref, bound):
    assert got.shape == ref.shape
    return float((got.double() - ref).abs().max()) / bound


def _refs(p, dev, bias):
    """(plain reference, bound against it, folded reference or None, sharp bound) for one launch"""
    B, H, Nq, Nk, D = p["dims"]
    q, k, vt = dev
    ref, T = RR.weighted_ref(q, k, vt, bias, B, H, Nq, Nk, D, p["scale"], **p["desc"])
    Bmax, vmax = RR.bias_max(bias, Nk), p["vmax"]
    cls = RR.kbias_kernel_class(B, H, Nq, Nk, D)
    if cls != "w8":
        return ref.view(B * Nq, H * D), RR.kbias_bound(Nk, D, vmax, T, Bmax), None, None
    A = KR.attention_fold_amplitude(q, k, B, H, Nq, Nk, D, p["scale"], **p["desc"])
    reff, Tf = RR.weighted_ref(q, k, vt, bias, B, H, Nq, Nk, D, p["scale"], **p["desc"], folded=True)
    return (ref.view(B * Nq, H * D), RR.kbias_bound(Nk, D, vmax, T, Bmax, A), reff.view(B * Nq, H * D),
            RR.kbias_bound(Nk, D, vmax, Tf, Bmax))


@pytest.mark.parametrize("pattern", RR.PATTERNS)
@pytest.mark.parametrize("cls,case", RR.ALL_CASES, ids=lambda v: v if isinstance(v, str) else RR.case_id(v))
def test_kbias_attention_vs_fp64(cls, case, pattern):
    """guards and poison, two launches with the same bits, every element against the bound(s)"""
    assert RR.kbias_kernel_class(*case) == cls
    p = RR.problem(case)
    B, H, Nq, Nk, D = p["dims"]
    C, M = H * D, B * Nq
    dev = _dev(p)
    bias = RR.bias_rows(case, pattern).cuda()
    assert bias.shape[1] > Nk and bool(torch.isnan(bias[:, Nk:]).all())
    buf = torch.full((M + 16, C + 16), SENTINEL, dtype=torch.float16, device="cuda")
    y = _launch(p, dev, bias, out=buf[:M, 8:8 + C])
    assert y.data_ptr() == buf[:M, 8:8 + C].data_ptr()
    assert bool((buf[M:] == SENTINEL).all()), "rows behind the last query were written"
    assert bool((buf[:M, :8] == SENTINEL).all()) and bool((buf[:M, 8 + C:] == SENTINEL).all()), "columns outside the slice were written"
    got = buf[:M, 8:8 + C].contiguous()
    assert bool(torch.isfinite(got).all()), "NaN from a pad position reached the output (or an element is not finite)"
    assert not bool((got == SENTINEL).any()), "an output element was not written"
    assert torch.equal(_launch(p, dev, bias), got), "two launches, different bits"
    ref, bound, reff, sharp = _refs(p, dev, bias)
    r = _ratio(got, ref, bound)
    line = f"[refmix-kernels] {cls} {RR.case_id(case)} {pattern}: err / vmax {r * bound / p['vmax']:.3e}, / bound {r:.3f}"
    rf = None
    if reff is not None:
        rf = _ratio(got, reff, sharp)
        line += f"; against the folded reference / sharp bound {rf:.3f}"
    print(line)
    assert r <= 1.0, (cls, case, pattern, r)
    assert rf is None or rf <= 1.0, (cls, case, pattern, rf)


# one case per class for the properties below (the first of each class that has more than one key tile)
ONE_PER_CLASS = [("w4", (1, 2, 300, 148, 40)), ("w8", (13, 8, 1030, 148, 40)), ("d80", (1, 2, 150, 296, 80)),
                 ("d160", (2, 2, 64, 296, 160))]
_ids = lambda v: v if isinstance(v, str) else RR.case_id(v)     # noqa: E731


@pytest.mark.parametrize("cls,case", RR.ALL_CASES, ids=_ids)
def test_zero_bias_is_the_plain_kernel_bit_for_bit(cls, case):
    """an all-zero bias against ops.attention without one: the same bits wherever pfd_attention_f16 launches the same kernel class"""
    p = RR.problem(case)
    assert KR.attention_kernel_class(*case) == cls, "the plain entry point takes another kernel here"
    dev = _dev(p)
    bias = RR.bias_rows(case, "zero").cuda()
    assert torch.equal(_launch(p, dev, bias), _launch(p, dev))


def test_zero_bias_where_the_plain_entry_takes_attention3():
    """(32, 8, 256, 128, 40) is attention3_kernel's without a bias and the 4-wave kernel's with one: compared within the bound"""
    case = (32, 8, 256, 128, 40)
    assert KR.attention_kernel_class(*case) == "a3" and RR.kbias_kernel_class(*case) == "w4"
    p = RR.problem(case)
    B, H, Nq, Nk, D = case
    dev = _dev(p)
    bias = torch.zeros((B, RR.kb_stride(Nk)), dtype=torch.float32, device="cuda")
    a, b = _launch(p, dev, bias), _launch(p, dev)
    A = KR.attention_fold_amplitude(*dev[:2], B, H, Nq, Nk, D, p["scale"], **p["desc"])
    ref, T = RR.weighted_ref(*dev, bias, B, H, Nq, Nk, D, p["scale"], **p["desc"])
    ra = _ratio(a, ref.view(B * Nq, -1), RR.kbias_bound(Nk, D, p["vmax"], T, 0.0))
    rb = _ratio(b, ref.view(B * Nq, -1), KR.attention_bound(Nk, p["vmax"], A))
    print(f"[refmix-kernels] zero bias on an a3 shape: biased w4 / bound {ra:.3f}, plain a3 / its bound {rb:.3f}, bits equal: {torch.equal(a, b)}")
    assert ra <= 1.0 and rb <= 1.0, (ra, rb)


@pytest.mark.parametrize("cls,case", ONE_PER_CLASS, ids=_ids)
def test_trailing_masked_keys_equal_the_shorter_launch(cls, case):
    """keys Nk' .. Nk - 1 at -inf against the same launch with Nk' keys (Nk' = 84: a partly masked tile, then tiles masked in
    full), within the bound; whether the bits are equal is reported"""
    p = RR.problem(case)
    B, H, Nq, Nk, D = case
    short = 84
    dev = _dev(p)
    bias = torch.zeros((B, RR.kb_stride(Nk)), dtype=torch.float32, device="cuda")
    bias[:, short:] = float("-inf")
    a = _launch(p, dev, bias)
    b = _launch(p, dev, bias[:, :RR.kb_stride(short)].contiguous(), Nk=short)
    ref, T = RR.weighted_ref(*dev, bias, B, H, Nq, Nk, D, p["scale"], **p["desc"])
    A = KR.attention_fold_amplitude(*dev[:2], B, H, Nq, Nk, D, p["scale"], **p["desc"]) if cls == "w8" else 0.0
    bound = RR.kbias_bound(Nk, D, p["vmax"], T, 0.0, A)
    ra, rb = _ratio(a, ref.view(B * Nq, -1), bound), _ratio(b, ref.view(B * Nq, -1), bound)
    print(f"[refmix-kernels] {cls} {RR.case_id(case)}: keys {short}.. masked / bound {ra:.3f}, {short}-key launch / bound {rb:.3f}, "
          f"bits equal: {torch.equal(a, b)}")
    assert ra <= 1.0 and rb <= 1.0, (ra, rb)
    assert _ratio(a, b.double(), bound) <= 1.0


@pytest.mark.parametrize("cls,case", ONE_PER_CLASS, ids=_ids)
def test_duplicate_and_permutation_invariance(cls, case):
    """every key twice at logit - 1 is the original; permuting keys together with their V columns and logits changes nothing --
    both within the bound"""
    from lib.hip import ops
    p = RR.problem(case)
    B, H, Nq, Nk, D = case
    C = H * D
    q, k, vt, desc = KR.attention_densified(p)
    Nkp = (Nk + 7) // 8 * 8
    bias = RR.bias_rows(case, "three")[:, :Nk]
    A = KR.attention_fold_amplitude(q, k, B, H, Nq, Nk, D, p["scale"], **desc) if cls == "w8" else 0.0

    def run(k_, vt_, bias_, nk):
        nkp = (nk + 7) // 8 * 8
        kb = torch.full((B, RR.kb_stride(nk)), float("nan"), dtype=torch.float32)
        kb[:, :nk] = bias_
        return ops.attention(q.cuda(), k_.cuda(), vt_.cuda(), B, H, Nq, nk, D, p["scale"], ldq=C, ldk=C, ldvt=B * nkp, q_bs=Nq * C,
                             k_bs=nk * C, vt_bs=nkp, kbias=kb.cuda())
    base = run(k, vt, bias, Nk)
    ref, T = RR.weighted_ref(q.cuda(), k.cuda(), vt.cuda(), bias.cuda(), B, H, Nq, Nk, D, p["scale"], **desc)
    bound = RR.kbias_bound(2 * Nk, D, p["vmax"], T + 1.0, RR.bias_max(bias, Nk) + 1.0, A)
    # duplicates
    k2 = torch.cat([k.view(B, Nk, C)] * 2, 1).reshape(-1)
    v = vt.view(C, B, Nkp)[:, :, :Nk]
    vt2 = torch.zeros((C, B, 2 * Nk + (-2 * Nk) % 8), dtype=torch.float16)
    vt2[:, :, :2 * Nk] = torch.cat([v, v], 2)
    dup = run(k2, vt2.reshape(-1), torch.cat([bias, bias], 1) - 1.0, 2 * Nk)
    # permutation
    perm = torch.randperm(Nk, generator=torch.Generator().manual_seed(Nk))
    at0 = int((perm == 0).nonzero()[0, 0])                                   # key 0 (finite for every sample) stays first
    perm[at0], perm[0] = int(perm[0]), 0
    vtp = torch.zeros((C, B, Nkp), dtype=torch.float16)
    vtp[:, :, :Nk] = v[:, :, perm]
    per = run(k.view(B, Nk, C)[:, perm].reshape(-1), vtp.reshape(-1), bias[:, perm], Nk)
    rd, rp = _ratio(dup, base.double(), bound), _ratio(per, base.double(), bound)
    r0 = _ratio(base, ref.view(B * Nq, -1), bound)
    print(f"[refmix-kernels] {cls} {RR.case_id(case)}: keys doubled at -1 / bound {rd:.3f}, keys permuted / bound {rp:.3f} (base {r0:.3f})")
    assert rd <= 1.0 and rp <= 1.0 and r0 <= 1.0, (rd, rp, r0)


# ------------------------------------------------------------------------------------------------
# arguments
# ------------------------------------------------------------------------------------------------
def _args(B=1, H=2, Nq=16, Nk=16, D=40):
    C = H * D
    g = torch.Generator().manual_seed(1)
    q = torch.randn(B * Nq * C, generator=g).half().cuda()
    k = torch.randn(B * Nk * C, generator=g).half().cuda()
    vt = torch.randn(C * B * Nk, generator=g).half().cuda()
    kw = dict(ldq=C, ldk=C, ldvt=B * Nk, q_bs=Nq * C, k_bs=Nk * C, vt_bs=Nk)
    out = torch.full((B * Nq, C), SENTINEL, dtype=torch.float16, device="cuda")
    return q, k, vt, (B, H, Nq, Nk, D, D ** -0.5), kw, out


@pytest.mark.parametrize("D,Nk", [(96, 16), (512, 32)])
def test_kbias_rejects_unserved_head_sizes(D, Nk):
    from lib.hip import binding as _b, ops
    H = 1 if D == 512 else 2
    q, k, vt, dims, kw, out = _args(H=H, Nk=Nk, D=D)
    kb = torch.zeros((1, Nk + 4), dtype=torch.float32, device="cuda")
    with pytest.raises(_b.PfdError, match="PFD_ESHAPE"):
        ops.attention(q, k, vt, *dims, **kw, out=out, kbias=kb)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    ops.attention(q, k, vt, *dims, **kw, out=out)                       # (the plain entry point serves them)
    assert not bool((out == SENTINEL).any())


def test_kbias_entry_point_rejects_null_and_misaligned_logits():
    """the C entry point itself: PFD_EINVAL for kbias == NULL, a pointer 4 bytes into a 16-byte unit, kb_bs % 4 != 0 and
    kb_bs < Nk; nothing is written.  ops.attention refuses the same before the call."""
    from lib.hip import binding as _b, ops
    q, k, vt, (B, H, Nq, Nk, D, scale), kw, out = _args()
    kb = torch.zeros((B, Nk + 8), dtype=torch.float32, device="cuda")
    d = _b.PfdAttnDesc()
    d.Q, d.K, d.Vt, d.O = q.data_ptr(), k.data_ptr(), vt.data_ptr(), out.data_ptr()
    d.ldq, d.ldk, d.ldvt, d.ldo = kw["ldq"], kw["ldk"], kw["ldvt"], out.stride(0)
    d.q_bs, d.k_bs, d.vt_bs, d.o_bs = kw["q_bs"], kw["k_bs"], kw["vt_bs"], Nq * out.stride(0)
    d.B, d.H, d.Nq, d.Nk, d.D, d.scale = B, H, Nq, Nk, D, scale
    lib, s = _b.load(), torch.cuda.current_stream().cuda_stream
    for ptr, bs in ((None, Nk + 8), (kb.data_ptr() + 4, Nk + 8), (kb.data_ptr(), Nk + 6), (kb.data_ptr(), Nk - 4)):
        assert lib.pfd_attention_kbias_f16(ctypes.byref(d), ptr, bs, s) == _b.PFD_EINVAL, (ptr, bs)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    with pytest.raises(ValueError, match="16-byte"):
        ops.attention(q, k, vt, B, H, Nq, Nk, D, scale, **kw, out=out, kbias=kb.view(-1)[1:1 + B * (Nk + 4)], kb_bs=Nk + 4)
    with pytest.raises(ValueError, match="multiple of 4"):
        ops.attention(q, k, vt, B, H, Nq, Nk, D, scale, **kw, out=out, kbias=kb, kb_bs=Nk + 6)
    with pytest.raises(TypeError, match="float32"):
        ops.attention(q, k, vt, B, H, Nq, Nk, D, scale, **kw, out=out, kbias=kb.half())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.attention(q, k, vt, B, H, Nq, Nk, D, scale, **kw, out=out, kbias=kb.cpu())
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    assert lib.pfd_attention_kbias_f16(ctypes.byref(d), kb.data_ptr(), Nk + 8, s) == 0
    torch.cuda.synchronize()
    assert not bool((out == SENTINEL).any())


@pytest.mark.parametrize("cls", RR.KBIAS_CLASSES)
@pytest.mark.parametrize("mutant", RR.refmix.MUTANTS)
def test_kernel_is_the_specification_where_the_mutants_are_not(mutant, cls):
    """the operands on which tests/test_refmix_cpu.py shows `mutant` a thousand bounds from the specification, in every kernel
    class (refmix_refs.DISC_DIMS reaches each by the dispatcher's rule): the kernel is within one (masked keys 12 to 40 log2
    units above the live ones, weights of 2^-40, every score at -12); w8 also within the sharp bound of the folded reference"""
    p = RR.discriminating(mutant, cls)
    B, H, Nq, Nk, D = p["dims"]
    assert RR.kbias_kernel_class(B, H, Nq, Nk, D) == cls
    dev = _dev(p)
    bias = torch.full((B, RR.kb_stride(Nk)), float("nan"), dtype=torch.float32)
    bias[:, :Nk] = p["bias"]
    bias = bias.cuda()
    got = _launch(p, dev, bias)
    ref, bound, reff, sharp = _refs(p, dev, bias)
    r = _ratio(got, ref, bound)
    rf = None if reff is None else _ratio(got, reff, sharp)
    print(f"[refmix-kernels] {cls} operands of mutant {mutant}: / bound {r:.3f}" + ("" if rf is None else f", / sharp bound {rf:.3f}"))
    assert bool(torch.isfinite(got).all()) and r <= 1.0 and (rf is None or rf <= 1.0), (mutant, cls, r, rf)
