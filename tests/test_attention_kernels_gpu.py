"""GPU (-m gpu): the six kernels behind pfd_attention_f16 (csrc/attention.hip, csrc/attention3_kernel.h), each reached through
ops.attention by the dispatcher's own rule (kernel_refs.attention_kernel_class; no environment hook except the per-launch
PFD_ATTN512_SLICES), against the plain fp64 references of tests/kernel_refs.py computed on the device.  Every element is held to
the per-element bound kernel_refs.attention_bound derives from the number formats; the folded-maximum kernels (w8, a3) also to the
sharp bound against the reference that shares their fp16 Q'.  Operands come in the layouts the models pass, with NaN in every
position a launch may read but must not use; outputs go to a column slice of a sentinel-filled buffer.
tests/test_attention_kernels_cpu.py qualifies the references and the operands; the measured ratios are in
profiles/attention_kernel_tests.md."""
import pytest
import torch

import kernel_refs as KR

pytestmark = pytest.mark.gpu

SENTINEL = 1234.0           # exact in fp16, far outside every result below


def _cls(case, slices=2):
    return KR.attention_kernel_class(*case[:5], slices=slices)


def _operands(p, zero_pads=False):
    """the three flat buffers on the device (Q and K share one when the layout fuses them)"""
    def put(name):
        t = p[name]
        if zero_pads:
            t = torch.where(p[name + "_valid"], t, torch.zeros((), dtype=torch.float16))
        return t.cuda()
    q = put("q")
    return q, (q if p["k"] is p["q"] else put("k")), put("vt")


def _launch(p, ops_, out=None):
    from lib.hip import ops
    B, H, Nq, Nk, D = p["dims"]
    d = p["desc"]
    q, k, vt = ops_
    return ops.attention(q[d["q_off"]:], k[d["k_off"]:], vt[d["vt_off"]:], B, H, Nq, Nk, D, p["scale"], ldq=d["ldq"], ldk=d["ldk"],
                         ldvt=d["ldvt"], q_bs=d["q_bs"], k_bs=d["k_bs"], vt_bs=d["vt_bs"], out=out)


def _ratio(got, ref, bound):
    assert got.shape == ref.shape
    return float((got.double() - ref).abs().max()) / bound


def _compare(case, variant=None, slices=2):
    """one case: guards and poison, three launches, zeros for NaNs, every element against the bound(s)"""
    p = KR.attention_problem(case, variant)
    B, H, Nq, Nk, D = p["dims"]
    C, M = H * D, B * Nq
    cls = _cls(case, slices)
    dev = _operands(p)
    buf = torch.full((M + 16, C + 16), SENTINEL, dtype=torch.float16, device="cuda")
    y = _launch(p, dev, out=buf[:M, 8:8 + C])
    assert y.data_ptr() == buf[:M, 8:8 + C].data_ptr()
    assert bool((buf[M:] == SENTINEL).all()), "rows behind the last query were written"
    assert bool((buf[:M, :8] == SENTINEL).all()) and bool((buf[:M, 8 + C:] == SENTINEL).all()), "columns outside the slice were written"
    got = buf[:M, 8:8 + C].contiguous()
    assert bool(torch.isfinite(got).all()), "NaN from a pad position reached the output (or an element is not finite)"
    assert not bool((got == SENTINEL).any()), "an output element was not written"
    for _ in range(2):
        assert torch.equal(_launch(p, dev), got), "two launches, different bits"
    assert torch.equal(_launch(p, _operands(p, zero_pads=True)), got), "the pad values changed the result"
    q, k, vt = dev
    ref = KR.attention_ref(q, k, vt, B, H, Nq, Nk, D, p["scale"], **p["desc"]).view(M, C)
    vmax = p["vmax"]
    A = KR.attention_fold_amplitude(q, k, B, H, Nq, Nk, D, p["scale"], **p["desc"]) if cls in KR.ATTN_FOLDED else 0.0
    r = _ratio(got, ref, KR.attention_bound(Nk, vmax, A))
    e = float((got.double() - ref).abs().max()) / vmax
    line = f"[attn-kernels] {cls} {KR.attn_case_id(case)}{' ' + variant if variant else ''}: err / vmax {e:.3e}, / bound {r:.3f}"
    rf = None
    if cls in KR.ATTN_FOLDED:
        reff = KR.attention_ref_folded(q, k, vt, B, H, Nq, Nk, D, p["scale"], **p["desc"]).view(M, C)
        rf = _ratio(got, reff, KR.attention_bound(Nk, vmax))
        line += f" (A = {A:.1f}); against the folded reference / sharp bound {rf:.3f}"
    print(line)
    assert r <= 1.0, (cls, case, variant, r)
    assert rf is None or rf <= 1.0, (cls, case, variant, rf)
    return got


# ------------------------------------------------------------------------------------------------
# every case, every element
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in KR.ATTN_CASES if c[4] != 512], ids=KR.attn_case_id)
def test_attention_vs_fp64(case):
    _compare(case)


@pytest.mark.parametrize("slices", [2, 4])
@pytest.mark.parametrize("case", [c for c in KR.ATTN_CASES if c[4] == 512], ids=KR.attn_case_id)
def test_attention512_vs_fp64(case, slices, monkeypatch):
    monkeypatch.setenv("PFD_ATTN512_SLICES", str(slices))
    _compare(case, slices=slices)


@pytest.mark.parametrize("case", KR.ATTN_STAIRCASE, ids=KR.attn_case_id)
def test_attention_staircase(case):
    """folded kernels: the tile maximum rises by 5 log2 units per tile -- odd tiles stay under the +6 threshold with P up to 2^5
    in fp16, even tiles take the rescale"""
    _compare(case, "staircase")


@pytest.mark.parametrize("case", KR.ATTN_PEAKED, ids=KR.attn_case_id)
def test_attention_peaked_rows(case):
    """four query rows x 6: rows dominated by one key (scores around +-80 log2 units)"""
    _compare(case, "peaked")


# ------------------------------------------------------------------------------------------------
# once per class
# ------------------------------------------------------------------------------------------------
PERMUTED = [(1, 2, 300, 148, 40, "dense", 0), (16, 8, 1024, 200, 40, "dense", 0), (32, 8, 256, 320, 40, "fused_qk", 0),
            (1, 2, 150, 148, 80, "dense", 0), (1, 3, 148, 148, 96, "dense", 0), (2, 2, 64, 148, 160, "dense", 0),
            (1, 1, 200, 96, 512, "dense", 0)]


def _dense_launch(p, q, k, vt, desc):
    from lib.hip import ops
    B, H, Nq, Nk, D = p["dims"]
    return ops.attention(q.cuda(), k.cuda(), vt.cuda(), B, H, Nq, Nk, D, p["scale"], **desc)


@pytest.mark.parametrize("case", PERMUTED, ids=KR.attn_case_id)
def test_attention_key_permutation(case, monkeypatch):
    """softmax . V does not depend on the order of the keys: permuting K rows together with V columns moves no element by more
    than the bound (both slice forms at d = 512)"""
    p = KR.attention_problem(case)
    B, H, Nq, Nk, D = p["dims"]
    C, Nkp = H * D, (Nk + 7) // 8 * 8
    q, k, vt, desc = KR.attention_densified(p)
    perm = torch.randperm(Nk, generator=torch.Generator().manual_seed(Nk))
    kp = k.view(B, Nk, C)[:, perm].reshape(-1)
    vtp = vt.view(C, B, Nkp).clone()
    vtp[:, :, :Nk] = vt.view(C, B, Nkp)[:, :, perm]
    A = KR.attention_fold_amplitude(q, k, B, H, Nq, Nk, D, p["scale"], **desc) if _cls(case) in KR.ATTN_FOLDED else 0.0
    for sl in ((2, 4) if D == 512 else (2,)):
        monkeypatch.setenv("PFD_ATTN512_SLICES", str(sl))
        a, b = _dense_launch(p, q, k, vt, desc), _dense_launch(p, q, kp, vtp.reshape(-1), desc)
        r = _ratio(a, b.double(), KR.attention_bound(Nk, p["vmax"], A))
        print(f"[attn-kernels] {_cls(case, sl)} {KR.attn_case_id(case)}: keys permuted, difference / bound {r:.3f}")
        assert r <= 1.0, (case, sl, r)


@pytest.mark.parametrize("case", [c for c in KR.ATTN_CASES if c[4] == 512], ids=KR.attn_case_id)
def test_attention512_slice_forms_agree(case, monkeypatch):
    p = KR.attention_problem(case)
    dev = _operands(p)
    outs = []
    for sl in (2, 4):
        monkeypatch.setenv("PFD_ATTN512_SLICES", str(sl))
        outs.append(_launch(p, dev))
    r = _ratio(outs[0], outs[1].double(), KR.attention_bound(case[3], p["vmax"]))
    print(f"[attn-kernels] d512 {KR.attn_case_id(case)}: 2 slices vs 4, difference / bound {r:.3f}")
    assert r <= 1.0, (case, r)


# ------------------------------------------------------------------------------------------------
# arguments
# ------------------------------------------------------------------------------------------------
def _args(B=1, H=2, Nq=16, Nk=16, D=40, slack=0):
    C = H * D
    g = torch.Generator().manual_seed(1)
    q = torch.randn(B * Nq * C + slack, generator=g).half().cuda()
    k = torch.randn(B * Nk * C + slack, generator=g).half().cuda()
    vt = torch.randn(C * B * Nk + slack, generator=g).half().cuda()
    kw = dict(ldq=C, ldk=C, ldvt=B * Nk, q_bs=Nq * C, k_bs=Nk * C, vt_bs=Nk)
    out = torch.full((B * Nq, C), SENTINEL, dtype=torch.float16, device="cuda")
    return q, k, vt, (B, H, Nq, Nk, D, D ** -0.5), kw, out


def test_attention_rejects_misaligned_operands():
    """PFD_EINVAL for ldq / ldk / ldvt / vt_bs that are no multiple of 8 and for a Q view that starts 8 bytes into a 16-byte
    unit; nothing is written"""
    from lib.hip import binding as _b, ops
    q, k, vt, dims, kw, out = _args(slack=64)
    for name in ("ldq", "ldk", "ldvt", "vt_bs"):
        with pytest.raises(_b.PfdError, match="PFD_EINVAL"):
            ops.attention(q, k, vt, *dims, **{**kw, name: kw[name] + 4}, out=out)
    with pytest.raises(_b.PfdError, match="PFD_EINVAL"):
        ops.attention(q[4:], k, vt, *dims, **kw, out=out)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    ops.attention(q, k, vt, *dims, **kw, out=out)              # (the same arguments are fine when aligned)
    assert not bool((out == SENTINEL).any())


@pytest.mark.parametrize("B,H,Nq,Nk,D", [(1, 2, 16, 16, 64), (1, 2, 16, 32, 512), (1, 1, 16, 40, 512)],
                         ids=["d64", "d512-two-heads", "d512-40-keys"])
def test_attention_rejects_unserved_shapes(B, H, Nq, Nk, D):
    from lib.hip import binding as _b, ops
    assert KR.attention_kernel_class(B, H, Nq, Nk, D) is None
    q, k, vt, dims, kw, out = _args(B, H, Nq, Nk, D)
    with pytest.raises(_b.PfdError, match="PFD_ESHAPE"):
        ops.attention(q, k, vt, *dims, **kw, out=out)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())


def test_ops_attention_validates_its_tensors():
    from lib.hip import ops
    q, k, vt, dims, kw, out = _args()
    M, C = out.shape
    for bad in ((q.cpu(), k, vt), (q, k.cpu(), vt), (q, k, vt.cpu())):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            ops.attention(*bad, *dims, **kw)
    for bad in ((q.float(), k, vt), (q, k.float(), vt), (q, k, vt.float())):
        with pytest.raises(TypeError, match="float16"):
            ops.attention(*bad, *dims, **kw)
    with pytest.raises(ValueError, match="innermost stride"):
        ops.attention(q.view(-1, 2)[:, 0], k, vt, *dims, **kw)
    wide = torch.full((M, 2 * C + 8), SENTINEL, dtype=torch.float16, device="cuda")
    with pytest.raises(TypeError):
        ops.attention(q, k, vt, *dims, **kw, out=out.float())
    with pytest.raises(RuntimeError):
        ops.attention(q, k, vt, *dims, **kw, out=out.cpu())
    with pytest.raises(ValueError):
        ops.attention(q, k, vt, *dims, **kw, out=wide[:, ::2])                   # column stride 2
    with pytest.raises(ValueError, match="attention: out"):
        ops.attention(q, k, vt, *dims, **kw, out=out[:M - 1])                    # a row short
    with pytest.raises(ValueError, match="attention: out"):
        ops.attention(q, k, vt, *dims, **kw, out=out[:, :C - 8])                 # eight columns short
    with pytest.raises(ValueError, match="attention: out"):
        ops.attention(q, k, vt, *dims, **kw, out=wide.view(-1)[:M * (C + 4)].view(M, C + 4))   # row stride % 8 != 0
    with pytest.raises(ValueError, match="attention: out"):
        ops.attention(q, k, vt, *dims, **kw, out=out.view(1, M, C))              # not a matrix
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((wide == SENTINEL).all())
    y = ops.attention(q, k, vt, *dims, **kw, out=wide[:, 8:8 + C])               # a column slice of a wider matrix is served
    assert bool((wide[:, :8] == SENTINEL).all()) and bool((wide[:, 8 + C:] == SENTINEL).all())
    assert torch.equal(y, ops.attention(q, k, vt, *dims, **kw))
