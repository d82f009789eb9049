"""Block-level tests of the UNet host layer on the device: every case of tests/block_refs.py through the real `.hip` methods on
libpfd_hip.so against the plain fp64 formula, within T = 4 f (f: the floor of the case, the stand-in run of the same host path on
the CPU against the same formula -- see tests/test_blocks_cpu.py for why the margin is 4; T never depends on the device result).
Switch positions, carried state, the path census, repeatability and the host layer's argument errors."""
import os
import time

import pytest
import torch

import block_refs as BR
import kernel_refs as KR
import ops_standin as SI

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "block_paths.txt")
IDS = [c["id"] for c in BR.CASES]
_SPENT = [0.0]


@pytest.fixture(autouse=True)
def _clock():
    t = time.time()
    yield
    _SPENT[0] += time.time() - t
    print(f"[blocks-gpu] file total so far {_SPENT[0]:.1f} s")


@pytest.mark.parametrize("cid", IDS)
def test_case_on_device(cid):
    """.hip on the device within T of the fp64 formula; the census is the recorded one and names the case's branch; a second
    launch gives the same bits; the inputs are unchanged"""
    c = BR.CASE[cid]
    b = BR.built(cid)
    T = 4 * SI.floor(c)
    y, cen, same, kept = BR.run_gpu(c, census=True)
    e = BR.err_units(y, b.ref64, b.B)
    print(f"[blocks-gpu] {cid}: f {T / 4:.3f} T {T:.3f} err {e:.3f} err / T {e / T:.3f}")
    assert e <= T
    assert same, "second launch differs"
    assert kept, "an input was modified"
    gold = BR.read_golden_paths(GOLDEN)[cid]
    assert cen.log == gold
    assert c["branch"] in " ".join(cen.log), (c["branch"], cen.log)
    assert cen.again == cen.remembered(), "a run from the decline memory of the last one asked the library again"
    if b.gn_carried is not None:
        # wherever the output carries GroupNorm statistics: per (sample, producer group) they are the sums over the stored tensor
        # (summed over a sample's slabs, which does not depend on the row order the phase-folded upsample emits them in);
        # bound: fp32 sums of 64 N / 32 values per slab (tests/test_gemm_kernels_gpu.py), added over the slabs
        N = y.shape[-1]
        cpg, g = N // 32, 160 // (N // 32)
        stored = y.reshape(-1, N)
        want = KR.gn_out_ref(stored)[:, :, :g].reshape(b.B, -1, N // 160, g, 2)
        v = stored.double().reshape(-1, 64, N // 160, g, cpg)
        bnd = (64 * cpg * 2.0 ** -24 * torch.stack([v.abs().sum((1, 4)), (v * v).sum((1, 4))], -1)).reshape(want.shape)
        got = b.gn_carried[:, :, :g].double().reshape(want.shape)
        n_slab = want.shape[1]
        ratio = float(((got.sum(1) - want.sum(1)).abs() / (bnd.sum(1) + n_slab * 2.0 ** -24 * want.abs().sum(1))).max())
        print(f"[blocks-gpu] {cid}: carried gn statistics per sample err / bound {ratio:.3f}")
        assert ratio <= 1.0
    if b.ln_carried is not None:
        # the partial row sums CrossAttention.hip hands on: fp32 sums of 160 stored values (tests/test_gemm_kernels_gpu.py)
        stored, st = b.ln_carried
        M, N = stored.shape
        v = stored.double().reshape(M, N // 160, 160)
        bnd = 160 * 2.0 ** -24 * torch.stack([v.abs().sum(-1), (v * v).sum(-1)], -1)
        ratio = float(((st.double() - KR.ln_out_ref(stored)).abs() / bnd).max())
        print(f"[blocks-gpu] {cid}: carried ln statistics err / bound {ratio:.3f}")
        assert ratio <= 1.0


@pytest.mark.parametrize("cid", [c["id"] for c in BR.CASES if c["forward"]])
def test_forward_calling_convention(cid):
    """one case per class through .forward (NCHW / [B, N, C], any float dtype in)"""
    c = BR.CASE[cid]
    b = BR.built(cid)
    T = 4 * SI.floor(c, fwd=True)
    y = BR.run_gpu(c, fwd=True)[0]
    e = BR.err_units(y, BR.ref_of(b, True), b.B)
    print(f"[blocks-gpu] {cid} .forward: T {T:.3f} err {e:.3f} err / T {e / T:.3f}")
    assert e <= T


# (switch, case, further switches held, bit-equal positions).  Equal in bits where the existing tests demand it: the GroupNorm
# prologue with producer statistics and the fused reduction off (tests/test_hip_kernels_fullsize.py), the CFG pair without copies
# (tests/test_hip_parity.py)
_PLAIN_GN = {"GN_PSTATS": False, "fuse_reduce_groupnorm": False}
SWITCH_CASES = [("LN_FOLD", "btb-folded", {}, False), ("LN_FOLD", "st-conv", {}, False), ("GN_PSTATS", "rb-1x1-320-640", {}, False),
                ("GN_PSTATS", "unet-plain", {}, False), ("GEMM_FUSE", "rb-cat-320+320-a2", {}, False),
                ("GEMM_FUSE", "btb-folded-zhalf-77", {}, False), ("UPS_FOLD", "up-16-fold", {}, False),
                ("fuse_groupnorm", "rb-w32-prologue-x2", {}, False), ("fuse_groupnorm", "rb-w32-prologue", _PLAIN_GN, True),
                ("fuse_reduce_groupnorm", "rb-1280-next-res", {}, False), ("pair_without_copies", "st-pair", {}, True)]


@pytest.mark.parametrize("switch,cid,held,bits", SWITCH_CASES, ids=[f"{s}-{c}" for s, c, _, _ in SWITCH_CASES])
def test_switch_positions(switch, cid, held, bits):
    """each position against the reference (not only against the other one), the two within 2 T of each other"""
    b = BR.built(cid)
    ys, Ts = [], []
    for pos in (True, False):
        c = dict(BR.CASE[cid], switches=dict(BR.CASE[cid]["switches"], **held, **{switch: pos}))
        T = 4 * SI.floor(c)
        y = BR.run_gpu(c)[0]
        e = BR.err_units(y, b.ref64, b.B)
        print(f"[blocks-gpu] {cid} {switch}={pos}: T {T:.3f} err {e:.3f} err / T {e / T:.3f}")
        assert e <= T, (switch, pos)
        ys.append(y)
        Ts.append(T)
    d = max(BR.err_units(ys[0], ys[1].double(), b.B), BR.err_units(ys[1], ys[0].double(), b.B))
    print(f"[blocks-gpu] {cid} {switch}: positions differ by {d:.3f} (2 T = {2 * max(Ts):.3f}), equal bits: {torch.equal(ys[0], ys[1])}")
    assert d <= 2 * max(Ts)
    if bits:
        assert torch.equal(ys[0], ys[1])


# ------------------------------------------------------------------------------------------------
# carried state
# ------------------------------------------------------------------------------------------------
def _rb(cid):
    b = BR.built(cid)
    mods, inputs = BR._dev(b, "cuda")
    return b, mods, inputs


def test_carried_statistics_are_those_of_the_stored_tensor():
    from lib.hip import ops
    for cid, N in (("rb-identity-320", 320), ("rb-1x1-320-640", 640), ("up-16-nofold", 320), ("down-16", 320), ("st-conv", 320)):
        b, mods, inputs = _rb(cid)
        with pytest.MonkeyPatch.context() as mp:      # (the phase-folded upsample emits its slabs in another row order: 9-tap form)
            BR.apply_switches(mp, BR.CASE[cid]["switches"])
            h = b.run(mods, inputs)
        st = ops.get_gn_stats(h)
        assert st is not None, cid
        stored = h.detach().cpu().reshape(-1, N)
        cpg = N // 32
        want = KR.gn_out_ref(stored)[:, :, :160 // cpg]
        v = stored.double().reshape(-1, 64, N // 160, 160 // cpg, cpg)
        bnd = 64 * cpg * 2.0 ** -24 * torch.stack([v.abs().sum((1, 4)), (v * v).sum((1, 4))], -1)      # tests/test_gemm_kernels_gpu.py
        ratio = float(((st.cpu()[:, :, :160 // cpg].double() - want).abs() / bnd).max())
        print(f"[blocks-gpu] {cid}: carried gn statistics err / bound {ratio:.3f}")
        assert ratio <= 1.0, cid


def test_carried_normalised_result_and_its_invalidation():
    from lib.hip import ops
    from lib.model_zoo import openaimodel as OM
    b, mods, inputs = _rb("rb-1280-next-res")
    rb, nxt = mods["rb"], mods["next"]
    norm = nxt.in_layers[0]
    h = rb.hip(inputs["x"], inputs["semb"], next_norm=(norm, True))
    key = norm.fuse_key(True)
    y = ops.get_normed(h, key)
    assert y is not None, "the library did not serve the fused reduction at 4 x 8 x 8 x 1280 (the golden census says it does)"
    raw = h.detach().cpu().reshape(-1, 1280)
    g, be = norm.weight.detach().cpu().half(), norm.bias.detach().cpu().half()
    want = KR.groupnorm32_ref(raw, 64, g, be, norm.eps, True)
    ratio, used = KR.bound_ratio(y.detach().cpu().reshape(-1, 1280), want, KR.groupnorm32_allowance(raw, 64, g, be, norm.eps, True, 0.0))
    print(f"[blocks-gpu] carried normalised result err / bound {ratio:.3f} (allowance used {used:.3f})")
    assert ratio <= 1.0
    # a consumer with a SiLU it was not computed for, another eps, other parameters: not taken
    assert ops.get_normed(h, norm.fuse_key(False)) is None
    other = OM.normalization(1280).half().cuda()
    assert ops.get_normed(h, other.fuse_key(True)) is None
    gp, bp = norm._pk()
    assert ops.get_normed(h, (gp.data_ptr(), bp.data_ptr(), 1e-6, True)) is None
    assert norm.hip(h, silu=True) is y and norm.hip(h, silu=False) is not y
    # a write through a view of the tensor: statistics and normalised result are gone
    b2, mods2, inputs2 = _rb("rb-identity-320")
    h2 = mods2["rb"].hip(inputs2["x"], inputs2["semb"])
    assert ops.get_gn_stats(h2) is not None
    ops.add(h2[0:1], h2[1:2].contiguous(), out=h2[0:1])
    assert ops.get_gn_stats(h2) is None
    ops.add(h[0:1], h[1:2].contiguous(), out=h[0:1])
    assert ops.get_normed(h, key) is None and ops.get_gn_stats(h) is None
    assert norm.hip(h, silu=True) is not y


def test_declined_phase_fold_is_remembered_and_its_pack_dropped(monkeypatch):
    """Conv2d.hip at 8 x 8: the fold is asked of the library once, the folded pack is not kept, the 9-tap form serves"""
    from lib.hip import ops
    monkeypatch.setattr(ops, "_DECLINED", set())
    b, mods, inputs = _rb("up-8-declined")
    conv = mods["m"].conv
    asked = []
    real = ops.conv
    monkeypatch.setattr(ops, "conv", lambda *a, **k: (asked.append(k.get("ups")), real(*a, **k))[1])
    y1 = b.run(mods, inputs)
    assert asked == [2, True] and len(ops._DECLINED) == 1
    assert "w_ups" not in conv._pk_cache and "w" in conv._pk_cache
    y2 = b.run(mods, inputs)
    assert asked == [2, True, True], "a declined shape was asked again"
    assert "w_ups" not in conv._pk_cache and torch.equal(y1, y2)


# ------------------------------------------------------------------------------------------------
# argument errors of the host layer: raised before anything is launched
# ------------------------------------------------------------------------------------------------
def test_argument_errors_before_any_launch(monkeypatch):
    from lib.hip import ops
    from lib.model_zoo import attention as AT
    b, mods, inputs = _rb("attn-cross-192-add-rowvec")
    attn, norm, x = mods["attn"], mods["norm"], inputs["x"]
    kv = AT.ContextKV(inputs["ctx"])
    b3, mods3, inputs3 = _rb("attn-cross-zhalf")
    kv3 = AT.ContextKV(inputs3["ctx"])
    st3 = ops.ln_rowstats(inputs3["x"])
    stD = BR.seed_module(AT.SpatialTransformer(320, 8, 40, context_dim=768, disable_self_attn=True), 3).half().cuda()
    xs = BR.rand16((1, 8, 8, 320), 4).cuda()
    kvD = AT.ContextKV(BR.rand16((2, 20, 768), 5).cuda())
    kvD.zero_lead = 1
    torch.cuda.synchronize()
    launches = []
    for name in ("_launch", "_stream"):
        real = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda *a, _r=real, **k: (launches.append(1), _r(*a, **k))[1])
    with pytest.raises(ValueError, match="ln_foldable"):                    # ln= at a shape the fold does not serve
        attn.hip(x, 2, 64, kv, res=x, ln=(norm, torch.zeros(128, 1, 2, device="cuda")))
    with pytest.raises(ValueError, match="single=True"):                    # zero_lead is 0 here: not half the batch
        mods3["attn"].hip(inputs3["x"], 2, 64, kv3, res=inputs3["x"], ln=(mods3["norm"], st3), stats_out=True, single=True)
    kv3.zero_lead = 1
    with pytest.raises(ValueError, match="single=True"):                    # no statistics asked for
        mods3["attn"].hip(inputs3["x"][:64], 2, 64, kv3, res=inputs3["x"][:64], ln=(mods3["norm"], st3[:64]), single=True)
    with pytest.raises(ValueError, match="context batch"):
        mods3["attn"].hip(inputs3["x"], 4, 32, kv3, res=inputs3["x"])
    with pytest.raises(ValueError, match="cfg_pair needs"):
        stD.hip(xs, kvD, cfg_pair=True)
    assert not launches, f"{len(launches)} calls reached the library before the error"
    assert not kv._kv and not kv3._kv and not kvD._kv, "a context projection was computed before the error"
