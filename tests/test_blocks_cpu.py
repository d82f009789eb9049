"""Block-level tests of the UNet host layer (lib/hip/layers.py, lib/model_zoo/openaimodel.py, lib/model_zoo/attention.py) without a
GPU: the real `.hip` methods run over tests/ops_standin.py, a torch stand-in of lib.hip.ops, and are compared with the plain fp64
formulas of tests/block_refs.py.

  floor      f = err of the stand-in run (every optional form served) against the fp64 formula: what rounding to fp16 at the
             documented stores alone costs.  err = max_e |y_e - ref_e| / (|ref_e| + rms(ref over the sample)) in units of 2^-11.
  tolerance  T = 4 f.  The HIP path rounds at the same stores and adds at most one further rounding of comparable size per store
             (f16 split-K slabs, the staged value in front of a residual, W o gamma in fp16), its fp32 accumulation is invisible at
             these depths (profiles/gemm_kernel_tests.md: at most 0.002 of the allowance), and a factor of two remains for the
             maximum over 10^4 to 10^5 elements.  T comes from the reference side only.
  separation every wrong variant of block_refs.WRONG, in fp64, is at least 4 T away on some case of every block class it applies to.
"""
import os

import pytest
import torch
import torch.nn.functional as F

import block_refs as BR
import kernel_refs as KR
import ops_standin as SI
import pfd_oracle as O

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "block_paths.txt")
IDS = [c["id"] for c in BR.CASES]


# ------------------------------------------------------------------------------------------------
# the formulas, in fp32, against the oracle (which tests/test_oracle_golden.py pins to the reference itself)
# ------------------------------------------------------------------------------------------------
def _rel(a, b):
    return float((a.double() - b.double()).abs().max() / b.double().abs().max())


def _sd32(cid, name):
    return {k: v.float() for k, v in BR.built(cid).mods[name].state_dict().items()}


def test_formulas_pinned_to_oracle(monkeypatch):
    f32 = torch.float32
    b = BR.built("rb-1x1-320-640")
    sd = _sd32("rb-1x1-320-640", "rb")
    x, emb = BR.nchw(b.inputs["x"].float()), b.inputs["semb"].float()
    assert _rel(BR.res_block(BR.P(sd, dtype=f32), x, F.silu(emb)), O.res_block(O.SD(sd), x, emb)) <= 1e-5
    b = BR.built("rb-3x3skip")
    sd = _sd32("rb-3x3skip", "rb")
    assert _rel(BR.res_block(BR.P(sd, dtype=f32), x, F.silu(emb)), O.res_block(O.SD(sd), x, emb)) <= 1e-5
    b = BR.built("rb-cat-640+320-straddle")                        # the virtual concat is torch.cat in front of the oracle
    sd = _sd32("rb-cat-640+320-straddle", "rb")
    x1, x2 = BR.nchw(b.inputs["x"].float()), BR.nchw(b.inputs["x2"].float())
    assert _rel(BR.res_block(BR.P(sd, dtype=f32), x1, F.silu(emb), x2), O.res_block(O.SD(sd), torch.cat([x1, x2], 1), emb)) <= 1e-5
    for cid, f, g in (("up-16-fold", BR.upsample, lambda p, v: O.conv2d(p.sub("conv."), F.interpolate(v, scale_factor=2, mode="nearest"), padding=1)),
                      ("down-9x7", BR.downsample, lambda p, v: O.conv2d(p.sub("op."), v, stride=2, padding=1))):
        b, sd = BR.built(cid), _sd32(cid, "m")
        v = BR.nchw(b.inputs["x"].float())
        assert _rel(f(BR.P(sd, dtype=f32), v), g(O.SD(sd), v)) <= 1e-5
    b, sd = BR.built("btb-folded"), _sd32("btb-folded", "blk")
    t, ctx = b.inputs["x"].float().reshape(2, 64, 320), b.inputs["ctx"].float()
    p, q = BR.P(sd, dtype=f32), O.SD(sd)
    assert _rel(BR.cross_attention(p.sub("attn1."), t, None, 8), O.cross_attention(q.sub("attn1."), t, None, 8)) <= 1e-5
    assert _rel(BR.cross_attention(p.sub("attn2."), t, ctx, 8), O.cross_attention(q.sub("attn2."), t, ctx, 8)) <= 1e-5
    assert _rel(BR.basic_transformer_block(p, t, ctx, 8), O.basic_transformer_block(q, t, ctx, 8)) <= 1e-5
    b, sd = BR.built("st-conv"), _sd32("st-conv", "st")
    v, ctx = BR.nchw(b.inputs["x"].float()), b.inputs["ctx"].float()
    assert _rel(BR.spatial_transformer(BR.P(sd, dtype=f32), v, ctx, 8), O.spatial_transformer(O.SD(sd), v, ctx, 8)) <= 1e-5
    # the walk: the oracle's own order lists for this configuration, with and without control residuals and mixing
    monkeypatch.setattr(O, "unet_layout", lambda *a, **k: _layout())
    for cid in ("unet-plain", "unet-control", "unet-mix"):
        b, sd = BR.built(cid), _sd32(cid, "net")
        i = b.inputs
        v = BR.nchw(i["x"].float())
        p = BR.P(sd, dtype=f32)
        if cid == "unet-mix":
            sd2 = _sd32(cid, "net2")
            mine = BR.unet(b.mods["net"], p, v, i["t"], [(p, i["ctx"].float(), 0.7), (BR.P(sd2, dtype=f32), i["ctx2"].float(), 0.8)], 8)
            both = dict(sd)
            both.update({"n2." + k: t for k, t in sd2.items()})
            theirs = _oracle_mix(monkeypatch, both, v, i["t"], [("", i["ctx"].float(), 0.7), ("n2.", i["ctx2"].float(), 0.8)])
        else:
            ctrl = [BR.nchw(i[f"c{n}"].float()) for n in range(5)] if cid == "unet-control" else None
            mine = BR.unet(b.mods["net"], p, v, i["t"], [(p, i["ctx"].float(), 1.0)], 8, ctrl)
            theirs = O.unet_apply(sd, "", v, i["t"], i["ctx"].float(), ctrl)
        assert _rel(mine, theirs) <= 1e-5, cid


_layout_orig = O.unet_layout


def _layout():
    return _layout_orig(channel_mult=(1, 2), num_res_blocks=(1, 1), attention_resolutions=(1, 2))


class _Mix:
    def __init__(self, items):
        self.items = items


def _oracle_mix(monkeypatch, sd, x, t, ctxs):
    """O.unet_apply's multi-context form runs every context through the SAME net's transformers; the mixing of pfd.py:366-386 runs
    context i through net i's.  Here: the oracle's own walk and its own spatial_transformer per (net, context), mixed the way
    O.unet_apply mixes (ratios normalised to 1)"""
    real = O.spatial_transformer
    tot = sum(r for _, _, r in ctxs)

    def st(q, h, context, heads):
        if isinstance(context, _Mix):
            tail = q.prefix                                          # "context_blocks.<i>.0."
            return sum(real(O.SD(sd, pre + tail), h, c, heads) * (r / tot) for pre, c, r in context.items)
        return real(q, h, context, heads)
    monkeypatch.setattr(O, "spatial_transformer", st)
    return O.unet_apply(sd, "", x, t, _Mix(ctxs))


# ------------------------------------------------------------------------------------------------
# floor, tolerance, separation
# ------------------------------------------------------------------------------------------------
def test_every_wrong_variant_is_separated():
    """every variant, in fp64, is >= 4 T from the formula on some case of every block class it applies to"""
    best = {}
    for c in BR.CASES:
        if not c["sep"]:
            continue
        b = BR.built(c["id"])
        T = 4 * SI.floor(c)
        for w in b.applies:
            assert w in BR.WRONG, w
            e = BR.err_units(b.ref(wrong=w), b.ref64, b.B) / T
            if e > best.get((w, c["cls"]), ("", -1.0))[1]:
                best[(w, c["cls"])] = (c["id"], e)
    print("\nvariant                       class      best case                         err / T")
    for (w, cls), (cid, e) in sorted(best.items()):
        print(f"{w:29s} {cls:10s} {cid:32s} {e:9.1f}")
    assert {w for w, _ in best} == set(BR.WRONG), set(BR.WRONG) - {w for w, _ in best}
    weak = {k: v for k, v in best.items() if v[1] < 4.0}
    assert not weak, f"variants no case separates at 4 T: {weak}"


@pytest.mark.parametrize("mode", ["serve", "decline"])
@pytest.mark.parametrize("cid", IDS)
def test_host_path_over_standin(cid, mode):
    """the real .hip methods over the stand-in, every optional form served / declined: within T of the fp64 formula, nothing
    reaches the real library"""
    c = BR.CASE[cid]
    b = BR.built(cid)
    f = SI.floor(c)
    assert 0 < f < 16, f"floor {f}: the stand-in path itself is far from the formula"
    y, _, pol = SI.run_standin(c, mode)
    e = BR.err_units(y, b.ref64, b.B)
    print(f"{cid} {mode}: f {f:.3f} T {4 * f:.3f} err {e:.3f} asked {pol.asked}")
    assert e <= 4 * f
    if mode == "decline":
        assert not any(served for _, served in pol.asked)
    assert not SI.FELL_THROUGH


@pytest.mark.parametrize("cid", IDS)
def test_census_equals_golden(cid):
    """the calls the host layer makes on the CPU, with the stand-in declining what the recorded device run says the library
    declined, are the recorded ones; the branch the case is written for is among them"""
    c = BR.CASE[cid]
    gold = BR.read_golden_paths(GOLDEN)
    assert set(gold) == set(IDS)
    _, cen, _ = SI.run_standin(c, BR.golden_decisions(gold[cid]), census=True)
    assert cen.log == gold[cid]
    assert c["branch"] in " ".join(cen.log), (c["branch"], cen.log)
    # a further run from the decline memory this one left: what was declined is not asked of the library again
    assert cen.again == cen.remembered()
    b = BR.built(cid)
    if b.ln_carried is not None:
        # a SLICE check: the stand-in forms these sums with ln_out_ref itself, so only a host layer that hands on the sums of
        # other rows (the zero_rows / add_rowvec / single paths assemble them from parts) can fail here; values: the GPU file
        stored, st = b.ln_carried
        assert torch.equal(st, KR.ln_out_ref(stored).float())


def test_declined_phase_fold_is_remembered_and_its_pack_dropped(monkeypatch):
    """Conv2d.hip: the fold is asked once per shape, the folded pack is not kept after a decline, the 9-tap form serves"""
    from lib.hip import ops
    pol = SI.install(monkeypatch, SI.Policy("serve"))
    b = BR.built("up-8-declined")
    mods, inputs = BR._dev(b, "cpu")
    conv = mods["m"].conv
    y1 = b.run(mods, inputs)
    assert pol.asked == [("ups2", False)] and len(ops._DECLINED) == 1
    assert "w_ups" not in conv._pk_cache and "w" in conv._pk_cache
    y2 = b.run(mods, inputs)
    assert pol.asked == [("ups2", False)], "a declined shape was asked again"
    assert "w_ups" not in conv._pk_cache and torch.equal(y1, y2)
    b16 = BR.built("up-16-fold")                                   # another shape is asked, and served
    m16, i16 = BR._dev(b16, "cpu")
    b16.run(m16, i16)
    assert pol.asked == [("ups2", False), ("ups2", True)] and "w_ups" in m16["m"].conv._pk_cache


def test_device_guards_still_raise_on_cpu():
    from lib.hip import layers as L
    from lib.model_zoo import attention as AT
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        L._dev16(torch.zeros(4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        AT.ContextKV(torch.zeros(1, 8, 64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        L.Linear(64, 64)._pk()


def test_standin_uses_what_it_is_handed(monkeypatch):
    """the stand-in normalises with the statistics it is handed, so a host layer that hands over a wrong slice is seen"""
    from lib.hip import ops
    SI.install(monkeypatch)
    x, g, be = KR.ln_operands(64, 320, 3)
    w = BR.rand16((320, 320), 4, 320 ** -0.5)
    from lib.hip import layers as L
    wg, cs, bp = L.fold_layernorm(w, None, g, be)
    st = ops.ln_rowstats(x)
    good = ops.gemm(x, wg, bias=bp, ln=(st, cs, 1e-5)).double()
    ref = F.linear(F.layer_norm(x.double(), (320,), g.double(), be.double(), 1e-5), w.double())
    assert float((good - ref).abs().max()) < 0.02
    bad = ops.gemm(x, wg, bias=bp, ln=(st.roll(1, 0).contiguous(), cs, 1e-5)).double()
    assert float((bad - ref).abs().max()) > 0.2
    # GroupNorm from carried statistics: the producer's, not recomputed
    a = BR.rand16((128, 320), 5)
    o = ops.gemm(a, w, gn_out=True)
    y = ops.set_gn_stats(o.view(2, 8, 8, 320), ops.get_gn_stats(o))
    gam, bet = BR.rand16((320,), 6, 0.2, 1.0), BR.rand16((320,), 7, 0.1)
    n1 = ops.groupnorm(y, gam, bet, 32, 1e-5).double()
    refn = KR.groupnorm_ref(y.view(128, 320), None, 2, 64, 32, gam, bet, 1e-5, False).view(2, 8, 8, 320)
    assert float((n1 - refn).abs().max()) < 0.01
    ops.set_gn_stats(y, ops.get_gn_stats(y).flip(0).contiguous())
    assert float((ops.groupnorm(y, gam, bet, 32, 1e-5).double() - refn).abs().max()) > 0.05


# ------------------------------------------------------------------------------------------------
# host-only packers against their definitions, in fp64
# ------------------------------------------------------------------------------------------------
@pytest.fixture
def cpu_params(monkeypatch):
    from lib.hip import layers as L
    monkeypatch.setattr(L, "_require_gpu", lambda t, message: None)


def test_pack_conv_weight(cpu_params):
    from lib.hip import layers as L
    w = BR.rand16((64, 128, 3, 3), 1)
    x = BR.rand16((2, 5, 6, 128), 2)
    pk = L.pack_conv_weight(w)
    assert pk.shape == (64, 9 * 128)
    X = KR.gemm_conv_operand(x.double(), (3, 1, 1, 0, 5, 6))
    got = (X @ pk.double().t()).view(2, 5, 6, 64)
    ref = BR.nhwc(F.conv2d(BR.nchw(x.double()), w.double(), padding=1))
    assert float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max())
    w4 = BR.rand16((32, 4, 3, 3), 3)                               # K = 36 -> padded to 64 with zeros
    pk = L.pack_conv_weight(w4)
    assert pk.shape == (32, 64) and float(pk[:, 36:].abs().max()) == 0
    assert torch.equal(pk[:, :36].view(32, 3, 3, 4), w4.permute(0, 2, 3, 1))


def test_pack_conv_weight_ups_is_conv_of_nearest_2x():
    from lib.hip import layers as L
    w = torch.randn(8, 16, 3, 3, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    x = torch.randn(2, 5, 7, 16, dtype=torch.float64, generator=torch.Generator().manual_seed(2))
    wf = L.pack_conv_weight_ups(w, dtype=torch.float64)
    assert wf.shape == (4, 8, 64)
    xp = F.pad(x, (0, 0, 1, 1, 1, 1))
    got = torch.empty(2, 10, 14, 8, dtype=torch.float64)
    for py in range(2):
        for px in range(2):            # output pixel (2y+py, 2x+px) reads the low-res pixels (y+py-1+ty, x+px-1+tx) (include/pfd_hip.h)
            acc = 0
            for ty in range(2):
                for tx in range(2):
                    t = ty * 2 + tx
                    acc = acc + xp[:, py + ty:py + ty + 5, px + tx:px + tx + 7] @ wf[py * 2 + px][:, t * 16:(t + 1) * 16].t()
            got[:, py::2, px::2] = acc
    ref = BR.nhwc(F.conv2d(F.interpolate(BR.nchw(x), scale_factor=2, mode="nearest"), w, padding=1))
    assert float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max())


def test_fold_layernorm_identity():
    """LN(x) W^T + b == rstd (x W'^T - mean s) + b' in fp64, the fp16 rounding of W' the only difference"""
    from lib.hip import layers as L
    x, g, be = KR.ln_operands(32, 320, 5)
    w, b = BR.rand16((96, 320), 6, 320 ** -0.5), BR.rand16((96,), 7, 0.1)
    wg, cs, bp = L.fold_layernorm(w, b, g, be)
    assert wg.dtype == torch.float16 and cs.dtype == torch.float32 and bp.dtype == torch.float16
    xd = x.double()
    mean = xd.mean(1, keepdim=True)
    rstd = 1 / torch.sqrt((xd * xd).mean(1, keepdim=True) - mean * mean + 1e-5)
    W1 = w.double() * g.double()                                    # W' before its rounding
    b1 = (w.double() * be.double()).sum(1) + b.double()
    ref = F.linear(F.layer_norm(xd, (320,), g.double(), be.double(), 1e-5), w.double(), b.double())
    exact = rstd * (xd @ W1.t() - mean * W1.sum(1)) + b1
    assert float((exact - ref).abs().max()) <= 1e-12 * float(ref.abs().max())
    assert torch.equal(wg, W1.half())
    assert float((bp.double() - b1).abs().max()) <= 2.0 ** -11 * float(b1.abs().max()) + 320 * 2.0 ** -24 * float((w.double() * be.double()).abs().sum(1).max())
    assert float((cs.double() - wg.double().sum(1)).abs().max()) <= 320 * 2.0 ** -24 * float(wg.double().abs().sum(1).max())
    got = rstd * (xd @ wg.double().t() - mean * cs.double()) + bp.double()
    bound = float((rstd * (xd.abs() @ (W1 - wg.double()).abs().t() + mean.abs() * (W1 - wg.double()).abs().sum(1))).max()) + 2.0 ** -11 * float(b1.abs().max()) + 1e-6
    assert float((got - exact).abs().max()) <= bound


def test_geglu_interleave_for_both_group_sizes(cpu_params):
    from lib.hip import binding
    from lib.model_zoo import attention as AT
    lib = binding.load()
    groups = set()
    for dim_in, n in ((320, 1280), (64, 96), (128, 160), (64, 32)):
        gr = int(lib.pfd_gemm_geglu_group(2 * n))
        groups.add(gr)
        m = BR.seed_module(AT.GEGLU(dim_in, n), n)
        wi, bi = m._pk()
        wx, wg = KR.geglu_unpack(wi, gr)
        assert torch.equal(torch.cat([wx, wg]), m.proj.weight.half()), (n, gr)
        bx, bg = KR.geglu_unpack(bi.reshape(-1, 1), gr)
        assert torch.equal(torch.cat([bx, bg]).reshape(-1), m.proj.bias.half())
        # by index: packed row (j // gr) * 2 gr + h * gr + j % gr holds logical row h * n + j
        j = torch.arange(n)
        for h in (0, 1):
            assert torch.equal(wi[(j // gr) * 2 * gr + h * gr + j % gr], m.proj.weight.half()[h * n + j])
    assert groups == {2, 32}, f"the library reports the group sizes {groups}"


def test_stacked_qkv_packs(cpu_params):
    from lib.hip import layers as L
    from lib.model_zoo import attention as AT
    a = BR.seed_module(AT.CrossAttention(320, None, 8, 40), 3)
    q, k, v = (t.weight.half() for t in (a.to_q, a.to_k, a.to_v))
    assert torch.equal(a._pk_qk(), torch.cat([q, k]))
    assert torch.equal(a._pk_qkv(), torch.cat([q, k, v]))
    n = BR.seed_module(L.LayerNorm(320), 4)
    wg, cs, bp = a._pk_qkv_ln(n)
    W1 = torch.cat([q, k, v]).float() * n.weight.float()
    assert torch.equal(wg, W1.half()) and torch.equal(bp, (torch.cat([q, k, v]).float() * n.bias.float()).sum(1).half())
    assert torch.equal(cs, wg.float().sum(1))


def test_emb_pack_column_map(cpu_params):
    from lib.model_zoo import openaimodel as OM
    net = BR.built("unet-plain").mods["net"]
    net = __import__("copy").deepcopy(net)
    w, bias, cols = net._emb_pack()
    blocks = [m for seq in net.data_blocks for m in seq if isinstance(m, OM.ResBlock)]
    assert w.shape == (sum(b.out_channels for b in blocks), 1280) and len(cols) == len(blocks)
    spans = []
    for b in blocks:
        c0 = cols[id(b)]
        assert torch.equal(w[c0:c0 + b.out_channels], b.emb_layers[1].weight.half())
        assert torch.equal(bias[c0:c0 + b.out_channels], b.emb_layers[1].bias.half())
        spans.append((c0, c0 + b.out_channels))
    spans.sort()
    assert spans[0][0] == 0 and all(a[1] == b[0] for a, b in zip(spans, spans[1:])) and spans[-1][1] == w.shape[0]
