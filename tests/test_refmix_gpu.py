"""GPU (-m gpu): several references mixed in one UNet pass above the kernel -- SpatialTransformer.hip with a mixed ContextKV
against the plain fp64 block formulas of tests/block_refs.py extended by the weighted attention (refmix_refs), and
generate(image=[...], image_weights=[...]) / submit(...) on the small net: the collapse to the plain request bit for bit,
(1/2, 1/2) of one picture, the stages run by hand, graphed against eager, order invariance, the other request kinds, and the
server's batching.  This mixing is not the reference's context_mixing and is not compared with it."""
import threading

import numpy as np
import pytest
import torch

import block_refs as BR
import ops_standin as SI
import refmix_refs as RR
from lib import refmix

pytestmark = pytest.mark.gpu

T = torch.from_numpy
STEPS = 4


def rel_l2(a, ref):
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    return float((a - ref).norm() / ref.norm())


# ---- the block ---------------------------------------------------------------------------------------------------------
def _mixed_rows(B, t, pad=0):
    """[B, 2 t + pad]: two references of t tokens at 0.7 / 0.3, rotated per sample, -inf on the padding"""
    rows = [refmix.key_bias((0.7, 0.3) if b % 2 == 0 else (0.3, 0.7), t, 2 * t + pad) for b in range(B)]
    return T(np.stack(rows))


# (registered block case whose floor applies -- the weighted attention adds no store and no rounding site to the block --,
#  keyword arguments of block_refs.build_st, switches, what the unconditional half is)
BLOCKS = [("folded", "st-conv", dict(), {}, None),
          ("unfolded", "st-conv", dict(), {"LN_FOLD": False}, None),
          ("cfg-pair-zero-uncond", "st-pair", dict(cfg_pair=True, zero_lead=1), {}, None),
          ("padded-uncond", "st-conv", dict(), {}, "padded")]


@pytest.mark.parametrize("name,floor_of,kw,switches,uncond", BLOCKS, ids=[b[0] for b in BLOCKS])
def test_spatial_transformer_with_a_mixed_context(name, floor_of, kw, switches, uncond, monkeypatch):
    """within T = 4 f of the fp64 formula, f the floor of the registered block case with the same path (tests/test_blocks_gpu.py)"""
    from lib.model_zoo import attention as AT
    BR.apply_switches(monkeypatch, switches)
    b = BR.build_st(Nk=40, **kw)
    bias = _mixed_rows(b.B, 20)
    if uncond == "padded":                       # sample 0: an unconditional context of 20 tokens, zero tokens at -inf behind it
        b.inputs["ctx"][0, 20:] = 0
        bias[0, :20], bias[0, 20:] = 0.0, float("-inf")
    mods, inputs = BR._dev(b, "cuda")
    kv = AT.ContextKV(inputs["ctx"], bias.cuda())
    kv.zero_lead = kw.get("zero_lead", 0)
    y = mods["st"].hip(inputs["x"], kv, cfg_pair=kw.get("cfg_pair", False))
    with RR.weighted_cross_attention(bias.double()):
        ref = b.ref()
    plain = b.ref()
    case = dict(BR.CASE[floor_of])
    if switches:
        case["switches"] = dict(case.get("switches") or {}, **switches)
    Tol = 4 * SI.floor(case)
    e, moved = BR.err_units(y, ref, b.B), BR.err_units(ref, plain, b.B)
    print(f"[refmix] SpatialTransformer {name}: T {Tol:.3f} err {e:.3f} err / T {e / Tol:.3f}; the weights move the formula by {moved:.1f} units")
    assert e <= Tol and moved > 4 * Tol
    assert torch.equal(mods["st"].hip(inputs["x"], kv, cfg_pair=kw.get("cfg_pair", False)), y)


# (registered block case whose floor applies, mode of block_refs.build_unet)
UNETS = [("plain", "unet-plain", "plain"), ("cfg-pair-zero-uncond", "unet-cfg-pair", "cfg_pair"), ("control-residuals", "unet-control", "control")]


@pytest.mark.parametrize("name,floor_of,mode", UNETS, ids=[u[0] for u in UNETS])
def test_miniature_unet_walk_with_a_mixed_context(name, floor_of, mode):
    """UNetModel2D_Next.hip over a mixed ContextKV (two references of 20 tokens, rows differing per sample) against the fp64 walk
    of block_refs.unet with the weighted attention in every context block: plain, as a CFG pair whose unconditional half takes
    the zero-context shortcut, and with ControlNet residuals added to the middle block and the skips.  T = 4 f of the registered
    case with the same path (its context has 20 tokens instead of 40: the stores that f counts are the same)."""
    from lib.model_zoo import attention as AT
    b = BR.build_unet(mode=mode)
    pair = mode == "cfg_pair"
    z = b.B // 2 if pair else 0
    b.inputs["ctx"] = BR._ctx_input(b.B, 40, z, 33)
    bias = _mixed_rows(b.B, 20)
    mods, inputs = BR._dev(b, "cuda")
    kv = AT.ContextKV(inputs["ctx"], bias.cuda())
    kv.zero_lead = z
    ctrl = [inputs[f"c{n}"] for n in range(5)] if mode == "control" else None
    y = mods["net"].hip(inputs["x"], inputs["t"], kv, control=ctrl, cfg_pair=pair)
    with RR.weighted_cross_attention(bias.double()):
        ref = b.ref()
    plain = b.ref()
    Tol = 4 * SI.floor(BR.CASE[floor_of])
    e, moved = BR.err_units(y, ref, b.B), BR.err_units(ref, plain, b.B)
    print(f"[refmix] miniature UNet {name}: T {Tol:.3f} err {e:.3f} err / T {e / Tol:.3f}; the weights move the formula by {moved:.1f} units")
    assert e <= Tol and moved > 4 * Tol


# ---- generate ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def refs(golden):
    return T(golden["see.img"]), T(golden["see2.img"])


@pytest.fixture(scope="module")
def plain_A(net, refs):
    from lib.pipeline import PromptFreePipeline
    return PromptFreePipeline(net).generate(refs[0], 2, 64, 64, steps=STEPS, scale=2.0, seed=11, decode=False)[1]


@pytest.fixture(scope="module")
def mixed_73(net, refs):
    from lib.pipeline import PromptFreePipeline
    return PromptFreePipeline(net).generate(list(refs), 2, 64, 64, steps=STEPS, scale=2.0, seed=11, decode=False,
                                            image_weights=[0.7, 0.3])[1]


def test_weights_one_zero_are_the_first_reference_bit_for_bit(net, refs, plain_A):
    from lib.pipeline import PromptFreePipeline
    got = PromptFreePipeline(net).generate(list(refs), 2, 64, 64, steps=STEPS, scale=2.0, seed=11, decode=False,
                                           image_weights=[1.0, 0.0])[1]
    assert torch.equal(got, plain_A)


def test_the_same_reference_twice_is_the_single_reference(net, refs, plain_A):
    from lib.pipeline import PromptFreePipeline
    got = PromptFreePipeline(net).generate([refs[0], refs[0]], 2, 64, 64, steps=STEPS, scale=2.0, seed=11, decode=False,
                                           image_weights=[0.5, 0.5])[1]
    r = rel_l2(got, plain_A)
    print(f"[refmix] image=[A, A] at (1/2, 1/2) vs image=A: rel-L2 {r:.3e} (gate 1e-2), bits equal: {torch.equal(got, plain_A)}")
    assert r <= 1e-2


def test_mixed_request_equals_the_stages_run_by_hand(net, refs, mixed_73, plain_A):
    """SeeCoder per reference, tokens concatenated, refmix.key_bias, the sampler with c_info['key_bias']: the same bits; and
    the mix is neither of its references"""
    from lib.model_zoo.ddim import DDIMSampler
    from lib.pipeline import shard_xT
    toks = [net.ctx_encode(im.cuda(), 'image') for im in refs]
    nk = toks[0].shape[1]
    cond = torch.cat(toks, 1).repeat(2, 1, 1)
    bias = T(refmix.key_bias([0.7, 0.3], nk, 2 * nk)).cuda()[None].repeat(2, 1)
    xT = shard_xT(2, 64, 64, 11, 0, 1)
    c_info = {'type': 'image', 'conditioning': cond, 'unconditional_conditioning': torch.zeros_like(cond),
              'unconditional_guidance_scale': 2.0, 'key_bias': bias}
    want = DDIMSampler(net).sample(steps=STEPS, shape=list(xT.shape), x_info={'type': 'image', 'xt': xT.cuda()}, c_info=c_info,
                                   eta=0., verbose=False)[0]
    assert torch.equal(mixed_73, want)
    assert rel_l2(mixed_73, plain_A) > 1e-2


def test_graphed_equals_eager_and_plain_requests_keep_their_graph(net, refs, mixed_73, plain_A):
    from lib.pipeline import PromptFreePipeline
    pipe = PromptFreePipeline(net)
    pipe.enable_graph(True)
    kw = dict(steps=STEPS, scale=2.0, seed=11, decode=False)
    assert torch.equal(pipe.generate(list(refs), 2, 64, 64, image_weights=[0.7, 0.3], **kw)[1], mixed_73)
    assert len(pipe.sampler._graphs) == 1 and next(iter(pipe.sampler._graphs))[-1] == 'key_bias'
    other = pipe.generate(list(refs), 2, 64, 64, image_weights=[0.2, 0.8], **kw)[1]      # other weights: the same graph
    assert len(pipe.sampler._graphs) == 1 and not torch.equal(other, mixed_73)
    assert torch.equal(other, PromptFreePipeline(net).generate(list(refs), 2, 64, 64, image_weights=[0.2, 0.8], **kw)[1])
    assert torch.equal(pipe.generate(refs[0], 2, 64, 64, **kw)[1], plain_A)
    keys = list(pipe.sampler._graphs)
    assert len(keys) == 2 and keys[1][-1] != 'key_bias'                                  # the plain key is what it was


def test_the_order_of_the_references_is_immaterial(net, refs, mixed_73):
    from lib.pipeline import PromptFreePipeline
    got = PromptFreePipeline(net).generate([refs[1], refs[0]], 2, 64, 64, steps=STEPS, scale=2.0, seed=11, decode=False,
                                           image_weights=[0.3, 0.7])[1]
    r = rel_l2(got, mixed_73)
    print(f"[refmix] references swapped with their weights: rel-L2 {r:.3e} (gate 1e-2)")
    assert r <= 1e-2


@pytest.mark.parametrize("how", ["dpmpp_2m", "per-sample-scale", "init+mask", "uncond"])
def test_mixed_requests_of_every_kind(net, refs, mixed_73, how):
    """graphed against eager bit for bit, finite, and not the plain mixed request"""
    from lib.pipeline import PromptFreePipeline
    import img2img_refs as I
    kw = dict(steps=STEPS, scale=2.0, seed=11, decode=False, image_weights=[0.7, 0.3])
    if how == "dpmpp_2m":
        kw.update(solver='dpmpp_2m')
    elif how == "per-sample-scale":
        kw.update(scale=[1.5, 3.0])
    elif how == "init+mask":
        m = np.zeros((64, 64), dtype=np.uint8)
        m[16:48, 8:40] = 255
        kw.update(init=I.picture_u8(64, 64, seed=3), strength=0.75, mask=m)
    else:
        tok = net.ctx_encode(refs[1].cuda(), 'image')
        kw.update(uncond=(0.25 * tok).to(tok.dtype))                                      # 148 tokens against 296: padded
    eager = PromptFreePipeline(net).generate(list(refs), 2, 64, 64, **kw)[1]
    pipe = PromptFreePipeline(net)
    pipe.enable_graph(True)
    assert torch.equal(pipe.generate(list(refs), 2, 64, 64, **kw)[1], eager)
    assert bool(torch.isfinite(eager).all()) and eager.shape == mixed_73.shape and not torch.equal(eager, mixed_73)


def test_controlnet_attends_with_the_weights(net, refs):
    """a mixed request with a control picture: the ControlNet's own context layers take the same ContextKV.  Weights (1, 0) are
    the plain ControlNet request bit for bit; [A, A] at (1/2, 1/2) -- the ControlNet and the UNet through the kernels with the
    logits -- is the plain request within the gate; graphed equals eager; (0.7, 0.3) is another result"""
    from lib.pipeline import PromptFreePipeline
    ctl = torch.rand((1, 3, 64, 64), generator=torch.Generator().manual_seed(4))
    kw = dict(steps=STEPS, scale=2.0, seed=11, decode=False, control=ctl)
    pipe = PromptFreePipeline(net)
    plain = pipe.generate(refs[0], 2, 64, 64, **kw)[1]
    nocontrol = pipe.generate(refs[0], 2, 64, 64, steps=STEPS, scale=2.0, seed=11, decode=False)[1]
    assert rel_l2(plain, nocontrol) > 1e-2                                  # the ControlNet is in the path
    assert torch.equal(pipe.generate(list(refs), 2, 64, 64, image_weights=[1.0, 0.0], **kw)[1], plain)
    twice = pipe.generate([refs[0], refs[0]], 2, 64, 64, image_weights=[0.5, 0.5], **kw)[1]
    r = rel_l2(twice, plain)
    print(f"[refmix] with ControlNet, image=[A, A] at (1/2, 1/2) vs image=A: rel-L2 {r:.3e} (gate 1e-2)")
    assert r <= 1e-2
    mixed = pipe.generate(list(refs), 2, 64, 64, image_weights=[0.7, 0.3], **kw)[1]
    assert rel_l2(mixed, plain) > 1e-2 and bool(torch.isfinite(mixed).all())
    graphed = PromptFreePipeline(net)
    graphed.enable_graph(True)
    assert torch.equal(graphed.generate(list(refs), 2, 64, 64, image_weights=[0.7, 0.3], **kw)[1], mixed)


# ---- the server --------------------------------------------------------------------------------------------------------
def test_server_coalesces_mixed_requests_and_keeps_plain_ones_apart(net, refs):
    from lib.pipeline import PromptFreePipeline
    from lib.serving import PromptFreeServer
    A, Bp = refs
    Cp = Bp.flip(-1).contiguous()
    common = dict(steps=STEPS, as_uint8=False, height=64, width=64)
    submits = [(([A, Bp],), dict(seed=5, image_weights=[0.7, 0.3], **common)),
               ((A,), dict(seed=6, **common)),
               (([A, Bp, Cp],), dict(seed=7, image_weights=[0.5, 0.3, 0.2], **common))]
    srv = PromptFreeServer(net, use_graph=False, max_batch=4)
    try:
        gate = threading.Event()
        srv.call(lambda n: gate.wait(30))
        futs = [srv.submit(*submits[i][0], **submits[i][1]) for i in (0, 2, 1)]      # the two mixed ones adjacent: one batch
        gate.set()
        m2, m3, p1 = [f.result(300) for f in futs]
        assert srv.batches == [2, 1]
        gate = threading.Event()
        srv.call(lambda n: gate.wait(30))
        futs = [srv.submit(*a, **k) for a, k in submits]                             # the plain one between them: three batches
        gate.set()
        outs = [f.result(300) for f in futs]
        assert srv.batches == [2, 1, 1, 1, 1]
    finally:
        srv.close()
    pipe = PromptFreePipeline(net)
    solo = []
    for a, k in submits:
        kw = {x: v for x, v in k.items() if x not in ('as_uint8', 'height', 'width')}
        solo.append(pipe.generate(a[0], 1, 64, 64, scale=2.0, **kw)[0].float().cpu())
    assert torch.equal(p1.float().cpu(), solo[1]) and torch.equal(outs[1].float().cpu(), solo[1])     # the plain path, bit for bit
    for name, o, j in (("2 refs, coalesced", m2, 0), ("3 refs, coalesced", m3, 2), ("2 refs, alone", outs[0], 0), ("3 refs, alone", outs[2], 2)):
        r = rel_l2(o.float().cpu(), solo[j])
        print(f"[refmix] served {name} vs its solo run: rel-L2 {r:.3e} (gate 1e-2), bits equal: {torch.equal(o.float().cpu(), solo[j])}")
        assert r <= 1e-2
