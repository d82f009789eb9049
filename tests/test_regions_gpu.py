"""GPU (-m gpu): regional reference mixing above the kernel -- generate(image=[...], regions=, region_weights=) on the small net at
64 x 64 pixels, 2 samples: one region is the image_weights request bit for bit, a map of all zeros with rows (1, 0) / (0, 1) is
the plain request of reference 0, a left / right map equals the stages run by hand (SeeCoder per reference, regions.region_bias,
the sampler with c_info['region_bias'] / ['region_map']), swapping references and columns together, graphed against eager with a
second map replaying the same graph, and one case each with DPM-Solver++, img2img plus mask and a control picture.
In front of them the blocks: SpatialTransformer.hip and the miniature UNet walk over a regional ContextKV -- plain, as a CFG pair
with the zero-context shortcut, with ControlNet residuals -- against the fp64 block formulas of tests/block_refs.py extended by the
regional attention (regions_refs.regional_cross_attention), at the floors tests/test_refmix_gpu.py uses for the same blocks."""
import numpy as np
import pytest
import torch

import block_refs as BR
import ops_standin as SI
import regions_refs as GR
from lib import regions

pytestmark = pytest.mark.gpu

T = torch.from_numpy
STEPS = 4
KW = dict(steps=STEPS, scale=2.0, seed=11, decode=False)


def rel_l2(a, ref):
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    return float((a - ref).norm() / ref.norm())


# ---- the blocks --------------------------------------------------------------------------------------------------------
def _regional_kv(b, z=0):
    """the query grids the block's context layers run (learnt from one pass of the fp64 formula), a table and a map per grid,
    the ContextKV built from them -> (kv, tab, maps)"""
    from lib.model_zoo import attention as AT
    seen = set()
    with GR.regional_cross_attention(None, None, seen):
        b.ref()
    sizes = sorted(seen, reverse=True)
    tab, maps = GR.block_regions(b.B, 20, sizes)
    mods, inputs = BR._dev(b, "cuda")
    qmaps = torch.cat([maps[n] for n in sizes], 1).contiguous().cuda()
    kv = AT.ContextKV(inputs["ctx"], None, (tab.cuda(), qmaps, sizes))
    kv.zero_lead = z
    return mods, inputs, kv, tab, maps


BLOCKS = [("folded", "st-conv", dict(), {}), ("unfolded", "st-conv", dict(), {"LN_FOLD": False}),
          ("cfg-pair-zero-uncond", "st-pair", dict(cfg_pair=True, zero_lead=1), {})]


@pytest.mark.parametrize("name,floor_of,kw,switches", BLOCKS, ids=[b[0] for b in BLOCKS])
def test_spatial_transformer_with_a_regional_context(name, floor_of, kw, switches, monkeypatch):
    """within T = 4 f of the fp64 formula, f the floor of the registered block case with the same path"""
    BR.apply_switches(monkeypatch, switches)
    b = BR.build_st(Nk=40, **kw)
    mods, inputs, kv, tab, maps = _regional_kv(b, kw.get("zero_lead", 0))
    y = mods["st"].hip(inputs["x"], kv, cfg_pair=kw.get("cfg_pair", False))
    with GR.regional_cross_attention(tab.double(), maps):
        ref = b.ref()
    plain = b.ref()
    case = dict(BR.CASE[floor_of])
    if switches:
        case["switches"] = dict(case.get("switches") or {}, **switches)
    Tol = 4 * SI.floor(case)
    e, moved = BR.err_units(y, ref, b.B), BR.err_units(ref, plain, b.B)
    print(f"[regions] SpatialTransformer {name}: T {Tol:.3f} err {e:.3f} err / T {e / Tol:.3f}; the regions move the formula by {moved:.1f} units")
    assert e <= Tol and moved > 4 * Tol
    assert torch.equal(mods["st"].hip(inputs["x"], kv, cfg_pair=kw.get("cfg_pair", False)), y)


UNETS = [("plain", "unet-plain", "plain"), ("cfg-pair-zero-uncond", "unet-cfg-pair", "cfg_pair"), ("control-residuals", "unet-control", "control")]


@pytest.mark.parametrize("name,floor_of,mode", UNETS, ids=[u[0] for u in UNETS])
def test_miniature_unet_walk_with_a_regional_context(name, floor_of, mode):
    """UNetModel2D_Next.hip over a regional ContextKV (two references of 20 tokens, three regions, one map per query grid of the
    walk, rows and maps differing per sample) against the fp64 walk of block_refs.unet with the regional attention in every
    context block: plain, as a CFG pair whose unconditional half takes the zero-context shortcut, and with ControlNet residuals"""
    b = BR.build_unet(mode=mode)
    pair = mode == "cfg_pair"
    z = b.B // 2 if pair else 0
    b.inputs["ctx"] = BR._ctx_input(b.B, 40, z, 33)
    mods, inputs, kv, tab, maps = _regional_kv(b, z)
    assert len(maps) >= 2                                                       # more than one query grid: a map per level
    ctrl = [inputs[f"c{n}"] for n in range(5)] if mode == "control" else None
    y = mods["net"].hip(inputs["x"], inputs["t"], kv, control=ctrl, cfg_pair=pair)
    with GR.regional_cross_attention(tab.double(), maps):
        ref = b.ref()
    plain = b.ref()
    Tol = 4 * SI.floor(BR.CASE[floor_of])
    e, moved = BR.err_units(y, ref, b.B), BR.err_units(ref, plain, b.B)
    print(f"[regions] miniature UNet {name}: T {Tol:.3f} err {e:.3f} err / T {e / Tol:.3f}; the regions move the formula by {moved:.1f} units")
    assert e <= Tol and moved > 4 * Tol


# ---- generate ----------------------------------------------------------------------------------------------------------
def _lr_map(Hm=48, Wm=80):
    m = np.zeros((Hm, Wm), dtype=np.uint8)
    m[:, Wm // 2:] = 1
    return m


@pytest.fixture(scope="module")
def refs(golden):
    return T(golden["see.img"]), T(golden["see2.img"])


@pytest.fixture(scope="module")
def pipe(net):
    from lib.pipeline import PromptFreePipeline
    return PromptFreePipeline(net)


@pytest.fixture(scope="module")
def plain_A(pipe, refs):
    return pipe.generate(refs[0], 2, 64, 64, **KW)[1]


@pytest.fixture(scope="module")
def left_right(pipe, refs):
    """reference A alone on the left half (its row masks the whole of B), B alone on the right (masks A: the first key tiles)"""
    return pipe.generate(list(refs), 2, 64, 64, regions=_lr_map(), region_weights=[[1.0, 0.0], [0.0, 1.0]], **KW)[1]


def test_one_region_is_the_image_weights_request_bit_for_bit(pipe, refs):
    want = pipe.generate(list(refs), 2, 64, 64, image_weights=[0.7, 0.3], **KW)[1]
    got = pipe.generate(list(refs), 2, 64, 64, regions=np.zeros((5, 7), dtype=np.uint8), region_weights=[[0.7, 0.3]], **KW)[1]
    assert torch.equal(got, want)


def test_a_map_of_all_zeros_is_the_plain_request_of_reference_0(pipe, refs, plain_A):
    """regions (1, 0) / (0, 1), every query in region 0: the tokens of B are masked for every query, and a masked key
    contributes exactly nothing -- the bits of generate(image=A)"""
    got = pipe.generate(list(refs), 2, 64, 64, regions=np.zeros((64, 64), dtype=np.uint8),
                        region_weights=[[1.0, 0.0], [0.0, 1.0]], **KW)[1]
    print(f"[regions] all-zero map vs the plain request: rel-L2 {rel_l2(got, plain_A):.3e}, bits equal: {torch.equal(got, plain_A)}")
    assert torch.equal(got, plain_A)


def test_left_right_map_equals_the_stages_run_by_hand(net, refs, left_right, plain_A):
    from lib.model_zoo.ddim import DDIMSampler
    from lib.pipeline import shard_xT
    toks = [net.ctx_encode(im.cuda(), 'image') for im in refs]
    nk = toks[0].shape[1]
    cond = torch.cat(toks, 1).repeat(2, 1, 1)
    table = T(regions.region_bias([[1.0, 0.0], [0.0, 1.0]], nk, 2 * nk)).cuda()[None].repeat(2, 1, 1)
    assert bool(torch.isneginf(table[:, 1, :nk]).all()) and nk >= 64           # region 1 masks the first key tile in full
    xT = shard_xT(2, 64, 64, 11, 0, 1)
    c_info = {'type': 'image', 'conditioning': cond, 'unconditional_conditioning': torch.zeros_like(cond),
              'unconditional_guidance_scale': 2.0, 'region_bias': table, 'region_map': _lr_map()}
    want = DDIMSampler(net).sample(steps=STEPS, shape=list(xT.shape), x_info={'type': 'image', 'xt': xT.cuda()}, c_info=c_info,
                                   eta=0., verbose=False)[0]
    assert bool(torch.isfinite(left_right).all())
    assert torch.equal(left_right, want)
    assert rel_l2(left_right, plain_A) > 1e-2


def test_swapping_references_and_columns_together_changes_nothing(pipe, refs, left_right):
    """(the gate of the order test of tests/test_refmix_gpu.py: the keys are summed in another order)"""
    got = pipe.generate([refs[1], refs[0]], 2, 64, 64, regions=_lr_map(), region_weights=[[0.0, 1.0], [1.0, 0.0]], **KW)[1]
    r = rel_l2(got, left_right)
    print(f"[regions] references and columns swapped: rel-L2 {r:.3e} (gate 1e-2)")
    assert r <= 1e-2


def test_graphed_equals_eager_and_a_second_map_replays_the_same_graph(net, refs, left_right, plain_A):
    from lib.pipeline import PromptFreePipeline
    g = PromptFreePipeline(net)
    g.enable_graph(True)
    rw = [[1.0, 0.0], [0.0, 1.0]]
    assert torch.equal(g.generate(list(refs), 2, 64, 64, regions=_lr_map(), region_weights=rw, **KW)[1], left_right)
    assert len(g.sampler._graphs) == 1 and next(iter(g.sampler._graphs))[-1][0] == 'regions'
    tb = np.ascontiguousarray(_lr_map(64, 64).T)                                          # top / bottom, another size
    other = g.generate(list(refs), 2, 64, 64, regions=tb, region_weights=rw, **KW)[1]
    assert len(g.sampler._graphs) == 1 and not torch.equal(other, left_right)
    assert torch.equal(other, PromptFreePipeline(net).generate(list(refs), 2, 64, 64, regions=tb, region_weights=rw, **KW)[1])
    assert torch.equal(g.generate(refs[0], 2, 64, 64, **KW)[1], plain_A)
    keys = list(g.sampler._graphs)
    assert len(keys) == 2 and not (isinstance(keys[1][-1], tuple) and keys[1][-1][:1] == ('regions',))   # the plain key is what it was


@pytest.mark.parametrize("how", ["dpmpp_2m", "init+mask", "control"])
def test_regional_requests_of_every_kind(net, refs, golden, how):
    from lib.pipeline import PromptFreePipeline
    kw = dict(KW, regions=_lr_map(), region_weights=[[1.0, 0.25], [0.0, 1.0]])
    if how == "dpmpp_2m":
        kw["solver"] = "dpmpp_2m"
    elif how == "init+mask":
        import img2img_refs as I
        m = np.zeros((64, 64), dtype=np.uint8)
        m[16:48, 8:40] = 255
        kw.update(init=I.picture_u8(64, 64, seed=3), strength=0.75, mask=m)
    else:
        kw["control"] = torch.rand((1, 3, 64, 64), generator=torch.Generator().manual_seed(6))
    eager = PromptFreePipeline(net).generate(list(refs), 2, 64, 64, **kw)[1]
    gp = PromptFreePipeline(net)
    gp.enable_graph(True)
    assert bool(torch.isfinite(eager).all())
    assert torch.equal(gp.generate(list(refs), 2, 64, 64, **kw)[1], eager)
    same = PromptFreePipeline(net).generate(list(refs), 2, 64, 64, **dict(kw, regions=np.zeros((8, 8), dtype=np.uint8)))[1]
    assert not torch.equal(same, eager)                                                    # the map matters


def test_generate_checks_the_regional_arguments_before_the_device(pipe, refs):
    m = _lr_map()
    for kw, msg in ((dict(regions=m), "together"), (dict(regions=m, region_weights=[[1, 0], [0, 1]], image_weights=[1, 1]), "exclude"),
                    (dict(regions=m, region_weights=[[1, 0]]), "only 1 regions"), (dict(regions=m, region_weights=[[1, 0, 1], [0, 1, 1]]), "reference pictures"),
                    (dict(regions=m.astype(np.int32), region_weights=[[1, 0], [0, 1]]), "uint8"),
                    (dict(regions=m, region_weights=[[1, 0], [0, 0]]), "at least one")):
        with pytest.raises(ValueError, match=msg):
            pipe.generate(list(refs), 2, 64, 64, **KW, **kw)


# ---- the server --------------------------------------------------------------------------------------------------------
def test_server_coalesces_regional_requests_and_keeps_a_plain_one_apart(net, refs):
    """two regional requests (maps of different sizes, different weights) share one batch and equal the direct calls within the
    gate tests/test_refmix_gpu.py uses for coalesced requests (another batch size is another GEMM tiling); alone they are the
    direct call bit for bit; a plain request keeps its own batch and its bits"""
    import threading
    from lib.pipeline import PromptFreePipeline
    from lib.serving import PromptFreeServer
    A, Bp = refs
    common = dict(steps=STEPS, as_uint8=False, height=64, width=64)
    tb = np.ascontiguousarray(_lr_map(40, 40).T)
    submits = [(([A, Bp],), dict(seed=5, regions=_lr_map(), region_weights=[[1.0, 0.0], [0.0, 1.0]], **common)),
               ((A,), dict(seed=6, **common)),
               (([Bp, A],), dict(seed=7, regions=tb, region_weights=[[1.0, 0.5], [0.0, 1.0]], **common))]
    srv = PromptFreeServer(net, use_graph=False, max_batch=4)
    try:
        gate = threading.Event()
        srv.call(lambda n: gate.wait(30))
        futs = [srv.submit(*submits[i][0], **submits[i][1]) for i in (0, 2, 1)]      # the two regional ones adjacent: one batch
        gate.set()
        r1, r2, p1 = [f.result(300) for f in futs]
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
    assert torch.equal(outs[0].float().cpu(), solo[0]) and torch.equal(outs[2].float().cpu(), solo[2])  # alone: the direct call
    for name, o, j in (("left / right, coalesced", r1, 0), ("top / bottom, coalesced", r2, 2)):
        r = rel_l2(o.float().cpu(), solo[j])
        print(f"[regions] served {name} vs its direct call: rel-L2 {r:.3e} (gate 1e-2), bits equal: {torch.equal(o.float().cpu(), solo[j])}")
        assert r <= 1e-2
    assert rel_l2(r1.float().cpu(), solo[2]) > 1e-2                                  # each kept its own map and table
