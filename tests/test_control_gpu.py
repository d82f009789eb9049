"""GPU (-m gpu): ControlNet strength above the kernel -- the miniature UNet walk with a strength table against the fp64 walk with
scaled residuals, then generate(control=, control_scale=, control_layer_scales=, control_window=, control_cond_only=) on the
small net at 64 x 64 pixels, 2 samples, 4 steps: the default spellings and a ones table are the plain control request bit for
bit, nothing left of the control is the request without it, a scaled request equals the stages run by hand and each sample its
own single-strength run, a window runs the ControlNet on its steps only (counted on the full schedule, also under img2img),
cond_only, graphed against eager with a second strength replaying the same graph, the server, and one combination with
DPM-Solver++, several references and a mask."""
import threading

import numpy as np
import pytest
import torch

import block_refs as BR
import control_refs as R
import ops_standin as SI
from lib import control

pytestmark = pytest.mark.gpu

T = torch.from_numpy
STEPS = 4
KW = dict(steps=STEPS, scale=2.0, seed=11, decode=False)


def scaled_err(a, ref):
    """the measure of tests/test_mixed_batches_gpu.py::check"""
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    return float((a - ref).abs().max() / max(1.0, float(ref.abs().max())))


# ---- the block -------------------------------------------------------------------------------------------------------------
def test_miniature_unet_walk_with_a_strength_table():
    """UNetModel2D_Next.hip(control=, control_scale=) with a table whose rows and columns all differ, within T = 4 f of the fp64
    walk of block_refs.unet over the scaled residuals (f: the floor of the registered `unet-control` case, the rule of
    tests/test_regions_gpu.py); the table moves the formula by more than 4 T; a table of ones gives the bits of the plain walk"""
    b = BR.build_unet(mode="control")
    tab = R.unet_table(b.B)
    assert len(set(tab.reshape(-1).tolist())) == tab.size

    def run(table):
        mods, inputs = BR._dev(b, "cuda")
        ctrl = [inputs[f"c{n}"].clone() for n in range(5)]
        how = {} if table is None else {'control_scale': T(table).cuda()}
        return mods["net"].hip(inputs["x"], inputs["t"], BR._context(inputs, 0), control=ctrl, **how)
    y = run(tab)
    ref, plain = R.unet_ref_scaled(b, tab), b.ref()
    Tol = 4 * SI.floor(BR.CASE["unet-control"])
    e, moved = BR.err_units(y, ref, b.B), BR.err_units(ref, plain, b.B)
    print(f"[control] miniature UNet: T {Tol:.3f} err {e:.3f} err / T {e / Tol:.3f}; the table moves the formula by {moved:.1f} units")
    assert e <= Tol and moved > 4 * Tol
    assert torch.equal(run(np.ones((b.B, 5), dtype=np.float32)), run(None))
    with pytest.raises(ValueError, match="control_scale"):
        run(np.ones((b.B, 4), dtype=np.float32))


# ---- generate --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def img(golden):
    return T(golden["see.img"])


@pytest.fixture(scope="module")
def ctl():
    c = torch.zeros(1, 3, 64, 64)                  # a white square on black
    c[..., 16:48, 16:48] = 1.0
    return c


@pytest.fixture(scope="module")
def pipe(net):
    from lib.pipeline import PromptFreePipeline
    return PromptFreePipeline(net)


@pytest.fixture(scope="module")
def plain(pipe, img, ctl):
    """the plain control request"""
    return pipe.generate(img, 2, 64, 64, control=ctl, **KW)[1]


@pytest.fixture(scope="module")
def uncontrolled(pipe, img):
    return pipe.generate(img, 2, 64, 64, **KW)[1]


@pytest.fixture(scope="module")
def soft_mixed(pipe, img, ctl):
    return pipe.generate(img, 2, 64, 64, control=ctl, control_scale=[1.0, 0.4], control_layer_scales='soft', **KW)[1]


def _by_hand(net, pipe, img, ctl, table=None, steps=None, xT=None, **x_extra):
    """the stages run by hand: SeeCoder, the hint, the sampler called directly"""
    from lib.model_zoo.ddim import DDIMSampler
    from lib.pipeline import shard_xT
    cond = net.ctx_encode(img.cuda(), 'image').repeat(2, 1, 1)
    xT = shard_xT(2, 64, 64, 11, 0, 1) if xT is None else xT
    c_info = {'type': 'image', 'conditioning': cond, 'unconditional_conditioning': torch.zeros_like(cond),
              'unconditional_guidance_scale': 2.0, 'control': pipe.control_hint(ctl, 64, 64)}
    if table is not None:
        c_info['control_scale'] = T(table).cuda()
    if steps is not None:
        c_info['control_steps'] = steps
    return DDIMSampler(net).sample(steps=STEPS, shape=list(xT.shape), x_info=dict({'type': 'image', 'xt': xT.cuda()}, **x_extra),
                                   c_info=c_info, eta=0., verbose=False)[0]


def test_a_ones_table_over_every_step_is_the_plain_control_request(net, pipe, img, ctl, plain, uncontrolled):
    got = _by_hand(net, pipe, img, ctl, control.scale_table(1.0, None, 2, 2), (0, STEPS))
    assert bool(torch.isfinite(plain).all()) and torch.equal(got, plain)
    assert torch.equal(_by_hand(net, pipe, img, ctl), plain)
    d = scaled_err(plain, uncontrolled)
    print(f"[control] the plain control request vs the uncontrolled one: {d:.3e}")
    assert d > 10 * R.COMPANY


def test_every_default_spelling_is_the_plain_request_and_makes_no_graph_key(net, img, ctl, plain):
    from lib.pipeline import PromptFreePipeline
    g = PromptFreePipeline(net)
    g.enable_graph(True)
    assert torch.equal(g.generate(img, 2, 64, 64, control=ctl, **KW)[1], plain)
    keys = list(g.sampler._graphs)
    for kw in (dict(control_scale=1.0), dict(control_scale=[1.0, 1.0], control_layer_scales=[1.0] * 13, control_window=[0, 1])):
        assert torch.equal(g.generate(img, 2, 64, 64, control=ctl, **KW, **kw)[1], plain)
        assert list(g.sampler._graphs) == keys and len(keys) == 1


@pytest.mark.parametrize("kw", [dict(control_scale=0), dict(control_window=(0, 0)), dict(control_window=(0.5, 0.5))],
                         ids=["scale-0", "window-0-0", "window-half-half"])
def test_nothing_left_of_the_control_is_the_uncontrolled_request(net, pipe, img, ctl, uncontrolled, kw, monkeypatch):
    def never(*a, **k):
        raise AssertionError("the ControlNet ran")
    monkeypatch.setattr(net.ctl, "prepare_hint", never)
    assert torch.equal(pipe.generate(img, 2, 64, 64, control=ctl, **KW, **kw)[1], uncontrolled)


def test_scaled_request_equals_the_stages_by_hand(net, pipe, img, ctl, soft_mixed, plain):
    want = _by_hand(net, pipe, img, ctl, control.scale_table([1.0, 0.4], 'soft', 2, 2), (0, STEPS))
    assert bool(torch.isfinite(soft_mixed).all())
    assert torch.equal(soft_mixed, want) and not torch.equal(soft_mixed, plain)


def test_each_sample_lands_on_its_single_strength_run(pipe, img, ctl, soft_mixed):
    """sample 0 of the [1.0, 0.4] request against the request at 1.0 for both samples, sample 1 against the one at 0.4 for both:
    within the company-invariance bound (the batch is the same, only the other sample's strength differs); and the strength
    matters: sample 1 differs between the two single-strength runs by more than 10 times the bound"""
    one = pipe.generate(img, 2, 64, 64, control=ctl, control_scale=1.0, control_layer_scales='soft', **KW)[1]
    low = pipe.generate(img, 2, 64, 64, control=ctl, control_scale=0.4, control_layer_scales='soft', **KW)[1]
    e0, e1 = scaled_err(soft_mixed[0], one[0]), scaled_err(soft_mixed[1], low[1])
    apart = scaled_err(low[1], one[1])
    print(f"[control] sample 0 vs its run at 1.0: {e0:.3e}, sample 1 vs its run at 0.4: {e1:.3e} (bound {R.COMPANY:g}); "
          f"sample 1 at 0.4 vs at 1.0: {apart:.3e}")
    assert e0 <= R.COMPANY and e1 <= R.COMPANY
    assert apart > 10 * R.COMPANY


def _count_controlnet(net, monkeypatch):
    calls = []
    hip = net.ctl.hip

    def counted(*a, **k):
        calls.append(1)
        return hip(*a, **k)
    monkeypatch.setattr(net.ctl, "hip", counted)
    return calls


def _hand_loop(net, pipe, img, ctl, on_steps, x=None, k=STEPS):
    """the sampler's loop written out (DDIM, eta 0, CFG with the zero unconditional context): the control on `on_steps` only"""
    from lib.hip import ops
    from lib.model_zoo.controlnet import PreparedHint
    from lib.model_zoo.ddim import DDIMSampler
    from lib.pipeline import shard_xT
    s = DDIMSampler(net)
    s.make_schedule(STEPS, verbose=False)
    cond = net.ctx_encode(img.cuda(), 'image').repeat(2, 1, 1)
    ctx = net.prepare_context(torch.cat([torch.zeros_like(cond), cond]))
    ctx.zero_lead = 2
    hint = PreparedHint(net.ctl.prepare_hint(pipe.control_hint(ctl, 64, 64)).feat)
    x = (shard_xT(2, 64, 64, 11, 0, 1) if x is None else x).cuda().float().contiguous()
    ts = np.flip(s.ddim_timesteps[:k])
    t_table = torch.as_tensor(np.array(ts).copy(), device='cuda').long()[:, None].repeat(1, 4)
    emb_all, _ = net.diffuser['image'].emb_projections(t_table[:, 0].contiguous())
    coef = s._coef_table(2.0)
    xin = ops.to_nhwc(x, rep=1)
    for i in range(k):
        eps = net.apply_model_nhwc('image', xin, t_table[i], 'image', ctx, control=hint if i in on_steps else None,
                                   emb_table=emb_all[i:i + 1], cfg_pair=True)
        x, _, xin = ops.cfg_ddim_step(eps, 2, x, coef[k - i - 1], want_next=True, rep=1)
    return x.to(cond.dtype)


def test_window_runs_the_controlnet_on_its_steps_only(net, pipe, img, ctl, plain, uncontrolled, monkeypatch):
    want = _hand_loop(net, pipe, img, ctl, (0, 1))
    assert torch.equal(_hand_loop(net, pipe, img, ctl, (0, 1, 2, 3)), plain)          # the loop written out is the sampler's
    calls = _count_controlnet(net, monkeypatch)
    got = pipe.generate(img, 2, 64, 64, control=ctl, control_window=(0, 0.5), **KW)[1]
    assert len(calls) == 2
    assert torch.equal(got, want)
    d_full, d_none = scaled_err(got, plain), scaled_err(got, uncontrolled)
    print(f"[control] window (0, 0.5) vs full control: {d_full:.3e}, vs uncontrolled: {d_none:.3e} (10 x bound {10 * R.COMPANY:g})")
    assert d_full > 10 * R.COMPANY and d_none > 10 * R.COMPANY


def test_window_under_img2img_counts_on_the_full_schedule(net, pipe, img, ctl, monkeypatch):
    """strength 0.5 of 4 steps runs positions 2 and 3: a window (0, 0.75) controls position 2 alone -- run step 0 --, a window
    (0, 0.5) ended before the run began and leaves the img2img request without control"""
    import img2img_refs as I
    init = I.picture_u8(64, 64, seed=3)
    kw = dict(KW, init=init, strength=0.5)
    calls = _count_controlnet(net, monkeypatch)
    got = pipe.generate(img, 2, 64, 64, control=ctl, control_window=(0, 0.75), **kw)[1]
    assert len(calls) == 1
    full = pipe.generate(img, 2, 64, 64, control=ctl, **kw)[1]
    assert len(calls) == 3
    none = pipe.generate(img, 2, 64, 64, **kw)[1]
    assert torch.equal(pipe.generate(img, 2, 64, 64, control=ctl, control_window=(0, 0.5), **kw)[1], none) and len(calls) == 3
    assert not torch.equal(got, full) and not torch.equal(got, none)
    # the run step that is controlled is step 0: the loop written out from the request's own start
    from lib.pipeline import shard_noise_keys
    x_t, k = pipe.init_latent(init, 64, 64, STEPS, 0.5, shard_noise_keys(2, 11, 0, 1))
    assert k == 2 and torch.equal(_hand_loop(net, pipe, img, ctl, (0,), x=x_t, k=2), got)


def test_cond_only_zeroes_the_unconditional_rows(net, pipe, img, ctl, plain):
    got = pipe.generate(img, 2, 64, 64, control=ctl, control_cond_only=True, **KW)[1]
    tab = control.scale_table(1.0, None, 2, 2, cond_only=True)
    assert np.all(tab[:2] == 0) and np.all(tab[2:] == 1)
    assert torch.equal(got, _by_hand(net, pipe, img, ctl, tab, (0, STEPS)))
    assert bool(torch.isfinite(got).all()) and not torch.equal(got, plain)


def test_graphed_equals_eager_and_a_second_strength_replays_the_same_graph(net, pipe, img, ctl, soft_mixed):
    from lib.pipeline import PromptFreePipeline
    g = PromptFreePipeline(net)
    g.enable_graph(True)
    kw = dict(KW, control=ctl, control_layer_scales='soft')
    assert torch.equal(g.generate(img, 2, 64, 64, control_scale=[1.0, 0.4], **kw)[1], soft_mixed)
    assert len(g.sampler._graphs) == 1 and next(iter(g.sampler._graphs))[-1] == ('control', 0, STEPS)
    other = g.generate(img, 2, 64, 64, control_scale=[0.3, 0.9], **kw)[1]
    assert len(g.sampler._graphs) == 1 and not torch.equal(other, soft_mixed)
    assert torch.equal(other, pipe.generate(img, 2, 64, 64, control_scale=[0.3, 0.9], **kw)[1])
    win = g.generate(img, 2, 64, 64, control_scale=[0.3, 0.9], control_window=(0, 0.5), **kw)[1]      # another window: another graph
    assert len(g.sampler._graphs) == 2 and list(g.sampler._graphs)[-1][-1] == ('control', 0, 2)
    assert torch.equal(win, pipe.generate(img, 2, 64, 64, control_scale=[0.3, 0.9], control_window=(0, 0.5), **kw)[1])


def test_server_coalesces_requests_that_differ_in_strength(net, golden, img, ctl):
    """two control requests with strengths 1.0 and 0.5 and the same window share one batch, each within the company bound of its
    direct call; a control request without the arguments is not merged with them"""
    from lib.pipeline import PromptFreePipeline
    from lib.serving import PromptFreeServer
    img2 = T(golden["see2.img"])
    common = dict(steps=STEPS, as_uint8=False, control=ctl)
    submits = [((img, 1, 64, 64), dict(common, seed=5, control_scale=1.0, control_window=(0, 0.5))),
               ((img2, 1, 64, 64), dict(common, seed=6, control_scale=0.5, control_window=(0, 0.5))),
               ((img, 1, 64, 64), dict(common, seed=7))]
    srv = PromptFreeServer(net, use_graph=False, max_batch=4, mixed_batches=True)
    try:
        gate = threading.Event()
        srv.call(lambda n: gate.wait(30))
        futs = [srv.submit(*a, **k) for a, k in submits]
        gate.set()
        outs = [f.result(300) for f in futs]
        assert srv.batches == [2, 1]
    finally:
        srv.close()
    pipe = PromptFreePipeline(net)
    direct = []
    for i, ((a, k), o) in enumerate(zip(submits, outs)):
        kw = {x: v for x, v in k.items() if x != 'as_uint8'}
        direct.append(pipe.generate(a[0], 1, 64, 64, scale=2.0, **kw)[0].float().cpu())
        e = scaled_err(o.float().cpu(), direct[-1])
        print(f"[control] served request {i} vs its direct call: {e:.3e} (bound {R.COMPANY:g})")
        assert e <= R.COMPANY
    strong = pipe.generate(img2, 1, 64, 64, scale=2.0, **dict({x: v for x, v in submits[1][1].items() if x != 'as_uint8'},
                                                                 control_scale=1.0))[0].float().cpu()
    assert scaled_err(outs[1].float().cpu(), strong) > scaled_err(outs[1].float().cpu(), direct[1])     # request 1 kept ITS strength


def test_combination_with_solver_references_and_mask(net, golden, img, ctl):
    from lib.pipeline import PromptFreePipeline
    import img2img_refs as I
    m = np.zeros((64, 64), dtype=np.uint8)
    m[16:48, 8:40] = 255
    kw = dict(KW, solver='dpmpp_2m', image_weights=[0.7, 0.3], init=I.picture_u8(64, 64, seed=3), strength=0.75, mask=m,
              control=ctl, control_scale=[0.8, 0.5], control_layer_scales='soft', control_window=(0, 0.75), control_cond_only=True)
    refs = [img, T(golden["see2.img"])]
    eager = PromptFreePipeline(net).generate(refs, 2, 64, 64, **kw)[1]
    g = PromptFreePipeline(net)
    g.enable_graph(True)
    assert bool(torch.isfinite(eager).all())
    assert torch.equal(g.generate(refs, 2, 64, 64, **kw)[1], eager)
    assert next(iter(g.sampler._graphs))[-1] == ('control', 0, 2)          # 3 of 4 steps run: positions 1 .. 3, controlled below 3
    assert not torch.equal(PromptFreePipeline(net).generate(refs, 2, 64, 64, **dict(kw, control_window=(0.0, 1.0)))[1], eager)
