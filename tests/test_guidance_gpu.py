"""GPU (-m gpu): guidance rescale above the kernels -- generate(guidance_rescale=) on the small net at 64 x 64 pixels, 2 samples,
4 steps: 0, [0, 0] and absent are the plain request bit for bit, a rescaled request equals the stages run by hand (statistics
launch plus step, per step), each sample is bit for bit its sample of the run in which both samples carry its phi and within
the company bound of its run alone, graphed against eager with a second phi replaying the same graph, the size of the effect
at scale 7.5 and phi 0.7, one combination with DPM-Solver++, a mask and two references, and the server."""
import threading

import numpy as np
import pytest
import torch

from control_refs import COMPANY

pytestmark = pytest.mark.gpu

T = torch.from_numpy
STEPS = 4
KW = dict(steps=STEPS, scale=7.5, seed=11, decode=False)
PHI = [0.7, 0.25]


def scaled_err(a, ref):
    """the measure of tests/test_mixed_batches_gpu.py::check"""
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    return float((a - ref).abs().max() / max(1.0, float(ref.abs().max())))


@pytest.fixture(scope="module")
def img(golden):
    return T(golden["see.img"])


@pytest.fixture(scope="module")
def pipe(net):
    from lib.pipeline import PromptFreePipeline
    return PromptFreePipeline(net)


@pytest.fixture(scope="module")
def plain(pipe, img):
    return pipe.generate(img, 2, 64, 64, **KW)[1]


@pytest.fixture(scope="module")
def mixed(pipe, img):
    return pipe.generate(img, 2, 64, 64, guidance_rescale=PHI, **KW)[1]


def test_every_default_spelling_is_the_plain_request_and_makes_no_graph_key(net, img, plain):
    from lib.pipeline import PromptFreePipeline
    g = PromptFreePipeline(net)
    g.enable_graph(True)
    assert bool(torch.isfinite(plain).all()) and torch.equal(g.generate(img, 2, 64, 64, **KW)[1], plain)
    keys = list(g.sampler._graphs)
    for kw in (dict(guidance_rescale=0), dict(guidance_rescale=0.0), dict(guidance_rescale=[0, 0]), dict(guidance_rescale=torch.zeros(2))):
        assert torch.equal(g.generate(img, 2, 64, 64, **KW, **kw)[1], plain)
        assert list(g.sampler._graphs) == keys and len(keys) == 1
    assert not any(e == ('rescale',) for e in keys[0])


def _hand_loop(net, img, phi, scale=7.5, xT=None):
    """the sampler's loop written out (DDIM, eta 0, CFG with the zero unconditional context): per step the UNet, the statistics
    launch and the step with its factors"""
    from lib.hip import ops
    from lib.model_zoo.ddim import DDIMSampler
    from lib.pipeline import shard_xT
    s = DDIMSampler(net)
    s.make_schedule(STEPS, verbose=False)
    x = (shard_xT(2, 64, 64, 11, 0, 1) if xT is None else xT).cuda().float().contiguous()
    n = x.shape[0]
    cond = net.ctx_encode(img.cuda(), 'image').repeat(n, 1, 1)
    ctx = net.prepare_context(torch.cat([torch.zeros_like(cond), cond]))
    ctx.zero_lead = n
    t_table = torch.as_tensor(np.array(np.flip(s.ddim_timesteps)).copy(), device='cuda').long()[:, None].repeat(1, 2 * n)
    emb_all, _ = net.diffuser['image'].emb_projections(t_table[:, 0].contiguous())
    coef = s._coef_table(scale)
    phi = torch.tensor(phi, dtype=torch.float32, device='cuda')
    xin = ops.to_nhwc(x, rep=1)
    muls = []
    for i in range(STEPS):
        row = coef[STEPS - i - 1]
        eps = net.apply_model_nhwc('image', xin, t_table[i], 'image', ctx, emb_table=emb_all[i:i + 1], cfg_pair=True)
        mul = ops.guidance_rescale(eps, row[4:5], phi)
        muls.append(mul)
        x, _, xin = ops.cfg_ddim_step(eps, 2, x, row, want_next=True, rep=1, eps_mul=mul)
    return x.to(cond.dtype), torch.stack(muls).cpu()


def test_rescaled_request_equals_the_stages_by_hand(net, img, mixed, plain):
    want, muls = _hand_loop(net, img, PHI)
    print(f"[guidance] factors per step (rows) and sample (columns), scale 7.5, phi {PHI}:\n{muls.numpy()}")
    assert bool(torch.isfinite(mixed).all()) and torch.equal(mixed, want) and not torch.equal(mixed, plain)
    assert bool(torch.isfinite(muls).all()) and bool((muls > 0).all()) and not bool((muls == 1).any())


def test_each_sample_is_its_own_run(net, pipe, img, mixed):
    """sample b of the [0.7, 0.25] request is bit for bit sample b of the request in which both samples carry phi[b] (the other
    sample's phi touches nothing of it: statistics and step are per sample); run ALONE, in a batch of one, it is the same
    trajectory up to the UNet's tile choice at another batch size -- the bound of
    test_device_noise_gpu.py::test_a_sample_does_not_depend_on_its_company, as for the plain request; and phi matters"""
    from lib.pipeline import shard_xT
    hi = pipe.generate(img, 2, 64, 64, guidance_rescale=0.7, **KW)[1]
    lo = pipe.generate(img, 2, 64, 64, guidance_rescale=0.25, **KW)[1]
    assert torch.equal(mixed[0], hi[0]) and torch.equal(mixed[1], lo[1])
    xT = shard_xT(2, 64, 64, 11, 0, 1)
    for b in range(2):
        alone, _ = _hand_loop(net, img, PHI[b:b + 1], xT=xT[b:b + 1])
        e = scaled_err(alone[0], mixed[b])
        print(f"[guidance] sample {b} alone vs in the batch of two: {e:.3e} (bound 4e-3)")
        assert e <= 4e-3
    apart = scaled_err(lo[1], hi[1])
    print(f"[guidance] sample 1 at phi 0.25 vs at 0.7: {apart:.3e}")
    assert apart > 10 * COMPANY


def test_graphed_equals_eager_and_a_second_phi_replays_the_same_graph(net, pipe, img, mixed):
    from lib.pipeline import PromptFreePipeline
    g = PromptFreePipeline(net)
    g.enable_graph(True)
    assert torch.equal(g.generate(img, 2, 64, 64, guidance_rescale=PHI, **KW)[1], mixed)
    assert len(g.sampler._graphs) == 1 and next(iter(g.sampler._graphs))[-1] == ('rescale',)
    other = g.generate(img, 2, 64, 64, guidance_rescale=[0.1, 0.9], **KW)[1]
    assert len(g.sampler._graphs) == 1 and not torch.equal(other, mixed)
    assert torch.equal(other, pipe.generate(img, 2, 64, 64, guidance_rescale=[0.1, 0.9], **KW)[1])
    g.generate(img, 2, 64, 64, **KW)                                    # the plain request: its own graph, as before
    assert len(g.sampler._graphs) == 2 and list(g.sampler._graphs)[-1][-1] != ('rescale',)


def test_the_latent_moves_by_more_than_a_thousand_tolerances(pipe, img, plain):
    """scale 7.5, phi 0.7 against the plain request; the comparison tolerance of this file is exact equality for the stages by
    hand and 1e-5 (scaled max-abs, the step's tolerance against fp64) for everything computed another way"""
    got = pipe.generate(img, 2, 64, 64, guidance_rescale=0.7, **KW)[1]
    d = scaled_err(got, plain)
    print(f"[guidance] scale 7.5: phi 0.7 against plain, scaled max-abs {d:.3e}; std of the latent {float(plain.float().std()):.3f} -> "
          f"{float(got.float().std()):.3f}")
    assert d > 1e3 * 1e-5


def test_combination_with_solver_mask_and_two_references(net, golden, img):
    from lib.pipeline import PromptFreePipeline
    import img2img_refs as I
    m = np.zeros((64, 64), dtype=np.uint8)
    m[16:48, 8:40] = 255
    kw = dict(KW, scale=[7.5, 3.0], solver='dpmpp_2m', image_weights=[0.7, 0.3], init=I.picture_u8(64, 64, seed=3), strength=0.75,
              mask=m, guidance_rescale=PHI)
    refs = [img, T(golden["see2.img"])]
    eager = PromptFreePipeline(net).generate(refs, 2, 64, 64, **kw)[1]
    g = PromptFreePipeline(net)
    g.enable_graph(True)
    assert bool(torch.isfinite(eager).all())
    assert torch.equal(g.generate(refs, 2, 64, 64, **kw)[1], eager)
    assert next(iter(g.sampler._graphs))[-1] == ('rescale',)
    assert not torch.equal(PromptFreePipeline(net).generate(refs, 2, 64, 64, **dict(kw, guidance_rescale=0.0))[1], eager)


def test_server_gives_each_request_its_phi_in_one_batch(net, golden, img):
    """two requests with different phi (and, the server mixing batches, different scales) share one batch, each within the
    company bound of its direct call; a request without rescale is not merged with them"""
    from lib.pipeline import PromptFreePipeline
    from lib.serving import PromptFreeServer
    img2 = T(golden["see2.img"])
    common = dict(steps=STEPS, as_uint8=False)
    submits = [((img, 1, 64, 64), dict(common, seed=5, scale=7.5, guidance_rescale=0.7)),
               ((img2, 1, 64, 64), dict(common, seed=6, scale=5.0, guidance_rescale=0.2)),
               ((img, 1, 64, 64), dict(common, seed=7, scale=7.5))]
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
        direct.append(pipe.generate(a[0], 1, 64, 64, **kw)[0].float().cpu())
        e = scaled_err(o.float().cpu(), direct[-1])
        print(f"[guidance] served request {i} vs its direct call: {e:.3e} (bound {COMPANY:g})")
        assert e <= COMPANY
    other = pipe.generate(img2, 1, 64, 64, **dict({x: v for x, v in submits[1][1].items() if x != 'as_uint8'},
                                                  guidance_rescale=0.7))[0].float().cpu()
    assert scaled_err(outs[1].float().cpu(), other) > scaled_err(outs[1].float().cpu(), direct[1])     # request 1 kept ITS phi
