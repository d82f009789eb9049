"""GPU (-m gpu): masked regeneration -- pfd_cfg_step_masked, pfd_mask_grid_u8 and pfd_composite_u8 against lib/inpaint.py
(the specification in fp64), the masked step against the unmasked entry points bit for bit, the pipeline against the
sampler run by hand, graphed vs eager, and the server's batching of masked requests.

The inputs of the kernel tests, their tolerance and the cases are tests/inpaint_refs.py: tests/test_inpaint_cpu.py shows
on the same inputs that every named mutant of the specification leaves that tolerance."""
import functools
import threading

import numpy as np
import pytest
import torch

import img2img_refs as I
import inpaint_refs as R

pytestmark = pytest.mark.gpu

T = torch.from_numpy


def scaled(a, ref):
    """tests/test_hip_parity.py::err"""
    a, ref = a.detach().double().cpu(), torch.as_tensor(ref).double()
    return float((a - ref).abs().max() / max(1.0, float(ref.abs().max())))


def rel_l2(a, ref):
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    return float((a - ref).norm() / ref.norm())


# ---- the masked step ---------------------------------------------------------------------------------------------------
def _dev(c):
    """a case's arrays on the device, once per call"""
    d = {k: (T(np.ascontiguousarray(v)).cuda() if isinstance(v, np.ndarray) else v) for k, v in c.items()}
    return d


def _masked(c, d=None, **over):
    from lib.hip import ops
    d = dict(_dev(c) if d is None else d, **over)
    out = ops.cfg_step_masked(d['eps'], c['nb'], d['x'], d['coef'], solver=c['solver'], x0_prev=d['x0_prev'],
                              keep_key=d['keys'], step=c['index'], x0_keep=d['x0'], mask=d['mask'], ksq=float(d['ksq']),
                              ks=float(d['ks']), noise_mul=c['noise_mul'], scale=d['scale'], want_next=True, rep=c['rep'])
    torch.cuda.synchronize()
    return out


def _unmasked(c, d=None):
    """the corresponding unmasked entry point on the same inputs"""
    from lib.hip import ops
    d = _dev(c) if d is None else d
    ps = {} if d['scale'] is None else {'scale': d['scale']}
    if c['solver'] == 'ddim':
        noise = dict(noise_key=d['keys'], step=c['index'], noise_mul=c['noise_mul']) if float(c['coef'][2]) != 0. else {}
        return ops.cfg_ddim_step(d['eps'], c['nb'], d['x'], d['coef'], want_next=True, rep=c['rep'], **ps, **noise)
    return ops.cfg_dpmpp_step(d['eps'], c['nb'], d['x'], d['coef'], d['x0_prev'], want_next=True, rep=c['rep'], **ps)


CASES = R.cases()


@functools.lru_cache(maxsize=None)
def _reference(i):
    """the specification on case i: computed once, shared, never modified"""
    return R.reference(CASES[i])


def _judge(c, got, ref, what):
    xo, pr, xin = (t.cpu().numpy() for t in got)
    B, C, h, w = c['shape']
    assert xo.shape == pr.shape == c['shape'] and xin.shape == (c['rep'] * B, h, w, C)
    e = max(R.scaled_err(xo, ref[0]), R.scaled_err(pr, ref[1]))
    ex = R.xin_err(xin[:B], ref[0])
    print(f"[inpaint] {what} {R.name(c)}: x_out / pred_x0 err {e:.2e}, xin_next beyond its rounding {ex:.2e} (tol {R.TOL:g})")
    want_in = np.transpose(xo, (0, 2, 3, 1)).astype(np.float16)
    for r in range(c['rep']):                  # the next UNet input is half(x_out) at the NHWC positions, in every copy
        assert np.array_equal(xin[r * B:(r + 1) * B], want_in)
    assert e <= R.TOL and ex <= R.TOL
    return xo, pr


@pytest.mark.parametrize("i", range(len(CASES)), ids=[R.name(c).replace(' ', '_') for c in CASES])
def test_masked_step_matches_the_host_specification(i):
    """1e-5 scaled max-abs on x_out and pred_x0: the generator of tests/test_device_noise_gpu.py followed by an fp32 chain
    of the kind of the fused step's.  xin_next is half(x_out) of the device's x_out, bit for bit; against the specification
    it is judged beyond the half ulp its own f16 rounding may cost (inpaint_refs.xin_err): where the two x_out straddle an
    f16 rounding boundary their halves differ by a whole f16 ulp, 1e-3 relative, with both sides right."""
    c = CASES[i]
    xo, _ = _judge(c, _masked(c), _reference(i), "step")
    if c['mask_kind'] == 'zeros':
        assert not np.array_equal(xo, c['x0'])       # mid-run the kept region is noised


@pytest.mark.parametrize("form", R.FORMS)
def test_masked_step_grid_stride_loop(form):
    """2^20 + 1 quads: one more than the 4096 x 256 threads of the largest grid, for each of the five forms (B = 1 only:
    the host specification of four million elements is seconds of numpy; w = 2^20 + 1 takes the scalar instantiations)"""
    c = R.case(form, R.PAST_THE_GRID, 1, 'binary')
    got = _masked(c)
    xo, pr = _judge(c, got, R.reference(c), "step")
    assert not np.array_equal(xo[0, :, 0, -1], np.zeros(4, np.float32)) and pr[0, 3, 0, -1] != 0      # the last quad was written


@pytest.mark.parametrize("form", R.FORMS)
@pytest.mark.parametrize("shape", [R.SHAPES[0], R.SHAPES[3]], ids=["vec", "scalar"])
def test_mask_of_ones_is_the_unmasked_entry_point_bit_for_bit(form, shape):
    for last in (False, True):
        for Bm in (1, shape[0]):
            c = R.case(form, shape, Bm, 'ones', nb=2, rep=2, last=last)
            d = _dev(c)
            got, want = _masked(c, d), _unmasked(c, d)
            for g, w_, what in zip(got, want, ("x_out", "pred_x0", "xin_next")):
                assert torch.equal(g, w_), (form, shape, last, Bm, what)


@pytest.mark.parametrize("form", R.FORMS)
def test_last_step_keeps_x0_bit_for_bit_and_pred_x0_ignores_the_mask(form):
    for shape in (R.SHAPES[0], R.SHAPES[1]):
        for kind in ('binary', 'zeros', 'soft'):
            c = R.case(form, shape, 1, kind, last=True)
            assert (float(c['ksq']), float(c['ks'])) == (1.0, 0.0)
            d = _dev(c)
            xo, pr, _ = _masked(c, d)
            kept = (d['mask'] == 0)[:, None].expand_as(xo)
            assert bool(kept.any()) and torch.equal(xo[kept], d['x0'][kept]), (form, shape, kind)
            assert torch.equal(pr, _unmasked(c, d)[1]), (form, shape, kind)
        c = R.case(form, shape, 1, 'soft')              # ... and mid-run too
        d = _dev(c)
        assert torch.equal(_masked(c, d)[1], _unmasked(c, d)[1])


@pytest.mark.parametrize("form", ["ddim_seeded", "ddim_ps", "dpm2"])
def test_rows_are_independent(form):
    """permuting key rows, masks, x0 (and everything else of a sample) permutes the outputs bit for bit; a shared mask
    gives what B copies of it give"""
    shape = (3, 4, 8, 8)
    c = R.case(form, shape, 3, 'soft', nb=2, rep=2)
    d = _dev(c)
    base = _masked(c, d)
    perm = [2, 0, 1]
    B = shape[0]
    p = dict(d)
    for k in ('x', 'x0', 'keys', 'mask', 'x0_prev', 'scale'):
        if d[k] is not None:
            p[k] = d[k][perm].contiguous()
    p['eps'] = d['eps'].reshape(2, B, *d['eps'].shape[1:])[:, perm].reshape(d['eps'].shape).contiguous()
    got = _masked(c, p)
    assert torch.equal(got[0], base[0][perm]) and torch.equal(got[1], base[1][perm])
    xin = base[2].reshape(2, B, *base[2].shape[1:])[:, perm].reshape(base[2].shape)
    assert torch.equal(got[2], xin)
    one = R.case(form, shape, 1, 'soft', nb=2, rep=2)
    d1 = _dev(one)
    shared = _masked(one, d1)
    copies = _masked(one, d1, mask=d1['mask'].repeat(B, 1, 1).contiguous())
    assert all(torch.equal(a, b) for a, b in zip(shared, copies))
    # another key moves the kept region of that row only
    k2 = d1['keys'].clone()
    k2[1, 1] += 7
    moved = _masked(one, d1, keys=k2)
    assert torch.equal(moved[0][[0, 2]], shared[0][[0, 2]]) and not torch.equal(moved[0][1], shared[0][1])


def test_ops_refuse_bad_arguments():
    from lib.hip import ops
    c = R.case('ddim', R.SHAPES[0])
    d = _dev(c)
    for over in (dict(mask=d['mask'].double()), dict(mask=d['mask'][:, :4]), dict(x0=d['x0'][:1]), dict(keys=d['keys'][:1]),
                 dict(keys=d['keys'].int()), dict(mask=d['mask'].cpu()), dict(eps=d['eps'][:3]), dict(eps=d['eps'].float()),
                 dict(eps=d['eps'].cpu())):
        with pytest.raises(ValueError):
            _masked(c, d, **over)
    with pytest.raises(ValueError):
        ops.cfg_step_masked(d['eps'], 2, d['x'], d['coef'], solver='euler', keep_key=d['keys'], step=1, x0_keep=d['x0'],
                            mask=d['mask'], ksq=1.0, ks=0.0)
    with pytest.raises(ValueError):
        ops.cfg_step_masked(d['eps'], 2, d['x'], d['coef'], keep_key=d['keys'], step=1, x0_keep=d['x0'], mask=d['mask'])


# ---- the mask ingest and the composite ---------------------------------------------------------------------------------
def test_mask_grid_kernel_is_byte_exact():
    from lib import inpaint
    from lib.hip import ops
    masks = [(R.mask_u8(Hm, Wm, i)[None], g) for i, ((Hm, Wm), g) in enumerate(R.GRIDS)]
    masks.append((np.stack([R.mask_u8(100, 80, s) for s in range(3)]), (64, 64)))
    for m, (gh, gw) in masks:
        for dt, nd in ((torch.float32, np.float32), (torch.uint8, np.uint8)):
            got = ops.mask_grid_u8(T(m).cuda(), gh, gw, dt)
            want = inpaint.mask_grid_batch(m, gh, gw, nd)
            assert got.dtype == dt and np.array_equal(got.cpu().numpy(), want), (m.shape, gh, gw)
            assert 0 < want.sum() < want.size
    for m, want in R.worked_masks():
        assert np.array_equal(ops.mask_grid_u8(T(m).cuda(), 8, 8).cpu().numpy()[0], want)
    with pytest.raises(ValueError):
        ops.mask_grid_u8(T(masks[0][0]).cuda().float(), 8, 8)


def test_composite_kernel_is_byte_exact():
    from lib import inpaint
    from lib.hip import ops
    dec = np.stack([I.picture_u8(64, 64, s) for s in range(3)])
    for Bi, Bs in ((1, 1), (3, 1), (1, 3), (3, 3)):
        init = np.stack([I.picture_u8(64, 64, 7 + s) for s in range(Bi)])
        sel = np.stack([(R.mask_u8(64, 64, s) >= 128).astype(np.uint8) for s in range(Bs)])
        got = ops.composite_u8(T(dec).cuda(), T(init).cuda(), T(sel).cuda())
        assert np.array_equal(got.cpu().numpy(), inpaint.composite(dec, init, sel)), (Bi, Bs)
    with pytest.raises(ValueError):
        ops.composite_u8(T(dec).cuda(), T(init).cuda()[:, :32], T(sel).cuda())


# ---- sampler and pipeline ----------------------------------------------------------------------------------------------
STEPS, STRENGTH, K = 8, 0.75, 6


def _init_u8():
    return I.picture_u8(96, 72, seed=1)


def _mask_u8(which=0):
    """96 x 72 like the picture: the first worked mask (cells 2..5 x 2..5 of the 8 x 8 latent grid), or a band"""
    m = np.zeros((96, 72), dtype=np.uint8)
    if which == 0:
        m[24:72, 18:54] = 255
    else:
        m[40:96, 0:30] = 200
    return m


def _cells(mask_u8, n=2):
    """bool [n, 4, 8, 8]: the latent elements the mask regenerates (lib/inpaint.py)"""
    from lib import inpaint
    g = T(inpaint.mask_grid(mask_u8, 8, 8)) > 0
    return g[None, None].expand(n, 4, -1, -1).cuda()


@pytest.fixture(scope="module")
def eager_masked(net, golden):
    """computed once, never modified: generate(init=, mask=) eager, n = 2, seed 11 -> (latents, images)"""
    from lib.pipeline import PromptFreePipeline
    img, lat = PromptFreePipeline(net).generate(T(golden["see.img"]), 2, 64, 64, steps=STEPS, scale=2.0, seed=11,
                                                init=_init_u8(), strength=STRENGTH, mask=_mask_u8())
    return lat, img


def test_generate_keeps_the_clean_latent_outside_the_mask(net, golden, eager_masked):
    from lib.pipeline import PromptFreePipeline, shard_noise_keys
    lat, img = eager_masked
    pipe = PromptFreePipeline(net)
    x_t, k, x0 = pipe.init_latent(_init_u8(), 64, 64, STEPS, STRENGTH, shard_noise_keys(2, 11, 0, 1), want_x0=True)
    assert k == K and x0.shape == (2, 4, 8, 8) and img.shape == (2, 3, 64, 64) and bool(torch.isfinite(img).all())
    assert torch.equal(pipe.init_latent(_init_u8(), 64, 64, STEPS, STRENGTH, shard_noise_keys(2, 11, 0, 1))[0], x_t)
    regen = _cells(_mask_u8())
    assert int(regen[0, 0].sum()) == 16
    want = x0.to(lat.dtype)
    assert torch.equal(lat[~regen], want[~regen])                       # kept cells: the clean latent itself, bit for bit
    plain = pipe.generate(T(golden["see.img"]), 2, 64, 64, steps=STEPS, scale=2.0, seed=11, init=_init_u8(), strength=STRENGTH,
                          decode=False)[1]
    d_plain = (lat.float() - plain.float()).abs()[regen]
    d_x0 = (lat.float() - x0).abs()[regen]
    print(f"[inpaint] regenerated cells: mean |masked - img2img| {float(d_plain.mean()):.3e}, mean |masked - x0| {float(d_x0.mean()):.3e}")
    assert float(d_plain.max()) > 1e-2 and float(d_x0.max()) > 1e-2      # regenerated cells: neither the plain run nor x0
    assert float((plain.float() - x0).abs()[~regen].max()) > 1e-2        # ... and the plain run keeps nothing


def test_generate_takes_a_float_mask_per_sample(net, golden):
    """[n, h, w]: sample j keeps what ITS mask keeps, bit for bit"""
    from lib.pipeline import PromptFreePipeline, shard_noise_keys
    pipe = PromptFreePipeline(net)
    per = torch.stack([_cells(_mask_u8(0), 1)[0, 0], _cells(_mask_u8(1), 1)[0, 0]]).float().cpu()      # [2, 8, 8]
    lat = pipe.generate(T(golden["see.img"]), 2, 64, 64, steps=STEPS, scale=2.0, seed=11, init=_init_u8(), strength=STRENGTH,
                        mask=per, decode=False)[1]
    x0 = pipe.init_latent(_init_u8(), 64, 64, STEPS, STRENGTH, shard_noise_keys(2, 11, 0, 1), want_x0=True)[2].to(lat.dtype)
    keep = (per == 0)[:, None].expand(-1, 4, -1, -1).cuda()
    assert not torch.equal(keep[0], keep[1]) and torch.equal(lat[keep], x0[keep])
    assert float((lat.float() - x0.float()).abs()[~keep].max()) > 1e-2
    with pytest.raises(ValueError):
        pipe.generate(T(golden["see.img"]), 2, 64, 64, steps=STEPS, init=_init_u8(), mask=torch.zeros(3, 8, 8), decode=False)


def _by_hand(net, golden, solver, mask_u8, keys):
    """the sampler run by hand from host-specified inputs: the picture encoded on the device, (x0, x_t) from
    lib/img2img.py, the mask grid from lib/inpaint.py, K steps of STEPS"""
    from lib import img2img, inpaint
    from lib.hip import ops
    from lib.model_zoo.ddim import DDIMSampler
    from lib.pipeline import PromptFreePipeline
    pipe = PromptFreePipeline(net)
    pic = ops.image_from_u8(T(_init_u8()).cuda()[None], (64, 64), layout='nhwc')
    m = net.vae_encode_moments(pic, 'image')
    s = DDIMSampler(net)
    s.make_schedule(STEPS, ddim_eta=0., verbose=False)
    a_t = img2img.level(net.alphas_cumprod.float().cpu().numpy(), s.ddim_timesteps, K)
    x0, x_t = img2img.latent_start_batch(I.nchw(m.cpu().numpy()), np.asarray(keys), net.latent_scale_factor['image'], a_t)
    n = len(keys)
    cond, zeros = pipe.encode_reference(T(golden["see.img"]).cuda(), n)
    x_info = {'type': 'image', 'xt': T(x_t).cuda(), 'xt_steps': K, 'x0_keep': T(x0).cuda(),
              'mask': T(inpaint.mask_grid(mask_u8, 8, 8))[None].cuda(), 'keep_key': torch.tensor(keys, dtype=torch.int64)}
    c_info = {'type': 'image', 'conditioning': cond, 'unconditional_conditioning': zeros, 'unconditional_guidance_scale': 2.0}
    how = {} if solver == 'ddim' else {'solver': solver}
    return s.sample(steps=STEPS, shape=[n, 4, 8, 8], x_info=x_info, c_info=c_info, eta=0., verbose=False, **how)[0]


@pytest.mark.parametrize("solver", ["ddim", "dpmpp_2m"])
def test_generate_with_a_mask_matches_the_sampler_run_by_hand(net, golden, eager_masked, solver):
    """from host-specified inputs: the trajectory bound of tests/test_hip_parity.py (rel-L2 1e-2)"""
    from lib.pipeline import PromptFreePipeline
    if solver == 'ddim':
        got = eager_masked[0]
    else:
        got = PromptFreePipeline(net).generate(T(golden["see.img"]), 2, 64, 64, steps=STEPS, scale=2.0, seed=11, init=_init_u8(),
                                               strength=STRENGTH, mask=_mask_u8(), decode=False, solver=solver)[1]
    want = _by_hand(net, golden, solver, _mask_u8(), [(11, 0), (11, 1)])
    r = rel_l2(got, want)
    print(f"[inpaint] generate(init, mask, {solver}) vs by hand from host inputs: rel-L2 {r:.3e} (tol 1e-2)")
    assert r <= 1e-2
    if solver != 'ddim':
        assert float((got.float() - eager_masked[0].float()).abs().max()) > 1e-3     # another solver, another result


def test_composite_keeps_the_init_pictures_bytes(net, golden):
    from lib import inpaint
    from lib.hip import ops
    from lib.pipeline import PromptFreePipeline
    pipe = PromptFreePipeline(net)
    kw = dict(steps=STEPS, scale=2.0, seed=11, init=_init_u8(), strength=STRENGTH, mask=_mask_u8(), as_uint8=True)
    comp = pipe.generate(T(golden["see.img"]), 2, 64, 64, composite=True, **kw)[0]
    raw = pipe.generate(T(golden["see.img"]), 2, 64, 64, **kw)[0]
    assert comp.dtype == torch.uint8 and comp.shape == raw.shape == (2, 64, 64, 3)
    init64 = ops.image_from_u8(T(_init_u8()).cuda()[None], (64, 64), layout='u8')
    sel = T(inpaint.mask_grid(_mask_u8(), 64, 64, np.uint8)).bool().cuda()
    assert 0 < int(sel.sum()) < sel.numel()
    assert torch.equal(comp[:, ~sel], init64.expand(2, -1, -1, -1)[:, ~sel]) and torch.equal(comp[:, sel], raw[:, sel])
    assert not torch.equal(comp, raw)


# ---- the graph ---------------------------------------------------------------------------------------------------------
def test_graphed_equals_eager(net, golden, eager_masked):
    """bit for bit; one captured loop serves another mask and another seed; the plain img2img and the plain request still
    capture graphs of their own"""
    from lib.pipeline import PromptFreePipeline
    pipe = PromptFreePipeline(net)
    pipe.enable_graph(True)
    img = T(golden["see.img"])
    kw = dict(steps=STEPS, scale=2.0, strength=STRENGTH, decode=False, init=_init_u8())
    a = pipe.generate(img, 2, 64, 64, seed=11, mask=_mask_u8(), **kw)[1]
    assert torch.equal(a, eager_masked[0]) and len(pipe.sampler._graphs) == 1
    eager = PromptFreePipeline(net)
    b = pipe.generate(img, 2, 64, 64, seed=12, mask=_mask_u8(1), **kw)[1]
    assert torch.equal(b, eager.generate(img, 2, 64, 64, seed=12, mask=_mask_u8(1), **kw)[1])
    assert len(pipe.sampler._graphs) == 1 and not torch.equal(a, b)
    assert torch.equal(pipe.generate(img, 2, 64, 64, seed=11, mask=_mask_u8(), **kw)[1], a)
    # a float mask at latent resolution is the same request
    from lib import inpaint
    soft = T(inpaint.mask_grid(_mask_u8(), 8, 8))
    assert torch.equal(pipe.generate(img, 2, 64, 64, seed=11, mask=soft, **kw)[1], a) and len(pipe.sampler._graphs) == 1
    # the plain img2img request and the plain request: graphs of their own, results of the eager path
    p = pipe.generate(img, 2, 64, 64, seed=11, **kw)[1]
    assert len(pipe.sampler._graphs) == 2 and torch.equal(p, eager.generate(img, 2, 64, 64, seed=11, **kw)[1])
    q = pipe.generate(img, 2, 64, 64, steps=STEPS, scale=2.0, seed=11, decode=False)[1]
    assert len(pipe.sampler._graphs) == 3 and torch.equal(q, eager.generate(img, 2, 64, 64, steps=STEPS, scale=2.0, seed=11,
                                                                              decode=False)[1])
    assert not torch.equal(p, a)


# ---- the server --------------------------------------------------------------------------------------------------------
def _held(srv, submits):
    """submit everything while the worker is held (tests/test_dpm_solver_gpu.py::_held)"""
    gate = threading.Event()
    srv.call(lambda n: gate.wait(30))
    futs = [srv.submit(*a, **k) for a, k in submits]
    gate.set()
    return [f.result(300) for f in futs]


def test_server_batches_masked_requests_among_themselves(net, golden):
    """two masked requests of equal k share a batch, each with its own picture, mask and keys; a masked and an unmasked
    request do not; every caller gets what its solo run gives (5e-3 scaled, the bound of the img2img server test)"""
    from lib.pipeline import PromptFreePipeline
    from lib.serving import PromptFreeServer
    img1, img2 = T(golden["see.img"]), T(golden["see2.img"])
    pics = (_init_u8(), I.picture_u8(64, 64, seed=5))
    # 4 steps, as the served requests of the other GPU files: k = 3
    submits = [((im, 1, 64, 64), dict(steps=4, seed=sd, as_uint8=False, init=pic, strength=0.75, **m))
               for im, sd, pic, m in ((img1, 5, pics[0], dict(mask=_mask_u8(0))), (img2, 6, pics[1], dict(mask=_mask_u8(1))),
                                      (img1, 7, pics[0], {}))]
    srv = PromptFreeServer(net, use_graph=False, max_batch=4)
    try:
        outs = _held(srv, submits[:2])
        assert srv.batches == [2]
        outs += _held(srv, submits[:1] + submits[2:])
        assert srv.batches == [2, 1, 1]
    finally:
        srv.close()
    pipe = PromptFreePipeline(net)
    solo = []
    for a, k in submits:
        kw = dict(k)
        kw.pop('as_uint8')
        solo.append(pipe.generate(a[0], a[1], a[2], a[3], scale=2.0, **kw)[0].float().cpu())
    for i, (o, j) in enumerate(zip(outs, (0, 1, 0, 2))):
        e = scaled(o, solo[j])
        print(f"[inpaint] served request {i} vs its solo run: scaled max-abs err {e:.3e} (tol 5e-3)")
        assert e <= 5e-3
    assert float((solo[0] - solo[2]).abs().max()) > 1e-3          # the mask matters
