"""GPU (-m gpu): img2img from an init picture -- pfd_latent_start against lib/img2img.py (the specification in fp64), the VAE
encoder's NHWC moments against `encode`, the reference fixture and the 256x256 oracle fixture, the pipeline against the
sampler run by hand from the host-specified start, graphed vs eager, and the server's batching by step count.

The inputs of the kernel tests, their tolerance and the cases are tests/img2img_refs.py: tests/test_img2img_cpu.py shows
on the same inputs that every named mutant of the specification leaves that tolerance."""
import os
import threading

import numpy as np
import pytest
import torch

import img2img_refs as R

pytestmark = pytest.mark.gpu

T = torch.from_numpy
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL_STAGE = 1e-2                     # tests/test_hip_parity.py::TOL


def scaled(a, ref):
    """tests/test_hip_parity.py::err"""
    a, ref = a.detach().double().cpu(), torch.as_tensor(ref).double()
    return float((a - ref).abs().max() / max(1.0, float(ref.abs().max())))


def rel_l2(a, ref):
    a, ref = a.detach().double().cpu(), ref.detach().double().cpu()
    return float((a - ref).norm() / ref.norm())


# ---- the kernel ------------------------------------------------------------------------------------------------------
def _run_kernel(m, k, post, want_x0=True):
    from lib.hip import ops
    out = ops.latent_start(T(m).cuda(), T(k).cuda(), R.SCALE_FACTOR, R.A_T, posterior=post, want_x0=want_x0)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("post", ["sample", "mode"])
@pytest.mark.parametrize("shape,Bm", [(s, Bm) for s in R.SHAPES for Bm in sorted({1, s[0]})])
def test_kernel_matches_the_host_specification(shape, Bm, post):
    """1e-5 scaled max-abs, the bound of tests/test_device_noise_gpu.py: the generator is the same and the chain behind it
    -- one expf, three products, two sums in fp32 -- is of the kind of the fused step's.  'mode' x0 is one fp32 rounding of
    an exact product on both sides: bit for bit."""
    m, k = R.moments(shape, Bm), R.keys(shape[0])
    x0, xt = _run_kernel(m, k, post)
    r0, rt = R.reference(m, k, post)
    assert x0.shape == xt.shape == shape and x0.dtype == xt.dtype == torch.float32
    e0, et = R.scaled_err(x0.cpu().numpy(), r0), R.scaled_err(xt.cpu().numpy(), rt)
    print(f"[img2img] kernel {shape} Bm={m.shape[0]} {post}: x0 err {e0:.2e}, x_t err {et:.2e} (tol {R.TOL:g})")
    if post == 'mode':
        assert np.array_equal(x0.cpu().numpy(), r0)
    assert e0 <= R.TOL and et <= R.TOL
    # x0 is optional, and leaving it out changes nothing
    assert torch.equal(_run_kernel(m, k, post, want_x0=False), xt)


def test_kernel_clamps_the_logvar_at_both_ends():
    """logvar -40 and +25 in turn: std = exp(-15) and exp(10).  On its own, so that values of 2e4 do not set the scale the
    ordinary case is judged at"""
    shape = R.SHAPES[0]
    m, k = R.moments(shape, shape[0], 'clamp'), R.keys(shape[0])
    x0, xt = _run_kernel(m, k, 'sample')
    r0, rt = R.reference(m, k, 'sample')
    assert float(np.abs(r0).max()) > 1e3 and bool(torch.isfinite(xt).all())
    e0, et = R.scaled_err(x0.cpu().numpy(), r0), R.scaled_err(xt.cpu().numpy(), rt)
    print(f"[img2img] kernel clamp case: x0 err {e0:.2e}, x_t err {et:.2e}, max|x0| {float(np.abs(r0).max()):.3e}")
    assert e0 <= R.TOL and et <= R.TOL
    # where the clamp gave exp(-15) the posterior noise is gone below fp32 resolution of the mean: relative check there
    lo = np.transpose(m[..., 4:].astype(np.float64), (0, 3, 1, 2)) < 0
    d = np.abs(x0.cpu().numpy().astype(np.float64) - r0)[lo] / np.maximum(np.abs(r0[lo]), 1e-3)
    assert float(d.max()) <= 1e-5


def test_kernel_grid_stride_loop():
    """2^18 + 1 quads: one more than the 1024 x 256 threads of the largest grid (csrc/latent.hip)"""
    shape = R.PAST_THE_GRID
    m, k = R.moments(shape, 1), R.keys(1)
    x0, xt = _run_kernel(m, k, 'sample')
    r0, rt = R.reference(m, k, 'sample')
    e0, et = R.scaled_err(x0.cpu().numpy(), r0), R.scaled_err(xt.cpu().numpy(), rt)
    print(f"[img2img] kernel {shape}: x0 err {e0:.2e}, x_t err {et:.2e}")
    assert e0 <= R.TOL and et <= R.TOL
    assert not np.array_equal(xt.cpu().numpy()[0, :, 0, -1], np.zeros(4, np.float32))      # the last quad was written


def test_rows_are_independent():
    """tests/test_device_noise_gpu.py::test_rows_are_independent for the start: permuting the key rows (and the pictures
    with them) permutes the outputs, bit for bit; changing one row's key changes that row only"""
    from lib.hip import ops
    shape = (4, 4, 8, 8)
    m = T(R.moments(shape, 4)).cuda()
    rows = [(0, 3), (-1, 1), ((1 << 40) + 12345, 2), (20, 0)]
    key = lambda r: torch.tensor(r, dtype=torch.int64).cuda()      # noqa: E731
    b0, bt = ops.latent_start(m, key(rows), R.SCALE_FACTOR, R.A_T, want_x0=True)
    perm = [2, 0, 3, 1]
    p0, pt = ops.latent_start(m[perm].contiguous(), key([rows[i] for i in perm]), R.SCALE_FACTOR, R.A_T, want_x0=True)
    assert torch.equal(p0, b0[perm]) and torch.equal(pt, bt[perm])
    for changed in ((0, 4), (1, 3)):
        rows2 = list(rows)
        rows2[1] = changed
        o0, ot = ops.latent_start(m, key(rows2), R.SCALE_FACTOR, R.A_T, want_x0=True)
        assert not torch.equal(ot[1], bt[1]) and not torch.equal(o0[1], b0[1])
        assert torch.equal(ot[[0, 2, 3]], bt[[0, 2, 3]]) and torch.equal(o0[[0, 2, 3]], b0[[0, 2, 3]])
    # a shared picture: row b of the broadcast call is row b of the call that was given B copies
    one = m[:1].contiguous()
    s0, st = ops.latent_start(one, key(rows), R.SCALE_FACTOR, R.A_T, want_x0=True)
    c0, ct = ops.latent_start(one.repeat(4, 1, 1, 1), key(rows), R.SCALE_FACTOR, R.A_T, want_x0=True)
    assert torch.equal(s0, c0) and torch.equal(st, ct)
    # a key on the host is accepted (copied)
    assert torch.equal(ops.latent_start(m, torch.tensor(rows, dtype=torch.int64), R.SCALE_FACTOR, R.A_T), bt)


def test_null_arguments_are_einval():
    from lib.hip import binding
    lib = binding.load()
    m = torch.zeros(1, 2, 2, 8, device='cuda', dtype=torch.float16)
    key = torch.zeros(1, 2, device='cuda', dtype=torch.int64)
    x = torch.zeros(1, 4, 2, 2, device='cuda')
    for args in ((None, 1, key.data_ptr()), (m.data_ptr(), 1, None), (m.data_ptr(), 2, key.data_ptr())):
        rc = lib.pfd_latent_start(*args, 1.0, 0.5, 0.5, 1.0, None, x.data_ptr(), 1, 4, 2, 2, None)
        assert rc == binding.PFD_EINVAL
    assert lib.pfd_latent_start(m.data_ptr(), 1, key.data_ptr(), 1.0, 0.5, 0.5, 1.0, None, None, 1, 4, 2, 2, None) == binding.PFD_EINVAL


# ---- the encoder -----------------------------------------------------------------------------------------------------
def test_moments_are_encodes_moments(net, golden):
    x = T(golden["vaeenc.x"]).cuda()
    m = net.vae_encode_moments(x, 'image')
    B, C2, h, w = golden["vaeenc.moments"].shape
    assert m.dtype == torch.float16 and m.shape == (B, h, w, C2) and C2 == 8 and m.is_contiguous()
    post = net.vae['image'].encode(x, out_posterior=True)
    assert torch.equal(m.permute(0, 3, 1, 2).to(post.parameters.dtype), post.parameters)
    e = scaled(m.permute(0, 3, 1, 2), golden["vaeenc.moments"])
    print(f"[img2img] vae_encode_moments {x.shape[2]}x{x.shape[3]} vs reference fixture: scaled max-abs err {e:.3e} (tol {TOL_STAGE:g})")
    assert e <= TOL_STAGE


@pytest.fixture(scope="module")
def fixture256():
    return dict(np.load(os.path.join(REPO, "tests", "golden", "img2img.npz"), allow_pickle=False))


def test_moments_at_256_match_the_oracle_fixture(net, fixture256):
    """65536 rows at the top level: the smallest picture that reaches the wide-tile dispatch a 512x512 request takes"""
    x = T(R.picture_f32(256, 256)).cuda().half()
    m = net.vae_encode_moments(x, 'image')
    assert m.shape == (1, 32, 32, 8)
    ref = fixture256["moments"]
    e = scaled(m.permute(0, 3, 1, 2), ref)
    print(f"[img2img] vae_encode_moments 256x256 vs oracle fixture: scaled max-abs err {e:.3e} (tol {TOL_STAGE:g}), "
          f"max|ref| {float(np.abs(ref).max()):.3f}")
    assert e <= TOL_STAGE


def test_uint8_picture_is_resized_into_the_encoders_layout(net):
    """a 100x80 uint8 picture -> 64x64: the f16 NHWC picture of the resize kernel, encoded, equals `ingest` (the same
    resize into NCHW) followed by the NCHW entry -- no float NCHW picture on the new path"""
    from lib.hip import ops
    from lib.pipeline import PromptFreePipeline
    u8 = R.picture_u8(100, 80, seed=3)
    pipe = PromptFreePipeline(net)
    nchw = pipe.ingest(u8, (64, 64), 'init')
    assert nchw.shape == (1, 3, 64, 64)
    nhwc = ops.image_from_u8(T(u8).cuda()[None], (64, 64), layout='nhwc')
    assert nhwc.shape == (1, 64, 64, 3) and torch.equal(nhwc.permute(0, 3, 1, 2), nchw)
    a, b = net.vae_encode_moments(nhwc, 'image'), net.vae_encode_moments(nchw, 'image')
    assert a.shape == (1, 8, 8, 8) and torch.equal(a, b)
    with pytest.raises(ValueError):
        net.vae['image'].encode_moments_nhwc(nhwc.float(), layout='nhwc')


# ---- sampler and pipeline --------------------------------------------------------------------------------------------
STEPS, STRENGTH, K = 8, 0.75, 6


def _init_u8():
    return R.picture_u8(96, 72, seed=1)


def _by_hand(net, golden, init_u8, keys, solver='ddim', host_start=True, posterior='sample'):
    """the sampler run by hand: the picture encoded on the device, the start from lib/img2img.py on the host (or from the
    kernel), K steps of STEPS -> (final latents, start)"""
    from lib import img2img
    from lib.hip import ops
    from lib.model_zoo.ddim import DDIMSampler
    from lib.pipeline import PromptFreePipeline
    pipe = PromptFreePipeline(net)
    pic = ops.image_from_u8(T(init_u8).cuda()[None], (64, 64), layout='nhwc')
    m = net.vae_encode_moments(pic, 'image')
    s = DDIMSampler(net)
    s.make_schedule(STEPS, ddim_eta=0., verbose=False)
    a_t = img2img.level(net.alphas_cumprod.float().cpu().numpy(), s.ddim_timesteps, K)
    assert a_t == float(s.ddim_alphas[K - 1])
    sf = net.latent_scale_factor['image']
    if host_start:
        start = T(img2img.latent_start_batch(R.nchw(m.cpu().numpy()), np.asarray(keys), sf, a_t, posterior)[1]).cuda()
    else:
        start = ops.latent_start(m, torch.tensor(keys, dtype=torch.int64), sf, a_t, posterior=posterior)
    n = len(keys)
    cond, zeros = pipe.encode_reference(T(golden["see.img"]).cuda(), n)
    x_info = {'type': 'image', 'xt': start, 'xt_steps': K}
    c_info = {'type': 'image', 'conditioning': cond, 'unconditional_conditioning': zeros, 'unconditional_guidance_scale': 2.0}
    how = {} if solver == 'ddim' else {'solver': solver}
    x, inter = s.sample(steps=STEPS, shape=[n, 4, 8, 8], x_info=x_info, c_info=c_info, eta=0., verbose=False, **how)
    assert len(s.ddim_timesteps) == STEPS
    return x, start


@pytest.fixture(scope="module")
def eager_i2i(net, golden):
    """computed once, never modified: generate(init=...) eager, n = 2, seed 11 -> (latents, timings)"""
    from lib.pipeline import PromptFreePipeline
    t = {}
    pipe = PromptFreePipeline(net)
    img, lat = pipe.generate(T(golden["see.img"]), 2, 64, 64, steps=STEPS, scale=2.0, seed=11, init=_init_u8(),
                             strength=STRENGTH, timings=t)
    return lat, t, img


@pytest.mark.parametrize("solver", ["ddim", "dpmpp_2m"])
def test_generate_with_init_matches_the_sampler_run_by_hand(net, golden, eager_i2i, solver):
    """from the host-specified start: the trajectory bound of tests/test_hip_parity.py (rel-L2 1e-2); from the kernel's
    start: the same launches, bit for bit"""
    from lib.pipeline import PromptFreePipeline
    keys = [(11, 0), (11, 1)]
    if solver == 'ddim':
        got, t, img = eager_i2i
        assert set(t) == {'ctx_encode_ms', 'init_encode_ms', 'ddim_loop_ms', 'vae_decode_ms'} and t['init_encode_ms'] > 0
        assert img.shape == (2, 3, 64, 64) and bool(torch.isfinite(img).all())
    else:
        got = PromptFreePipeline(net).generate(T(golden["see.img"]), 2, 64, 64, steps=STEPS, scale=2.0, seed=11,
                                               init=_init_u8(), strength=STRENGTH, decode=False, solver=solver)[1]
    want, start = _by_hand(net, golden, _init_u8(), keys, solver)
    r = rel_l2(got, want)
    print(f"[img2img] generate(init, {solver}) vs by hand from the host start: rel-L2 {r:.3e} (tol 1e-2)")
    assert r <= 1e-2
    same, dev_start = _by_hand(net, golden, _init_u8(), keys, solver, host_start=False)
    assert torch.equal(got, same)
    assert R.scaled_err(dev_start.cpu().numpy(), start.cpu().numpy()) <= R.TOL
    # the picture matters, the strength matters, and the run is not the plain one
    other = PromptFreePipeline(net).generate(T(golden["see.img"]), 2, 64, 64, steps=STEPS, scale=2.0, seed=11, decode=False,
                                             **({} if solver == 'ddim' else {'solver': solver}))[1]
    assert float((other.float() - got.float()).abs().max()) > 1e-2


def test_graphed_equals_eager(net, golden, eager_i2i):
    """as tests/test_device_noise_gpu.py asserts it for the seeded step noise: bit for bit, one captured loop, and a
    replay follows another picture and another seed"""
    from lib.pipeline import PromptFreePipeline
    pipe = PromptFreePipeline(net)
    pipe.enable_graph(True)
    img = T(golden["see.img"])
    kw = dict(steps=STEPS, scale=2.0, strength=STRENGTH, decode=False)
    a = pipe.generate(img, 2, 64, 64, seed=11, init=_init_u8(), **kw)[1]
    assert torch.equal(a, eager_i2i[0]) and len(pipe.sampler._graphs) == 1 and len(pipe._enc_stage.graphs) == 1
    eager = PromptFreePipeline(net)
    other = R.picture_u8(64, 64, seed=5)
    b = pipe.generate(img, 2, 64, 64, seed=12, init=other, **kw)[1]
    assert torch.equal(b, eager.generate(img, 2, 64, 64, seed=12, init=other, **kw)[1])
    assert len(pipe.sampler._graphs) == 1 and not torch.equal(a, b)
    assert torch.equal(pipe.generate(img, 2, 64, 64, seed=11, init=_init_u8(), **kw)[1], a)
    # a float init takes the NCHW entry of the encoder: the same picture, the same result
    f = eager.ingest(_init_u8(), (64, 64), 'init')
    assert torch.equal(eager.generate(img, 2, 64, 64, seed=11, init=f, **kw)[1], a)
    # the plain request still captures and replays its own graph
    p = pipe.generate(img, 2, 64, 64, steps=STEPS, scale=2.0, seed=11, decode=False)[1]
    assert len(pipe.sampler._graphs) == 2 and torch.equal(p, eager.generate(img, 2, 64, 64, steps=STEPS, scale=2.0, seed=11,
                                                                              decode=False)[1])


def test_a_sample_is_keyed_not_positioned(net, golden):
    """sample (seed, j = 2): its start has the same bits alone (keys (seed, 2)) and as row 2 of the global batch of 4 --
    and as row 0 of rank 1 of 2.  Behind the start the UNet picks its tiles by batch size, so the two trajectories are two
    fp16 evaluations of one trajectory: they agree within the trajectory bound of tests/test_hip_parity.py (rel-L2 1e-2)"""
    from lib.pipeline import PromptFreePipeline, shard_noise_keys
    pipe = PromptFreePipeline(net)
    init = _init_u8()
    four, k = pipe.init_latent(init, 64, 64, STEPS, STRENGTH, shard_noise_keys(4, 11, 0, 1))
    alone, _ = pipe.init_latent(init, 64, 64, STEPS, STRENGTH, torch.tensor([[11, 2]]))
    rank1, _ = pipe.init_latent(init, 64, 64, STEPS, STRENGTH, shard_noise_keys(4, 11, 1, 2))
    assert k == K and four.shape == (4, 4, 8, 8)
    assert torch.equal(four[2:3], alone) and torch.equal(four[2:], rank1)
    assert not torch.equal(four[2], four[1])
    img = T(golden["see.img"])
    kw = dict(steps=STEPS, scale=2.0, seed=11, init=init, strength=STRENGTH, decode=False)
    whole = pipe.generate(img, 4, 64, 64, **kw)[1].float()
    half = PromptFreePipeline(net, rank=1, world_size=2).generate(img, 4, 64, 64, **kw)[1].float()
    d, r = float((whole[2:] - half).abs().max()), rel_l2(half, whole[2:])
    print(f"[img2img] samples 2, 3 of 4: one rank vs rank 1 of 2, final latents max|diff| {d:.2e}, rel-L2 {r:.2e} (tol 1e-2)")
    assert r <= 1e-2


# ---- the server ------------------------------------------------------------------------------------------------------
def _held(srv, submits):
    """submit everything while the worker is held (tests/test_dpm_solver_gpu.py::_held)"""
    gate = threading.Event()
    srv.call(lambda n: gate.wait(30))
    futs = [srv.submit(*a, **k) for a, k in submits]
    gate.set()
    return [f.result(300) for f in futs]


def test_server_batches_img2img_requests_by_step_count(net, golden):
    """two requests of equal k share a batch, each with its own picture and keys; a request of another strength runs on its
    own; every caller gets what its solo run gives (the bound of tests/test_dpm_solver_gpu.py::test_server_batches_by_solver)"""
    from lib.pipeline import PromptFreePipeline
    from lib.serving import PromptFreeServer
    img1, img2 = T(golden["see.img"]), T(golden["see2.img"])
    pics = (_init_u8(), R.picture_u8(64, 64, seed=5), _init_u8())
    # 4 steps, as the served requests of the other GPU files: k = 3, 3 and 2
    submits = [((im, 1, 64, 64), dict(steps=4, seed=sd, as_uint8=False, init=pic, strength=st))
               for im, sd, pic, st in ((img1, 5, pics[0], 0.75), (img2, 6, pics[1], 0.75), (img1, 7, pics[2], 0.5))]
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
    for i, (a, k) in enumerate(submits):
        kw = dict(k)
        kw.pop('as_uint8')
        solo.append(pipe.generate(a[0], a[1], a[2], a[3], scale=2.0, **kw)[0].float().cpu())
    for i, (o, j) in enumerate(zip(outs, (0, 1, 0, 2))):
        e = scaled(o, solo[j])
        print(f"[img2img] served request {i} vs its solo run: scaled max-abs err {e:.3e} (tol 5e-3)")
        assert e <= 5e-3
    assert float((solo[0] - solo[2]).abs().max()) > 1e-3          # another strength is another picture
