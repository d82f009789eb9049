"""GPU (-m gpu): one guidance scale per sample in the fused CFG + DDIM step (pfd_cfg_ddim_step_ps) -- the kernel against the
closed formula in fp64 and, bit for bit, against the batch-wide kernels; the sampler eager and graphed (one graph for every
mixture of scales); PromptFreePipeline.generate(scale=[...]); PromptFreeServer(mixed_batches=True) coalescing requests that
differ in scale or in control picture.  Measured maxima: profiles/mixed_batches.md."""
import math
import threading

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

T = torch.from_numpy
SCALES = [1.5, 2.0, 7.25]
ROWS = [(-1, 1), ((1 << 40) + 12345, 6), (20, 0)]
A_T, A_PREV, SIG = 0.4, 0.6, 0.1
STEP, MUL = 7, 0.5


def close(a, ref, tol):
    """tests/test_hip_kernels.py::close, the reference in fp64"""
    e = float((a.double().cpu() - ref.double().cpu()).abs().max() / max(1.0, float(ref.abs().max())))
    assert e <= tol, e
    return e


def check(name, a, ref, tol):
    """tests/test_hip_parity.py::check"""
    a, ref = a.detach().double().cpu(), torch.as_tensor(ref).double().cpu()
    e = float((a - ref).abs().max() / max(1.0, float(ref.abs().max())))
    print(f"[mixed_batches] {name}: scaled max-abs err {e:.3e} (tol {tol:g})")
    assert e <= tol, f"{name}: {e} > {tol}"


def _operands(shape, nb):
    B, C, h, w = shape
    g = torch.Generator().manual_seed(B * 100 + w + nb)
    eps = torch.randn((nb * B, h, w, C), generator=g).half().cuda()
    x = torch.randn(shape, generator=g).cuda()
    z = torch.randn(shape, generator=g).cuda()
    return eps, x, z


def _coef(scale):
    return torch.tensor([A_T, A_PREV, SIG, math.sqrt(1 - A_T), scale], device='cuda')


def _noise_kw(mode, z, B):
    if mode == "tensor":
        return dict(noise=z)
    if mode == "key":
        return dict(noise_key=torch.tensor(ROWS[:B], dtype=torch.int64).cuda(), step=STEP, noise_mul=MUL)
    return {}


# ---- the kernel ------------------------------------------------------------------------------------------------------
# (3,4,8,8): the 16-byte path, B = 3 catches b mixed up with b % 2 or with the CFG half; (2,4,5,6): w % 4 != 0, the scalar
# path with whole quads; (3,3,3,3): C*h*w = 27, a sample's last quad has a tail.
SHAPES = [(3, 4, 8, 8), (2, 4, 5, 6), (3, 3, 3, 3)]


@pytest.mark.parametrize("mode", ["none", "tensor", "key"])
@pytest.mark.parametrize("rep", [1, 2])
@pytest.mark.parametrize("nb", [1, 2])
@pytest.mark.parametrize("shape", SHAPES)
def test_kernel_matches_the_closed_formula_in_fp64(shape, nb, rep, mode):
    """tolerances of test_device_noise_gpu.py::test_fused_step_matches_two_launches_and_the_formula"""
    from lib import noise
    from lib.hip import ops
    B, C, h, w = shape
    eps, x, z = _operands(shape, nb)
    scale = torch.tensor(SCALES[:B], device='cuda')
    xp, p0, xin = ops.cfg_ddim_step(eps, nb, x, _coef(-99.0), rep=rep, scale=scale, **_noise_kw(mode, z, B))   # coef[4] is ignored
    s = scale.double().cpu().reshape(B, 1, 1, 1)
    e = eps.double().cpu().permute(0, 3, 1, 2)
    e = e[:B] + s * (e[B:] - e[:B]) if nb == 2 else e * s
    if mode == "tensor":
        nz = z.double().cpu()
    elif mode == "key":
        nz = MUL * T(np.stack([noise.normal(sd, j, STEP, C * h * w) for sd, j in ROWS[:B]])).double().reshape(shape)
    else:
        nz = torch.zeros(shape, dtype=torch.float64)
    r0 = (x.double().cpu() - math.sqrt(1 - A_T) * e) / math.sqrt(A_T)
    rp = math.sqrt(A_PREV) * r0 + math.sqrt(1 - A_PREV - SIG ** 2) * e + SIG * nz
    e0, e1 = close(p0, r0, 1e-5), close(xp, rp, 1e-5)
    assert xin.shape == (rep * B, h, w, C) and xin.dtype == torch.float16
    e2 = max(close(xin[r * B:(r + 1) * B].permute(0, 3, 1, 2), rp, 2e-3) for r in range(rep))
    print(f"[mixed_batches] kernel {shape} nb={nb} rep={rep} noise={mode}: pred_x0 {e0:.2e} x_prev {e1:.2e} xin {e2:.2e}")


@pytest.mark.parametrize("mode", ["none", "tensor", "key"])
@pytest.mark.parametrize("nb", [1, 2])
@pytest.mark.parametrize("shape", SHAPES)
def test_kernel_is_bitwise_the_batch_wide_kernel_per_sample(shape, nb, mode):
    """elementwise, the same operations in the same order: no tolerance"""
    from lib.hip import ops
    B, C, h, w = shape
    eps, x, z = _operands(shape, nb)
    kw = _noise_kw(mode, z, B)
    scalar = {s: ops.cfg_ddim_step(eps, nb, x, _coef(s), **kw) for s in SCALES[:B]}
    for s in SCALES[:B]:                                    # a uniform vector is the batch-wide call
        got = ops.cfg_ddim_step(eps, nb, x, _coef(-99.0), scale=torch.full((B,), s, device='cuda'), **kw)
        for a, b in zip(got, scalar[s]):
            assert torch.equal(a, b), (s, mode)
    xp, p0, xin = ops.cfg_ddim_step(eps, nb, x, _coef(-99.0), scale=torch.tensor(SCALES[:B], device='cuda'), **kw)
    for b, s in enumerate(SCALES[:B]):                      # row b of a mixed call is row b of the call at scale[b]
        wp, w0, win = scalar[s]
        assert torch.equal(xp[b], wp[b]) and torch.equal(p0[b], w0[b]), (b, mode)
        for r in range(nb):
            assert torch.equal(xin[r * B + b], win[r * B + b]), (b, r, mode)
    assert not torch.equal(xp[0], scalar[SCALES[1]][0][0])  # ... and the scales do differ in their effect


def test_missing_scale_is_einval():
    from lib.hip import binding
    lib = binding.load()
    x = torch.zeros(1, 4, 8, 8, device='cuda')
    eps = torch.zeros(1, 8, 8, 4, device='cuda', dtype=torch.float16)
    coef = torch.ones(5, device='cuda')
    rc = lib.pfd_cfg_ddim_step_ps(eps.data_ptr(), 1, x.data_ptr(), None, None, 0, 1.0, coef.data_ptr(), None, x.data_ptr(),
                                  x.data_ptr(), None, 1, 1, 4, 8, 8, None)
    assert rc == binding.PFD_EINVAL


# ---- the sampler -----------------------------------------------------------------------------------------------------
def _sample(net, golden, sampler, scale, eta=0., keys=None, n=3):
    """test_device_noise_gpu.py::_sample with the scale as a parameter"""
    xT = torch.randn([n, 4, 8, 8], generator=torch.Generator().manual_seed(1))
    c = T(golden["see.ctx"]).cuda().half().repeat(n, 1, 1)
    x_info = {'type': 'image', 'xt': xT.cuda()}
    if keys is not None:
        x_info['noise_key'] = torch.tensor(keys, dtype=torch.int64)
    c_info = {'type': 'image', 'conditioning': c, 'unconditional_conditioning': torch.zeros_like(c),
              'unconditional_guidance_scale': scale}
    return sampler.sample(steps=4, shape=[n, 4, 8, 8], x_info=x_info, c_info=c_info, eta=eta, verbose=False)


@pytest.fixture(scope="module")
def scalar_runs(net, golden):
    """the batch of three at each batch-wide scale, eager: computed once, never modified"""
    from lib.model_zoo.ddim import DDIMSampler
    s = DDIMSampler(net)
    return {v: _sample(net, golden, s, v)[0].float() for v in (1.5, 2.0, 3.0)}


def test_sampler_uniform_vector_equals_the_scalar_run(net, golden, scalar_runs):
    from lib.model_zoo.ddim import DDIMSampler
    eager, graphed = DDIMSampler(net), DDIMSampler(net)
    graphed.enable_graph(True)
    for form in ([2.0, 2.0, 2.0], torch.full((3,), 2.0), np.full(3, 2.0)):
        assert torch.equal(_sample(net, golden, eager, form)[0].float(), scalar_runs[2.0])
    assert torch.equal(_sample(net, golden, graphed, [2.0, 2.0, 2.0])[0].float(), scalar_runs[2.0])
    c = T(golden["see.ctx"]).cuda().half().repeat(3, 1, 1)
    with pytest.raises(ValueError):                         # CFG is always on with a vector: it needs the unconditional context
        eager.sample(steps=4, shape=[3, 4, 8, 8], x_info={'type': 'image'}, verbose=False,
                     c_info={'type': 'image', 'conditioning': c, 'unconditional_guidance_scale': [1.5, 2.0, 3.0]})
    with pytest.raises(ValueError):
        _sample(net, golden, eager, [1.5, 2.0])             # two scales for three samples


def test_sampler_mixed_scales_row_by_row(net, golden, scalar_runs):
    """row b of the mixed run against row b of the same batch run at scale[b]: the bound of
    test_device_noise_gpu.py::test_a_sample_does_not_depend_on_its_company"""
    from lib.model_zoo.ddim import DDIMSampler
    mixed = _sample(net, golden, DDIMSampler(net), [1.5, 2.0, 3.0])[0].float()
    for b, v in enumerate((1.5, 2.0, 3.0)):
        ref = scalar_runs[v][b]
        lim = 4e-3 * max(1.0, float(ref.abs().max()))
        d = float((mixed[b] - ref).abs().max())
        print(f"[mixed_batches] sampler, row {b} at scale {v} vs the batch-wide run: max|diff| {d:.2e} (limit {lim:.2e})")
        assert d <= lim
    for b in (0, 2):                                        # the scale was really used
        assert float((mixed[b] - scalar_runs[2.0][b]).abs().max()) > 1e-2


def test_one_graph_serves_every_mixture_of_scales(net, golden):
    from lib.model_zoo.ddim import DDIMSampler
    eager, graphed = DDIMSampler(net), DDIMSampler(net)
    graphed.enable_graph(True)
    res = []
    for vec in ([1.5, 2.0, 3.0], [3.0, 1.5, 2.0], [2.5, 2.5, 7.25], [1.5, 2.0, 3.0]):
        xe, ie = _sample(net, golden, eager, vec)
        xg, ig = _sample(net, golden, graphed, vec)
        assert torch.equal(xe, xg), vec
        assert torch.equal(ie['pred_x0'][-1], ig['pred_x0'][-1])
        res.append(xg.float())
        assert len(graphed._graphs) == 1
    assert torch.equal(res[0], res[3]) and not torch.equal(res[0], res[1])
    xs, _ = _sample(net, golden, graphed, 2.0)              # a batch-wide scale afterwards: its own graph, as before
    assert len(graphed._graphs) == 2
    assert torch.equal(xs, _sample(net, golden, eager, 2.0)[0])


def test_one_graph_with_seeded_noise_follows_both_static_buffers(net, golden):
    from lib.model_zoo.ddim import DDIMSampler
    eager, graphed = DDIMSampler(net), DDIMSampler(net)
    graphed.enable_graph(True)
    runs = [([1.5, 2.0, 3.0], [(20, 0), (20, 1), (20, 2)]), ([3.0, 1.5, 2.0], [(-7, 0), ((1 << 40) + 12345, 3), (5, 1)]),
            ([1.5, 2.0, 3.0], [(-7, 0), ((1 << 40) + 12345, 3), (5, 1)]), ([1.5, 2.0, 3.0], [(20, 0), (20, 1), (20, 2)])]
    res = []
    for vec, keys in runs:
        xe = _sample(net, golden, eager, vec, eta=0.5, keys=keys)[0]
        xg = _sample(net, golden, graphed, vec, eta=0.5, keys=keys)[0]
        assert torch.equal(xe, xg), (vec, keys)
        res.append(xg.float())
    assert len(graphed._graphs) == 1
    assert torch.equal(res[0], res[3])
    assert float((res[1] - res[2]).abs().max()) > 1e-2      # same keys, other scales
    assert float((res[2] - res[3]).abs().max()) > 1e-2      # same scales, other keys


# ---- the pipeline ----------------------------------------------------------------------------------------------------
def test_pipeline_takes_one_scale_per_sample(net, golden):
    from lib.pipeline import PromptFreePipeline
    img = T(golden["see.img"])
    pipe = PromptFreePipeline(net)
    scales = [1.5, 3.0]
    mixed = pipe.generate(img, 2, 64, 64, steps=4, scale=scales, seed=9, decode=False)[0].float()
    for b, v in enumerate(scales):
        ref = pipe.generate(img, 2, 64, 64, steps=4, scale=v, seed=9, decode=False)[0].float()[b]
        lim = 4e-3 * max(1.0, float(ref.abs().max()))
        d = float((mixed[b] - ref).abs().max())
        print(f"[mixed_batches] pipeline, row {b} at scale {v} vs generate(scale={v}): max|diff| {d:.2e} (limit {lim:.2e})")
        assert d <= lim
    assert float((mixed[0] - mixed[1]).abs().max()) > 1e-2
    with pytest.raises(ValueError):
        pipe.generate(img, 2, 64, 64, steps=4, scale=[1.5, 2.0, 3.0], seed=9, decode=False)


def test_pipeline_takes_one_hint_per_sample(net, golden):
    """control [n,3,H,W]: row b is guided by hint b -- it lands within the company-invariance bound of the run that gives
    every sample hint b, and closer to it than to the run that gives every sample the other hint"""
    from lib.pipeline import PromptFreePipeline
    img = T(golden["see.img"])
    pipe = PromptFreePipeline(net)
    hints = [kw['control'] for _, kw in _control_submits(golden)[:2]]
    hints[0] = pipe.ingest(hints[0], (64, 64), 'control').float().cpu()
    gen = lambda c: pipe.generate(img, 2, 64, 64, steps=4, scale=2.0, seed=9, control=c, decode=False)[0].float()  # noqa: E731
    both, shared = gen(torch.cat(hints)), [gen(h) for h in hints]
    for b in range(2):
        own, other = shared[b][b], shared[1 - b][b]
        lim = 4e-3 * max(1.0, float(own.abs().max()))
        d_own, d_other = float((both[b] - own).abs().max()), float((both[b] - other).abs().max())
        print(f"[mixed_batches] pipeline, row {b} under its own hint: max|diff| {d_own:.2e} (limit {lim:.2e}); "
              f"against the run under the other hint: {d_other:.2e}")
        assert d_own <= lim and d_own < d_other
    with pytest.raises(ValueError):
        gen(torch.cat(hints + hints[:1]))                   # three hints for two samples


# ---- the server ------------------------------------------------------------------------------------------------------
def _held(srv, submits):
    """submit everything while the worker is held (test_hip_parity.py::test_serving_queue_batches_requests_...)"""
    gate = threading.Event()
    srv.call(lambda n: gate.wait(30))
    futs = [srv.submit(*a, **k) for a, k in submits]
    gate.set()
    return [f.result(300) for f in futs]


def _scale_submits(golden):
    img1, img2 = T(golden["see.img"]), T(golden["see2.img"])
    return [((im, 1, 64, 64), dict(steps=4, seed=sd, scale=sc, as_uint8=False))
            for im, sd, sc in ((img1, 5, 1.5), (img2, 6, 2.0), (img1, 7, 3.0))]


def _control_submits(golden):
    img1, img2 = T(golden["see.img"]), T(golden["see2.img"])
    g = torch.Generator().manual_seed(3)
    ctl_u8 = torch.randint(0, 256, (100, 80, 3), generator=g, dtype=torch.uint8).numpy()      # a uint8 picture of another size
    ctl_f = torch.zeros(1, 3, 64, 64)                  # a white square on black: far from the noise picture above
    ctl_f[..., 16:48, 16:48] = 1.0
    return [((img1, 1, 64, 64), dict(steps=4, seed=5, control=ctl_u8, as_uint8=False)),
            ((img2, 1, 64, 64), dict(steps=4, seed=6, control=ctl_f, as_uint8=False)),
            ((img1, 1, 64, 64), dict(steps=4, seed=7, as_uint8=False))]


def _direct(pipe, a, k, **over):
    kw = dict(k, **over)
    kw.pop('as_uint8')
    return pipe.generate(a[0], a[1], a[2], a[3], scale=kw.pop('scale', 2.0), **kw)[0].float().cpu()


def test_server_coalesces_requests_that_differ_in_scale(net, golden):
    from lib.pipeline import PromptFreePipeline
    from lib.serving import PromptFreeServer
    submits = _scale_submits(golden)
    srv = PromptFreeServer(net, use_graph=False, max_batch=4, mixed_batches=True)
    try:
        outs = _held(srv, submits)
        assert srv.batches == [3]
    finally:
        srv.close()
    pipe = PromptFreePipeline(net)
    for i, ((a, k), o) in enumerate(zip(submits, outs)):
        check(f"served request {i} (scale {k['scale']}) vs direct call", o, _direct(pipe, a, k), 5e-3)


def test_server_coalesces_control_requests_each_with_its_own_hint(net, golden):
    from lib.pipeline import PromptFreePipeline
    from lib.serving import PromptFreeServer
    submits = _control_submits(golden)
    srv = PromptFreeServer(net, use_graph=False, max_batch=4, mixed_batches=True)
    try:
        outs = _held(srv, submits)
        assert srv.batches == [2, 1]
    finally:
        srv.close()
    pipe = PromptFreePipeline(net)
    for i, ((a, k), o) in enumerate(zip(submits, outs)):
        check(f"served control request {i} vs direct call", o, _direct(pipe, a, k), 5e-3)
    # request 1 saw ITS control picture, not request 0's
    other = _direct(pipe, submits[1][0], submits[1][1], control=submits[0][1]['control'])
    d = float((outs[1].float().cpu() - other).abs().max())
    print(f"[mixed_batches] served control request 1 vs a direct call with request 0's picture: max|diff| {d:.2e}")
    assert d > 1e-3


def test_server_without_the_flag_batches_as_before(net, golden):
    from lib.serving import PromptFreeServer
    for submits in (_scale_submits(golden), _control_submits(golden)):
        srv = PromptFreeServer(net, use_graph=False, max_batch=4)
        try:
            _held(srv, submits)
            assert srv.batches == [1, 1, 1]
        finally:
            srv.close()
