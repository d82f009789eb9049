"""GPU (-m gpu): the fused CFG + DPM-Solver++(2M) step (pfd_cfg_dpmpp_step) -- the kernel against the closed formula in
fp64 (the DDIM formula on a first-order step) and, bit for bit, against the DDIM kernels' pred_x0; the sampler with
solver='dpmpp_1' against DDIM, the update rule of 'dpmpp_2m' step by step from the logged intermediates, eager against
graphed; PromptFreePipeline.generate(solver=...); PromptFreeServer batching by solver.  Measured maxima:
profiles/dpm_solver.md."""
import math
import threading

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

T = torch.from_numpy
SCALES = [1.5, 2.0, 7.25]
SCALE_ALL = 2.5


def close(a, ref, tol):
    """tests/test_hip_kernels.py::close, the reference in fp64"""
    e = float((a.double().cpu() - ref.double().cpu()).abs().max() / max(1.0, float(ref.abs().max())))
    assert e <= tol, e
    return e


def check(name, a, ref, tol):
    """tests/test_hip_parity.py::check"""
    a, ref = a.detach().double().cpu(), torch.as_tensor(ref).double().cpu()
    e = float((a - ref).abs().max() / max(1.0, float(ref.abs().max())))
    print(f"[dpm_solver] {name}: scaled max-abs err {e:.3e} (tol {tol:g})")
    assert e <= tol, f"{name}: {e} > {tol}"


def _schedule(S):
    """the project's schedule (linear-sqrt betas 0.00085 .. 0.012, T = 1000, uniform) -> (alphas, alphas_prev) in fp64"""
    from lib.model_zoo.diffusion_utils import make_beta_schedule, make_ddim_sampling_parameters, make_ddim_timesteps
    acp = np.cumprod(1.0 - make_beta_schedule("linear", 1000, linear_start=0.00085, linear_end=0.012))
    _, a, ap = make_ddim_sampling_parameters(acp, make_ddim_timesteps("uniform", S, 1000, verbose=False), 0.0, verbose=False)
    return np.asarray(a, dtype=np.float64), np.asarray(ap, dtype=np.float64)


def _rows():
    """(row index, fp64 table row, a_s) of the real 10-step table: a middle row and the row with the largest |w_prev|"""
    from lib import solver
    a, ap = _schedule(10)
    tab = solver.dpmpp_2m_table(a, ap, SCALE_ALL)
    big = int(np.argmax(np.abs(tab[:, 5])))
    mid = 5 if big != 5 else 4
    assert tab[mid, 5] != 0.0 and tab[big, 5] != 0.0
    return [(i, tab[i], float(ap[i])) for i in (mid, big)]


def _operands(shape, nb):
    B, C, h, w = shape
    g = torch.Generator().manual_seed(B * 100 + w + nb)
    eps = torch.randn((nb * B, h, w, C), generator=g).half().cuda()
    x = torch.randn(shape, generator=g).cuda()
    hist = torch.randn(shape, generator=g).cuda()
    return eps, x, hist


def _dev(row):
    return torch.tensor(row, dtype=torch.float32, device='cuda')


def _guided(eps, nb, B, s):
    """the guided eps in fp64, NCHW; s: one number or fp64 [B,1,1,1]"""
    e = eps.double().cpu().permute(0, 3, 1, 2)
    return e[:B] + s * (e[B:] - e[:B]) if nb == 2 else e * s


# ---- the kernel ------------------------------------------------------------------------------------------------------
# the shapes of test_mixed_batches_gpu.py: (3,4,8,8): B = 3 catches b mixed up with b % 2 or with the CFG half; (2,4,5,6):
# w % 4 != 0; (3,3,3,3): C*h*w = 27, odd everything, the grid's last block is partly idle.
SHAPES = [(3, 4, 8, 8), (2, 4, 5, 6), (3, 3, 3, 3)]


@pytest.mark.parametrize("per_sample", [False, True])
@pytest.mark.parametrize("history", [False, True])
@pytest.mark.parametrize("rep", [1, 2])
@pytest.mark.parametrize("nb", [1, 2])
@pytest.mark.parametrize("shape", SHAPES)
def test_kernel_matches_the_closed_formula_in_fp64(shape, nb, rep, history, per_sample):
    """tolerances of the step-kernel family (test_mixed_batches_gpu.py): 1e-5 on the fp32 outputs, 2e-3 on the f16 copy.
    Without history the reference is the DDIM formula of include/pfd_hip.h at sigma = 0, not the solver's."""
    from lib.hip import ops
    B, C, h, w = shape
    eps, x, hist = _operands(shape, nb)
    for i, row, a_s in _rows():
        coef = _dev(row)
        if per_sample:
            coef[6] = -99.0                                   # ignored
            scale = torch.tensor(SCALES[:B], device='cuda')
            s = scale.double().cpu().reshape(B, 1, 1, 1)
        else:
            scale, s = None, SCALE_ALL
        xn, p0, xin = ops.cfg_dpmpp_step(eps, nb, x, coef, hist if history else None, want_next=True, rep=rep, scale=scale)
        e = _guided(eps, nb, B, s)
        a_t = row[0]
        r0 = (x.double().cpu() - math.sqrt(1 - a_t) * e) / math.sqrt(a_t)
        if history:
            rn = row[2] * x.double().cpu() + row[3] * (row[4] * r0 + row[5] * hist.double().cpu())
        else:
            rn = math.sqrt(a_s) * r0 + math.sqrt(1 - a_s) * e
        e0, e1 = close(p0, r0, 1e-5), close(xn, rn, 1e-5)
        assert xin.shape == (rep * B, h, w, C) and xin.dtype == torch.float16
        e2 = max(close(xin[r * B:(r + 1) * B].permute(0, 3, 1, 2), rn, 2e-3) for r in range(rep))
        print(f"[dpm_solver] kernel {shape} nb={nb} rep={rep} history={history} per_sample={per_sample} row {i}: "
              f"pred_x0 {e0:.2e} x_next {e1:.2e} xin {e2:.2e}")
        _, _, none = ops.cfg_dpmpp_step(eps, nb, x, coef, hist if history else None, scale=scale)
        assert none is None                                   # want_next defaults to False


@pytest.mark.parametrize("history", [False, True])
@pytest.mark.parametrize("nb", [1, 2])
@pytest.mark.parametrize("shape", SHAPES)
def test_pred_x0_is_bitwise_the_ddim_kernels(shape, nb, history):
    """the same operations in the same order: no tolerance"""
    from lib.hip import ops
    B, C, h, w = shape
    eps, x, hist = _operands(shape, nb)
    hp = hist if history else None
    for i, row, a_s in _rows():
        ddim = torch.tensor([row[0], a_s, 0.0, row[1], SCALE_ALL], dtype=torch.float32, device='cuda')
        _, want, _ = ops.cfg_ddim_step(eps, nb, x, ddim)
        _, got, _ = ops.cfg_dpmpp_step(eps, nb, x, _dev(row), hp)
        assert torch.equal(got, want), (i, "coef[6]")
        scale = torch.tensor(SCALES[:B], device='cuda')
        _, want, _ = ops.cfg_ddim_step(eps, nb, x, ddim, scale=scale)
        _, got, _ = ops.cfg_dpmpp_step(eps, nb, x, _dev(row), hp, scale=scale)
        assert torch.equal(got, want), (i, "scale vector")


@pytest.mark.parametrize("history", [False, True])
@pytest.mark.parametrize("nb", [1, 2])
@pytest.mark.parametrize("shape", SHAPES)
def test_kernel_is_bitwise_the_batch_wide_call_per_sample(shape, nb, history):
    """test_mixed_batches_gpu.py::test_kernel_is_bitwise_the_batch_wide_kernel_per_sample for this kernel"""
    from lib.hip import ops
    B, C, h, w = shape
    eps, x, hist = _operands(shape, nb)
    hp = hist if history else None
    _, row, _ = _rows()[1]

    def coef(s):
        c = _dev(row)
        c[6] = s
        return c

    scalar = {s: ops.cfg_dpmpp_step(eps, nb, x, coef(s), hp, want_next=True) for s in SCALES[:B]}
    for s in SCALES[:B]:                                    # a uniform vector is the batch-wide call
        got = ops.cfg_dpmpp_step(eps, nb, x, coef(-99.0), hp, want_next=True, scale=torch.full((B,), s, device='cuda'))
        for a, b in zip(got, scalar[s]):
            assert torch.equal(a, b), s
    xn, p0, xin = ops.cfg_dpmpp_step(eps, nb, x, coef(-99.0), hp, want_next=True, scale=torch.tensor(SCALES[:B], device='cuda'))
    for b, s in enumerate(SCALES[:B]):                      # row b of a mixed call is row b of the call at scale[b]
        wn, w0, win = scalar[s]
        assert torch.equal(xn[b], wn[b]) and torch.equal(p0[b], w0[b]), b
        for r in range(nb):
            assert torch.equal(xin[r * B + b], win[r * B + b]), (b, r)
    assert not torch.equal(xn[0], scalar[SCALES[1]][0][0])  # ... and the scales do differ in their effect


@pytest.mark.parametrize("nb", [1, 2])
@pytest.mark.parametrize("shape", SHAPES)
def test_a_sample_reads_its_own_history_only(shape, nb):
    from lib.hip import ops
    B, C, h, w = shape
    eps, x, hist = _operands(shape, nb)
    _, row, _ = _rows()[1]
    base = ops.cfg_dpmpp_step(eps, nb, x, _dev(row), hist, want_next=True)
    for b in range(B):
        other = hist.clone()
        for bb in range(B):
            if bb != b:
                other[bb] += 3.0
        got = ops.cfg_dpmpp_step(eps, nb, x, _dev(row), other, want_next=True)
        assert torch.equal(got[0][b], base[0][b]) and torch.equal(got[1], base[1])
        for r in range(nb):
            assert torch.equal(got[2][r * B + b], base[2][r * B + b])
        assert not torch.equal(got[0][(b + 1) % B], base[0][(b + 1) % B])      # the history is read


def test_aliased_history_is_einval():
    from lib.hip import binding
    lib = binding.load()
    x = torch.zeros(1, 4, 8, 8, device='cuda')
    out = torch.zeros(2, 4, 8, 8, device='cuda')
    eps = torch.zeros(1, 8, 8, 4, device='cuda', dtype=torch.float16)
    coef = torch.ones(8, device='cuda')
    for hist in (out[0], out[1]):
        rc = lib.pfd_cfg_dpmpp_step(eps.data_ptr(), 1, x.data_ptr(), hist.data_ptr(), coef.data_ptr(), None,
                                    out[0].data_ptr(), out[1].data_ptr(), None, 1, 1, 4, 8, 8, None)
        assert rc == binding.PFD_EINVAL


# ---- the sampler -----------------------------------------------------------------------------------------------------
def _sample(net, golden, sampler, solver, steps=4, scale=2.0, seed=1, n=3, fp32_log=False, **kw):
    """test_mixed_batches_gpu.py::_sample with the solver as a parameter.  fp32_log: the context as an fp32 tensor of the
    same fp16 values, so that the sampler returns its fp32 latents and intermediates unrounded"""
    xT = torch.randn([n, 4, 8, 8], generator=torch.Generator().manual_seed(seed))
    c = T(golden["see.ctx"]).cuda().half().repeat(n, 1, 1)
    if fp32_log:
        c = c.float()
    x_info = {'type': 'image', 'xt': xT.cuda()}
    c_info = {'type': 'image', 'conditioning': c, 'unconditional_conditioning': torch.zeros_like(c),
              'unconditional_guidance_scale': scale}
    how = {} if solver is None else {'solver': solver}
    return sampler.sample(steps=steps, shape=[n, 4, 8, 8], x_info=x_info, c_info=c_info, eta=0., verbose=False, **how, **kw)


def _check_update_rule(name, x_start, inter, tab, first_row):
    """every logged step against x_next = c_x x + c_d (w_cur x0 + w_prev x0_last) in fp64, from the logged tensors and the
    fp32 table alone; first-order on the first and on the last step.  first_row: the table row of the run's first step"""
    xs, x0s = [t.double().cpu() for t in inter['pred_xt']], [t.double().cpu() for t in inter['pred_x0']]
    assert len(xs) == len(x0s) == first_row + 1
    x = x_start.double().cpu()
    worst = 0.0
    for i in range(first_row + 1):
        a_t, s1m, c_x, c_d, w_cur, w_prev = (float(v) for v in tab[first_row - i, :6])
        if i == 0 or i == first_row:
            d = x0s[i]
        else:
            assert w_prev < 0.0
            d = w_cur * x0s[i] + w_prev * x0s[i - 1]
        ref = c_x * x + c_d * d
        worst = max(worst, close(xs[i], ref, 1e-5))
        x = xs[i]
    print(f"[dpm_solver] {name}: update rule over {first_row + 1} steps, worst scaled max-abs err {worst:.2e} (tol 1e-05)")


@pytest.fixture(scope="module")
def eager_runs(net, golden):
    """computed once, never modified: DDIM and both solvers, eager, on the same inputs"""
    from lib.model_zoo.ddim import DDIMSampler
    s = DDIMSampler(net)
    return {k: _sample(net, golden, s, k, log_every_t=1) for k in ('ddim', 'dpmpp_1', 'dpmpp_2m')}


def test_sampler_dpmpp_1_is_ddim(net, golden, eager_runs):
    """4 steps; the difference is fp32 rounding fed through the fp16 UNet: the project's fp16 latent tolerance"""
    from lib.model_zoo.ddim import DDIMSampler
    check("dpmpp_1 vs ddim, final latents", eager_runs['dpmpp_1'][0], eager_runs['ddim'][0].double(), 1e-2)
    assert torch.equal(_sample(net, golden, DDIMSampler(net), None, log_every_t=1)[0], eager_runs['ddim'][0])   # the default


def test_sampler_dpmpp_2m_follows_the_update_rule(net, golden):
    from lib.model_zoo.ddim import DDIMSampler
    s = DDIMSampler(net)
    x, inter = _sample(net, golden, s, 'dpmpp_2m', fp32_log=True, log_every_t=1)
    assert x.dtype == torch.float32 and torch.equal(x, inter['pred_xt'][-1])
    xT = torch.randn([3, 4, 8, 8], generator=torch.Generator().manual_seed(1))
    tab = s._dpmpp_table(2.0, 2).double().cpu().numpy()
    assert tab.shape == (4, 8)
    _check_update_rule("dpmpp_2m, 4 steps", xT, inter, tab, 3)
    # dpmpp_1: the same check with the first-order table passes too, and it is another trajectory
    x1, inter1 = _sample(net, golden, s, 'dpmpp_1', fp32_log=True, log_every_t=1)
    xs = [xT.double()] + [t.double().cpu() for t in inter1['pred_xt']]
    for i in range(4):
        c_x, c_d = float(tab[3 - i, 2]), float(tab[3 - i, 3])
        close(xs[i + 1], c_x * xs[i] + c_d * inter1['pred_x0'][i].double().cpu(), 1e-5)


def test_sampler_history_is_used(net, golden):
    """6 steps: the second-order middle steps move the final latents away from the first-order run"""
    from lib.model_zoo.ddim import DDIMSampler
    s = DDIMSampler(net)
    second = _sample(net, golden, s, 'dpmpp_2m', steps=6)[0].float()
    first = _sample(net, golden, s, 'dpmpp_1', steps=6)[0].float()
    d = float((second - first).abs().max())
    print(f"[dpm_solver] 6 steps, dpmpp_2m vs dpmpp_1, final latents: max|diff| {d:.2e}")
    assert d > 1e-2


def test_graphed_equals_eager_and_replays_follow_the_static_buffers(net, golden, eager_runs):
    """the comparison of test_mixed_batches_gpu.py::test_one_graph_serves_every_mixture_of_scales: bit for bit"""
    from lib.model_zoo.ddim import DDIMSampler
    eager, graphed = DDIMSampler(net), DDIMSampler(net)
    graphed.enable_graph(True)
    res = []
    for seed in (1, 2, 1):
        xe, ie = (eager_runs['dpmpp_2m'] if seed == 1 else _sample(net, golden, eager, 'dpmpp_2m', seed=seed, log_every_t=1))
        xg, ig = _sample(net, golden, graphed, 'dpmpp_2m', seed=seed, log_every_t=1)
        assert torch.equal(xe, xg), seed
        assert len(ig['pred_x0']) == 4 and all(torch.equal(a, b) for a, b in zip(ie['pred_x0'], ig['pred_x0']))
        res.append(xg.float())
        assert len(graphed._graphs) == 1
    assert torch.equal(res[0], res[2]) and not torch.equal(res[0], res[1])
    # the graph key: the solver name only where it is not DDIM
    key = next(iter(graphed._graphs))
    assert key[-1] == 'dpmpp_2m'
    xd = _sample(net, golden, graphed, 'ddim', log_every_t=1)[0]
    assert len(graphed._graphs) == 2 and torch.equal(xd, eager_runs['ddim'][0])
    assert len([k for k in graphed._graphs if k != key][0]) == len(key) - 1
    x1 = _sample(net, golden, graphed, 'dpmpp_1', log_every_t=1)[0]
    assert len(graphed._graphs) == 3 and torch.equal(x1, eager_runs['dpmpp_1'][0])


def test_one_graph_serves_every_scale_vector(net, golden):
    from lib.model_zoo.ddim import DDIMSampler
    eager, graphed = DDIMSampler(net), DDIMSampler(net)
    graphed.enable_graph(True)
    res = []
    for vec in ([1.5, 2.0, 3.0], [3.0, 1.5, 2.0], [1.5, 2.0, 3.0]):
        xe = _sample(net, golden, eager, 'dpmpp_2m', scale=vec)[0]
        xg = _sample(net, golden, graphed, 'dpmpp_2m', scale=vec)[0]
        assert torch.equal(xe, xg), vec
        res.append(xg.float())
        assert len(graphed._graphs) == 1
    assert torch.equal(res[0], res[2]) and not torch.equal(res[0], res[1])
    # a uniform vector is the batch-wide scale
    assert torch.equal(_sample(net, golden, eager, 'dpmpp_2m', scale=[2.0, 2.0, 2.0])[0],
                       _sample(net, golden, eager, 'dpmpp_2m', scale=2.0)[0])


def test_img2img_start_is_first_order(net, golden, monkeypatch):
    """x_info['x0']: q_sample to ddim index 5 of 8, then 5 steps whose first has no history (the table row says second-order)"""
    from lib.model_zoo.ddim import DDIMSampler
    noise = T(golden["i2i.noise"]).cuda()
    monkeypatch.setattr(torch, "randn_like", lambda t, *a, **k: noise.to(dtype=t.dtype, device=t.device))
    s = DDIMSampler(net)
    cond = T(golden["see.ctx"]).cuda().half().float()
    x0 = T(golden["i2i.x0"]).cuda()
    x_info = {'type': 'image', 'x0': x0, 'x0_forward_timesteps': 5}
    c_info = {'type': 'image', 'conditioning': cond, 'unconditional_conditioning': torch.zeros_like(cond),
              'unconditional_guidance_scale': 2.0}
    x, inter = s.sample(steps=8, shape=[1, 4, 8, 8], x_info=x_info, c_info=c_info, eta=0., verbose=False, log_every_t=1,
                        solver='dpmpp_2m')
    assert len(s.ddim_timesteps) == 8
    ts = torch.full((1,), int(s.ddim_timesteps[5]), device='cuda', dtype=torch.long)
    x_start = net.q_sample(x0.float(), ts)
    tab = s._dpmpp_table(2.0, 2).double().cpu().numpy()
    assert tab[4, 5] != 0.0                                  # the row of the first step carries second-order weights
    _check_update_rule("img2img, dpmpp_2m, 5 of 8 steps", x_start, inter, tab, 4)
    assert bool(torch.isfinite(x).all())


# ---- the pipeline ----------------------------------------------------------------------------------------------------
def test_pipeline_hands_the_solver_to_the_sampler(net, golden):
    from lib.model_zoo.ddim import DDIMSampler
    from lib.pipeline import PromptFreePipeline, shard_xT
    img = T(golden["see.img"])
    pipe = PromptFreePipeline(net)
    got = pipe.generate(img, 2, 64, 64, steps=4, scale=2.0, seed=9, decode=False, solver='dpmpp_2m')[1]
    cond, zeros = pipe.encode_reference(img.to('cuda'), 2)
    x_info = {'type': 'image', 'xt': shard_xT(2, 64, 64, 9, 0, 1).cuda()}
    c_info = {'type': 'image', 'conditioning': cond, 'unconditional_conditioning': zeros, 'unconditional_guidance_scale': 2.0}
    want = DDIMSampler(net).sample(steps=4, shape=[2, 4, 8, 8], x_info=x_info, c_info=c_info, verbose=False,
                                   solver='dpmpp_2m')[0]
    assert torch.equal(got, want)
    ddim = pipe.generate(img, 2, 64, 64, steps=4, scale=2.0, seed=9, decode=False)[1]
    assert torch.equal(ddim, pipe.generate(img, 2, 64, 64, steps=4, scale=2.0, seed=9, decode=False, solver='ddim')[1])
    assert float((got.float() - ddim.float()).abs().max()) > 1e-2
    with pytest.raises(ValueError):
        pipe.generate(img, 2, 64, 64, steps=4, eta=0.5, decode=False, solver='dpmpp_2m')


# ---- the server ------------------------------------------------------------------------------------------------------
def _held(srv, submits):
    """submit everything while the worker is held (test_mixed_batches_gpu.py::_held)"""
    gate = threading.Event()
    srv.call(lambda n: gate.wait(30))
    futs = [srv.submit(*a, **k) for a, k in submits]
    gate.set()
    return [f.result(300) for f in futs]


def test_server_batches_by_solver(net, golden):
    """two dpmpp_2m requests share a batch; a ddim request queued after them runs in its own, and so does the dpmpp_2m
    request behind it (order is preserved); every caller gets what a direct call gives"""
    from lib.pipeline import PromptFreePipeline
    from lib.serving import PromptFreeServer
    img1, img2 = T(golden["see.img"]), T(golden["see2.img"])
    submits = [((im, 1, 64, 64), dict(steps=4, seed=sd, as_uint8=False, **how))
               for im, sd, how in ((img1, 5, dict(solver='dpmpp_2m')), (img2, 6, dict(solver='dpmpp_2m')), (img1, 7, {}),
                                   (img2, 8, dict(solver='dpmpp_2m')))]
    srv = PromptFreeServer(net, use_graph=False, max_batch=4)
    try:
        outs = _held(srv, submits)
        assert srv.batches == [2, 1, 1]
    finally:
        srv.close()
    pipe = PromptFreePipeline(net)
    for i, ((a, k), o) in enumerate(zip(submits, outs)):
        kw = dict(k)
        kw.pop('as_uint8')
        direct = pipe.generate(a[0], a[1], a[2], a[3], scale=2.0, **kw)[0].float().cpu()
        check(f"served request {i} ({k.get('solver', 'ddim')}) vs direct call", o, direct, 5e-3)
    # the solver reached the sampler: request 0 differs from the same request run with DDIM
    kw = dict(submits[0][1], solver='ddim')
    kw.pop('as_uint8')
    other = pipe.generate(img1, 1, 64, 64, scale=2.0, **kw)[0].float().cpu()
    d = float((outs[0].float().cpu() - other).abs().max())
    print(f"[dpm_solver] served dpmpp_2m request 0 vs a direct DDIM call: max|diff| {d:.2e}")
    assert d > 1e-3
