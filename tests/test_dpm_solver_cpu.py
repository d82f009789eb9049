"""CPU: DPM-Solver++(2M) on the host -- lib/solver.py (the specification of pfd_cfg_dpmpp_step) against first principles,
against DDIM at order 1 and against an exact solution (it really is second-order); the C ABI declaration and argument
checks; what the sampler refuses, what `generate` hands the sampler and which requests the server lets share a batch."""
import ctypes
import os
import re
import threading

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _schedule(S):
    """the project's schedule: linear-sqrt betas 0.00085 .. 0.012, T = 1000, uniform timesteps -> (alphas, alphas_prev, acp)"""
    from lib.model_zoo.diffusion_utils import make_beta_schedule, make_ddim_sampling_parameters, make_ddim_timesteps
    acp = np.cumprod(1.0 - make_beta_schedule("linear", 1000, linear_start=0.00085, linear_end=0.012))
    ts = make_ddim_timesteps("uniform", S, 1000, verbose=False)
    _, a, ap = make_ddim_sampling_parameters(acp, ts, 0.0, verbose=False)
    return np.asarray(a, dtype=np.float64), np.asarray(ap, dtype=np.float64), acp


def _rel(a, b):
    return float(np.max(np.abs(a - b) / np.maximum(np.abs(b), 1e-300)))


# ---- the table -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [10, 50])
def test_table_against_first_principles(S):
    from lib import solver
    a, ap, acp = _schedule(S)
    assert ap[0] == acp[0] and np.array_equal(ap[1:], a[:-1])          # the last step targets alphas_cumprod[0], as DDIM
    tab = solver.dpmpp_2m_table(a, ap, 2.5)
    assert tab.dtype == np.float64 and tab.shape == (len(a), 8)
    a_t, s1m, c_x, c_d, w_cur, w_prev, scale, pad = tab.T
    assert np.array_equal(a_t, a) and np.array_equal(scale, np.full(len(a), 2.5)) and not pad.any()
    e1 = _rel(s1m, np.sqrt(1 - a))
    e2 = _rel(c_x * np.sqrt(1 - a), np.sqrt(1 - ap))
    e3 = _rel(w_cur + w_prev, np.ones(len(a)))
    e4 = _rel(c_d, np.sqrt(ap) - c_x * np.sqrt(a))
    print(f"[dpm_solver] table S={S}: sqrt(1-a_t) {e1:.1e}  c_x {e2:.1e}  w sum {e3:.1e}  c_d {e4:.1e}")
    assert max(e1, e2, e3, e4) <= 1e-12
    for row in (0, len(a) - 1):                                        # the last and the first step of a run
        assert w_cur[row] == 1.0 and w_prev[row] == 0.0
    # the middle rows: r = h_last / h with h_last the step BEFORE in the run (row i + 1), from the definition
    lam = lambda v: 0.5 * np.log(v / (1 - v))                          # noqa: E731
    h = lam(ap) - lam(a)
    assert (h > 0).all()
    for i in range(1, len(a) - 1):
        assert abs(w_prev[i] - (-0.5 * h[i] / h[i + 1])) <= 1e-12 * abs(w_prev[i]) and w_prev[i] < 0
    first = solver.dpmpp_2m_table(a, ap, 2.5, order=1)
    assert np.array_equal(first[:, 4], np.ones(len(a))) and not first[:, 5].any()
    assert np.array_equal(first[:, :4], tab[:, :4])
    with pytest.raises(ValueError):
        solver.dpmpp_2m_table(a, ap, 2.5, order=3)
    with pytest.raises(ValueError):
        solver.solver_order("euler")
    assert [solver.solver_order(s) for s in ("ddim", "dpmpp_2m", "dpmpp_1")] == [None, 2, 1]


def test_order_1_is_ddim_at_eta_0():
    """dpmpp_2m_run(order=1) against the closed DDIM formula of include/pfd_hip.h (sigma = 0), in fp64, on one random eps_fn"""
    from lib import solver
    a, ap, _ = _schedule(10)
    rng = np.random.default_rng(5)
    W = rng.standard_normal((16, 16)) / 4.0
    x_T = rng.standard_normal((3, 16))

    def eps_fn(x, i):
        return np.tanh(x @ W + 0.01 * i)

    x = x_T.copy()
    for i in range(len(a) - 1, -1, -1):
        e = eps_fn(x, i)
        p0 = (x - np.sqrt(1 - a[i]) * e) / np.sqrt(a[i])
        x = np.sqrt(ap[i]) * p0 + np.sqrt(1 - ap[i]) * e
    got = solver.dpmpp_2m_run(eps_fn, x_T, a, ap, order=1)
    err = float(np.abs(got - x).max() / max(1.0, np.abs(x).max()))
    print(f"[dpm_solver] order 1 vs DDIM over 10 steps: scaled max-abs err {err:.2e}")
    assert err <= 1e-12
    second = solver.dpmpp_2m_run(eps_fn, x_T, a, ap, order=2)           # ... and order 2 is another trajectory
    assert float(np.abs(second - x).max()) > 1e-4


def _gaussian_error(s2, S, order):
    """Gaussian data of variance s2: eps and the solution are known in closed form; scaled max error at the last target"""
    from lib import solver
    a, ap, acp = _schedule(S)
    x_T = np.random.default_rng(11).standard_normal(64)
    var = lambda v: v * s2 + 1 - v                                      # noqa: E731
    got = solver.dpmpp_2m_run(lambda x, i: np.sqrt(1 - a[i]) * x / var(a[i]), x_T, a, ap, order=order)
    exact = x_T * np.sqrt(var(acp[0]) / var(a[-1]))
    return float(np.abs(got - exact).max() / np.abs(exact).max())


@pytest.mark.parametrize("s2", [1, 4])
def test_the_solver_is_second_order(s2):
    err2 = {S: _gaussian_error(s2, S, 2) for S in (20, 50, 100)}
    err1 = {S: _gaussian_error(s2, S, 1) for S in (20, 50, 100)}
    for S in (20, 50, 100):
        print(f"[dpm_solver] s2={s2} S={S}: 2M {err2[S]:.3e}  first-order {err1[S]:.3e}  ratio {err1[S] / err2[S]:.2f}")
        assert err2[S] <= err1[S] / 1.4
    print(f"[dpm_solver] s2={s2}: err(50)/err(100)  2M {err2[50] / err2[100]:.2f}  first-order {err1[50] / err1[100]:.2f}")
    assert err2[50] / err2[100] >= 3.0
    assert err1[50] / err1[100] <= 2.1


# ---- header, binding, C ABI ------------------------------------------------------------------------------------------
def test_header_declares_and_binding_lists_the_entry_point():
    from lib.hip import binding
    src = open(os.path.join(REPO, "include", "pfd_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+pfd_cfg_dpmpp_step\s*\(([^)]*)\)\s*;", code)
    assert m and len(m.group(1).split(",")) == 15
    assert len(binding.SIGNATURES["pfd_cfg_dpmpp_step"][1]) == 15
    assert re.search(r"#define\s+PFD_ABI_VERSION\s+10\b", src) and binding.ABI_VERSION == 10     # added, not bumped
    assert binding.load().pfd_abi_version() == 10


def test_cabi_rejects_bad_arguments_without_a_gpu():
    """argument validation happens before any launch"""
    from lib.hip import binding
    lib = binding.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    good = dict(eps=p, nb=2, x=p, x0_prev=None, coef=p, scale=None, x_next=p, pred_x0=p, xin_next=None, rep=1, B=1, C=1,
                h=1, w=1)

    def call(**over):
        return lib.pfd_cfg_dpmpp_step(*dict(good, **over).values(), None)

    for name in ("eps", "x", "coef", "x_next", "pred_x0"):
        assert call(**{name: None}) == binding.PFD_EINVAL, name
    assert call(nb=3) == binding.PFD_EINVAL and call(nb=0) == binding.PFD_EINVAL
    assert call(xin_next=p, rep=0) == binding.PFD_EINVAL
    for name in ("B", "C", "h", "w"):
        assert call(**{name: 0}) == binding.PFD_EINVAL, name
    assert call(C=1 << 15, h=1 << 10, w=1 << 10) == binding.PFD_EINVAL      # C*h*w > 2^34, the bound of the siblings
    other = ctypes.cast(ctypes.create_string_buffer(64), ctypes.c_void_p)
    assert call(x0_prev=p, x_next=other) == binding.PFD_EINVAL               # the history aliases pred_x0


def test_ops_refuse_malformed_operands():
    from lib.hip import ops
    x = torch.zeros(2, 4, 2, 2)
    eps = torch.zeros(2, 2, 2, 4, dtype=torch.float16)
    with pytest.raises(ValueError, match="coef"):
        ops.cfg_dpmpp_step(eps, 1, x, torch.zeros(5))                        # a DDIM row
    with pytest.raises(ValueError, match="x0_prev"):
        ops.cfg_dpmpp_step(eps, 1, x, torch.zeros(8), x0_prev=torch.zeros(2, 4, 2, 3))
    with pytest.raises(ValueError, match="per-sample guidance scale"):
        ops.cfg_dpmpp_step(eps, 1, x, torch.zeros(8), scale=[1.5, 2.0])


# ---- sampler ---------------------------------------------------------------------------------------------------------
def _bare_sampler():
    from lib.model_zoo.ddim import DDIMSampler
    s = DDIMSampler.__new__(DDIMSampler)
    s.model = None                                       # every refusal comes before the model is looked at
    return s


def test_sampler_refuses_an_unknown_solver_and_everything_that_draws_noise():
    s = _bare_sampler()
    c = torch.zeros(1, 1, 1)
    c_info = {'type': 'image', 'conditioning': c, 'unconditional_conditioning': c, 'unconditional_guidance_scale': 2.0}
    kw = dict(steps=4, shape=[1, 4, 8, 8], c_info=c_info, verbose=False)
    with pytest.raises(ValueError, match="euler"):
        s.sample(x_info={'type': 'image'}, solver='euler', **kw)
    for solver in ('dpmpp_2m', 'dpmpp_1'):
        with pytest.raises(ValueError, match=solver):
            s.sample(x_info={'type': 'image'}, eta=0.5, solver=solver, **kw)
        with pytest.raises(ValueError, match=solver):
            s.sample(x_info={'type': 'image', 'noise_key': torch.zeros(1, 2, dtype=torch.int64)}, solver=solver, **kw)
        with pytest.raises(ValueError, match=solver):
            s.sample(x_info={'type': 'image'}, noise_dropout=0.1, solver=solver, **kw)
        with pytest.raises(ValueError, match=solver):
            s.sample_multicontext(4, [1, 4, 8, 8], {'type': 'image'}, [c_info], verbose=False, solver=solver)
    # ddim_sampling on its own checks the schedule it was given
    s.ddim_sigmas = np.array([0.0, 0.1])
    with pytest.raises(ValueError, match="dpmpp_2m"):
        s.ddim_sampling([1, 4, 8, 8], {'type': 'image'}, c_info, solver='dpmpp_2m')
    with pytest.raises(ValueError, match="euler"):
        s.ddim_sampling([1, 4, 8, 8], {'type': 'image'}, c_info, solver='euler')


# ---- pipeline --------------------------------------------------------------------------------------------------------
def test_generate_hands_the_solver_on_only_when_it_is_not_the_default():
    from stubs import StubNet
    from lib.pipeline import PromptFreePipeline

    class _Old:                                          # the stand-in of the existing tests: it knows no `solver`
        def sample(self, steps, shape, x_info, c_info, eta=0., verbose=True):
            return x_info['xt'], {}

    seen = {}

    class _New:
        def sample(self, steps, shape, x_info, c_info, eta=0., verbose=True, **kw):
            seen.update(kw=kw, steps=steps)
            return x_info['xt'] * 2, {}

    img = torch.rand(1, 3, 64, 64)
    PromptFreePipeline(StubNet(), sampler=_Old()).generate(img, 2, 64, 64, steps=2, decode=False)
    PromptFreePipeline(StubNet(), sampler=_Old()).generate(img, 2, 64, 64, steps=2, decode=False, solver='ddim')
    pipe = PromptFreePipeline(StubNet(), sampler=_New())
    pipe.generate(img, 2, 64, 64, steps=2, decode=False)
    assert seen['kw'] == {}
    pipe.generate(img, 2, 64, 64, steps=2, decode=False, solver='ddim')
    assert seen['kw'] == {}
    x, _ = pipe.generate(img, 2, 64, 64, steps=3, decode=False, solver='dpmpp_2m')
    assert seen['kw'] == {'solver': 'dpmpp_2m'} and seen['steps'] == 3 and tuple(x.shape) == (2, 4, 8, 8)
    pipe.generate(img, 2, 64, 64, steps=3, decode=False, solver='dpmpp_1')
    assert seen['kw'] == {'solver': 'dpmpp_1'}
    for bad in (dict(solver='euler'), dict(solver='dpmpp_2m', eta=0.5), dict(solver='dpmpp_2m', device_noise=True)):
        with pytest.raises(ValueError):
            pipe.generate(img, 2, 64, 64, steps=2, decode=False, **bad)


# ---- server (the pattern of tests/test_mixed_batches_cpu.py) ---------------------------------------------------------
def _server(monkeypatch, max_batch=4, **kw):
    """PromptFreeServer with the device work stubbed: `_generate` records its batches as lists of (seed, solver)"""
    from lib import serving

    class _Pipe:
        def __init__(self, net):
            pass

        def enable_graph(self, on):
            pass

    monkeypatch.setattr(serving, "PromptFreePipeline", _Pipe)
    srv = serving.PromptFreeServer(object(), use_graph=False, max_batch=max_batch, **kw)
    calls = []

    def fake_generate(batch):
        calls.append([(r.seed, r.solver) for r in batch])
        return [torch.full((r.n, 1), float(r.seed)) for r in batch]

    srv._generate = fake_generate
    return srv, calls


def _queued(srv, submits):
    """submit everything while the worker is held, so that all of it is queued when the worker looks"""
    gate = threading.Event()
    srv.call(lambda n: gate.wait(30))
    futs = [srv.submit(*a, **k) for a, k in submits]
    gate.set()
    return [f.result(30) for f in futs]


IMG = torch.rand(1, 3, 64, 64)


def _req(seed, **kw):
    return ((IMG, 1, 64, 64), dict(seed=seed, steps=4, **kw))


def test_request_key_carries_the_solver_only_when_it_is_not_ddim():
    from lib import serving
    kw = dict(image=IMG, n=1, height=64, width=64, steps=4, seed=1, eta=0.0, scale=1.5)
    R = serving._Request
    for mixed in (None, True):
        assert R(solver='ddim', mixed=mixed, **kw).key() == R(mixed=mixed, **kw).key()
        assert R(solver='dpmpp_2m', mixed=mixed, **kw).key() != R(mixed=mixed, **kw).key()
        assert R(solver='dpmpp_2m', mixed=mixed, **kw).key() == R(solver='dpmpp_2m', mixed=mixed, **kw).key()
        assert R(solver='dpmpp_2m', mixed=mixed, **kw).key() != R(solver='dpmpp_1', mixed=mixed, **kw).key()
    assert R(solver='ddim', **kw).key() == (64, 64, 4, 1.5, 0.0, True, True, False, False)      # today's tuple
    assert R(solver='dpmpp_2m', **kw).shareable()


@pytest.mark.parametrize("mixed", [False, True])
def test_server_never_mixes_solvers_in_a_batch(monkeypatch, mixed):
    srv, calls = _server(monkeypatch, mixed_batches=mixed)
    try:
        outs = _queued(srv, [_req(1, solver='dpmpp_2m'), _req(2, solver='dpmpp_2m'), _req(3), _req(4, solver='ddim'),
                             _req(5, solver='dpmpp_2m'), _req(6, solver='dpmpp_1')])
        assert calls == [[(1, 'dpmpp_2m'), (2, 'dpmpp_2m')], [(3, 'ddim'), (4, 'ddim')], [(5, 'dpmpp_2m')], [(6, 'dpmpp_1')]]
        assert [float(o[0, 0]) for o in outs] == [1.0, 2.0, 3.0, 4.0, 5.0, 6.0]             # each caller gets ITS result
    finally:
        srv.close()


def test_server_validates_the_solver_on_the_callers_thread(monkeypatch):
    srv, calls = _server(monkeypatch)
    try:
        for bad in (dict(solver='euler'), dict(solver='dpmpp_2m', eta=0.5), dict(solver='dpmpp_2m', device_noise=True),
                    dict(solver='dpmpp_1', eta=0.5, device_noise=True)):
            with pytest.raises(ValueError):
                srv.submit(IMG, 1, 64, 64, steps=4, **bad)
        assert srv.submit(IMG, 1, 64, 64, steps=4, seed=7, solver='ddim', eta=0.5).result(30) is not None   # DDIM: as before
        assert calls == [[(7, 'ddim')]]
    finally:
        srv.close()


def test_server_generate_forwards_the_solver():
    """the real `_generate` over stand-ins for the device work"""
    from stubs import StubNet
    from lib import serving

    seen = {}

    class _Sampler:
        def enable_graph(self, on=True):
            pass

        def sample(self, steps, shape, x_info, c_info, eta=0., verbose=True, **kw):
            seen['kw'] = kw
            return x_info['xt'], {}

    kw = dict(image=IMG, height=64, width=64, steps=2, eta=0.0, scale=2.0, as_uint8=False, future=None)
    srv = serving.PromptFreeServer(StubNet(), use_graph=False, max_batch=8)
    try:
        srv.pipe.sampler = _Sampler()
        R = serving._Request
        outs = srv._generate([R(n=2, seed=1, solver='dpmpp_2m', **kw), R(n=1, seed=2, solver='dpmpp_2m', **kw)])
        assert [o.shape[0] for o in outs] == [2, 1] and seen['kw'] == {'solver': 'dpmpp_2m'}
        srv._generate([R(n=1, seed=1, solver='ddim', **kw)])
        assert seen['kw'] == {}
        srv._generate([R(n=1, seed=1, **kw)])                # a request built without the slot: today's call
        assert seen['kw'] == {}
    finally:
        srv.close()
