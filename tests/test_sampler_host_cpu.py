"""CPU: the sampler's host layer (lib/model_zoo/ddim.py: sample, ddim_sampling, sample_multicontext, p_sample_ddim,
p_sample_ddim_multicontext) over tests/sampler_standin.py.

Per case of sampler_standin.CASES:
  * the call log -- every model call and every step launch with its nb, rep, want_next, coefficient row (exact float32), step index,
    noise / key / scale / history arguments --, the position of the global generator afterwards and the shapes, dtypes and list
    lengths of what comes back equal tests/golden/sampler_host_calls.txt line for line;
  * the returned tensors equal (torch.equal) a plain loop written here from the stand-in's formulas: `_step` is the one step
    function of every solver and noise source, what differs between the cases is the numbers it is given.
"""
import types

import numpy as np
import pytest
import torch

import sampler_standin as SS
from lib import solver as _solver
from lib.model_zoo.diffusion_utils import make_ddim_sampling_parameters, make_ddim_timesteps

CASES = {c['id']: c for c in SS.CASES}


@pytest.fixture(scope="module")
def pinned():
    return SS.read_fixture()


def test_fixture_names_exactly_the_cases(pinned):
    assert list(pinned) == SS.CASE_IDS


# ---- the plain loop --------------------------------------------------------------------------------------------------
def _f32(v):
    return torch.tensor(float(v), dtype=torch.float32)


def _step(x, eps_u, eps_c, s, k, nz, hist):
    """guided eps, pred_x0, the update: every solver and noise source is a choice of the numbers in k"""
    e = eps_u + s * (eps_c - eps_u)
    p0 = (x - k.s1m * e) * k.isq
    return k.cx * x + k.cp * (k.wc * p0 + k.wp * hist) + k.ce * e + k.sg * nz, p0


def _ddim_numbers(a, ap, sg, s1):
    """a_t, a_prev, sigma, sqrt(1 - a_t) of one step (float32, as the coefficient table holds them)"""
    a, ap, sg, s1 = _f32(a), _f32(ap), _f32(sg), _f32(s1)
    return types.SimpleNamespace(s1m=s1, isq=1.0 / torch.sqrt(a), cx=_f32(0), cp=torch.sqrt(ap), wc=_f32(1), wp=_f32(0),
                                 ce=torch.sqrt(torch.clamp(1.0 - ap - sg * sg, min=0.0)), sg=sg)


def _dpmpp_numbers(row, first_order):
    r = [_f32(np.float32(v)) for v in row]
    wc, wp = (_f32(1), _f32(0)) if first_order else (r[4], r[5])
    return types.SimpleNamespace(s1m=r[1], isq=1.0 / torch.sqrt(r[0]), cx=r[2], cp=r[3], wc=wc, wp=wp, ce=_f32(0), sg=_f32(0))


def _contexts(case, c, bs):
    """(nb, scale [bs,1,1,1] fp32, bias of the unconditional rows | None, bias of the conditional rows)"""
    scale = case['scale']
    lst = c if isinstance(c, list) else [dict(c, ratio=1.0)]
    per_sample = isinstance(scale, list)
    nb = 2 if per_sample or not (scale == 1. or 'unconditional_conditioning' not in lst[0]) else 1
    s = torch.tensor(scale if per_sample else [scale] * bs, dtype=torch.float32).reshape(bs, 1, 1, 1)
    full = lambda u: u.expand(bs, -1, -1)                               # noqa: E731
    if isinstance(c, list):
        bias = lambda name: SS.mix_bias([(full(ci[name]), ci['ratio']) for ci in lst])   # noqa: E731
    else:
        bias = lambda name: SS.context_bias(full(c[name]))              # noqa: E731
    return nb, s, (bias('unconditional_conditioning') if nb == 2 else None), bias('conditioning')


def _eps(x, t, bias, hint):
    return SS.eps_formula(SS.nhwc_formula(x), bias, t, hint).float().permute(0, 3, 1, 2)


def _noise_source(case, x_info):
    """noise(x, index) of the case: zeros at eta 0, the keyed function, or the next draw of the global generator"""
    temperature, p = case['temperature'], case['dropout']
    if case['eta'] == 0.:
        return lambda x, index: torch.zeros_like(x)
    if case['key']:
        return lambda x, index: temperature * SS.keyed_noise(x_info['noise_key'], index, x.shape)

    def draw(x, index):
        n = torch.randn((1, *x.shape[1:])).repeat(x.shape[0], 1, 1, 1) if case['repeat'] else torch.randn_like(x)
        n = n * temperature
        return torch.nn.functional.dropout(n, p=p) if p > 0. else n
    return draw


def _plain_trajectory(case, model):
    x_info, c = SS.build_inputs(case)
    bs, dtype = SS.SHAPE[0], case['cdtype']
    torch.manual_seed(SS.SEED)
    acp = model.alphas_cumprod.float().numpy()
    ts = make_ddim_timesteps("uniform", case['steps'], 1000, verbose=False)
    sg, a, ap = make_ddim_sampling_parameters(acp, ts, case['eta'], verbose=False)
    order = _solver.solver_order(case['solver'])
    s1 = np.sqrt(1. - a)
    rows = None if order is None else _solver.dpmpp_2m_table(a, ap, 1.0, order)
    if case['start'] == 'xt':
        x = x_info['xt'].float()
    elif case['start'] == 'x0':
        k = x_info['x0_forward_timesteps']
        x = SS.q_formula(model.alphas_cumprod, x_info['x0'], torch.full((bs,), int(ts[k])), torch.randn_like(x_info['x0']))
        ts = ts[:k]
    else:
        x = torch.randn(SS.SHAPE, dtype=dtype).float()
    nb, s, bias_u, bias_c = _contexts(case, c, bs)
    hint = SS.hint_formula(c['control']) if case['control'] else None
    noise = _noise_source(case, x_info)
    n = len(ts)
    hist = torch.zeros_like(x)
    xs, x0s = [], []
    for i in range(n):
        index, t = n - 1 - i, int(ts[n - 1 - i])
        eps_c = _eps(x, t, bias_c, hint)
        eps_u = _eps(x, t, bias_u, hint) if nb == 2 else torch.zeros_like(x)
        k = _ddim_numbers(a[index], ap[index], sg[index], s1[index]) if order is None else \
            _dpmpp_numbers(rows[index], first_order=i == 0)
        x, hist = _step(x, eps_u, eps_c, s, k, noise(x, index), hist)
        if index % case['log_every_t'] == 0 or index == n - 1:
            xs.append(x.to(dtype))
            x0s.append(hist.to(dtype))
    return x.to(dtype), xs, x0s


def _plain_single_step(case, model):
    x_info, c = SS.build_inputs(case)
    x = x_info['x']
    bs, index = x.shape[0], case['index']
    torch.manual_seed(SS.SEED)
    acp, acp_prev = model.alphas_cumprod, model.alphas_cumprod_prev
    if case['orig']:
        sg = case['eta'] * torch.sqrt((1 - acp_prev) / (1 - acp) * (1 - acp / acp_prev))
        k = _ddim_numbers(acp[index], acp_prev[index], sg[index], torch.sqrt(1. - acp)[index])
        sigma = float(sg[index])
    else:
        ts = make_ddim_timesteps("uniform", case['steps'], 1000, verbose=False)
        sg, a, ap = make_ddim_sampling_parameters(acp.numpy(), ts, case['eta'], verbose=False)
        k = _ddim_numbers(a[index], ap[index], sg[index], np.sqrt(1. - a)[index])
        sigma = float(sg[index])
    assert (sigma != 0.) == (case['eta'] != 0.)
    nb, s, bias_u, bias_c = _contexts(case, c, bs)
    xf = x.float()
    t = 617 if case['orig'] else 501
    eps_c = _eps(xf, t, bias_c, None)
    eps_u = _eps(xf, t, bias_u, None) if nb == 2 else torch.zeros_like(xf)
    x_prev, p0 = _step(xf, eps_u, eps_c, s, k, _noise_source(case, x_info)(xf, index), torch.zeros_like(xf))
    return x_prev.to(x.dtype), p0.to(x.dtype), (torch.cat([x] * 2) if nb == 2 else x)


# ---- the cases -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", SS.CASE_IDS)
def test_sampler_host_layer(cid, pinned, monkeypatch):
    case = CASES[cid]
    lines, res = SS.run_case(case, monkeypatch)
    want = pinned[cid]
    for i, (g, w) in enumerate(zip(lines, want)):
        assert g == w, f"{cid}: line {i + 1} of the call log differs\n  now:    {g}\n  pinned: {w}"
    assert len(lines) == len(want), f"{cid}: {len(lines)} lines now, {len(want)} pinned"
    model = SS.StubModel()
    if 'error' in res:
        assert cid == "p_sample_ddim_multicontext_per_sample_scale" and "per-sample guidance scale" in str(res['error'])
        return
    if case['kind'] in ('p', 'pmc'):
        x_prev, p0, left = _plain_single_step(case, model)
        assert torch.equal(res['x_prev'], x_prev) and torch.equal(res['pred_x0'], p0)
        assert res['x_prev'].dtype == case['cdtype'] and torch.equal(res['x_info']['x'], left)
    else:
        x, xs, x0s = _plain_trajectory(case, model)
        assert res['x'].dtype == case['cdtype'] and torch.equal(res['x'], x)
        assert res['x_info']['x'] is res['x']
        assert sorted(res['inter']) == ['pred_x0', 'pred_xt']
        for got, ref in ((res['inter']['pred_xt'], xs), (res['inter']['pred_x0'], x0s)):
            assert len(got) == len(ref) and all(torch.equal(g, r) and g.dtype == r.dtype for g, r in zip(got, ref))
    # the plain loop drew what the sampler drew: the generator stands where the fixture says
    assert "generator %.5f" % float(torch.randn(1)) in want


def test_first_step_after_an_x0_start_is_first_order(pinned):
    """the shortened run of an img2img start begins without a history, at row 1 of a 4-row table whose weights are second-order"""
    steps = [ln for ln in pinned["x0_start_dpmpp_2m"] if ln.startswith("cfg_dpmpp_step")]
    assert len(steps) == 2 and all("x0_prev=None" in ln for ln in steps)       # (the last step of a run is first-order too)
    full = [ln for ln in pinned["dpmpp_2m"] if ln.startswith("cfg_dpmpp_step")]
    assert ["x0_prev=None" in ln for ln in full] == [True, False, False, True]
    assert all("x0_prev=None" in ln for ln in pinned["dpmpp_1"] if ln.startswith("cfg_dpmpp_step"))
    assert not any("ANOTHER TENSOR" in ln for lines in pinned.values() for ln in lines)
    row = lambda ln: ln.split("coef=")[1].split()[0]                    # noqa: E731
    assert row(steps[0]) == row(full[2]) and float.fromhex(row(steps[0]).split(",")[5]) != 0.


def test_standin_refuses_what_the_wrappers_refuse():
    x = torch.zeros(2, 4, 2, 2)
    eps = torch.zeros(2, 2, 2, 4, dtype=torch.float16)
    key = torch.zeros(2, 2, dtype=torch.int64)
    with pytest.raises(ValueError, match="either noise or noise_key"):
        SS.cfg_ddim_step(eps, 1, x, torch.ones(5), noise=x, noise_key=key, step=0)
    with pytest.raises(ValueError, match="step index"):
        SS.cfg_ddim_step(eps, 1, x, torch.ones(5), noise_key=key)
    with pytest.raises(ValueError, match="noise_key must be"):
        SS.cfg_ddim_step(eps, 1, x, torch.ones(5), noise_key=key[:1], step=0)
    for step in (SS.cfg_ddim_step, SS.cfg_dpmpp_step):
        with pytest.raises(ValueError, match="per-sample guidance scale"):
            step(eps, 1, x, torch.ones(5 if step is SS.cfg_ddim_step else 8), scale=[1.5, 2.0])
    with pytest.raises(ValueError, match="coef"):
        SS.cfg_dpmpp_step(eps, 1, x, torch.zeros(5))
    with pytest.raises(ValueError, match="x0_prev"):
        SS.cfg_dpmpp_step(eps, 1, x, torch.ones(8), x0_prev=torch.zeros(2, 4, 2, 3))
