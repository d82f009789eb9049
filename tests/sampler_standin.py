"""TEST INFRASTRUCTURE: the sampler's host layer (lib/model_zoo/ddim.py) on a machine without a GPU.

Three things, all torch on the CPU:
  * stand-ins of `ops.to_nhwc`, `ops.cfg_ddim_step` and `ops.cfg_dpmpp_step` with the signatures and the argument refusals of
    lib/hip/ops.py.  They compute the formulas documented in include/pfd_hip.h in fp32, operation for operation in the order of
    the kernels (`ddim_formula`, `dpmpp_formula`); the keyed noise is lib/noise.py, the DPM row has the layout of lib/solver.py.
    Every call appends one line to `LOG`;
  * `StubModel`: what DDIMSampler reads of the composite model (device, schedule buffers, prepare_context, prepare_context_mix,
    diffuser[x_type].emb_projections, apply_model_nhwc, q_sample, ctl.prepare_hint).  Its eps is `eps_formula`, a cheap deterministic
    function of the input, the context and the timestep; every apply_model_nhwc call is logged;
  * `CASES` and `run_case`: the sampler calls whose call log, generator position and output shapes are pinned line for line in
    tests/golden/sampler_host_calls.txt (tests/test_sampler_host_cpu.py).

`install(monkeypatch)` patches the attributes of lib.hip.ops, as tests/ops_standin.py::install does.

The fixture is regenerated with

    python tests/sampler_standin.py --write

Regenerate it only for a change that is MEANT to change the launch sequence, and read the diff: it is the change.
"""
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path.insert(0, os.path.join(REPO, "prompt-free-diffusion_amd"))

from lib import noise as _noise                                             # noqa: E402
from lib.hip import ops                                                     # noqa: E402
from lib.model_zoo.diffusion_utils import make_beta_schedule                # noqa: E402

FIXTURE = os.path.join(REPO, "tests", "golden", "sampler_host_calls.txt")
LOG = []
_LAST_PRED = [None]
SEED = 1234            # the global generator at the start of every case
SHAPE = [2, 4, 3, 5]


# ----------------------------------------------------------------------------------------------------------------------
# formulas (fp32, the kernels' order of operations)
# ----------------------------------------------------------------------------------------------------------------------
def nhwc_formula(x, mul=1.0, add=0.0, rep=1):
    return (x.float() * mul + add).permute(0, 2, 3, 1).to(torch.float16).repeat(rep, 1, 1, 1).contiguous()


def guided_eps(eps, nb, scale):
    """eps NHWC f16 [nb*B, h, w, C] -> the guided eps fp32 NCHW [B, C, h, w]; scale: 0-d or [B, 1, 1, 1] fp32"""
    B = eps.shape[0] // nb
    e = eps.float().permute(0, 3, 1, 2)
    if nb == 2:
        eu, ec = e[:B], e[B:]
        return eu + scale * (ec - eu)
    return e * scale


def keyed_noise(key, step, shape):
    """fp32 [B, C, h, w]: z(key row, step, element) of lib/noise.py"""
    ns = int(np.prod(shape[1:]))
    rows = [_noise.normal(int(s), int(i), int(step), ns) for s, i in key.tolist()]
    return torch.from_numpy(np.stack(rows)).reshape(shape)


def ddim_formula(e, x, coef, noise_term):
    """(x_prev, pred_x0) of pfd_cfg_ddim_step*: coef {a_t, a_prev, sigma, sqrt(1-a_t), scale}; noise_term: what sigma multiplies"""
    a_t, a_prev, sigma, s1mat = coef[0], coef[1], coef[2], coef[3]
    isq_at = 1.0 / torch.sqrt(a_t)
    sq_aprev = torch.sqrt(a_prev)
    dirc = torch.sqrt(torch.clamp(1.0 - a_prev - sigma * sigma, min=0.0))
    p0 = (x - s1mat * e) * isq_at
    xp = sq_aprev * p0 + dirc * e
    if noise_term is not None:
        xp = xp + sigma * noise_term
    return xp, p0


def dpmpp_formula(e, x, coef, x0_prev):
    """(x_next, pred_x0) of pfd_cfg_dpmpp_step: coef {a_t, sqrt(1-a_t), c_x, c_d, w_cur, w_prev, scale, 0}"""
    a_t, s1mat, c_x, c_d, w_cur, w_prev = (coef[i] for i in range(6))
    isq_at = 1.0 / torch.sqrt(a_t)
    p0 = (x - s1mat * e) * isq_at
    d = p0 if x0_prev is None else w_cur * p0 + w_prev * x0_prev
    return c_x * x + c_d * d, p0


def eps_formula(x_nhwc, bias, t0, hint=None):
    """the stub UNet: x NHWC f16 [N, h, w, C], bias fp32 [N] (from the context), t0 the step's timestep -> eps NHWC f16"""
    e = 0.5 * x_nhwc.float() - 0.25 * bias.reshape(-1, 1, 1, 1) + float(t0) * 1e-3
    if hint is not None:
        e = e + hint
    return e.to(torch.float16)


def context_bias(c):
    return c.float().mean(dim=(1, 2))


# ----------------------------------------------------------------------------------------------------------------------
# lib.hip.ops stand-ins
# ----------------------------------------------------------------------------------------------------------------------
def _hexrow(coef):
    return ",".join(float(v).hex() for v in coef.detach().to(torch.float32).reshape(-1).tolist())


def _scale_rows(scale, B, device):
    """ops.guidance_scale_rows without its insistence on a GPU tensor"""
    if not (torch.is_tensor(scale) and scale.dtype == torch.float32 and tuple(scale.shape) == (B,) and scale.is_contiguous()):
        raise ValueError(f"a per-sample guidance scale must be a contiguous float32 tensor [{B}]")
    if scale.device != torch.device(device):
        raise ValueError(f"a per-sample guidance scale must live on {device}, next to x")
    return scale


def _outputs(xp, p0, want_next, rep):
    xp, p0 = xp.contiguous(), p0.contiguous()
    xin = nhwc_formula(xp, rep=rep) if want_next else None
    _LAST_PRED[0] = p0
    return xp, p0, xin


def to_nhwc(x, mul=1.0, add=0.0, rep=1):
    if x.dtype not in (torch.float32, torch.float16):
        x = x.float()
    LOG.append(f"to_nhwc shape={tuple(x.shape)} rep={rep}")
    return nhwc_formula(x, mul, add, rep)


def cfg_ddim_step(eps, nb, x, coef, *, noise=None, want_next=True, rep=None, noise_key=None, step=None, noise_mul=1.0,
                  scale=None):
    B, Cc, h, w = x.shape
    rep = nb if rep is None else rep
    if noise_key is not None:
        if noise is not None:
            raise ValueError("cfg_ddim_step: give either noise or noise_key, not both")
        if step is None:
            raise ValueError("cfg_ddim_step: noise_key needs the DDIM step index (step=)")
        noise_key = ops.noise_key_rows(noise_key, B, x.device)
    if scale is not None:
        scale = _scale_rows(scale, B, x.device)
    assert tuple(coef.shape) == (5,) and coef.dtype == torch.float32 and tuple(eps.shape) == (nb * B, h, w, Cc)
    assert x.dtype == torch.float32 and x.is_contiguous() and (noise is None or (noise.is_contiguous() and noise.shape == x.shape))
    nz = "None" if noise is None else "(%.5f,%.5f)" % tuple(noise.reshape(-1)[:2].tolist())
    LOG.append(f"cfg_ddim_step nb={nb} rep={rep} want_next={want_next} coef={_hexrow(coef)} step={step} noise={nz} "
               f"key={noise_key is not None} noise_mul={float(noise_mul)!r} scale={scale is not None}")
    e = guided_eps(eps, nb, coef[4] if scale is None else scale.reshape(B, 1, 1, 1))
    term = noise
    if noise_key is not None:
        term = float(noise_mul) * keyed_noise(noise_key, step, x.shape)
    return _outputs(*ddim_formula(e, x, coef, term), want_next, rep)


def cfg_dpmpp_step(eps, nb, x, coef, x0_prev=None, want_next=False, rep=None, scale=None):
    B, Cc, h, w = x.shape
    rep = nb if rep is None else rep
    if tuple(coef.shape) != (8,) or coef.dtype != torch.float32:
        raise ValueError(f"cfg_dpmpp_step: coef must be a float32 row of 8 numbers: got {tuple(coef.shape)} {coef.dtype}")
    if x0_prev is not None and not (x0_prev.shape == x.shape and x0_prev.dtype == torch.float32 and
                                    x0_prev.device == x.device and x0_prev.is_contiguous()):
        raise ValueError("cfg_dpmpp_step: x0_prev must be a contiguous float32 tensor of x's shape, next to x")
    if scale is not None:
        scale = _scale_rows(scale, B, x.device)
    assert tuple(eps.shape) == (nb * B, h, w, Cc) and x.dtype == torch.float32 and x.is_contiguous()
    hist = "None" if x0_prev is None else ("previous pred_x0" if x0_prev is _LAST_PRED[0] else "ANOTHER TENSOR")
    LOG.append(f"cfg_dpmpp_step nb={nb} rep={rep} want_next={want_next} coef={_hexrow(coef)} x0_prev={hist} "
               f"scale={scale is not None}")
    e = guided_eps(eps, nb, coef[6] if scale is None else scale.reshape(B, 1, 1, 1))
    return _outputs(*dpmpp_formula(e, x, coef, x0_prev), want_next, rep)


def _fell_through(*a, **k):
    raise AssertionError("sampler on the stand-in: a call fell through to the real library")


def install(monkeypatch):
    """patch lib.hip.ops for this test: the three functions above and a trap on the stream lookup of the real wrappers"""
    del LOG[:]
    _LAST_PRED[0] = None
    for name in ("to_nhwc", "cfg_ddim_step", "cfg_dpmpp_step"):
        monkeypatch.setattr(ops, name, globals()[name])
    monkeypatch.setattr(ops, "_stream", _fell_through)


# ----------------------------------------------------------------------------------------------------------------------
# the model
# ----------------------------------------------------------------------------------------------------------------------
class _Ctx:
    def __init__(self, c):
        self.c = c
        self.zero_lead = 0

    def bias(self):
        return context_bias(self.c)


class _Mix:
    def __init__(self, c_info_list):
        self.contexts = [_Ctx(ci['c']) for ci in c_info_list]
        self.ratios = [float(ci['ratio']) for ci in c_info_list]

    @property
    def zero_lead(self):
        return [k.zero_lead for k in self.contexts]

    def bias(self):
        return mix_bias([(k.c, r) for k, r in zip(self.contexts, self.ratios)])


def mix_bias(pairs):
    b = 0.
    for c, r in pairs:
        b = b + r * context_bias(c)
    return b


class _Hint:
    def __init__(self, feat):
        self.feat = feat


def hint_formula(control):
    return control.float().mean().reshape(1, 1, 1, 1) * 0.125


class _Ctl:
    def prepare_hint(self, control):
        LOG.append(f"prepare_hint shape={tuple(control.shape)}")
        return _Hint(hint_formula(control))


class _Diffuser:
    def emb_projections(self, timesteps):
        LOG.append(f"emb_projections t={timesteps.tolist()}")
        return timesteps.float()[:, None] * 1e-3, None


class StubModel:
    device = 'cpu'
    num_timesteps = 1000

    def __init__(self):
        betas = make_beta_schedule("linear", 1000, linear_start=0.00085, linear_end=0.012)
        acp = np.cumprod(1.0 - betas)
        self.betas = torch.tensor(betas, dtype=torch.float32)
        self.alphas_cumprod = torch.tensor(acp, dtype=torch.float32)
        self.alphas_cumprod_prev = torch.tensor(np.append(1.0, acp[:-1]), dtype=torch.float32)
        self.diffuser = {'image': _Diffuser()}
        self.ctl = _Ctl()

    def prepare_context(self, c):
        return _Ctx(c)

    def prepare_context_mix(self, c_info_list, mixing_type='attention'):
        return _Mix(c_info_list)

    def q_sample(self, x_start, t, noise=None):
        noise = torch.randn_like(x_start) if noise is None else noise
        LOG.append(f"q_sample t={t.tolist()} noise=({noise.reshape(-1)[0]:.5f},{noise.reshape(-1)[1]:.5f})")
        return q_formula(self.alphas_cumprod, x_start, t, noise)

    def apply_model_nhwc(self, x_type, x_nhwc, timesteps, c_type, context, control=None, emb_table=None, cfg_pair=False):
        LOG.append(f"apply_model_nhwc x_type={x_type} shape={tuple(x_nhwc.shape)} t0={int(timesteps[0])} nt={timesteps.numel()} "
                   f"c_type={c_type} cfg_pair={cfg_pair} zero_lead={context.zero_lead} control={control is not None} "
                   f"emb_table={emb_table is not None}")
        assert x_nhwc.dtype == torch.float16
        x = torch.cat([x_nhwc, x_nhwc]) if cfg_pair else x_nhwc
        hint = None if control is None else (control.feat if hasattr(control, 'feat') else hint_formula(control))
        return eps_formula(x, context.bias(), timesteps[0], hint)


def q_formula(acp, x0, t, noise):
    a = acp[t].reshape(-1, 1, 1, 1)
    return torch.sqrt(a) * x0 + torch.sqrt(1.0 - a) * noise


# ----------------------------------------------------------------------------------------------------------------------
# the pinned cases
# ----------------------------------------------------------------------------------------------------------------------
def _case(cid, kind='sample', **kw):
    c = dict(id=cid, kind=kind, steps=4, eta=0., temperature=1., dropout=0., scale=2.5, uc='rand', key=False, solver='ddim',
             start='randn', log_every_t=100, callback=False, control=False, shortcut=True, share=True, cdtype=torch.float16,
             # multi-context: the contexts' uc; single steps: index, repeat_noise, use_original_steps
             ucs=('rand', 'zero'), index=2, repeat=False, orig=False)
    c.update(kw)
    return c


def _steps(prefix, kind):
    return [_case(f"{prefix}_no_noise", kind),
            _case(f"{prefix}_generator", kind, eta=1., temperature=0.75),
            _case(f"{prefix}_generator_dropout", kind, eta=1., dropout=0.25),
            _case(f"{prefix}_repeat_noise", kind, eta=1., repeat=True),
            _case(f"{prefix}_noise_key", kind, eta=1., key=True, temperature=0.75),
            _case(f"{prefix}_key_at_sigma_0", kind, key=True),
            _case(f"{prefix}_original_steps", kind, eta=1., orig=True, index=617),
            _case(f"{prefix}_scale_1", kind, eta=1., scale=1.0),
            _case(f"{prefix}_per_sample_scale", kind, eta=1., scale=[1.0, 3.5])]


CASES = [
    _case("eta0"),
    _case("eta1_generator", eta=1.),
    _case("eta1_generator_dropout", eta=1., dropout=0.25),
    _case("eta1_noise_key", eta=1., key=True),
    _case("temperature_generator", eta=1., temperature=0.75),
    _case("temperature_noise_key", eta=1., temperature=0.75, key=True),
    _case("scale_1", scale=1.0),
    _case("scale_1_eta1", scale=1.0, eta=1.),
    _case("no_uncond", uc=None),
    _case("per_sample_scale", scale=[1.0, 3.5]),
    _case("per_sample_scale_noise_key", scale=[1.0, 3.5], eta=1., key=True),
    _case("uncond_batch_1", uc='b1'),
    _case("zero_uncond_shortcut_on", uc='zero'),
    _case("zero_uncond_shortcut_off", uc='zero', shortcut=False),
    _case("share_cfg_prefix_off", share=False),
    _case("dpmpp_2m", solver='dpmpp_2m'),
    _case("dpmpp_2m_per_sample_scale", solver='dpmpp_2m', scale=[1.0, 3.5]),
    _case("dpmpp_2m_scale_1", solver='dpmpp_2m', scale=1.0),
    _case("dpmpp_1", solver='dpmpp_1'),
    _case("xt_start", start='xt'),
    _case("x0_start_ddim", start='x0'),
    _case("x0_start_ddim_eta1", start='x0', eta=1.),
    _case("x0_start_dpmpp_2m", start='x0', solver='dpmpp_2m'),
    _case("one_step", steps=1),
    _case("one_step_dpmpp_2m", steps=1, solver='dpmpp_2m'),
    _case("log_every_t_1", log_every_t=1),
    _case("fp32_context", cdtype=torch.float32, eta=1.),
    _case("control", control=True),
    _case("callback", kind='ddim_sampling', callback=True, eta=1.),
    _case("multicontext_scale_1_eta0", 'mc', scale=1.0),
    _case("multicontext_scale_1_eta1", 'mc', scale=1.0, eta=1.),
    _case("multicontext_scale_2_eta0", 'mc', scale=2.0),
    _case("multicontext_scale_2_eta1", 'mc', scale=2.0, eta=1., temperature=0.75, dropout=0.25),
    _case("multicontext_shortcut_off_x0_start", 'mc', scale=2.0, shortcut=False, start='x0', log_every_t=1),
] + _steps("p_sample_ddim", 'p') + _steps("p_sample_ddim_multicontext", 'pmc')
CASE_IDS = [c['id'] for c in CASES]


def build_inputs(case):
    """fresh x_info / c_info (or c_info_list) of a case, drawn from a generator of their own"""
    g = torch.Generator().manual_seed(7)
    bs = SHAPE[0]
    rn = lambda *s: torch.randn(*s, generator=g)                        # noqa: E731

    def c_info(uc):
        d = {'type': 'image', 'conditioning': rn(bs, 3, 8).to(case['cdtype']), 'unconditional_guidance_scale': case['scale']}
        if uc is not None:
            u = rn(1 if uc == 'b1' else bs, 3, 8).to(case['cdtype'])
            d['unconditional_conditioning'] = torch.zeros_like(u) if uc == 'zero' else u
        return d

    x_info = {'type': 'image'}
    if case['start'] == 'xt':
        x_info['xt'] = rn(*SHAPE)
    elif case['start'] == 'x0':
        x_info['x0'] = rn(*SHAPE)
        x_info['x0_forward_timesteps'] = 2
    if case['key']:
        x_info['noise_key'] = torch.from_numpy(_noise.sample_keys(99, 5, bs))
    if case['kind'] in ('p', 'pmc'):
        x_info['x'] = rn(*SHAPE).to(case['cdtype'])
    if case['kind'] in ('mc', 'pmc'):
        c = [dict(c_info(u), ratio=r) for u, r in zip(case['ucs'], (0.75, 0.25))]
    else:
        c = c_info(case['uc'])
        if case['control']:
            c['control'] = rn(1, 3, 6, 10)
    return x_info, c


def _desc(t):
    return f"{str(t.dtype).replace('torch.', '')}{tuple(t.shape)}"


def run_case(case, monkeypatch):
    """the case through DDIMSampler over the stand-ins -> (fixture lines, result dict)"""
    from lib.model_zoo.ddim import DDIMSampler
    install(monkeypatch)
    model = StubModel()
    s = DDIMSampler(model)
    s.zero_uncond_shortcut, s.share_cfg_prefix = case['shortcut'], case['share']
    x_info, c = build_inputs(case)
    kw = dict(noise_dropout=case['dropout'], temperature=case['temperature'])
    torch.manual_seed(SEED)
    res = dict(x_info=x_info, c=c)
    kind = case['kind']
    called = []
    try:
        if kind == 'sample':
            res['x'], res['inter'] = s.sample(case['steps'], SHAPE, x_info, c, eta=case['eta'], verbose=False,
                                              log_every_t=case['log_every_t'], solver=case['solver'], **kw)
        elif kind == 'ddim_sampling':
            s.make_schedule(case['steps'], ddim_eta=case['eta'], verbose=False)
            res['x'], res['inter'] = s.ddim_sampling(SHAPE, x_info, c, log_every_t=case['log_every_t'], solver=case['solver'],
                                                     callback=called.append if case['callback'] else None, **kw)
            LOG.append(f"callback calls={called}")
        elif kind == 'mc':
            res['x'], res['inter'] = s.sample_multicontext(case['steps'], SHAPE, x_info, c, eta=case['eta'], verbose=False,
                                                           log_every_t=case['log_every_t'], **kw)
        else:
            s.make_schedule(case['steps'], ddim_eta=case['eta'], verbose=False)
            fn = s.p_sample_ddim if kind == 'p' else s.p_sample_ddim_multicontext
            t = torch.full((SHAPE[0],), 617 if case['orig'] else 501, dtype=torch.long)
            res['x_prev'], res['pred_x0'] = fn(x_info, c, t, case['index'], repeat_noise=case['repeat'],
                                               use_original_steps=case['orig'], **kw)
    except ValueError as e:
        res['error'] = e
        LOG.append(f"ValueError: {e}")
    lines = list(LOG)
    lines.append("generator %.5f" % float(torch.randn(1)))
    if 'x' in res:
        lines.append(f"returns x={_desc(res['x'])} " + " ".join(
            f"{k}={[_desc(t) for t in v]}" for k, v in sorted(res['inter'].items())))
    if 'x_prev' in res:
        lines.append(f"returns x_prev={_desc(res['x_prev'])} pred_x0={_desc(res['pred_x0'])}")
    lines.append("x_info['x']=" + (_desc(x_info['x']) if 'x' in x_info else "absent") +
                 " c=" + ",".join(_desc(ci['c']) if 'c' in ci else "absent" for ci in (c if isinstance(c, list) else [c])))
    return lines, res


def read_fixture():
    """{case id: [lines]}"""
    out, cur = {}, None
    for line in open(FIXTURE).read().splitlines():
        if line.startswith("== "):
            cur = out.setdefault(line[3:], [])
        elif line and not line.startswith("#"):
            cur.append(line)
    return out


def write_fixture():
    import pytest
    text = ["# the sampler's host layer over tests/sampler_standin.py: every launch, generator position and output shape of every case.",
            "# Written by `python tests/sampler_standin.py --write`; pinned by tests/test_sampler_host_cpu.py."]
    for case in CASES:
        with pytest.MonkeyPatch.context() as mp:
            lines, _ = run_case(case, mp)
        text += ["", "== " + case['id']] + lines
    with open(FIXTURE, "w") as f:
        f.write("\n".join(text) + "\n")
    print(f"{FIXTURE}: {len(CASES)} cases, {len(text)} lines")


if __name__ == "__main__":
    if sys.argv[1:] != ["--write"]:
        sys.exit(__doc__)
    write_fixture()
