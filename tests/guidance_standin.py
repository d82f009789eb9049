"""TEST INFRASTRUCTURE: guidance rescale over the sampler's stand-ins (tests/sampler_standin.py, left as it is): a torch
stand-in of `ops.guidance_rescale` (lib/guidance.py's formula in fp32 torch) and wrappers of `cfg_ddim_step` /
`cfg_dpmpp_step` that take the `eps_mul=` keyword.  Without the keyword a wrapper IS the stand-in underneath -- the same
log line, the same numbers -- so a plain request over this module logs what it logs over sampler_standin alone; with it, the
guided eps is multiplied per sample and the log line says so.  Every call of the statistics stand-in appends a line to
sampler_standin.LOG."""
import torch

import sampler_standin as SS
from lib.hip import ops


def guidance_rescale(eps, scale_or_rows, phi_rows):
    assert eps.dtype == torch.float16 and eps.dim() == 4 and eps.shape[0] % 2 == 0 and eps.is_contiguous()
    B = eps.shape[0] // 2
    assert phi_rows.dtype == torch.float32 and tuple(phi_rows.shape) == (B,)
    assert scale_or_rows.dtype == torch.float32 and (scale_or_rows.numel() == 1 or tuple(scale_or_rows.shape) == (B,))
    SS.LOG.append(f"guidance_rescale B={B} scales={scale_or_rows.numel()} phi={[round(float(v), 4) for v in phi_rows]}")
    e = eps.float().reshape(2, B, -1)
    s = scale_or_rows.reshape(-1, 1) if scale_or_rows.numel() == B and B > 1 else scale_or_rows.reshape(1, 1)
    g = e[0] + s * (e[1] - e[0])
    ratio = e[1].std(dim=1, unbiased=False) / g.std(dim=1, unbiased=False)
    mul = phi_rows * ratio + (1.0 - phi_rows)
    return torch.where(phi_rows == 0, torch.ones_like(mul), mul)


def _check_mul(eps_mul, nb, B):
    if nb != 2:
        raise ValueError("eps_mul (guidance rescale) needs the unconditional half: nb must be 2")
    assert eps_mul.dtype == torch.float32 and tuple(eps_mul.shape) == (B,)
    return eps_mul.reshape(B, 1, 1, 1)


def cfg_ddim_step(eps, nb, x, coef, *, eps_mul=None, **kw):
    if eps_mul is None:
        return SS.cfg_ddim_step(eps, nb, x, coef, **kw)
    B = x.shape[0]
    m = _check_mul(eps_mul, nb, B)
    noise, key, step, scale = kw.get('noise'), kw.get('noise_key'), kw.get('step'), kw.get('scale')
    rep = nb if kw.get('rep') is None else kw['rep']
    SS.LOG.append(f"cfg_ddim_step eps_mul=True nb={nb} rep={rep} want_next={kw.get('want_next', True)} step={step} "
                  f"noise={noise is not None} key={key is not None} scale={scale is not None}")
    e = m * SS.guided_eps(eps, nb, coef[4] if scale is None else scale.reshape(B, 1, 1, 1))
    term = noise
    if key is not None:
        term = float(kw.get('noise_mul', 1.0)) * SS.keyed_noise(key, step, x.shape)
    return SS._outputs(*SS.ddim_formula(e, x, coef, term), kw.get('want_next', True), rep)


def cfg_dpmpp_step(eps, nb, x, coef, x0_prev=None, want_next=False, rep=None, scale=None, eps_mul=None):
    if eps_mul is None:
        return SS.cfg_dpmpp_step(eps, nb, x, coef, x0_prev, want_next=want_next, rep=rep, scale=scale)
    B = x.shape[0]
    m = _check_mul(eps_mul, nb, B)
    rep = nb if rep is None else rep
    SS.LOG.append(f"cfg_dpmpp_step eps_mul=True nb={nb} rep={rep} want_next={want_next} x0_prev={x0_prev is not None} "
                  f"scale={scale is not None}")
    e = m * SS.guided_eps(eps, nb, coef[6] if scale is None else scale.reshape(B, 1, 1, 1))
    return SS._outputs(*SS.dpmpp_formula(e, x, coef, x0_prev), want_next, rep)


def install(monkeypatch):
    """sampler_standin.install, then the three functions above over it"""
    SS.install(monkeypatch)
    for name in ("guidance_rescale", "cfg_ddim_step", "cfg_dpmpp_step"):
        monkeypatch.setattr(ops, name, globals()[name])


def launches():
    """the step and statistics lines of the log, shortened to their names"""
    return [ln.split()[0] + (" eps_mul" if " eps_mul=True" in ln else "") for ln in SS.LOG
            if ln.startswith(("guidance_rescale", "cfg_ddim_step", "cfg_dpmpp_step"))]
