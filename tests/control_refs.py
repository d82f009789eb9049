"""TEST INFRASTRUCTURE shared by tests/test_control_cpu.py, test_control_kernels_gpu.py and test_control_gpu.py: the cases of the
scaled-add kernel (pfd_add_scaled_rows_f16) with its error bound, a sampler stand-in model that accepts `control_scale`, and
the miniature UNet walk with scaled ControlNet residuals in fp64.

The kernel's bound, per element, against y64 = x + s * r evaluated in fp64 on the f16 inputs and the fp32 scale:

    |y - y64| <= 2^-11 |y64| + 2^-24 (|x| + |s r|) + 2^-25

one f16 rounding of the result (half an ulp, relative 2^-11), one fp32 rounding of the fma (relative 2^-24 of the result,
bounded by the operands' magnitudes, which also covers the cancelling case x ~ -s r) and half the spacing of the f16
subnormals (2^-25), below which the relative term means nothing."""
import numpy as np
import torch

import block_refs as BR
import sampler_standin as SS

COMPANY = 5e-3          # the company-invariance bound of tests/test_mixed_batches_gpu.py (scaled max-abs error)

# (B, n_per_sample): one vector, a size that is no multiple of the block (41 vectors), more than one block per sample
SHAPES = [(B, n) for B in (1, 3) for n in (8, 328, 40960)]
STRIDES = (1, 13)
ALIASES = (0, 1, 2)     # y apart, y = x, y = r
BIG = (8, 64 * 64 * 320)


def bound(x, r, s, y64):
    sr = np.abs(s.astype(np.float64).reshape(-1, 1) * r.astype(np.float64))
    return 2.0 ** -11 * np.abs(y64) + 2.0 ** -24 * (np.abs(x.astype(np.float64)) + sr) + 2.0 ** -25


def operands(B, n, kind, seed):
    """x, r f16 [B, n] and s fp32 [B] of a case: 'act' at activation range, 'small' at 1e-4, 'cancel' with x ~ -s r,
    'ones' / 'zeros' the scale exactly 1 / 0 (r holding NaN at scale 0: it must not be read)"""
    g = np.random.default_rng(seed)
    s = g.uniform(0.05, 2.0, B).astype(np.float32)
    mag = 1e-4 if kind == 'small' else 3.0
    x = (g.standard_normal((B, n)) * mag).astype(np.float16)
    r = (g.standard_normal((B, n)) * mag).astype(np.float16)
    if kind == 'cancel':
        x = (-(s.astype(np.float64)[:, None] * r.astype(np.float64)) * (1 + 1e-3 * g.standard_normal((B, n)))).astype(np.float16)
    elif kind == 'ones':
        s[:] = 1.0
    elif kind == 'zeros':
        s[:] = 0.0
        r[:, ::3] = np.nan
    elif kind == 'mixed':              # one sample off, the others on: the branch is per sample
        s[0] = 0.0
        r[0, ::5] = np.nan
    return x, r, s


def kernel_cases():
    """every shape x stride x alias once, the kinds going round"""
    kinds = ('act', 'small', 'cancel', 'ones', 'zeros', 'mixed')
    out, i = [], 0
    for B, n in SHAPES:
        for stride in STRIDES:
            for alias in ALIASES:
                out.append(dict(B=B, n=n, stride=stride, alias=alias, kind=kinds[i % len(kinds)], seed=100 + i))
                i += 1
    return out


def case_id(c):
    return f"B{c['B']}-n{c['n']}-stride{c['stride']}-alias{c['alias']}-{c['kind']}"


def strided_scale(s, stride):
    """the scale vector as column 0 of a [B, stride] fp32 table filled with another number"""
    tab = np.full((s.shape[0], stride), 7.5, dtype=np.float32)
    tab[:, 0] = s
    return tab


def judge(y, x, r, s):
    """-> the largest error in units of the bound; rows of scale 0 must be x's bits"""
    from lib import control
    y64 = control.add_scaled(x, r, s)
    on = s != 0
    for b in np.nonzero(~on)[0]:
        assert np.array_equal(y[b].view(np.uint16), x[b].view(np.uint16)), f"sample {b}: scale 0 must give x's bits"
    if not on.any():
        return 0.0
    e = np.abs(y[on].astype(np.float64) - y64[on]) / bound(x[on], r[on], s[on], y64[on])
    return float(e.max())


# ---- the sampler stand-in ------------------------------------------------------------------------------------------------
class ControlStub(SS.StubModel):
    """tests/sampler_standin.py::StubModel with the control_scale keyword: the hint enters eps weighted by the mean of the
    sample's table row, and every call is logged with whether it carried a control and a table"""

    def apply_model_nhwc(self, x_type, x_nhwc, timesteps, c_type, context, control=None, emb_table=None, cfg_pair=False,
                         control_scale=None):
        eps = super().apply_model_nhwc(x_type, x_nhwc, timesteps, c_type, context, control=None, emb_table=emb_table,
                                       cfg_pair=cfg_pair)
        SS.LOG[-1] = SS.LOG[-1].replace("control=False", f"control={control is not None} table={control_scale is not None}")
        if control is not None:
            w = torch.ones(eps.shape[0]) if control_scale is None else control_scale.float().mean(1)
            eps = (eps.float() + w.reshape(-1, 1, 1, 1) * control.feat).to(torch.float16)
        return eps


def model_calls():
    return [ln.split("control=")[1].split(" emb_table")[0] for ln in SS.LOG if ln.startswith("apply_model_nhwc")]


# ---- the miniature UNet walk ---------------------------------------------------------------------------------------------
def unet_table(B, n_res=5):
    """rows and columns all different, between 0.3 and 1.7"""
    t = 0.3 + 1.4 * (np.arange(B * n_res, dtype=np.float64).reshape(B, n_res) * 7 % (B * n_res)) / (B * n_res - 1)
    return t.astype(np.float32)


def unet_ref_scaled(b, table, dtype=torch.float64):
    """block_refs.unet over the case of build_unet(mode='control') with residual n of sample j weighted table[j, n]: the
    formula h + s r is the plain walk over the residuals s r"""
    i = b.inputs
    x = BR.nchw(i["x"].to(dtype))
    p = BR.P(BR._sd(b, "net"), dtype=dtype)
    tab = torch.from_numpy(np.asarray(table, dtype=np.float64)).to(dtype)
    ctrl = [BR.nchw(i[f"c{n}"].to(dtype)) * tab[:, n].reshape(-1, 1, 1, 1) for n in range(tab.shape[1])]
    return BR.nhwc(BR.unet(b.mods["net"], p, x, i["t"], [(p, i["ctx"].to(dtype), 1.0)], 8, ctrl, 0, None))
