"""GPU (-m gpu): the two guidance-rescale kernels on the card through lib.hip.ops -- pfd_guidance_rescale_f32 against the fp64
specification within the derived bound (tests/guidance_refs.py), its invariances bit for bit, and pfd_cfg_step_mul with
factors of one against each of the five step entry points it stands for."""
import numpy as np
import pytest
import torch

import guidance_refs as R
import step_bits_refs as S
from lib import guidance as G

pytestmark = pytest.mark.gpu

T = torch.from_numpy
GRID = [(shape, B) for shape in R.SHAPES for B in R.BATCHES] + [(R.LONGEST, 1)]


def _mul(eps, s, phi, offset=0):
    """ops.guidance_rescale on numpy inputs; offset: eps starts that many halves behind a 16-byte boundary"""
    from lib.hip import ops
    buf = torch.empty(eps.size + 8, dtype=torch.float16, device='cuda')
    e = buf[offset:offset + eps.size].view(*eps.shape)
    e.copy_(T(eps))
    assert e.is_contiguous() and e.data_ptr() % 16 == 2 * offset
    out = ops.guidance_rescale(e, T(np.asarray(s, dtype=np.float32)).cuda(), T(np.asarray(phi, dtype=np.float32)).cuda())
    torch.cuda.synchronize()
    return out.cpu().numpy()


@pytest.fixture(scope="module")
def grid():
    """every (shape, B) of the grid once: (eps, scale, phi, mul)"""
    out = {}
    for shape, B in GRID:
        eps, s, phi = R.make_eps(B, shape), R.rows(R.SCALES, B), R.rows(R.PHIS, B)
        out[shape, B] = (eps, s, phi, _mul(eps, s, phi))
    return out


@pytest.mark.parametrize("shape,B", GRID, ids=[f"{'x'.join(map(str, s))}-B{b}" for s, b in GRID])
def test_statistics_kernel_meets_the_specification_within_the_derived_bound(grid, shape, B):
    eps, s, phi, mul = grid[shape, B]
    e = R.rel_err(mul, G.factor(eps, s, phi))
    print(f"[guidance] {shape} B {B}: |mul - f| / f = {e / 2.0 ** -24:.2f} x 2^-24, bound {R.bound(shape) / 2.0 ** -24:.0f} x 2^-24")
    assert e <= R.bound(shape)


def test_alignment_and_company_do_not_change_the_bits(grid):
    for shape in R.SHAPES:
        eps, s, phi, mul = grid[shape, 3]
        assert np.array_equal(_mul(eps, s, phi, offset=1).view(np.uint32), mul.view(np.uint32)), shape
        for b in range(3):
            alone = _mul(eps[[b, 3 + b]], s[b:b + 1], phi[b:b + 1])
            assert alone.view(np.uint32)[0] == mul.view(np.uint32)[b], (shape, b)


def test_phi_0_constant_eps_and_a_scale_view():
    from lib.hip import ops
    eps = R.make_eps(3, (4, 8, 8))
    s = R.rows(R.SCALES, 3)
    nan = eps.copy()
    nan[[1, 4]] = np.nan
    mul = _mul(nan, s, [0.7, 0.0, 1.0])
    assert mul[1] == np.float32(1.0) and np.all(np.isfinite(mul))
    assert mul.view(np.uint32)[0] == _mul(eps, s, [0.7, 0.0, 1.0]).view(np.uint32)[0]
    assert np.array_equal(_mul(np.full((4, 8, 8, 4), 0.375, dtype=np.float16), s[:2], [0.7, 0.25]), np.ones(2, dtype=np.float32))
    # the scale as the sampler hands it over: one element of a coefficient row (stride 0), or a column of a table (stride 13)
    e, phi = T(eps).cuda(), T(R.rows(R.PHIS, 3)).cuda()
    row = torch.tensor([0.1, 0.2, 0.3, 0.4, 7.5], device='cuda')
    tab = torch.full((3, 13), float('nan'), device='cuda')
    tab[:, 0] = T(s).cuda()
    one = ops.guidance_rescale(e, row[4:5], phi).cpu().numpy()
    col = ops.guidance_rescale(e, tab[:, 0], phi).cpu().numpy()
    assert R.rel_err(one, G.factor(eps, 7.5, R.rows(R.PHIS, 3))) <= R.bound((4, 8, 8))
    assert np.array_equal(col.view(np.uint32), _mul(eps, s, R.rows(R.PHIS, 3)).view(np.uint32))


def _run(c, eps_mul):
    """a case of the step fixture through the ops wrapper of its entry point, with or without eps_mul"""
    from lib.hip import ops

    def dev(a):
        return None if a is None else T(np.array(a)).cuda()
    how = {} if eps_mul is None else {'eps_mul': eps_mul}
    x, eps, coef, scale, keys = dev(c['x']), dev(c['eps']), dev(c['coef']), dev(c['scale']), dev(c['keys'])
    if c['entry'] == 'masked':
        out = ops.cfg_step_masked(eps, c['nb'], x, coef, solver=c['solver'], x0_prev=dev(c['x0_prev']), keep_key=keys,
                                  step=c['step'], x0_keep=dev(c['x0_keep']), mask=dev(c['mask']), ksq=c['ksq'], ks=c['ks'],
                                  noise_mul=c['noise_mul'], scale=scale, want_next=True, rep=c['rep'], **how)
    elif c['entry'] == 'dpmpp':
        out = ops.cfg_dpmpp_step(eps, c['nb'], x, coef, x0_prev=dev(c['x0_prev']), want_next=True, rep=c['rep'], scale=scale, **how)
    else:
        out = ops.cfg_ddim_step(eps, c['nb'], x, coef, noise=dev(c['noise']), want_next=True, rep=c['rep'], noise_key=keys,
                                step=c['step'] if keys is not None else None, noise_mul=c['noise_mul'], scale=scale, **how)
    torch.cuda.synchronize()
    return out


def test_step_mul_with_ones_is_each_of_the_five_entry_points():
    """every nb = 2 form of every entry point on the 16-byte and on the scalar shape (the seeded ones included: the same kernel
    on the same card draws the same noise); factors below one move the result"""
    _, cases = S.load()
    seen = set()
    for c in cases:
        if c['nb'] != 2 or c['offset'] != 0 or c['shape'] not in ([2, 4, 8, 8], [2, 3, 3, 5]):
            continue
        B = c['shape'][0]
        plain = _run(c, None)
        ones = _run(c, torch.ones(B, device='cuda'))
        for a, b in zip(plain, ones):
            assert torch.equal(a, b), c['name']
        low = _run(c, torch.tensor([0.57, 0.97], device='cuda'))
        assert not torch.equal(low[0], plain[0]) and not torch.equal(low[1], plain[1]) and bool(torch.isfinite(low[0]).all())
        seen.add(c['entry'])
    assert seen == set(S.ENTRY_POINTS)


def test_bad_arguments_are_codes_and_nothing_runs():
    from lib.hip import binding, ops
    lib = ops._lib()
    eps = T(R.make_eps(2, (4, 8, 8))).cuda()
    s, phi, mul = torch.ones(2, device='cuda'), torch.ones(2, device='cuda'), torch.full((2,), -7.0, device='cuda')
    p = lambda t: t.data_ptr()      # noqa: E731
    n = 256
    for args in ((None, p(s), 1, p(phi), 1, p(mul), 2, n), (p(eps), None, 1, p(phi), 1, p(mul), 2, n),
                 (p(eps), p(s), 1, None, 1, p(mul), 2, n), (p(eps), p(s), 1, p(phi), 1, None, 2, n),
                 (p(eps), p(s), 1, p(phi), 1, p(mul), 0, n), (p(eps), p(s), 1, p(phi), 1, p(mul), 2, 0),
                 (p(eps), p(s), -1, p(phi), 1, p(mul), 2, n), (p(eps), p(s), 1, p(phi), -1, p(mul), 2, n)):
        assert lib.pfd_guidance_rescale_f32(*args, None) == binding.PFD_EINVAL, args
    torch.cuda.synchronize()
    assert mul.tolist() == [-7.0, -7.0]
    x = torch.zeros(2, 4, 8, 8, device='cuda')
    coef = torch.tensor([0.5, 0.6, 0.0, 0.7, 2.0], device='cuda')
    with pytest.raises(ValueError, match="nb must be 2"):
        ops.cfg_ddim_step(eps[:2], 1, x, coef, eps_mul=torch.ones(2, device='cuda'))
    with pytest.raises(ValueError, match="eps_mul"):
        ops.cfg_ddim_step(eps, 2, x, coef, eps_mul=torch.ones(3, device='cuda'))
    xo, po = torch.empty_like(x), torch.empty_like(x)
    common = (p(eps), 2, p(x), 0, None, None, None, 0, 1.0, p(coef), None)
    tail = (None, None, 0, 1.0, 0.0, p(xo), p(po), None, 1, 2, 4, 8, 8, None)
    assert lib.pfd_cfg_step_mul(*common, None, *tail) == binding.PFD_EINVAL                      # no factors
    assert lib.pfd_cfg_step_mul(p(eps), 1, *common[2:], p(mul), *tail) == binding.PFD_EINVAL     # no unconditional half
    assert lib.pfd_cfg_step_mul(*common, p(mul), p(x), *tail[1:]) == binding.PFD_EINVAL          # x0_keep without a mask
