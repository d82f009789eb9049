"""GPU (-m gpu): the seeded counter-based noise of the stochastic DDIM step on the device -- the generator against
lib/noise.py (the specification in fp64), the fused step against the two-launch form and the closed formula, the
sampler graphed vs eager at eta > 0, and the independence of a sample's trajectory from the batch it rides in."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

T = torch.from_numpy
SEEDS = (0, -1, (1 << 40) + 12345)


def close(a, ref, tol):
    """tests/test_hip_kernels.py::close"""
    e = float((a.float().cpu() - ref.float().cpu()).abs().max() / max(1.0, float(ref.abs().max())))
    assert e <= tol, e
    return e


def _keys(rows):
    return torch.tensor(rows, dtype=torch.int64)


def _host_normal(rows, step, n):
    from lib import noise
    return T(np.stack([noise.normal(s, j, step, n) for s, j in rows]))


# ---- the generator ---------------------------------------------------------------------------------------------------
# 1e-5 absolute: u and v are exact in fp32, rad <= 5.77, and a few ulp each of logf, sqrtf, cospif / sinpif and the
# product come to about 2.5e-6 at the top of the range (naive fp32 numpy Box-Muller sits 1.8e-6 from fp64); one wrong
# bit anywhere in the Philox rounds gives O(1).  Measured maxima: profiles/device_noise.md.
@pytest.mark.parametrize("step", [0, 49])
@pytest.mark.parametrize("n", [4, 7, 256, 4100])
def test_generator_matches_the_host_specification(n, step):
    from lib.hip import ops
    rows = [(s, j) for s, j in zip(SEEDS, (3, 1, 0x1_0000_0002))]
    got = ops.philox_normal(_keys(rows).cuda(), step, n)
    assert got.shape == (3, n) and got.dtype == torch.float32
    d = float((got.cpu().double() - _host_normal(rows, step, n).double()).abs().max())
    print(f"[device_noise] generator B=3 n={n} step={step}: max|diff| {d:.3e}")
    assert d <= 1e-5


def test_generator_grid_stride_loop():
    """2^22 + 4 elements = 2^20 + 1 quads: one more than the 4096 x 256 threads of the largest grid"""
    from lib.hip import ops
    n = (1 << 22) + 4
    rows = [((1 << 40) + 12345, 5)]
    got = ops.philox_normal(_keys(rows).cuda(), 49, n)
    d = float((got.cpu().double() - _host_normal(rows, 49, n).double()).abs().max())
    print(f"[device_noise] generator B=1 n=2^22+4 step=49: max|diff| {d:.3e}")
    assert d <= 1e-5


def test_rows_are_independent():
    from lib.hip import ops
    rows = [(0, 3), (-1, 1), ((1 << 40) + 12345, 2), (20, 0)]
    base = ops.philox_normal(_keys(rows).cuda(), 7, 4100)
    perm = [2, 0, 3, 1]
    assert torch.equal(ops.philox_normal(_keys([rows[i] for i in perm]).cuda(), 7, 4100), base[perm])
    for changed in ((0, 4), (1, 3)):       # another sample_id, another seed in row 1
        rows2 = list(rows)
        rows2[1] = changed
        other = ops.philox_normal(_keys(rows2).cuda(), 7, 4100)
        assert not torch.equal(other[1], base[1])
        assert torch.equal(other[[0, 2, 3]], base[[0, 2, 3]])
    # an odd sample length (scalar stores): the same values
    assert torch.equal(ops.philox_normal(_keys(rows).cuda(), 7, 4099), base[:, :4099])


# ---- the fused step --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rep", [1, 2])
@pytest.mark.parametrize("nb", [1, 2])
@pytest.mark.parametrize("shape", [(2, 4, 8, 8), (1, 4, 3, 5)])
def test_fused_step_matches_two_launches_and_the_formula(shape, nb, rep):
    from lib.hip import ops
    B, C, h, w = shape
    g = torch.Generator().manual_seed(B * 100 + w)
    eps = torch.randn((nb * B, h, w, C), generator=g).half().cuda()
    x = torch.randn(shape, generator=g).cuda()
    rows = [(-1, 1), ((1 << 40) + 12345, 6)][:B]
    key = _keys(rows)
    a_t, a_prev, sig, scale = 0.4, 0.6, 0.1, 2.0
    coef = torch.tensor([a_t, a_prev, sig, math.sqrt(1 - a_t), scale], device='cuda')
    xp, p0, xin = ops.cfg_ddim_step(eps, nb, x, coef, noise_key=key.cuda(), step=7, noise_mul=0.5, rep=rep)
    # (a) the generator launch + the noise-tensor kernel
    z = ops.philox_normal(key.cuda(), 7, C * h * w).reshape(shape)
    xp2, p02, xin2 = ops.cfg_ddim_step(eps, nb, x, coef, noise=0.5 * z, rep=rep)
    close(xp, xp2, 1e-5)
    close(p0, p02, 1e-5)
    close(xin, xin2, 2e-3)
    # (b) the closed formula fed the host specification
    zh = _host_normal(rows, 7, C * h * w).reshape(shape).cuda()
    e = eps.float().permute(0, 3, 1, 2)
    e = e[:B] + scale * (e[B:] - e[:B]) if nb == 2 else e * scale
    r0 = (x - math.sqrt(1 - a_t) * e) / math.sqrt(a_t)
    rp = math.sqrt(a_prev) * r0 + math.sqrt(1 - a_prev - sig ** 2) * e + sig * 0.5 * zh
    close(p0, r0, 1e-5)
    close(xp, rp, 1e-5)
    assert xin.shape == (rep * B, h, w, C)
    for r in range(rep):
        close(xin[r * B:(r + 1) * B].permute(0, 3, 1, 2), rp, 2e-3)
    # a key on the host is accepted (copied); noise and noise_key together are refused
    xp3, _, _ = ops.cfg_ddim_step(eps, nb, x, coef, noise_key=key, step=7, noise_mul=0.5, rep=rep)
    assert torch.equal(xp3, xp)
    with pytest.raises(ValueError):
        ops.cfg_ddim_step(eps, nb, x, coef, noise=z, noise_key=key.cuda(), step=7)


def test_missing_key_is_einval():
    from lib.hip import binding
    lib = binding.load()
    x = torch.zeros(1, 4, 8, 8, device='cuda')
    eps = torch.zeros(1, 8, 8, 4, device='cuda', dtype=torch.float16)
    coef = torch.ones(5, device='cuda')
    rc = lib.pfd_cfg_ddim_step_rng(eps.data_ptr(), 1, x.data_ptr(), None, 0, 1.0, coef.data_ptr(), x.data_ptr(),
                                   x.data_ptr(), None, 1, 1, 4, 8, 8, None)
    assert rc == binding.PFD_EINVAL


# ---- the sampler -----------------------------------------------------------------------------------------------------
KEYS_A = [(20, 0), (20, 1)]
KEYS_B = [(-7, 0), ((1 << 40) + 12345, 3)]


def _sample(net, golden, sampler, keys, eta=0.5, xT=None, **kw):
    n = len(keys) if keys is not None else 2
    if xT is None:
        xT = torch.randn([n, 4, 8, 8], generator=torch.Generator().manual_seed(1))
    c = T(golden["see.ctx"]).cuda().half().repeat(n, 1, 1)
    x_info = {'type': 'image', 'xt': xT.cuda()}
    if keys is not None:
        x_info['noise_key'] = _keys(keys)            # on the host: the sampler moves it
    c_info = {'type': 'image', 'conditioning': c, 'unconditional_conditioning': torch.zeros_like(c),
              'unconditional_guidance_scale': 2.0}
    return sampler.sample(steps=4, shape=[n, 4, 8, 8], x_info=x_info, c_info=c_info, eta=eta, verbose=False, **kw)


def test_stochastic_schedule_replays_as_one_graph(net, golden):
    """the shape of test_hip_parity.py::test_hipgraph_replay_matches_eager at eta = 0.5: the captured trajectory gives
    the eager result and follows a new key tensor on replay"""
    from lib.model_zoo.ddim import DDIMSampler
    eager, graphed = DDIMSampler(net), DDIMSampler(net)
    graphed.enable_graph(True)
    res = []
    for keys in (KEYS_A, KEYS_B, KEYS_A):
        xe, ie = _sample(net, golden, eager, keys)
        xg, ig = _sample(net, golden, graphed, keys)
        assert torch.equal(xe, xg), keys
        assert len(ie['pred_x0']) == len(ig['pred_x0']) and torch.equal(ie['pred_x0'][-1], ig['pred_x0'][-1])
        res.append(xe.float())
    assert len(graphed._graphs) == 1
    assert torch.equal(res[0], res[2])
    assert float((res[0] - res[1]).abs().max()) > 1e-2                 # other keys, other noise
    x0, _ = _sample(net, golden, eager, KEYS_A, eta=0.)
    assert float((res[0] - x0.float()).abs().max()) > 1e-2             # eta = 0.5 is not eta = 0
    with pytest.raises(ValueError):
        _sample(net, golden, eager, KEYS_A, noise_dropout=0.1)


def test_per_step_api_takes_the_key(net, golden):
    """p_sample_ddim with x_info['noise_key']: deterministic, and the noise it adds is sigma * z(key, index)"""
    from lib.model_zoo.ddim import DDIMSampler
    s = DDIMSampler(net)
    s.make_schedule(ddim_num_steps=4, ddim_eta=0.5, verbose=False)
    c = T(golden["see.ctx"]).cuda().half().repeat(2, 1, 1)
    x = torch.randn([2, 4, 8, 8], generator=torch.Generator().manual_seed(1)).cuda()
    t = torch.full((2,), int(s.ddim_timesteps[2]), device='cuda', dtype=torch.long)

    def step(keys):
        x_info = {'type': 'image', 'x': x.clone()}
        if keys is not None:
            x_info['noise_key'] = _keys(keys)
        c_info = {'type': 'image', 'conditioning': c, 'unconditional_conditioning': torch.zeros_like(c),
                  'unconditional_guidance_scale': 2.0}
        return s.p_sample_ddim(x_info, c_info, t, 2)[0]

    a, b = step(KEYS_A), step(KEYS_A)
    assert torch.equal(a, b)
    sig = float(s.ddim_sigmas[2])
    assert sig > 0
    # x_prev(keys A) - x_prev(keys B) = sigma * (z_A - z_B): everything else in the step is the same
    zA = _host_normal(KEYS_A, 2, 256).reshape(2, 4, 8, 8)
    zB = _host_normal(KEYS_B, 2, 256).reshape(2, 4, 8, 8)
    d = (a - step(KEYS_B)).double().cpu()
    # each x_prev rounds its last add once (half an ulp of |x_prev|, twice) and each z is within 1e-5 of the host's
    lim = 2 * 2.0 ** -24 * float(a.abs().max()) + sig * 2e-5
    err = float((d - sig * (zA - zB).double()).abs().max())
    print(f"[device_noise] per-step API: |(x_A - x_B) - sigma (z_A - z_B)| max {err:.2e} (limit {lim:.2e})")
    assert err <= lim


def test_a_sample_does_not_depend_on_its_company(net, golden):
    """sample key K alone, then as row 0 and as row 1 of a batch of two beside another key, from the same x_T row: the
    same trajectory up to the tile choice of another batch size (the bound of
    test_hip_parity.py::test_cfg_prefix_sharing_matches_doubled_batch)"""
    from lib.model_zoo.ddim import DDIMSampler
    K, other = (20, 1), (-3, 0)
    g = torch.Generator().manual_seed(5)
    xK, xO = torch.randn([1, 4, 8, 8], generator=g), torch.randn([1, 4, 8, 8], generator=g)
    s = DDIMSampler(net)
    alone = _sample(net, golden, s, [K], xT=xK)[0].float()
    row0 = _sample(net, golden, s, [K, other], xT=torch.cat([xK, xO]))[0].float()
    row1 = _sample(net, golden, s, [other, K], xT=torch.cat([xO, xK]))[0].float()
    lim = 4e-3 * max(1.0, float(alone.abs().max()))
    for name, got in (("row 0", row0[0:1]), ("row 1", row1[1:2])):
        d = float((got - alone).abs().max())
        print(f"[device_noise] company invariance, {name} of 2 vs alone: max|diff| {d:.2e} (limit {lim:.2e})")
        assert d <= lim
    assert float((row0[1:2] - alone).abs().max()) > 1e-2               # the neighbour is another sample


# ---- the pipeline ----------------------------------------------------------------------------------------------------
def test_pipeline_device_noise_is_seeded_and_the_old_path_is_untouched(net, golden, monkeypatch):
    from lib.hip import binding, ops
    from lib.pipeline import PromptFreePipeline
    img = T(golden["see.img"])
    pipe = PromptFreePipeline(net)

    def gen(seed, **kw):
        return pipe.generate(img, 2, 64, 64, steps=4, scale=2.0, eta=0.5, seed=seed, decode=False, **kw)[0].float()

    a, b, c = gen(5, device_noise=True), gen(5, device_noise=True), gen(6, device_noise=True)
    assert torch.equal(a, b)
    assert float((a - c).abs().max()) > 1e-2
    # it does not touch the global generator
    torch.manual_seed(1)
    before = torch.cuda.get_rng_state().clone()
    gen(5, device_noise=True)
    assert torch.equal(torch.cuda.get_rng_state(), before)
    # graphed == eager through the pipeline too
    graphed = PromptFreePipeline(net)
    graphed.enable_graph(True)
    xg = graphed.generate(img, 2, 64, 64, steps=4, scale=2.0, eta=0.5, seed=5, decode=False, device_noise=True)[0]
    assert torch.equal(xg.float(), a) and len(graphed.sampler._graphs) == 1

    # device_noise=False: the step is the parent commit's -- pfd_cfg_ddim_step fed one torch.randn draw of the global
    # generator per step.  Run it as it is, then with cfg_ddim_step replaced by the parent's wrapper (which knows no
    # key) recording the noise it is handed: the same bits, and the noise is the generator's stream under that seed.
    torch.manual_seed(77)
    old = gen(5)
    assert float((old - a).abs().max()) > 1e-2
    seen = []

    def parent_cfg_ddim_step(eps, nb, x, coef, *, noise=None, want_next=True, rep=None):
        B, Cc, h, w = x.shape
        rep = nb if rep is None else rep
        x_prev, pred_x0 = torch.empty_like(x), torch.empty_like(x)
        xin = torch.empty((rep * B, h, w, Cc), dtype=torch.float16, device=x.device) if want_next else None
        rc = binding.load().pfd_cfg_ddim_step(eps.data_ptr(), nb, x.data_ptr(), noise.data_ptr(), coef.data_ptr(),
                                              x_prev.data_ptr(), pred_x0.data_ptr(),
                                              None if xin is None else xin.data_ptr(), rep, B, Cc, h, w,
                                              torch.cuda.current_stream().cuda_stream)
        binding.check(rc, "pfd_cfg_ddim_step")
        seen.append(noise.clone())
        return x_prev, pred_x0, xin

    monkeypatch.setattr(ops, "cfg_ddim_step", parent_cfg_ddim_step)
    torch.manual_seed(77)
    again = gen(5)
    monkeypatch.undo()
    assert torch.equal(again, old)
    torch.manual_seed(77)
    assert len(seen) == 4
    for nz in seen:
        assert torch.equal(nz, torch.randn_like(nz))
