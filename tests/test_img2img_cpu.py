"""CPU: the seeded img2img start -- the stream word of lib/noise.py, lib/img2img.py (the specification of csrc/latent.hip)
and its mutants against the GPU test's tolerance, the kernel on the CPU emulation, the C ABI's argument checks, the
sampler's shortened run over tests/sampler_standin.py, and the pipeline / server layers over the stubs of the other CPU
tests with a stand-in for ops.latent_start built on lib/img2img.py."""
import ctypes
import os
import re
import subprocess
import sys
import threading

import numpy as np
import pytest
import torch

import img2img_refs as R
import sampler_standin as SS
from lib import solver as _solver
from lib.model_zoo.diffusion_utils import make_ddim_sampling_parameters, make_ddim_timesteps

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get("EMU_CXX", "/opt/rocm/lib/llvm/bin/clang++")


# ---- the stream word -------------------------------------------------------------------------------------------------
def test_stream_0_is_the_step_noise_bit_for_bit_and_the_streams_differ():
    from lib import noise
    for seed, sid, step in ((20, 3, 49), (-1, 0, 0), ((1 << 40) + 12345, 0x1_0000_0002, 7)):
        base = noise.normal(seed, sid, step, 4099)
        assert np.array_equal(noise.normal(seed, sid, step, 4099, stream=0), base)
        s1, s2 = noise.normal(seed, sid, step, 4099, stream=1), noise.normal(seed, sid, step, 4099, stream=2)
        for a, b in ((s1, base), (s2, base), (s1, s2)):
            assert a.dtype == np.float32 and np.abs(a - b).max() > 0.1
            assert abs(float(np.corrcoef(a, b)[0, 1])) < 0.08          # five standard errors of 4099 independent pairs
    # the word is the counter's fourth: Philox itself says so
    want = noise.philox4x32_10(np.array([5, 0, 3, 2], dtype=np.uint32), np.array(noise.key_words(20), dtype=np.uint32))
    u = ((int(want[0]) >> 8) + 1) * 2.0 ** -24
    v = (int(want[1]) >> 8) * 2.0 ** -24
    z = np.sqrt(-2 * np.log(u)) * np.cos(2 * np.pi * v)
    assert np.float32(z) == noise.normal(20, 3, 0, 24, stream=2)[20]


def test_start_steps():
    from lib.img2img import start_steps
    assert start_steps(50, 1.0) == 50 and start_steps(50, 0.5) == 25 and start_steps(8, 0.75) == 6
    for steps, strength in ((50, 0.01), (50, 0), (50, 1.01), (50, float('nan')), (50, -0.5), (50, 'much')):
        with pytest.raises(ValueError):
            start_steps(steps, strength)


def test_level_is_that_of_the_first_timestep_evaluated():
    from lib.img2img import kernel_scalars, level
    acp = SS.StubModel().alphas_cumprod.numpy()
    ts = make_ddim_timesteps("uniform", 8, 1000, verbose=False)
    assert level(acp, ts, 6) == float(acp[ts[5]]) and level(acp, ts, 8) == float(acp[ts[7]])
    for k in (0, 9):
        with pytest.raises(ValueError):
            level(acp, ts, k)
    sf, sa, sb = kernel_scalars(0.18215, 0.4375)
    assert sf.dtype == np.float32 and sa == np.float32(np.sqrt(0.4375)) and sb == np.float32(0.75)


# ---- the specification and its neighbours ----------------------------------------------------------------------------
def _inputs():
    """every (name, moments, keys, posterior) the GPU test judges the kernel on"""
    for shape in R.SHAPES:
        for Bm in sorted({1, shape[0]}):
            for post in ('sample', 'mode'):
                yield f"{shape} Bm={Bm} {post}", R.moments(shape, Bm), R.keys(shape[0]), post
    yield "clamp", R.moments(R.SHAPES[0], R.SHAPES[0][0], 'clamp'), R.keys(R.SHAPES[0][0]), 'sample'


def test_specification_on_the_gpu_tests_inputs():
    from lib import noise
    for name, m, k, post in _inputs():
        x0, xt = R.reference(m, k, post)
        B, C = k.shape[0], m.shape[3] // 2
        assert x0.shape == xt.shape == (B, C) + m.shape[1:3] and x0.dtype == xt.dtype == np.float32
        # written out once more, element by element, for sample B - 1
        b, mb = B - 1, R.nchw(m)[(B - 1) if m.shape[0] > 1 else 0]
        zq = noise.normal64(int(k[b, 0]), int(k[b, 1]), 0, x0[b].size, stream=1).reshape(x0[b].shape)
        zp = noise.normal64(int(k[b, 0]), int(k[b, 1]), 0, x0[b].size, stream=2).reshape(x0[b].shape)
        sf = float(np.float32(R.SCALE_FACTOR))
        want0 = sf * (mb[:C] + (np.exp(0.5 * np.clip(mb[C:], -30, 20)) * zp if post == 'sample' else 0.0))
        wantt = float(np.float32(np.sqrt(R.A_T))) * want0 + float(np.float32(np.sqrt(1 - R.A_T))) * zq
        assert np.array_equal(x0[b], want0.astype(np.float32)) and np.array_equal(xt[b], wantt.astype(np.float32)), name
    # a shared picture is the same picture for every sample: rows of equal keys are equal
    m = R.moments((2, 4, 8, 8), 1)
    x0, xt = R.reference(m, np.array([[5, 1], [5, 1]]))
    assert np.array_equal(x0[0], x0[1]) and np.array_equal(xt[0], xt[1])


def test_every_mutant_leaves_the_gpu_tests_tolerance():
    """the tolerance of tests/test_img2img_gpu.py tells lib/img2img.py from each of its named neighbours on that test's
    own inputs: every mutant that touches the posterior draw under 'sample', those that touch x_t alone under 'mode'
    too, and 'no_clamp' on the input that reaches the clamps (it is the specification where no logvar does)"""
    from lib.img2img import MUTANTS
    assert set(MUTANTS) == {'streams_swapped', 'stream0', 'no_clamp', 'logvar_as_std', 'level_of_k', 'unscaled'}
    moved = {w: 0 for w in MUTANTS}
    for name, m, k, post in _inputs():
        x0, xt = R.reference(m, k, post)
        for w in MUTANTS:
            w0, wt = R.reference(m, k, post, wrong=w)
            e = max(R.scaled_err(w0, x0), R.scaled_err(wt, xt))
            if w == 'no_clamp':
                assert (e > 1e3 * R.TOL) == (name == 'clamp'), (name, e)
            elif post == 'mode' and w == 'logvar_as_std':
                assert e == 0.0                                       # the mode has no std
            else:
                assert e > 1e3 * R.TOL, (name, w, e)
            moved[w] += e > 1e3 * R.TOL
    assert all(moved.values()), moved
    with pytest.raises(ValueError):
        R.reference(m, k, 'sample', wrong='something_else')
    with pytest.raises(ValueError):
        R.reference(m, k, 'median')


# ---- the kernel on the CPU emulation ---------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu_latent(tmp_path_factory):
    if not os.path.exists(CXX):
        pytest.skip("clang++ of the ROCm toolchain not available")
    out = str(tmp_path_factory.mktemp("pfd_cpu_emu_latent"))
    subprocess.run([sys.executable, os.path.join(REPO, "tools", "cpu_emu", "build.py"), out], check=True,
                   stdout=subprocess.DEVNULL, env=dict(os.environ, EMU_ONLY="emu_latent", EMU_OPT="-O1"))
    return os.path.join(out, "emu_latent")


def _emu_case(tmp, i, shape, m, k, post, offset=0, want_x0=1):
    from lib.img2img import kernel_scalars
    path = os.path.join(tmp, f"case{i}.bin")
    with open(path, "wb") as f:
        f.write(np.ascontiguousarray(k, dtype=np.int64).tobytes() + np.ascontiguousarray(m, dtype=np.float16).tobytes())
    B, C, h, w = shape
    sf, sa, sb = (float(v).hex() for v in kernel_scalars(R.SCALE_FACTOR, R.A_T))
    return f"{B},{m.shape[0]},{C},{h},{w},{sf},{sa},{sb},{1.0 if post == 'sample' else 0.0},{offset},{want_x0},{path}", path


def test_kernel_on_the_emulation_matches_the_specification(emu_latent, tmp_path):
    """csrc/latent.hip compiled for the host: the GPU test's shapes, both Bm, both posteriors, the clamp input, the
    scalar path forced by a misaligned output, x0 left out, and one quad past the grid -- return code, one launch, guard
    bands, and the values against lib/img2img.py at the GPU test's tolerance ('mode' x0: bit for bit)"""
    cases = []
    for shape in R.SHAPES:
        for Bm in sorted({1, shape[0]}):
            for post in ('sample', 'mode'):
                cases.append((shape, R.moments(shape, Bm), R.keys(shape[0]), post, 0, 1))
    s0 = R.SHAPES[0]
    cases.append((s0, R.moments(s0, s0[0], 'clamp'), R.keys(s0[0]), 'sample', 0, 1))
    cases.append((s0, R.moments(s0, s0[0]), R.keys(s0[0]), 'sample', 1, 1))          # misaligned: scalar stores
    cases.append((s0, R.moments(s0, 1), R.keys(s0[0]), 'sample', 0, 0))              # x0 == NULL
    cases.append((R.PAST_THE_GRID, R.moments(R.PAST_THE_GRID, 1), R.keys(1), 'sample', 0, 1))
    args, paths = zip(*[_emu_case(str(tmp_path), i, c[0], c[1], c[2], c[3], c[4], c[5]) for i, c in enumerate(cases)])
    r = subprocess.run([emu_latent, *args], capture_output=True, text=True, timeout=600)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith(("ok", "FAIL"))]
    assert r.returncode == 0 and len(lines) == len(cases) and all(ln.startswith("ok") for ln in lines), r.stdout[-3000:] + r.stderr[-1000:]
    for (shape, m, k, post, offset, want_x0), path, line in zip(cases, paths, lines):
        vec = offset == 0 and (shape[1] * shape[2] * shape[3]) % 4 == 0
        assert ("latent_start_kernel<true>" in line) == vec, line
        x0, xt = R.reference(m, k, post)
        got = np.fromfile(path + ".xt", dtype=np.float32).reshape(xt.shape)
        e = R.scaled_err(got, xt)
        print(f"[img2img emu] {shape} Bm={m.shape[0]} {post} offset={offset}: x_t err {e:.2e}")
        assert e <= R.TOL, (line, e)
        assert os.path.exists(path + ".x0") == bool(want_x0)
        if want_x0:
            got0 = np.fromfile(path + ".x0", dtype=np.float32).reshape(x0.shape)
            if post == 'mode':
                assert np.array_equal(got0, x0), line
            else:
                assert R.scaled_err(got0, x0) <= R.TOL, line


# ---- the C ABI --------------------------------------------------------------------------------------------------------
def test_header_declares_and_binding_lists_the_entry_point():
    from lib.hip import binding
    src = open(os.path.join(REPO, "include", "pfd_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+pfd_latent_start\s*\(([^)]*)\)\s*;", code)
    assert m and len(m.group(1).split(",")) == 14
    assert len(binding.SIGNATURES["pfd_latent_start"][1]) == 14
    for cite in ("distributions.py:24-62", "pfd.py:204-207", "ddim.py:213-219"):
        assert cite in src, cite
    assert re.search(r"#define\s+PFD_ABI_VERSION\s+10\b", src) and binding.ABI_VERSION == 10     # an added entry point
    mk = open(os.path.join(REPO, "prompt-free-diffusion_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\blatent\.hip\b", mk, flags=re.M)


def test_cabi_argument_checks_need_no_gpu():
    """every refusal happens before a launch and leaves a message behind"""
    from lib.hip import binding
    lib = binding.load()
    buf = ctypes.create_string_buffer(256)
    p = ctypes.cast(buf, ctypes.c_void_p)

    def call(moments=p, Bm=1, key=p, x0=p, xt=p, B=1, C=4, h=2, w=2):
        return lib.pfd_latent_start(moments, Bm, key, 0.18215, 0.5, 0.5, 1.0, x0, xt, B, C, h, w, None)

    for kw in (dict(moments=None), dict(key=None), dict(xt=None), dict(Bm=2, B=3), dict(Bm=0), dict(Bm=3, B=2),
               dict(B=0), dict(C=0), dict(h=-1), dict(w=0)):
        assert call(**kw) == binding.PFD_EINVAL, kw
        assert b"pfd_latent_start" in lib.pfd_last_error(), kw


def test_ops_wrapper_refuses_before_it_touches_a_device():
    from lib.hip import ops
    m = torch.zeros(1, 2, 2, 8, dtype=torch.float16)
    key = torch.zeros(2, 2, dtype=torch.int64)
    with pytest.raises(ValueError, match="posterior"):
        ops.latent_start(m, key, 0.18215, 0.5, posterior='median')
    with pytest.raises(ValueError, match="f16 NHWC"):
        ops.latent_start(m.float(), key, 0.18215, 0.5)
    with pytest.raises(ValueError, match="pictures for"):
        ops.latent_start(torch.zeros(3, 2, 2, 8, dtype=torch.float16), key, 0.18215, 0.5)
    with pytest.raises(ValueError, match="a_t"):
        ops.latent_start(m, key, 0.18215, 1.5)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.latent_start(m, key, 0.18215, 0.5)


# ---- the sampler's shortened run ---------------------------------------------------------------------------------------
def _plain_loop(case, model, x, k):
    """the k steps ddim_timesteps[:k], reversed, from x: the plain loop of tests/test_sampler_host_cpu.py"""
    import test_sampler_host_cpu as H
    _, c = SS.build_inputs(case)
    bs, dtype = SS.SHAPE[0], case['cdtype']
    acp = model.alphas_cumprod.float().numpy()
    ts = make_ddim_timesteps("uniform", case['steps'], 1000, verbose=False)
    sg, a, ap = make_ddim_sampling_parameters(acp, ts, case['eta'], verbose=False)
    order = _solver.solver_order(case['solver'])
    rows = None if order is None else _solver.dpmpp_2m_table(a, ap, 1.0, order)
    s1 = np.sqrt(1. - a)
    ts = ts[:k]
    nb, s, bias_u, bias_c = H._contexts(case, c, bs)
    hist = torch.zeros_like(x)
    for i in range(k):
        index, t = k - 1 - i, int(ts[k - 1 - i])
        eps_c = H._eps(x, t, bias_c, None)
        eps_u = H._eps(x, t, bias_u, None) if nb == 2 else torch.zeros_like(x)
        num = H._ddim_numbers(a[index], ap[index], sg[index], s1[index]) if order is None else \
            H._dpmpp_numbers(rows[index], first_order=i == 0 or index == 0)
        x, hist = H._step(x, eps_u, eps_c, s, num, torch.zeros_like(x), hist)
    return x.to(dtype)


@pytest.mark.parametrize("solver", ["ddim", "dpmpp_2m"])
@pytest.mark.parametrize("k", [1, 3, 4])
def test_xt_steps_runs_exactly_k_steps(solver, k, monkeypatch):
    from lib.model_zoo.ddim import DDIMSampler
    case = SS._case("xt_steps", start='xt', solver=solver)
    SS.install(monkeypatch)
    model = SS.StubModel()
    x_info, c = SS.build_inputs(case)
    x_info['xt_steps'] = k
    start = x_info['xt'].clone()
    x, inter = DDIMSampler(model).sample(case['steps'], SS.SHAPE, x_info, c, eta=0., verbose=False, solver=solver)
    ts = make_ddim_timesteps("uniform", case['steps'], 1000, verbose=False)
    calls = [ln for ln in SS.LOG if ln.startswith("apply_model_nhwc")]
    assert [int(re.search(r"t0=(\d+)", ln).group(1)) for ln in calls] == [int(t) for t in ts[:k][::-1]]
    emb = [ln for ln in SS.LOG if ln.startswith("emb_projections")]
    assert emb == [f"emb_projections t={[int(t) for t in ts[:k][::-1]]}"]
    steps = [ln for ln in SS.LOG if ln.startswith("cfg_")]
    assert len(steps) == k
    if solver == 'dpmpp_2m':      # the first step of the shortened run has no history; nor has the last of any run
        assert ["x0_prev=None" in ln for ln in steps] == [i == 0 or i == k - 1 for i in range(k)]
    assert torch.equal(x, _plain_loop(case, model, start.float(), k))
    assert not any(ln.startswith("q_sample") for ln in SS.LOG)


def test_xt_steps_serves_the_multicontext_loop_and_refuses_a_bad_k(monkeypatch):
    from lib.model_zoo.ddim import DDIMSampler
    SS.install(monkeypatch)
    model = SS.StubModel()
    case = SS._case("xt_steps_mc", 'mc', start='xt', scale=2.0)
    x_info, c = SS.build_inputs(case)
    x_info['xt_steps'] = 2
    DDIMSampler(model).sample_multicontext(4, SS.SHAPE, x_info, c, eta=0., verbose=False)
    ts = make_ddim_timesteps("uniform", 4, 1000, verbose=False)
    calls = [ln for ln in SS.LOG if ln.startswith("apply_model_nhwc")]
    assert [int(re.search(r"t0=(\d+)", ln).group(1)) for ln in calls] == [int(ts[1]), int(ts[0])]
    for bad in (0, 5, -1, 2.5):
        x_info, c = SS.build_inputs(SS._case("bad", start='xt'))
        x_info['xt_steps'] = bad
        with pytest.raises(ValueError, match="xt_steps"):
            DDIMSampler(model).sample(4, SS.SHAPE, x_info, c, eta=0., verbose=False)
    # without the key nothing changed: four steps
    del SS.LOG[:]
    x_info, c = SS.build_inputs(SS._case("plain", start='xt'))
    DDIMSampler(model).sample(4, SS.SHAPE, x_info, c, eta=0., verbose=False)
    assert len([ln for ln in SS.LOG if ln.startswith("cfg_")]) == 4


# ---- pipeline and server over the stubs --------------------------------------------------------------------------------
def _net():
    from stubs import StubNet

    class Net(StubNet):
        latent_scale_factor = {'image': R.SCALE_FACTOR}
        alphas_cumprod = SS.StubModel().alphas_cumprod
        encodes = 0

        def vae_encode_moments(self, x, which):
            """per-picture stand-in with the real shapes: f16 NHWC [1, H/8, W/8, 8]"""
            assert which == 'image' and tuple(x.shape[:2]) == (1, 3)
            Net.encodes += 1
            p = torch.nn.functional.avg_pool2d(x.float(), 8)                          # [1, 3, h, w]
            m = torch.cat([p * 4 - 2, p.flip(1) - 1.5, p[:, :1] * 3 - 3, p[:, 1:2] - 4], 1)      # 4 means, 4 logvars
            return m.permute(0, 2, 3, 1).contiguous().to(torch.float16)
    Net.encodes = 0
    return Net()


def _standin_latent_start(moments_nhwc, key, scale_factor, a_t, B=None, posterior='sample', want_x0=False):
    """ops.latent_start on the host: lib/img2img.py"""
    from lib import img2img
    x0, xt = img2img.latent_start_batch(R.nchw(moments_nhwc.numpy()), key.numpy(), scale_factor, a_t, posterior)
    return (torch.from_numpy(x0), torch.from_numpy(xt)) if want_x0 else torch.from_numpy(xt)


class _Sampler:
    def __init__(self):
        self.x_infos, self.steps = [], []

    def enable_graph(self, on=True):
        pass

    def sample(self, steps, shape, x_info, c_info, eta=0., verbose=True, **how):
        assert list(x_info['xt'].shape) == list(shape)
        self.x_infos.append(dict(x_info))
        self.steps.append(steps)
        return x_info['xt'], {}


def _picture(seed=0):
    return torch.from_numpy(R.picture_f32(64, 64, seed))


def test_generate_with_init_is_keyed_per_global_sample_whatever_the_world_size(monkeypatch):
    from lib import pipeline
    from lib.hip import ops
    from lib.img2img import level
    monkeypatch.setattr(ops, "latent_start", _standin_latent_start)
    img, init = torch.rand(1, 3, 64, 64), _picture()
    n_global, seed = 4, (1 << 35) + 9

    def run(rank, world, **kw):
        s = _Sampler()
        t = {}
        pipeline.PromptFreePipeline(_net(), rank=rank, world_size=world, sampler=s).generate(
            img, n_global, 64, 64, steps=8, seed=seed, timings=t, **kw)
        return s, t

    monkeypatch.setattr(pipeline, "shard_xT", lambda *a, **k: pytest.fail("an img2img request draws no x_T"))
    one, t_one = run(0, 1, init=init, strength=0.75)
    xi = one.x_infos[0]
    assert xi['xt_steps'] == 6 and one.steps == [8] and tuple(xi['xt'].shape) == (4, 4, 8, 8) and 'noise_key' not in xi
    assert 'init_encode_ms' in t_one and set(t_one) == {'ctx_encode_ms', 'ddim_loop_ms', 'vae_decode_ms', 'init_encode_ms'}
    halves = [run(r, 2, init=init, strength=0.75)[0] for r in range(2)]
    assert torch.equal(torch.cat([h.x_infos[0]['xt'] for h in halves]), xi['xt'])
    # ... and it is the host specification at the level of the first timestep evaluated, sample j keyed (seed, j)
    net = _net()
    ts = make_ddim_timesteps("uniform", 8, 1000, verbose=False)
    a_t = level(net.alphas_cumprod.numpy(), ts, 6)
    m = net.vae_encode_moments(init, 'image')
    want = _standin_latent_start(m, torch.tensor([[seed, j] for j in range(4)]), R.SCALE_FACTOR, a_t)
    assert torch.equal(xi['xt'], want) and a_t == float(net.alphas_cumprod[int(ts[5])])
    assert not torch.equal(xi['xt'][0], xi['xt'][1])
    mode = run(0, 1, init=init, strength=0.75, init_posterior='mode')[0].x_infos[0]['xt']
    assert not torch.equal(mode, xi['xt'])
    # device_noise rides along unchanged
    assert run(0, 1, init=init, strength=0.5, eta=0.5, device_noise=True)[0].x_infos[0]['noise_key'].tolist() == \
        [[seed, j] for j in range(4)]
    monkeypatch.undo()
    # without init: what it was -- x_T from the generator, no new timing, no 'xt_steps'
    plain, t_plain = run(0, 1)
    assert 'xt_steps' not in plain.x_infos[0] and set(t_plain) == {'ctx_encode_ms', 'ddim_loop_ms', 'vae_decode_ms'}
    assert torch.equal(plain.x_infos[0]['xt'], pipeline.shard_xT(n_global, 64, 64, seed, 0, 1))


def test_generate_validates_before_anything_touches_the_device():
    from lib.pipeline import PromptFreePipeline

    class Untouchable:
        device = 'cpu'

        def __getattr__(self, name):
            raise AssertionError(f"the model was touched ({name}) before the arguments were checked")

    pipe = PromptFreePipeline(Untouchable(), sampler=_Sampler())
    img, init = torch.rand(1, 3, 64, 64), _picture()
    for kw in (dict(strength=0), dict(strength=1.01), dict(strength=0.01), dict(init_posterior='median'),
               dict(init=torch.rand(1, 3, 32, 64)), dict(init=torch.zeros(1, 3, 64, 64, dtype=torch.int32)),
               dict(init=np.zeros((64, 64, 4), dtype=np.uint8)), dict(init=np.zeros((2000, 64, 3), dtype=np.uint8))):
        with pytest.raises(ValueError):
            pipe.generate(img, 2, 64, 64, steps=8, **dict(dict(init=init), **kw))


def _stub_server(monkeypatch, max_batch=4):
    """tests/test_device_noise_cpu.py::_server: the device work stubbed, `_generate` records its batches"""
    from lib import serving

    class _Pipe:
        def __init__(self, net):
            pass

        def enable_graph(self, on):
            pass

    monkeypatch.setattr(serving, "PromptFreePipeline", _Pipe)
    srv = serving.PromptFreeServer(object(), use_graph=False, max_batch=max_batch)
    calls = []

    def fake_generate(batch):
        calls.append([r.seed for r in batch])
        return [torch.full((r.n, 1), float(r.seed)) for r in batch]

    srv._generate = fake_generate
    return srv, calls


def _queued(srv, submits):
    gate = threading.Event()
    srv.call(lambda n: gate.wait(30))
    futs = [srv.submit(*a, **k) for a, k in submits]
    gate.set()
    return [f.result(30) for f in futs]


def test_batch_keys_with_and_without_init():
    from lib import serving
    img = torch.rand(1, 3, 64, 64)
    kw = dict(image=img, n=1, height=64, width=64, steps=8, scale=2.0, eta=0.0, seed=1)
    plain = serving._Request(**kw)
    # a request without init keeps the key it had
    assert plain.key() == (64, 64, 8, 2.0, 0.0, True, True, False, False)
    assert serving._Request(solver='dpmpp_2m', **kw).key() == plain.key() + ('dpmpp_2m',)
    assert serving._Request(mixed=True, **kw).key() == (64, 64, 8, False, 0.0, True, True, False, False)
    a = serving._Request(init=_picture(0), strength=0.75, init_k=6, **kw)
    b = serving._Request(init=_picture(1), strength=0.8, init_k=6, **dict(kw, seed=2))       # int(8 * 0.8) = 6 too
    c = serving._Request(init=_picture(0), strength=0.5, init_k=4, **kw)
    assert a.key() == plain.key() + (('init', 6),) == b.key() and c.key() != a.key() and a.key() != plain.key()
    assert serving._Request(init=_picture(0), init_k=6, solver='dpmpp_2m', **kw).key() == plain.key() + ('dpmpp_2m', ('init', 6))
    assert serving._Request(init=_picture(0), init_k=6, mixed=True, **kw).key()[-1] == ('init', 6)
    assert a.shareable() and plain.shareable()
    assert not serving._Request(init=_picture(0), init_k=6, **dict(kw, eta=0.5)).shareable()            # unchanged


def test_server_coalesces_img2img_requests_of_equal_k_only(monkeypatch):
    srv, calls = _stub_server(monkeypatch)
    img = torch.rand(1, 3, 64, 64)
    try:
        outs = _queued(srv, [((img, 1, 64, 64), dict(seed=1, steps=8, init=_picture(0), strength=0.75)),
                             ((img, 1, 64, 64), dict(seed=2, steps=8, init=_picture(1), strength=0.75)),
                             ((img, 1, 64, 64), dict(seed=3, steps=8, init=_picture(0), strength=0.5)),
                             ((img, 1, 64, 64), dict(seed=4, steps=8)),
                             ((img, 1, 64, 64), dict(seed=5, steps=8))])
        assert [float(o[0, 0]) for o in outs] == [1.0, 2.0, 3.0, 4.0, 5.0]
        assert calls == [[1, 2], [3], [4, 5]]
    finally:
        srv.close()


def test_submit_checks_on_the_callers_thread(monkeypatch):
    srv, calls = _stub_server(monkeypatch)
    img = torch.rand(1, 3, 64, 64)
    try:
        for kw in (dict(strength=0), dict(strength=1.5), dict(strength=0.01), dict(init=torch.rand(1, 3, 64, 32)),
                   dict(init=torch.rand(3, 64, 64)), dict(init=np.zeros((64, 64), dtype=np.uint8)),
                   dict(init=np.zeros((64 * 17, 64, 3), dtype=np.uint8))):
            with pytest.raises(ValueError):
                srv.submit(img, 1, 64, 64, steps=8, **dict(dict(init=_picture(), strength=0.75), **kw))
        # a uint8 picture of another size is accepted as it is: the worker resizes it
        r = srv.submit(img, 1, 64, 64, steps=8, seed=9, init=R.picture_u8(100, 80), strength=1.0).result(30)
        assert float(r[0, 0]) == 9.0 and calls == [[9]]
    finally:
        srv.close()


def test_server_generate_gives_each_request_its_own_picture_and_keys(monkeypatch):
    """the real `_generate` over the stubs: a coalesced batch starts every request where its solo run starts"""
    from lib import serving
    from lib.hip import ops
    monkeypatch.setattr(ops, "latent_start", _standin_latent_start)
    s = _Sampler()
    srv = serving.PromptFreeServer(_net(), use_graph=False, max_batch=8)
    try:
        srv.pipe.sampler = s
        img = torch.rand(1, 3, 64, 64)
        kw = dict(image=img, height=64, width=64, steps=8, scale=2.0, eta=0.0, as_uint8=False, future=None, strength=0.75,
                  init_k=6)
        reqs = [serving._Request(n=2, seed=-5, init=_picture(0), **kw), serving._Request(n=1, seed=1 << 40, init=_picture(1), **kw)]
        monkeypatch.setattr(serving, "shard_xT", lambda *a, **k: pytest.fail("an img2img request draws no x_T"))
        before = torch.get_rng_state().clone()
        outs = srv._generate(reqs)
        assert torch.equal(torch.get_rng_state(), before) and [o.shape[0] for o in outs] == [2, 1]
        both = s.x_infos[-1]
        assert both['xt_steps'] == 6 and tuple(both['xt'].shape) == (3, 4, 8, 8) and srv.batches == [3]
        solo = [srv._generate([r]) and s.x_infos[-1]['xt'] for r in reqs]
        assert torch.equal(both['xt'], torch.cat(solo))
        for r, rows in zip(reqs, solo):       # ... which is the pipeline's start for (picture, (seed, j))
            want, k = srv.pipe.init_latent(r.init, 64, 64, 8, 0.75, torch.tensor([[r.seed, j] for j in range(r.n)]))
            assert k == 6 and torch.equal(rows, want)
        assert not torch.equal(solo[0][0], solo[0][1])
    finally:
        srv.close()


# ---- the fixture -------------------------------------------------------------------------------------------------------
def test_golden_moments_are_the_oracles():
    """tests/golden/img2img.npz recomputed from oracle/ on the picture formula (tools/make_img2img_golden.py)"""
    sys.path.insert(0, os.path.join(REPO, "tools"))
    import json
    import make_img2img_golden as G
    z = np.load(G.GOLDEN, allow_pickle=False)
    meta = json.loads(str(z["meta"]))
    assert os.path.getsize(G.GOLDEN) < 100 << 10 and meta["side"] == 256 and z["moments"].shape == (1, 8, 32, 32)
    now = G.oracle_moments()
    assert float(np.abs(now - z["moments"]).max()) <= 1e-5 * max(1.0, float(np.abs(now).max()))
    pic = R.picture_u8(256, 256)
    assert pic.dtype == np.uint8 and pic.min() < 32 and pic.max() > 224 and len(np.unique(pic)) > 128
