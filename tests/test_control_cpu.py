"""CPU: ControlNet strength -- lib/control.py (the specification: window, layer weights, the table, the kernel's formula, what a
request's arguments come to) and its mutants; csrc/control.hip on the CPU emulation (tools/cpu_emu/emu_control.cpp) against the
specification at the bound of tests/control_refs.py and bit for bit against the emulated pfd_add_f16; the sampler's host loop
on the stand-in (which steps carry the control and the table, the graph key, the refusals); the arguments of
PromptFreePipeline.generate and PromptFreeServer.submit, checked before any device call, sharded over ranks, and batched."""
import math
import os
import subprocess
import sys
import threading
from fractions import Fraction

import numpy as np
import pytest
import torch

import control_refs as R
import sampler_standin as SS
from lib import control

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get("EMU_CXX", "/opt/rocm/lib/llvm/bin/clang++")
GRID = [Fraction(a, b) for b in (1, 2, 3, 4, 5, 8, 10) for a in range(b + 1)]
WINDOWS = sorted({(s, e) for s in GRID for e in GRID if s <= e})


# ---- the specification ---------------------------------------------------------------------------------------------------
def _brute(total, k, s, e):
    """the rule in exact rational arithmetic: step i is controlled iff ceil(s total) <= total - k + i < floor(e total)"""
    on = [i for i in range(k) if math.ceil(s * total) <= total - k + i < math.floor(e * total)]
    return (on[0], on[-1] + 1) if on else (0, 0)


def test_window_steps_against_the_rational_rule():
    n = 0
    for total in range(1, 13):
        for k in range(1, total + 1):
            for s, e in WINDOWS:
                assert control.window_steps(total, k, (float(s), float(e))) == _brute(total, k, s, e), (total, k, s, e)
                n += 1
    assert n == 78 * len(WINDOWS) and len(WINDOWS) > 150
    for total in range(1, 13):
        for k in range(1, total + 1):
            assert control.window_steps(total, k, (0, 1)) == (0, k)
            for s in GRID:
                assert control.window_steps(total, k, (float(s), float(s))) == (0, 0)


def test_a_window_names_the_same_positions_for_every_k():
    for total in (4, 6, 10, 12):
        for s, e in WINDOWS:
            lo, hi = control.window_steps(total, total, (float(s), float(e)))
            full = set(range(lo, hi))
            for k in range(1, total + 1):
                a, b = control.window_steps(total, k, (float(s), float(e)))
                assert {total - k + i for i in range(a, b)} == {p for p in full if p >= total - k}, (total, k, s, e)


@pytest.mark.parametrize("bad", [(0.5, 0.25), (-0.1, 1), (0, 1.5), (0,), "ab", None, (float('nan'), 1)])
def test_window_arguments(bad):
    with pytest.raises(ValueError):
        control.window_steps(4, 4, bad)


def test_window_steps_refuses_a_run_longer_than_the_schedule():
    for total, k in ((4, 5), (4, 0), (0, 0)):
        with pytest.raises(ValueError):
            control.window_steps(total, k, (0, 1))


def test_layer_scales():
    assert np.array_equal(control.layer_scales(None), np.ones(13))
    soft = control.layer_scales('soft')
    assert soft.dtype == np.float64 and soft[12] == 1.0 and soft[0] == 0.825 ** 12
    assert np.allclose(soft[1:] / soft[:-1], 1 / 0.825, rtol=1e-14)
    seq = [0.1 * i for i in range(13)]
    assert np.array_equal(control.layer_scales(seq), np.array(seq))
    assert np.array_equal(control.layer_scales(tuple(seq)), np.array(seq))
    for bad in ('hard', [1.0] * 12, [1.0] * 14, [1.0] * 12 + [-0.5], [1.0] * 12 + [float('inf')], [1.0] * 12 + ['x'], 3.0):
        with pytest.raises(ValueError):
            control.layer_scales(bad)


def test_scale_table_values_rounding_and_zero_rows():
    t = control.scale_table([1.0, 0.4, 0.7], 'soft', 3, 2)
    assert t.dtype == np.float32 and t.shape == (6, 13) and t.flags['C_CONTIGUOUS']
    want = (np.array([1.0, 0.4, 0.7])[:, None] * (0.825 ** (12.0 - np.arange(13)))[None]).astype(np.float32)   # one rounding
    assert np.array_equal(t[:3], want) and np.array_equal(t[3:], want)
    assert not np.array_equal(t[1], (np.float32(0.4) * control.layer_scales('soft').astype(np.float32)))       # ... not two
    one = control.scale_table(0.7, None, 2, 1)
    assert one.shape == (2, 13) and np.all(one == np.float32(0.7))
    co = control.scale_table([1.0, 0.4], 'soft', 2, 2, cond_only=True)
    assert np.all(co[:2] == 0.0) and not np.signbit(co[:2]).any() and np.array_equal(co[2:], t[:2])
    assert np.array_equal(control.scale_table([1.0, 0.4], 'soft', 2, 1, cond_only=True), t[:2])      # no CFG: nothing to zero
    for bad in ([1.0], [1.0, -1.0], [1.0, float('nan')], 'x', [[1.0, 1.0]], -0.5, float('inf')):
        with pytest.raises(ValueError):
            control.scale_table(bad, None, 2, 2)
    with pytest.raises(ValueError):
        control.scale_table(1.0, None, 2, 3)


def test_add_scaled_formula():
    x, r, s = R.operands(3, 8, 'mixed', 5)
    y = control.add_scaled(x, r, s)
    assert y.dtype == np.float64 and np.array_equal(y[0], x[0].astype(np.float64))          # r[0] holds NaN: not consulted
    assert np.array_equal(y[1:], x[1:].astype(np.float64) + s[1:, None].astype(np.float64) * r[1:].astype(np.float64))
    with pytest.raises(ValueError):
        control.add_scaled(x, r[:2], s)


def test_normalise():
    n, total = 2, 6
    for spelling in (dict(), dict(scale=1), dict(scale=[1.0, 1.0]), dict(scale=np.ones(2)), dict(layers=[1.0] * 13),
                     dict(layers=np.ones(13)), dict(window=[0, 1]), dict(window=(0.0, 1.0)), dict(cond_only=True, nb=1)):
        kw = dict(scale=1.0, layers=None, window=(0.0, 1.0), cond_only=False, nb=2)
        kw.update(spelling)
        nb = kw.pop('nb')
        assert control.normalise(kw['scale'], kw['layers'], kw['window'], kw['cond_only'], n, total, total, nb) is None, spelling
    assert control.normalise(1.0, None, (0, 1), False, n, total, 4) is None          # a shortened run, wholly inside the window
    for off in (dict(scale=0), dict(scale=[0.0, 0.0]), dict(layers=[0.0] * 13), dict(window=(0, 0)), dict(window=(0.5, 0.5)),
                dict(window=(0.4, 0.6), total=4), dict(window=(0, 0.5), k=2)):
        kw = dict(scale=1.0, layers=None, window=(0.0, 1.0), total=total, k=None)
        kw.update(off)
        k = kw['total'] if kw['k'] is None else kw['k']
        assert control.normalise(kw['scale'], kw['layers'], kw['window'], False, n, kw['total'], k) == 'off', off
    tab, steps = control.normalise([1.0, 0.4], 'soft', (0, 0.5), True, n, total, 4)
    assert steps == (0, 1) and np.array_equal(tab, control.scale_table([1.0, 0.4], 'soft', 2, 2, True))
    tab, steps = control.normalise(1.0, None, (0, 0.5), False, n, total, total)
    assert steps == (0, 3) and np.all(tab == 1.0)
    tab, steps = control.normalise(1.0, None, (0, 1), True, n, total, total)           # cond_only under CFG is no default
    assert steps == (0, total) and np.all(tab[:2] == 0) and np.all(tab[2:] == 1)
    for bad in (dict(scale=-1), dict(layers='hard'), dict(window=(1, 0))):            # checked whatever the outcome
        kw = dict(scale=0.0, layers=None, window=(0.0, 1.0))
        kw.update(bad)
        with pytest.raises(ValueError):
            control.normalise(kw['scale'], kw['layers'], kw['window'], False, n, total, total)


def test_every_mutant_differs_from_the_specification():
    assert set(control.MUTANTS) == {'window_lo_off_by_one', 'window_hi_off_by_one', 'window_of_run', 'layers_reversed',
                                    'uncond_not_zeroed', 'scale_on_x'}
    moved = dict.fromkeys(control.MUTANTS, 0)
    cases = [(total, k, (float(s), float(e))) for total in (4, 6, 10) for k in (total, total // 2) for s, e in WINDOWS]
    for wr in ('window_lo_off_by_one', 'window_hi_off_by_one', 'window_of_run'):
        for total, k, w in cases:
            moved[wr] += control.window_steps(total, k, w, wrong=wr) != control.window_steps(total, k, w)
        assert control.window_steps(6, 6, (0, 0.5), wrong=wr) != (0, 3) or wr == 'window_of_run'
    assert control.window_steps(6, 6, (0, 0.5), wrong='window_lo_off_by_one') == (1, 3)
    assert control.window_steps(6, 6, (0, 0.5), wrong='window_hi_off_by_one') == (0, 4)
    assert control.window_steps(6, 4, (0, 0.5)) == (0, 1) and control.window_steps(6, 4, (0, 0.5), wrong='window_of_run') == (0, 2)
    moved['layers_reversed'] += not np.array_equal(control.scale_table(1.0, 'soft', 2, 2, wrong='layers_reversed'),
                                                   control.scale_table(1.0, 'soft', 2, 2))
    assert np.array_equal(control.layer_scales('soft', wrong='layers_reversed'), control.layer_scales('soft')[::-1])
    moved['uncond_not_zeroed'] += not np.array_equal(control.scale_table(1.0, None, 2, 2, True, wrong='uncond_not_zeroed'),
                                                     control.scale_table(1.0, None, 2, 2, True))
    for kind in ('act', 'small', 'cancel'):
        x, r, s = R.operands(2, 64, kind, 3)
        y, ym = control.add_scaled(x, r, s), control.add_scaled(x, r, s, wrong='scale_on_x')
        far = np.abs(ym - y) > 4 * R.bound(x, r, s, y)
        moved['scale_on_x'] += bool(far.any())
    assert all(moved.values()), moved
    with pytest.raises(ValueError):
        control.window_steps(4, 4, (0, 1), wrong='something_else')


# ---- the kernel on the CPU emulation ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu_control(tmp_path_factory):
    if not os.path.exists(CXX):
        pytest.skip("clang++ of the ROCm toolchain not available")
    out = str(tmp_path_factory.mktemp("pfd_cpu_emu_control"))
    subprocess.run([sys.executable, os.path.join(REPO, "tools", "cpu_emu", "build.py"), out], check=True,
                   stdout=subprocess.DEVNULL, env=dict(os.environ, EMU_ONLY="emu_control", EMU_OPT="-O1"))
    return os.path.join(out, "emu_control")


def _run_emu(exe, args):
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=900)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith(("ok", "FAIL"))]
    assert r.returncode == 0 and len(lines) == len(args) and all(ln.startswith("ok") for ln in lines), \
        r.stdout[-3000:] + r.stderr[-1000:]
    return lines


def _scaled_arg(path, x, r, s, stride, alias, offset=0, rc=0):
    tab = R.strided_scale(s, stride).reshape(-1)[:(s.shape[0] - 1) * stride + 1]
    with open(path, "wb") as f:
        f.write(x.tobytes() + r.tobytes() + tab.tobytes())
    return f"scaled,{x.shape[0]},{x.shape[1]},{stride},{alias},{offset},{rc},{path}"


def test_kernel_on_the_emulation_matches_the_specification(emu_control, tmp_path):
    """every shape (B 1 and 3; 8, 328 and 40960 elements per sample), scale strides 1 and 13, out of place and in place on x and
    on r: return code, one launch, guard bands; within the bound of control_refs against fp64; scale 1 bit-equal to the emulated
    pfd_add_f16; scale 0 gives x's bits with NaN in r"""
    cases = R.kernel_cases()
    args, data = [], []
    for i, c in enumerate(cases):
        x, r, s = R.operands(c['B'], c['n'], c['kind'], c['seed'])
        path = str(tmp_path / f"case{i}.bin")
        args.append(_scaled_arg(path, x, r, s, c['stride'], c['alias']))
        data.append((path, x, r, s))
        if c['kind'] == 'ones':
            apath = str(tmp_path / f"add{i}.bin")
            with open(apath, "wb") as f:
                f.write(x.tobytes() + r.tobytes())
            args.append(f"add,{x.size},{apath}")
    lines = _run_emu(emu_control, args)
    assert all("add_scaled_rows_kernel" in ln for ln in lines if " scaled " in ln)
    kinds = set()
    for i, (c, (path, x, r, s)) in enumerate(zip(cases, data)):
        y = np.fromfile(path + ".out", dtype=np.float16).reshape(x.shape)
        e = R.judge(y, x, r, s)
        print(f"[control emu] {R.case_id(c)}: error / bound {e:.3f}")
        assert e <= 1.0, (R.case_id(c), e)
        if c['kind'] == 'ones':
            add = np.fromfile(str(tmp_path / f"add{i}.bin") + ".out", dtype=np.float16).reshape(x.shape)
            assert np.array_equal(y.view(np.uint16), add.view(np.uint16)), R.case_id(c)
        if c['kind'] == 'zeros':
            assert np.array_equal(y.view(np.uint16), x.view(np.uint16))
        kinds.add(c['kind'])
    assert kinds == {'act', 'small', 'cancel', 'ones', 'zeros', 'mixed'}


def test_kernel_on_the_emulation_refuses_bad_arguments(emu_control, tmp_path):
    """n % 8 != 0 and a misaligned pointer are PFD_ESHAPE, nothing is launched and nothing written"""
    args = []
    for i, (n, offset) in enumerate(((12, 0), (7, 0), (16, 1), (16, 4))):
        x, r, s = R.operands(2, n, 'act', i)
        args.append(_scaled_arg(str(tmp_path / f"bad{i}.bin"), x, r, s, 1, 0, offset, rc=-2))
    _run_emu(emu_control, args)
    for i in range(4):
        assert set(np.fromfile(str(tmp_path / f"bad{i}.bin") + ".out", dtype=np.uint8).tolist()) == {0xA5}


def test_header_declares_and_binding_lists_the_entry_point():
    from lib.hip import binding
    text = open(os.path.join(REPO, "include", "pfd_hip.h")).read()
    assert "int pfd_add_scaled_rows_f16(const void* x, const void* r, const float* scale, int64_t scale_stride, void* y, int32_t B," in text
    assert len(binding.SIGNATURES["pfd_add_scaled_rows_f16"][1]) == 8 and binding.ABI_VERSION == 10


def test_ops_wrapper_checks_its_operands_before_the_library():
    from lib.hip import ops
    x = torch.zeros(2, 16, dtype=torch.float16)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.add_scaled_rows(x, x, torch.ones(2))
    with pytest.raises(TypeError):
        ops.add_scaled_rows(x.float(), x, torch.ones(2))


# ---- the sampler on the stand-in -------------------------------------------------------------------------------------------
def _sampler(monkeypatch):
    from lib.model_zoo.ddim import DDIMSampler
    SS.install(monkeypatch)
    return DDIMSampler(R.ControlStub())


def _infos(bs=2, k=None, table=None, steps=None, scale=2.5):
    g = torch.Generator().manual_seed(7)
    x_info = {'type': 'image', 'xt': torch.randn(bs, 4, 3, 5, generator=g)}
    if k is not None:
        x_info['xt_steps'] = k
    c = {'type': 'image', 'conditioning': torch.randn(bs, 3, 8, generator=g).half(), 'unconditional_guidance_scale': scale,
         'unconditional_conditioning': torch.randn(bs, 3, 8, generator=g).half(), 'control': torch.randn(1, 3, 6, 10, generator=g)}
    if table is not None:
        c['control_scale'] = torch.from_numpy(table)
    if steps is not None:
        c['control_steps'] = steps
    return x_info, c


def test_sampler_calls_the_model_with_the_control_inside_the_window_only(monkeypatch):
    """the exact sequence of model calls (total = 8: the uniform schedule has no form with 6 entries -- 6 steps give 7)"""
    from lib.pipeline import schedule_length
    total = 8
    assert schedule_length(total, 1000) == total and schedule_length(6, 1000) == 7
    ones = control.scale_table(1.0, None, 2, 2)
    soft = control.scale_table([1.0, 0.4], 'soft', 2, 2)
    want = {
        'plain': (None, None, None, ["True table=False"] * 8),
        'window': (None, ones, control.window_steps(total, total, (0, 0.5)), ["True table=True"] * 4 + ["False table=False"] * 4),
        'window_k6': (6, ones, control.window_steps(total, 6, (0, 0.5)), ["True table=True"] * 2 + ["False table=False"] * 4),
        'full_with_table': (None, soft, (0, total), ["True table=True"] * 8),
        'steps_left_out': (None, soft, None, ["True table=True"] * 8),
        'empty': (None, soft, (2, 2), ["False table=False"] * 8),
    }
    outs = {}
    for name, (k, tab, steps, calls) in want.items():
        s = _sampler(monkeypatch)
        x_info, c = _infos(k=k, table=tab, steps=steps)
        outs[name], _ = s.sample(total, [2, 4, 3, 5], x_info, c, verbose=False)
        assert R.model_calls() == calls, name
        assert sum(ln.startswith("prepare_hint") for ln in SS.LOG) == 1
    assert torch.equal(outs['steps_left_out'], outs['full_with_table'])
    assert not torch.equal(outs['window'], outs['plain']) and not torch.equal(outs['full_with_table'], outs['plain'])
    # an empty window is the run without the control; a ones table over every step the plain control run (on the stand-in
    # the table enters eps as a factor 1.0)
    s = _sampler(monkeypatch)
    x_info, c = _infos()
    del c['control']
    assert torch.equal(s.sample(total, [2, 4, 3, 5], x_info, c, verbose=False)[0], outs['empty'])
    s = _sampler(monkeypatch)
    x_info, c = _infos(table=ones, steps=(0, total))
    assert torch.equal(s.sample(total, [2, 4, 3, 5], x_info, c, verbose=False)[0], outs['plain'])


def test_sampler_checks_the_table_and_the_steps(monkeypatch):
    ones = control.scale_table(1.0, None, 2, 2)
    bad = [dict(table=ones[:2]), dict(table=ones.astype(np.float64)), dict(table=ones[:, :12].copy()), dict(steps=(0, 2)),
           dict(table=ones, steps=(0, 5)), dict(table=ones, steps=(3, 2)), dict(table=ones, steps=(0.5, 2)), dict(table=ones, steps=3)]
    for kw in bad:
        s = _sampler(monkeypatch)
        x_info, c = _infos(**kw)
        with pytest.raises(ValueError, match="control_s"):
            s.sample(4, [2, 4, 3, 5], x_info, c, verbose=False)
    s = _sampler(monkeypatch)
    x_info, c = _infos(table=ones)
    del c['control']
    with pytest.raises(ValueError, match="need c_info\\['control'\\]"):
        s.sample(4, [2, 4, 3, 5], x_info, c, verbose=False)


class _OnDevice(torch.Tensor):
    """a CPU tensor that says it is on the device: the sampler then takes its graph branch, whose capture the test replaces"""
    is_cuda = property(lambda self: True)


def _graph_keys(monkeypatch, **kw):
    from lib.model_zoo.ddim import DDIMSampler
    s = _sampler(monkeypatch)
    keys = []

    class _Loop:
        def __init__(self, run_loop):
            self.run_loop = run_loop

        def replay(self, inputs):
            return self.run_loop(*inputs)

    start = DDIMSampler._start_latent
    monkeypatch.setattr(DDIMSampler, "_start_latent", lambda self, *a: (lambda x, t: (x.as_subclass(_OnDevice), t))(*start(self, *a)))
    monkeypatch.setattr(DDIMSampler, "_weights_signature", lambda self: 0)
    monkeypatch.setattr(DDIMSampler, "_capture", lambda self, run_loop, t_table, inputs, coef: _Loop(run_loop))
    graph_for = DDIMSampler._graph_for
    monkeypatch.setattr(DDIMSampler, "_graph_for", lambda self, key, capture: (keys.append(key), graph_for(self, key, capture))[1])
    s.enable_graph(True)
    x_info, c = _infos(**kw)
    out, _ = s.sample(6, [2, 4, 3, 5], x_info, c, verbose=False)
    return keys[0], torch.Tensor(out), s


def test_graph_key_gains_a_trailing_element(monkeypatch):
    ones = control.scale_table(1.0, None, 2, 2)
    plain, xp, _ = _graph_keys(monkeypatch)
    key, x, s = _graph_keys(monkeypatch, table=ones, steps=(0, 3))
    assert key[-1] == ('control', 0, 3) and key[:-1] == plain
    assert not any(isinstance(e, tuple) and e and e[0] == 'control' for e in plain)
    other, _, _ = _graph_keys(monkeypatch, table=control.scale_table([0.3, 0.9], 'soft', 2, 2), steps=(0, 3))
    assert other == key                                            # another strength: the same graph
    assert _graph_keys(monkeypatch, table=ones, steps=(0, 2))[0] != key
    # the graphed branch computes what the eager one does
    s2 = _sampler(monkeypatch)
    x_info, c = _infos(table=ones, steps=(0, 3))
    assert torch.equal(s2.sample(6, [2, 4, 3, 5], x_info, c, verbose=False)[0], x)


def test_entry_points_without_the_loop_refuse_the_new_keys(monkeypatch):
    ones = control.scale_table(1.0, None, 2, 2)
    for kw in (dict(table=ones), dict(table=ones, steps=(0, 2))):
        s = _sampler(monkeypatch)
        s.make_schedule(4, verbose=False)
        x_info, c = _infos(**kw)
        x_info['x'] = x_info['xt'].half()
        t = torch.full((2,), 501, dtype=torch.long)
        with pytest.raises(ValueError, match="p_sample_ddim takes no"):
            s.p_sample_ddim(x_info, c, t, 2)
        cl = [dict(c, ratio=0.5), dict(c, ratio=0.5)]
        with pytest.raises(ValueError, match="takes no"):
            s.p_sample_ddim_multicontext(x_info, cl, t, 2)
        with pytest.raises(ValueError, match="takes no"):
            s.sample_multicontext(4, [2, 4, 3, 5], x_info, cl, verbose=False)
        with pytest.raises(ValueError, match="takes no"):
            s.ddim_sampling_multicontext([2, 4, 3, 5], x_info, cl)


# ---- the UNet's host layer -----------------------------------------------------------------------------------------------
def test_apply_model_passes_the_table_only_when_there_is_one():
    """StubModel.apply_model_nhwc of tests/sampler_standin.py has no control_scale parameter: the default call must not name it"""
    from lib.model_zoo.pfd import PromptFreeDiffusion
    seen = []

    class _UNet:
        def hip(self, x, t, context, **kw):
            seen.append(sorted(kw))
            return x

    class _Model:
        diffuser = {'image': _UNet()}
        global_layer_ptr = None

        def _control_residuals(self, x, t, ctx, control, cfg_pair=False):
            return None if control is None else [control]
    fn = PromptFreeDiffusion.apply_model_nhwc.__wrapped__.__wrapped__
    x = torch.zeros(1, 2, 2, 4, dtype=torch.float16)
    fn(_Model(), 'image', x, torch.zeros(1), 'image', object(), control=x)
    fn(_Model(), 'image', x, torch.zeros(1), 'image', object(), control=x, control_scale=torch.ones(1, 1))
    assert seen == [['cfg_pair', 'context_net', 'control', 'emb_table'], ['cfg_pair', 'context_net', 'control', 'control_scale', 'emb_table']]
    with pytest.raises(ValueError, match="without control"):
        fn(_Model(), 'image', x, torch.zeros(1), 'image', object(), control_scale=torch.ones(1, 1))


# ---- pipeline and server: arguments, sharding, batching --------------------------------------------------------------------
IMG = torch.rand(1, 3, 64, 64)
CTL = torch.rand(1, 3, 64, 64)


class _Seen:
    def __init__(self):
        self.c = None

    def enable_graph(self, on=True):
        pass

    def sample(self, steps, shape, x_info, c_info, eta=0., verbose=True):
        self.c = dict(c_info, xt_steps=x_info.get('xt_steps'))
        return x_info['xt'], {}


def _pipe(rank=0, world=1, touch_ok=True):
    from stubs import StubNet
    from lib.pipeline import PromptFreePipeline

    class _Net(StubNet):
        def ctx_encode(self, image, which):
            if not touch_ok:
                raise AssertionError("the device was touched before the arguments were checked")
            return super().ctx_encode(image, which)
    seen = _Seen()
    return PromptFreePipeline(_Net(), rank=rank, world_size=world, sampler=seen), seen


BAD = [dict(control_scale=-1.0), dict(control_scale=[1.0, 0.5, 0.2]), dict(control_scale=float('nan')), dict(control_scale='x'),
       dict(control_layer_scales='hard'), dict(control_layer_scales=[1.0] * 12), dict(control_layer_scales=[-1.0] * 13),
       dict(control_window=(0.5, 0.2)), dict(control_window=(0, 2)), dict(control_window=0.5)]


@pytest.mark.parametrize("bad", BAD, ids=[str(b) for b in BAD])
def test_generate_checks_the_arguments_before_the_device(bad):
    pipe, _ = _pipe(touch_ok=False)
    with pytest.raises(ValueError, match="control_"):
        pipe.generate(IMG, 2, 64, 64, steps=4, control=CTL, decode=False, **bad)


@pytest.mark.parametrize("kw", [dict(control_scale=0.5), dict(control_layer_scales='soft'), dict(control_window=(0, 0.5)),
                                dict(control_cond_only=True), dict(control_scale=0.0)])
def test_generate_refuses_the_arguments_without_a_control(kw):
    pipe, _ = _pipe(touch_ok=False)
    with pytest.raises(ValueError, match="need a control picture"):
        pipe.generate(IMG, 2, 64, 64, steps=4, decode=False, **kw)


def test_generate_hands_the_sampler_what_normalise_says():
    pipe, seen = _pipe()
    gen = lambda **kw: pipe.generate(IMG, 2, 64, 64, steps=4, control=CTL, decode=False, **kw)      # noqa: E731
    for plain in (dict(), dict(control_scale=1.0), dict(control_scale=[1.0, 1.0]), dict(control_layer_scales=[1.0] * 13),
                  dict(control_window=[0, 1]), dict(control_cond_only=True, scale=1.0)):
        gen(**plain)
        assert seen.c['control'] is not None and 'control_scale' not in seen.c and 'control_steps' not in seen.c, plain
    for off in (dict(control_scale=0), dict(control_window=(0, 0)), dict(control_window=(0.5, 0.5)), dict(control_scale=[0, 0])):
        gen(**off)
        assert 'control' not in seen.c and 'control_scale' not in seen.c and 'control_steps' not in seen.c, off
    gen(control_scale=[1.0, 0.4], control_layer_scales='soft', control_window=(0, 0.5), control_cond_only=True)
    assert seen.c['control_steps'] == (0, 2) and seen.c['control_scale'].dtype == torch.float32
    assert np.array_equal(seen.c['control_scale'].numpy(), control.scale_table([1.0, 0.4], 'soft', 2, 2, True))
    gen(control_scale=0.5, scale=1.0)                               # no CFG: one row per sample
    assert tuple(seen.c['control_scale'].shape) == (2, 13) and seen.c['control_steps'] == (0, 4)


def test_a_per_sample_strength_is_sharded_like_the_guidance_scale():
    """rank r of 2 gets the rows of ITS samples of the global batch; the whole vector is checked on every rank"""
    strengths = [1.0, 0.4, 0.0, 0.7]
    for rank in range(2):
        pipe, seen = _pipe(rank, 2)
        pipe.generate(IMG, 4, 64, 64, steps=4, control=CTL, decode=False, control_scale=strengths, control_layer_scales='soft')
        want = control.scale_table(strengths[2 * rank:2 * rank + 2], 'soft', 2, 2)
        assert np.array_equal(seen.c['control_scale'].numpy(), want) and seen.c['control_steps'] == (0, 4)
        with pytest.raises(ValueError, match="control_scale"):
            pipe.generate(IMG, 4, 64, 64, steps=4, control=CTL, decode=False, control_scale=[1.0, 0.4, 0.0, -0.7])
        with pytest.raises(ValueError, match="control_scale"):
            pipe.generate(IMG, 4, 64, 64, steps=4, control=CTL, decode=False, control_scale=[1.0, 0.4])
    pipe, seen = _pipe(1, 2)                       # a rank whose samples all have strength 0 runs them without the control
    pipe.generate(IMG, 4, 64, 64, steps=4, control=CTL, decode=False, control_scale=[1.0, 0.4, 0.0, 0.0])
    assert 'control' not in seen.c


def test_the_window_of_an_img2img_request_counts_on_the_full_schedule():
    pipe, seen = _pipe()
    pipe.net.num_timesteps = 1000

    class _Latent:
        def __call__(self, init, height, width, steps, strength, keys, posterior='sample', want_x0=False):
            from lib import image_io
            k = image_io.check_img2img(init, height, width, steps, strength, posterior)
            return torch.zeros(keys.shape[0], 4, height // 8, width // 8), k
    pipe.init_latent = _Latent()
    init = torch.rand(1, 3, 64, 64)
    pipe.generate(IMG, 2, 64, 64, steps=4, control=CTL, decode=False, init=init, strength=0.5, control_window=(0, 0.75))
    assert seen.c['xt_steps'] == 2 and seen.c['control_steps'] == (0, 1)        # positions 2, 3 of 4; the window ends at 3
    pipe.generate(IMG, 2, 64, 64, steps=4, control=CTL, decode=False, init=init, strength=0.5, control_window=(0, 0.5))
    assert 'control' not in seen.c                                                # the window ended before the run began


def _server(monkeypatch, **kw):
    from lib import serving

    class _Pipe:
        def __init__(self, net):
            pass

        def enable_graph(self, on):
            pass
    monkeypatch.setattr(serving, "PromptFreePipeline", _Pipe)
    srv = serving.PromptFreeServer(object(), use_graph=False, max_batch=4, **kw)
    calls = []

    def fake_generate(batch):
        calls.append([r.seed for r in batch])
        return [torch.full((r.n, 1), float(r.seed)) for r in batch]
    srv._generate = fake_generate
    return srv, calls


def _queued(srv, submits):
    gate = threading.Event()
    srv.call(lambda n: gate.wait(30))
    futs = [srv.submit(IMG, 1, 64, 64, steps=4, **k) for k in submits]
    gate.set()
    return [f.result(30) for f in futs]


W = dict(control=CTL, control_window=(0, 0.5))
SHARING = [
    # strengths differ, window equal: one batch; the plain control request keeps to itself
    ([dict(W, control_scale=1.0), dict(W, control_scale=0.5), dict(control=CTL)], [[1, 2], [3]]),
    ([dict(control=CTL), dict(W), dict(control=CTL)], [[1], [2], [3]]),
    # another window, other layer weights, cond_only: no sharing
    ([dict(W), dict(control=CTL, control_window=(0, 0.75))], [[1], [2]]),
    ([dict(W), dict(W, control_layer_scales='soft')], [[1], [2]]),
    ([dict(W), dict(W, control_cond_only=True)], [[1], [2]]),
    ([dict(W, control_layer_scales='soft', control_scale=0.3), dict(W, control_layer_scales='soft')], [[1, 2]]),
    # every default spelling is the plain control request; nothing left of the control is the uncontrolled request
    ([dict(control=CTL), dict(control=CTL, control_scale=1.0, control_layer_scales=[1.0] * 13, control_window=[0, 1])], [[1, 2]]),
    ([dict(), dict(control=CTL, control_scale=0.0), dict(control=CTL, control_window=(0.5, 0.5)), dict()], [[1, 2, 3, 4]]),
]


@pytest.mark.parametrize("case", range(len(SHARING)))
def test_server_batch_sharing(monkeypatch, case):
    submits, want = SHARING[case]
    srv, calls = _server(monkeypatch, mixed_batches=True)
    try:
        outs = _queued(srv, [dict(k, seed=i + 1) for i, k in enumerate(submits)])
        assert calls == want
        assert [float(o[0, 0]) for o in outs] == [float(i + 1) for i in range(len(submits))]
    finally:
        srv.close()


def test_server_without_mixed_batches_runs_control_requests_alone_as_before(monkeypatch):
    srv, calls = _server(monkeypatch)
    try:
        _queued(srv, [dict(W, seed=1), dict(W, seed=2), dict(seed=3), dict(seed=4)])
        assert calls == [[1], [2], [3, 4]]
    finally:
        srv.close()


def test_submit_checks_the_arguments_on_the_callers_thread(monkeypatch):
    srv, calls = _server(monkeypatch)
    try:
        for bad in BAD:
            if bad == dict(control_scale=[1.0, 0.5, 0.2]):
                bad = dict(control_scale=[1.0, 0.5])               # one sample in the request
            with pytest.raises(ValueError, match="control_"):
                srv.submit(IMG, 1, 64, 64, steps=4, control=CTL, **bad)
        with pytest.raises(ValueError, match="need a control picture"):
            srv.submit(IMG, 1, 64, 64, steps=4, control_scale=0.5)
        assert calls == []
    finally:
        srv.close()


def test_request_key_without_the_arguments_is_what_it_was():
    from lib import serving
    kw = dict(image=IMG, n=1, height=64, width=64, steps=4, seed=1, eta=0.0)
    R_ = serving._Request
    assert R_(scale=1.5, **kw).key() == (64, 64, 4, 1.5, 0.0, True, True, False, False)
    a = R_(scale=1.5, control=CTL, ctl=(np.ones(1), (1.0,) * 13, (0, 2), False), **kw)
    assert a.key() == (64, 64, 4, 1.5, 0.0, False, True, False, False, ('control', (1.0,) * 13, (0, 2), False))
    b = R_(scale=1.5, control=CTL, ctl=(np.full(1, 0.3), (1.0,) * 13, (0, 2), False), **kw)
    assert a.key() == b.key()


def test_server_generate_builds_the_table_of_the_batch():
    """the real `_generate` over stand-ins for the device work: each sample gets the rows of ITS request's strength"""
    from stubs import StubNet
    from lib import serving
    seen = _Seen()
    kw = dict(image=IMG, height=64, width=64, steps=4, eta=0.0, as_uint8=False, future=None, control=CTL, mixed=True)
    lay = tuple(float(v) for v in control.layer_scales('soft'))
    srv = serving.PromptFreeServer(StubNet(), use_graph=False, max_batch=8, mixed_batches=True)
    try:
        srv.pipe.sampler = seen
        Rq = serving._Request
        srv._generate([Rq(n=2, seed=1, scale=2.0, ctl=(np.array([1.0, 0.4]), lay, (0, 2), True), **kw),
                       Rq(n=1, seed=2, scale=3.0, ctl=(np.array([0.5]), lay, (0, 2), True), **kw)])
        assert seen.c['control_steps'] == (0, 2) and tuple(seen.c['control'].shape) == (3, 3, 64, 64)
        assert np.array_equal(seen.c['control_scale'].numpy(), control.scale_table([1.0, 0.4, 0.5], 'soft', 3, 2, True))
        srv._generate([Rq(n=1, seed=1, scale=1.0, ctl=(np.array([0.5]), lay, (0, 4), False), **kw)])      # scale 1: no CFG
        assert np.array_equal(seen.c['control_scale'].numpy(), control.scale_table([0.5], 'soft', 1, 1))
        srv._generate([Rq(n=1, seed=1, scale=2.0, **kw)])
        assert 'control_scale' not in seen.c and 'control_steps' not in seen.c
    finally:
        srv.close()
