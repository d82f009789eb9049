"""CPU: guidance rescale (lib/guidance.py, csrc/guidance.hip, pfd_cfg_step_mul) -- the specification and its
mutants, the two kernels on the CPU emulation (tools/cpu_emu/emu_guidance.cpp) against the specification and against the
recorded bits of tests/golden/step_bits.npz, and the host layers (sampler, pipeline, server) over torch stand-ins."""
import math
import os
import subprocess
import sys
import threading

import numpy as np
import pytest
import torch

import guidance_refs as R
import guidance_standin as GS
import inpaint_refs as IR
import sampler_standin as SS
import step_bits_refs as S
from lib import guidance as G

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get("EMU_CXX", "/opt/rocm/lib/llvm/bin/clang++")
GRID = [(shape, B) for shape in R.SHAPES for B in R.BATCHES] + [(R.LONGEST, 1)]


# ---- the specification ---------------------------------------------------------------------------------------------------
def test_factor_written_out_element_by_element():
    eu = [0.5, -0.25, 1.0, 0.125, -1.5, 0.75]
    ec = [0.75, -0.5, 1.25, 0.5, -1.0, 0.25]
    s, phi = 7.5, 0.7
    g = [float(np.float32(u + s * float(np.float32(c - u)))) for u, c in zip(eu, ec)]
    mc, mg = sum(ec) / 6, sum(g) / 6
    sd_c = math.sqrt(sum((v - mc) ** 2 for v in ec) / 6)
    sd_g = math.sqrt(sum((v - mg) ** 2 for v in g) / 6)
    want = phi * sd_c / sd_g + (1 - phi)
    eps = np.array([eu, ec], dtype=np.float16).reshape(2, 1, 2, 3)
    got = G.factor(eps, s, phi)
    assert got.shape == (1,) and abs(got[0] - want) <= 1e-15 * want
    gg, e = G.rescaled_eps(eps, s, got)
    assert np.array_equal(gg[0], np.array(g, dtype=np.float32))
    assert np.array_equal(e[0], (np.float64(np.float32(got[0])) * np.array(g, dtype=np.float64)).astype(np.float32))


def test_identities():
    eps = R.make_eps(3, (4, 8, 8))
    s, phi = R.rows(R.SCALES, 3), R.rows(R.PHIS, 3)
    f = G.factor(eps, s, phi)
    # phi == 0: exactly 1, sample by sample; phi == 1: the pure ratio
    assert np.array_equal(G.factor(eps, s, [0.7, 0.0, 1.0])[1:2], [1.0]) and np.array_equal(G.factor(eps, s, 0.0), np.ones(3))
    pure = G.factor(eps, s, 1.0)
    assert np.allclose(f, phi * pure + (1 - phi), rtol=1e-15)
    # a constant guided eps: exactly 1
    const = np.full((2, 2, 2, 4), 0.375, dtype=np.float16)
    assert np.array_equal(G.factor(const, 7.5, 0.7), [1.0])
    # the correction of the std cancels: the unbiased estimators give the same ratio
    e = eps.astype(np.float64).reshape(6, -1)
    for b in range(3):
        gb = G.guided(e[b].astype(np.float32), e[3 + b].astype(np.float32), s[b]).astype(np.float64)
        assert abs(np.std(e[3 + b], ddof=1) / np.std(gb, ddof=1) - pure[b]) <= 1e-14 * pure[b]
    # scale 1: the guided eps IS the conditional eps, nothing to rescale
    assert np.allclose(G.factor(eps, 1.0, 0.7), 1.0, rtol=0, atol=1e-12)
    # a sample does not depend on its company
    for b in range(3):
        assert G.factor(eps[[b, 3 + b]], s[b], phi[b])[0] == f[b]
    # the factor shrinks as the scale grows: 2 -> 7.5 -> 12 on one sample
    one = eps[[0, 3]]
    f3 = [G.factor(one, v, 0.7)[0] for v in R.SCALES]
    assert 1 > f3[0] > f3[1] > f3[2] > 0.3


def test_only_a_cfg_batch_is_defined_and_arguments_are_checked():
    with pytest.raises(ValueError, match="unconditional half first"):
        G.factor(np.zeros((3, 2, 2, 4), dtype=np.float16), 2.0, 0.5)
    eps = R.make_eps(2, (4, 8, 8))
    for bad in (-0.1, 1.5, float('nan'), [0.5], [0.5, 0.5, 0.5], 'x', [0.5, float('inf')]):
        with pytest.raises(ValueError, match="guidance_rescale"):
            G.factor(eps, 2.0, bad)
    with pytest.raises(ValueError, match="scale"):
        G.factor(eps, [2.0, 3.0, 4.0], 0.5)
    with pytest.raises(ValueError, match="unknown mutant"):
        G.factor(eps, 2.0, 0.5, wrong='nope')
    assert G.normalise(None, 2) is None and G.normalise(0.0, 2) is None and G.normalise([0, 0], 2) is None
    assert G.normalise(0.7, 2, nb=1) is None
    v = G.normalise([0.0, 0.7], 2)
    assert v.dtype == np.float32 and v.tolist() == [0.0, np.float32(0.7)]
    with pytest.raises(ValueError, match="guidance_rescale"):
        G.normalise(1.5, 2, nb=1)                         # checked whatever the outcome


def test_chain_length_follows_the_ownership_rule():
    assert G.chain_length(120) == 8 + 10 and G.chain_length(75) == 8 + 10 and G.chain_length(5) == 5 + 10
    assert G.chain_length(4 * 64 * 64) == 16 + 10          # 2048 groups, two per thread
    assert G.chain_length(4 * 96 * 96) == 40 + 10          # 4608 groups: 4.5 per thread, thread 0 has five
    assert G.chain_length(4 * 192 * 192) == 144 + 10
    assert R.bound(R.LONGEST) == 162 * 2.0 ** -24


@pytest.mark.parametrize("shape,B", GRID, ids=[f"{'x'.join(map(str, s))}-B{b}" for s, b in GRID])
def test_every_mutant_leaves_a_thousand_bounds(shape, B):
    eps, s, phi = R.make_eps(B, shape), R.rows(R.SCALES, B), R.rows(R.PHIS, B)
    f = G.factor(eps, s, phi)
    for wrong in G.MUTANTS[:5]:
        if wrong == 'stats_over_batch' and B == 1:
            continue                                      # one sample IS the batch
        d = R.rel_err(G.factor(eps, s, phi, wrong=wrong), f)
        assert d >= R.MUTANT_MARGIN * R.bound(shape), (wrong, d / R.bound(shape))
    # rescale_after_pred_x0: pred_x0 moves by (1 - f) sqrt(1 - a_t) / sqrt(a_t) |g|, far above the step's tolerance
    C, h, w = shape
    x = np.random.default_rng(5).standard_normal((B, h * w * C))
    a_t, a_prev = float(IR.ALPHAS[1]), float(IR.ALPHAS_PREV[1])
    xp, p0 = G.ddim_step(eps, x, a_t, a_prev, s, f)
    xw, pw = G.ddim_step(eps, x, a_t, a_prev, s, f, wrong='rescale_after_pred_x0')
    assert IR.scaled_err(pw, p0) >= R.MUTANT_MARGIN * IR.TOL and IR.scaled_err(xw, xp) >= R.MUTANT_MARGIN * IR.TOL


# ---- the kernels on the emulation -------------------------------------------------------------------------------------------
def _stats_cases(out):
    """every statistics case of this file -> {name: (case argument, B, path)}"""
    cases = {}

    def add(name, eps, s, phi, **kw):
        path = os.path.join(out, f"{name}.bin")
        cases[name] = (R.emu_stats_case(path, eps, s, phi, **kw), kw.get('B', eps.shape[0] // 2), path)
    for shape, B in GRID:
        eps, s, phi = R.make_eps(B, shape), R.rows(R.SCALES, B), R.rows(R.PHIS, B)
        tag = f"{'x'.join(map(str, shape))}-B{B}"
        add(f"grid-{tag}", eps, s, phi)
        if shape != R.LONGEST:
            add(f"off-{tag}", eps, s, phi, offset=1)           # the base 2 bytes behind a 16-byte boundary
        if B == 3:
            for b in range(3):
                add(f"alone-{tag}-{b}", eps[[b, 3 + b]], s[b:b + 1], phi[b:b + 1])
    eps = R.make_eps(3, (4, 8, 8))
    nan = eps.copy()
    nan[[1, 4]] = np.nan
    add("phi0-nan", nan, R.rows(R.SCALES, 3), np.array([0.7, 0.0, 1.0], dtype=np.float32))
    add("constant", np.full((4, 8, 8, 4), 0.375, dtype=np.float16), R.rows(R.SCALES, 2), R.rows(R.PHIS, 2))
    for ss, ps in ((0, 1), (1, 0), (13, 1), (1, 13), (0, 0), (13, 13)):
        s = np.full(3, 7.5, dtype=np.float32) if ss == 0 else R.rows(R.SCALES, 3)
        phi = np.full(3, 0.7, dtype=np.float32) if ps == 0 else R.rows(R.PHIS, 3)
        add(f"stride-{ss}-{ps}", eps, s, phi, sstride=ss, pstride=ps)
    one = eps[[0, 3]]
    for name, kw in (("null-eps", dict(null=1)), ("null-scale", dict(null=2)), ("null-phi", dict(null=4)), ("null-mul", dict(null=8)),
                     ("B0", dict(B=0)), ("Bneg", dict(B=-1)), ("n0", dict(n=0)), ("nneg", dict(n=-8)),
                     ("sstride-neg", dict(sstride=-1)), ("pstride-neg", dict(pstride=-1))):
        if 'n' in kw or 'B' in kw:       # the driver's buffers then hold one sample of one element
            add(f"bad-{name}", np.zeros((2, 1, 1, 1), dtype=np.float16), [7.5], [0.7], rc=-1, **kw)
        else:
            add(f"bad-{name}", one, [7.5], [0.7], rc=-1, **kw)
    return cases


def _step_cases(out):
    """one generator-free nb = 2 case of the step fixture per instantiation, through pfd_cfg_step_mul: with ones, and with
    factors that differ per sample; and the refusals -> [(name, case argument, fixture case, path, mul or None)]"""
    _, cases = S.load()
    picked = {}
    for c in cases:
        if c['generator_free'] and c['nb'] == 2 and c['rep'] == 1:
            picked.setdefault(S.kernel_of(c), c)
    assert len(picked) == 10, sorted(picked)
    runs = []
    for i, c in enumerate(picked.values()):
        B = c['shape'][0]
        for tag, mul in (("ones", np.ones(B, dtype=np.float32)), ("mul", np.linspace(0.57, 0.97, B).astype(np.float32))):
            path = os.path.join(out, f"step{i}-{tag}.bin")
            arg = "step,0," + S.emu_case(c, path)
            mul.tofile(path + ".mulin")
            runs.append((f"{tag}-{c['name']}", arg, c, path, mul))
    # refusals: no factors; nb = 1; (below) pointer rules of the entry point stood for
    c = next(iter(picked.values()))
    path = os.path.join(out, "step-nomul.bin")
    runs.append(("refused-null-mul", "step,-1," + S.emu_case(c, path), c, path, None))
    c1 = next(k for k in cases if k['nb'] == 1 and k['entry'] == 'ddim')
    path = os.path.join(out, "step-nb1.bin")
    np.ones(c1['shape'][0], dtype=np.float32).tofile(path + ".mulin")
    runs.append(("refused-nb1", "step,-1," + S.emu_case(c1, path), c1, path, None))
    return runs


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    """emu_guidance built once, every case of this file through it in one run -> (stats {name: (line, mul)}, steps [...])"""
    if not os.path.exists(CXX):
        pytest.skip("clang++ of the ROCm toolchain not available")
    out = str(tmp_path_factory.mktemp("pfd_cpu_emu_guidance"))
    subprocess.run([sys.executable, os.path.join(REPO, "tools", "cpu_emu", "build.py"), out], check=True,
                   stdout=subprocess.DEVNULL, env=dict(os.environ, EMU_ONLY="emu_guidance", EMU_OPT="-O1"))
    stats, steps = _stats_cases(out), _step_cases(out)
    args = [a for a, _, _ in stats.values()] + [r[1] for r in steps]
    r = subprocess.run([os.path.join(out, "emu_guidance"), *args], capture_output=True, text=True, timeout=900)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith(("ok", "FAIL"))]
    assert len(lines) == len(args), r.stdout[-3000:] + r.stderr[-1000:]
    got_stats = {name: (ln, R.read_mul(path, max(B, 1))) for (name, (_, B, path)), ln in zip(stats.items(), lines)}
    got_steps = []
    for (name, _, c, path, mul), ln in zip(steps, lines[len(stats):]):
        outs = tuple(np.fromfile(path + ext, dtype=dt).reshape(c[k].shape)
                     for (k, dt), ext in zip(S.OUTPUTS, (".xout", ".pred", ".xin")))
        got_steps.append((name, ln, c, mul, outs))
    return got_stats, got_steps


def test_every_case_returns_its_code_with_its_guard_bands_intact(emu):
    stats, steps = emu
    for name, (ln, _) in stats.items():
        assert ln.startswith("ok") and "OUTSIDE" not in ln, (name, ln)
    for name, ln, *_ in steps:
        assert ln.startswith("ok") and "OUTSIDE" not in ln, (name, ln)


@pytest.mark.parametrize("shape,B", GRID, ids=[f"{'x'.join(map(str, s))}-B{b}" for s, b in GRID])
def test_statistics_kernel_meets_the_specification_within_the_derived_bound(emu, shape, B):
    eps, s, phi = R.make_eps(B, shape), R.rows(R.SCALES, B), R.rows(R.PHIS, B)
    ln, mul = emu[0][f"grid-{'x'.join(map(str, shape))}-B{B}"]
    n = int(np.prod(shape))
    assert ln.endswith("guidance_rescale_kernel<%s>" % ("true" if n % 8 == 0 else "false")), ln
    f = G.factor(eps, s, phi)
    e = R.rel_err(mul, f)
    print(f"[guidance emu] {shape} B {B}: |mul - f| / f = {e / 2.0 ** -24:.2f} x 2^-24, bound {R.bound(shape) / 2.0 ** -24:.0f} x 2^-24")
    assert e <= R.bound(shape)


def test_an_unaligned_base_takes_the_scalar_path_to_the_same_bits(emu):
    n = 0
    for shape, B in GRID:
        if shape == R.LONGEST:
            continue
        tag = f"{'x'.join(map(str, shape))}-B{B}"
        (la, a), (lo, o) = emu[0][f"grid-{tag}"], emu[0][f"off-{tag}"]
        assert lo.endswith("guidance_rescale_kernel<false>"), lo
        assert np.array_equal(a.view(np.uint32), o.view(np.uint32)), tag
        n += la.endswith("<true>")
    assert n >= 6        # the comparison crossed the two load paths


def test_a_sample_does_not_depend_on_its_company(emu):
    for shape in R.SHAPES:
        tag = f"{'x'.join(map(str, shape))}-B3"
        batch = emu[0][f"grid-{tag}"][1]
        for b in range(3):
            assert emu[0][f"alone-{tag}-{b}"][1].view(np.uint32)[0] == batch.view(np.uint32)[b], (tag, b)


def test_phi_0_writes_one_whatever_the_eps_holds_and_constant_eps_gives_one(emu):
    mul = emu[0]["phi0-nan"][1]
    assert mul[1] == np.float32(1.0) and np.all(np.isfinite(mul))
    plain = emu[0]["grid-4x8x8-B3"][1]
    assert mul.view(np.uint32)[0] == plain.view(np.uint32)[0]          # its neighbours are untouched by the NaN sample
    assert np.array_equal(emu[0]["constant"][1], np.ones(2, dtype=np.float32))


def test_strided_scale_and_phi(emu):
    eps = R.make_eps(3, (4, 8, 8))
    for ss, ps in ((0, 1), (1, 0), (13, 1), (1, 13), (0, 0), (13, 13)):
        s = np.full(3, 7.5, dtype=np.float32) if ss == 0 else R.rows(R.SCALES, 3)
        phi = np.full(3, 0.7, dtype=np.float32) if ps == 0 else R.rows(R.PHIS, 3)
        mul = emu[0][f"stride-{ss}-{ps}"][1]
        assert R.rel_err(mul, G.factor(eps, s, phi)) <= R.bound((4, 8, 8)), (ss, ps)
    assert np.array_equal(emu[0]["stride-13-13"][1].view(np.uint32), emu[0]["grid-4x8x8-B3"][1].view(np.uint32))


def test_statistics_kernel_refuses_bad_arguments(emu):
    bad = [k for k in emu[0] if k.startswith("bad-")]
    assert len(bad) == 10
    for k in bad:
        assert " rc -1 (expected -1)" in emu[0][k][0], emu[0][k][0]


def test_step_mul_with_ones_reproduces_the_recorded_bits_of_all_ten_instantiations(emu):
    seen = set()
    for name, ln, c, mul, outs in emu[1]:
        if not name.startswith("ones-"):
            continue
        assert ln.endswith("| " + S.kernel_of(c)) and " rc 0 " in ln and " launches 1" in ln, ln
        seen.add(S.kernel_of(c))
        for (k, _), g in zip(S.OUTPUTS, outs):
            assert np.array_equal(g.reshape(-1), c[k].reshape(-1)), f"{name}: {k} differs from the recording"
    assert len(seen) == 10


def test_step_mul_with_factors_meets_the_fp64_formula(emu):
    n = 0
    for name, ln, c, mul, outs in emu[1]:
        if not name.startswith("mul-"):
            continue
        n += 1
        B, C, h, w = c['shape']
        eps64 = c['eps'].astype(np.float64) * np.concatenate([mul, mul]).astype(np.float64)[:, None, None, None]
        ref = S.specification(dict(c, eps=eps64))       # the guided eps is linear in eps: mul_b (eu + s (ec - eu))
        xout, pred, xin = outs[0].view(np.float32), outs[1].view(np.float32), outs[2].view(np.float16)
        e = max(IR.scaled_err(xout, ref[0]), IR.scaled_err(pred, ref[1]))
        plain = S.specification(c)
        moved = IR.scaled_err(ref[1], plain[1])
        print(f"[guidance emu] {name}: err {e:.2e} (TOL {IR.TOL:g}); the factors move pred_x0 by {moved:.2e}")
        assert e <= IR.TOL and moved >= R.MUTANT_MARGIN * IR.TOL
        assert np.array_equal(xin.reshape(B, h, w, C), np.transpose(xout, (0, 2, 3, 1)).astype(np.float16))
    assert n == 10


def test_step_mul_refuses_what_it_must(emu):
    names = {name: ln for name, ln, *_ in emu[1] if name.startswith("refused-")}
    assert set(names) == {"refused-null-mul", "refused-nb1"}
    for ln in names.values():
        assert " rc -1 (expected -1) launches 0" in ln, ln


# ---- header, binding, ops -----------------------------------------------------------------------------------------------------
def test_header_declares_and_binding_lists_the_two_entry_points():
    from lib.hip import binding
    header = open(os.path.join(REPO, "include", "pfd_hip.h")).read()
    assert "Lin et al. 2023" in header and "rescale_noise_cfg" in header
    for name, nargs in (("pfd_guidance_rescale_f32", 9), ("pfd_cfg_step_mul", 26)):
        assert f"int {name}(" in header and len(binding.SIGNATURES[name][1]) == nargs
    assert binding.ABI_VERSION == 10 and "#define PFD_ABI_VERSION 10" in header


def test_ops_wrappers_check_their_operands_before_the_library(monkeypatch):
    from lib.hip import ops
    monkeypatch.setattr(ops, "_lib", lambda: pytest.fail("the library was reached"))
    eps = torch.zeros(4, 2, 2, 4, dtype=torch.float16)
    with pytest.raises(ValueError, match="guidance_rescale"):
        ops.guidance_rescale(eps[:3], torch.ones(1), torch.ones(2))
    with pytest.raises(ValueError, match="guidance_rescale"):
        ops.guidance_rescale(eps.float(), torch.ones(1), torch.ones(2))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.guidance_rescale(eps, torch.ones(1), torch.ones(2))


# ---- the sampler on the stand-in ------------------------------------------------------------------------------------------
def _sampler(monkeypatch):
    from lib.model_zoo.ddim import DDIMSampler
    GS.install(monkeypatch)
    return DDIMSampler(SS.StubModel())


def _infos(bs=2, phi=None, scale=2.5, key=False):
    g = torch.Generator().manual_seed(7)
    x_info = {'type': 'image', 'xt': torch.randn(bs, 4, 3, 5, generator=g)}
    if key:
        from lib import noise
        x_info['noise_key'] = torch.from_numpy(noise.sample_keys(99, 5, bs))
    c = {'type': 'image', 'conditioning': torch.randn(bs, 3, 8, generator=g).half(), 'unconditional_guidance_scale': scale,
         'unconditional_conditioning': torch.randn(bs, 3, 8, generator=g).half()}
    if phi is not None:
        c['guidance_rescale'] = phi
    return x_info, c


def _run(monkeypatch, steps=4, **kw):
    how = {k: kw.pop(k) for k in ('solver', 'eta') if k in kw}
    s = _sampler(monkeypatch)
    x_info, c = _infos(**kw)
    x, _ = s.sample(steps, [2, 4, 3, 5], x_info, c, verbose=False, **how)
    return x, list(SS.LOG), GS.launches()


def test_default_spellings_leave_the_launch_sequence_unchanged(monkeypatch):
    x0, log0, _ = _run(monkeypatch)
    assert not any("guidance_rescale" in ln or "eps_mul" in ln for ln in log0)
    for phi in (0.0, [0.0, 0.0], torch.zeros(2), np.zeros(2)):
        x, log, _ = _run(monkeypatch, phi=phi)
        assert log == log0 and torch.equal(x, x0)
    # no unconditional half: phi means nothing and the run is the plain scale-1 run
    x1, log1, _ = _run(monkeypatch, scale=1.0)
    x, log, _ = _run(monkeypatch, scale=1.0, phi=0.7)
    assert log == log1 and torch.equal(x, x1)
    # ... and over the sampler's own stand-ins, whose step functions have no eps_mul keyword at all
    from lib.model_zoo.ddim import DDIMSampler
    SS.install(monkeypatch)
    x_info, c = _infos(phi=[0.0, 0.0])
    assert torch.equal(DDIMSampler(SS.StubModel()).sample(4, [2, 4, 3, 5], x_info, c, verbose=False)[0], x0)
    assert list(SS.LOG) == log0


@pytest.mark.parametrize("how", [dict(), dict(solver='dpmpp_2m'), dict(eta=1.0, key=True), dict(scale=[2.0, 7.5])],
                         ids=["ddim", "dpmpp_2m", "keyed-eta1", "per-sample-scale"])
def test_a_rescaled_request_is_two_launches_per_step(monkeypatch, how):
    x0, _, plain = _run(monkeypatch, **how)
    x, log, seq = _run(monkeypatch, phi=[0.7, 0.25], **how)
    step = "cfg_dpmpp_step" if how.get('solver') else "cfg_ddim_step"
    assert plain == [step] * 4 and seq == ["guidance_rescale", step + " eps_mul"] * 4
    assert not torch.equal(x, x0) and bool(torch.isfinite(x).all())
    stats = [ln for ln in log if ln.startswith("guidance_rescale")]
    per_sample = isinstance(how.get('scale'), list)
    assert all(f"scales={2 if per_sample else 1} phi=[0.7, 0.25]" in ln for ln in stats), stats
    # one number is that number for every sample; a sample with phi 0 among others keeps the two-launch path
    assert torch.equal(_run(monkeypatch, phi=0.7, **how)[0], _run(monkeypatch, phi=[0.7, 0.7], **how)[0])
    assert _run(monkeypatch, phi=[0.0, 0.7], **how)[2] == seq


def test_the_factor_the_step_receives_is_the_specifications(monkeypatch):
    """the stand-in's statistics on the first step's eps against lib/guidance.py, and the scale it is handed is the row's"""
    from lib.hip import ops
    seen = []
    GS.install(monkeypatch)
    inner = ops.guidance_rescale

    def spy(eps, sc, phi):
        mul = inner(eps, sc, phi)
        seen.append((eps.clone(), sc.clone(), phi.clone(), mul.clone()))
        return mul
    monkeypatch.setattr(ops, "guidance_rescale", spy)
    from lib.model_zoo.ddim import DDIMSampler
    x_info, c = _infos(phi=[0.7, 0.25], scale=7.5)
    DDIMSampler(SS.StubModel()).sample(4, [2, 4, 3, 5], x_info, c, verbose=False)
    assert len(seen) == 4
    eps, sc, phi, mul = seen[0]
    assert sc.numel() == 1 and float(sc) == 7.5 and phi.tolist() == [np.float32(0.7), 0.25]
    assert R.rel_err(mul.numpy(), G.factor(eps.numpy(), 7.5, phi.numpy())) < 1e-5


def test_sampler_checks_phi(monkeypatch):
    for bad in (-0.1, 1.01, [0.5], [0.5, 0.5, 0.5], float('nan'), 'x'):
        s = _sampler(monkeypatch)
        x_info, c = _infos(phi=bad)
        with pytest.raises(ValueError, match="guidance_rescale"):
            s.sample(4, [2, 4, 3, 5], x_info, c, verbose=False)


class _OnDevice(torch.Tensor):
    """a CPU tensor that says it is on the device: the sampler then takes its graph branch, whose capture the test replaces"""
    is_cuda = property(lambda self: True)


def _graph_keys(monkeypatch, **kw):
    from lib.model_zoo.ddim import DDIMSampler
    s = _sampler(monkeypatch)
    keys, inputs_seen = [], []

    class _Loop:
        def __init__(self, run_loop):
            self.run_loop = run_loop

        def replay(self, inputs):
            inputs_seen.append(inputs)
            return self.run_loop(*inputs)

    start = DDIMSampler._start_latent
    monkeypatch.setattr(DDIMSampler, "_start_latent", lambda self, *a: (lambda x, t: (x.as_subclass(_OnDevice), t))(*start(self, *a)))
    monkeypatch.setattr(DDIMSampler, "_weights_signature", lambda self: 0)
    monkeypatch.setattr(DDIMSampler, "_capture", lambda self, run_loop, t_table, inputs, coef: _Loop(run_loop))
    graph_for = DDIMSampler._graph_for
    monkeypatch.setattr(DDIMSampler, "_graph_for", lambda self, key, capture: (keys.append(key), graph_for(self, key, capture))[1])
    s.enable_graph(True)
    x_info, c = _infos(**kw)
    out, _ = s.sample(4, [2, 4, 3, 5], x_info, c, verbose=False)
    return keys[0], torch.Tensor(out), inputs_seen[0]


def test_graph_key_gains_rescale_only_when_present_and_phi_is_an_input(monkeypatch):
    plain, xp, inputs0 = _graph_keys(monkeypatch)
    assert _graph_keys(monkeypatch, phi=0.0)[0] == plain and _graph_keys(monkeypatch, phi=[0.0, 0.0])[0] == plain
    key, x, inputs = _graph_keys(monkeypatch, phi=[0.7, 0.25])
    assert key[-1] == ('rescale',) and key[:-1] == plain and ('rescale',) not in plain
    assert len(inputs0) == 5 and len(inputs) == 13 and all(t is None for t in inputs[5:12])
    assert inputs[12].dtype == torch.float32 and inputs[12].tolist() == [np.float32(0.7), 0.25]
    assert _graph_keys(monkeypatch, phi=[0.1, 0.9])[0] == key          # another phi: the same graph
    assert torch.equal(_run(monkeypatch, phi=[0.7, 0.25])[0], x)        # the graphed branch computes what the eager one does


def test_single_step_takes_it_and_multicontext_refuses(monkeypatch):
    t = torch.full((2,), 501, dtype=torch.long)

    def one(phi):
        s = _sampler(monkeypatch)
        s.make_schedule(4, verbose=False)
        x_info, c = _infos(phi=phi)
        x_info['x'] = x_info['xt'].half()
        return s.p_sample_ddim(x_info, c, t, 2), GS.launches()
    (xp, p0), seq = one([0.7, 0.25])
    (xq, q0), plain = one(None)
    assert seq == ["guidance_rescale", "cfg_ddim_step eps_mul"] and plain == ["cfg_ddim_step"]
    assert not torch.equal(xp, xq) and not torch.equal(p0, q0)
    assert one(0.0)[1] == plain and torch.equal(one([0.0, 0.0])[0][0], xq)
    s = _sampler(monkeypatch)
    s.make_schedule(4, verbose=False)
    x_info, c = _infos(phi=0.7)
    x_info['x'] = x_info['xt'].half()
    cl = [dict(c, ratio=0.5), dict(c, ratio=0.5)]
    for call in (lambda: s.p_sample_ddim_multicontext(x_info, cl, t, 2),
                 lambda: s.sample_multicontext(4, [2, 4, 3, 5], x_info, cl, verbose=False),
                 lambda: s.ddim_sampling_multicontext([2, 4, 3, 5], x_info, cl)):
        with pytest.raises(ValueError, match="takes no c_info\\['guidance_rescale'\\]"):
            call()


# ---- pipeline and server ---------------------------------------------------------------------------------------------------
IMG = torch.rand(1, 3, 64, 64)


class _Seen:
    def __init__(self):
        self.c = None

    def enable_graph(self, on=True):
        pass

    def sample(self, steps, shape, x_info, c_info, eta=0., verbose=True):
        self.c = dict(c_info)
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


@pytest.mark.parametrize("bad", [-0.5, 1.5, float('nan'), [0.5, 0.5, 0.5], 'x'], ids=str)
def test_generate_checks_phi_before_the_device(bad):
    pipe, _ = _pipe(touch_ok=False)
    with pytest.raises(ValueError, match="guidance_rescale"):
        pipe.generate(IMG, 2, 64, 64, steps=4, decode=False, guidance_rescale=bad)


def test_generate_hands_the_sampler_phi_only_when_something_is_left_of_it():
    pipe, seen = _pipe()
    for plain in (dict(), dict(guidance_rescale=0.0), dict(guidance_rescale=[0, 0]), dict(guidance_rescale=0.7, scale=1.0)):
        pipe.generate(IMG, 2, 64, 64, steps=4, decode=False, **plain)
        assert 'guidance_rescale' not in seen.c, plain
    pipe.generate(IMG, 2, 64, 64, steps=4, decode=False, guidance_rescale=0.7)
    assert seen.c['guidance_rescale'].dtype == torch.float32 and seen.c['guidance_rescale'].tolist() == [np.float32(0.7)] * 2
    pipe.generate(IMG, 2, 64, 64, steps=4, decode=False, guidance_rescale=[0.0, 0.25], scale=[1.0, 7.5])
    assert seen.c['guidance_rescale'].tolist() == [0.0, 0.25]


def test_phi_is_sharded_like_the_guidance_scale():
    phi = [0.7, 0.25, 0.0, 1.0]
    for rank in range(2):
        pipe, seen = _pipe(rank, 2)
        pipe.generate(IMG, 4, 64, 64, steps=4, decode=False, guidance_rescale=phi)
        assert seen.c['guidance_rescale'].tolist() == [float(np.float32(v)) for v in phi[2 * rank:2 * rank + 2]]
        with pytest.raises(ValueError, match="guidance_rescale"):      # the whole vector is checked on every rank
            pipe.generate(IMG, 4, 64, 64, steps=4, decode=False, guidance_rescale=[0.7, 0.25, 0.0, 1.5])
        with pytest.raises(ValueError, match="guidance_rescale"):
            pipe.generate(IMG, 4, 64, 64, steps=4, decode=False, guidance_rescale=[0.7, 0.25])
    pipe, seen = _pipe(1, 2)                       # a rank whose samples all have phi 0 runs the plain request
    pipe.generate(IMG, 4, 64, 64, steps=4, decode=False, guidance_rescale=[0.7, 0.25, 0.0, 0.0])
    assert 'guidance_rescale' not in seen.c


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


SHARING = [
    # requests with rescale share a batch whatever their phi; one without never joins them
    (dict(), [dict(guidance_rescale=0.7), dict(guidance_rescale=0.25), dict()], [[1, 2], [3]]),
    (dict(), [dict(), dict(guidance_rescale=0.7), dict()], [[1], [2], [3]]),
    # 0, and scale 1, is the request without it
    (dict(), [dict(), dict(guidance_rescale=0.0), dict(guidance_rescale=[0.0])], [[1, 2, 3]]),
    (dict(), [dict(scale=1.0), dict(scale=1.0, guidance_rescale=0.7)], [[1, 2]]),
    # a mixed server: scales and phi both differ inside one batch
    (dict(mixed_batches=True), [dict(scale=7.5, guidance_rescale=0.7), dict(scale=3.0, guidance_rescale=0.2), dict(scale=3.0)],
     [[1, 2], [3]]),
]


@pytest.mark.parametrize("case", range(len(SHARING)))
def test_server_batch_sharing(monkeypatch, case):
    how, submits, want = SHARING[case]
    srv, calls = _server(monkeypatch, **how)
    try:
        outs = _queued(srv, [dict(k, seed=i + 1) for i, k in enumerate(submits)])
        assert calls == want
        assert [float(o[0, 0]) for o in outs] == [float(i + 1) for i in range(len(submits))]
    finally:
        srv.close()


def test_request_key_gains_has_rescale_not_the_values_and_submit_checks_phi(monkeypatch):
    from lib import serving
    kw = dict(image=IMG, n=1, height=64, width=64, steps=4, seed=1, eta=0.0)
    R_ = serving._Request
    assert R_(scale=1.5, **kw).key() == (64, 64, 4, 1.5, 0.0, True, True, False, False)
    a, b = R_(scale=1.5, rescale=np.float32([0.7]), **kw), R_(scale=1.5, rescale=np.float32([0.2]), **kw)
    assert a.key() == b.key() == (64, 64, 4, 1.5, 0.0, True, True, False, False, 'rescale')
    srv, calls = _server(monkeypatch)
    try:
        for bad in (-0.5, 1.5, float('nan'), [0.5, 0.5], 'x'):
            with pytest.raises(ValueError, match="guidance_rescale"):
                srv.submit(IMG, 1, 64, 64, steps=4, guidance_rescale=bad)
        assert calls == []
    finally:
        srv.close()


def test_server_generate_gives_each_sample_its_phi():
    """the real `_generate` over stand-ins for the device work"""
    from stubs import StubNet
    from lib import serving
    seen = _Seen()
    kw = dict(image=IMG, height=64, width=64, steps=4, eta=0.0, as_uint8=False, future=None, mixed=True)
    srv = serving.PromptFreeServer(StubNet(), use_graph=False, max_batch=8, mixed_batches=True)
    try:
        srv.pipe.sampler = seen
        Rq = serving._Request
        srv._generate([Rq(n=2, seed=1, scale=2.0, rescale=np.float32([0.7, 0.0]), **kw),
                       Rq(n=1, seed=2, scale=3.0, rescale=np.float32([0.25]), **kw)])
        assert seen.c['guidance_rescale'].tolist() == [np.float32(0.7), 0.0, 0.25]
        assert seen.c['unconditional_guidance_scale'].tolist() == [2.0, 2.0, 3.0]
        srv._generate([Rq(n=1, seed=1, scale=2.0, **kw)])
        assert 'guidance_rescale' not in seen.c
    finally:
        srv.close()
