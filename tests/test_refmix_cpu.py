"""CPU: several references mixed in one UNet pass (lib/refmix.py) below the GPU -- the fp64 specification and its properties,
key_bias, the named mutants against the tolerance of the GPU kernel tests, the torch reference the GPU tests use against the
numpy specification, the biased kernels of all four classes on the CPU emulation, and the host layers over stand-ins: the
sampler (tests/sampler_standin.py), PromptFreePipeline.generate and PromptFreeServer."""
import os
import subprocess
import sys
import threading

import numpy as np
import pytest
import torch

import refmix_refs as RR
import sampler_standin as SS
from lib import refmix

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get("EMU_CXX", "/opt/rocm/lib/llvm/bin/clang++")


# ------------------------------------------------------------------------------------------------
# the specification
# ------------------------------------------------------------------------------------------------
def _rand(B=2, H=2, Nq=5, Nk=12, D=8, seed=0):
    g = np.random.default_rng(seed)
    return g.standard_normal((B, H, Nq, D)), g.standard_normal((B, H, Nk, D)), g.standard_normal((B, H, Nk, D))


def _bias(B, Nk, seed=1, holes=True):
    g = np.random.default_rng(seed)
    b = -12.0 * g.random((B, Nk))
    if holes:
        b[:, 3::4] = -np.inf
    return b


def test_shifting_every_bias_changes_nothing():
    q, k, v = _rand()
    b = _bias(2, 12)
    o = refmix.weighted_attention(q, k, v, b, 0.35)
    for shift in (-7.5, 3.0, 100.0):
        assert np.abs(refmix.weighted_attention(q, k, v, b + shift, 0.35) - o).max() <= 1e-13


def test_keys_doubled_at_minus_one_equal_the_original():
    q, k, v = _rand()
    b = _bias(2, 12)
    o = refmix.weighted_attention(q, k, v, b, 0.35)
    o2 = refmix.weighted_attention(q, np.concatenate([k, k], 2), np.concatenate([v, v], 2), np.concatenate([b, b], 1) - 1.0, 0.35)
    assert np.abs(o2 - o).max() <= 1e-13


def test_a_masked_key_equals_the_key_removed_whatever_it_holds():
    q, k, v = _rand()
    b = _bias(2, 12)
    live = np.isfinite(b[0])
    assert np.array_equal(live, np.isfinite(b[1]))
    o = refmix.weighted_attention(q, k, v, b, 0.35)
    short = refmix.weighted_attention(q, k[:, :, live], v[:, :, live], b[:, live], 0.35)
    assert np.abs(o - short).max() <= 1e-13
    k2, v2 = k.copy(), v.copy()
    k2[:, :, ~live], v2[:, :, ~live] = 1e30, np.nan                   # exactly nothing
    assert np.array_equal(refmix.weighted_attention(q, k2, v2, b, 0.35), o)


def test_the_order_of_the_keys_is_immaterial_and_the_weights_mean_what_they_say():
    q, k, v = _rand()
    b = _bias(2, 12)
    perm = np.random.default_rng(5).permutation(12)
    o = refmix.weighted_attention(q, k, v, b, 0.35)
    assert np.abs(refmix.weighted_attention(q, k[:, :, perm], v[:, :, perm], b[:, perm], 0.35) - o).max() <= 1e-13
    # two references of 6 tokens: (1/2, 1/2) of the same reference is that reference; only the ratio of the weights matters
    one = refmix.weighted_attention(q, k[:, :, :6], v[:, :, :6], np.zeros((2, 6)), 0.35)
    kk, vv = np.concatenate([k[:, :, :6]] * 2, 2), np.concatenate([v[:, :, :6]] * 2, 2)
    half = np.stack([refmix.key_bias([0.5, 0.5], 6, 12)] * 2).astype(np.float64)
    assert np.abs(refmix.weighted_attention(q, kk, vv, half, 0.35) - one).max() <= 1e-13
    a = np.stack([refmix.key_bias([0.7, 0.3], 6, 12)] * 2)
    c = np.stack([refmix.key_bias([7.0, 3.0], 6, 12)] * 2)
    assert np.array_equal(a, c)
    swapped = np.stack([refmix.key_bias([0.3, 0.7], 6, 12)] * 2).astype(np.float64)
    ks, vs = np.concatenate([k[:, :, 6:], k[:, :, :6]], 2), np.concatenate([v[:, :, 6:], v[:, :, :6]], 2)
    assert np.abs(refmix.weighted_attention(q, ks, vs, swapped, 0.35) - refmix.weighted_attention(q, k, v, a.astype(np.float64), 0.35)).max() <= 1e-13


def test_key_bias_layout_checks_and_exact_zeros():
    b = refmix.key_bias([0.7, 0.3], 148, 296)
    assert b.dtype == np.float32 and b.shape == (296,)
    assert np.all(b[:148] == 0.0) and np.all(b[148:] == np.float32(np.log2(0.3 / 0.7)))
    b = refmix.key_bias([0.2, 0.5, 0.3], 3, 16)
    assert np.all(b[3:6] == 0.0) and np.all(np.isneginf(b[9:])) and np.all(np.isfinite(b[:9]))
    assert np.array_equal(b[:3], np.full(3, np.float32(np.log2(0.2 / 0.5))))
    assert np.array_equal(refmix.key_bias([3.5], 148, 152), np.r_[np.zeros(148), np.full(4, -np.inf)].astype(np.float32))
    for bad in ([], [1.0] * 9, [1.0, np.nan], [1.0, np.inf], [1.0, -0.5], [1.0, 0.0], [0.0]):
        with pytest.raises(ValueError):
            refmix.key_bias(bad, 2, 64)
    with pytest.raises(ValueError, match="dropped"):
        refmix.key_bias([1.0, 0.0], 2, 64)
    with pytest.raises(ValueError, match="do not fit"):
        refmix.key_bias([1.0, 1.0], 5, 9)
    assert refmix.drop_zero_weights([0.0, 2.0, 0.0, 1.0])[0] == [1, 3]
    for bad in ([0.0, 0.0], [1.0, -1.0], [1.0] * 9, [np.nan]):
        with pytest.raises(ValueError):
            refmix.drop_zero_weights(bad)
    q, k, v = _rand(Nk=4)
    for bad in (np.full((2, 4), -np.inf), np.full((2, 4), np.nan), np.full((2, 4), np.inf), np.zeros((2, 5))):
        with pytest.raises(ValueError):
            refmix.weighted_attention(q, k, v, bad, 0.35)


# ------------------------------------------------------------------------------------------------
# the reference of the GPU tests is the specification; the mutants are far from it
# ------------------------------------------------------------------------------------------------
SMALL = [("w4", (1, 2, 130, 129, 40)), ("w4", (1, 1, 33, 1, 40)), ("d80", (1, 2, 150, 296, 80)), ("d160", (2, 2, 64, 296, 160))]


@pytest.mark.parametrize("pattern", RR.PATTERNS)
@pytest.mark.parametrize("cls,case", SMALL, ids=lambda v: v if isinstance(v, str) else RR.case_id(v))
def test_torch_reference_is_the_numpy_specification(cls, case, pattern):
    """refmix_refs.weighted_ref (fp64 torch, strided operands: what the GPU tests compare with) against
    lib/refmix.weighted_attention on the same operands; the poisoned pad columns reach neither"""
    p = RR.problem(case)
    B, H, Nq, Nk, D = p["dims"]
    bias = RR.bias_rows(case, pattern)
    ref, T = RR.weighted_ref(p["q"], p["k"], p["vt"], bias, B, H, Nq, Nk, D, p["scale"], **p["desc"])
    q, k, v = RR.to_spec(p["q"], p["k"], p["vt"], B, H, Nq, Nk, D, p["desc"])
    spec = refmix.weighted_attention(q, k, v, bias[:, :Nk].double().numpy(), p["scale"])
    got = ref.view(B, Nq, H, D).permute(0, 2, 1, 3).numpy()
    assert np.isfinite(got).all() and np.abs(got - spec).max() <= 1e-12
    reff, _ = RR.weighted_ref(p["q"], p["k"], p["vt"], bias, B, H, Nq, Nk, D, p["scale"], **p["desc"], folded=True)
    assert float((reff - ref).abs().max()) <= RR.kbias_bound(Nk, D, p["vmax"], T, RR.bias_max(bias, Nk), 40.0)


def test_dispatch_restated_and_cases_reach_their_classes():
    import kernel_refs as KR
    for cls, c in RR.ALL_CASES:
        assert RR.kbias_kernel_class(*c) == cls
        assert KR.attention_kernel_class(*c) == cls          # the zero-bias bit comparison runs the same class on both sides
    assert RR.kbias_kernel_class(32, 8, 256, 128, 40) == "w4" and KR.attention_kernel_class(32, 8, 256, 128, 40) == "a3"
    assert RR.kbias_kernel_class(1, 2, 16, 16, 96) is None and RR.kbias_kernel_class(1, 1, 16, 32, 512) is None
    for c in [c for _, c in RR.ALL_CASES]:
        for pat in RR.PATTERNS:
            b = RR.bias_rows(c, pat)
            assert b.shape[1] % 4 == 0 and b.shape[1] > c[3] and bool(torch.isfinite(b[:, 0]).all())
    rag = RR.bias_rows((3, 2, 64, 296, 40), "ragged")
    assert bool(torch.isneginf(rag[0, 148:296]).all()) and bool(torch.isfinite(rag[1, :296]).all())     # tiles 3, 4 of sample 0 masked in full


@pytest.mark.parametrize("cls", RR.KBIAS_CLASSES)
@pytest.mark.parametrize("mutant", refmix.MUTANTS)
def test_every_mutant_is_a_thousand_tolerances_from_the_specification(mutant, cls):
    """on its discriminating operands (refmix_refs.discriminating; the GPU kernel tests hold the kernel to the specification
    on the same operands) the mutant differs from the specification by at least 1e3 times the bound the GPU tests use -- the
    bound is 1.5e-3 vmax, so that is 1.5 vmax: the specification says +vmax where the mutant says -vmax (or 0 / 0).  Where
    its slip cannot show, a mutant is the specification itself.  Per kernel class, at the class's head size (one head and 32
    queries of the class's problem: every head and query holds the same numbers); w8 against the reference that shares the folded
    kernel's fp16 Q' and the sharp bound, as the GPU test does."""
    p = RR.discriminating(mutant, cls, reduced=True)
    B, H, Nq, Nk, D = p["dims"]
    ref, T = RR.weighted_ref(p["q"], p["k"], p["vt"], p["bias"], B, H, Nq, Nk, D, p["scale"], **p["desc"], folded=cls == "w8")
    spec = ref.view(B, Nq, H, D).permute(0, 2, 1, 3).numpy()
    bound = RR.kbias_bound(Nk, D, p["vmax"], T, RR.bias_max(p["bias"], Nk))
    d = np.abs(RR.mutant_output(p, mutant) - spec)
    r = float(np.where(np.isnan(d), np.inf, d).max()) / bound
    print(f"[refmix] mutant {mutant}, class {cls}: {r:.0f} x the GPU bound")
    assert r >= 1e3, (mutant, r)
    # ... and is the specification where it does not apply: one reference, nothing masked, one sample
    q, k, v = _rand(B=1)
    zero = np.zeros((1, 12))
    o = refmix.weighted_attention(q, k, v, zero, 0.35)
    if mutant in refmix.ATTN_MUTANTS:
        assert np.array_equal(refmix.weighted_attention(q, k, v, zero, 0.35, wrong=mutant), o)
    else:
        assert np.array_equal(refmix.key_bias([2.0], 12, 16, wrong=mutant), refmix.key_bias([2.0], 12, 16))


# ------------------------------------------------------------------------------------------------
# the kernels on the CPU emulation
# ------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(CXX), reason="clang++ of the ROCm toolchain not available")
def test_biased_kernels_of_all_four_classes_on_the_emulation(tmp_path):
    """tools/cpu_emu/emu_attn --kbias: pfd_attention_kbias_f16 through the real dispatcher -- the 8-wave folded d = 40 form,
    d = 80, d = 160, and (--w4) the 4-wave d = 40 form -- with tiles masked in full, holes and NaN behind the keys, against the
    weighted softmax in double precision"""
    env = dict(os.environ, EMU_ONLY="emu_attn")
    subprocess.run([sys.executable, os.path.join(REPO, "tools", "cpu_emu", "build.py"), str(tmp_path)], check=True, env=env,
                   stdout=subprocess.DEVNULL)
    exe = os.path.join(str(tmp_path), "emu_attn")
    for extra, n, dims in ((["--kbias"], 7, {"D40", "D80", "D160"}), (["--kbias", "--w4"], 3, {"D40"})):
        r = subprocess.run([exe] + extra, capture_output=True, text=True, timeout=900)
        lines = [l for l in r.stdout.splitlines() if l.startswith(("ok", "FAIL"))]
        assert r.returncode == 0 and len(lines) == n and all(l.startswith("ok") for l in lines), r.stdout[-2000:] + r.stderr[-1000:]
        assert {w for l in lines for w in l.split() if w.startswith("D")} == dims, lines


def test_header_declares_and_binding_lists_the_entry_point():
    import re
    from lib.hip import binding
    src = open(os.path.join(REPO, "include", "pfd_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+pfd_attention_kbias_f16\s*\(([^)]*)\)\s*;", code)
    assert m and len(m.group(1).split(",")) == 4 and len(binding.SIGNATURES["pfd_attention_kbias_f16"][1]) == 4
    assert re.search(r"#define\s+PFD_ABI_VERSION\s+10\b", src) and binding.ABI_VERSION == 10
    for phrase in ("BEFORE the running maximum", "must be finite", "kb_bs % 4 == 0", "PFD_ESHAPE", "context_mixing"):
        assert phrase in src, phrase


# ------------------------------------------------------------------------------------------------
# sampler
# ------------------------------------------------------------------------------------------------
class _BiasModel(SS.StubModel):
    """the stand-in model, told about the bias: it logs it and adds its finite mean to the context's stand-in bias"""

    def prepare_context(self, c, bias=None):
        ctx = super().prepare_context(c)
        if bias is not None:
            SS.LOG.append(f"prepare_context bias={tuple(bias.shape)} {bias.dtype}")
            self.seen_bias = bias.clone()
        return ctx


@pytest.mark.parametrize("cid", [SS.CASE_IDS[0], SS.CASE_IDS[len(SS.CASE_IDS) // 2]])
def test_sampler_without_a_bias_makes_the_pinned_calls(cid, monkeypatch):
    case = {c['id']: c for c in SS.CASES}[cid]
    lines, _ = SS.run_case(case, monkeypatch)
    assert lines == SS.read_fixture()[cid]


def _sample(monkeypatch, c_extra, solver='ddim', uc='rand', scale=2.0, steps=4):
    from lib.model_zoo.ddim import DDIMSampler
    SS.install(monkeypatch)
    model = _BiasModel()
    s = DDIMSampler(model)
    g = torch.Generator().manual_seed(3)
    bs = SS.SHAPE[0]
    c = {'type': 'image', 'conditioning': torch.randn(bs, 3, 8, generator=g), 'unconditional_guidance_scale': scale}
    if uc is not None:
        c['unconditional_conditioning'] = torch.randn(bs, 3, 8, generator=g)
    c.update(c_extra)
    x_info = {'type': 'image', 'xt': torch.randn(*SS.SHAPE, generator=g)}
    x, _ = s.sample(steps, SS.SHAPE, x_info, c, eta=0., verbose=False, solver=solver)
    return model, x, list(SS.LOG)


def test_sampler_concatenates_the_bias_like_the_contexts(monkeypatch):
    bs = SS.SHAPE[0]
    kb = torch.tensor(refmix.key_bias([0.7, 0.3], 1, 3))[None].repeat(bs, 1)
    ukb = torch.tensor([[0.0, 0.0, float('-inf')]]).repeat(bs, 1)
    plain = _sample(monkeypatch, {})
    for extra, want in (({'key_bias': kb}, torch.cat([torch.zeros(bs, 3), kb])),
                        ({'key_bias': kb, 'unconditional_key_bias': ukb}, torch.cat([ukb, kb])),
                        ({'unconditional_key_bias': ukb}, torch.cat([ukb, torch.zeros(bs, 3)]))):
        for solver in ('ddim', 'dpmpp_2m'):
            model, x, log = _sample(monkeypatch, extra, solver=solver)
            assert torch.equal(model.seen_bias, want) and model.seen_bias.dtype == torch.float32
            assert sum(l.startswith("prepare_context bias") for l in log) == 1
            if solver == 'ddim':      # the stand-in's eps ignores the bias: everything else is the plain request, call for call
                assert [l for l in log if not l.startswith("prepare_context")] == plain[2] and torch.equal(x, plain[1])
    model, _, _ = _sample(monkeypatch, {'key_bias': kb}, uc=None, scale=1.0)       # no CFG: the conditional rows alone
    assert torch.equal(model.seen_bias, kb)
    for bad in (kb[:, :2], kb[:1], kb.long(), kb.tolist()):
        with pytest.raises(ValueError, match="one logit per context token"):
            _sample(monkeypatch, {'key_bias': bad})


def test_multicontext_sampling_refuses_a_bias():
    from lib.model_zoo.ddim import DDIMSampler
    s = DDIMSampler.__new__(DDIMSampler)
    s.model = None
    ci = {'unconditional_guidance_scale': 2.0, 'conditioning': torch.zeros(2, 1, 1), 'unconditional_conditioning': torch.zeros(2, 1, 1),
          'key_bias': torch.zeros(2, 1)}
    with pytest.raises(ValueError, match="key_bias"):
        s._mix_for([ci], 2)
    with pytest.raises(ValueError, match="key_bias"):
        s.sample_multicontext(2, [2, 4, 8, 8], {'type': 'image'}, [ci], verbose=False)


# ------------------------------------------------------------------------------------------------
# pipeline
# ------------------------------------------------------------------------------------------------
def _pipe(seen, fail_encode=False):
    from stubs import StubNet
    from lib.pipeline import PromptFreePipeline

    class _Net(StubNet):
        encoded = []

        def ctx_encode(self, image, which):
            if fail_encode:
                raise AssertionError("the device was touched before the arguments were checked")
            _Net.encoded.append(float(image.mean()))
            return super().ctx_encode(image, which)

    class _Sampler:
        def sample(self, steps, shape, x_info, c_info, eta=0., verbose=True, **how):
            seen.update(c_info=c_info, how=how)
            return x_info['xt'], {}

    _Net.encoded = []
    return PromptFreePipeline(_Net(), sampler=_Sampler()), _Net


def _pic(v):
    return torch.full((1, 3, 64, 64), float(v))


def test_generate_checks_its_references_before_the_device():
    pipe, _ = _pipe({}, fail_encode=True)
    A, Bp = _pic(0.25), _pic(0.5)
    bad = [dict(image=[A, Bp], image_weights=None), dict(image=A, image_weights=[1.0]), dict(image=[A, Bp], image_weights=[1.0]),
           dict(image=[A, Bp], image_weights=[1.0, -1.0]), dict(image=[A, Bp], image_weights=[0.0, 0.0]),
           dict(image=[A, Bp], image_weights=[1.0, float('nan')]), dict(image=[A] * 9, image_weights=[1.0] * 9),
           dict(image=[A, torch.zeros(2, 3, 64, 64)], image_weights=[1.0, 1.0]),
           dict(image=[A, np.zeros((8, 8, 3), dtype=np.uint8)], image_weights=[1.0, 1.0])]
    for kw in bad:
        with pytest.raises(ValueError):
            pipe.generate(kw['image'], 2, 64, 64, steps=2, decode=False, image_weights=kw['image_weights'])


def test_generate_mixes_drops_and_collapses():
    seen = {}
    pipe, Net = _pipe(seen)
    A, Bp, Cp = _pic(0.25), _pic(0.5), _pic(0.75)
    pipe.generate([A, Bp, Cp], 2, 64, 64, steps=2, decode=False, image_weights=[0.5, 0.0, 0.25])
    ci = seen['c_info']
    assert Net.encoded == [0.25, 0.75]                                         # the zero-weight reference was never encoded
    assert tuple(ci['conditioning'].shape) == (2, 296, 768) and not bool(ci['unconditional_conditioning'].any())
    assert tuple(ci['unconditional_conditioning'].shape) == (2, 296, 768) and 'unconditional_key_bias' not in ci
    want = torch.from_numpy(refmix.key_bias([0.5, 0.25], 148, 296))
    assert ci['key_bias'].dtype == torch.float32 and torch.equal(ci['key_bias'], want[None].repeat(2, 1))
    assert float(ci['conditioning'][0, 0, 0]) == 0.25 and float(ci['conditioning'][1, 148, 0]) == 0.75
    # one reference left: the plain request -- no bias, the call of image=A
    Net.encoded.clear()
    pipe.generate([A, Bp], 2, 64, 64, steps=2, decode=False, image_weights=[1.0, 0.0])
    mixed = seen['c_info']
    pipe.generate(A, 2, 64, 64, steps=2, decode=False)
    plain = seen['c_info']
    assert Net.encoded == [0.25, 0.25] and set(mixed) == set(plain) and 'key_bias' not in mixed
    assert all(torch.equal(mixed[k], plain[k]) for k in ('conditioning', 'unconditional_conditioning'))
    # an uncond with fewer tokens than the mix: zero tokens at -inf behind it
    un = torch.full((1, 148, 768), 0.5)
    pipe.generate([A, Bp], 2, 64, 64, steps=2, decode=False, image_weights=[0.7, 0.3], uncond=un, solver='dpmpp_2m')
    ci = seen['c_info']
    assert tuple(ci['unconditional_conditioning'].shape) == (2, 296, 768) and seen['how'] == {'solver': 'dpmpp_2m'}
    assert bool((ci['unconditional_conditioning'][:, :148] == 0.5).all()) and not bool(ci['unconditional_conditioning'][:, 148:].any())
    ub = ci['unconditional_key_bias']
    assert tuple(ub.shape) == (2, 296) and bool((ub[:, :148] == 0).all()) and bool(torch.isneginf(ub[:, 148:]).all())
    with pytest.raises(ValueError, match="longer than the mix"):
        pipe.generate([A, Bp], 2, 64, 64, steps=2, decode=False, image_weights=[0.7, 0.3], uncond=torch.zeros(1, 300, 768))
    # the world size does not enter: each rank builds the same rows for its samples
    from lib.pipeline import PromptFreePipeline
    for rank in range(2):
        PromptFreePipeline(pipe.net, rank=rank, world_size=2, sampler=pipe.sampler).generate(
            [A, Bp], 4, 64, 64, steps=2, decode=False, image_weights=[0.7, 0.3])
        assert tuple(seen['c_info']['key_bias'].shape) == (2, 296)
        assert torch.equal(seen['c_info']['key_bias'][0], torch.from_numpy(refmix.key_bias([0.7, 0.3], 148, 296)))


# ------------------------------------------------------------------------------------------------
# server
# ------------------------------------------------------------------------------------------------
def _server(monkeypatch, max_batch=4, **kw):
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
        calls.append([r.seed for r in batch])
        return [torch.full((r.n, 1), float(r.seed)) for r in batch]

    srv._generate = fake_generate
    return srv, calls


def test_server_batches_mixed_requests_with_each_other_only(monkeypatch):
    A, Bp, Cp = _pic(0.25), _pic(0.5), _pic(0.75)
    srv, calls = _server(monkeypatch)
    try:
        gate = threading.Event()
        srv.call(lambda n: gate.wait(30))
        futs = [srv.submit([A, Bp], image_weights=[0.7, 0.3], seed=1, height=64, width=64, steps=4),
                srv.submit([A, Bp, Cp], image_weights=[0.5, 0.3, 0.2], seed=2, height=64, width=64, steps=4),
                srv.submit(A, seed=3, height=64, width=64, steps=4),
                srv.submit([A, Bp], image_weights=[1.0, 0.0], seed=4, height=64, width=64, steps=4),     # = a plain request
                srv.submit([Bp, Cp], image_weights=[1.0, 1.0], seed=5, height=64, width=64, steps=4)]
        gate.set()
        assert [float(f.result(30)[0, 0]) for f in futs] == [1.0, 2.0, 3.0, 4.0, 5.0]
        assert calls == [[1, 2], [3, 4], [5]]
        for bad in (dict(image=[A, Bp]), dict(image=A, image_weights=[1.0]), dict(image=[A, Bp], image_weights=[0.0, 0.0]),
                    dict(image=[A, torch.rand(1, 3, 16, 16)], image_weights=[1.0, 1.0])):
            with pytest.raises(ValueError):
                srv.submit(bad.pop('image'), height=64, width=64, steps=4, **bad)
    finally:
        srv.close()
    from lib import serving
    kw = dict(image=A, n=1, height=64, width=64, steps=4, seed=1, eta=0.0, scale=2.0)
    R = serving._Request
    assert R(**kw).key() == (64, 64, 4, 2.0, 0.0, True, True, False, False)                      # a plain key is what it was
    assert R(weights=[0.7, 0.3], **kw).key() == R(weights=[0.5, 0.3, 0.2], **kw).key() != R(**kw).key()


def test_server_generate_pads_to_the_longest_context_with_a_row_per_sample():
    from stubs import StubNet
    from lib import serving
    seen = {}

    class _Sampler:
        def enable_graph(self, on=True):
            pass

        def sample(self, steps, shape, x_info, c_info, eta=0., verbose=True):
            seen['c_info'] = c_info
            return x_info['xt'], {}

    A, Bp, Cp = _pic(0.25), _pic(0.5), _pic(0.75)
    kw = dict(height=64, width=64, steps=2, eta=0.0, as_uint8=False, future=None, scale=2.0)
    srv = serving.PromptFreeServer(StubNet(), use_graph=False, max_batch=8)
    try:
        srv.pipe.sampler = _Sampler()
        R = serving._Request
        outs = srv._generate([R(n=2, seed=1, image=[A, Bp], weights=[0.7, 0.3], **kw),
                              R(n=1, seed=2, image=[A, Bp, Cp], weights=[0.5, 0.3, 0.2], **kw)])
        ci = seen['c_info']
        assert [o.shape[0] for o in outs] == [2, 1] and srv.batches == [3]
        assert tuple(ci['conditioning'].shape) == (3, 444, 768) and tuple(ci['key_bias'].shape) == (3, 444)
        two = torch.from_numpy(refmix.key_bias([0.7, 0.3], 148, 444))
        assert torch.equal(ci['key_bias'][0], two) and torch.equal(ci['key_bias'][1], two)
        assert torch.equal(ci['key_bias'][2], torch.from_numpy(refmix.key_bias([0.5, 0.3, 0.2], 148, 444)))
        assert not bool(ci['conditioning'][:2, 296:].any()) and float(ci['conditioning'][2, 296, 0]) == 0.75
        assert tuple(ci['unconditional_conditioning'].shape) == (3, 444, 768) and 'unconditional_key_bias' not in ci
        # a plain request: no bias, the call it always was
        srv._generate([R(n=1, seed=3, image=A, **kw)])
        assert 'key_bias' not in seen['c_info'] and tuple(seen['c_info']['conditioning'].shape) == (1, 148, 768)
    finally:
        srv.close()
