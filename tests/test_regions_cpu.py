"""CPU: regional reference mixing (lib/regions.py) below the GPU -- the fp64 specification and its properties, region_bias against
refmix.key_bias, region_grid's integer rule, the named mutants against the tolerance of the GPU kernel tests, the torch reference
the GPU tests use against the numpy specification, pfd_attention_rbias_f16 on the CPU emulation through the real dispatcher, the
header against the binding, the registers / scratch of the new kernels, and the host layers over stand-ins: the sampler
(tests/sampler_standin.py), PromptFreePipeline.generate and PromptFreeServer (tests/stubs.py)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import refmix_refs as RR
import regions_refs as GR
from lib import refmix, regions

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get("EMU_CXX", "/opt/rocm/lib/llvm/bin/clang++")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def _rand(B=2, H=2, Nq=7, Nk=12, D=8, seed=0):
    g = np.random.default_rng(seed)
    return g.standard_normal((B, H, Nq, D)), g.standard_normal((B, H, Nk, D)), g.standard_normal((B, H, Nk, D))


# ------------------------------------------------------------------------------------------------
# the specification
# ------------------------------------------------------------------------------------------------
def test_region_bias_of_one_region_is_key_bias_bit_for_bit():
    for w, t, nkp in (((0.7, 0.3), 74, 152), ((1.0,), 148, 148), ((0.2, 0.5, 0.3), 5, 16), ((3.0, 3.0), 4, 8)):
        a, b = regions.region_bias([w], t, nkp), refmix.key_bias(w, t, nkp)
        assert a.dtype == np.float32 and a.shape == (1, nkp) and a[0].tobytes() == b.tobytes()


def test_region_bias_masks_a_zero_weight_and_checks_its_arguments():
    rb = regions.region_bias([[1.0, 0.0], [0.0, 2.0], [1.0, 0.25]], 3, 8)
    assert rb.shape == (3, 8) and rb.dtype == np.float32
    assert rb[0].tolist() == [0, 0, 0] + [-np.inf] * 5
    assert rb[1].tolist() == [-np.inf] * 3 + [0, 0, 0] + [-np.inf] * 2       # the whole first reference masked, not dropped
    assert rb[2].tolist() == [0, 0, 0, -2, -2, -2, -np.inf, -np.inf]
    for bad in ([[1.0, 0.0], [0.0, 0.0]], [[-1.0, 1.0]], [[np.nan, 1.0]], [1.0, 2.0], [[1.0]] * 9, [[1.0] * 9]):
        with pytest.raises(ValueError):
            regions.region_bias(bad, 1, 16)
    with pytest.raises(ValueError, match="do not fit"):
        regions.region_bias([[1.0, 1.0]], 5, 9)
    keep, w = regions.drop_zero_columns([[1.0, 0.0, 0.5], [0.0, 0.0, 2.0]])
    assert keep == [0, 2] and w.tolist() == [[1.0, 0.5], [0.0, 2.0]]


def test_region_grid_is_the_identity_at_the_maps_own_size_and_follows_the_integer_rule():
    g = np.random.default_rng(3)
    m = g.integers(0, 5, size=(7, 11), dtype=np.uint8)
    assert np.array_equal(regions.region_grid(m, 7, 11), m.reshape(-1))
    for (Hm, Wm), (h, w) in (((7, 11), (3, 5)), ((13, 9), (64, 64)), ((5, 5), (8, 3)), ((1, 1), (4, 4)), ((512, 384), (8, 6))):
        m = g.integers(0, 8, size=(Hm, Wm), dtype=np.uint8)
        got = regions.region_grid(m, h, w)
        assert got.dtype == np.uint8 and got.shape == (h * w,)
        for y in range(h):
            for x in range(w):      # Python integers: no float picks an index
                assert int(got[y * w + x]) == int(m[((2 * y + 1) * Hm) // (2 * h)][((2 * x + 1) * Wm) // (2 * w)])
    # every level from the user's map, not from the level above: a one-pixel-wide stripe survives where the centre hits it
    m = np.zeros((8, 8), dtype=np.uint8)
    m[:, 3] = 1
    assert regions.region_grid(m, 8, 8).reshape(8, 8)[:, 3].all() and not regions.region_grid(m, 4, 4).reshape(4, 4)[:, 0].any()
    assert regions.region_grid(m, 4, 4).reshape(4, 4)[:, 1].all()            # centre of cell 1 is pixel (2 + 1) * 8 // 8 = 3


def test_region_grid_raises_on_an_id_out_of_range_and_on_a_wrong_picture():
    m = np.zeros((4, 4), dtype=np.uint8)
    m[3, 3] = 2
    regions.region_grid(m, 2, 2, nr=3)
    with pytest.raises(ValueError, match="only 2 regions"):
        regions.region_grid(m, 2, 2, nr=2)       # although no cell centre of the 2 x 2 grid lands on that pixel... the MAP is checked
    for bad in (m.astype(np.int32), m[0], m[:0]):
        with pytest.raises(ValueError):
            regions.region_grid(bad, 2, 2)


def test_regional_attention_is_weighted_attention_region_by_region():
    q, k, v = _rand()
    g = np.random.default_rng(5)
    tab = -12.0 * g.random((2, 3, 12))
    tab[:, 1, :6] = -np.inf                        # region 1 starts on key 6
    tab[:, 2, 3::4] = -np.inf
    qreg = np.stack([(np.arange(7) + b) % 3 for b in range(2)])
    o = regions.regional_attention(q, k, v, tab, qreg, 0.35)
    for r in range(3):
        one = refmix.weighted_attention(q, k, v, tab[:, r], 0.35)
        for b in range(2):
            sel = qreg[b] == r
            assert np.abs(o[b][:, sel] - one[b][:, sel]).max() <= 1e-14
    # a shared map is the same map for every sample; NaN in K / V of a masked key of EVERY region is a contract matter, V of a
    # key masked for the query at hand is not read
    assert np.array_equal(regions.regional_attention(q, k, v, tab, qreg[0], 0.35)[0], o[0])
    with pytest.raises(ValueError, match="no finite key"):
        bad = tab.copy()
        bad[1, 2] = -np.inf
        regions.regional_attention(q, k, v, bad, np.full((2, 7), 2), 0.35)
    with pytest.raises(ValueError, match="region ids"):
        regions.regional_attention(q, k, v, tab, np.full((2, 7), 3), 0.35)


# ------------------------------------------------------------------------------------------------
# the reference of the GPU tests is the specification; the mutants are far from it
# ------------------------------------------------------------------------------------------------
SMALL = [("w4", (1, 2, 130, 129, 40)), ("w4", (3, 2, 64, 296, 40)), ("d80", (1, 2, 150, 296, 80)), ("d160", (2, 2, 64, 296, 160))]
_ids = lambda v: v if isinstance(v, str) else GR.case_id(v) if isinstance(v, tuple) else str(v)     # noqa: E731


@pytest.mark.parametrize("shared", [True, False])
@pytest.mark.parametrize("cls,case", SMALL, ids=_ids)
def test_torch_reference_is_the_numpy_specification(cls, case, shared):
    p = GR.problem(case)
    B, H, Nq, Nk, D = p["dims"]
    tab, qreg = GR.table(case), GR.region_map(case, shared)
    ref, T = GR.regional_ref(p["q"], p["k"], p["vt"], tab, qreg, B, H, Nq, Nk, D, p["scale"], **p["desc"])
    q, k, v = RR.to_spec(p["q"], p["k"], p["vt"], B, H, Nq, Nk, D, p["desc"])
    spec = regions.regional_attention(q, k, v, tab[..., :Nk].double().numpy(), qreg.numpy().astype(np.int64), p["scale"])
    got = ref.view(B, Nq, H, D).permute(0, 2, 1, 3).numpy()
    assert np.isfinite(got).all() and np.abs(got - spec).max() <= 1e-12 and 0 < T < 60


def test_dispatch_restated_tables_and_maps():
    # one build per head size, 4 waves: what the entry point launched in the pinned dry run of the host code, under every test hook
    pinned = open(os.path.join(REPO, "tests", "golden", "attention_dispatch.txt")).read()
    launched = set(re.findall(r"^rbias .* \| (\S+<.*>) grid", pinned, re.M))
    assert launched == {f"attention_rbias_kernel<{D}, 4, false, false>" for D in (40, 80, 160)} and pinned.count("# hooks: ") == 4
    for cls, c in GR.ALL_CASES:
        assert GR.rbias_kernel_class(*c) == cls and RR.kbias_kernel_class(*c) == cls       # the bit comparison runs one class
        assert c in RR.KBIAS_CASES[cls]
        tab = GR.table(c)
        Nk = c[3]
        assert tab.shape == (c[0], 8, RR.kb_stride(Nk)) and bool(torch.isfinite(tab[..., :Nk]).any(-1).all())
        assert bool(torch.isneginf(tab[:, 0, :64]).all()) and bool(torch.isneginf(tab[:, 1, -(-Nk // 64) * 64 - 64 + 0:Nk]).all())
        assert bool(torch.isfinite(tab[:, list(GR.KEY0_ROWS), 0]).all()) and len(GR.KEY0_ROWS) == 6
        for shared in (True, False):
            m = GR.region_map(c, shared)
            assert m.dtype == torch.uint8 and m.shape[-1] == c[2] and int(m.max()) == 7
            row = m if shared else m[0]
            inside = (row[1:] != row[:-1]).nonzero().flatten() + 1
            assert bool((inside % 32 != 0).any()) and (c[2] <= 32 or bool((inside % 32 == 0).any()))
    assert GR.rbias_kernel_class(1, 2, 16, 16, 96) is None and GR.rbias_kernel_class(*GR.W8_SHAPE) == "w4"


@pytest.mark.parametrize("cls", GR.RBIAS_CLASSES)
@pytest.mark.parametrize("mutant", regions.MUTANTS)
def test_every_mutant_is_a_thousand_tolerances_from_the_specification(mutant, cls):
    """on its discriminating operands (regions_refs.discriminating; the GPU kernel tests hold the kernel to the specification on
    the same operands) the mutant differs from the specification by at least 1e3 times the bound the GPU tests use: the
    specification says +vmax where the mutant says -vmax.  Where its slip cannot show, a mutant is the specification itself."""
    p = GR.discriminating(mutant, cls)
    B, H, Nq, Nk, D = p["dims"]
    ref, T = GR.regional_ref(p["q"], p["k"], p["vt"], p["table"], p["qreg"], B, H, Nq, Nk, D, p["scale"], **p["desc"])
    spec = ref.view(B, Nq, H, D).permute(0, 2, 1, 3).numpy()
    q, k, v = GR.spec_operands(p)
    assert np.abs(regions.regional_attention(q, k, np.nan_to_num(v), p["table"].double().numpy(), p["qreg"].numpy(), p["scale"]) - spec).max() <= 1e-12
    bound = GR.bound(Nk, D, p["vmax"], T, GR.table_max(p["table"], Nk))
    d = np.abs(GR.mutant_output(p, mutant) - spec)
    r = float(np.where(np.isnan(d), np.inf, d).max()) / bound
    print(f"[regions] mutant {mutant}, class {cls}: {r:.0f} x the GPU bound")
    assert r >= 1e3, (mutant, r)
    # ... and is the specification where it does not apply: one region, one sample, nothing masked / a map of the grid's own size
    q, k, v = _rand(B=1)
    tab, reg = -3.0 * np.random.default_rng(1).random((1, 1, 12)), np.zeros((1, 7), dtype=np.int64)
    if mutant in regions.ATTN_MUTANTS:
        assert np.array_equal(regions.regional_attention(q, k, v, tab, reg, 0.35, wrong=mutant), regions.regional_attention(q, k, v, tab, reg, 0.35))
    else:
        m = np.arange(36, dtype=np.uint8).reshape(6, 6) % 5
        m = np.maximum(m, m.T)                       # symmetric: the transposed grid is the grid
        assert np.array_equal(regions.region_grid(m, 6, 6, wrong=mutant), regions.region_grid(m, 6, 6))


# ------------------------------------------------------------------------------------------------
# the kernels on the CPU emulation
# ------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists(CXX), reason="clang++ of the ROCm toolchain not available")
def test_regional_kernels_of_every_class_on_the_emulation(tmp_path):
    """tools/cpu_emu/emu_attn --rbias: pfd_attention_rbias_f16 through the real dispatcher -- the 4-wave d = 40 form, d = 80,
    d = 160 -- with the first key tile masked in full for some regions (and for the only region of one case), a middle tile,
    the trailing tiles, NaN behind the keys, 1 to 8 regions, shared and per-sample maps, against double precision"""
    env = dict(os.environ, EMU_ONLY="emu_attn")
    subprocess.run([sys.executable, os.path.join(REPO, "tools", "cpu_emu", "build.py"), str(tmp_path)], check=True, env=env,
                   stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.join(str(tmp_path), "emu_attn"), "--rbias"], capture_output=True, text=True, timeout=900)
    lines = [l for l in r.stdout.splitlines() if l.startswith(("ok", "FAIL"))]
    assert r.returncode == 0 and len(lines) == 20 and all(l.startswith("ok") for l in lines), r.stdout[-2000:] + r.stderr[-1000:]
    # ... and on the operands of the named mutants (the construction of regions_refs.discriminating: the specification says
    # +-1 exactly, every mutant the opposite sign somewhere) the kernel text stays inside the bound of the GPU tests, per class
    disc = [l for l in lines if "mutant-operands" in l]
    assert len(disc) == 15 and {(l.split()[5], l.split()[6]) for l in disc} == {(str(k), f"D{D}") for k in range(5) for D in (40, 80, 160)}
    lines = [l for l in lines if "mutant-operands" not in l]
    assert {w for l in lines for w in l.split() if w.startswith("D")} == {"D40", "D80", "D160"}, lines
    assert any(" nr 8 " in l for l in lines) and any(" nr 1 " in l for l in lines)


def test_header_declares_and_binding_lists_the_entry_point():
    from lib.hip import binding
    src = open(os.path.join(REPO, "include", "pfd_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+pfd_attention_rbias_f16\s*\(([^)]*)\)\s*;", code)
    assert m, "pfd_attention_rbias_f16 is not declared"
    args = [a.strip() for a in m.group(1).split(",")]
    sig = binding.SIGNATURES["pfd_attention_rbias_f16"]
    assert len(args) == 8 and len(sig[1]) == 8
    import ctypes as C
    kinds = [C.c_int64 if a.startswith("int64_t") else C.c_int32 if a.startswith("int ") else None for a in args]
    for want, have in zip(kinds, sig[1]):
        assert want is None or want is have, (args, sig[1])
    assert re.search(r"#define\s+PFD_ABI_VERSION\s+10\b", src) and binding.ABI_VERSION == 10
    for phrase in ("at least one finite key", "rb_rs % 4 == 0", "PFD_ESHAPE", "qr_bs == 0"):
        assert phrase in src, phrase


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_the_new_kernels_use_no_scratch_and_the_d40_build_keeps_four_waves():
    sys.path.insert(0, os.path.join(REPO, "tools"))
    try:
        import isa_audit
    finally:
        sys.path.pop(0)
    rows = [(k, v) for f, k, v in isa_audit.store_policy_rows([os.path.join(isa_audit.CSRC, "attention.hip")])
            if "attention_rbias_kernel" in k]
    assert len(rows) == 3, [k for k, _ in rows]
    for k, v in rows:
        assert v["scratch"] == 0, (k, v)
        if "ILi40E" in k:
            assert v["vgprs"] <= 128, (k, v)


# ------------------------------------------------------------------------------------------------
# host layers
# ------------------------------------------------------------------------------------------------
def test_check_regions_routes_and_refuses_on_the_host():
    from lib.pipeline import check_regions
    A, B, C = (torch.full((1, 3, 32, 32), v) for v in (0.1, 0.2, 0.3))
    m = np.zeros((6, 6), dtype=np.uint8)
    m[:, 3:] = 1
    assert check_regions(A, None, None, None) == (A, None, None)
    img, w, reg = check_regions([A, B], m[:, :3], [[0.7, 0.3]], None)          # one region IS the image_weights request
    assert img == [A, B] and w == [0.7, 0.3] and reg is None
    img, w, reg = check_regions([A, B, C], m, [[0.0, 0.0, 1.0], [0.0, 0.0, 2.0]], None)      # one reference left: the plain request
    assert img is C and w is None and reg is None
    img, w, reg = check_regions([A, B, C], m, [[1.0, 0.0, 0.0], [0.0, 0.0, 1.0]], None)      # B is used by no region: dropped
    assert img == [A, C] and w is None and reg[1].tolist() == [[1.0, 0.0], [0.0, 1.0]] and np.array_equal(reg[0], m)
    for args, msg in ((([A, B], m, None, None), "together"), (([A, B], m, [[1, 0], [0, 1]], [1, 1]), "exclude"), ((A, m, [[1], [1]], None), "image="),
                      (([A, B], m, [[1, 0]], None), "only 1 regions"), (([A, B], m[0], [[1, 0], [0, 1]], None), r"\[Hm, Wm\]"),
                      (([A, B], m, [[1, 0, 0], [0, 1, 0]], None), "reference pictures")):
        with pytest.raises(ValueError, match=msg):
            check_regions(*args)


def test_level_maps_take_every_level_from_the_map_itself():
    m = np.zeros((64, 64), dtype=np.uint8)
    m[:, 32:] = 1
    m[:, 33] = 2                                           # a one-pixel stripe: seen where a cell centre lands on it, not inherited
    maps, sizes = regions.level_maps(m, 2, 8, 8, 4, nr=3)
    assert sizes == [64, 16, 4, 1] and maps.shape == (2, 85) and maps.dtype == np.uint8 and np.array_equal(maps[0], maps[1])
    off = 0
    for (h, w), n in zip(regions.level_sizes(8, 8, 4), sizes):
        assert np.array_equal(maps[0, off:off + n], regions.region_grid(m, h, w))
        off += n
    assert regions.level_sizes(5, 3, 4) == [(5, 3), (3, 2), (2, 1), (1, 1)] and regions.level_sizes(1, 1, 4) == [(1, 1)]
    per = np.stack([m, np.zeros_like(m)])
    maps2, _ = regions.level_maps(per, 2, 8, 8, 4, nr=3)
    assert np.array_equal(maps2[0], maps[0]) and not maps2[1].any()
    with pytest.raises(ValueError, match="only 2 regions"):
        regions.level_maps(m, 2, 8, 8, 4, nr=2)


# ---- sampler (tests/sampler_standin.py) --------------------------------------------------------------------------------
import sampler_standin as SS


class _RegionModel(SS.StubModel):
    """the stand-in model, told about regions: it logs and keeps what prepare_context is handed"""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.diffuser['image'].channel_mult = (1, 2, 4)

    def prepare_context(self, c, bias=None, regions=None):
        ctx = super().prepare_context(c)
        if regions is not None:
            assert bias is None
            SS.LOG.append(f"prepare_context regions table={tuple(regions[0].shape)} maps={tuple(regions[1].shape)} sizes={list(regions[2])}")
            self.seen = (regions[0].clone(), regions[1].clone(), list(regions[2]))
        return ctx


def _sample(monkeypatch, c_extra, solver='ddim', uc='rand', scale=2.0, steps=4, model=None):
    from lib.model_zoo.ddim import DDIMSampler
    SS.install(monkeypatch)
    model = model or _RegionModel()
    s = DDIMSampler(model)
    g = torch.Generator().manual_seed(3)
    bs = SS.SHAPE[0]
    c = {'type': 'image', 'conditioning': torch.randn(bs, 4, 8, generator=g), 'unconditional_guidance_scale': scale}
    if uc is not None:
        c['unconditional_conditioning'] = torch.randn(bs, 4, 8, generator=g)
    c.update(c_extra)
    x_info = {'type': 'image', 'xt': torch.randn(*SS.SHAPE, generator=g)}
    x, _ = s.sample(steps, SS.SHAPE, x_info, c, eta=0., verbose=False, solver=solver)
    return model, x, list(SS.LOG)


def test_sampler_concatenates_table_and_maps_like_the_contexts(monkeypatch):
    bs, (h, w) = SS.SHAPE[0], SS.SHAPE[2:]
    rb = torch.from_numpy(regions.region_bias([[1.0, 0.0], [0.0, 1.0], [0.5, 1.0]], 2, 4))[None].repeat(bs, 1, 1)
    urb = torch.zeros_like(rb)
    urb[:, :, 3] = float('-inf')
    m = np.zeros((6, 10), dtype=np.uint8)
    m[:, 5:] = 1
    m[4:, :] = 2
    want_maps, sizes = regions.level_maps(m, bs, h, w, 3, 3)
    assert sizes == [h * w, ((h + 1) // 2) * ((w + 1) // 2), ((h + 3) // 4) * ((w + 3) // 4)]
    plain = _sample(monkeypatch, {})
    for extra, want in (({'region_bias': rb, 'region_map': m}, torch.cat([torch.zeros_like(rb), rb])),
                        ({'region_bias': rb, 'region_map': torch.from_numpy(m), 'unconditional_region_bias': urb}, torch.cat([urb, rb])),
                        ({'region_bias': rb, 'region_map': [m] * bs}, torch.cat([torch.zeros_like(rb), rb]))):
        for solver in ('ddim', 'dpmpp_2m'):
            model, x, log = _sample(monkeypatch, extra, solver=solver)
            tab, maps, sz = model.seen
            assert torch.equal(tab, want) and tab.dtype == torch.float32 and sz == sizes
            assert maps.dtype == torch.uint8 and torch.equal(maps, torch.from_numpy(np.concatenate([want_maps, want_maps])))
            assert sum(l.startswith("prepare_context regions") for l in log) == 1
            if solver == 'ddim':      # the stand-in's eps ignores the regions: everything else is the plain request, call for call
                assert [l for l in log if not l.startswith("prepare_context")] == plain[2] and torch.equal(x, plain[1])
    model, _, _ = _sample(monkeypatch, {'region_bias': rb, 'region_map': m}, uc=None, scale=1.0)      # no CFG: the conditional rows alone
    assert torch.equal(model.seen[0], rb) and torch.equal(model.seen[1], torch.from_numpy(want_maps))
    per = np.stack([m, np.zeros_like(m)])                                                             # one map per sample
    model, _, _ = _sample(monkeypatch, {'region_bias': rb, 'region_map': per})
    assert not bool(model.seen[1][1].any()) and bool(model.seen[1][0].any())
    bad_map = m.copy()
    bad_map[0, 0] = 3
    for extra, msg in (({'region_bias': rb}, "come together"), ({'region_map': m}, "come together"),
                       ({'region_bias': rb[:, :, :3], 'region_map': m}, "region_bias"), ({'region_bias': rb[:1], 'region_map': m}, "region_bias"),
                       ({'region_bias': rb, 'region_map': bad_map}, "only 3 regions"),
                       ({'region_bias': rb, 'region_map': m, 'key_bias': rb[:, 0]}, "exclude each other"),
                       ({'region_bias': rb, 'region_map': m, 'unconditional_region_bias': urb[:, :2]}, "unconditional_region_bias")):
        with pytest.raises(ValueError, match=msg):
            _sample(monkeypatch, extra)
    # a model that does not state its resolutions: refused here, in front of the loop, not as a missing map inside it
    bare = _RegionModel()
    del bare.diffuser['image'].channel_mult
    with pytest.raises(ValueError, match="states its resolutions"):
        _sample(monkeypatch, {'region_bias': rb, 'region_map': m}, model=bare)


def test_multicontext_sampling_refuses_regions():
    from lib.model_zoo.ddim import DDIMSampler
    s = DDIMSampler.__new__(DDIMSampler)
    s.model = None
    ci = {'unconditional_guidance_scale': 2.0, 'conditioning': torch.zeros(2, 1, 1), 'unconditional_conditioning': torch.zeros(2, 1, 1),
          'region_bias': torch.zeros(2, 1, 1), 'region_map': np.zeros((2, 2), dtype=np.uint8)}
    with pytest.raises(ValueError, match="region_bias"):
        s._mix_for([ci], 2)
    with pytest.raises(ValueError, match="region_bias"):
        s.sample_multicontext(2, [2, 4, 8, 8], {'type': 'image'}, [ci], verbose=False)


# ---- pipeline and server (tests/stubs.py) ------------------------------------------------------------------------------
def _pic(v):
    return torch.full((1, 3, 64, 64), float(v))


def _pipe(seen):
    from stubs import StubNet
    from lib.pipeline import PromptFreePipeline

    class _Net(StubNet):
        encoded = []

        def ctx_encode(self, image, which):
            _Net.encoded.append(float(image.mean()))
            return super().ctx_encode(image, which)

    class _Sampler:
        def sample(self, steps, shape, x_info, c_info, eta=0., verbose=True, **how):
            seen.update(c_info=c_info, how=how)
            return x_info['xt'], {}

    _Net.encoded = []
    return PromptFreePipeline(_Net(), sampler=_Sampler()), _Net


def test_generate_builds_the_table_drops_and_collapses():
    seen = {}
    pipe, Net = _pipe(seen)
    A, Bp, Cp = _pic(0.25), _pic(0.5), _pic(0.75)
    m = np.zeros((10, 6), dtype=np.uint8)
    m[:, 3:] = 1
    rw = [[1.0, 0.0, 0.0], [0.5, 0.0, 1.0]]
    pipe.generate([A, Bp, Cp], 2, 64, 64, steps=2, decode=False, regions=m, region_weights=rw, solver='dpmpp_2m')
    ci = seen['c_info']
    assert Net.encoded == [0.25, 0.75] and seen['how'] == {'solver': 'dpmpp_2m'}      # the reference no region uses was never encoded
    assert tuple(ci['conditioning'].shape) == (2, 296, 768) and 'key_bias' not in ci and 'unconditional_region_bias' not in ci
    want = torch.from_numpy(regions.region_bias([[1.0, 0.0], [0.5, 1.0]], 148, 296))
    assert ci['region_bias'].dtype == torch.float32 and torch.equal(ci['region_bias'], want[None].repeat(2, 1, 1))
    assert bool(torch.isneginf(ci['region_bias'][:, 0, 148:]).all()) and np.array_equal(ci['region_map'], m)
    # one region: the image_weights request of its row, call for call
    pipe.generate([A, Bp], 2, 64, 64, steps=2, decode=False, regions=m[:, :3], region_weights=[[0.7, 0.3]])
    one = seen['c_info']
    pipe.generate([A, Bp], 2, 64, 64, steps=2, decode=False, image_weights=[0.7, 0.3])
    mix = seen['c_info']
    assert set(one) == set(mix) and 'region_bias' not in one and torch.equal(one['key_bias'], mix['key_bias'])
    # one reference left: the plain request
    Net.encoded.clear()
    pipe.generate([A, Bp], 2, 64, 64, steps=2, decode=False, regions=m, region_weights=[[0.0, 1.0], [0.0, 2.0]])
    assert Net.encoded == [0.5] and 'region_bias' not in seen['c_info'] and 'key_bias' not in seen['c_info']
    # an uncond with fewer tokens than the references: zero tokens at -inf behind it, for every region alike
    pipe.generate([A, Bp], 2, 64, 64, steps=2, decode=False, regions=m, region_weights=[[1, 0], [0, 1]], uncond=torch.full((1, 148, 768), 0.5))
    ub = seen['c_info']['unconditional_region_bias']
    assert tuple(ub.shape) == (2, 2, 296) and bool((ub[:, :, :148] == 0).all()) and bool(torch.isneginf(ub[:, :, 148:]).all())
    # the world size does not enter
    from lib.pipeline import PromptFreePipeline
    for rank in range(2):
        PromptFreePipeline(pipe.net, rank=rank, world_size=2, sampler=pipe.sampler).generate(
            [A, Bp], 4, 64, 64, steps=2, decode=False, regions=m, region_weights=[[1, 0], [0, 1]])
        assert tuple(seen['c_info']['region_bias'].shape) == (2, 2, 296)


def test_server_batches_regional_requests_with_their_like_only(monkeypatch):
    import threading
    from lib import serving

    class _Pipe:
        def __init__(self, net):
            pass

        def enable_graph(self, on):
            pass

    monkeypatch.setattr(serving, "PromptFreePipeline", _Pipe)
    srv = serving.PromptFreeServer(object(), use_graph=False, max_batch=4)
    calls = []
    srv._generate = lambda batch: (calls.append([r.seed for r in batch]), [torch.full((r.n, 1), float(r.seed)) for r in batch])[1]
    A, Bp, Cp = _pic(0.25), _pic(0.5), _pic(0.75)
    m, m2 = np.zeros((8, 8), dtype=np.uint8), np.ones((5, 9), dtype=np.uint8)
    kw = dict(height=64, width=64, steps=4)
    try:
        gate = threading.Event()
        srv.call(lambda n: gate.wait(30))
        futs = [srv.submit([A, Bp], regions=m, region_weights=[[1, 0], [0, 1]], seed=1, **kw),
                srv.submit([Bp, Cp], regions=m2, region_weights=[[1, 1], [0.2, 1]], seed=2, **kw),       # another map, another size: shared
                srv.submit([A, Bp], image_weights=[0.7, 0.3], seed=3, **kw),                           # per-key weights: apart
                srv.submit([A, Bp], regions=m, region_weights=[[0.7, 0.3]], seed=4, **kw),              # one region = image_weights: with 3
                srv.submit([A, Bp, Cp], regions=m2, region_weights=[[1, 0, 0], [0, 1, 1]], seed=5, **kw),   # three references: apart
                srv.submit([A, Bp], regions=np.full((4, 4), 2, dtype=np.uint8), region_weights=[[1, 0], [0, 1], [1, 1]], seed=6, **kw),   # three regions
                srv.submit(A, seed=7, **kw),
                srv.submit([A, Bp], regions=m, region_weights=[[1, 0], [2, 0]], seed=8, **kw)]           # one reference left: plain, with 7
        gate.set()
        assert [float(f.result(30)[0, 0]) for f in futs] == [1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0]
        assert calls == [[1, 2], [3, 4], [5], [6], [7, 8]]
        for bad in (dict(regions=m), dict(regions=m, region_weights=[[1, 0], [0, 1]], image_weights=[1, 1]),
                    dict(regions=m2, region_weights=[[1, 0]]), dict(regions=m, region_weights=[[1, 0], [0, 1]], uncond=torch.zeros(1, 148, 768))):
            with pytest.raises(ValueError):
                srv.submit([A, Bp], **kw, **bad)
    finally:
        srv.close()
    R = serving._Request
    k = dict(image=A, n=1, height=64, width=64, steps=4, seed=1, eta=0.0, scale=2.0)
    assert R(**k).key() == (64, 64, 4, 2.0, 0.0, True, True, False, False)                      # a plain key is what it was
    assert R(weights=[0.7, 0.3], **k).key()[-1] == 'refmix'                                     # ... and so is the per-key one
    assert R(weights=[1.0, 1.0], regional=(m, np.ones((2, 2))), **k).key()[-1] == ('regions', 2, 2)


def test_server_generate_hands_each_sample_its_own_table_and_map():
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
    m, m2 = np.zeros((8, 8), dtype=np.uint8), np.ones((5, 9), dtype=np.uint8)
    kw = dict(height=64, width=64, steps=2, eta=0.0, as_uint8=False, future=None, scale=2.0)
    srv = serving.PromptFreeServer(StubNet(), use_graph=False, max_batch=8)
    try:
        srv.pipe.sampler = _Sampler()
        R = serving._Request
        w1, w2 = np.array([[1.0, 0.0], [0.0, 1.0]]), np.array([[1.0, 1.0], [0.2, 1.0]])
        outs = srv._generate([R(n=2, seed=1, image=[A, Bp], weights=[1.0, 1.0], regional=(m, w1), **kw),
                              R(n=1, seed=2, image=[Bp, Cp], weights=[1.0, 1.0], regional=(m2, w2), **kw)])
        ci = seen['c_info']
        assert [o.shape[0] for o in outs] == [2, 1] and srv.batches == [3] and 'key_bias' not in ci
        assert tuple(ci['conditioning'].shape) == (3, 296, 768) and tuple(ci['region_bias'].shape) == (3, 2, 296)
        assert torch.equal(ci['region_bias'][1], torch.from_numpy(regions.region_bias(w1, 148, 296)))
        assert torch.equal(ci['region_bias'][2], torch.from_numpy(regions.region_bias(w2, 148, 296)))
        assert len(ci['region_map']) == 3 and ci['region_map'][0] is m and ci['region_map'][1] is m and ci['region_map'][2] is m2
        maps, sizes = regions.level_maps(ci['region_map'], 3, 8, 8, 4, 2)             # maps of different sizes side by side
        assert maps.shape == (3, 85) and not maps[:2].any() and maps[2].all()
    finally:
        srv.close()
