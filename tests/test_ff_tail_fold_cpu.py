"""The transformer tail fold (SpatialTransformer.ff_tail_fold, layers.fold_ff_tail) without a GPU:

    h2 = h1 + W2 g + b2,  y = Wpo h2 + bpo + x      ==      y = [Wpo | Wpo W2] [h1 | g] + (Wpo b2 + bpo) + x

the algebra in fp64, the two forms after their fp16 roundings against the fp64 result, and the host path of
SpatialTransformer.hip over tests/ops_standin.py: which launches it makes, that the pack follows the weights, and when it keeps
the two launches.  Weights are drawn at 1 / sqrt(fan_in) (block_refs.seed_module): proj_out is zero in a fresh module, and a zero
branch hides every error inside it."""
import math
import os
import subprocess
import sys

import pytest
import torch

import block_refs as BR
import ops_standin as SI
from lib.hip import layers as L, ops
from lib.model_zoo import attention as AT


def _operands(C, M, seed, dtype):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s, scale=1.0: (torch.randn(s, generator=g) * scale).half().to(dtype)  # noqa: E731
    inner = C
    return dict(wpo=r(C, inner, scale=inner ** -0.5), bpo=r(C, scale=0.1), w2=r(inner, 4 * inner, scale=(4 * inner) ** -0.5),
                b2=r(inner, scale=0.1), h1=r(M, inner), g=r(M, 4 * inner, scale=0.7), x=r(M, C))


def _two_launch64(o):
    d = {k: v.double() for k, v in o.items()}
    h2 = d["h1"] + d["g"] @ d["w2"].t() + d["b2"]
    return h2 @ d["wpo"].t() + d["bpo"] + d["x"]


def _scaled(y, ref):
    return float((y.double() - ref).abs().max() / ref.abs().max())


@pytest.mark.parametrize("C", [320, 640])
def test_fold_algebra_is_exact_in_fp64(C):
    o = _operands(C, 96, C, torch.float64)
    w, b = L.fold_ff_tail(o["wpo"], o["bpo"], o["w2"], o["b2"])
    assert w.dtype == torch.float64 and tuple(w.shape) == (C, 5 * C) and tuple(b.shape) == (C,)
    y = torch.cat([o["h1"], o["g"]], 1) @ w.t() + b + o["x"]
    ref = _two_launch64(o)
    assert _scaled(y, ref) <= 1e-13
    # a 1x1 convolution's weight, and absent biases
    w4, b0 = L.fold_ff_tail(o["wpo"].reshape(C, C, 1, 1), None, o["w2"], None)
    assert torch.equal(w4, w) and float(b0.abs().max()) == 0


@pytest.mark.parametrize("C", [320, 640])
def test_one_rounding_against_two(C, monkeypatch):
    """fp16 operands: the folded launch (W' rounded once, the result rounded once) and the two launches (h2 rounded to fp16 in
    between) against the fp64 result on the same operands.  The fold rounds less often; the factor 2 covers the rounding of
    Wpo W2."""
    SI.install(monkeypatch)
    o = _operands(C, 128, C + 1, torch.float16)
    ref = _two_launch64(o)
    w, b = L.fold_ff_tail(o["wpo"], o["bpo"], o["w2"], o["b2"])
    assert w.dtype == torch.float16 and b.dtype == torch.float16 and w.is_contiguous()
    assert torch.equal(w[:, :C], o["wpo"])
    wf64 = o["wpo"].double() @ o["w2"].double()
    assert float((w[:, C:].double() - wf64).abs().max()) <= 2.0 ** -11 * float(wf64.abs().max())      # ONE rounding of the fp64 product
    y_fold = ops.gemm(o["h1"], w, bias=b, a2=o["g"], res=o["x"])
    h2 = ops.gemm(o["g"], o["w2"], bias=o["b2"], res=o["h1"])
    y_two = ops.gemm(h2, o["wpo"], bias=o["bpo"], res=o["x"])
    e_fold, e_two = _scaled(y_fold, ref), _scaled(y_two, ref)
    print(f"C {C}: folded {e_fold:.3e} two-launch {e_two:.3e} (scaled max-abs against fp64)")
    assert 0 < e_two < 2e-3
    assert e_fold <= 2 * e_two


def _run(cid, fold, monkeypatch, mods=None):
    """the case's SpatialTransformer.hip over the stand-in -> (result, [keyword arguments of every ops.gemm call], modules)"""
    b = BR.built(cid)
    SI.install(monkeypatch)
    BR.apply_switches(monkeypatch, BR.CASE[cid]["switches"])
    monkeypatch.setattr(AT.SpatialTransformer, "ff_tail_fold", fold)
    monkeypatch.setattr(AT.SpatialTransformer, "ff_tail_fold_min_rows", 0)      # (the cases are 128 ... 256 rows)
    calls = []
    real = ops.gemm
    monkeypatch.setattr(ops, "gemm", lambda *a, **k: (calls.append(k), real(*a, **k))[1])
    m, inputs = BR._dev(b, "cpu")
    mods = mods or m
    y = b.run(mods, inputs)
    assert not SI.FELL_THROUGH
    return y, calls, mods


def _folded(calls):
    return [k for k in calls if k.get("a2") is not None]


def _plain_res(calls):
    return [k for k in calls if k.get("res") is not None and k.get("a2") is None and not k.get("zero_rows")]


@pytest.mark.parametrize("cid", ["st-conv", "st-linear", "st-pair", "st-pair-copies", "st-pstats-off"])
def test_host_path_folds_and_stays_within_twice_the_two_launch_error(cid, monkeypatch):
    b = BR.built(cid)
    with monkeypatch.context() as mp:
        y0, c0, _ = _run(cid, False, mp)
    with monkeypatch.context() as mp:
        y1, c1, _mods = _run(cid, True, mp)
    assert not _folded(c0) and len(_folded(c1)) == 1
    assert len(c1) == len(c0)      # one launch less in the pass; this first run also forms Wpo W2 for the pack
    with monkeypatch.context() as mp:
        _, c2, _ = _run(cid, True, mp, mods=_mods)
    assert len(c2) == len(c0) - 1 and len(_folded(c2)) == 1
    k = _folded(c1)[0]
    assert k.get("res") is not None and k.get("bias") is not None
    assert (k.get("res_rows") is not None) == (cid == "st-pair")
    assert bool(k.get("gn_out")) == (cid in ("st-conv", "st-pair", "st-pair-copies"))
    assert (ops.get_gn_stats(y1) is not None) == (ops.get_gn_stats(y0) is not None)
    e0, e1 = BR.err_units(y0, b.ref64, b.B), BR.err_units(y1, b.ref64, b.B)
    print(f"{cid}: two launches {e0:.3f}, folded {e1:.3f} (units of 2^-11)")
    assert e1 <= 2 * e0


def test_c640_and_gelu_feed_forward(monkeypatch):
    """inner = 640, and a Linear + GELU feed-forward in front of the fold"""
    for kw, glu in ((dict(C=640, heads=8, seed=21), True), (dict(C=320, seed=22), False)):
        b = BR.build_st(**kw)
        if not glu:      # the GELU form of the feed-forward (gated_ff=False), same state-dict walk in the formula
            st = BR.seed_module(AT.SpatialTransformer(320, 8, 40, context_dim=[768]), 22)
            st.transformer_blocks[0].ff = BR.seed_module(AT.FeedForward(320, glu=False), 23)
            b.mods = {"st": st}
            ref = BR.nhwc(BR.spatial_transformer(BR.P(BR._sd(b, "st")), BR.nchw(b.inputs["x"].double()), b.inputs["ctx"].double(), 8,
                                                 glu=False))
        else:
            ref = b.ref()
        errs = []
        for fold in (False, True):
            with monkeypatch.context() as mp:
                SI.install(mp)
                mp.setattr(AT.SpatialTransformer, "ff_tail_fold", fold)
                mp.setattr(AT.SpatialTransformer, "ff_tail_fold_min_rows", 0)
                mods, inputs = BR._dev(b, "cpu")
                assert mods["st"].tail_foldable(kw["C"], 128) == fold
                errs.append(BR.err_units(b.run(mods, inputs), ref, b.B))
        print(f"{kw} glu {glu}: two launches {errs[0]:.3f}, folded {errs[1]:.3f}")
        assert errs[1] <= 2 * errs[0]


def test_depth2_folds_only_the_last_block(monkeypatch):
    y, calls, mods = _run("st-depth2", True, monkeypatch)
    assert len(_folded(calls)) == 1 and calls[-1].get("a2") is not None
    st = mods["st"]
    w, _ = st._pk_tail()
    w2_last = st.transformer_blocks[1].ff.net[2].weight.detach().double()
    assert float((w[:, 320:].double() - st.proj_out.weight.detach().double().reshape(320, 320) @ w2_last).abs().max()) < 1e-3
    # the first block's feed-forward ran whole: its output Linear with its residual, 1280 columns in
    ff_out = [k for k in _plain_res(calls) if k["res"].shape[-1] == 320 and k.get("ln_out") is None]
    assert len(ff_out) == 1
    b = BR.built("st-depth2")
    assert BR.err_units(y, b.ref64, b.B) <= 4 * SI.floor(BR.CASE["st-depth2"])


@pytest.mark.parametrize("cid", ["st-96", "st-pair-384-no-stats", "st-gemmfuse-off", "st-pair-gemmfuse-off"])
def test_fallback_keeps_the_two_launches(cid, monkeypatch):
    """C_out = 96 (no wide tile), C_out = 384 (128-wide tiles: no statistics-emitting store pass), and the wide-tile forms switched off
    (wide_tile_ok fails): nothing changes"""
    with monkeypatch.context() as mp:
        y0, c0, _ = _run(cid, False, mp)
    with monkeypatch.context() as mp:
        y1, c1, mods = _run(cid, True, mp)
    assert not _folded(c1) and len(c1) == len(c0)
    assert torch.equal(y0, y1)
    assert "ff_tail" not in mods["st"].__dict__.get("_pk_cache", {})


def test_default_row_threshold(monkeypatch):
    """the class default folds from 1024 output rows up (a CFG pair counted doubled); below, the two launches"""
    assert AT.SpatialTransformer.ff_tail_fold_min_rows == 1024
    SI.install(monkeypatch)
    st = BR._dev(BR.built("st-conv"), "cpu")[0]["st"]
    monkeypatch.setattr(AT.SpatialTransformer, "ff_tail_fold", True)
    assert not st.tail_foldable(320, 128) and not st.tail_foldable(320, 960) and st.tail_foldable(320, 1024)
    assert st.tail_foldable(320, 32768) and not st.tail_foldable(320, 1024 + 32)
    calls = []
    real = ops.gemm
    monkeypatch.setattr(ops, "gemm", lambda *a, **k: (calls.append(k), real(*a, **k))[1])
    b = BR.built("st-conv")
    b.run(*BR._dev(b, "cpu"))
    assert not _folded(calls)                                          # 128 rows
    b = BR.built("st-pair")                                            # 64 rows in, 128 out
    b.run(*BR._dev(b, "cpu"))
    assert not _folded(calls)


def test_switch_off_is_the_two_launch_path(monkeypatch):
    _, calls, mods = _run("st-conv", False, monkeypatch)
    assert not _folded(calls) and not mods["st"].tail_foldable(320, 128)
    assert "ff_tail" not in mods["st"].__dict__.get("_pk_cache", {})


def test_pack_follows_in_place_weight_updates(monkeypatch):
    b = BR.built("st-conv")
    y0, _, mods = _run("st-conv", True, monkeypatch)
    st = mods["st"]
    pk0 = st._pk_cache["ff_tail"][1]
    assert st._pk_tail()[0] is pk0[0]                                  # cached
    assert "w" not in st.proj_out.__dict__.get("_pk_cache", {})        # the plain packs of the two layers are not built
    assert "w" not in st.transformer_blocks[0].ff.net[2].__dict__.get("_pk_cache", {})
    ff2 = st.transformer_blocks[0].ff.net[2]
    for prm, f in ((st.proj_out.weight, 0.5), (st.proj_out.bias, -1.0), (ff2.weight, 2.0), (ff2.bias, 3.0)):
        before = st._pk_tail()
        with torch.no_grad():
            prm.mul_(f)
        after = st._pk_tail()
        assert after[0] is not before[0], "the fold was not rebuilt after an in-place update"
        assert not (torch.equal(after[0], before[0]) and torch.equal(after[1], before[1]))
    # the result is that of the updated weights
    y1 = b.run(mods, BR._dev(b, "cpu")[1])
    sd = {k: v.half() for k, v in st.state_dict().items()}
    ref = BR.nhwc(BR.spatial_transformer(BR.P(sd), BR.nchw(b.inputs["x"].double()), b.inputs["ctx"].double(), 8))
    assert BR.err_units(y1, ref, b.B) <= 4 * SI.floor(BR.CASE["st-conv"])
    assert BR.err_units(y0, ref, b.B) > 16 * SI.floor(BR.CASE["st-conv"])
    # weights edited through .data: invalidate_packed, as for every other pack
    st.proj_out.weight.data.mul_(2.0)
    assert st._pk_tail()[0] is after[0]
    L.invalidate_packed(st)
    assert st._pk_tail()[0] is not after[0]


def test_fold_magnitudes_are_fp16_safe():
    """Wpo W2 at trained magnitude stays far inside fp16: entries ~ 1 / sqrt(4 inner)"""
    o = _operands(640, 8, 5, torch.float64)
    w, _ = L.fold_ff_tail(o["wpo"], o["bpo"], o["w2"], o["b2"])
    assert float(w.abs().max()) < 1.0 and float(w[:, 640:].abs().mean()) > 0.1 / math.sqrt(2560)


EMU_CXX = os.environ.get("EMU_CXX", "/opt/rocm/lib/llvm/bin/clang++")


@pytest.mark.skipif(not os.path.exists(EMU_CXX), reason="clang++ of the ROCm toolchain not available")
def test_folded_launch_on_the_cpu_emulation(tmp_path):
    """the launch the fold makes -- two sources + residual with one wrap + group sums of the output, never combined before -- through
    the real kernels of csrc/gemm_glds.hip on the host emulation (tools/cpu_emu): the store pass of the 128- and 64-row
    eight-wave tiles and the split-K reduction, against double precision, the sums against the stored values"""
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.run([sys.executable, os.path.join(repo, "tools", "cpu_emu", "build.py"), str(tmp_path)], check=True,
                   stdout=subprocess.DEVNULL)
    r = subprocess.run([str(tmp_path / "emu_gemm"), "tail fold"], capture_output=True, text=True, timeout=600)
    lines = [l for l in r.stdout.splitlines() if l.startswith(("ok", "FAIL"))]
    assert r.returncode == 0 and len(lines) == 3 and all(l.startswith("ok") and "statistics err" in l for l in lines), \
        r.stdout[-3000:] + r.stderr[-1000:]
