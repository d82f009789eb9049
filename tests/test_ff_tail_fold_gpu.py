"""GPU (-m gpu): the transformer tail fold (SpatialTransformer.ff_tail_fold) on the device.

SpatialTransformer.hip with the fold on and off against the fp64 evaluation of oracle/pfd_oracle.py's spatial_transformer on the
same inputs.  The yardstick is the error of the two-launch path (switch off), never a number from the folded one: the folded
path's scaled max-abs error must not exceed twice it (it rounds less often; the factor 2 covers the one extra rounding of
Wpo W2).  The launch the fold makes -- k_split + residual (+ res_rows) + statistics, split and unsplit -- is also checked on its
own against the per-element bound of tests/kernel_refs.py (gemm_allowance), and the GroupNorm statistics that ride on the output
against the fp64 sums of the stored tensor."""
import functools

import pytest
import torch

import block_refs as BR
import kernel_refs as KR
import ops_standin as SI
import pfd_oracle as O

pytestmark = pytest.mark.gpu


class SD64(O.SD):
    """the oracle's state-dict view in fp64"""

    def __getitem__(self, k):
        return self.sd[self.prefix + k].double()

    def sub(self, p):
        return SD64(self.sd, self.prefix + p)


def scaled_err(a, ref):
    """the `close` metric of tests/test_hip_kernels.py"""
    return float((a.double().cpu() - ref).abs().max() / max(1.0, float(ref.abs().max())))


@functools.lru_cache(maxsize=None)
def problem(C, B, pair, H=8, W=8):
    """seeded module (every weight at 1 / sqrt(fan_in), proj_out too), inputs and the fp64 oracle result, once per case.
    pair: x holds one copy of a CFG pair, the first half of the batch has an all-zero context"""
    from lib.model_zoo import attention as AT
    heads = 8
    st = BR.seed_module(AT.SpatialTransformer(C, heads, C // heads, context_dim=[768]), 31 + C)
    Bx = B // 2 if pair else B
    x = BR.rand16((Bx, H, W, C), 32 + C, 1.0, 0.3)
    ctx = BR.rand16((B, 20, 768), 33 + C)
    if pair:
        ctx[:B // 2] = 0
    sd = {k: v.half() for k, v in st.state_dict().items()}
    xr = BR.nchw(x.double())
    if pair:
        xr = torch.cat([xr, xr])
    ref = BR.nhwc(O.spatial_transformer(SD64(sd), xr, ctx.double(), heads))
    return dict(st=st, x=x, ctx=ctx, ref=ref, B=B, pair=pair)


def run(p, fold):
    """SpatialTransformer.hip on the device with the switch in that position -> the result (statistics riding on it)"""
    import copy
    from lib.model_zoo import attention as AT
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(AT.SpatialTransformer, "ff_tail_fold", fold)
        mp.setattr(AT.SpatialTransformer, "ff_tail_fold_min_rows", 0)      # (the cases are 128 ... 512 rows)
        st = copy.deepcopy(p["st"]).half().cuda()
        kv = AT.ContextKV(p["ctx"].cuda())
        kv.zero_lead = p["B"] // 2 if p["pair"] else 0
        y = st.hip(p["x"].cuda(), kv, cfg_pair=p["pair"])
        y2 = st.hip(p["x"].cuda(), kv, cfg_pair=p["pair"])      # (the second call takes the cached pack)
        torch.cuda.synchronize()
        assert torch.equal(y, y2), "second launch differs"
        assert ("ff_tail" in st.__dict__.get("_pk_cache", {})) == fold
    return y


def stats_ratio(y, st):
    """the statistics against the fp64 sums of the stored tensor, over the bound of an fp32 sum of 64 * N / 32 values per slab
    (tests/test_blocks_gpu.py): <= 1 passes"""
    N = y.shape[-1]
    cpg, g = N // 32, 160 // (N // 32)
    stored = y.detach().cpu().reshape(-1, N)
    want = KR.gn_out_ref(stored)[:, :, :g]
    v = stored.double().reshape(-1, 64, N // 160, g, cpg)
    bnd = 64 * cpg * 2.0 ** -24 * torch.stack([v.abs().sum((1, 4)), (v * v).sum((1, 4))], -1)
    assert tuple(st.shape) == (stored.shape[0] // 64, N // 160, 16, 2)
    return float(((st.cpu()[:, :, :g].double() - want).abs() / bnd).max())


CASES = [(320, 2, False), (320, 2, True), (1280, 8, False)]


@pytest.mark.parametrize("C,B,pair", CASES, ids=["c320", "c320-cfg-pair", "c1280-b8-splitk"])
def test_fold_against_two_launches_and_fp64(C, B, pair):
    """c320: 128 x 320 x 1600; c320-cfg-pair: the residual stored once (res_rows); c1280-b8: 512 x 1280 x 6400, which the
    library splits over K"""
    from lib.hip import ops
    p = problem(C, B, pair)
    y_two, y_fold = run(p, False), run(p, True)
    e_two, e_fold = scaled_err(y_two, p["ref"]), scaled_err(y_fold, p["ref"])
    print(f"[ff-tail-fold] C {C} B {B} pair {pair}: scaled max-abs two launches {e_two:.3e}, folded {e_fold:.3e}, "
          f"ratio {e_fold / e_two:.2f}")
    assert 0 < e_two < 1e-2, e_two                 # the yardstick itself is a handful of fp16 roundings of O(1) values
    assert e_fold <= 2 * e_two, (e_fold, e_two)
    # the statistics that ride on the output: present where the two-launch path carries them, sums of the stored tensor
    s_two, s_fold = ops.get_gn_stats(y_two), ops.get_gn_stats(y_fold)
    assert (s_fold is None) == (s_two is None)
    assert (s_fold is not None) == bool(ops.gn_stats_wanted(B, 64, C))
    if s_fold is not None:
        r = stats_ratio(y_fold, s_fold)
        print(f"[ff-tail-fold] C {C} pair {pair}: carried statistics err / bound {r:.3f}")
        assert r <= 1.0


@functools.lru_cache(maxsize=None)
def gemm_problem(M, N, ks, rr, slabs):
    """the folded launch on its own: operands at the magnitudes of the block (h1, x ~ 1, g ~ 0.7, W' = [Wpo | Wpo W2] from
    weights at 1 / sqrt(fan_in)) and the fp64 result with its per-element allowance for a launch with `slabs` slabs, once"""
    from lib.hip import layers as L
    g = torch.Generator().manual_seed(M + N + ks + rr)
    r = lambda *s, scale=1.0: (torch.randn(s, generator=g) * scale).half()  # noqa: E731
    wpo, w2 = r(N, ks, scale=ks ** -0.5), r(ks, 4 * ks, scale=(4 * ks) ** -0.5)
    w64, b64 = L.fold_ff_tail(wpo.double(), r(N, scale=0.1).double(), w2.double(), r(ks, scale=0.1).double())
    p = dict(case=SI._case(cls="lin", M=M, N=N, K=5 * ks, k_split=ks, res_rows=rr), A=r(M, ks), A2=r(M, 4 * ks, scale=0.7),
             W=w64.half(), bias=b64.half(), rowvec=None, R=r(rr or M, N), gn_table=None)
    p["ref"] = KR.gemm_ref(p)["out"]
    p["a"] = KR.gemm_allowance(p, splits=slabs, wide=True)["out"]
    return p


# (M, N, k_split, res_rows, forced tile code, slabs): variant v with s splits is 1000 + 100 v + s (include/pfd_hip.h)
LAUNCHES = [(1024, 320, 320, 512, 0, 1), (1024, 320, 320, 512, 9200, 1), (1024, 320, 320, 512, 5304, 4), (128, 1280, 1280, 0, 0, 4),
            (128, 1280, 1280, 0, 5301, 1), (576, 2560, 448, 0, 0, 2)]


@pytest.mark.parametrize("M,N,ks,rr,tile,slabs", LAUNCHES, ids=[f"M{c[0]}-N{c[1]}-rr{c[3]}-tile{c[4]}" for c in LAUNCHES])
def test_folded_launch_and_its_statistics(M, N, ks, rr, tile, slabs):
    """k_split + residual (+ res_rows) + gn_out under the heuristic and forced variants: the statistics-emitting store pass, the
    statistics-emitting split-K reduction (4 slabs of 7 K tiles at K = 1600: slab 0 holds tiles of BOTH sources; 128 x 1280 x
    6400 is split 4 ways by the heuristic itself, like the mid block's 512 rows, which the block test above runs; 576 x 2560 x
    2240 has more than 128 64-row tiles: the dispatcher's rule for the fold gives it two-stage 128-row tiles, split in two, the
    plain reduction -- what 2048 x 1280 x 6400 of the 16^2 level gets, at a size whose fp64 reference takes seconds)"""
    from lib.hip import ops
    p = gemm_problem(M, N, ks, rr, slabs)
    a, a2, w, b, R = (p[k].cuda() for k in ("A", "A2", "W", "bias", "R"))
    gn = N in (320, 640, 1280)
    y = ops.gemm(a, w, bias=b, a2=a2, res=R, gn_out=gn, res_rows=rr or None, tile=tile)
    st = ops.get_gn_stats(y)
    torch.cuda.synchronize()
    ratio, used = KR.bound_ratio(y, p["ref"], p["a"])
    r_st = stats_ratio(y, st) if gn else 0.0
    print(f"[ff-tail-fold] launch M{M} N{N} K{5 * ks} rr{rr} tile{tile}: err / bound {ratio:.3f} (allowance used {used:.3f}), "
          f"statistics err / bound {r_st:.3f}")
    assert ratio <= 1.0
    assert r_st <= 1.0
    if M == 576:                   # the rule's choice: variant 82 (two-stage 128-row tiles on eight waves), two slabs
        assert torch.equal(y, ops.gemm(a, w, bias=b, a2=a2, res=R, tile=9202))
    if (M, tile) == (128, 0):      # the heuristic's own choice at the mid block's width and depth: the 64-row ring, four slabs
        assert torch.equal(y, ops.gemm(a, w, bias=b, a2=a2, res=R, gn_out=True, tile=5304))


def test_weight_hot_swap_refolds_on_the_device(monkeypatch):
    from lib.hip import layers as L
    from lib.model_zoo import attention as AT
    import copy
    monkeypatch.setattr(AT.SpatialTransformer, "ff_tail_fold", True)
    monkeypatch.setattr(AT.SpatialTransformer, "ff_tail_fold_min_rows", 0)
    p = problem(320, 2, False)
    st = copy.deepcopy(p["st"]).half().cuda()
    kv = AT.ContextKV(p["ctx"].cuda())
    y1 = st.hip(p["x"].cuda(), kv).clone()
    w1 = st._pk_tail()[0]
    assert st._pk_tail()[0] is w1
    with torch.no_grad():
        st.transformer_blocks[0].ff.net[2].weight.mul_(-0.5)
    w2 = st._pk_tail()[0]
    po, ff2 = st.proj_out, st.transformer_blocks[0].ff.net[2]
    assert w2 is not w1 and torch.equal(w2, L.fold_ff_tail(po.weight, po.bias, ff2.weight, ff2.bias)[0])
    want = (po.weight.detach().double().reshape(320, 320) @ ff2.weight.detach().double()).cpu()
    assert float((w2[:, 320:].double().cpu() - want).abs().max()) <= 2.0 ** -11 * float(want.abs().max())      # one rounding
    assert not torch.equal(st.hip(p["x"].cuda(), kv), y1)


def test_default_folds_from_1024_rows_up():
    """the class defaults: 2 x 32 x 16 tokens = 1024 rows fold, within the gate above of the two launches' error against fp64 and
    with the statistics riding on the output; 128 rows keep the two launches"""
    import copy
    from lib.hip import ops
    from lib.model_zoo import attention as AT
    assert AT.SpatialTransformer.ff_tail_fold and AT.SpatialTransformer.ff_tail_fold_min_rows == 1024
    small, p = problem(320, 2, False), problem(320, 2, False, 32, 16)
    st = copy.deepcopy(p["st"]).half().cuda()
    calls = []
    real = ops.gemm
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(ops, "gemm", lambda *a, **k: (calls.append(k.get("a2") is not None), real(*a, **k))[1])
        st.hip(small["x"].cuda(), AT.ContextKV(small["ctx"].cuda()))
        assert not any(calls) and "ff_tail" not in st.__dict__.get("_pk_cache", {})
        y = st.hip(p["x"].cuda(), AT.ContextKV(p["ctx"].cuda()))
        assert sum(calls) == 1 and calls[-1]
        mp.setattr(AT.SpatialTransformer, "ff_tail_fold", False)
        y0 = st.hip(p["x"].cuda(), AT.ContextKV(p["ctx"].cuda()))
    e_two, e_fold = scaled_err(y0, p["ref"]), scaled_err(y, p["ref"])
    print(f"[ff-tail-fold] 1024 rows, default switches: scaled max-abs two launches {e_two:.3e}, folded {e_fold:.3e}")
    assert 0 < e_two < 1e-2 and e_fold <= 2 * e_two
    assert ops.get_gn_stats(y) is not None and stats_ratio(y, ops.get_gn_stats(y)) <= 1.0
