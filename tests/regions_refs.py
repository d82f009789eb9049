"""Helpers of the regional-mixing tests (tests/test_regions_*.py): the cases, logit tables and region maps of the kernel tests, the
fp64 regional attention on torch tensors in the layouts the kernels take (pinned to lib/regions.regional_attention, the numpy
specification, by tests/test_regions_cpu.py), and operands that tell every
named mutant of lib/regions.py from the specification.  Imports kernel_refs and refmix_refs; changes nothing in them.

The bound is refmix_refs.kbias_bound with Bmax and T taken over the table: the accumulator start is the same construction (the
logit of the lane's own region instead of a broadcast one).  The handling of masked leading tiles adds no arithmetic and no term:
the running maximum starts at a finite -2^100 log2 units instead of -inf, the rescale factor of the first live tile is
exp2(-2^100 - m) = 0 exactly as exp2(-inf) is, and it multiplies accumulators that are still 0."""
import functools
import math

import numpy as np
import torch

import kernel_refs as KR
import refmix_refs as RR

from lib import refmix, regions

RBIAS_CLASSES = ("w4", "d80", "d160")          # no folded 8-wave build: the 4-wave d = 40 kernel takes those shapes
# (B, H, Nq, Nk, D): the smallest shapes of refmix_refs.KBIAS_CASES that reach each class
RBIAS_CASES = {
    "w4": [(1, 2, 300, 148, 40), (1, 2, 130, 129, 40), (3, 2, 64, 296, 40), (1, 2, 300, 444, 40)],
    "d80": [(1, 2, 150, 296, 80)],
    "d160": [(2, 2, 64, 296, 160)],
}
ALL_CASES = [(cls, c) for cls in RBIAS_CLASSES for c in RBIAS_CASES[cls]]
W8_SHAPE = (16, 8, 1024, 296, 40)              # pfd_attention_kbias_f16 folds this one; here it is the 4-wave kernel's
NR = 8
# what row g of a table is (the same for every sample; the numbers differ)
ROW_KINDS = ("leading_masked", "trailing_masked", "middle_masked", "random", "zero", "two_refs", "leading_masked_2", "random")
case_id = RR.case_id


def rbias_kernel_class(B, H, Nq, Nk, D):
    """which kernel pfd_attention_rbias_f16 launches.  None: PFD_ESHAPE."""
    return KR.attention_kernel_class(B, H, Nq, Nk, D, operand="rbias")


@functools.lru_cache(maxsize=None)
def table(case):
    """fp32 [B, NR, kb_stride(Nk)] (CPU): the logits of keys 0 .. Nk - 1 per region, NaN behind them.  Row
      0  masks every key below max(64, Nk // 2): the first key tile in full (a region that uses only the second reference)
      1  masks every key from Nk // 2 on: trailing tiles in full
      2  masks keys 64 .. 127 (a middle tile; the tail where Nk < 128) and every fifth key, key 0 finite
      3  random in [-12, 0]
      4  all 0
      5  two references 0.7 / 0.3 (refmix.key_bias)
      6  masks every key below 128 where Nk > 192 (two leading tiles), else like row 0
      7  random in [-12, 0]
    Every row keeps a finite key; rows 1 2 3 4 5 7 have key 0 finite.  Do not modify the result."""
    B, H, Nq, Nk, D = case[:5]
    assert Nk >= 66
    g = torch.Generator().manual_seed(Nk * 7919 + B * 31 + D + 77)
    out = torch.full((B, NR, RR.kb_stride(Nk)), float("nan"), dtype=torch.float32)
    j = torch.arange(Nk)
    for b in range(B):
        for r, kind in enumerate(ROW_KINDS):
            row = -12.0 * torch.rand(Nk, generator=g)
            if kind == "leading_masked":
                row[j < max(64, Nk // 2)] = float("-inf")
            elif kind == "trailing_masked":
                row[j >= Nk // 2] = float("-inf")
            elif kind == "middle_masked":
                row[((j >= 64) & (j < 128)) | ((j % 5 == 0) & (j > 0))] = float("-inf")
            elif kind == "zero":
                row = torch.zeros(Nk)
            elif kind == "two_refs":
                row = torch.from_numpy(refmix.key_bias((0.7, 0.3) if b % 2 == 0 else (0.3, 0.7), Nk // 2, Nk))
            elif kind == "leading_masked_2":
                row[j < (128 if Nk > 192 else 64)] = float("-inf")
            assert bool(torch.isfinite(row).any())
            out[b, r, :Nk] = row
    return out


KEY0_ROWS = tuple(r for r, k in enumerate(ROW_KINDS) if k not in ("leading_masked", "leading_masked_2"))


@functools.lru_cache(maxsize=None)
def region_map(case, shared):
    """uint8 [Nq] (shared) or [B, Nq]: the region changes every 9 queries (inside a wave's 32) and once more at every multiple of
    32 (wave and block boundaries); sample b is shifted by 3 b; the last query (ragged Nq) is put into region 7.  Every id
    0 .. 7 occurs.  Do not modify the result."""
    B, H, Nq, Nk, D = case[:5]
    i = torch.arange(Nq)
    rows = []
    for b in range(1 if shared else B):
        m = (i // 9 + i // 32 + 3 * b) % NR
        m[-1] = 7
        assert set(m.tolist()) == set(range(NR))
        rows.append(m.to(torch.uint8))
    return rows[0] if shared else torch.stack(rows)


def problem(case):
    return RR.problem(case)


def regional_ref(q, k, vt, tab, qreg, B, H, Nq, Nk, D, scale, *, ldq, ldk, ldvt, q_bs, k_bs, vt_bs, q_off=0, k_off=0, vt_off=0):
    """lib/regions.regional_attention on the flat fp16 operands of a launch (any device), in fp64 torch: tab [B or 1, NR, >= Nk]
    in log2 units, qreg uint8 [Nq] or [B, Nq].  -> ([B, Nq, H * D], T) with T = the largest |biased score| (log2 units) among
    the live (query, key) pairs."""
    Q, K, V = KR._attn_views(q, k, vt, B, H, Nq, Nk, D, ldq, ldk, ldvt, q_bs, k_bs, vt_bs, q_off, k_off, vt_off)
    out = torch.empty((B, Nq, H * D), dtype=torch.float64, device=q.device)
    T = 0.0
    for b in range(B):
        reg = (qreg if qreg.dim() == 1 else qreg[b])[:Nq].to(device=q.device, dtype=torch.long)
        rows = tab[b if tab.shape[0] > 1 else 0, :, :Nk].to(device=q.device, dtype=torch.float64)[reg]     # [Nq, Nk]
        live = torch.isfinite(rows)
        t = (Q[b].double() @ K[b].double().transpose(-1, -2)) * (scale * KR.LOG2E)                           # [H, Nq, Nk]
        tb = torch.where(live, t + torch.where(live, rows, 0.0), float("-inf"))
        T = max(T, float(tb[live.expand_as(tb)].abs().max()))
        p = torch.exp2(tb - tb.amax(-1, keepdim=True))
        # V of a key no query of the launch sees live may hold anything finite (never NaN inside Nk: the contract)
        out[b] = ((p @ V[b].double()) / p.sum(-1, keepdim=True)).transpose(0, 1).reshape(Nq, H * D)
    return out, T


def table_max(tab, Nk):
    t = tab[..., :Nk]
    return float(t[torch.isfinite(t)].abs().max())


def bound(Nk, D, vmax, T, Bmax):
    return RR.kbias_bound(Nk, D, vmax, T, Bmax)


# ------------------------------------------------------------------------------------------------
# operands that tell every mutant of lib/regions.py from the specification (shared by the CPU and the GPU kernel tests)
# ------------------------------------------------------------------------------------------------
# two references of 74 tokens, 36 queries = a 6 x 6 grid; every head and query holds the same numbers
DISC_DIMS = {"w4": (2, 1, 36, 148, 40), "d80": (2, 1, 36, 148, 80), "d160": (2, 1, 36, 148, 160)}
DISC_GRID = (6, 6)


@functools.lru_cache(maxsize=None)
def discriminating(mutant, cls="w4"):
    """one problem per mutant on which the specification gives +1 where the mutant gives -1 (or the other way round): every query
    and key along one sign vector u, so that the score of key j is a chosen t_j (log2 units) for every query; keys 0 .. 73 are
    reference 0 (V = +1), 74 .. 147 reference 1 (V = -1).  Two regions: row 0 masks reference 1, row 1 masks reference 0 -- the
    whole first key tile -- so a query answers +1 in region 0 and -1 in region 1.
      region_ignored, region_of_next_query   regions alternate from query to query
      table_of_sample0                       sample 1 has the two rows swapped
      masked_leading_tile_scored_zero        the live keys of region 1 at -12: 64 masked keys scored 0 outweigh them 2^12 to 1
      grid_transposed                        a left / right map on the 6 x 6 grid (transposed: top / bottom)
      grid_top_left                          a 12 x 12 map with region 1 on the pixels (odd row, odd column) only: under every
                                             cell's centre, never at a cell's top-left corner
    -> dict(q, k, vt flat fp16; desc; scale; table fp32 [B, 2, Nk]; qreg uint8 [B, Nq]; map uint8 or None; dims)"""
    assert mutant in regions.MUTANTS
    B, H, Nq, Nk, D = DISC_DIMS[cls]
    assert rbias_kernel_class(B, H, Nq, Nk, D) == cls and DISC_GRID[0] * DISC_GRID[1] == Nq
    t_ref = Nk // 2
    scale = D ** -0.5
    c = scale * KR.LOG2E
    g = torch.Generator().manual_seed(regions.MUTANTS.index(mutant) + 23)
    u = torch.sign(torch.randn(D, generator=g))
    inB = torch.arange(Nk) >= t_ref
    t = torch.where(inB, torch.tensor(-12.0 if mutant == "masked_leading_tile_scored_zero" else 0.0), torch.tensor(0.0))
    v = torch.where(inB, -1.0, 1.0)
    rowA = torch.where(inB, float("-inf"), 0.0)
    rowB = torch.where(inB, 0.0, float("-inf"))
    tab = torch.stack([rowA, rowB])[None].repeat(B, 1, 1)
    if mutant == "table_of_sample0":
        tab[1] = torch.stack([rowB, rowA])
    m = None
    if mutant == "grid_transposed":
        m = np.zeros((12, 12), dtype=np.uint8)
        m[:, 6:] = 1                                        # left / right
        qreg = torch.from_numpy(regions.region_grid(m, *DISC_GRID, nr=2))
    elif mutant == "grid_top_left":
        m = np.zeros((12, 12), dtype=np.uint8)
        m[1::2, 1::2] = 1                                   # the pixel under every cell's centre is (2 y + 1, 2 x + 1): all region 1;
        qreg = torch.from_numpy(regions.region_grid(m, *DISC_GRID, nr=2))      # its top-left pixel (2 y, 2 x): all region 0
        assert bool((qreg == 1).all())
    else:
        qreg = (torch.arange(Nq) % 2).to(torch.uint8)
    qreg = qreg[None].repeat(B, 1).contiguous()
    C = H * D
    uh = u.repeat(H)
    Q = uh[None, None].expand(B, Nq, C).half()
    K = ((t / (D * c))[None, :, None] * uh).expand(B, Nk, C).half()
    Nkp = (Nk + 7) // 8 * 8
    vt = KR._poisoned(C * B * Nkp).view(C, B, Nkp)
    vt[:, :, :Nk] = v.half()[None, None].expand(C, B, Nk)
    desc = dict(ldq=C, ldk=C, ldvt=B * Nkp, q_bs=Nq * C, k_bs=Nk * C, vt_bs=Nkp)
    return dict(q=Q.reshape(-1).contiguous(), k=K.reshape(-1).contiguous(), vt=vt.reshape(-1), desc=desc, scale=scale,
                table=tab.float(), qreg=qreg, map=m, vmax=1.0, dims=(B, H, Nq, Nk, D))


def spec_operands(p):
    B, H, Nq, Nk, D = p["dims"]
    d = p["desc"]
    Q, K, V = KR._attn_views(p["q"], p["k"], p["vt"], B, H, Nq, Nk, D, d["ldq"], d["ldk"], d["ldvt"], d["q_bs"], d["k_bs"],
                             d["vt_bs"], 0, 0, 0)
    return tuple(a.double().numpy() for a in (Q, K, V))


def mutant_output(p, mutant):
    """what `mutant` computes on problem p, through lib/regions.py (numpy, fp64) -> [B, H, Nq, D]"""
    q, k, v = spec_operands(p)
    tab, qreg = p["table"].double().numpy(), p["qreg"].numpy()
    if mutant in regions.GRID_MUTANTS:
        qreg = regions.region_grid(p["map"], *DISC_GRID, nr=2, wrong=mutant)
        return regions.regional_attention(q, k, v, tab, qreg, p["scale"])
    return regions.regional_attention(q, k, v, tab, qreg, p["scale"], wrong=mutant)


def padded_table(tab, Nk):
    """[B, NR, Nk] -> [B, NR, kb_stride(Nk)] with NaN behind the keys (what a launch is handed)"""
    out = torch.full(tab.shape[:2] + (RR.kb_stride(Nk),), float("nan"), dtype=torch.float32)
    out[..., :Nk] = tab
    return out


# ------------------------------------------------------------------------------------------------
# block_refs extended by the regional attention (block_refs.py itself is not touched)
# ------------------------------------------------------------------------------------------------
import contextlib


@contextlib.contextmanager
def regional_cross_attention(tab, maps, seen=None):
    """inside the block: block_refs.cross_attention with the logits of the query's region wherever a context is given -- softmax
    over scale q k^T + ln 2 * tab[b, maps[N][b, i], :] for the N queries of the call (tab [B, NR, Nk] in log2 units, -inf = no
    such key for that region; maps: {N: integer tensor [B, N]}); self-attention is what it was.  seen: a set that collects the N
    of every context call (how a test learns which query grids a block runs).  The block formulas are block_refs' own."""
    import block_refs as BR
    orig = BR.cross_attention

    def cross_attention(p, x, context, heads, wrong=None):
        if context is None:
            return orig(p, x, context, heads, wrong)
        q, k, v = BR.linear(p.sub("to_q."), x), BR.linear(p.sub("to_k."), context), BR.linear(p.sub("to_v."), context)
        B, N, Cd = q.shape
        if seen is not None:
            seen.add(int(N))
        if maps is None:
            return orig(p, x, context, heads, wrong)
        d = Cd // heads
        sp = lambda t: t.reshape(B, -1, heads, d).permute(0, 2, 1, 3)  # noqa: E731
        q, k, v = sp(q), sp(k), sp(v)
        rows = torch.stack([tab[b].to(q.dtype)[maps[int(N)][b].long()] for b in range(B)])          # [B, N, Nk]
        s = (q @ k.transpose(-1, -2)) * d ** -0.5 + (rows * math.log(2.0))[:, None]
        return BR.linear(p.sub("to_out.0."), (s.softmax(dim=-1) @ v).permute(0, 2, 1, 3).reshape(B, N, Cd))
    BR.cross_attention = cross_attention
    try:
        yield
    finally:
        BR.cross_attention = orig


def block_regions(B, t, sizes):
    """a table and maps for a block with two references of t tokens: region 0 listens to reference 0 alone, region 1 to reference
    1 alone (the leading t keys masked), region 2 to both at 0.7 / 0.3; sample b starts its regions at b, a region lasts five
    queries.  -> (fp32 [B, 3, 2 t], {N: uint8 [B, N]})"""
    w = [[1.0, 0.0], [0.0, 1.0], [0.7, 0.3]]
    tab = torch.from_numpy(regions.region_bias(w, t, 2 * t))[None].repeat(B, 1, 1)
    maps = {int(n): torch.stack([((torch.arange(n) // 5 + b) % 3).to(torch.uint8) for b in range(B)]) for n in sizes}
    return tab, maps
