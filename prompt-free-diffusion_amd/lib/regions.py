"""Regional reference mixing: WHICH reference a query listens to depends on where it lies -- numpy only, fp64.

lib/refmix.py gives every key one weight for the whole picture.  Here a request carries a region map (a uint8 picture whose
pixel value is the region id) and one weight row per region; query i of sample b lies in region g = qreg[b, i] and sees key j
at the weight of its reference IN THAT REGION:

    O[b,i,h,:] = sum_j 2^table[b,g,j] exp(s_ij) V[b,j,h,:] / sum_j 2^table[b,g,j] exp(s_ij),    s_ij = scale <Q[b,i,h,:], K[b,j,h,:]>

What the device is handed (pfd_attention_rbias_f16, include/pfd_hip.h) is `region_bias` -- row g is refmix.key_bias of region
g's weights, with a zero weight MASKED (-inf) instead of dropped, because another region may use that reference -- and
`region_grid`, the map reduced to the query grid of one UNet level.  `regional_attention` is the specification of what it
computes with them.

The contract is weaker than the per-key operand's "key 0 is finite": every region id that occurs among a sample's queries keeps
at least one finite key SOMEWHERE.  A region that uses only the second reference masks the whole first key tile.
"""
import numpy as np

from . import refmix

MAX_REGIONS = 8
MAX_REFS = refmix.MAX_REFS
# named ways to get it wrong (tests/test_regions_cpu.py shows that the tolerance of the GPU tests tells the specification from each)
ATTN_MUTANTS = ('region_ignored', 'region_of_next_query', 'table_of_sample0', 'masked_leading_tile_scored_zero')
GRID_MUTANTS = ('grid_transposed', 'grid_top_left')
MUTANTS = ATTN_MUTANTS + GRID_MUTANTS


def check_region_weights(region_weights):
    """-> float64 [NR, R]; ValueError unless 1 <= NR <= MAX_REGIONS, 1 <= R <= MAX_REFS, every weight finite and >= 0 and every
    row with at least one positive entry.  (A reference whose whole COLUMN is 0 is dropped by the caller before it is encoded,
    `drop_zero_columns`; it is legal here and is masked in every row.)"""
    w = np.asarray(region_weights, dtype=np.float64)
    if w.ndim != 2:
        raise ValueError(f"region_weights must be [NR, R], got shape {w.shape}")
    if not 1 <= w.shape[0] <= MAX_REGIONS:
        raise ValueError(f"between 1 and {MAX_REGIONS} regions, got {w.shape[0]}")
    if not 1 <= w.shape[1] <= MAX_REFS:
        raise ValueError(f"between 1 and {MAX_REFS} references can be mixed, got {w.shape[1]}")
    if not np.all(np.isfinite(w)) or np.any(w < 0):
        raise ValueError(f"region_weights must be finite and >= 0, got {w.tolist()}")
    if not np.all((w > 0).any(axis=1)):
        raise ValueError("every region needs at least one reference with a weight > 0")
    return w


def drop_zero_columns(region_weights):
    """-> (indices of the references kept, [NR, R'] weights): a reference no region uses is not encoded at all"""
    w = check_region_weights(region_weights)
    keep = [r for r in range(w.shape[1]) if np.any(w[:, r] > 0)]
    return keep, w[:, keep]


def region_bias(region_weights, tokens_per_ref, nkp):
    """fp32 [NR, nkp], log2 units: row g holds log2(w[g, r] / max_r w[g, :]) on the tokens_per_ref tokens of reference r, -inf
    where w[g, r] == 0 and behind the last reference.  With NR == 1 (and no zero) the row is refmix.key_bias bit for bit."""
    w = check_region_weights(region_weights)
    t, nkp = int(tokens_per_ref), int(nkp)
    NR, R = w.shape
    if t < 1 or R * t > nkp:
        raise ValueError(f"{R} references of {t} tokens do not fit {nkp} keys")
    out = np.full((NR, nkp), -np.inf, dtype=np.float64)
    for g in range(NR):
        rel = w[g] / w[g].max()
        with np.errstate(divide='ignore'):
            lg = np.log2(rel)                      # log2(0) = -inf: the masked reference
        lg[rel == 1.0] = 0.0
        out[g, :R * t] = np.repeat(lg, t)
    return out.astype(np.float32)


def region_grid(map_u8, h, w, nr=None, wrong=None):
    """uint8 [h * w]: the region of every query of an h x w grid.  map_u8 is a uint8 picture [Hm, Wm] of any size whose pixel
    value is the region id; cell (y, x) takes map[((2 y + 1) Hm) // (2 h), ((2 x + 1) Wm) // (2 w)] -- the pixel under the cell's
    centre by an exact integer rule, evaluated from the user's map for every level on its own (no pyramid).
    nr: if given, a value >= nr raises ValueError (on the host, before anything touches the device).
    wrong: None or one of GRID_MUTANTS."""
    if wrong is not None and wrong not in GRID_MUTANTS:
        raise ValueError(f"unknown mutant {wrong!r}")
    m = np.asarray(map_u8)
    if m.dtype != np.uint8 or m.ndim != 2 or m.shape[0] < 1 or m.shape[1] < 1:
        raise ValueError(f"the region map must be a uint8 picture [Hm, Wm], got {m.dtype} {m.shape}")
    h, w = int(h), int(w)
    if h < 1 or w < 1:
        raise ValueError(f"query grid {h} x {w}")
    if nr is not None and int(m.max()) >= int(nr):
        raise ValueError(f"the region map holds id {int(m.max())}, but there are only {int(nr)} regions")
    Hm, Wm = m.shape
    if wrong == 'grid_top_left':
        ys = [(y * Hm) // h for y in range(h)]
        xs = [(x * Wm) // w for x in range(w)]
    else:
        ys = [((2 * y + 1) * Hm) // (2 * h) for y in range(h)]
        xs = [((2 * x + 1) * Wm) // (2 * w) for x in range(w)]
    g = m[np.asarray(ys)[:, None], np.asarray(xs)[None, :]]
    if wrong == 'grid_transposed':
        if h != w:
            raise ValueError("the transposed-grid mutant is defined on square grids")
        g = g.T
    return np.ascontiguousarray(g).reshape(-1)


def level_sizes(h, w, n_levels):
    """the query grids a UNet of n_levels resolutions (a stride-2 convolution between them: ceil(h / 2)) runs at the latent
    size (h, w) -> [(h_l, w_l)], cut where the token count would repeat"""
    out = []
    for _ in range(int(n_levels)):
        if out and out[-1] == (h, w):
            break
        out.append((int(h), int(w)))
        h, w = (h + 1) // 2, (w + 1) // 2
    return out


def level_maps(map_u8, bs, h, w, n_levels, nr):
    """the user's map -- uint8 [Hm, Wm], or [bs, Hm, Wm] / a list of bs maps [Hm_b, Wm_b] with one map per sample (a list may
    hold maps of different sizes) -- reduced to every grid of `level_sizes` (each from the map itself)
    -> (uint8 [bs, sum_l h_l w_l], [h_l w_l]); ValueError for an id >= nr"""
    if isinstance(map_u8, (list, tuple)):
        m = [np.asarray(x) for x in map_u8]
        if len(m) != int(bs):
            raise ValueError(f"{len(m)} region maps for {bs} samples")
    else:
        m = np.asarray(map_u8)
        if m.ndim == 2:
            m = np.broadcast_to(m[None], (int(bs),) + m.shape)
        if m.ndim != 3 or m.shape[0] != int(bs) or m.dtype != np.uint8:
            raise ValueError(f"the region map must be uint8 [Hm, Wm] or [{bs}, Hm, Wm], got {m.dtype} {m.shape}")
    sizes = level_sizes(h, w, n_levels)
    rows = [np.concatenate([region_grid(m[b], hl, wl, nr=nr) for hl, wl in sizes]) for b in range(int(bs))]
    return np.stack(rows), [hl * wl for hl, wl in sizes]


def regional_attention(q, k, v, table, qreg, scale, wrong=None):
    """q [B, H, Nq, D], k / v [B, H, Nk, D], table [B, NR, Nk] (log2 units, finite or -inf), qreg [B, Nq] or [Nq] integers < NR
    -> float64 [B, H, Nq, D]: the formula of the module text.  Every region that occurs among a sample's queries has at least
    one finite key.  A key at -inf contributes exactly nothing, whatever its K and V hold.
    wrong: None or one of ATTN_MUTANTS."""
    if wrong is not None and wrong not in ATTN_MUTANTS:
        raise ValueError(f"unknown mutant {wrong!r}")
    q, k, v = (np.asarray(a, dtype=np.float64) for a in (q, k, v))
    table = np.asarray(table, dtype=np.float64)
    B, H, Nq, D = q.shape
    Nk = k.shape[2]
    if table.ndim != 3 or table.shape[0] != B or table.shape[2] != Nk or not 1 <= table.shape[1] <= MAX_REGIONS:
        raise ValueError(f"table must be [{B}, NR <= {MAX_REGIONS}, {Nk}], got {table.shape}")
    NR = table.shape[1]
    qreg = np.asarray(qreg)
    if qreg.ndim == 1:
        qreg = np.broadcast_to(qreg[None], (B, qreg.shape[0]))
    if qreg.shape != (B, Nq) or not np.issubdtype(qreg.dtype, np.integer):
        raise ValueError(f"qreg must be integers [{B}, {Nq}] or [{Nq}], got {qreg.dtype} {qreg.shape}")
    qreg = qreg.astype(np.int64)
    if qreg.min() < 0 or qreg.max() >= NR:
        raise ValueError(f"region ids must lie in 0 .. {NR - 1}")
    if np.any(np.isnan(table)) or np.any(table == np.inf):
        raise ValueError("table values are finite or -inf")
    if wrong == 'region_ignored':
        qreg = np.zeros_like(qreg)
    elif wrong == 'region_of_next_query':
        qreg = np.concatenate([qreg[:, 1:], qreg[:, -1:]], axis=1)
    if wrong == 'table_of_sample0':
        table = np.broadcast_to(table[:1], table.shape)
    rows = np.stack([table[b, qreg[b]] for b in range(B)])                          # [B, Nq, Nk]
    if not np.all(np.isfinite(rows).any(axis=-1)):
        raise ValueError("a region that occurs among the queries has no finite key")
    live = np.isfinite(rows)[:, None]                                               # [B, 1, Nq, Nk]
    t = np.einsum('bhid,bhjd->bhij', q, k) * (float(scale) * np.log2(np.e))          # log2 units
    b4 = np.where(live, rows[:, None], 0.0)
    if wrong == 'masked_leading_tile_scored_zero':
        # a kernel that cannot start on a masked tile: where a region's first 64 keys are all masked, those keys take part with
        # score 0 (and their V) instead of not at all
        lead = ~np.isfinite(rows[..., :64]).any(axis=-1)                            # [B, Nq]
        zero = np.zeros_like(live)
        zero[..., :64] = lead[:, None, :, None]
        tb = np.where(live, t + b4, np.where(zero, 0.0, -np.inf))
        live = live | zero
    else:
        tb = np.where(live, t + b4, -np.inf)
    p = np.where(live, np.exp2(tb - tb.max(-1, keepdims=True)), 0.0)
    den = p.sum(-1, keepdims=True)
    # (V of a masked key never meets a non-zero p; einsum over p = 0 and a finite V is exact)
    num = np.einsum('bhij,bhjd->bhid', p, np.nan_to_num(v))
    return num / den
