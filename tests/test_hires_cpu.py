"""CPU: the start of the second pass of a two-pass ("hires fix") request as lib/hires.py specifies it -- against torch's
interpolate in float64, written out element by element from Python integers, the identity, the noise stream, and every named
mutant of the specification against the tolerance a device implementation will be held to (tests/hires_refs.py)."""
import numpy as np
import pytest
import torch

import hires_refs as R


# ---- the specification -----------------------------------------------------------------------------------------------
def test_hires_steps_modes_and_scalars():
    from lib import hires, img2img, noise
    assert hires.hires_steps(4, 0.5) == 2 == img2img.start_steps(4, 0.5) and hires.hires_steps(50, 1.0) == 50
    for steps, strength in ((50, 0.01), (50, 0), (50, 1.01), (50, float('nan'))):
        with pytest.raises(ValueError):
            hires.hires_steps(steps, strength)
    assert hires.MODES == R.MODES and [hires.MODE_ID[m] for m in R.MODES] == [0, 1, 2]
    with pytest.raises(ValueError, match="hires_resample"):
        hires.check_mode('lanczos')
    sa, sb = hires.kernel_scalars(0.4375)
    assert sa.dtype == np.float32 and sa == np.float32(np.sqrt(0.4375)) and sb == np.float32(0.75)
    with pytest.raises(ValueError):
        hires.kernel_scalars(1.5)
    assert hires.STREAM_HIRES == noise.STREAM_HIRES == 4
    assert (noise.STREAM_STEP, noise.STREAM_Q, noise.STREAM_POSTERIOR, noise.STREAM_KEEP) == (0, 1, 2, 3)   # keep their bits
    for bad in ((8, 4), (0, 4)):       # there is no reduction
        with pytest.raises(ValueError):
            hires.taps(bad[0], bad[1], 'bicubic')
    with pytest.raises(ValueError):
        hires.hires_start(np.zeros((4, 8, 8)), 0, 0, 0.5, (8, 4))


@pytest.mark.parametrize("mode", R.MODES)
def test_resample_agrees_with_torch_where_the_rules_agree(mode):
    """fp64 against F.interpolate on float64 input (align_corners=False for the two interpolating modes) at the sizes
    where torch's fp32 nearest rule picks the integer rule's indices: 1e-12"""
    from lib import hires
    pairs_2d = [((8, 8), (12, 12)), ((5, 7), (9, 16)), ((8, 12), (16, 24)), ((6, 6), (6, 6)), ((3, 4), (11, 5)),
                ((64, 64), (96, 128)), ((64, 64), (80, 96)), ((7, 64), (16, 80))]
    assert {(a, b) for (h, w), (h2, w2) in pairs_2d for a, b in ((h, h2), (w, w2))} == set(hires.TORCH_NEAREST_AGREES)
    g = np.random.default_rng(5)
    worst = 0.0
    for (h, w), (h2, w2) in pairs_2d:
        x = 5.0 * g.standard_normal((2, 3, h, w))
        kw = {} if mode == 'nearest' else {'align_corners': False}
        want = torch.nn.functional.interpolate(torch.from_numpy(x), size=(h2, w2), mode=mode, **kw).numpy()
        got = hires.resample(x, h2, w2, mode)
        assert got.dtype == np.float64 and got.shape == want.shape
        e = float(np.abs(got - want).max())
        worst = max(worst, e)
        if mode == 'nearest':
            assert e == 0.0, ((h, w), (h2, w2))
        assert e <= 1e-12, ((h, w), (h2, w2), e)
    print(f"[hires] resample '{mode}' vs F.interpolate (float64): worst |diff| {worst:.2e} (tol 1e-12)")


def test_nearest_is_the_integer_rule():
    """the first size pair at which torch's fp32 floor(d * scale) leaves it: 14 -> 46 at d = 23 (23 * 14 = 7 * 46)"""
    from lib import hires
    idx, wt = hires.taps(14, 46, 'nearest')
    assert idx.shape == (46, 1) and int(idx[23, 0]) == 7 and int(idx[22, 0]) == 6 and np.all(wt == 1.0)
    assert int(idx.max()) == 13 and int(idx.min()) == 0 and bool(np.all(np.diff(idx[:, 0]) >= 0))
    assert "14 -> 46" in hires.__doc__ and "372" in hires.__doc__


def _scalar_taps(d, n_in, n_out, mode):
    """the rule of the issue, one output index at a time, in Python integers and fractions of them"""
    if mode == 'nearest':
        return [(min((d * n_in) // n_out, n_in - 1), 1.0)]
    num = (2 * d + 1) * n_in - n_out
    i0 = num // (2 * n_out)
    t = (num - i0 * 2 * n_out) / (2 * n_out)
    if mode == 'bilinear':
        if num < 0:
            i0, t = 0, 0.0
        return [(i0, 1.0 - t), (min(i0 + 1, n_in - 1), t)]
    A = -0.75
    inner = lambda u: ((A + 2) * u - (A + 3)) * u * u + 1          # noqa: E731
    outer = lambda u: ((A * u - 5 * A) * u + 8 * A) * u - 4 * A    # noqa: E731
    ws = (outer(t + 1), inner(t), inner(1 - t), outer(2 - t))
    return [(min(max(i0 - 1 + k, 0), n_in - 1), ws[k]) for k in range(4)]


@pytest.mark.parametrize("mode", R.MODES)
def test_one_sample_written_out_element_by_element(mode):
    from lib import hires, noise
    case = R.CASES[2]                                  # (2, 3, 3, 5, 5, 7)
    B, C, h, w, h2, w2 = case
    x, k = R.latent(case), R.keys(B)
    r, xt = R.reference(case, mode)
    assert r.shape == xt.shape == (B, C, h2, w2) and r.dtype == xt.dtype == np.float32
    b = B - 1
    z = noise.normal64(int(k[b, 0]), int(k[b, 1]), 0, C * h2 * w2, stream=4)
    sa, sb = (float(v) for v in hires.kernel_scalars(R.A_T))
    for c in range(C):
        for y in range(h2):
            for xo in range(w2):
                v = sum(wy * wx * float(x[b, c, iy, ix]) for iy, wy in _scalar_taps(y, h, h2, mode)
                        for ix, wx in _scalar_taps(xo, w, w2, mode))
                assert abs(v - float(r[b, c, y, xo])) <= 1e-6 * max(1.0, abs(v)), (c, y, xo)       # one fp32 rounding
                want = sa * v + sb * z[(c * h2 + y) * w2 + xo]
                assert abs(want - float(xt[b, c, y, xo])) <= 1e-6 * max(1.0, abs(want)), (c, y, xo)


def test_identity_is_the_input_bit_for_bit():
    from lib import hires
    x = R.latent(R.IDENTITY)
    for mode in R.MODES:
        r, xt = R.reference(R.IDENTITY, mode)
        assert np.array_equal(r, x), mode
        assert not np.array_equal(xt, x)
    w = hires.cubic_weights(0.0)
    assert w[0] == 0.0 and w[3] == 0.0 and w[1] == 1.0 and w[2] == 0.0
    idx, wt = hires.taps(6, 6, 'bicubic')
    assert np.array_equal(idx[:, 1], np.arange(6)) and np.all(wt[:, 0] == 0.0) and np.all(wt[:, 3] == 0.0) and np.all(wt[:, 1] == 1.0)
    assert np.allclose(hires.taps(8, 12, 'bicubic')[1].sum(axis=1), 1.0, atol=1e-15)


def test_stream_4_is_a_stream_of_its_own():
    """tests/test_img2img_cpu.py's bound: five standard errors of 4099 independent pairs"""
    from lib import noise
    for seed, sid in ((20, 3), (-1, 0), ((1 << 40) + 12345, 0x1_0000_0002)):
        s4 = noise.normal(seed, sid, 0, 4099, stream=noise.STREAM_HIRES)
        for other in (0, 1, 2, 3):
            o = noise.normal(seed, sid, 0, 4099, stream=other)
            assert np.abs(s4 - o).max() > 0.1 and abs(float(np.corrcoef(s4, o)[0, 1])) < 0.08, (seed, other)
        assert np.array_equal(noise.normal(seed, sid, 0, 4099), noise.normal(seed, sid, 0, 4099, stream=0))


def _is_the_specification(wrong, case, mode):
    """where a named mutant IS the specification, by reasoning: the tap mutants on an axis that is unchanged (t = 0: the
    inner tap alone, no tap past an edge) or has one source pixel (every tap is that pixel, the weights sum to one)"""
    B, C, h, w, h2, w2 = case
    trivial = lambda a, b: a == b or a == 1                      # noqa: E731
    both = trivial(h, h2) and trivial(w, w2)
    if wrong == 'align_corners':
        return mode == 'nearest' or both
    if wrong == 'catmull_rom':
        return mode != 'bicubic' or both
    if wrong == 'edge_zero':                                     # one source pixel is not trivial here: its neighbours are zeros
        return mode == 'nearest' or (h == h2 and w == w2)
    if wrong == 'nearest_round':
        return mode != 'nearest' or both
    if wrong == 'axes_swapped':
        return h * w2 == w * h2
    if wrong == 'element_index_of_input':
        return h == h2 and w == w2
    return False                                                 # stream_q, level_of_k: never


def test_every_mutant_leaves_the_tolerance():
    """the tolerance of tests/hires_refs.py tells lib/hires.py from each of its named neighbours on the shared inputs: by
    1e3 x TOL wherever the neighbour is not the specification itself, and there it is equal"""
    from lib.hires import MUTANTS
    assert set(MUTANTS) >= {'align_corners', 'catmull_rom', 'edge_zero', 'axes_swapped', 'nearest_round', 'stream_q',
                            'level_of_k', 'element_index_of_input'}
    moved = {w: 0 for w in MUTANTS}
    for case in R.ALL_CASES:
        for mode in R.MODES:
            r, xt = R.reference(case, mode)
            for w in MUTANTS:
                wr, wt = R.mutant(case, mode, w)
                e = max(R.scaled_err(wr, r), R.scaled_err(wt, xt))
                if _is_the_specification(w, case, mode):
                    assert e == 0.0, (case, mode, w, e)
                else:
                    assert e > 1e3 * R.TOL, (case, mode, w, e)
                    moved[w] += 1
    assert all(moved.values()), moved
    with pytest.raises(ValueError):
        R.mutant(R.CASES[0], 'bicubic', 'something_else')
