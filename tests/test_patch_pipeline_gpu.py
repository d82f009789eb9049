"""GPU (-m gpu): the fragment pipeline of the wave-specialised 3x3 patch kernel (conv3x3_patch_ws_kernel).  Its
consumer waves read the A fragments of a tap's first half step BEFORE the barrier of that tap, from the patch buffer of the
current channel block.  The CPU emulation cannot see a premature read (a copy lands when it is issued there), so this file
covers it on hardware: every shape below runs through pfd_gemm_f16_ex as tests/test_gemm_kernels_gpu.py does, under the
heuristic and under the forced forms 96 (3-stage weight ring), 98 (two weight stages; the GroupNorm-prologue instances) and
99 (the 8-wave kernel without loader waves, whose loop is untouched), against the fp64 reference and bound of
tests/kernel_refs.py, and bit for bit across the forms of one split count.  Every 64-channel block of the image comes from
its own seed and sits at its own level, so that a fragment from the other patch buffer, or from a buffer that is not complete,
cannot cancel: one channel block, two (one hand-over), three (both hand-overs and one buffer reuse), five; split-K slices of
two, two and ONE block; whole-row tiles and pixel tiles (pt_w 16 / 32)."""
import zlib

import pytest
import torch

import kernel_refs as KR
import test_gemm_kernels_gpu as G

pytestmark = pytest.mark.gpu

FORMS = (0, 96, 98, 99)


def heuristic_splits(M, N, Cin):
    """the split count the dispatcher takes for a patch problem (pfd_gemm160_try, restated): aim at 256 blocks below 200
    tiles, at most 8 slices, at least two channel blocks per slice"""
    tl, ncb, s = (M // 256) * (N // 160), Cin // 64, 1
    if tl < 200:
        s = min(8, -(-256 // tl))
        while s > 1 and ncb // s < 2:
            s -= 1
    return s


ROWVEC = dict(bias=True, rowvec=True)
RES_GN = dict(bias=True, res=True, gn_out=True)


def _problems():
    """name -> (B, H, W, Cin, N, forced split count or 0, case options)"""
    P = {}
    for Cin in (64, 128, 192, 320):
        for N in (160, 320):
            P[f"16x16-c{Cin}-n{N}-rowvec"] = (1, 16, 16, Cin, N, 0, ROWVEC)
        P[f"16x16-c{Cin}-n320-res-gn_out"] = (1, 16, 16, Cin, 320, 0, RES_GN)
    for W, H in ((32, 8), (64, 4), (48, 16), (96, 8)):      # 48: pt_w 16, three tiles; 96: pt_w 32
        P[f"{W}x{H}-c128-n160-rowvec"] = (1, H, W, 128, 160, 0, ROWVEC)
    P["2x16x16-c256-n160-rowvec-forced2"] = (2, 16, 16, 256, 160, 2, ROWVEC)
    P["2x16x16-c320-n160-rowvec-forced3"] = (2, 16, 16, 320, 160, 3, ROWVEC)      # slices of 2, 2 and 1 channel blocks
    P["2x16x16-c320-n320-res-gn_out-forced3"] = (2, 16, 16, 320, 320, 3, RES_GN)
    for Cin in (128, 192):
        for c1, silu in ((Cin, False), (Cin, True), (64, True)):
            P[f"16x16-c{Cin}-n160-prologue-{c1}{'+' + str(Cin - c1) if c1 < Cin else ''}{'-silu' if silu else ''}"] = \
                (1, 16, 16, Cin, 160, 0, dict(ROWVEC, gn_pro=(c1, silu)))
    P["48x16-c128-n160-prologue-64+64-silu"] = (1, 16, 48, 128, 160, 0, dict(ROWVEC, gn_pro=(64, True)))
    return P


PROBLEMS = _problems()


def _forms(name):
    return (0, 98) if "prologue" in name else FORMS      # a GroupNorm prologue is served by the two-stage loader form only


def _case(name, v):
    B, H, W, Cin, N, s, opt = PROBLEMS[name]
    geo, M, K, hw = KR._conv_geom(B, H, W, Cin)
    hs = heuristic_splits(M, N, Cin)
    if opt.get("gn_pro") is not None:
        kernel = f"conv3x3_patch_ws_kernel<{2 if opt['gn_pro'][1] else 1}, 2>"
    else:
        kernel = "conv3x3_patch_ws_kernel<0, 3>" if v == 0 else None
    return KR._wide(f"{name}-v{v}", "patch", v, s, M, N, K, conv=True, rows_per_rv=hw, hsplit=0 if s else hs, kernel=kernel, **opt, **geo)


_problem_cache = {}


def _problem(name, v):
    """operands as kernel_refs.gemm_problem lays them out, the image drawn per 64-channel block: block b from seed (name, b),
    centred at 0.25 (b + 1) with spread 1 + b / 4"""
    c = _case(name, v)
    if name not in _problem_cache:
        B, H, W, Cin = c["image"]
        M, N, K = c["M"], c["N"], c["K"]
        blocks = []
        for b in range(Cin // 64):
            g = torch.Generator().manual_seed(zlib.crc32(f"{name}/block{b}".encode()))
            blocks.append(torch.randn((B, H, W, 64), generator=g) * (1 + b / 4) + 0.25 * (b + 1))
        x = torch.cat(blocks, -1)
        g = torch.Generator().manual_seed(zlib.crc32(name.encode()))
        rn = lambda *s: torch.randn(s, generator=g)
        q = dict(A2=None, bias=None, rowvec=None, R=None, gn_table=None)
        c1 = c["gn_pro"][0] if c["gn_pro"] is not None else Cin
        q["A"] = x[..., :c1].half()
        if c1 < Cin:
            q["A2"] = x[..., c1:].half()
        if c["gn_pro"] is not None:      # the GroupNorm(32) table of the image in fp64, rounded to fp32 (as kernel_refs.gemm_problem)
            xc = x.half().double().reshape(B, H * W, 32, Cin // 32)
            mean = xc.mean((1, 3), keepdim=True)
            rstd = 1.0 / torch.sqrt((xc * xc).mean((1, 3), keepdim=True) - mean * mean + 1e-5)
            gamma, beta = (1 + 0.2 * rn(Cin)).double().reshape(32, -1), (0.1 * rn(Cin)).double().reshape(32, -1)
            scale = (rstd[:, 0] * gamma).reshape(B, Cin)
            shift = (beta - mean[:, 0] * rstd[:, 0] * gamma).reshape(B, Cin)
            q["gn_table"] = torch.stack([scale, shift], 1).float()
            act = KR.ACT_SILU if c["gn_pro"][1] else KR.ACT_NONE
            xx, tab = x.half(), q["gn_table"]
            v64 = KR.activation_ref(xx.double() * tab[:, None, None, 0].double() + tab[:, None, None, 1].double(), act, torch.float64)
            v32 = KR.activation_ref(xx.float() * tab[:, None, None, 0] + tab[:, None, None, 1], act, torch.float32)
            q["pro_delta"] = KR.fp32_allowance(v64, v32)
        q["W"] = (rn(N, K) * K ** -0.5).half()
        if c["bias"]:
            q["bias"] = (0.5 * rn(N)).half()
        if c["rowvec"]:
            q["rowvec"] = (0.5 * rn(B, N)).half()
        if c["res"]:
            q["R"] = rn(M, N).half()
        _problem_cache[name] = q
    return dict(_problem_cache[name], case=c)


_ref_cache = {}


def _ref(name):
    """fp64 reference of the problem, computed once (it does not depend on the form)"""
    if name not in _ref_cache:
        _ref_cache[name] = KR.gemm_ref(_problem(name, _forms(name)[0]))["out"]
    return _ref_cache[name]


_ran = {}


def _run(name, v):
    """one launch into a sentinel-framed column slice; the stored values (and the GroupNorm statistics) on the CPU"""
    if (name, v) in _ran:
        return _ran[name, v]
    from lib.hip import ops
    p = _problem(name, v)
    c = p["case"]
    M, N = c["M"], c["N"]
    d = G._device_operands(p)
    buf, out, _, n_out = G._outputs(c)
    ks, stride, pad, ups, Ho, Wo = c["geom"]
    kw = dict(stride=stride, pad=pad, bias=d["bias"], rowvec=d["rowvec"], res=d["R"], out=out, tile=c["tile"], out_hw=(Ho, Wo), gn_out=c["gn_out"])
    if c["gn_pro"] is not None:
        kw["gn"] = (d["gn_table"], d.get("A2"), c["gn_pro"][1])
    r = ops.conv(d["A"], d["W"], ks, **kw)
    torch.cuda.synchronize()
    assert r.data_ptr() == out.data_ptr()
    assert bool((buf[M:] == G.SENTINEL).all()) and bool((buf[:M, :8] == G.SENTINEL).all()) and bool((buf[:M, 8 + n_out:] == G.SENTINEL).all())
    got = dict(out=buf[:M, 8:8 + n_out].contiguous().cpu())
    assert bool(torch.isfinite(got["out"]).all()) and not bool((got["out"] == G.SENTINEL).any())
    if c["gn_out"]:
        st = ops.get_gn_stats(r)
        assert st is not None
        got["gn_out"] = st.reshape(M // 64, N // 160, 16, 2)[:, :, :160 // (N // 32)].cpu()
    _ran[name, v] = got
    return got


@pytest.mark.parametrize("name,v", [(n, v) for n in sorted(PROBLEMS) for v in _forms(n)])
def test_patch_conv_vs_fp64(name, v):
    p = _problem(name, v)
    c = p["case"]
    M, N = c["M"], c["N"]
    got = _run(name, v)
    a = KR.gemm_allowance(p, c["splits"], True)["out"]
    ratio, used = KR.bound_ratio(got["out"], _ref(name), a)
    parts = [f"out err / bound {ratio:.3f}, allowance used {used:.3f}"]
    worst = ratio
    if "gn_out" in got:                # fp32 sums of n = 64 N / 32 stored values (the bound of tests/test_gemm_kernels_gpu.py)
        cpg = N // 32
        want = KR.gn_out_ref(got["out"])[:, :, :160 // cpg]
        vv = got["out"].double().reshape(M // 64, 64, N // 160, 160 // cpg, cpg)
        bnd = 64 * cpg * 2.0 ** -24 * torch.stack([vv.abs().sum((1, 4)), (vv * vv).sum((1, 4))], -1)
        r2 = float(((got["gn_out"].double() - want).abs() / bnd).max())
        parts.append(f"gn_out err / bound {r2:.3f}")
        worst = max(worst, r2)
    print(f"[patch-pipeline] {name} v{v} splits {c['splits']}: " + "; ".join(parts))
    assert worst <= 1.0, (name, v, parts)


@pytest.mark.parametrize("name", sorted(PROBLEMS))
def test_forms_of_one_problem_are_bitwise_equal(name):
    """same split count, same summation order: the heuristic, the two loader-wave forms and the 8-wave kernel store the same bits"""
    forms = _forms(name)
    splits = {v: _case(name, v)["splits"] for v in forms}
    assert len(set(splits.values())) == 1, splits
    base = _run(name, forms[-1])       # 99 (the loop this change does not touch) where it serves the problem
    for v in forms[:-1]:
        g = _run(name, v)
        n = int((g["out"] != base["out"]).sum())
        assert n == 0, f"{name}: form {v} differs from form {forms[-1]} in {n} elements"
