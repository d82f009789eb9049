"""CPU: masked regeneration -- lib/inpaint.py (the specification of csrc/inpaint.hip) and its mutants against the GPU
test's tolerance, the three kernels on the CPU emulation, the C ABI's argument checks, the sampler's masked loop over
tests/sampler_standin.py, and the pipeline / server layers over the stubs of the other CPU tests with stand-ins for the
new ops built on lib/inpaint.py."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import img2img_refs as I
import inpaint_refs as R
import sampler_standin as SS

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get("EMU_CXX", "/opt/rocm/lib/llvm/bin/clang++")


# ---- the specification's own properties ----------------------------------------------------------------------------------
def test_stream_3_is_a_stream_of_its_own():
    from lib import noise
    assert noise.STREAM_KEEP == 3 and (noise.STREAM_STEP, noise.STREAM_Q, noise.STREAM_POSTERIOR) == (0, 1, 2)
    src = open(os.path.join(REPO, "prompt-free-diffusion_amd", "csrc", "philox.h")).read()
    assert re.search(r"#define\s+PFD_STREAM_KEEP\s+3u\b", src)
    z3 = noise.normal(20, 3, 5, 4099, stream=noise.STREAM_KEEP)
    for s in (0, 1, 2):
        other = noise.normal(20, 3, 5, 4099, stream=s)
        assert np.abs(z3 - other).max() > 0.1 and abs(float(np.corrcoef(z3, other)[0, 1])) < 0.08


def test_blend_is_exact_at_mask_0_and_1():
    """m = 1 gives the unmasked update's bits, m = 0 gives known's; pred_x0 never depends on the mask"""
    from lib import inpaint, noise
    for form in R.FORMS:
        for last in (False, True):
            ones, zeros = R.case(form, R.SHAPES[0], 1, 'ones', last=last), R.case(form, R.SHAPES[0], 1, 'zeros', last=last)
            soft = R.case(form, R.SHAPES[0], 2, 'soft', last=last)
            xo1, p1, xin1 = R.reference(ones)
            xo0, p0, xin0 = R.reference(zeros)
            # the unmasked update, written out: what the blend of a zero-weight x0 = NaN-free known leaves untouched
            free = dict(ones, x0=np.zeros_like(ones['x0']), ks=np.float32(0), ksq=np.float32(0))
            assert np.array_equal(R.reference(free)[0], xo1), (form, last)
            B, C, h, w = ones['shape']
            zk = np.stack([noise.normal64(int(k[0]), int(k[1]), zeros['index'], C * h * w, stream=3) for k in zeros['keys']])
            known = float(zeros['ksq']) * zeros['x0'].astype(np.float64) + float(zeros['ks']) * zk.reshape(zeros['x0'].shape)
            assert np.array_equal(xo0, known.astype(np.float32)), (form, last)
            if last:
                assert (float(zeros['ksq']), float(zeros['ks'])) == (1.0, 0.0) and np.array_equal(xo0, zeros['x0'])
            assert np.array_equal(p1, p0) and np.array_equal(p1, R.reference(soft)[1])
            assert np.array_equal(xin1, np.transpose(xo1, (0, 2, 3, 1)).astype(np.float16))
    ksq, ks = inpaint.step_constants(0.5625, 3)
    assert ksq.dtype == np.float32 and ksq == np.float32(0.75) and ks == np.float32(np.sqrt(0.4375))
    assert inpaint.step_constants(0.5625, 0) == (1.0, 0.0)


@pytest.mark.parametrize("n_in", [1, 5, 7, 8, 9, 64, 72, 96, 100, 513])
@pytest.mark.parametrize("n_out", [1, 8, 64])
def test_footprints_cover_the_axis_and_are_never_empty(n_in, n_out):
    from lib.inpaint import footprint
    spans = [footprint(i, n_in, n_out) for i in range(n_out)]
    assert all(0 <= lo < hi <= n_in for lo, hi in spans)
    covered = np.zeros(n_in, dtype=bool)
    for lo, hi in spans:
        covered[lo:hi] = True
    assert covered.all() and spans[0][0] == 0 and spans[-1][1] == n_in
    assert all(a[0] <= b[0] and a[1] <= b[1] for a, b in zip(spans, spans[1:]))


def test_worked_masks_and_dilation():
    from lib import inpaint
    for m, want in R.worked_masks():
        got = inpaint.mask_grid(m, 8, 8)
        assert got.dtype == np.float32 and np.array_equal(got, want)
        assert np.array_equal(inpaint.mask_grid(m[:, :, None], 8, 8, np.uint8), want.astype(np.uint8))
    (a, wa), _ = R.worked_masks()
    assert int(wa.sum()) == 16 and int((1 - wa).sum()) == 48
    # one marked pixel marks its cell, whatever the sizes; 127 marks nothing
    for (Hm, Wm), (gh, gw) in R.GRIDS:
        for y, x in ((0, 0), (Hm - 1, Wm - 1), (Hm // 2, Wm // 3)):
            m = np.full((Hm, Wm), 127, dtype=np.uint8)
            assert inpaint.mask_grid(m, gh, gw).sum() == 0
            m[y, x] = 128
            g = inpaint.mask_grid(m, gh, gw)
            assert g.sum() >= 1
            cy = [i for i in range(gh) if inpaint.footprint(i, Hm, gh)[0] <= y < inpaint.footprint(i, Hm, gh)[1]]
            cx = [i for i in range(gw) if inpaint.footprint(i, Wm, gw)[0] <= x < inpaint.footprint(i, Wm, gw)[1]]
            assert all(g[i, j] == 1 for i in cy for j in cx) and g.sum() == len(cy) * len(cx)
    with pytest.raises(ValueError):
        inpaint.mask_grid(np.zeros((4, 4), dtype=np.float32), 2, 2)


def test_composite_specification():
    from lib import inpaint
    dec, init = I.picture_u8(16, 24, 1)[None].repeat(2, 0), I.picture_u8(16, 24, 2)[None]
    dec[1] = 255 - dec[1]
    sel = (R.mask_u8(16, 24) >= 128).astype(np.uint8)[None]
    out = inpaint.composite(dec, init, sel)
    assert out.dtype == np.uint8 and np.array_equal(out[:, sel[0] == 1], dec[:, sel[0] == 1])
    assert np.array_equal(out[1][sel[0] == 0], init[0][sel[0] == 0]) and 0 < sel.sum() < sel.size
    with pytest.raises(ValueError):
        inpaint.composite(dec, init[:, :8], sel)


# ---- the specification and its neighbours ----------------------------------------------------------------------------------
def _outs_err(got, ref):
    return max(R.scaled_err(g, r) for g, r in zip(got, ref))


def test_every_mutant_leaves_the_gpu_tests_tolerance():
    """the tolerance of tests/test_inpaint_gpu.py tells lib/inpaint.py from each of its named neighbours on that test's own
    inputs.  A mutant is the specification itself where it cannot show: the mask ones and zeros are their own channel-major
    reading, and so is a one-cell mask; 'last_step_noised' shows on the last step only, 'stream0' and 'no_keep_noise' on the
    others only; an all-ones mask hides what happens to the kept region, an all-zeros one what happens to pred_x0's blend
    nowhere.  Everywhere else every mutant moves the result by more than a thousand tolerances."""
    from lib.inpaint import MUTANTS
    assert set(MUTANTS) >= {'mask_inverted', 'stream0', 'no_keep_noise', 'level_of_t', 'last_step_noised',
                            'mask_channel_major', 'blend_pred_x0'}
    moved = {w: 0 for w in MUTANTS}
    for c in R.cases():
        ref = R.reference(c)
        h, w = c['shape'][2:]
        for wr in MUTANTS:
            e = _outs_err(R.reference(c, wrong=wr), ref)
            kind, last = c['mask_kind'], c['index'] == 0
            if wr == 'mask_inverted':
                shows = True
            elif wr == 'mask_channel_major':
                shows = kind in ('binary', 'soft') and h * w > 1
            elif wr == 'last_step_noised':
                shows = last and kind != 'ones'
            elif wr in ('blend_pred_x0', 'level_of_t'):     # (the level of t noises the last step's kept region too)
                shows = kind != 'ones'
            else:                      # stream0, no_keep_noise: the kept region's noise
                shows = not last and kind != 'ones'
            if shows:
                assert e > 1e3 * R.TOL, (R.name(c), wr, e)
            else:
                assert e == 0.0, (R.name(c), wr, e)
            moved[wr] += shows
    assert all(moved.values()), moved
    with pytest.raises(ValueError):
        R.reference(c, wrong='something_else')


# ---- the kernels on the CPU emulation --------------------------------------------------------------------------------------
def _build_emu(tmp_path_factory, driver):
    if not os.path.exists(CXX):
        pytest.skip("clang++ of the ROCm toolchain not available")
    out = str(tmp_path_factory.mktemp("pfd_cpu_" + driver))
    subprocess.run([sys.executable, os.path.join(REPO, "tools", "cpu_emu", "build.py"), out], check=True,
                   stdout=subprocess.DEVNULL, env=dict(os.environ, EMU_ONLY=driver, EMU_OPT="-O1"))
    return os.path.join(out, driver)


@pytest.fixture(scope="module")
def emu_inpaint(tmp_path_factory):
    return _build_emu(tmp_path_factory, "emu_inpaint")


@pytest.fixture(scope="module")
def emu_step(tmp_path_factory):
    return _build_emu(tmp_path_factory, "emu_step")


def _emu_step_case(tmp, i, c, offset=0):
    path = os.path.join(tmp, f"step{i}.bin")
    coef = np.zeros(8, dtype=np.float32)
    coef[:c['coef'].size] = c['coef']
    parts = [np.ascontiguousarray(c['keys'], dtype=np.int64), coef]
    if c['scale'] is not None:
        parts.append(c['scale'].astype(np.float32))
    parts += [c['eps'], c['x']] + ([c['x0_prev']] if c['x0_prev'] is not None else []) + [c['x0'], c['mask']]
    with open(path, "wb") as f:
        f.write(b"".join(np.ascontiguousarray(p).tobytes() for p in parts))
    B, C, h, w = c['shape']
    return (f"masked,{B},{c['Bm']},{C},{h},{w},{c['nb']},{c['rep']},{0 if c['solver'] == 'ddim' else 1},"
            f"{int(c['scale'] is not None)},{int(c['x0_prev'] is not None)},0,1,{c['index']},{float(c['noise_mul']).hex()},"
            f"{float(c['ksq']).hex()},{float(c['ks']).hex()},{offset},{path}"), path


def _run_emu(exe, args):
    r = subprocess.run([exe, *args], capture_output=True, text=True, timeout=900)
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith(("ok", "FAIL"))]
    assert r.returncode == 0 and len(lines) == len(args) and all(ln.startswith("ok") for ln in lines), \
        r.stdout[-3000:] + r.stderr[-1000:]
    return lines


def test_step_kernel_on_the_emulation_matches_the_specification(emu_step, tmp_path):
    """csrc/step.hip compiled for the host, through pfd_cfg_step_masked: every shared case (all shapes but the one past the grid, which the GPU test
    covers: a million emulated quads are minutes of host threads), both solvers, plus the scalar path forced by misaligned
    tensors -- return code, one launch, guard bands, the instantiation, and x_out / pred_x0 / xin_next against
    lib/inpaint.py at the GPU test's tolerance (xin_next beyond the half ulp of its own f16 rounding, inpaint_refs.xin_err);
    xin_next is half(x_out) at the NHWC positions in every copy, bit for bit"""
    cases = [(c, 0) for c in R.cases()]
    cases += [(R.case(f, R.SHAPES[0], 2, 'soft'), 1) for f in ('ddim_seeded', 'dpm2')]          # misaligned: scalar accesses
    args, paths = zip(*[_emu_step_case(str(tmp_path), i, c, off) for i, (c, off) in enumerate(cases)])
    lines = _run_emu(emu_step, args)
    seen = set()
    for (c, off), path, line in zip(cases, paths, lines):
        B, C, h, w = c['shape']
        vec = off == 0 and w % 4 == 0
        inst = f"cfg_step_kernel<{0 if c['solver'] == 'ddim' else 1}, true, true, {'true' if vec else 'false'}>"
        assert inst in line, (inst, line)
        seen.add(inst)
        ref = R.reference(c)
        xout = np.fromfile(path + ".xout", dtype=np.float32).reshape(c['shape'])
        pred = np.fromfile(path + ".pred", dtype=np.float32).reshape(c['shape'])
        xin = np.fromfile(path + ".xin", dtype=np.float16).reshape(c['rep'], B, h, w, C)
        e, ex = _outs_err((xout, pred), ref[:2]), R.xin_err(xin[0], ref[0])
        print(f"[inpaint emu] {R.name(c)} offset={off}: err {e:.2e}, xin_next beyond its rounding {ex:.2e}")
        assert e <= R.TOL and ex <= R.TOL, (line, e, ex)
        for r in range(c['rep']):
            assert np.array_equal(xin[r], np.transpose(xout, (0, 2, 3, 1)).astype(np.float16)), line
        if c['mask_kind'] == 'zeros' and c['index'] == 0:
            assert np.array_equal(xout, c['x0'])
    assert len(seen) == 4, seen      # VEC x {ddim, dpmpp}: every masked instantiation (a per-sample scale is a runtime branch)


def test_mask_and_composite_kernels_on_the_emulation_are_byte_exact(emu_inpaint, tmp_path):
    from lib import inpaint
    args, checks = [], []
    masks = [(R.mask_u8(Hm, Wm, i)[None], g) for i, ((Hm, Wm), g) in enumerate(R.GRIDS)]
    masks += [(m[None], (8, 8)) for m, _ in R.worked_masks()]
    masks.append((np.stack([R.mask_u8(100, 80, s) for s in range(3)]), (64, 64)))
    i = 0
    for m, (gh, gw) in masks:
        for f32 in (1, 0):
            path = str(tmp_path / f"grid{i}.bin")
            i += 1
            m.tofile(path)
            args.append(f"grid,{m.shape[0]},{m.shape[1]},{m.shape[2]},{gh},{gw},{f32},{path}")
            checks.append((path, inpaint.mask_grid_batch(m, gh, gw, np.float32 if f32 else np.uint8)))
    dec = np.stack([I.picture_u8(24, 40, s) for s in range(3)])
    for Bi, Bs in ((1, 1), (3, 1), (1, 3), (3, 3)):
        init = np.stack([I.picture_u8(24, 40, 7 + s) for s in range(Bi)])
        sel = np.stack([(R.mask_u8(24, 40, s) >= 128).astype(np.uint8) for s in range(Bs)])
        path = str(tmp_path / f"comp{Bi}{Bs}.bin")
        with open(path, "wb") as f:
            f.write(dec.tobytes() + init.tobytes() + sel.tobytes())
        args.append(f"comp,3,{Bi},{Bs},24,40,3,{path}")
        checks.append((path, inpaint.composite(dec, init, sel)))
    _run_emu(emu_inpaint, args)
    for path, want in checks:
        got = np.fromfile(path + ".out", dtype=want.dtype).reshape(want.shape)
        assert np.array_equal(got, want), path
    for (m, want), (path, got) in zip(R.worked_masks(), checks[2 * len(R.GRIDS)::2]):
        assert np.array_equal(got[0], want)


# ---- the C ABI --------------------------------------------------------------------------------------------------------
def test_header_declares_and_binding_lists_the_entry_points():
    from lib.hip import binding
    src = open(os.path.join(REPO, "include", "pfd_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name, nargs in (("pfd_cfg_step_masked", 24), ("pfd_mask_grid_u8", 9), ("pfd_composite_u8", 11)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", code)
        assert m and len(m.group(1).split(",")) == nargs, name
        assert len(binding.SIGNATURES[name][1]) == nargs, name
    for phrase in ("x_out = m * xp + (1 - m) * known", "lib/inpaint.py", "dilates and never erodes"):
        assert phrase in src, phrase
    assert re.search(r"#define\s+PFD_ABI_VERSION\s+10\b", src) and binding.ABI_VERSION == 10     # entry points added only
    mk = open(os.path.join(REPO, "prompt-free-diffusion_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\binpaint\.hip\b", mk, flags=re.M)
    assert re.search(r"^SRCS\s*:=.*\bstep\.hip\b", mk, flags=re.M)
    # the shared per-element functions exist once, in the file of the one step kernel
    csrc = os.path.join(REPO, "prompt-free-diffusion_amd", "csrc")
    for fn in ("guided_eps", "pred_x0_of", "emit_next", "nhwc_index", "struct DdimStep"):
        defs = [f for f in ("elementwise.hip", "inpaint.hip", "step.hip")
                if re.search(r"(float|void|long)\s+" + fn + r"\s*\(|" + re.escape(fn) + r"\s*\{", open(os.path.join(csrc, f)).read())]
        assert defs == ["step.hip"], (fn, defs)


def test_cabi_argument_checks_need_no_gpu():
    """every refusal happens before a launch and leaves a message behind"""
    from lib.hip import binding
    lib = binding.load()
    bufs = [ctypes.create_string_buffer(4096) for _ in range(10)]
    eps, x, hist, key, coef, scale, x0, mask, xo, pr = (ctypes.cast(b, ctypes.c_void_p) for b in bufs)

    def step(eps=eps, nb=2, x=x, solver=0, x0_prev=None, key=key, step=1, coef=coef, scale=None, x0_keep=x0, mask=mask, Bm=1,
             x_out=xo, pred_x0=pr, xin_next=None, rep=1, B=1, C=4, h=2, w=2):
        return lib.pfd_cfg_step_masked(eps, nb, x, solver, x0_prev, key, step, 1.0, coef, scale, x0_keep, mask, Bm, 0.5, 0.5,
                                       x_out, pred_x0, xin_next, rep, B, C, h, w, None)

    for kw in (dict(eps=None), dict(x=None), dict(key=None), dict(coef=None), dict(x0_keep=None), dict(mask=None),
               dict(x_out=None), dict(pred_x0=None), dict(solver=2), dict(solver=-1), dict(step=-1), dict(Bm=2, B=3),
               dict(Bm=0), dict(Bm=3, B=2), dict(x0_keep=xo), dict(x0_keep=pr), dict(solver=1, x0_prev=xo),
               dict(solver=1, x0_prev=pr), dict(solver=0, x0_prev=hist), dict(nb=0), dict(nb=3), dict(B=0), dict(C=0),
               dict(h=-1), dict(w=0), dict(xin_next=eps, rep=0), dict(xin_next=eps, rep=3)):
        assert step(**kw) == binding.PFD_EINVAL, kw
        assert b"pfd_cfg_step_masked" in lib.pfd_last_error(), kw
    assert step(C=1 << 12, h=1 << 12, w=(1 << 10) + 1) == binding.PFD_ESHAPE       # C*h*w > 2^34
    assert b"2^34" in lib.pfd_last_error()

    def grid(mask=mask, Bm=1, Hm=8, Wm=8, out=xo, gh=2, gw=2):
        return lib.pfd_mask_grid_u8(mask, Bm, Hm, Wm, out, 1, gh, gw, None)

    for kw in (dict(mask=None), dict(out=None), dict(Bm=0), dict(Hm=0), dict(Wm=-1), dict(gh=0), dict(gw=0)):
        assert grid(**kw) == binding.PFD_EINVAL and b"pfd_mask_grid_u8" in lib.pfd_last_error(), kw
    assert grid(Hm=8193) == binding.PFD_ESHAPE and grid(gw=8193) == binding.PFD_ESHAPE

    def comp(decoded=eps, init=x, Bi=1, sel=mask, Bs=1, out=xo, n=2, H=4, W=4, C=3):
        return lib.pfd_composite_u8(decoded, init, Bi, sel, Bs, out, n, H, W, C, None)

    for kw in (dict(decoded=None), dict(init=None), dict(sel=None), dict(out=None), dict(n=0), dict(H=0), dict(W=0), dict(C=0),
               dict(Bi=3), dict(Bs=3), dict(Bi=0), dict(out=eps), dict(out=x), dict(out=mask)):
        assert comp(**kw) == binding.PFD_EINVAL and b"pfd_composite_u8" in lib.pfd_last_error(), kw
    assert comp(H=8193) == binding.PFD_ESHAPE and comp(C=5) == binding.PFD_ESHAPE


def test_ops_wrappers_refuse_before_they_touch_a_device():
    from lib.hip import ops
    c = R.case('ddim', R.SHAPES[0])
    t = {k: (torch.from_numpy(np.ascontiguousarray(v)) if isinstance(v, np.ndarray) else v) for k, v in c.items()}
    good = dict(solver='ddim', keep_key=t['keys'], step=1, x0_keep=t['x0'], mask=t['mask'], ksq=0.9, ks=0.4)

    def call(coef=t['coef'], x=t['x'], **kw):
        return ops.cfg_step_masked(t['eps'], 2, x, coef, **dict(good, **kw))

    for kw, match in ((dict(solver='euler'), "solver"), (dict(mask=None), "required"), (dict(ksq=None), "required"),
                      (dict(keep_key=None), "required"), (dict(step=-1), "step"), (dict(step=1.5), "step"),
                      (dict(coef=torch.zeros(8)), "coef"), (dict(solver='dpmpp'), "coef"), (dict(x0_prev=t['x']), "x0_prev"),
                      (dict(x0_keep=t['x0'][:1]), "x0_keep"), (dict(x0_keep=t['x0'].double()), "x0_keep"),
                      (dict(mask=t['mask'].double()), "mask"), (dict(mask=t['mask'][:, :4]), "mask"),
                      (dict(mask=torch.zeros(2, 2, 8, 8)), "one channel"), (dict(mask=torch.zeros(3, 8, 8)), "mask"),
                      (dict(keep_key=t['keys'][:1]), "keep_key"), (dict(keep_key=t['keys'].int()), "keep_key"),
                      (dict(x=t['x'].double()), "float32"), (dict(ksq=float('nan')), "finite"), (dict(ks=float('inf')), "finite"),
                      (dict(rep=3), "rep")):
        with pytest.raises(ValueError, match=match):
            call(**kw)
    # eps is checked too: a wrong-sized one would be read out of bounds
    for eps in (t['eps'].float(), t['eps'][:3], t['eps'][:, :4], t['eps'].permute(0, 2, 1, 3), None):
        with pytest.raises(ValueError, match="eps"):
            ops.cfg_step_masked(eps, 2, t['x'], t['coef'], **good)
    with pytest.raises(ValueError, match="nb"):
        ops.cfg_step_masked(t['eps'], 3, t['x'], t['coef'], **good)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        call()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        call(mask=t['mask'][:, None])                                  # [1, 1, h, w] is a legal mask
    m = torch.zeros(16, 16, dtype=torch.uint8)
    for a, kw in (((m.float(), 2, 2), {}), ((m, 0, 2), {}), ((m, 2, 9000), {}), ((m, 2, 2), dict(dtype=torch.float16)),
                  ((m[None, None], 2, 2), {})):
        with pytest.raises(ValueError, match="mask_grid_u8"):
            ops.mask_grid_u8(*a, **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.mask_grid_u8(m, 2, 2)
    dec, ini, sel = torch.zeros(2, 8, 8, 3, dtype=torch.uint8), torch.zeros(1, 8, 8, 3, dtype=torch.uint8), torch.zeros(1, 8, 8, dtype=torch.uint8)
    for a in ((dec.float(), ini, sel), (dec, ini[:, :4], sel), (dec, ini, sel[:, :4]), (dec, ini.repeat(3, 1, 1, 1), sel),
              (dec, ini, sel[0]), (dec, ini, sel.repeat(3, 1, 1))):
        with pytest.raises(ValueError, match="composite_u8"):
            ops.composite_u8(*a)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.composite_u8(dec, ini, sel)


# ---- the sampler's masked loop over the stand-in ---------------------------------------------------------------------------
def _standin_step_masked(eps, nb, x, coef, *, solver='ddim', x0_prev=None, keep_key=None, step=None, x0_keep=None, mask=None,
                         ksq=None, ks=None, noise_mul=1.0, scale=None, want_next=True, rep=None):
    """ops.cfg_step_masked on the host: lib/inpaint.py, one log line per call"""
    from lib import inpaint
    from lib.hip import ops
    B, C, h, w = x.shape
    rep = nb if rep is None else rep
    mask = ops.mask_rows(mask, B, h, w)
    hist = "None" if x0_prev is None else ("previous pred_x0" if x0_prev is SS._LAST_PRED[0] else "ANOTHER TENSOR")
    SS.LOG.append(f"cfg_step_masked solver={solver} nb={nb} rep={rep} step={step} ksq={float(ksq).hex()} ks={float(ks).hex()} "
                  f"coef={SS._hexrow(coef)} x0_prev={hist} noise_mul={float(noise_mul)!r} scale={scale is not None} "
                  f"mask={tuple(mask.shape)}")
    xo, p0, xin = inpaint.masked_step(eps.numpy(), nb, x.numpy(), coef.numpy(), keep_key.numpy(), step, x0_keep.numpy(),
                                      mask.numpy(), ksq, ks, solver=solver, x0_prev=None if x0_prev is None else x0_prev.numpy(),
                                      noise_mul=noise_mul, scale=None if scale is None else scale.numpy())
    p0 = torch.from_numpy(p0)
    SS._LAST_PRED[0] = p0
    return torch.from_numpy(xo), p0, (torch.from_numpy(xin).repeat(rep, 1, 1, 1) if want_next else None)


def _install(monkeypatch):
    from lib.hip import ops
    SS.install(monkeypatch)
    monkeypatch.setattr(ops, "cfg_step_masked", _standin_step_masked)


def _masked_x_info(case, soft=False, Bm=1):
    x_info, c = SS.build_inputs(case)
    B, C, h, w = SS.SHAPE
    g = torch.Generator().manual_seed(11)
    x_info['x0_keep'] = torch.randn(*SS.SHAPE, generator=g)
    x_info['mask'] = torch.from_numpy(R.mask('soft' if soft else 'binary', tuple(SS.SHAPE), Bm))
    x_info['keep_key'] = torch.from_numpy(I.keys(B))
    return x_info, c


@pytest.mark.parametrize("solver", ["ddim", "dpmpp_2m", "dpmpp_1"])
@pytest.mark.parametrize("k", [None, 3])
def test_with_a_mask_every_step_is_the_masked_op_with_its_constants(solver, k, monkeypatch):
    from lib import inpaint
    from lib.model_zoo.ddim import DDIMSampler
    case = SS._case("masked", start='xt', solver=solver)
    _install(monkeypatch)
    model = SS.StubModel()
    x_info, c = _masked_x_info(case, Bm=2 if solver == 'ddim' else 1)
    if k is not None:
        x_info['xt_steps'] = k
    s = DDIMSampler(model)
    x, inter = s.sample(case['steps'], SS.SHAPE, x_info, c, eta=0., verbose=False, solver=solver)
    n = case['steps'] if k is None else k
    steps = [ln for ln in SS.LOG if ln.startswith("cfg_")]
    assert len(steps) == n and all(ln.startswith("cfg_step_masked") for ln in steps)
    assert len([ln for ln in SS.LOG if ln.startswith("apply_model_nhwc")]) == n
    order = {'ddim': None, 'dpmpp_2m': 2, 'dpmpp_1': 1}[solver]
    for i, ln in enumerate(steps):
        index = n - 1 - i
        ksq, ks = inpaint.step_constants(s.ddim_alphas_prev[index], index)
        assert ksq == np.float32(np.sqrt(s.ddim_alphas_prev[index])) or index == 0
        assert f" step={index} ksq={float(ksq).hex()} ks={float(ks).hex()} " in ln, (i, ln)
        assert f"solver={'ddim' if order is None else 'dpmpp'} " in ln and "rep=1 " in ln and "nb=2 " in ln
        first_order = order != 2 or i == 0 or index == 0
        assert ("x0_prev=None" in ln) == first_order and "ANOTHER TENSOR" not in ln
    assert "ksq=0x1.0000000000000p+0 ks=0x0.0p+0" in steps[-1]                 # the last step: (1, 0) exactly
    # ... so what the mask keeps ends as x0_keep itself, and what it regenerates does not
    keep = (x_info['mask'] == 0)[:, None].expand(-1, 4, -1, -1).expand_as(x)
    want = x_info['x0_keep'].to(x.dtype)
    assert bool(keep.any()) and torch.equal(x[keep], want[keep]) and not torch.equal(x[~keep], want[~keep])
    assert not any(ln.startswith("q_sample") for ln in SS.LOG)


def test_masked_sampler_rules(monkeypatch):
    from lib.model_zoo.ddim import DDIMSampler
    _install(monkeypatch)
    model = SS.StubModel()

    def run(solver='ddim', eta=0., drop=(), entry='sample', **extra):
        case = SS._case("rules", start='xt', solver=solver)
        x_info, c = _masked_x_info(case)
        for name in drop:
            del x_info[name]
        x_info.update(extra)
        del SS.LOG[:]
        s = DDIMSampler(model)
        if entry == 'sample':
            return s.sample(4, SS.SHAPE, x_info, c, eta=eta, verbose=False, solver=solver, temperature=0.75)
        if entry == 'mc':
            return s.sample_multicontext(4, SS.SHAPE, x_info, [dict(c, ratio=1.0)], eta=eta, verbose=False)
        s.make_schedule(4, ddim_eta=eta, verbose=False)
        x_info['x'] = x_info['xt']
        t = torch.full((SS.SHAPE[0],), 501, dtype=torch.long)
        if entry == 'p':
            return s.p_sample_ddim(x_info, c, t, 2)
        return s.p_sample_ddim_multicontext(x_info, [dict(c, ratio=1.0)], t, 2)

    # all three or none
    for drop in (('mask',), ('x0_keep',), ('keep_key',), ('mask', 'x0_keep')):
        with pytest.raises(ValueError, match="all three or none"):
            run(drop=drop)
    # a keep_key is no noise_key: the multistep solvers run; a noise_key still makes them refuse
    run(solver='dpmpp_2m')
    with pytest.raises(ValueError, match="noise_key"):
        run(solver='dpmpp_2m', noise_key=torch.from_numpy(I.keys(2)))
    # eta > 0 draws nothing from the global generator: it needs the key, equal to keep_key
    with pytest.raises(ValueError, match="noise_key"):
        run(eta=1.)
    with pytest.raises(ValueError, match="equal"):
        run(eta=1., noise_key=torch.from_numpy(I.keys(2)) + 1)
    before = torch.get_rng_state().clone()
    run(eta=1., noise_key=torch.from_numpy(I.keys(2)))
    assert torch.equal(torch.get_rng_state(), before)
    assert all("noise_mul=0.75" in ln for ln in SS.LOG if ln.startswith("cfg_")) and \
        len([ln for ln in SS.LOG if ln.startswith("cfg_step_masked")]) == 4
    # per-sample scale, a [B, 1, h, w] mask and a mask per sample are all allowed
    case = SS._case("ps", start='xt', scale=[1.0, 3.5])
    x_info, c = _masked_x_info(case, soft=True, Bm=2)
    x_info['mask'] = x_info['mask'][:, None]
    del SS.LOG[:]
    DDIMSampler(model).sample(4, SS.SHAPE, x_info, c, eta=0., verbose=False)
    assert all("scale=True" in ln and "mask=(2, 3, 5)" in ln for ln in SS.LOG if ln.startswith("cfg_"))
    # bad shapes are refused
    for bad in (dict(mask=torch.zeros(1, 3, 4)), dict(mask=torch.zeros(3, 3, 5)), dict(x0_keep=torch.zeros(2, 4, 3, 4)),
                dict(keep_key=torch.zeros(3, 2, dtype=torch.int64)), dict(mask=torch.zeros(1, 3, 5, dtype=torch.float64))):
        with pytest.raises(ValueError):
            run(**bad)
    # the entry points without a masked form say so
    for entry in ('mc', 'p', 'pmc'):
        with pytest.raises(ValueError, match="no masked form"):
            run(entry=entry)


@pytest.mark.parametrize("cid", ["eta0", "eta1_noise_key", "per_sample_scale", "dpmpp_2m", "xt_start", "control",
                                 "multicontext_scale_2_eta0", "p_sample_ddim_no_noise"])
def test_without_a_mask_the_call_log_is_the_pinned_one(cid, monkeypatch):
    """tests/golden/sampler_host_calls.txt line for line (tests/test_sampler_host_cpu.py pins every case; these are the
    paths the masked loop was added next to), with the masked stand-in installed and never called"""
    from lib.hip import ops
    case = SS.CASES[SS.CASE_IDS.index(cid)]
    lines, _ = SS.run_case(case, monkeypatch)
    monkeypatch.setattr(ops, "cfg_step_masked", lambda *a, **k: pytest.fail("the masked op was called without a mask"))
    again, _ = SS.run_case(case, monkeypatch)
    assert lines == again == SS.read_fixture()[cid]


# ---- pipeline and server over the stubs --------------------------------------------------------------------------------
def _standin_mask_grid_u8(mask, gh, gw, dtype=torch.float32):
    from lib import inpaint
    m = mask[None] if mask.dim() == 2 else mask
    return torch.from_numpy(inpaint.mask_grid_batch(m.numpy(), gh, gw, np.float32 if dtype == torch.float32 else np.uint8))


def _patch_ops(monkeypatch):
    import test_img2img_cpu as TI
    from lib.hip import ops
    monkeypatch.setattr(ops, "latent_start", TI._standin_latent_start)
    monkeypatch.setattr(ops, "mask_grid_u8", _standin_mask_grid_u8)
    return TI


def _mask_u8(seed=0):
    m = np.zeros((96, 72), dtype=np.uint8)
    m[24 + 12 * seed:72, 18:54] = 255
    return m


def test_masked_generate_is_keyed_per_global_sample_whatever_the_world_size(monkeypatch):
    from lib import inpaint, pipeline
    TI = _patch_ops(monkeypatch)
    img, init = torch.rand(1, 3, 64, 64), TI._picture()
    n_global, seed = 4, (1 << 35) + 9

    def run(rank, world, **kw):
        s = TI._Sampler()
        pipeline.PromptFreePipeline(TI._net(), rank=rank, world_size=world, sampler=s).generate(
            img, n_global, 64, 64, steps=8, seed=seed, init=init, strength=0.75, decode=False, **kw)
        return s.x_infos[0]

    monkeypatch.setattr(pipeline, "shard_xT", lambda *a, **k: pytest.fail("a masked request draws no x_T"))
    one = run(0, 1, mask=_mask_u8())
    assert one['xt_steps'] == 6 and set(one) == {'type', 'xt', 'xt_steps', 'mask', 'x0_keep', 'keep_key'}
    assert one['keep_key'].tolist() == [[seed, j] for j in range(4)] and tuple(one['x0_keep'].shape) == (4, 4, 8, 8)
    assert one['mask'].dtype == torch.float32 and tuple(one['mask'].shape) == (1, 8, 8)
    assert np.array_equal(one['mask'][0].numpy(), inpaint.mask_grid(_mask_u8(), 8, 8))
    halves = [run(r, 2, mask=_mask_u8()) for r in range(2)]
    for name in ('xt', 'x0_keep', 'keep_key'):
        assert torch.equal(torch.cat([h[name] for h in halves]), one[name]), name
    assert all(torch.equal(h['mask'], one['mask']) for h in halves)
    # x0_keep is the clean latent of the very draw the start was noised from
    plain = run(0, 1)
    assert torch.equal(plain['xt'], one['xt']) and 'mask' not in plain and 'keep_key' not in plain
    # a float mask at latent resolution passes through; eta > 0 rides on the same keys
    soft = torch.from_numpy(R.mask('soft', (4, 4, 8, 8), 1))
    assert torch.equal(run(0, 1, mask=soft[0])['mask'], soft) and torch.equal(run(0, 1, mask=soft[:, None])['mask'], soft)
    noisy = run(0, 1, mask=_mask_u8(), eta=0.5, device_noise=True)
    assert torch.equal(noisy['noise_key'], noisy['keep_key'])
    # a float mask per LOCAL sample: [n, h, w] and [n, 1, h, w] pass through, rank by rank
    per = torch.from_numpy(R.mask('soft', (4, 4, 8, 8), 4))
    assert torch.equal(run(0, 1, mask=per)['mask'], per) and torch.equal(run(0, 1, mask=per[:, None])['mask'], per)
    assert torch.equal(run(1, 2, mask=per[2:])['mask'], per[2:])
    assert torch.equal(pipeline.PromptFreePipeline(TI._net()).mask_grid(per, 64, 64, n=4), per)
    for bad in (dict(n=None), dict(n=3)):          # ... and on its own the method holds the caller to the n it is told
        with pytest.raises(ValueError):
            pipeline.PromptFreePipeline(TI._net()).mask_grid(per, 64, 64, **bad)


def test_generate_validates_the_mask_before_anything_touches_the_device():
    import test_img2img_cpu as TI
    from lib.pipeline import PromptFreePipeline

    class Untouchable:
        device = 'cpu'

        def __getattr__(self, name):
            raise AssertionError(f"the model was touched ({name}) before the arguments were checked")

    pipe = PromptFreePipeline(Untouchable(), sampler=TI._Sampler())
    img, init, u8 = torch.rand(1, 3, 64, 64), TI._picture(), I.picture_u8(100, 80)
    base = dict(init=u8, mask=_mask_u8(), as_uint8=True)
    for kw in (dict(init=None), dict(mask=np.zeros((96, 72), dtype=np.float32)), dict(mask=np.zeros((96, 72, 3), dtype=np.uint8)),
               dict(mask=np.zeros((0, 72), dtype=np.uint8)), dict(mask=np.zeros((64 * 17, 64), dtype=np.uint8)),
               dict(mask=torch.zeros(16, 16)), dict(mask=torch.zeros(3, 8, 8)), dict(mask=torch.zeros(1, 2, 8, 8)),
               dict(mask=torch.zeros(4, 8, 8)), dict(mask=torch.zeros(3, 1, 8, 8)),        # n_local is 2: neither 3 nor 4 masks
               dict(mask=torch.zeros(8, 8, dtype=torch.int32)), dict(eta=0.5), dict(composite=True, as_uint8=False),
               dict(composite=True, init=init), dict(composite=True, mask=torch.zeros(8, 8)), dict(composite=True, mask=None),
               dict(composite=True, decode=False)):
        with pytest.raises(ValueError):
            pipe.generate(img, 2, 64, 64, steps=8, **dict(base, **kw))


def test_batch_keys_with_and_without_a_mask():
    import test_img2img_cpu as TI
    from lib import serving
    img = torch.rand(1, 3, 64, 64)
    kw = dict(image=img, n=1, height=64, width=64, steps=8, scale=2.0, eta=0.0, seed=1)
    plain = serving._Request(**kw)
    assert plain.key() == (64, 64, 8, 2.0, 0.0, True, True, False, False)                     # what it was
    i2i = serving._Request(init=TI._picture(0), strength=0.75, init_k=6, **kw)
    assert i2i.key() == plain.key() + (('init', 6),)                                          # what it was
    a = serving._Request(init=TI._picture(0), init_k=6, mask=_mask_u8(), composite=False, **kw)
    b = serving._Request(init=TI._picture(1), init_k=6, mask=_mask_u8(1), composite=False, **dict(kw, seed=2))
    c = serving._Request(init=TI._picture(0), init_k=6, mask=_mask_u8(), composite=True, **kw)
    d = serving._Request(init=TI._picture(0), init_k=4, mask=_mask_u8(), composite=False, **kw)
    assert a.key() == i2i.key() + (('mask', False),) == b.key() and c.key() == i2i.key() + (('mask', True),)
    assert d.key() != a.key() and a.key() != i2i.key() and a.shareable()
    assert serving._Request(init=TI._picture(0), init_k=6, mask=_mask_u8(), solver='dpmpp_2m', **kw).key() == \
        plain.key() + ('dpmpp_2m', ('init', 6), ('mask', False))


def test_server_coalesces_masked_requests_among_themselves_only(monkeypatch):
    import test_img2img_cpu as TI
    srv, calls = TI._stub_server(monkeypatch)
    img = torch.rand(1, 3, 64, 64)
    i2i = dict(steps=8, strength=0.75)
    try:
        outs = TI._queued(srv, [((img, 1, 64, 64), dict(seed=1, init=TI._picture(0), mask=_mask_u8(), **i2i)),
                                ((img, 1, 64, 64), dict(seed=2, init=TI._picture(1), mask=_mask_u8(1), **i2i)),
                                ((img, 1, 64, 64), dict(seed=3, init=TI._picture(0), **i2i)),
                                ((img, 1, 64, 64), dict(seed=4, init=TI._picture(0), **i2i)),
                                ((img, 1, 64, 64), dict(seed=5, init=TI._picture(0), mask=_mask_u8(), steps=8, strength=0.5)),
                                ((img, 1, 64, 64), dict(seed=6, init=I.picture_u8(64, 64), mask=_mask_u8(), composite=True, **i2i)),
                                ((img, 1, 64, 64), dict(seed=7, init=I.picture_u8(64, 64), mask=_mask_u8(), **i2i))])
        assert [float(o[0, 0]) for o in outs] == [1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0]
        assert calls == [[1, 2], [3, 4], [5], [6], [7]]
    finally:
        srv.close()


def test_submit_checks_the_mask_on_the_callers_thread(monkeypatch):
    import test_img2img_cpu as TI
    srv, calls = TI._stub_server(monkeypatch)
    img = torch.rand(1, 3, 64, 64)
    try:
        base = dict(init=I.picture_u8(100, 80), strength=0.75, mask=_mask_u8())
        for kw in (dict(init=None), dict(mask=np.zeros((96, 72), dtype=np.int32)), dict(mask=np.zeros((96, 72, 2), dtype=np.uint8)),
                   dict(mask=torch.zeros(4, 4)), dict(mask=torch.zeros(2, 8, 8)), dict(mask=np.zeros((64 * 17, 64), dtype=np.uint8)),
                   dict(eta=0.5), dict(composite=True, as_uint8=False), dict(composite=True, init=TI._picture()),
                   dict(composite=True, mask=torch.zeros(8, 8)), dict(composite=True, mask=None)):
            with pytest.raises(ValueError):
                srv.submit(img, 1, 64, 64, steps=8, **dict(base, **kw))
        r = srv.submit(img, 1, 64, 64, steps=8, seed=9, eta=0.5, device_noise=True, composite=True, **base).result(30)
        assert float(r[0, 0]) == 9.0 and calls == [[9]]
    finally:
        srv.close()


def test_server_generate_gives_each_masked_request_its_own_picture_mask_and_keys(monkeypatch):
    """the real `_generate` over the stubs: a coalesced masked batch hands the sampler, row for row, what each request's
    solo run hands it -- masks stacked to [B, h, w]"""
    from lib import serving
    TI = _patch_ops(monkeypatch)
    s = TI._Sampler()
    srv = serving.PromptFreeServer(TI._net(), use_graph=False, max_batch=8)
    try:
        srv.pipe.sampler = s
        img = torch.rand(1, 3, 64, 64)
        kw = dict(image=img, height=64, width=64, steps=8, scale=2.0, eta=0.0, as_uint8=False, future=None, strength=0.75,
                  init_k=6, composite=False)
        reqs = [serving._Request(n=2, seed=-5, init=TI._picture(0), mask=_mask_u8(0), **kw),
                serving._Request(n=1, seed=1 << 40, init=TI._picture(1), mask=_mask_u8(1), **kw)]
        before = torch.get_rng_state().clone()
        outs = srv._generate(reqs)
        assert torch.equal(torch.get_rng_state(), before) and [o.shape[0] for o in outs] == [2, 1]
        both = s.x_infos[-1]
        assert both['xt_steps'] == 6 and tuple(both['mask'].shape) == (3, 8, 8) and tuple(both['x0_keep'].shape) == (3, 4, 8, 8)
        assert both['keep_key'].tolist() == [[-5, 0], [-5, 1], [1 << 40, 0]] and 'noise_key' not in both
        solo = [srv._generate([r]) and s.x_infos[-1] for r in reqs]
        for name in ('xt', 'x0_keep', 'mask', 'keep_key'):
            assert torch.equal(both[name], torch.cat([x[name] for x in solo])), name
        assert not torch.equal(both['mask'][0], both['mask'][2]) and torch.equal(both['mask'][0], both['mask'][1])
        for r, x in zip(reqs, solo):       # ... which is the pipeline's own start and mask for (picture, mask, (seed, j))
            keys = torch.tensor([[r.seed, j] for j in range(r.n)])
            x_t, k, x0 = srv.pipe.init_latent(r.init, 64, 64, 8, 0.75, keys, want_x0=True)
            assert k == 6 and torch.equal(x['xt'], x_t) and torch.equal(x['x0_keep'], x0)
            assert torch.equal(x['mask'], srv.pipe.mask_grid(r.mask, 64, 64).expand(r.n, -1, -1))
        # an unmasked img2img request next to them is handed nothing of this
        srv._generate([serving._Request(n=1, seed=3, init=TI._picture(0), **dict(kw, composite=None))])
        assert set(s.x_infos[-1]) == {'type', 'xt', 'xt_steps'}
    finally:
        srv.close()
