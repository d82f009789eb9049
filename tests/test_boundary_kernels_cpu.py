"""CPU: the boundary kernels of csrc/elementwise.hip before a device sees them -- the oracles of tests/boundary_refs.py qualify
themselves (fp32 and fp64 evaluation agree on every fp16 input, every mutant separates, the activation formulas of
csrc/pfd_common.h alone stay inside the bounds), then the library's own entry points run on the CPU emulation
(tools/cpu_emu/emu_elementwise.cpp) on every fp16 input, in place, and with bad arguments, and the wrappers of lib/hip/ops.py
refuse bad operands before they touch the library.  The figures printed here are in profiles/boundary_kernel_tests.md."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import boundary_refs as BR
import kernel_refs as KR

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get("EMU_CXX", "/opt/rocm/lib/llvm/bin/clang++")


# ---- the oracles qualify themselves ------------------------------------------------------------------------------------------
def test_all_f16_is_every_pattern_of_its_kind():
    x, fin, nan = BR.all_f16("non_nan"), BR.all_f16("finite"), BR.all_f16("nan")
    assert (x.numel(), fin.numel(), nan.numel()) == (63490, 63488, 2046) and x.numel() + nan.numel() == 65536
    assert not bool(torch.isnan(x).any()) and bool(torch.isfinite(fin).all()) and bool(torch.isnan(nan).all())
    b = BR.bits_of(x)
    assert bool((b[1:] > b[:-1]).all())                                         # bit order, no pattern twice
    for pattern in (0x0000, 0x8000, 0x0001, 0x83FF, 0x7BFF, 0xFBFF, 0x7C00, 0xFC00):     # +-0, subnormals, +-65504, +-inf
        assert int((b == pattern).sum()) == 1
    assert int(torch.isinf(x).sum()) == 2 and float(fin.max()) == 65504.0 and float(fin.min()) == -65504.0


@pytest.mark.parametrize("f16_image", [True, False], ids=["f16", "f32"])
@pytest.mark.parametrize("mul,add", BR.IMAGE_MUL_ADD)
def test_image_oracle_in_fp32_and_fp64_gives_the_same_bytes(mul, add, f16_image):
    x = BR.all_f16("non_nan")
    r64, r32 = BR.image_u8_ref(x, mul, add, f16_image), BR.image_u8_ref(x, mul, add, f16_image, dtype=torch.float32)
    assert r64.dtype == torch.uint8 and r64.shape == x.shape
    diff = int((r64 != r32).sum())
    print(f"[boundary cpu] image_u8_ref ({mul}, {add}) {'f16' if f16_image else 'f32'} image: fp32 vs fp64 {diff} differences, "
          f"{len(set(r64.tolist()))} byte values occur")
    assert diff == 0
    assert len(set(r64.tolist())) == 256


def test_every_image_mutant_separates():
    assert set(BR.IMAGE_U8_MUTANTS) == {"no_f16_rounding", "product_not_rounded", "flag_swapped", "round_to_nearest"}
    x = BR.all_f16("non_nan")
    for name, (fn, applies) in BR.IMAGE_U8_MUTANTS.items():
        for f16_image in applies:
            n = int((fn(x, 0.5, 0.5, f16_image) != BR.image_u8_ref(x, 0.5, 0.5, f16_image)).sum())
            print(f"[boundary cpu] image mutant {name} on an {'f16' if f16_image else 'f32'} image: {n} inputs differ")
            assert n >= 100, (name, f16_image, n)


def test_every_activation_mutant_violates_its_bound():
    assert set(BR.ACT_MUTANTS) == {"gelu_tanh", "silu_1702"}
    x = BR.all_f16("finite")
    for name, (act, fn) in BR.ACT_MUTANTS.items():
        bad, _ = BR.act_violations(fn(x).half(), x, act)
        print(f"[boundary cpu] activation mutant {name} against the {BR.ACT_NAMES[act]} bound: {int(bad.sum())} inputs outside")
        assert int(bad.sum()) >= 100, (name, int(bad.sum()))
    # the zero-bound activations: a sign flipped, a zero for a value, -0 for a negative input
    for act, wrong in ((BR.ACT_NONE, lambda v: v.abs()), (BR.ACT_RELU, lambda v: torch.relu(v) * 0), (BR.ACT_RELU, lambda v: v * (v > 0))):
        assert int(BR.act_violations(wrong(x), x, act)[0].sum()) >= 100
    # ... and what the bound allows: the exact results, either zero for relu(-0)
    for act in range(4):
        right = KR.activation_ref(x, act).half()
        assert int(BR.act_violations(right, x, act)[0].sum()) == 0, act
    neg0 = torch.relu(x).clone()
    neg0[BR.bits_of(x) == 0x8000] = -0.0
    assert int(BR.act_violations(neg0, x, BR.ACT_RELU)[0].sum()) == 0


def test_half_ulp():
    v = torch.tensor([0.0, 2.0 ** -24, 2.0 ** -14 - 2.0 ** -24, 2.0 ** -14, 1.0 - 2.0 ** -11, 1.0, 1.5, 2.0, 65504.0, -3.0], dtype=torch.float64)
    want = [2.0 ** -25] * 4 + [2.0 ** -12, 2.0 ** -11, 2.0 ** -11, 2.0 ** -10, 2.0 ** 4, 2.0 ** -10]
    assert BR.half_ulp_f16(v).tolist() == want


def test_the_formulas_alone_meet_the_bounds():
    """pfd_gelu / pfd_silu as written, in float32 with a correctly rounded reciprocal and exp2, rounded to fp16 once: inside
    act_bound on all 63 488 finite inputs.  The fp32 error of the GELU form is the margin under 5e-7 the hardware's 1-ulp
    rcp / exp2 have to fit into."""
    x = BR.all_f16("finite")
    for act, form in ((BR.ACT_GELU, BR.gelu_form32), (BR.ACT_SILU, BR.silu_form32)):
        y32 = torch.from_numpy(form(x))
        ref = KR.activation_ref(x, act)
        e32 = (y32.double() - ref).abs()
        rel = e32 / ref.abs().clamp_min(2.0 ** -24)
        at = int(e32.argmax())
        bad, ratio = BR.act_violations(y32.half(), x, act)
        print(f"[boundary cpu] {BR.ACT_NAMES[act]} form in fp32: worst |fp32 - fp64| {float(e32.max()):.3e} at x = {float(x[at]):.4g}, "
              f"worst relative {float(rel.max()):.3e}; rounded to fp16: worst error / bound {float(ratio.max()):.3f}, "
              f"{int(bad.sum())} outside")
        assert int(bad.sum()) == 0
        if act == BR.ACT_GELU:
            assert float(e32.max()) < 5e-7                    # the claim of csrc/pfd_common.h, for the formula alone


# ---- the kernels on the CPU emulation ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    if not os.path.exists(CXX):
        pytest.skip("clang++ of the ROCm toolchain not available")
    out = str(tmp_path_factory.mktemp("pfd_cpu_emu_elementwise"))
    subprocess.run([sys.executable, os.path.join(REPO, "tools", "cpu_emu", "build.py"), out], check=True,
                   stdout=subprocess.DEVNULL, env=dict(os.environ, EMU_ONLY="emu_elementwise", EMU_OPT="-O1"))
    return os.path.join(out, "emu_elementwise")


class _Cases:
    """the cases of one run of the driver: add() writes the input file and returns the index; run() -> outputs as bytes"""

    def __init__(self, tmp_path):
        self.dir, self.args, self.paths = tmp_path, [], []

    def add(self, op, p0, p1=0, p2=0, *, inputs, alias=0, offin=0, offout=0, null=0, rc=0):
        path = str(self.dir / f"case{len(self.args)}.bin")
        with open(path, "wb") as f:
            for t in inputs:
                f.write(t.contiguous().numpy().tobytes())
        self.args.append(f"{op},{p0},{p1},{p2},{alias},{offin},{offout},{null},{rc},{path}")
        self.paths.append(path)
        return len(self.args) - 1

    def run(self, exe):
        r = subprocess.run([exe, *self.args], capture_output=True, text=True, timeout=900)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith(("ok", "FAIL"))]
        assert r.returncode == 0 and len(lines) == len(self.args) and all(ln.startswith("ok") for ln in lines), \
            "\n".join(ln for ln in lines if not ln.startswith("ok"))[-3000:] + r.stdout[-1000:] + r.stderr[-1000:]
        self.lines = lines
        return [np.fromfile(p + ".out", dtype=np.uint8) for p in self.paths]


def _f16(raw):
    return torch.from_numpy(raw.view(np.float16).copy())


def test_image_u8_on_the_emulation_on_every_input(emu, tmp_path):
    """all 63 490 non-NaN inputs (tail of 2), 63 487 of them (tail of 7), and 1, 7, 8, 9 values, both image types: the bytes
    of the oracle, guard bands intact (the driver), one launch each"""
    x = BR.all_f16("non_nan")
    c, want = _Cases(tmp_path), []
    for f16_image in (True, False):
        for k, (mul, add) in enumerate(BR.IMAGE_MUL_ADD):
            for xs in [x, x[3:]] + ([BR.image_u8_operand(n) for n in (1, 7, 8, 9)] if k == 0 else []):
                c.add("image", xs.numel(), int(f16_image), k, inputs=[xs])
                want.append((xs.numel(), f16_image, mul, add, BR.image_u8_ref(xs, mul, add, f16_image)))
    outs = c.run(emu)
    assert all("image_u8_kernel" in ln for ln in c.lines)
    assert {w[0] for w in want} == {63490, 63487, 1, 7, 8, 9}
    for got, (n, f16_image, mul, add, ref) in zip(outs, want):
        diff = int((torch.from_numpy(got) != ref).sum())
        assert got.size == n and diff == 0, (n, f16_image, mul, add, diff)


def test_activations_on_the_emulation_on_every_finite_input(emu, tmp_path):
    """the four activations on all 63 488 finite inputs and on 63 487 of them (a tail of 7), out of place and with y = x:
    inside act_bound, and the in-place launch gives the bits of the other"""
    x = BR.all_f16("finite")
    c, idx = _Cases(tmp_path), {}
    for act in range(4):
        for xs, tag in ((x, "all"), (x[1:], "tail")):
            for alias in (0, 1):
                idx[act, tag, alias] = c.add("act", xs.numel(), act, inputs=[xs], alias=alias)
    outs = c.run(emu)
    assert all("act_kernel" in ln for ln in c.lines)
    for act in range(4):
        for xs, tag in ((x, "all"), (x[1:], "tail")):
            y = _f16(outs[idx[act, tag, 0]])
            bad, ratio = BR.act_violations(y, xs, act)
            worst = "" if ratio is None else f", worst error / bound {float(ratio.max()):.3f} at x = {float(xs[int(ratio.argmax())]):.4g}"
            print(f"[boundary emu] act {BR.ACT_NAMES[act]} ({tag}): {int(bad.sum())} of {xs.numel()} outside the bound{worst}")
            assert int(bad.sum()) == 0, (act, tag, xs[bad][:8].tolist(), y[bad][:8].tolist())
            assert np.array_equal(outs[idx[act, tag, 1]], outs[idx[act, tag, 0]]), (act, tag, "in place")


def test_adds_on_the_emulation_in_place_give_the_bits_of_the_out_of_place_call(emu, tmp_path):
    """pfd_add_f16 (y = a, y = b, and the copy with b = NULL onto a), pfd_axpby_f16 (the same), pfd_add_rowvec_f16 and its
    statistics form (y = x) on (5, 160) and (3, 320) and, for the flat kernels, on a size with a tail: the out-of-place
    result is the fp32 formula rounded once, every aliasing include/pfd_hip.h allows gives the same bits"""
    c, idx, data = _Cases(tmp_path), {}, {}
    for R, C in BR.ROW_SHAPES:
        x, b, v = BR.row_operands(R, C, 0)
        data[R, C] = (x, b, v)
        for n in (R * C, R * C - 3):
            a_, b_ = x.reshape(-1)[:n], b.reshape(-1)[:n]
            for op in ("add", "axpby"):
                for alias in (0, 1, 2):
                    idx[op, n, alias, 0] = c.add(op, n, inputs=[a_, b_], alias=alias)
                for alias in (0, 1):
                    idx[op, n, alias, 3] = c.add(op, n, inputs=[a_, b_], alias=alias, null=3)
        for op in ("rowvec", "rowstat"):
            for alias in (0, 1):
                idx[op, R, C, alias] = c.add(op, R, C, inputs=[x, v], alias=alias)
    outs = c.run(emu)
    f32 = lambda t: t.float().numpy()                                              # noqa: E731
    for R, C in BR.ROW_SHAPES:
        x, b, v = data[R, C]
        for n in (R * C, R * C - 3):
            a_, b_ = x.reshape(-1)[:n], b.reshape(-1)[:n]
            want = {("add", 0): (f32(a_) + f32(b_)).astype(np.float16), ("add", 3): a_.numpy(),
                    ("axpby", 0): BR._fma32(np.float32(0.75), f32(a_), np.float32(-1.25) * f32(b_)).astype(np.float16),
                    ("axpby", 3): (np.float32(0.75) * f32(a_)).astype(np.float16)}
            for (op, null), w in want.items():
                base = outs[idx[op, n, 0, null]]
                assert np.array_equal(base.view(np.uint16), w.view(np.uint16)), (op, n, null)
                for alias in ((1, 2) if null == 0 else (1,)):
                    assert np.array_equal(outs[idx[op, n, alias, null]], base), (op, n, null, alias)
        w = (f32(x) + f32(v)[None]).astype(np.float16)
        plain, stat = outs[idx["rowvec", R, C, 0]], outs[idx["rowstat", R, C, 0]]
        assert np.array_equal(plain.view(np.uint16), w.reshape(-1).view(np.uint16))
        assert np.array_equal(stat[:plain.size], plain), "the statistics form stores other bits than the plain one"
        assert np.array_equal(outs[idx["rowvec", R, C, 1]], plain) and np.array_equal(outs[idx["rowstat", R, C, 1]], stat)
        st = stat[plain.size:].view(np.float32).reshape(R, C // 160, 2).astype(np.float64)
        yd = w.astype(np.float64).reshape(R, C // 160, 160)
        assert np.all(np.abs(st[..., 0] - yd.sum(-1)) <= 1e-5 * np.abs(yd).sum(-1))
        assert np.all(np.abs(st[..., 1] - (yd * yd).sum(-1)) <= 1e-5 * (yd * yd).sum(-1))


def test_bad_arguments_on_the_emulation_are_refused_with_nothing_written(emu, tmp_path):
    """a pointer 2 or 8 bytes off its alignment (16 bytes; 8 for the bytes of pfd_image_u8_f16, where 8 off is aligned and 4
    off is not), n = 0, NULL, an activation outside the four, C % 8 for the row-vector add: PFD_EINVAL; C % 160 for its
    statistics form: PFD_ESHAPE, as include/pfd_hip.h has it.  Nothing is launched (the driver), the output keeps its 0xA5"""
    x, b, v = BR.row_operands(5, 160, 1)
    flat, n = x.reshape(-1), 800
    c, E = _Cases(tmp_path), BR.PFD_EINVAL
    none = torch.zeros(0, dtype=torch.float16)
    for op, p1, ins in (("image", 1, [flat]), ("image", 0, [flat]), ("act", 3, [flat]), ("add", 0, [flat, b.reshape(-1)]),
                        ("axpby", 0, [flat, b.reshape(-1)])):
        for kw in (dict(offin=2), dict(offin=8), dict(offout=2), dict(offout=4 if op == "image" else 8), dict(null=1), dict(null=2)):
            c.add(op, n, p1, inputs=ins, rc=E, **kw)
        c.add(op, 0, p1, inputs=[none] * len(ins), rc=E)
    c.add("image", n, 1, inputs=[flat], offout=8)                                 # 8-byte aligned bytes: taken
    c.add("act", n, 4, inputs=[flat], rc=E)
    c.add("act", n, -1, inputs=[flat], rc=E)
    for op in ("rowvec", "rowstat"):
        for kw in (dict(offin=2), dict(offin=8), dict(offout=2), dict(offout=8), dict(null=1), dict(null=2), dict(null=3)):
            c.add(op, 5, 160, inputs=[x, v], rc=E, **kw)
        c.add(op, 0, 160, inputs=[none, v], rc=E)
    c.add("rowvec", 5, 12, inputs=[flat[:60], v[:12]], rc=E)
    c.add("rowvec", 5, 4, inputs=[flat[:20], v[:4]], rc=E)
    c.add("rowstat", 5, 168, inputs=[torch.cat([flat, flat[:40]]), torch.cat([v, v[:8]])], rc=BR.PFD_ESHAPE)
    c.add("rowstat", 5, 8, inputs=[flat[:40], v[:8]], rc=BR.PFD_ESHAPE)
    outs = c.run(emu)
    refused = 0
    for arg, out in zip(c.args, outs):
        if int(arg.split(",")[8]) != 0:
            assert set(out.tolist()) <= {0xA5}, arg
            refused += 1
    assert refused == len(outs) - 1


# ---- the wrappers refuse before they touch the library -----------------------------------------------------------------------
class _OnDevice(torch.Tensor):
    """a CPU tensor that says it is on the device: the checks behind _chk16's device test become reachable without one"""
    is_cuda = property(lambda self: True)


def _dev(*shape, dtype=torch.float16):
    return torch.zeros(shape, dtype=dtype).as_subclass(_OnDevice)


def test_ops_wrappers_check_their_operands_before_the_library(monkeypatch):
    from lib.hip import ops

    def no_library():
        raise AssertionError("the library was reached with a bad operand")
    monkeypatch.setattr(ops, "_lib", no_library)
    cpu = torch.zeros(4, 16, dtype=torch.float16)
    a, wide = _dev(4, 16), _dev(4, 32)
    assert a.is_cuda and wide[:, :16].is_cuda and not wide[:, :16].is_contiguous() and wide[:, :16].stride(-1) == 1
    for call in (lambda: ops.add(cpu, cpu), lambda: ops.axpby(cpu, 1.0), lambda: ops.activation(cpu, 3), lambda: ops.add_rowvec(cpu, cpu[0])):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    # a caller's out: float16, on the device, dense, of the result's size
    for fn in (lambda out: ops.add(a, a, out=out), lambda out: ops.axpby(a, 1.0, a, 1.0, out=out), lambda out: ops.axpby(a, 1.0, out=out),
               lambda out: ops.activation(a, 3, out=out)):
        with pytest.raises(TypeError):
            fn(_dev(4, 16, dtype=torch.float32))
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(cpu)
        with pytest.raises(ValueError):
            fn(wide[:, :16])
        with pytest.raises(ValueError):
            fn(wide[:, ::2])
        with pytest.raises(ValueError):
            fn(_dev(4, 8))
        with pytest.raises(AssertionError, match="the library was reached"):          # a good one passes every check
            fn(a)
    # b of axpby
    with pytest.raises(TypeError):
        ops.axpby(a, 1.0, _dev(4, 16, dtype=torch.float32), 1.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.axpby(a, 1.0, cpu, 1.0)
    with pytest.raises(ValueError):
        ops.axpby(a, 1.0, wide[:, :16], 1.0)
    with pytest.raises(ValueError):
        ops.axpby(a, 1.0, _dev(2, 16), 1.0)
    # v and out of add_rowvec: x and out may be strided matrices, v is a dense vector of C elements
    v = _dev(16)
    with pytest.raises(TypeError):
        ops.add_rowvec(a, _dev(16, dtype=torch.float32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.add_rowvec(a, cpu[0])
    with pytest.raises(ValueError):
        ops.add_rowvec(a, _dev(8))
    with pytest.raises(ValueError):
        ops.add_rowvec(a, _dev(32)[::2])
    with pytest.raises(ValueError):
        ops.add_rowvec(a, _dev(4, 16))
    with pytest.raises(TypeError):
        ops.add_rowvec(a, v, out=_dev(4, 16, dtype=torch.float32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.add_rowvec(a, v, out=cpu)
    with pytest.raises(ValueError):
        ops.add_rowvec(a, v, out=_dev(4, 8))
    with pytest.raises(ValueError):
        ops.add_rowvec(a, v, out=_dev(2, 16))
    with pytest.raises(ValueError):
        ops.add_rowvec(a, v, out=wide[:, ::2])
    for good in (lambda: ops.add_rowvec(a, v, out=wide[:, 16:]), lambda: ops.add_rowvec(wide[:, :16], v, out=wide[:, :16]),
                 lambda: ops.add_rowvec(a, v)):
        with pytest.raises(AssertionError, match="the library was reached"):
            good()
