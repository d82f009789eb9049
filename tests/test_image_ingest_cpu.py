"""uint8 pictures at the front door, what can be checked without a GPU (the GPU half is tests/test_image_ingest_gpu.py):

  (a) lib.image_io.pillow_bicubic_taps, evaluated in numpy with Pillow's 32-bit arithmetic, gives the bytes Pillow wrote into
      tests/golden/image_ingest.npz (tools/make_image_golden.py) on all eleven cases -- and Pillow's own, live, where Pillow
      can be imported;
  (b) csrc/image.hip compiled for the host (tools/cpu_emu/emu_image.cpp) gives the same bytes through the library's entry
      points, and its f32 / f16 outputs are u8 / 255 bit for bit;
  (c) PromptFreeServer.submit and PromptFreePipeline.generate refuse malformed uint8 input with ValueError on the caller's
      thread, before any device work;
  (d) ToTensor alone on all 256 byte values, through the same emulation;
  (e) the new kernels use no scratch;
  and the C ABI refuses what is outside its bounds with nothing launched (argument checks need no device).
Zero differing bytes everywhere: there is no tolerance in this file."""
import ctypes
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(REPO, "tools"), os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import make_image_golden as G  # noqa: E402  (the closed-form inputs and the case list; Pillow is imported by its main() only)
from lib.image_io import pillow_bicubic_taps  # noqa: E402

CXX = os.environ.get("EMU_CXX", "/opt/rocm/lib/llvm/bin/clang++")
EMU_CASES = ("up", "down", "h_same", "w_same", "gray", "clip")


@pytest.fixture(scope="module")
def fixture():
    g = dict(np.load(G.GOLDEN, allow_pickle=False))
    g["meta"] = json.loads(str(g["meta"]))
    return g


def resample_axis1(img, out):
    """one pass over axis 1 of [H, W, C] with the product's tap tables: int32 sums, arithmetic shift, clamp"""
    H, W, C = img.shape
    xmin, klen, kk = pillow_bicubic_taps(W, out)
    o = np.empty((H, out, C), np.uint8)
    im = img.astype(np.int32)
    for xx in range(out):
        k = np.asarray(kk[xx][:klen[xx]], np.int32)
        acc = (1 << 21) + (im[:, xmin[xx]:xmin[xx] + klen[xx], :] * k[None, :, None]).sum(1, dtype=np.int32)
        o[:, xx, :] = np.clip(acc >> 22, 0, 255)
    return o


def numpy_resize(a, oh, ow):
    """horizontal first into a rounded uint8 picture, then vertical; an axis that keeps its size is skipped"""
    t = a
    if t.shape[1] != ow:
        t = resample_axis1(t, ow)
    if t.shape[0] != oh:
        t = resample_axis1(t.transpose(1, 0, 2), oh).transpose(1, 0, 2)
    return np.ascontiguousarray(t)


# ---- (a) ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(G.CASES))
def test_tap_tables_reproduce_pillow_fixture(fixture, name):
    h, w, c, kind, oh, ow, stored = G.CASES[name]
    meta = fixture["meta"]["cases"][name]
    assert meta["input"] == [h, w, c] and meta["output"] == [oh, ow, c] and fixture["meta"]["pillow"]
    got = numpy_resize(G.source(name), oh, ow)
    assert got.shape == (oh, ow, c)
    if stored:
        assert int((got != fixture[name]).sum()) == 0
    assert hashlib.sha256(got.tobytes()).hexdigest() == meta["sha256"]
    if name == "clip":      # the clamp is exercised at both ends
        assert int((got == 0).sum()) > 5000 and int((got == 255).sum()) > 5000


def test_tap_table_shapes():
    """4 taps when enlarging, 64 at the documented bound 1024 -> 64; rows are padded to one pitch; windows stay inside"""
    for (i, o), taps in {(131, 192): 4, (97, 128): 4, (300, 128): 10, (200, 64): 13, (400, 64): 25, (300, 64): 19,
                         (1024, 64): 64}.items():
        xmin, klen, kk = pillow_bicubic_taps(i, o)
        assert len(xmin) == len(klen) == len(kk) == o and max(klen) == taps == len(kk[0])
        assert all(len(r) == taps for r in kk)
        assert all(0 <= a and a + n <= i and n >= 1 for a, n in zip(xmin, klen))
        assert all(abs(sum(r) - (1 << 22)) <= len(r) for r in kk)          # coefficients sum to one, up to rounding
        assert all(v == 0 for r, n in zip(kk, klen) for v in r[n:])
    with pytest.raises(ValueError):
        pillow_bicubic_taps(0, 4)


@pytest.mark.parametrize("name", list(G.CASES))
def test_tap_tables_reproduce_pillow_live(name):
    pytest.importorskip("PIL")
    h, w, c, kind, oh, ow, stored = G.CASES[name]
    a = G.source(name)
    assert int((numpy_resize(a, oh, ow) != G.pillow_resize(a, oh, ow)).sum()) == 0


def test_no_pillow_in_the_library():
    pkg = os.path.join(REPO, "prompt-free-diffusion_amd")
    for root, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(root, f)).read()
                assert "import PIL" not in src and "from PIL" not in src, os.path.join(root, f)


# ---- (b), (d): the kernels on the CPU emulation ---------------------------------------------------------------------
def _write_taps(path, i, o):
    xmin, klen, kk = pillow_bicubic_taps(i, o)
    np.concatenate([np.asarray([len(kk[0])], np.int32), np.asarray(xmin, np.int32), np.asarray(klen, np.int32),
                    np.asarray(kk, np.int32).ravel()]).tofile(path)


@pytest.fixture(scope="module")
def emu_run(tmp_path_factory, fixture):
    """build tools/cpu_emu/emu_image, run it once over the six fixture cases + three of its own; -> {name: outputs}"""
    if not os.path.exists(CXX):
        pytest.skip("clang++ of the ROCm toolchain not available")
    out = str(tmp_path_factory.mktemp("pfd_emu_image"))
    subprocess.run([sys.executable, os.path.join(REPO, "tools", "cpu_emu", "build.py"), out], check=True,
                   stdout=subprocess.DEVNULL, env=dict(os.environ, EMU_ONLY="emu_image"))
    cases = {}
    for name in EMU_CASES:
        h, w, c, kind, oh, ow, stored = G.CASES[name]
        cases[name] = (G.source(name), fixture[name], 0)
    # pointer alignment decides the load width of the vertical pass: the one-channel case once more, one byte off
    cases["gray_off1"] = (cases["gray"][0], cases["gray"][1], 1)
    # (d) all 256 byte values, ToTensor only; and the same with three channels (no pass, 12 bytes per thread)
    ramp = np.arange(256, dtype=np.uint8).reshape(16, 16, 1)
    cases["all256"] = (ramp, ramp, 0)
    cases["identity"] = (G.source("identity"), fixture["identity"], 0)
    with open(os.path.join(out, "cases.txt"), "w") as f:
        for name, (src, exp, off) in cases.items():
            (h, w, c), (oh, ow, _) = src.shape, exp.shape
            f.write(f"{name} {h} {w} {c} {oh} {ow} {off}\n")
            src.tofile(os.path.join(out, name + ".src"))
            np.ascontiguousarray(exp).tofile(os.path.join(out, name + ".exp"))      # the expected bytes, from the fixture
            if w != ow:
                _write_taps(os.path.join(out, name + ".htaps"), w, ow)
            if h != oh:
                _write_taps(os.path.join(out, name + ".vtaps"), h, oh)
    r = subprocess.run([os.path.join(out, "emu_image"), out], capture_output=True, text=True, timeout=600)
    lines = [l for l in r.stdout.splitlines() if l.startswith(("ok", "FAIL"))]
    assert r.returncode == 0 and len(lines) == len(cases) and all(l.startswith("ok") for l in lines), \
        r.stdout[-3000:] + r.stderr[-1000:]
    res = {}
    for name, (src, exp, off) in cases.items():
        oh, ow, c = exp.shape
        rd = lambda ext, dt: np.fromfile(os.path.join(out, name + ext), dtype=dt)      # noqa: E731
        res[name] = dict(exp=exp, u8=rd(".out_u8", np.uint8).reshape(oh, ow, c),
                         f32=rd(".out_f32", np.float32).reshape(c, oh, ow), f16=rd(".out_f16", np.float16).reshape(c, oh, ow),
                         nhwc=rd(".out_nhwc_f16", np.float16).reshape(oh, ow, c),
                         line=[l for l in lines if l.split()[1] == name][0])
    return res


@pytest.mark.parametrize("name", EMU_CASES + ("gray_off1", "identity"))
def test_kernels_on_the_emulation(emu_run, name):
    """uint8 output == Pillow's bytes; f32 / f16 NCHW (and f16 NHWC) == u8 / 255 bitwise, torch's own division and rounding"""
    r = emu_run[name]
    assert int((r["u8"] != r["exp"]).sum()) == 0
    want = torch.from_numpy(np.ascontiguousarray(r["exp"])).permute(2, 0, 1).float().div(255)     # ToTensor
    assert torch.equal(torch.from_numpy(r["f32"]).view(torch.int32), want.contiguous().view(torch.int32))
    assert torch.equal(torch.from_numpy(r["f16"]).view(torch.int16), want.half().contiguous().view(torch.int16))
    assert torch.equal(torch.from_numpy(r["nhwc"]).view(torch.int16),
                       want.half().permute(1, 2, 0).contiguous().view(torch.int16))


def test_emulation_covers_every_kernel_form(emu_run):
    """both passes, three- and one-channel, the 4-pixel and the 1-pixel form of the vertical pass"""
    seen = " ".join(r["line"] for r in emu_run.values())
    for k in ("image_resample_h_kernel<3>", "image_resample_h_kernel<1>", "image_resample_v_kernel<3, 4>",
              "image_resample_v_kernel<3, 1>", "image_resample_v_kernel<1, 4>", "image_resample_v_kernel<1, 1>"):
        assert k in seen, (k, seen)


def test_totensor_all_256_values_on_the_emulation(emu_run):
    r = emu_run["all256"]
    want = torch.arange(256, dtype=torch.uint8).float().div(255)
    assert torch.equal(torch.from_numpy(r["f32"]).reshape(-1).view(torch.int32), want.view(torch.int32))
    assert torch.equal(torch.from_numpy(r["f16"]).reshape(-1).view(torch.int16), want.half().view(torch.int16))
    assert torch.equal(torch.from_numpy(r["u8"]).reshape(-1), torch.arange(256, dtype=torch.uint8))
    # why the kernel divides: the reciprocal multiply is a different function in fp32
    assert int((torch.arange(256).float() * (1 / 255.) != want).sum()) > 100


# ---- (c) ------------------------------------------------------------------------------------------------------------
def _bad_pictures():
    ok = np.zeros((64, 64, 3), np.uint8)
    return {
        "rank 2": np.zeros((64, 64), np.uint8),
        "rank 4 with a batch": np.zeros((2, 64, 64, 3), np.uint8),
        "four channels": np.zeros((64, 64, 4), np.uint8),
        "channels first": torch.zeros(3, 64, 64, dtype=torch.uint8),
        "int16": ok.astype(np.int16),
        "float HWC numpy": ok.astype(np.float32),
        "a list": ok.tolist(),
    }


def test_submit_checks_uint8_pictures_on_the_callers_thread():
    from stubs import StubNet, StubSampler
    from lib.serving import PromptFreeServer
    srv = PromptFreeServer(StubNet(), use_graph=False, max_batch=4)
    srv.pipe.sampler = StubSampler(0)
    ran = []
    srv._generate = lambda batch: ran.append(len(batch)) or [None for _ in batch]
    try:
        good = torch.zeros(40, 50, 3, dtype=torch.uint8)
        for what, bad in _bad_pictures().items():
            with pytest.raises(ValueError):
                srv.submit(bad, 1, 64, 64)
            with pytest.raises(ValueError):
                srv.submit(good, 1, 64, 64, control=bad)
        for small in (torch.zeros(31, 64, 3, dtype=torch.uint8), np.zeros((64, 16, 3), np.uint8)):
            with pytest.raises(ValueError):
                srv.submit(small, 1, 64, 64)                          # a reference picture is at least 32 a side
        with pytest.raises(ValueError):
            srv.submit(good, 1, 64, 64, control=torch.zeros(2000, 64, 3, dtype=torch.uint8))   # shrinks by more than 16
        with pytest.raises(ValueError):
            srv.submit(torch.zeros(1, 3, 64, 64, dtype=torch.int32), 1, 64, 64)   # as before: not a float tensor
        assert ran == []                                               # nothing reached the worker
        # accepted: any size, [h, w, 3] or [1, h, w, 3], torch or numpy; a small control picture is fine (it is enlarged)
        srv.submit(good, 1, 64, 64).result(30)
        srv.submit(good[None].numpy(), 1, 64, 64, control=np.zeros((8, 9, 3), np.uint8)).result(30)
        srv.submit(torch.rand(1, 3, 64, 64), 1, 64, 64, control=torch.zeros(300, 200, 3, dtype=torch.uint8)).result(30)
        assert ran == [1, 1, 1]                                        # a control request runs alone, as before
    finally:
        srv.close()


def test_request_carries_the_bytes_and_the_worker_ingests_them():
    """no CPU fallback: with the stub net on the CPU the worker gets as far as the first kernel and the future carries its
    refusal -- the uint8 picture travelled in the request unchanged"""
    from stubs import StubNet, StubSampler
    from lib.serving import PromptFreeServer
    srv = PromptFreeServer(StubNet(), use_graph=False, max_batch=4)
    srv.pipe.sampler = StubSampler(0)
    try:
        f = srv.submit(torch.zeros(40, 50, 3, dtype=torch.uint8), 1, 64, 64)
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            f.result(30)
        assert srv.pipe.sampler.calls == 0
    finally:
        srv.close()


def test_generate_checks_uint8_pictures_before_any_device_work():
    from stubs import StubNet, StubSampler
    from lib.pipeline import PromptFreePipeline
    net, sampler = StubNet(), StubSampler(0)
    encoded = []
    net.ctx_encode = lambda image, which: encoded.append(1)
    pipe = PromptFreePipeline(net, sampler=sampler)
    good = np.zeros((48, 32, 3), np.uint8)
    for what, bad in _bad_pictures().items():
        if torch.is_tensor(bad) or isinstance(bad, list):
            continue        # (generate leaves torch tensors of other dtypes to the float path, as before)
        with pytest.raises(ValueError):
            pipe.generate(bad, 1, 64, 64, steps=2)
        with pytest.raises(ValueError):
            pipe.generate(good, 1, 64, 64, steps=2, control=bad)
    for bad in (torch.zeros(3, 64, 64, dtype=torch.uint8), torch.zeros(64, 20, 3, dtype=torch.uint8)):
        with pytest.raises(ValueError):
            pipe.generate(bad, 1, 64, 64, steps=2)
    with pytest.raises(ValueError):
        pipe.generate(good, 1, 64, 64, steps=2, control=np.zeros((64, 1100, 3), np.uint8))     # 1100 > 16 * 64
    assert encoded == [] and sampler.calls == 0
    with pytest.raises(RuntimeError, match="no CPU fallback"):      # a good picture reaches the kernel's front door
        pipe.generate(good, 1, 64, 64, steps=2)
    assert encoded == [] and sampler.calls == 0
    # float tensors: exactly as before
    img, lat = PromptFreePipeline(StubNet(), sampler=StubSampler(0)).generate(torch.rand(1, 3, 64, 64), 1, 64, 64, steps=2)
    assert img.shape == (1, 3, 64, 64)


# ---- C ABI bounds (nothing is launched on an error, so no device is needed) -----------------------------------------
def test_cabi_bounds_of_the_resampler():
    from lib.hip import binding
    lib = binding.load()
    assert binding.ABI_VERSION == 10 and lib.pfd_abi_version() == 10
    chk = lib.pfd_image_resample_check
    assert chk(1, 600, 900, 512, 768, 3) == 0 and chk(3, 1024, 1024, 64, 64, 1) == 0 and chk(1, 1, 1, 8192, 8192, 3) == 0
    for bad in ((0, 64, 64, 64, 64, 3), (1, 64, 64, 64, 64, 4), (1, 64, 64, 64, 64, 2), (1, 8193, 64, 64, 64, 3),
                (1, 64, 64, 64, 8193, 3), (1, 1025, 64, 64, 64, 3), (1, 64, 1025, 64, 64, 3), (1, 0, 64, 64, 64, 3),
                (1, 64, 64, 0, 64, 3)):
        assert chk(*bad) == binding.PFD_ESHAPE, bad
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    h, v = lib.pfd_image_resample_h_u8, lib.pfd_image_resample_v_u8
    assert h(None, p, 1, 4, 4, 8, 3, p, p, p, 4, None) == binding.PFD_EINVAL
    assert h(p, p, 1, 4, 4, 8, 3, None, p, p, 4, None) == binding.PFD_EINVAL
    assert h(p, p, 1, 4, 100, 4, 3, p, p, p, 4, None) == binding.PFD_ESHAPE          # 100 > 16 * 4
    assert h(p, p, 1, 4, 4, 8, 2, p, p, p, 4, None) == binding.PFD_ESHAPE            # two channels
    assert h(p, p, 1, 4, 4, 8, 3, p, p, p, 67, None) == binding.PFD_ESHAPE           # more taps than any table has
    assert v(p, None, 1, 1, 4, 4, 4, 3, None, None, None, 0, None) == binding.PFD_EINVAL
    assert v(p, p, 7, 1, 4, 4, 4, 3, None, None, None, 0, None) == binding.PFD_EINVAL          # no such output kind
    assert v(p, p, 1, 1, 4, 8, 4, 3, None, None, None, 0, None) == binding.PFD_ESHAPE          # resize without a table
    assert v(p, p, 1, 1, 200, 4, 4, 3, p, p, p, 4, None) == binding.PFD_ESHAPE
    with pytest.raises(binding.PfdError, match="PFD_ESHAPE"):
        binding.check(chk(1, 64, 64, 64, 64, 4), "pfd_image_resample_check")


# ---- (e) ------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")
def test_image_kernels_use_no_scratch():
    import isa_audit
    bad, rows = isa_audit.findings([os.path.join(REPO, "prompt-free-diffusion_amd", "csrc", "image.hip")])
    kernels = {k: v for _, k, v in rows}
    assert len(kernels) == 6, sorted(kernels)          # h: C = 3 | 1; v: (C, V) in {3, 1} x {4, 1}
    assert all(v["scratch"] == 0 for v in kernels.values()), kernels
    assert not [b for b in bad if "scratch" in b]
