"""Canny edge hints behind ControlNet.preprocess('canny'), what can be checked without a GPU (the GPU half is
tests/test_canny_gpu.py):

  (a) the numpy specification (lib/canny.py) reproduces tests/golden/canny.npz (tools/make_canny_golden.py) on every case, its
      two hysteresis formulations -- a stack flood and a 3x3 dilation within the candidates until nothing changes -- agree, and
      the serpentine pictures have the stated counts (one winding band of 2302 weak pixels behind 15 strong ones: 1148
      sweeps of the dilation; zero edges once the strong stretch is gone);
  (b) csrc/canny.hip compiled for the host (tools/cpu_emu/emu_canny.cpp; the threads of a block run concurrently) gives the
      specification's state bytes and edge bytes through the library's entry point, in every output form;
  (c) the C ABI refuses what is outside its bounds with nothing launched; the symbols exist and the ABI is still 10;
  (d) ControlNet.preprocess over a stand-in of ops.canny_u8: 'none', 'input', canny with kwargs, a refused path, the other
      annotators still raising;
  (e) PromptFreeServer.submit and PromptFreePipeline.generate refuse bad arguments with ValueError before any device work, the
      request carries the two new values, the batch key of a default call is what it was;
  (f) the new kernels use no scratch.
Zero differing bytes everywhere: there is no tolerance in this file.  The expected bytes are the numpy specification's; their
equality with cv2.Canny is unverified (the fixture's meta says so unless the tool ran where cv2 can be imported)."""
import ctypes
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

import make_canny_golden as G  # noqa: E402
from lib import canny as K  # noqa: E402

CXX = os.environ.get("EMU_CXX", "/opt/rocm/lib/llvm/bin/clang++")
META, PICS, CASES = G.load()


# ---- (a) ------------------------------------------------------------------------------------------------------------
def test_fixture_holds_the_cases():
    assert set(CASES) == {c for c, _, _ in G.case_list(PICS)} and "photo" in PICS and len(CASES) >= 30
    assert os.path.getsize(G.GOLDEN) < 200 * 1024
    assert META["cv2"] == "cv2 absent" and META["cv2_verified"].startswith("UNVERIFIED") or \
        all("cv2_differing" in m for m in META["cases"].values())
    shapes = {tuple(PICS[p].shape[:2]) for p in PICS}
    assert {(1, 1), (1, 17), (5, 3), (64, 64), (128, 256), (70, 150), (133, 200), (96, 130), (96, 128)} <= shapes
    assert {tuple(t) for _, t, _, _ in CASES.values()} == {(100, 200), (200, 100), (99.9, 200.5), (0, 0), (0, 2000)}
    for name, pic in G.pictures().items():                       # the closed-form pictures are what the tool draws today
        if not name.startswith("smooth"):                        # (the blurred noise is floating point: its bytes are stored)
            assert np.array_equal(pic, PICS[name]), name
    for name in ("smooth2", "smooth3", "photo", "p64", "p128x256", "p70x150", "p133x200"):
        assert META["cases"][name]["promoted"] > 100, name       # the hysteresis has work to do: not vacuous


@pytest.mark.parametrize("name", list(CASES))
def test_specification_reproduces_the_fixture(name):
    pic, thr, states, edges = CASES[name]
    st = K.canny_states(PICS[pic], *thr)
    assert st.dtype == np.uint8 and st.shape == PICS[pic].shape[:2] and int((st != states).sum()) == 0
    flood = K.hysteresis(st)
    dil, sweeps = K.hysteresis_by_dilation(st)
    assert int((flood != edges).sum()) == 0 and int((dil != flood).sum()) == 0
    assert np.array_equal(K.canny(PICS[pic], *thr), edges)
    m = META["cases"][name]
    assert (int((st == 2).sum()), int((st == 1).sum()), int((flood == 255).sum()), sweeps) == \
        (m["strong"], m["weak"], m["edges"], m["sweeps"])
    assert set(np.unique(flood)) <= {0, 255} and bool(((flood == 255) <= (st >= 1)).all()) and bool((flood[st == 2] == 255).all())


def test_swapped_and_fractional_thresholds():
    assert K.thresholds(200, 100) == (100, 200) and K.thresholds(99.9, 200.5) == (99, 200) and K.thresholds(-0.5, 3) == (-1, 3)
    for pic in G.SWEPT:
        assert np.array_equal(CASES[pic][3], CASES[G.case_name(pic, (200, 100))][3])
        assert int((CASES[G.case_name(pic, (0, 2000))][3] != 0).sum()) == 0            # nothing is strong: no edge
        st0 = CASES[G.case_name(pic, (0, 0))][2]
        assert int((st0 == 1).sum()) == 0 and int((st0 == 2).sum()) > 0                # every survivor is strong
    assert not np.array_equal(CASES["smooth2"][2], CASES[G.case_name("smooth2", (99.9, 200.5))][2])   # 99 is not 100
    with pytest.raises(ValueError):
        K.thresholds(float("nan"), 1)
    with pytest.raises(ValueError):
        K.canny(np.zeros((4, 4, 2), np.uint8))
    with pytest.raises(ValueError):
        K.canny(np.zeros((4, 4), np.float32))


def test_steps_and_flat_pictures():
    v, h = CASES["step_v"][3], CASES["step_h"][3]
    assert bool((v[:, 7] == 255).all()) and int((v != 0).sum()) == 16            # a vertical step at column 8 keeps column 7
    assert bool((h[7, :] == 255).all()) and int((h != 0).sum()) == 16            # a horizontal one keeps row 7
    for d in ("step_d1", "step_d2"):
        e = CASES[d][3]
        assert 16 <= int((e != 0).sum()) <= 32 and int((e != 0).sum(1).max()) <= 2     # a thin diagonal line
    assert not CASES["flat0"][3].any() and not CASES["flat255"][3].any()
    assert np.array_equal(CASES["step_d1"][3], CASES["step_d1"][3].T)            # the anti-diagonal step is symmetric


def test_channel_choice_and_its_tie_rule():
    """the three channels of `chan` carry different gradients at the same pixels: its edges are no single channel's.  In `ties`
    two channels often have equal magnitudes, and the lower index decides: with R and G swapped -- the same set of channels,
    the tie broken the other way -- states and edges differ"""
    a = PICS["chan"]
    e = CASES["chan"][3]
    singles = [K.canny(a[:, :, c]) for c in range(3)]
    assert all(not np.array_equal(e, s) for s in singles)
    t = PICS["ties"]
    swapped = np.ascontiguousarray(t[:, :, [1, 0, 2]])                          # G first: the tie goes the other way
    assert int((K.canny_states(swapped, 100, 200) != CASES["ties"][2]).sum()) >= 2
    assert not np.array_equal(K.canny(swapped), CASES["ties"][3])
    gray = np.repeat(PICS["serp70"][:, :, None], 3, 2)                          # three equal channels: the one-channel result
    assert np.array_equal(K.canny(gray), CASES["serp70"][3])


def test_serpentine_counts():
    m = META["cases"]
    assert (m["serp70"]["strong"], m["serp70"]["weak"], m["serp70"]["edges"], m["serp70"]["sweeps"]) == (15, 2302, 2317, 1148)
    assert (m["serp70_off"]["strong"], m["serp70_off"]["weak"], m["serp70_off"]["edges"]) == (0, 2316, 0)
    assert m["serp133"]["edges"] == m["serp133"]["strong"] + m["serp133"]["weak"] > 6000 and m["serp133"]["sweeps"] > 3000
    assert m["serp133_off"]["edges"] == 0 and m["serp133_off"]["weak"] > 6000
    # one component: every weak pixel hangs on the 15 strong ones, and a fixed number of sweeps well below 1148 misses most
    st = CASES["serp70"][2]
    edge, cand = st == 2, st >= 1
    for _ in range(64):
        p = np.pad(edge, 1)
        edge = np.logical_or.reduce([p[dy:dy + 70, dx:dx + 150] for dy in range(3) for dx in range(3)]) & cand
    assert int(edge.sum()) < 400 < int((CASES["serp70"][3] == 255).sum())


# ---- (b): the kernels on the CPU emulation ---------------------------------------------------------------------------
def _ithr(thr):
    return K.thresholds(*thr) if thr[0] <= thr[1] else tuple(int(np.floor(t)) for t in thr)      # the entry point swaps itself


@pytest.fixture(scope="module")
def emu_run(tmp_path_factory):
    """build tools/cpu_emu/emu_canny, run it once over every fixture case + a batch of two + an unaligned picture"""
    if not os.path.exists(CXX):
        pytest.skip("clang++ of the ROCm toolchain not available")
    out = str(tmp_path_factory.mktemp("pfd_emu_canny"))
    subprocess.run([sys.executable, os.path.join(REPO, "tools", "cpu_emu", "build.py"), out], check=True,
                   stdout=subprocess.DEVNULL, env=dict(os.environ, EMU_ONLY="emu_canny", EMU_OPT="-O1"))
    runs = {}        # name -> (source [b, h, w, c], (low, high), offset, forms, expected states [b, h, w], expected edges)
    for name, (pic, thr, states, edges) in CASES.items():
        a = PICS[pic].reshape(1, *PICS[pic].shape[:2], -1)
        forms = 3 if a.size <= 3 * 64 * 64 or name in ("smooth3", "serp70") else 1
        runs[name.replace("@", "_at_").replace(",", "_")] = (a, _ithr(thr), 0, forms, states[None], edges[None])
    two = np.stack([PICS["p70x150"], np.repeat(PICS["serp70"][:, :, None], 3, 2)])
    runs["batch_of_two"] = (two, (100, 200), 0, 3, np.stack([CASES["p70x150"][2], CASES["serp70"][2]]),
                            np.stack([CASES["p70x150"][3], CASES["serp70"][3]]))
    runs["photo_off3"] = (PICS["photo"][None], (100, 200), 3, 1, CASES["photo"][2][None], CASES["photo"][3][None])
    with open(os.path.join(out, "cases.txt"), "w") as f:
        for name, (a, (lo, hi), off, forms, _, _) in runs.items():
            b, h, w, c = a.shape
            f.write(f"{name} {b} {h} {w} {c} {lo} {hi} {off} {forms}\n")
            np.ascontiguousarray(a).tofile(os.path.join(out, name + ".src"))
    r = subprocess.run([os.path.join(out, "emu_canny"), out], capture_output=True, text=True, timeout=900)
    lines = [l for l in r.stdout.splitlines() if l.startswith(("ok", "FAIL"))]
    assert r.returncode == 0 and len(lines) == len(runs) and all(l.startswith("ok") for l in lines), \
        r.stdout[-3000:] + r.stderr[-1000:]
    res = {}
    for name, (a, thr, off, forms, states, edges) in runs.items():
        b, h, w, c = a.shape
        rd = lambda ext, dt: np.fromfile(os.path.join(out, name + ext), dtype=dt)      # noqa: E731
        res[name] = dict(states=states, edges=edges, got_states=rd(".states", np.uint8).reshape(b, h, w),
                         u8=rd(".out_u8", np.uint8).reshape(b, h, w), line=[l for l in lines if l.split()[1] == name][0])
        if forms & 2:
            res[name].update(f16=rd(".out_f16", np.float16).reshape(b, 3, h, w), f32=rd(".out_f32", np.float32).reshape(b, 3, h, w))
    return res


EMU_NAMES = [c.replace("@", "_at_").replace(",", "_") for c in CASES] + ["batch_of_two", "photo_off3"]


@pytest.mark.parametrize("name", EMU_NAMES)
def test_kernels_on_the_emulation(emu_run, name):
    """state bytes and edge bytes == the specification's; the hint forms are the edge map / 255 in three equal planes"""
    r = emu_run[name]
    assert int((r["got_states"] != r["states"]).sum()) == 0
    assert int((r["u8"] != r["edges"]).sum()) == 0
    if "f32" in r:
        want = np.repeat((r["edges"] // 255)[:, None], 3, 1)
        assert r["f32"].dtype == np.float32 and np.array_equal(r["f32"], want.astype(np.float32))
        assert np.array_equal(r["f16"].view(np.uint16), want.astype(np.float16).view(np.uint16))


def test_emulation_ran_every_kernel_four_launches_a_call(emu_run):
    seen = " ".join(r["line"] for r in emu_run.values())
    for k in ("canny_nms_kernel<3>", "canny_nms_kernel<1>", "canny_link_kernel", "canny_resolve_kernel", "canny_emit_kernel"):
        assert k in seen, (k, seen)
    # the launch count depends on nothing but the number of calls: the serpentine (1148 sweeps deep) and a flat picture alike
    assert " 4 launches" in emu_run["serp133"]["line"] and " 4 launches" in emu_run["p128x256"]["line"]
    assert " 12 launches" in emu_run["flat0"]["line"] and " 12 launches" in emu_run["serp70"]["line"]
    assert any(f32.any() for f32 in (r.get("f32") for r in emu_run.values()) if f32 is not None)


# ---- (c) C ABI bounds (nothing is launched on an error, so no device is needed) --------------------------------------
def test_cabi_bounds_of_the_detector():
    from lib.hip import binding
    lib = binding.load()
    assert binding.ABI_VERSION == 10 and lib.pfd_abi_version() == 10
    chk = lib.pfd_canny_check
    for good in ((1, 1, 1, 1), (1, 512, 512, 3), (2, 768, 1024, 3), (1, 4096, 4096, 3), (127, 4096, 4096, 1), (1 << 20, 1, 2047, 3)):
        assert chk(*good) == 0, good
    for bad in ((0, 64, 64, 3), (1, 64, 64, 2), (1, 64, 64, 4), (1, 64, 64, 0), (1, 0, 64, 3), (1, 64, 0, 3), (1, 4097, 64, 3),
                (1, 64, 4097, 1), (128, 4096, 4096, 3), (1 << 20, 1, 2048, 3), (-1, 64, 64, 3)):
        assert chk(*bad) == binding.PFD_ESHAPE, bad
    buf = ctypes.create_string_buffer(4096)
    p = ctypes.addressof(buf)
    run = lib.pfd_canny_u8
    for hole in range(5):        # src, states, parent, strong, out
        ptrs = [p] * 5
        ptrs[hole] = None
        assert run(ptrs[0], 1, 4, 4, 3, 100, 200, ptrs[1], ptrs[2], ptrs[3], ptrs[4], binding.IMG_U8, None) == binding.PFD_EINVAL
    assert run(p, 1, 4, 4, 3, 100, 200, p, p, p, p, binding.IMG_NHWC_F16, None) == binding.PFD_EINVAL     # no such output form
    assert run(p, 1, 4, 4, 3, 100, 200, p, p, p, p, 7, None) == binding.PFD_EINVAL
    assert run(p, 1, 4, 4, 2, 100, 200, p, p, p, p, binding.IMG_U8, None) == binding.PFD_ESHAPE
    assert run(p, 1, 4097, 4, 3, 100, 200, p, p, p, p, binding.IMG_U8, None) == binding.PFD_ESHAPE
    assert run(p, 0, 4, 4, 3, 100, 200, p, p, p, p, binding.IMG_NCHW_F32, None) == binding.PFD_ESHAPE
    assert bytes(buf) == bytes(4096)
    with pytest.raises(binding.PfdError, match="PFD_ESHAPE"):
        binding.check(chk(1, 64, 64, 4), "pfd_canny_check")


def test_symbols_are_added_and_the_abi_is_not_bumped():
    from lib.hip import binding
    header = open(os.path.join(REPO, "include", "pfd_hip.h")).read()
    assert "#define PFD_ABI_VERSION 10" in header
    lib = ctypes.CDLL(binding.lib_path())
    for name in ("pfd_canny_check", "pfd_canny_u8"):
        assert f"int {name}(" in header and name in binding.SIGNATURES and hasattr(lib, name)
    assert len(binding.SIGNATURES["pfd_canny_u8"][1]) == 13 and len(binding.SIGNATURES["pfd_canny_check"][1]) == 4
    assert "unverified" in header.lower() or "not been measured" in header            # no claim of equality with OpenCV


def test_ops_checks_come_before_any_launch():
    from lib.hip import ops
    x = torch.zeros(8, 8, 3, dtype=torch.uint8)
    for bad in (x.float(), x.numpy(), x[0], torch.zeros(1, 1, 8, 8, 3, dtype=torch.uint8)):
        with pytest.raises(ValueError):
            ops.canny_u8(bad)
    with pytest.raises(ValueError):
        ops.canny_u8(x, out='nhwc')
    with pytest.raises(ValueError):
        ops.canny_u8(x, out='hint', dtype=torch.bfloat16)
    for thr in ((float("nan"), 1), (1, float("inf")), ("a", 1), (None, 2)):
        with pytest.raises(ValueError):
            ops.canny_u8(x, *thr)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.canny_u8(x)
    assert ops.canny_thresholds(200, 100) == (100, 200) and ops.canny_thresholds(99.9, 200.5) == (99, 200)
    assert ops.canny_thresholds(-7, 1e12) == (-1, 2041) and ops.canny_thresholds(0, 2000) == (0, 2000)


# ---- (d) ControlNet.preprocess ---------------------------------------------------------------------------------------
def canny_u8_standin(img, low=100, high=200, out='u8', dtype=torch.float16, return_states=False):
    """what ops.canny_u8 computes, from the numpy specification, on the CPU (TEST INFRASTRUCTURE)"""
    x = img[None] if img.dim() == 3 else img
    assert x.dtype == torch.uint8 and x.dim() == 4
    st = np.stack([K.canny_states(a, low, high) for a in x.numpy()])
    e = torch.from_numpy(np.stack([K.hysteresis(s) for s in st]))
    res = e if out == 'u8' else (e // 255).to(dtype)[:, None].repeat(1, 3, 1, 1)
    return (res, torch.from_numpy(st)) if return_states else res


@pytest.fixture()
def ctl(monkeypatch):
    from lib.hip import ops
    from lib.model_zoo.controlnet import ControlNet
    monkeypatch.setattr(ops, "canny_u8", canny_u8_standin)
    return ControlNet.__new__(ControlNet)           # preprocess reads no weights


def _float_picture(name, dtype=torch.float32):
    return torch.from_numpy(PICS[name]).permute(2, 0, 1)[None].to(dtype).div(255)


def test_preprocess_types(ctl):
    x = torch.cat([_float_picture("smooth2"), _float_picture("smooth3")])
    assert ctl.preprocess(x, type='none') is None and ctl.preprocess(x, type=None) is None
    for t in ('input', 'shuffle_v11e'):
        y = ctl.preprocess(x.half(), type=t)
        assert y.dtype == torch.float32 and torch.equal(y, x.half().float())
    for t in ('canny', 'canny_v11p'):
        y = ctl.preprocess(x, type=t, size=[96, 130])              # the reference's call (app.py:246): size is ignored
        assert y.dtype == torch.float32 and tuple(y.shape) == (2, 3, 96, 130)
        for b in range(2):
            want = K.canny(x[b].mul(255).byte().permute(1, 2, 0).numpy()) // 255
            assert int(want.sum()) > 500
            for c in range(3):
                assert np.array_equal(y[b, c].numpy(), want.astype(np.float32))
    assert torch.equal(ctl.preprocess(x), ctl.preprocess(x, type='canny'))     # the default type
    y = ctl.preprocess(x[:1], type='canny', low_threshold=99.9, high_threshold=60, unknown_kwarg=1)
    assert np.array_equal(y[0, 0].numpy() * 255, K.canny(x[0].mul(255).byte().permute(1, 2, 0).numpy(), 60, 99))
    assert not torch.equal(y, ctl.preprocess(x[:1]))
    # fp16 pictures become bytes in fp16, as ToPILImage makes them on that tensor
    h = x[:1].half()
    want = K.canny(h[0].mul(255).byte().permute(1, 2, 0).numpy())
    assert np.array_equal(ctl.preprocess(h)[0, 1].numpy() * 255, want)


def test_preprocess_refusals(ctl):
    x = _float_picture("p64")
    with pytest.raises(ValueError, match="opens no files"):
        ctl.preprocess("assets/examples/some-input.jpg", type='canny')
    for bad in (x[0], x.mul(255).byte(), x[:, :1], PICS["p64"]):
        with pytest.raises(ValueError):
            ctl.preprocess(bad, type='canny')
    for t in ('depth', 'hed', 'softedge_v11p', 'mlsd', 'mlsd_v11p', 'normal', 'openpose', 'openpose_v11p', 'pidi',
              'scribble', 'lineart_v11p', 'lineart_anime_v11p', 'anything else'):
        with pytest.raises(NotImplementedError, match=t):
            ctl.preprocess(x, type=t)
    with pytest.raises(ValueError):
        ctl.preprocess(x, type='canny', low_threshold=float("nan"))


def test_preprocess_has_no_cpu_fallback():
    from lib.model_zoo.controlnet import ControlNet
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ControlNet.__new__(ControlNet).preprocess(_float_picture("p64"), type='canny')


# ---- (e) pipeline and server ------------------------------------------------------------------------------------------
BAD_PREPROCESS = [dict(control_preprocess='hed'), dict(control_preprocess='Canny'), dict(control_preprocess=1),
                  dict(control_preprocess='canny', control_thresholds=(float("nan"), 200)),
                  dict(control_preprocess='canny', control_thresholds=(100, float("inf"))),
                  dict(control_preprocess='canny', control_thresholds=(100,)),
                  dict(control_preprocess='canny', control_thresholds=(1, 2, 3)),
                  dict(control_preprocess='canny', control_thresholds=("low", "high")),
                  dict(control_preprocess='canny', control_thresholds=None),
                  dict(control_thresholds=(float("nan"), 1))]


def test_submit_refuses_bad_preprocess_arguments_on_the_callers_thread():
    from stubs import StubNet, StubSampler
    from lib.serving import PromptFreeServer
    srv = PromptFreeServer(StubNet(), use_graph=False, max_batch=4)
    srv.pipe.sampler = StubSampler(0)
    ran = []
    srv._generate = lambda batch: ran.append(batch) or [None for _ in batch]
    try:
        img = torch.rand(1, 3, 64, 64)
        u8, fl = np.zeros((40, 50, 3), np.uint8), torch.rand(1, 3, 64, 64)
        for kw in BAD_PREPROCESS:
            for control in (u8, fl):
                with pytest.raises(ValueError):
                    srv.submit(img, 1, 64, 64, control=control, **kw)
        with pytest.raises(ValueError, match="without a control"):
            srv.submit(img, 1, 64, 64, control_preprocess='canny')
        with pytest.raises(ValueError):
            srv.submit(img, 1, 64, 64, control=np.zeros((2000, 64, 3), np.uint8), control_preprocess='canny')
        assert ran == []                                               # nothing reached the worker
        # the request carries the two values; a default call carries None and the default pair
        srv.submit(img, 1, 64, 64, control=u8, control_preprocess='canny', control_thresholds=(50, 150.5)).result(30)
        srv.submit(img, 1, 64, 64, control=fl, control_preprocess='canny').result(30)
        srv.submit(img, 1, 64, 64, control=fl).result(30)
        srv.submit(img, 1, 64, 64).result(30)
        reqs = [b[0] for b in ran]
        assert [len(b) for b in ran] == [1, 1, 1, 1]
        assert [(r.control_preprocess, r.control_thresholds) for r in reqs] == \
            [('canny', (50.0, 150.5)), ('canny', (100.0, 200.0)), (None, (100.0, 200.0)), (None, (100.0, 200.0))]
        # a preprocessed control is a control: the key has no new field, and the default call's key is what it was
        assert reqs[0].key() == reqs[1].key() == reqs[2].key() == (64, 64, 50, 2.0, 0.0, False, True, True, False)
        assert reqs[3].key() == (64, 64, 50, 2.0, 0.0, True, True, True, False)
    finally:
        srv.close()


class _RecordingSampler:
    def __init__(self):
        self.controls = []

    def enable_graph(self, on=True):
        pass

    def sample(self, steps, shape, x_info, c_info, eta=0., verbose=True):
        self.controls.append(c_info.get('control'))
        return x_info['xt'] * 0.5, {}


def test_worker_applies_the_preprocessor_where_it_ingests_the_control(monkeypatch):
    """float control + 'canny' through submit, the detector replaced by its CPU stand-in: the sampler is handed the edge hint, at
    the request's thresholds; a uint8 control reaches the resampler's front door (no CPU fallback) and fails its own request"""
    from stubs import StubNet
    from lib.hip import ops
    from lib.model_zoo.controlnet import ControlNet
    from lib.serving import PromptFreeServer
    monkeypatch.setattr(ops, "canny_u8", canny_u8_standin)
    net = StubNet()
    net.ctl = ControlNet.__new__(ControlNet)
    srv = PromptFreeServer(net, use_graph=False, max_batch=4)
    srv.pipe.sampler = rec = _RecordingSampler()
    try:
        img, ctl_f = torch.rand(1, 3, 64, 64), _float_picture("p64")
        srv.submit(img, 1, 64, 64, steps=2, control=ctl_f, control_preprocess='canny', control_thresholds=(50, 120)).result(60)
        srv.submit(img, 1, 64, 64, steps=2, control=ctl_f).result(60)
        f = srv.submit(img, 1, 64, 64, steps=2, control=PICS["p64"], control_preprocess='canny')
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            f.result(60)
    finally:
        srv.close()
    assert len(rec.controls) == 2
    want = K.canny(ctl_f[0].mul(255).byte().permute(1, 2, 0).numpy(), 50, 120) // 255
    assert tuple(rec.controls[0].shape) == (1, 3, 64, 64) and int(want.sum()) > 100
    assert np.array_equal(rec.controls[0][0, 2].numpy(), want.astype(np.float32))
    assert torch.equal(rec.controls[1], ctl_f)                          # the default: the control picture is the hint


def test_generate_refuses_bad_preprocess_arguments_before_any_device_work(monkeypatch):
    from stubs import StubNet
    from lib.hip import ops
    from lib.model_zoo.controlnet import ControlNet
    from lib.pipeline import PromptFreePipeline
    net, rec = StubNet(), _RecordingSampler()
    encoded = []
    encode = net.ctx_encode
    net.ctx_encode = lambda image, which: encoded.append(1) or encode(image, which)
    pipe = PromptFreePipeline(net, sampler=rec)
    img, u8, fl = torch.rand(1, 3, 64, 64), np.zeros((40, 50, 3), np.uint8), _float_picture("p64")
    for kw in BAD_PREPROCESS:
        for control in (u8, fl):
            with pytest.raises(ValueError):
                pipe.generate(img, 1, 64, 64, steps=2, control=control, **kw)
            if kw.get("control_preprocess") is not None:
                with pytest.raises(ValueError):
                    pipe.control_hint(control, 64, 64, kw["control_preprocess"], kw.get("control_thresholds", (100, 200)))
    with pytest.raises(ValueError, match="without a control"):
        pipe.generate(img, 1, 64, 64, steps=2, control_preprocess='canny')
    assert encoded == [] and rec.controls == []
    with pytest.raises(RuntimeError, match="no CPU fallback"):          # a good uint8 control reaches the kernels' front door
        pipe.generate(img, 1, 64, 64, steps=2, control=u8, control_preprocess='canny')
    assert rec.controls == []
    # float control through net.ctl.preprocess (the detector's stand-in), and control_hint returns what the sampler is given
    monkeypatch.setattr(ops, "canny_u8", canny_u8_standin)
    net.ctl = ControlNet.__new__(ControlNet)
    pipe.generate(img, 1, 64, 64, steps=2, control=fl, control_preprocess='canny', control_thresholds=(200, 100), decode=False)
    hint = pipe.control_hint(fl, 64, 64, 'canny', (100, 200))
    assert torch.equal(rec.controls[-1], hint) and np.array_equal(hint[0, 0].numpy() * 255, K.canny(PICS["p64"]))
    assert torch.equal(pipe.control_hint(fl, 64, 64), fl)               # no preprocessor: the picture itself
    pipe.generate(img, 1, 64, 64, steps=2, control=fl, decode=False)    # the default call: as before
    assert torch.equal(rec.controls[-1], fl)


# ---- (f) ------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not available")
def test_canny_kernels_use_no_scratch():
    import isa_audit
    bad, rows = isa_audit.findings([os.path.join(REPO, "prompt-free-diffusion_amd", "csrc", "canny.hip")])
    kernels = {k: v for _, k, v in rows}
    assert len(kernels) == 5, sorted(kernels)          # nms: C = 3 | 1; link; resolve; emit
    assert all(v["scratch"] == 0 for v in kernels.values()), kernels
    assert not [b for b in bad if "scratch" in b]
    # the staging loads of the tile kernel are unconditional (clamped addresses): none is waited for on its own
    assert all(v["serialised"] == 0 for k, v in kernels.items() if "canny_nms_kernel" in k), kernels
