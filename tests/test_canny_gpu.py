"""Canny edge hints on the MI355X: ops.canny_u8 (csrc/canny.hip) against the numpy specification's bytes
(tests/golden/canny.npz, written by tools/make_canny_golden.py from lib/canny.py) on every case, in both output forms and both
hint dtypes; ControlNet.preprocess('canny'); and a request that goes from a uint8 photograph to latents through
PromptFreePipeline.generate and PromptFreeServer.submit with control_preprocess='canny'.
Zero differing bytes everywhere: there is no tolerance in this file.  The expected bytes are the specification's; their equality
with cv2.Canny is unverified.  (The CPU half is tests/test_canny_cpu.py.)"""
import json
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(REPO, "tools") not in sys.path:
    sys.path.insert(0, os.path.join(REPO, "tools"))

import make_canny_golden as G  # noqa: E402
import make_image_golden as GI  # noqa: E402  (the control photograph of the ingest tests and Pillow's resize of it)
from lib import canny as K  # noqa: E402

pytestmark = pytest.mark.gpu

META, PICS, CASES = G.load()


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def hwc(name):
    a = PICS[name]
    return a.reshape(a.shape[0], a.shape[1], -1)


def hint_of(edges, dtype):
    """ToTensor + repeat(1, 3, 1, 1) of an edge map [H, W] | [B, H, W] of 0 | 255 (host)"""
    e = torch.from_numpy(np.ascontiguousarray(edges))
    e = e[None] if e.dim() == 2 else e
    return e.float().div(255)[:, None].repeat(1, 3, 1, 1).to(dtype)


@pytest.mark.parametrize("name", list(CASES))
def test_canny_u8_matches_the_specification(name):
    from lib.hip import ops
    pic, thr, states, edges = CASES[name]
    src = dev(hwc(pic))
    got, st = ops.canny_u8(src, *thr, return_states=True)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (1,) + edges.shape == tuple(st.shape)
    nd_s, nd_e = int((st[0].cpu() != torch.from_numpy(states)).sum()), int((got[0].cpu() != torch.from_numpy(edges)).sum())
    print(f"{name}: {nd_s} state bytes and {nd_e} edge bytes of {edges.size} differ")
    assert nd_s == 0 and nd_e == 0
    for dtype in (torch.float16, torch.float32):
        h = ops.canny_u8(src, *thr, out='hint', dtype=dtype)
        assert h.dtype == dtype and tuple(h.shape) == (1, 3) + edges.shape
        assert torch.equal(h.cpu(), hint_of(edges, dtype))
    # the same call again, twice: the same bytes
    for _ in range(2):
        assert torch.equal(ops.canny_u8(src, *thr), got)


def test_batch_of_two_equals_two_single_calls():
    from lib.hip import ops
    for a, b in (("p70x150", "serp70"), ("smooth2", "smooth3"), ("serp133", "p133x200")):
        pa, pb = hwc(a), hwc(b)
        c = max(pa.shape[2], pb.shape[2])
        two = dev(np.stack([np.broadcast_to(pa, pa.shape[:2] + (c,)), np.broadcast_to(pb, pb.shape[:2] + (c,))]))
        for kw in (dict(), dict(out='hint', dtype=torch.float16), dict(out='hint', dtype=torch.float32)):
            got = ops.canny_u8(two, **kw)
            assert got.shape[0] == 2
            for i in range(2):
                assert torch.equal(got[i:i + 1], ops.canny_u8(two[i], **kw)), (a, b, kw, i)
        got = ops.canny_u8(two).cpu()
        assert torch.equal(got[0], torch.from_numpy(CASES[a][3])) and torch.equal(got[1], torch.from_numpy(CASES[b][3]))


def test_unaligned_views_give_the_same_bytes():
    """a picture that starts at an odd address (a slice of a larger buffer): same result"""
    from lib.hip import ops
    for name in ("photo", "p133x200", "t1x17"):
        a = hwc(name)
        buf = torch.zeros(a.size + 3, dtype=torch.uint8, device='cuda')
        for off in (1, 2, 3):
            buf[off:off + a.size] = dev(a).reshape(-1)
            view = buf[off:off + a.size].view(*a.shape)
            assert view.data_ptr() % 4 == off
            assert torch.equal(ops.canny_u8(view)[0].cpu(), torch.from_numpy(CASES[name][3]))


def test_capture_replays_on_another_picture():
    """four launches, no host synchronisation: the call is captured once and replayed after the input buffer is overwritten with
    another case of the same shape -- the serpentine, whose hysteresis is 1148 dilation sweeps deep"""
    from lib.hip import ops
    first, second = hwc("p70x150"), np.repeat(hwc("serp70"), 3, 2)
    x = dev(first)
    ops.canny_u8(x)
    ops.canny_u8(x, out='hint', dtype=torch.float16)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        e = ops.canny_u8(x)
        h = ops.canny_u8(x, 50, 150, out='hint', dtype=torch.float16)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(e[0].cpu(), torch.from_numpy(CASES["p70x150"][3]))
    assert torch.equal(h.cpu(), hint_of(K.canny(first, 50, 150), torch.float16))
    for _ in range(2):
        x.copy_(dev(second))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(e[0].cpu(), torch.from_numpy(CASES["serp70"][3]))
        assert torch.equal(h.cpu(), hint_of(K.canny(second, 50, 150), torch.float16))
    x.copy_(dev(np.repeat(hwc("serp70_off"), 3, 2)))
    g.replay()
    torch.cuda.synchronize()
    assert int(e.sum()) == 0                                           # nothing of the earlier replays is left behind


def test_out_of_bounds_requests_are_refused_before_launch():
    from lib.hip import binding, ops
    for shape in ((64, 64, 2), (64, 64, 4), (4097, 8, 3), (8, 4097, 1)):
        with pytest.raises(binding.PfdError, match="PFD_ESHAPE"):
            ops.canny_u8(torch.zeros(shape, dtype=torch.uint8, device='cuda'))
    lib = binding.load()
    t = torch.zeros(4096, dtype=torch.int32, device='cuda')
    p = t.data_ptr()
    assert lib.pfd_canny_u8(p, 1, 4097, 2, 3, 100, 200, p, p, p, p, 0, None) == binding.PFD_ESHAPE
    assert lib.pfd_canny_u8(p, 1, 8, 8, 2, 100, 200, p, p, p, p, 0, None) == binding.PFD_ESHAPE
    assert lib.pfd_canny_u8(p, 1, 8, 8, 3, 100, 200, p, p, p, p, 3, None) == binding.PFD_EINVAL
    assert lib.pfd_canny_u8(p, 1, 8, 8, 3, 100, 200, p, None, p, p, 0, None) == binding.PFD_EINVAL
    torch.cuda.synchronize()
    assert int(t.abs().sum()) == 0                                  # nothing was launched
    with pytest.raises(ValueError):
        ops.canny_u8(torch.zeros(8, 8, 3, device='cuda'))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.canny_u8(torch.zeros(8, 8, 3, dtype=torch.uint8))
    # the bound itself is served: one row and one column of 4096
    assert int(ops.canny_u8(torch.zeros(1, 4096, 3, dtype=torch.uint8, device='cuda')).sum()) == 0
    assert int(ops.canny_u8(torch.zeros(4096, 1, 1, dtype=torch.uint8, device='cuda')).sum()) == 0


def test_preprocess_on_float_pictures(net):
    """net.ctl.preprocess(x, type='canny') == canny(x.mul(255).byte()) of the specification, for an fp16 and an fp32 picture"""
    for dtype in (torch.float16, torch.float32):
        x = torch.stack([torch.from_numpy(PICS[n]).permute(2, 0, 1) for n in ("smooth2", "smooth3")]).to(dtype).div(255).cuda()
        y = net.ctl.preprocess(x, type='canny', size=[96, 130])
        assert y.dtype == torch.float32 and y.device == x.device and tuple(y.shape) == (2, 3, 96, 130)
        u8 = x.mul(255).byte().permute(0, 2, 3, 1).cpu().numpy()
        want = np.stack([K.canny(a) for a in u8])
        assert int((want == 255).sum()) > 1000
        assert torch.equal(y.cpu(), hint_of(want, torch.float32))
        y2 = net.ctl.preprocess(x[:1], type='canny_v11p', low_threshold=40.5, high_threshold=20)
        assert torch.equal(y2.cpu(), hint_of(K.canny(u8[0], 20, 40), torch.float32))
    assert net.ctl.preprocess(x, type='none') is None
    assert torch.equal(net.ctl.preprocess(x.half(), type='input'), x.half().float())
    with pytest.raises(NotImplementedError, match="hed"):
        net.ctl.preprocess(x, type='hed')
    with pytest.raises(ValueError):
        net.ctl.preprocess("picture.jpg")


@pytest.fixture(scope="module")
def request_inputs(net):
    """the reference picture and the control photograph of the ingest tests (400 x 300, resized to 64 x 64), and the hint a
    client of the float interface would build on the host: the specification's Canny of Pillow's resize (its bytes come from
    tests/golden/image_ingest.npz), ToTensor, three planes, in the model dtype"""
    pillow = dict(np.load(GI.GOLDEN, allow_pickle=False))
    assert json.loads(str(pillow["meta"]))["cases"]["down_big"]["output"] == [64, 64, 3]
    ref_u8, ctl_u8, resized = GI.source("up"), GI.source("down_big"), pillow["down_big"]
    dtype = net.get_dtype()
    hints = {thr: hint_of(K.canny(resized, *thr), dtype) for thr in ((100, 200), (360, 420))}
    assert [int(h[0, 0].sum()) for h in hints.values()] == [1219, 1008]      # (360, 420): 415 strong + 593 promoted weak
    assert not torch.equal(*hints.values())
    return ref_u8, ctl_u8, hints


def test_generate_with_canny_preprocess_equals_the_hint_from_the_host(net, request_inputs):
    from lib.pipeline import PromptFreePipeline
    ref_u8, ctl_u8, hints = request_inputs
    pipe = PromptFreePipeline(net)
    for thr, hint in hints.items():
        got_hint = pipe.control_hint(ctl_u8, 64, 64, 'canny', thr)
        assert got_hint.dtype == hint.dtype and torch.equal(got_hint.cpu(), hint)
    _, want = pipe.generate(ref_u8, 2, 64, 64, steps=4, scale=2.0, seed=11, control=hints[(100, 200)], decode=False)
    _, got = pipe.generate(ref_u8, 2, 64, 64, steps=4, scale=2.0, seed=11, control=ctl_u8, control_preprocess='canny',
                           decode=False)
    assert got.shape == (2, 4, 8, 8) and bool(torch.isfinite(got).all())
    assert torch.equal(got, want)
    _, got2 = pipe.generate(ref_u8, 2, 64, 64, steps=4, scale=2.0, seed=11, control=torch.from_numpy(ctl_u8)[None],
                            control_preprocess='canny', control_thresholds=(360, 420), decode=False)
    _, want2 = pipe.generate(ref_u8, 2, 64, 64, steps=4, scale=2.0, seed=11, control=hints[(360, 420)], decode=False)
    assert torch.equal(got2, want2) and not torch.equal(got2, got)      # the thresholds take part
    _, plain = pipe.generate(ref_u8, 2, 64, 64, steps=4, scale=2.0, seed=11, control=ctl_u8, decode=False)
    assert not torch.equal(plain, got)                                   # ... and so does the preprocessor
    # a float control picture goes through net.ctl.preprocess: the bytes are ToPILImage's of that tensor
    ctl_f = pipe.ingest(ctl_u8, (64, 64), 'control')
    _, got_f = pipe.generate(ref_u8, 2, 64, 64, steps=4, scale=2.0, seed=11, control=ctl_f, control_preprocess='canny',
                             decode=False)
    host = K.canny(ctl_f[0].mul(255).byte().permute(1, 2, 0).cpu().numpy())
    _, want_f = pipe.generate(ref_u8, 2, 64, 64, steps=4, scale=2.0, seed=11, control=hint_of(host, ctl_f.dtype), decode=False)
    assert torch.equal(got_f, want_f)


def test_served_request_with_canny_preprocess(net, request_inputs):
    from lib.serving import PromptFreeServer
    ref_u8, ctl_u8, hints = request_inputs
    srv = PromptFreeServer(net, use_graph=False, max_batch=4)
    try:
        f1 = srv.submit(ref_u8, 1, 64, 64, steps=4, seed=11, control=ctl_u8, control_preprocess='canny', as_uint8=True)
        f2 = srv.submit(ref_u8, 1, 64, 64, steps=4, seed=11, control=hints[(100, 200)], as_uint8=True)
        f3 = srv.submit(ref_u8, 1, 64, 64, steps=4, seed=11, control=ctl_u8, control_preprocess='canny',
                        control_thresholds=(420, 360), as_uint8=True)
        f4 = srv.submit(ref_u8, 1, 64, 64, steps=4, seed=11, control=hints[(360, 420)], as_uint8=True)
        with pytest.raises(ValueError):
            srv.submit(ref_u8, 1, 64, 64, steps=4, control=ctl_u8, control_preprocess='hed')
        with pytest.raises(ValueError):
            srv.submit(ref_u8, 1, 64, 64, steps=4, control_preprocess='canny')
        o1, o2, o3, o4 = (f.result(300) for f in (f1, f2, f3, f4))
        assert srv.batches == [1, 1, 1, 1]                           # control requests run alone, as before
    finally:
        srv.close()
    assert o1.dtype == torch.uint8 and o1.shape == (1, 64, 64, 3)
    assert torch.equal(o1, o2) and torch.equal(o3, o4) and not torch.equal(o1, o3)
