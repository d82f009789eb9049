"""uint8 pictures at the front door, on the MI355X: ops.image_from_u8 (csrc/image.hip) against Pillow's bytes
(tests/golden/image_ingest.npz, written by tools/make_image_golden.py) on all eleven cases, and a request that goes from
uint8 pictures to latents / uint8 pictures through PromptFreePipeline.generate and PromptFreeServer.submit.
Zero differing bytes everywhere: there is no tolerance in this file.  (The CPU half is tests/test_image_ingest_cpu.py.)"""
import hashlib
import json
import os
import sys

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if os.path.join(REPO, "tools") not in sys.path:
    sys.path.insert(0, os.path.join(REPO, "tools"))

import make_image_golden as G  # noqa: E402  (the closed-form inputs and the case list)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fixture():
    g = dict(np.load(G.GOLDEN, allow_pickle=False))
    g["meta"] = json.loads(str(g["meta"]))
    return g


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def to_tensor(u8_hwc):
    """torchvision's ToTensor on a uint8 HWC picture (host): CHW, .float().div(255)"""
    return torch.from_numpy(np.ascontiguousarray(u8_hwc)).permute(2, 0, 1).contiguous().float().div(255)[None]


@pytest.mark.parametrize("name", list(G.CASES))
def test_image_from_u8_matches_pillow(fixture, name):
    from lib.hip import ops
    h, w, c, kind, oh, ow, stored = G.CASES[name]
    src = dev(G.source(name))
    u8 = ops.image_from_u8(src, (oh, ow), layout='u8')
    assert u8.dtype == torch.uint8 and tuple(u8.shape) == (1, oh, ow, c)
    got = u8[0].cpu()
    if stored:
        want = torch.from_numpy(fixture[name])
        nd = int((got != want).sum())
        print(f"{name}: {nd} of {want.numel()} bytes differ")
        assert torch.equal(got, want)
    assert hashlib.sha256(got.numpy().tobytes()).hexdigest() == fixture["meta"]["cases"][name]["sha256"]
    # ToTensor fused into the last pass: bit for bit the host conversion of those bytes, fp32 and fp16, NCHW (and fp16 NHWC)
    want_f = to_tensor(got.numpy())
    f32 = ops.image_from_u8(src, (oh, ow), dtype=torch.float32)
    f16 = ops.image_from_u8(src, (oh, ow), dtype=torch.float16)
    nhwc = ops.image_from_u8(src, (oh, ow), dtype=torch.float16, layout='nhwc')
    assert f32.dtype == torch.float32 and f16.dtype == torch.float16 and tuple(f32.shape) == (1, c, oh, ow) == tuple(f16.shape)
    assert torch.equal(f32.cpu().view(torch.int32), want_f.view(torch.int32))
    assert torch.equal(f16.cpu().view(torch.int16), want_f.half().view(torch.int16))
    assert torch.equal(nhwc.cpu().view(torch.int16), want_f.half().permute(0, 2, 3, 1).contiguous().view(torch.int16))
    # the same call again, twice: the same bytes
    for _ in range(2):
        assert torch.equal(ops.image_from_u8(src, (oh, ow), layout='u8'), u8)
        assert torch.equal(ops.image_from_u8(src, (oh, ow), dtype=torch.float16), f16)


def test_totensor_only_all_256_values():
    from lib.hip import ops
    ramp = torch.arange(256, dtype=torch.uint8)
    want = ramp.float().div(255)
    for shape in ((16, 16, 1), (1, 256, 1), (4, 64, 1)):
        x = ramp.reshape(shape).cuda()
        assert torch.equal(ops.image_from_u8(x, None, dtype=torch.float32).cpu().reshape(-1).view(torch.int32), want.view(torch.int32))
        assert torch.equal(ops.image_from_u8(x, None, dtype=torch.float16).cpu().reshape(-1).view(torch.int16),
                           want.half().view(torch.int16))
        assert torch.equal(ops.image_from_u8(x, None, layout='u8').cpu().reshape(-1), ramp)
    rgb = torch.stack([ramp, ramp.flip(0), ramp.roll(7)], -1).reshape(16, 16, 3)       # three channels, [H, W, C] input
    out = ops.image_from_u8(rgb.cuda(), None, dtype=torch.float32)
    assert torch.equal(out.cpu(), to_tensor(rgb.numpy()))


def test_batch_of_three_equals_three_single_calls(fixture):
    from lib.hip import ops
    for name in ("up", "down", "w_same", "gray"):
        h, w, c, kind, oh, ow, stored = G.CASES[name]
        a = G.source(name)
        batch = dev(np.stack([a, a[::-1], np.roll(a, 5, axis=1)]))
        for kw in (dict(layout='u8'), dict(dtype=torch.float16), dict(dtype=torch.float32)):
            got = ops.image_from_u8(batch, (oh, ow), **kw)
            assert got.shape[0] == 3
            for i in range(3):
                assert torch.equal(got[i:i + 1], ops.image_from_u8(batch[i], (oh, ow), **kw)), (name, kw, i)
        assert torch.equal(ops.image_from_u8(batch, (oh, ow), layout='u8')[0].cpu(), torch.from_numpy(fixture[name]))


def test_unaligned_views_give_the_same_bytes(fixture):
    """a picture that starts at an odd address (a slice of a larger buffer) takes the byte-wise forms: same result"""
    from lib.hip import ops
    for name in ("up", "gray", "down"):
        h, w, c, kind, oh, ow, stored = G.CASES[name]
        a = G.source(name)
        buf = torch.zeros(a.size + 3, dtype=torch.uint8, device='cuda')
        for off in (1, 2, 3):
            buf[off:off + a.size] = dev(a).reshape(-1)
            view = buf[off:off + a.size].view(h, w, c)
            assert view.data_ptr() % 4 == off
            assert torch.equal(ops.image_from_u8(view, (oh, ow), layout='u8')[0].cpu(), torch.from_numpy(fixture[name]))


def test_out_of_bounds_requests_are_eshape():
    from lib.hip import binding, ops
    x = torch.zeros(64, 64, 3, dtype=torch.uint8, device='cuda')
    for img, size in ((x, (3, 64)), (x, (64, 3)), (x, (8193, 64)), (x, (64, 0)),
                      (torch.zeros(64, 64, 4, dtype=torch.uint8, device='cuda'), (32, 32)),
                      (torch.zeros(64, 64, 2, dtype=torch.uint8, device='cuda'), None),
                      (torch.zeros(1040, 8, 3, dtype=torch.uint8, device='cuda'), (64, 8))):
        with pytest.raises(binding.PfdError, match="PFD_ESHAPE"):
            ops.image_from_u8(img, size)
    lib = binding.load()
    t = torch.zeros(4096, dtype=torch.int32, device='cuda')
    p = t.data_ptr()
    assert lib.pfd_image_resample_h_u8(p, p, 1, 4, 100, 4, 3, p, p, p, 4, None) == binding.PFD_ESHAPE
    assert lib.pfd_image_resample_v_u8(p, p, 0, 1, 100, 4, 4, 3, p, p, p, 4, None) == binding.PFD_ESHAPE
    assert lib.pfd_image_resample_v_u8(p, p, 0, 1, 4, 8, 4, 3, None, None, None, 0, None) == binding.PFD_ESHAPE
    assert lib.pfd_image_resample_h_u8(None, p, 1, 4, 4, 8, 3, p, p, p, 4, None) == binding.PFD_EINVAL
    torch.cuda.synchronize()
    assert int(t.abs().sum()) == 0                                  # nothing was launched
    with pytest.raises(ValueError):
        ops.image_from_u8(x.float(), (32, 32))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.image_from_u8(x.cpu(), (32, 32))
    # the bound itself is served: 1024 -> 64 (64 taps), and enlarging far beyond 16
    assert ops.image_from_u8(torch.zeros(1024, 16, 3, dtype=torch.uint8, device='cuda'), (64, 16), layout='u8').shape == (1, 64, 16, 3)
    big = ops.image_from_u8(torch.full((2, 3, 3), 200, dtype=torch.uint8, device='cuda'), (700, 900), layout='u8')
    assert big.shape == (1, 700, 900, 3) and int(big.min()) == 200 and int(big.max()) == 200


def test_tap_table_for_a_new_size_is_refused_during_capture():
    from lib.hip import ops
    x = torch.zeros(40, 40, 3, dtype=torch.uint8, device='cuda')
    ops.image_from_u8(x, (48, 48))                                  # tables for 40 -> 48 now exist
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        y = ops.image_from_u8(x, (48, 48))                         # cached tables: capturable
        with pytest.raises(RuntimeError, match="during stream capture"):
            ops.image_from_u8(x, (47, 49))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(y, ops.image_from_u8(x, (48, 48)))


def _host_inputs(fixture, net):
    """what a client of the float interface builds on the host (app.py:232-244): ToTensor of the reference picture as it is,
    ToTensor of the control picture resized by Pillow -- its bytes come from the fixture -- both cast to the model dtype"""
    ref_u8, ctl_u8 = G.source("up"), G.source("down_big")
    dtype = net.get_dtype()
    return ref_u8, ctl_u8, to_tensor(ref_u8).to(dtype), to_tensor(fixture["down_big"]).to(dtype)


def test_generate_from_uint8_pictures_equals_the_float_path(net, fixture):
    """pipe.generate(u8 picture, control = u8 picture of another size) == pipe.generate(the float tensors built on the host from
    the fixture's bytes): the model input is bit-identical, so are the latents"""
    from lib.pipeline import PromptFreePipeline
    ref_u8, ctl_u8, ref_f, ctl_f = _host_inputs(fixture, net)
    assert ctl_u8.shape == (400, 300, 3) and tuple(ctl_f.shape) == (1, 3, 64, 64)
    pipe = PromptFreePipeline(net)
    assert torch.equal(pipe.ingest(ref_u8).cpu(), ref_f) and torch.equal(pipe.ingest(ctl_u8, (64, 64), 'control').cpu(), ctl_f)
    _, want = pipe.generate(ref_f, 2, 64, 64, steps=4, scale=2.0, seed=11, control=ctl_f, decode=False)
    _, got = pipe.generate(ref_u8, 2, 64, 64, steps=4, scale=2.0, seed=11, control=ctl_u8, decode=False)
    assert got.shape == (2, 4, 8, 8) and bool(torch.isfinite(got).all())
    assert torch.equal(got, want)
    _, got_t = pipe.generate(torch.from_numpy(ref_u8).cuda(), 2, 64, 64, steps=4, scale=2.0, seed=11,
                             control=torch.from_numpy(ctl_u8)[None], decode=False)       # torch uint8, on either side
    assert torch.equal(got_t, want)
    _, other = pipe.generate(ref_f, 2, 64, 64, steps=4, scale=2.0, seed=11, decode=False)
    assert not torch.equal(other, want)                              # the control picture takes part
    u8a, _ = pipe.generate(ref_u8, 1, 64, 64, steps=4, scale=2.0, seed=11, control=ctl_u8, as_uint8=True)
    u8b, _ = pipe.generate(ref_f, 1, 64, 64, steps=4, scale=2.0, seed=11, control=ctl_f, as_uint8=True)
    assert u8a.dtype == torch.uint8 and u8a.shape == (1, 64, 64, 3) and torch.equal(u8a, u8b)


def test_served_request_from_uint8_pictures_to_uint8_pictures(net, fixture):
    """the same through PromptFreeServer.submit(as_uint8=True): picture bytes in, picture bytes out, no float image on the host"""
    from lib.pipeline import PromptFreePipeline
    from lib.serving import PromptFreeServer
    ref_u8, ctl_u8, ref_f, ctl_f = _host_inputs(fixture, net)
    srv = PromptFreeServer(net, use_graph=False, max_batch=4)
    try:
        f1 = srv.submit(ref_u8, 1, 64, 64, steps=4, seed=11, control=ctl_u8, as_uint8=True)
        f2 = srv.submit(ref_f, 1, 64, 64, steps=4, seed=11, control=ctl_f, as_uint8=True)
        with pytest.raises(ValueError):
            srv.submit(ref_u8[:20], 1, 64, 64, steps=4)
        o1, o2 = f1.result(300), f2.result(300)                   # control requests run alone
        # (one after the other: queued together the two would share one DDIM batch, which is another computation)
        o3 = srv.submit(torch.from_numpy(ref_u8), 2, 64, 64, steps=4, seed=12, as_uint8=True).result(300)
        o4 = srv.submit(ref_f, 2, 64, 64, steps=4, seed=12, as_uint8=True).result(300)
        assert srv.batches == [1, 1, 2, 2]
    finally:
        srv.close()
    assert o1.dtype == torch.uint8 and o1.shape == (1, 64, 64, 3) and o3.shape == (2, 64, 64, 3)
    assert torch.equal(o1, o2) and torch.equal(o3, o4)
    direct, _ = PromptFreePipeline(net).generate(ref_u8, 1, 64, 64, steps=4, scale=2.0, seed=11, control=ctl_u8, as_uint8=True)
    assert torch.equal(o1, direct)
