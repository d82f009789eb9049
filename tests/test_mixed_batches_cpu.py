"""CPU: the host layers of the per-sample guidance scale (pfd_cfg_ddim_step_ps) and of the server's mixed batches: C ABI
declaration and argument checks, the refusals of ops.cfg_ddim_step, the world-size-invariant split of the scales, which
requests PromptFreeServer(mixed_batches=...) lets share a batch, and what `_generate` hands the sampler."""
import ctypes
import os
import re
import threading

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_declares_and_binding_lists_the_entry_point():
    from lib.hip import binding
    src = open(os.path.join(REPO, "include", "pfd_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    m = re.search(r"\bint\s+pfd_cfg_ddim_step_ps\s*\(([^)]*)\)\s*;", code)
    assert m and len(m.group(1).split(",")) == 18
    assert len(binding.SIGNATURES["pfd_cfg_ddim_step_ps"][1]) == 18
    assert "ddim.py:145-152" in src                      # the reference lines the entry point serves
    assert re.search(r"#define\s+PFD_ABI_VERSION\s+10\b", src) and binding.ABI_VERSION == 10     # added, not bumped


def test_cabi_rejects_bad_arguments_without_a_gpu():
    """argument validation happens before any launch"""
    from lib.hip import binding
    lib = binding.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)

    def call(nb=2, noise=None, key=None, scale=p, C=1):
        return lib.pfd_cfg_ddim_step_ps(p, nb, p, noise, key, 0, 1.0, p, scale, p, p, None, 1, 1, C, 1, 1, None)

    assert call(scale=None) == binding.PFD_EINVAL
    assert call(noise=p, key=p) == binding.PFD_EINVAL
    assert call(nb=3) == binding.PFD_EINVAL
    assert call(nb=0) == binding.PFD_EINVAL
    # the quad index of the seeded noise is one 32-bit counter word: C*h*w > 2^34 with a key is a shape error
    big = lib.pfd_cfg_ddim_step_ps(p, 2, p, None, p, 0, 1.0, p, p, p, p, None, 1, 1, 1 << 15, 1 << 10, 1 << 10, None)
    assert big == binding.PFD_ESHAPE
    assert lib.pfd_cfg_ddim_step_ps(p, 2, p, None, p, -1, 1.0, p, p, p, p, None, 1, 1, 1, 1, 1, None) == binding.PFD_EINVAL


def test_ops_refuse_a_malformed_scale():
    from lib.hip import ops
    x = torch.zeros(2, 4, 2, 2)
    eps = torch.zeros(2, 2, 2, 4, dtype=torch.float16)
    coef = torch.zeros(5)
    for bad in (torch.ones(2, dtype=torch.float64), torch.ones(2, dtype=torch.float16), torch.ones(3), torch.ones(2, 1),
                torch.ones(4)[::2], [1.5, 2.0], 2.0, torch.ones(2)):     # the last: right type and shape, but on the host
        with pytest.raises(ValueError, match="per-sample guidance scale"):
            ops.cfg_ddim_step(eps, 1, x, coef, scale=bad)
    with pytest.raises(ValueError, match="either noise or noise_key"):
        ops.cfg_ddim_step(eps, 1, x, coef, noise=torch.zeros_like(x), noise_key=torch.zeros(2, 2, dtype=torch.int64),
                          step=0, scale=torch.ones(2))


def test_sampler_classifies_and_checks_the_scale():
    from lib.model_zoo.ddim import is_per_sample, per_sample_scale
    import numpy as np
    for one in (2.0, 1, np.float32(2.0), torch.tensor(2.0)):
        assert not is_per_sample(one) and per_sample_scale(one, 3, 'cpu') is None
    for many in ([1.5, 2.0, 3.0], (1.5, 2.0, 3.0), np.array([1.5, 2.0, 3.0]), torch.tensor([1.5, 2.0, 3.0], dtype=torch.float64)):
        v = per_sample_scale(many, 3, 'cpu')
        assert v.dtype == torch.float32 and v.tolist() == [1.5, 2.0, 3.0] and v.is_contiguous()
    with pytest.raises(ValueError):
        per_sample_scale([1.5, 2.0], 3, 'cpu')
    with pytest.raises(ValueError):
        per_sample_scale(torch.ones(3, 1), 3, 'cpu')


def test_multicontext_sampling_refuses_a_per_sample_scale():
    from lib.model_zoo.ddim import DDIMSampler
    s = DDIMSampler.__new__(DDIMSampler)
    s.model = None                                      # the refusal comes before the model is looked at
    ci = {'unconditional_guidance_scale': [1.5, 2.0], 'conditioning': torch.zeros(2, 1, 1),
          'unconditional_conditioning': torch.zeros(2, 1, 1)}
    with pytest.raises(ValueError, match="out of scope"):
        s._mix_for([ci], 2)


def test_shard_scales_is_the_contiguous_split():
    from lib.pipeline import shard_scales
    scales = [1.5, 2.0, 3.0, 7.25]
    one = shard_scales(scales, 0, 1)
    assert one.dtype == torch.float32 and one.tolist() == scales
    halves = [shard_scales(scales, r, 2) for r in range(2)]
    assert [h.tolist() for h in halves] == [[1.5, 2.0], [3.0, 7.25]]
    assert torch.equal(torch.cat(halves), one)
    assert torch.equal(shard_scales(torch.tensor(scales), 1, 2), halves[1])
    with pytest.raises(ValueError):
        shard_scales(scales[:3], 0, 2)


def test_generate_checks_the_scale_length_and_the_hint_batch_before_the_device():
    from stubs import StubNet
    from lib.pipeline import PromptFreePipeline

    class _Net(StubNet):
        def ctx_encode(self, image, which):
            raise AssertionError("the device was touched before the arguments were checked")

    seen = {}

    class _Sampler:
        def sample(self, steps, shape, x_info, c_info, eta=0., verbose=True):
            seen['scale'] = c_info['unconditional_guidance_scale']
            return x_info['xt'], {}

    img = torch.rand(1, 3, 64, 64)
    pipe = PromptFreePipeline(_Net(), sampler=_Sampler())
    with pytest.raises(ValueError, match="one per sample"):
        pipe.generate(img, 2, 64, 64, steps=2, scale=[1.5, 2.0, 3.0], decode=False)
    with pytest.raises(ValueError, match="hint"):
        pipe.generate(img, 2, 64, 64, steps=2, control=torch.rand(3, 3, 64, 64), decode=False)
    # a good vector reaches the sampler as this rank's fp32 slice; one number is passed on as it is
    PromptFreePipeline(StubNet(), rank=1, world_size=2, sampler=_Sampler()).generate(
        img, 4, 64, 64, steps=2, scale=[1.5, 2.0, 3.0, 7.25], decode=False)
    assert seen['scale'].dtype == torch.float32 and seen['scale'].tolist() == [3.0, 7.25]
    PromptFreePipeline(StubNet(), sampler=_Sampler()).generate(img, 2, 64, 64, steps=2, scale=2.5, decode=False)
    assert seen['scale'] == 2.5 and isinstance(seen['scale'], float)


# ---- server: which requests share a batch (the pattern of tests/test_device_noise_cpu.py) ---------------------------
def _server(monkeypatch, max_batch=4, **kw):
    """PromptFreeServer with the device work stubbed: `_generate` records its batches as lists of seeds"""
    from lib import serving

    class _Pipe:
        def __init__(self, net):
            pass

        def enable_graph(self, on):
            pass

    monkeypatch.setattr(serving, "PromptFreePipeline", _Pipe)
    srv = serving.PromptFreeServer(object(), use_graph=False, max_batch=max_batch, **kw)
    calls = []

    def fake_generate(batch):
        calls.append([r.seed for r in batch])
        return [torch.full((r.n, 1), float(r.seed)) for r in batch]

    srv._generate = fake_generate
    return srv, calls


def _queued(srv, submits):
    """submit everything while the worker is held, so that all of it is queued when the worker looks"""
    gate = threading.Event()
    srv.call(lambda n: gate.wait(30))
    futs = [srv.submit(*a, **k) for a, k in submits]
    gate.set()
    return [f.result(30) for f in futs]


IMG = torch.rand(1, 3, 64, 64)
CTL = torch.rand(1, 3, 64, 64)


def _req(seed, **kw):
    return ((IMG, 1, 64, 64), dict(seed=seed, steps=4, **kw))


def _submissions():
    """(what is submitted, batches with mixed_batches=True, batches with the flag off)"""
    return [
        ([_req(1, scale=1.5), _req(2, scale=2.0), _req(3, scale=3.0)], [[1, 2, 3]], [[1], [2], [3]]),
        # scale 1 keeps its own key: the batch without CFG; order is preserved, so it also cuts the run in two
        ([_req(1, scale=1.5), _req(2, scale=1.0), _req(3, scale=1.0), _req(4, scale=3.0)], [[1], [2, 3], [4]],
         [[1], [2, 3], [4]]),
        ([_req(1, scale=1.5), _req(2, scale=2.0), _req(3, scale=1.0)], [[1, 2], [3]], [[1], [2], [3]]),
        ([_req(1, control=CTL), _req(2, control=CTL.flip(-1), scale=3.0)], [[1, 2]], [[1], [2]]),
        ([_req(1, control=CTL), _req(2)], [[1], [2]], [[1], [2]]),
        ([_req(1), _req(2, control=CTL), _req(3, control=CTL)], [[1], [2, 3]], [[1], [2], [3]]),
        # max_batch = 4
        ([_req(s, scale=1.0 + s) for s in (1, 2, 3, 4, 5)], [[1, 2, 3, 4], [5]], [[1], [2], [3], [4], [5]]),
        ([((IMG, 3, 64, 64), dict(seed=1, steps=4, scale=1.5)), ((IMG, 2, 64, 64), dict(seed=2, steps=4, scale=2.5)),
          _req(3, scale=3.5)], [[1], [2, 3]], [[1], [2], [3]]),
    ]


@pytest.mark.parametrize("case", range(8))
def test_server_with_the_flag_mixes_scales_and_control_pictures(monkeypatch, case):
    submits, want, _ = _submissions()[case]
    srv, calls = _server(monkeypatch, mixed_batches=True)
    try:
        outs = _queued(srv, submits)
        assert calls == want
        assert [float(o[0, 0]) for o in outs] == [float(k['seed']) for _, k in submits]      # each caller gets ITS result
    finally:
        srv.close()


@pytest.mark.parametrize("case", range(8))
def test_server_without_the_flag_batches_as_before(monkeypatch, case):
    """the default is guarded: one batch per scale value, control requests alone"""
    submits, _, want = _submissions()[case]
    srv, calls = _server(monkeypatch)
    try:
        _queued(srv, submits)
        assert calls == want
    finally:
        srv.close()


def test_request_key_and_shareable_with_and_without_the_flag():
    from lib import serving
    kw = dict(image=IMG, n=1, height=64, width=64, steps=4, seed=1, eta=0.0)
    R = serving._Request
    assert R(scale=1.5, **kw).key() != R(scale=2.0, **kw).key()                         # no `mixed` slot given: as before
    assert R(scale=1.5, **kw).key() == (64, 64, 4, 1.5, 0.0, True, True, False, False)
    assert not R(scale=2.0, control=CTL, **kw).shareable()
    assert R(scale=1.5, mixed=True, **kw).key() == R(scale=2.0, mixed=True, **kw).key()
    assert R(scale=1.0, mixed=True, **kw).key() != R(scale=2.0, mixed=True, **kw).key()
    assert R(scale=2.0, mixed=True, control=CTL, **kw).shareable()
    assert R(scale=2.0, mixed=True, control=CTL, **kw).key() != R(scale=2.0, mixed=True, **kw).key()
    assert not R(scale=2.0, mixed=True, control=CTL, **dict(kw, eta=0.5)).shareable()   # eta > 0 without device noise: alone


def test_server_generate_builds_the_scale_vector_and_the_hint_batch():
    """the real `_generate` over stand-ins for the device work"""
    from stubs import StubNet
    from lib import serving

    seen = {}

    class _Sampler:
        def enable_graph(self, on=True):
            pass

        def sample(self, steps, shape, x_info, c_info, eta=0., verbose=True):
            seen['scale'] = c_info['unconditional_guidance_scale']
            seen['control'] = c_info.get('control')
            return x_info['xt'], {}

    ctl = [torch.rand(1, 3, 64, 64, generator=torch.Generator().manual_seed(s)) for s in (1, 2, 3)]
    kw = dict(image=IMG, height=64, width=64, steps=2, eta=0.0, as_uint8=False, future=None)
    srv = serving.PromptFreeServer(StubNet(), use_graph=False, max_batch=8, mixed_batches=True)
    try:
        srv.pipe.sampler = _Sampler()
        R = serving._Request
        outs = srv._generate([R(n=2, seed=1, scale=1.5, mixed=True, **kw), R(n=1, seed=2, scale=7.25, mixed=True, **kw),
                              R(n=1, seed=3, scale=2.0, mixed=True, **kw)])
        assert [o.shape[0] for o in outs] == [2, 1, 1] and srv.batches == [4]
        assert torch.is_tensor(seen['scale']) and seen['scale'].dtype == torch.float32
        assert seen['scale'].tolist() == [1.5, 1.5, 7.25, 2.0] and seen['control'] is None
        # hints: row i of the batch is the control picture of the request that owns sample i
        srv._generate([R(n=1, seed=1, scale=1.5, control=ctl[0], mixed=True, **kw),
                       R(n=2, seed=2, scale=2.0, control=ctl[1], mixed=True, **kw),
                       R(n=1, seed=3, scale=3.0, control=ctl[2], mixed=True, **kw)])
        assert seen['scale'].tolist() == [1.5, 2.0, 2.0, 3.0]
        assert tuple(seen['control'].shape) == (4, 3, 64, 64)
        for row, owner in enumerate((0, 1, 1, 2)):
            assert torch.equal(seen['control'][row], ctl[owner][0]), row
        # scale 1 among themselves: one number, the batch without CFG
        srv._generate([R(n=1, seed=1, scale=1.0, mixed=True, **kw), R(n=1, seed=2, scale=1.0, mixed=True, **kw)])
        assert seen['scale'] == 1.0 and not torch.is_tensor(seen['scale'])
        # one request alone still takes the per-sample path: one graph per shape, whatever the scales
        srv._generate([R(n=2, seed=1, scale=2.0, mixed=True, **kw)])
        assert torch.is_tensor(seen['scale']) and seen['scale'].tolist() == [2.0, 2.0]
        # without the slot (flag off): today's call -- one number, one shared hint
        srv._generate([R(n=2, seed=1, scale=2.0, control=ctl[0], **kw)])
        assert seen['scale'] == 2.0 and not torch.is_tensor(seen['scale'])
        assert tuple(seen['control'].shape) == (1, 3, 64, 64)
    finally:
        srv.close()
