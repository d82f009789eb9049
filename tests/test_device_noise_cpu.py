"""CPU: the seeded counter-based noise of the stochastic DDIM step (lib/noise.py = the specification of csrc/philox.h)
and the host layers that carry its keys: C ABI declarations, server coalescing, world-size invariance of the keys."""
import os
import re
import threading

import numpy as np
import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# counter words, key words -> output words (Philox4x32-10; the first two are the Random123 known answers)
KAT = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
       ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
       ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
        (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]


def test_philox_known_answers():
    from lib import noise
    for ctr, key, out in KAT:
        got = noise.philox4x32_10(np.array(ctr, dtype=np.uint32), np.array(key, dtype=np.uint32))
        assert got.dtype == np.uint32 and [int(v) for v in got] == list(out), (ctr, [hex(int(v)) for v in got])
    # array inputs: all three at once
    got = noise.philox4x32_10(np.array([k[0] for k in KAT], dtype=np.uint32), np.array([k[1] for k in KAT], dtype=np.uint32))
    assert got.shape == (3, 4) and got.tolist() == [list(k[2]) for k in KAT]


def test_normal_is_deterministic_and_a_prefix_of_itself():
    from lib import noise
    a, b = noise.normal(20, 3, 49, 4100), noise.normal(20, 3, 49, 4100)
    assert a.dtype == np.float32 and a.shape == (4100,) and np.array_equal(a, b)
    assert np.array_equal(noise.normal(20, 3, 49, 7), a[:7])         # a tail quad is simply cut


def test_normal_moments_and_range():
    """2^20 draws: five standard errors of the mean (5 / 1024 = 4.9e-3), the standard deviation to the same figure
    (its standard error is 1 / sqrt(2 n) = 6.9e-4), and the hard bound of the construction sqrt(-2 ln 2^-24)"""
    from lib import noise
    z = noise.normal(12345, 1, 0, 1 << 20).astype(np.float64)
    print("mean", z.mean(), "std", z.std(), "max|z|", np.abs(z).max())
    assert abs(z.mean()) <= 5e-3
    assert abs(z.std() - 1.0) <= 5e-3
    assert np.abs(z).max() <= 5.7682


def test_every_key_word_and_the_step_change_the_output():
    from lib import noise
    base = noise.normal(7, 2, 5, 64)
    for seed, sid, step in ((8, 2, 5), (7 + (1 << 32), 2, 5), (7, 3, 5), (7, 2, 6)):
        other = noise.normal(seed, sid, step, 64)
        assert not np.array_equal(base, other), (seed, sid, step)
        assert np.abs(base - other).max() > 0.1
    neg = noise.normal(-1, 0, 0, 64)
    assert np.isfinite(neg).all() and noise.key_words(-1) == (0xffffffff, 0xffffffff)
    assert np.array_equal(neg, noise.normal(-1, 0, 0, 64)) and not np.array_equal(neg, noise.normal(-2, 0, 0, 64))
    assert noise.key_words((1 << 40) + 12345) == (12345, 1 << 8)


def test_header_declares_and_binding_lists_both_entry_points():
    from lib.hip import binding
    src = open(os.path.join(REPO, "include", "pfd_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name, nargs in (("pfd_philox_normal_f32", 6), ("pfd_cfg_ddim_step_rng", 16)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", code)
        assert m, name
        assert len(m.group(1).split(",")) == nargs
        assert name in binding.SIGNATURES and len(binding.SIGNATURES[name][1]) == nargs
    assert "ddim.py:166-169" in src                      # the reference lines the entry points serve
    assert re.search(r"#define\s+PFD_ABI_VERSION\s+10\b", src) and binding.ABI_VERSION == 10


def test_cabi_rejects_a_missing_key_without_a_gpu():
    """argument validation happens before any launch"""
    import ctypes
    from lib.hip import binding
    lib = binding.load()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.pfd_cfg_ddim_step_rng(p, 2, p, None, 0, 1.0, p, p, p, None, 1, 1, 1, 1, 1, None) == binding.PFD_EINVAL
    assert lib.pfd_philox_normal_f32(None, 0, p, 1, 4, None) == binding.PFD_EINVAL
    assert lib.pfd_philox_normal_f32(p, 0, p, 1, 0, None) == binding.PFD_EINVAL


def test_ops_refuse_noise_and_noise_key_together():
    from lib.hip import ops
    x = torch.zeros(1, 4, 2, 2)
    key = torch.zeros(1, 2, dtype=torch.int64)
    with pytest.raises(ValueError):
        ops.cfg_ddim_step(torch.zeros(1, 2, 2, 4, dtype=torch.float16), 1, x, torch.zeros(5), noise=torch.zeros_like(x),
                          noise_key=key, step=0)
    with pytest.raises(ValueError):
        ops.noise_key_rows(torch.zeros(2, 2, dtype=torch.int32), 2, 'cpu')
    with pytest.raises(ValueError):
        ops.noise_key_rows(torch.zeros(3, 2, dtype=torch.int64), 2, 'cpu')


# ---- server: which requests share a batch ---------------------------------------------------------------------------
def _server(monkeypatch, max_batch=4):
    """PromptFreeServer with the device work stubbed, as tests/test_host.py does: `_generate` records its batches"""
    from lib import serving

    class _Pipe:
        def __init__(self, net):
            pass

        def enable_graph(self, on):
            pass

    monkeypatch.setattr(serving, "PromptFreePipeline", _Pipe)
    srv = serving.PromptFreeServer(object(), use_graph=False, max_batch=max_batch)
    calls = []

    def fake_generate(batch):
        calls.append([(r.seed, bool(r.device_noise)) for r in batch])
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


def test_server_coalesces_device_noise_requests_at_eta_above_zero(monkeypatch):
    srv, calls = _server(monkeypatch)
    img = torch.rand(1, 3, 64, 64)
    try:
        outs = _queued(srv, [((img, 1, 64, 64), dict(seed=s, eta=0.5, device_noise=True)) for s in (1, 2, 3)])
        assert [float(o[0, 0]) for o in outs] == [1.0, 2.0, 3.0]
        assert calls == [[(1, True), (2, True), (3, True)]]                     # ONE batch
    finally:
        srv.close()


def test_server_runs_eta_above_zero_without_the_flag_alone(monkeypatch):
    srv, calls = _server(monkeypatch)
    img = torch.rand(1, 3, 64, 64)
    try:
        _queued(srv, [((img, 1, 64, 64), dict(seed=s, eta=0.5)) for s in (1, 2)])
        assert calls == [[(1, False)], [(2, False)]]
    finally:
        srv.close()


def test_server_never_mixes_flagged_and_unflagged_requests(monkeypatch):
    from lib import serving
    srv, calls = _server(monkeypatch)
    img = torch.rand(1, 3, 64, 64)
    try:
        # eta = 0: both kinds are shareable, but only with their own kind (the key carries the flag)
        _queued(srv, [((img, 1, 64, 64), dict(seed=1, device_noise=True)), ((img, 1, 64, 64), dict(seed=2)),
                      ((img, 1, 64, 64), dict(seed=3))])
        assert calls == [[(1, True)], [(2, False), (3, False)]]
        del calls[:]
        _queued(srv, [((img, 1, 64, 64), dict(seed=4, eta=0.5, device_noise=True)),
                      ((img, 1, 64, 64), dict(seed=5, eta=0.5)),
                      ((img, 1, 64, 64), dict(seed=6, eta=0.5, device_noise=True))])
        assert calls == [[(4, True)], [(5, False)], [(6, True)]]
        for batch in calls:
            assert len({flag for _, flag in batch}) == 1
    finally:
        srv.close()
    kw = dict(image=img, n=1, height=64, width=64, steps=4, scale=2.0, seed=1)
    a = serving._Request(eta=0.5, device_noise=True, **kw)
    b = serving._Request(eta=0.5, device_noise=False, **kw)
    assert a.key() != b.key() and a.shareable() and not b.shareable()
    assert not serving._Request(eta=0.5, device_noise=True, control=img, **kw).shareable()   # control: alone, as before


def test_server_generate_hands_each_request_its_own_keys_and_leaves_the_global_generator_alone():
    """the real `_generate` over stand-ins for the device work: rows (request seed, j) in batch order, and no
    torch.manual_seed for a device_noise request"""
    from stubs import StubNet
    from lib import serving

    seen = {}

    class _Sampler:
        def enable_graph(self, on=True):
            pass

        def sample(self, steps, shape, x_info, c_info, eta=0., verbose=True):
            seen['key'] = None if x_info.get('noise_key') is None else x_info['noise_key'].clone()
            return x_info['xt'], {}

    srv = serving.PromptFreeServer(StubNet(), use_graph=False, max_batch=8)
    try:
        srv.pipe.sampler = _Sampler()
        img = torch.rand(1, 3, 64, 64)
        kw = dict(image=img, height=64, width=64, steps=2, scale=2.0, as_uint8=False, future=None)
        torch.manual_seed(99)
        before = torch.get_rng_state().clone()
        srv._generate([serving._Request(n=2, seed=-5, eta=0.5, device_noise=True, **kw),
                       serving._Request(n=1, seed=1 << 40, eta=0.5, device_noise=True, **kw)])
        assert seen['key'].dtype == torch.int64
        assert seen['key'].tolist() == [[-5, 0], [-5, 1], [1 << 40, 0]]
        assert torch.equal(torch.get_rng_state(), before)
        srv._generate([serving._Request(n=1, seed=7, eta=0.5, **kw)])      # the old path: no key, reseeded from ITS seed
        assert seen['key'] is None and not torch.equal(torch.get_rng_state(), before)
    finally:
        srv.close()


# ---- pipeline: the keys do not depend on the world size -------------------------------------------------------------
def test_generate_hands_the_sampler_the_same_key_rows_at_world_sizes_1_and_2():
    from stubs import StubNet
    from lib.pipeline import PromptFreePipeline

    class _Sampler:
        def __init__(self):
            self.keys, self.xts = [], []

        def enable_graph(self, on=True):
            pass

        def sample(self, steps, shape, x_info, c_info, eta=0., verbose=True):
            self.keys.append(x_info.get('noise_key'))
            self.xts.append(x_info['xt'])
            return x_info['xt'], {}

    img = torch.rand(1, 3, 64, 64)
    n_global, seed = 4, (1 << 35) + 9

    def run(rank, world, **kw):
        s = _Sampler()
        PromptFreePipeline(StubNet(), rank=rank, world_size=world, sampler=s).generate(
            img, n_global, 64, 64, steps=2, eta=0.5, seed=seed, decode=False, **kw)
        return s

    one = run(0, 1, device_noise=True)
    full = one.keys[0]
    assert full.dtype == torch.int64 and full.tolist() == [[seed, j] for j in range(n_global)]
    halves = [run(r, 2, device_noise=True) for r in range(2)]
    assert torch.equal(torch.cat([h.keys[0] for h in halves]), full)
    assert torch.equal(torch.cat([h.xts[0] for h in halves]), one.xts[0])      # the same global samples
    assert run(0, 1).keys[0] is None                                           # off by default
