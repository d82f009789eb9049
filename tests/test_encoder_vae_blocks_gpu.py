"""Block-level tests of the SeeCoder and AutoKL host layers on the device: every case of tests/encoder_vae_refs.py through the real
`.hip` methods on libpfd_hip.so against the plain fp64 formula, within T = 4 f (f: the floor of the case, the stand-in run of the
same host path on the CPU against the same formula -- tests/test_blocks_cpu.py derives the margin; T never depends on the device
result).  The path census, repeatability, untouched inputs AND parameters, the two forms of AttnBlock, the positional-feature cache
and the host layer's argument errors."""
import os
import time

import pytest
import torch

import block_refs as BR
import encoder_vae_refs as EV
import ops_standin as SI

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "encoder_vae_block_paths.txt")
IDS = [c["id"] for c in EV.CASES]
_SPENT = [0.0]


@pytest.fixture(autouse=True)
def _clock():
    t = time.time()
    yield
    _SPENT[0] += time.time() - t
    print(f"[ev-blocks-gpu] file total so far {_SPENT[0]:.1f} s")


@pytest.mark.parametrize("cid", IDS)
def test_case_on_device(cid):
    """.hip on the device within T of the fp64 formula; the census is the recorded one and names the case's branch; a second
    launch gives the same bits; the inputs and every parameter of every module are unchanged"""
    c = BR.CASE[cid]
    b = BR.built(cid)
    T = 4 * SI.floor(c)
    t0 = time.time()
    y, cen, same, kept = BR.run_gpu(c, census=True, params=True)
    dt = time.time() - t0
    e = BR.err_units(y, b.ref64, b.B)
    print(f"[ev-blocks-gpu] {cid}: f {T / 4:.3f} T {T:.3f} err {e:.3f} err / T {e / T:.3f} device part {dt:.2f} s")
    print(f"[ev-blocks-gpu] census {cen.line(cid)}")
    assert y.shape == b.ref64.shape and e <= T
    assert same, "second launch differs"
    assert kept, "an input was modified"
    assert not b.params_changed, f"parameters were modified: {b.params_changed}"
    gold = BR.read_golden_paths(GOLDEN)[cid]
    assert cen.log == gold
    assert c["branch"] in " ".join(cen.log), (c["branch"], cen.log)
    assert cen.again == cen.remembered(), "a run from the decline memory of the last one asked the library again"


@pytest.mark.parametrize("cid", [c["id"] for c in EV.CASES if c["forward"]])
def test_forward_calling_convention(cid):
    """one case per class through .forward (NCHW, the caller's dtype)"""
    c = BR.CASE[cid]
    b = BR.built(cid)
    T = 4 * SI.floor(c, fwd=True)
    y = BR.run_gpu(c, fwd=True)[0]
    e = BR.err_units(y, BR.ref_of(b, True), b.B)
    print(f"[ev-blocks-gpu] {cid} .forward: T {T:.3f} err {e:.3f} err / T {e / T:.3f}")
    assert e <= T


def test_attn_forms_agree():
    """the fused D = 512 launch and the chunked GEMM form of AttnBlock (ROWS 128: a chunk of 128 and a tail of 64; ROWS 4096: one
    chunk) on the same input: each within its T of the reference, within 2 T of each other"""
    base = BR.CASE["vae-attn-512-gemm-12x16-rows128"]
    b = BR.built(base["id"])
    ys, Ts = [], []
    for sw in ({}, dict(base["switches"]), {"PFD_VAE_ATTN": "gemm"}):
        c = dict(base, switches=sw)
        T = 4 * SI.floor(c)
        y = BR.run_gpu(c)[0]
        e = BR.err_units(y, b.ref64, b.B)
        print(f"[ev-blocks-gpu] {base['id']} {sw or 'fused'}: T {T:.3f} err {e:.3f} err / T {e / T:.3f}")
        assert e <= T, sw
        ys.append(y)
        Ts.append(T)
    for y in ys[1:]:
        d = max(BR.err_units(ys[0], y.double(), b.B), BR.err_units(y, ys[0].double(), b.B))
        print(f"[ev-blocks-gpu] AttnBlock forms differ by {d:.3f} (2 T = {2 * max(Ts):.3f})")
        assert d <= 2 * max(Ts)


def test_ppe_feature_cache():
    pe = BR._dev(BR.built("see-ppe-5x7"), "cuda")[0]["pe"]
    a, _ = EV.ppe_cache_check(pe, torch.device("cuda", torch.cuda.current_device()))
    assert torch.equal(a.cpu(), BR.run_gpu(BR.CASE["see-ppe-5x7"])[0])
    f = pe.features(5, 7, a.device)
    assert f.is_cuda and torch.equal(f.cpu(), pe._features_host(5, 7).half())


def test_argument_errors_before_any_launch(monkeypatch):
    from lib.hip import ops
    calls = EV.refusals("cuda")
    torch.cuda.synchronize()
    launches = []
    for name in ("_launch", "_stream"):
        real = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda *a, _r=real, **k: (launches.append(1), _r(*a, **k))[1])
    cen = BR.Census().install(monkeypatch)
    for what, exc, call in calls:
        with pytest.raises(exc):
            call()
        assert cen.log == [] and not launches, f"{what}: {cen.log} / {len(launches)} launches before the refusal"
