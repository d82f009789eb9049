"""CPU: the fp64 references of tests/kernel_refs.py, which tests/test_encoder_kernels_gpu.py holds the HIP kernels of the
SeeCoder side against, pinned to the oracle (oracle/pfd_oracle.py, itself pinned to the reference project by
test_oracle_golden.py) -- and a check that the operands of the window-attention GPU test can tell a wrong kernel from a
right one."""
import pytest
import torch
import torch.nn.functional as F

import kernel_refs as KR
import pfd_oracle as O


def _block_sd(C, nH, g):
    """a Swin block whose attention output is visible: attn.proj = identity, mlp.fc2 = 0, everything else random"""
    r = lambda *s: torch.randn(s, generator=g)  # noqa: E731
    return {"norm1.weight": 1 + 0.2 * r(C), "norm1.bias": 0.1 * r(C),
            "attn.qkv.weight": 1.5 * C ** -0.5 * r(3 * C, C), "attn.qkv.bias": 0.5 * r(3 * C),
            "attn.relative_position_bias_table": r((2 * KR.WS - 1) ** 2, nH),
            "attn.proj.weight": torch.eye(C), "attn.proj.bias": torch.zeros(C),
            "norm2.weight": 1 + 0.2 * r(C), "norm2.bias": 0.1 * r(C),
            "mlp.fc1.weight": C ** -0.5 * r(8, C), "mlp.fc1.bias": r(8),
            "mlp.fc2.weight": torch.zeros(C, 8), "mlp.fc2.bias": torch.zeros(C)}


@pytest.mark.parametrize("shape", KR.SWIN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_swin_reference_is_the_oracles_block(shape):
    """O.swin_block(x) - x with an identity projection and a silent MLP is the window attention of qkv = linear(norm1(x)):
    fp32 oracle noise at |v| around 6 (5.7e-6 at most when this was written)"""
    B, H, W, nH, shift = shape
    C = nH * KR.HD
    g = torch.Generator().manual_seed(17 + sum(shape))
    sd = _block_sd(C, nH, g)
    p = O.SD(sd)
    x = torch.randn((B, H * W, C), generator=g)
    got = (O.swin_block(p, x, H, W, nH, KR.WS, shift) - x).reshape(B * H * W, C)
    qkv = O.linear(p.sub("attn.qkv."), O.layer_norm(p.sub("norm1."), x)).reshape(B * H * W, 3 * C)
    ref = KR.swin_window_attention_ref(qkv, sd["attn.qkv.bias"], sd["attn.relative_position_bias_table"], B, H, W, nH, shift,
                                       KR.HD ** -0.5)
    e = float((got.double() - ref).abs().max())
    print(f"[enc-kernels] swin reference vs oracle block {shape}: max abs {e:.2e} (max |ref| {float(ref.abs().max()):.2f})")
    assert e <= 1e-4, e


@pytest.mark.parametrize("mutant", KR.SWIN_MUTANTS)
def test_swin_operands_tell_wrong_variants_apart(mutant):
    """a condition on the INPUTS of the GPU test, not a measurement of the kernel: each wrong variant of the reference moves
    at least 30 % of the output elements of at least one listed shape by more than the GPU tolerance"""
    best = (0.0, None, 0.0)
    for shape in KR.SWIN_SHAPES:
        B, H, W, nH, shift = shape
        p = KR.swin_problem(shape)
        wrong = KR.swin_window_attention_ref(p["qkv"], p["qkv_bias"], p["rpb"], B, H, W, nH, shift, p["scale"], mutant=mutant)
        d = (wrong - p["ref"]).abs() / p["vmax"]
        share = float((d > KR.SWIN_TOL).double().mean())
        if share > best[0]:
            best = (share, shape, float(d.max()))
    print(f"[enc-kernels] mutant {mutant}: {100 * best[0]:.0f} % of the elements of {best[1]} move by more than "
          f"{KR.SWIN_TOL:.2e} vmax (largest {best[2]:.2f} vmax)")
    assert best[0] >= 0.30, best


def test_swin_reference_variants_only_differ_where_they_apply():
    """the mutants are the reference itself where their slip cannot show: no padding, no shift"""
    p = KR.swin_problem((1, 12, 12, 1, 0))
    for m in ("pad_reads_zero", "roll_reversed", "regions_from_unpadded"):
        assert torch.equal(KR.swin_window_attention_ref(p["qkv"], p["qkv_bias"], p["rpb"], 1, 12, 12, 1, 0, p["scale"], mutant=m),
                           p["ref"]), m


def test_patch_merge_reference_is_the_oracles_gather(monkeypatch):
    """the PatchMerging lines of O.swin_forward themselves (the oracle's sources are pinned by the trajectory fixture's digest,
    so they are watched in place, not factored out): a block-less Swin of width 48 on a 20x28 picture merges 5x7 -> 3x4 ->
    2x2 -> 1x1 tokens; every downsample norm's input is the restated gather of the tokens before it, bit for bit, and its
    output the fp64 gather + LayerNorm reference within fp32 noise"""
    B, dim = 2, 48
    g = torch.Generator().manual_seed(3)
    r = lambda *s: torch.randn(s, generator=g)  # noqa: E731
    sd = {"patch_embed.proj.weight": 0.2 * r(dim, 3, 4, 4), "patch_embed.proj.bias": 0.1 * r(dim),
          "patch_embed.norm.weight": 1 + 0.2 * r(dim), "patch_embed.norm.bias": 0.5 + 0.1 * r(dim)}
    for i in range(4):
        d = dim * 2 ** i
        sd.update({f"norm{i}.weight": torch.ones(d), f"norm{i}.bias": torch.zeros(d)})
        if i < 3:
            sd.update({f"layers.{i}.downsample.norm.weight": 1 + 0.2 * r(4 * d), f"layers.{i}.downsample.norm.bias": 0.1 * r(4 * d),
                       f"layers.{i}.downsample.reduction.weight": (4 * d) ** -0.5 * r(2 * d, 4 * d)})
    calls = []
    plain = O.layer_norm

    def spy(p, x, eps=1e-5):
        y = plain(p, x, eps)
        calls.append((p.prefix, x, y))
        return y

    monkeypatch.setattr(O, "layer_norm", spy)
    O.swin_forward(sd, "", r(B, 3, 20, 28), embed_dim=dim, depths=(0, 0, 0, 0), heads=(1, 1, 1, 1))
    by = {k: (x, y) for k, x, y in calls}
    hw = [(5, 7), (3, 4), (2, 2)]
    for i, (H, W) in enumerate(hw):
        d = dim * 2 ** i
        tokens = by[f"norm{i}."][0]                                   # the stage's tokens: what PatchMerging gathers from
        assert tuple(tokens.shape) == (B, H * W, d)
        gathered, normed = by[f"layers.{i}.downsample.norm."]
        x = tokens.view(B, H, W, d)
        assert torch.equal(KR.patch_merge_gather(x), gathered), i
        if H % 2:                                                     # the row below the image: the (1, 0) and (1, 1) parts are zero
            last = gathered.view(B, (H + 1) // 2, (W + 1) // 2, 4 * d)[:, -1]
            assert float(last[..., d:2 * d].abs().max()) == 0.0 and float(last[..., 3 * d:].abs().max()) == 0.0
        ref = KR.layernorm_patch_merge_ref(x, sd[f"layers.{i}.downsample.norm.weight"], sd[f"layers.{i}.downsample.norm.bias"])
        e = float((normed.reshape(-1, 4 * d).double() - ref).abs().max())
        print(f"[enc-kernels] gather LayerNorm reference vs oracle, {H}x{W}x{d}: max abs {e:.2e}")
        assert e <= 1e-5, e


def test_timestep_reference_and_its_fp64_yardstick():
    """O.timestep_embedding (fp32 frequencies, as the reference project defines them) against the all-fp64 formula: the
    argument t * f carries 2^-24 t f (its own rounding) + 3 * 2^-24 t f |ln f| (the exponent's three roundings,
    f |ln f| <= 1 / e) -> at t <= 999 below 999 * 2^-24 * (1 + 3 / e) * 1.5 = 1.9e-4 with the host's exp / cos / sin ulps"""
    t = torch.tensor([0, 1, 500, 999])
    for dim in (320, 321):
        a, b = O.timestep_embedding(t, dim), KR.timestep_embedding_ref64(t, dim)
        assert a.shape == b.shape == (4, dim)
        e = float((a.double() - b).abs().max())
        assert e <= 1.9e-4, e
        if dim % 2:
            assert float(a[:, -1].abs().max()) == 0.0 and float(b[:, -1].abs().max()) == 0.0


@pytest.mark.parametrize("cin", [3, 4])
@pytest.mark.parametrize("ks,stride,pad,extra", [(3, 1, 1, 0), (3, 2, 1, 0), (3, 2, 0, 1), (1, 1, 0, 0)])
def test_im2col_reference_is_a_convolution(cin, ks, stride, pad, extra):
    """col @ w in (tap, channel) order == conv2d, also with one more output row / column than symmetric padding gives (the
    bottom / right zero pad of the stride-2 callers); the pad columns of the patch matrix are zero"""
    B, H, W, N, kpad = 2, 6, 9, 5, 64
    g = torch.Generator().manual_seed(cin + ks + stride)
    x = torch.randn((B, H, W, cin), generator=g).half()
    w = torch.randn((N, cin, ks, ks), generator=g, dtype=torch.float64)
    ho, wo = (H + 2 * pad - ks) // stride + 1 + extra, (W + 2 * pad - ks) // stride + 1 + extra
    col = KR.im2col_ref(x, ks, stride, pad, kpad, ho if extra else None, wo if extra else None)
    assert tuple(col.shape) == (B * ho * wo, kpad) and float(col[:, ks * ks * cin:].abs().max()) == 0.0
    y = col[:, :ks * ks * cin].double() @ w.permute(0, 2, 3, 1).reshape(N, -1).t()
    xp = F.pad(x.double().permute(0, 3, 1, 2), (pad, pad + extra * stride, pad, pad + extra * stride))
    ref = F.conv2d(xp, w, stride=stride)[:, :, :ho, :wo].permute(0, 2, 3, 1).reshape(B * ho * wo, N)
    assert float((y - ref).abs().max()) <= 1e-12


def test_round_once_bound():
    """half an fp16 ulp of the value, 2^-25 where it is subnormal; every fp16 rounding of an in-range value passes without an allowance"""
    v = torch.tensor([0.0, 1e-7, 3e-5, 6.1e-5, 0.3, 1.0, 1000.0, 65000.0], dtype=torch.float64)
    b = KR.round_once_bound(v, 0.0)
    assert float(b[0]) == 2.0 ** -25 and float(b[5]) == 2.0 ** -11
    assert bool(((v.half().double() - v).abs() <= b).all())
    r, used = KR.bound_ratio(v.half(), v, 1e-9)            # a correct rounding: inside, and none of the allowance needed
    assert r <= 1.0 and used == 0.0
    r, used = KR.bound_ratio((v * (1 + 2.0 ** -9)).half(), v, 1e-9)
    assert r > 1.0 and used > 1.0
