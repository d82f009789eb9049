"""CPU: the upsample convolution as four 2x2-tap phase convolutions (PfdGemmDesc.ups = 2).  (a) the algebra of the host-side
weight fold (layers.pack_conv_weight_ups): `conv3x3(nearest-2x(x))` == four padded 2x2 convolutions over the low-res image
with the folded weights, written to the four output phases; (b) the kernel form on the CPU emulation (tools/cpu_emu)."""
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.environ.get("EMU_CXX", "/opt/rocm/lib/llvm/bin/clang++")
EMU_CASES = 5       # the "phase-fold:" cases of tools/cpu_emu/emu_gemm.cpp


def _phase_conv(x, wp):
    """x [B, Cin, H, W], wp [4, N, 4*Cin] (the pack: phase blocks [py][px], taps (ty, tx) major, channels minor), float64"""
    B, Cin, H, W = x.shape
    N = wp.shape[1]
    y = torch.zeros((B, N, 2 * H, 2 * W), dtype=torch.float64)
    for py in range(2):
        for px in range(2):
            k = wp[py * 2 + px].double().view(N, 2, 2, Cin).permute(0, 3, 1, 2)
            # tap (ty, tx) reads low-res pixel (y + py - 1 + ty, x + px - 1 + tx); zeros outside the image
            xp = F.pad(x, (1 - px, px, 1 - py, py))
            y[:, :, py::2, px::2] = F.conv2d(xp, k)
    return y


@pytest.mark.parametrize("H,W", [(8, 8), (4, 16)])
def test_folded_phase_weights_reproduce_the_upsample_convolution(H, W):
    from lib.hip.layers import pack_conv_weight_ups
    Cin, N = 64, 32
    g = torch.Generator().manual_seed(5 + H)
    x = torch.randn((2, Cin, H, W), generator=g, dtype=torch.float64).half().double()
    w = torch.randn((N, Cin, 3, 3), generator=g, dtype=torch.float64) * (9 * Cin) ** -0.5

    def ref(w_):
        return F.conv2d(F.interpolate(x, scale_factor=2, mode="nearest"), w_, padding=1)

    # before the f16 rounding the fold is exact
    wp = pack_conv_weight_ups(w, dtype=torch.float64)
    assert tuple(wp.shape) == (4, N, 4 * Cin) and wp.dtype == torch.float64
    r = ref(w)
    e = float((_phase_conv(x, wp) - r).abs().max() / max(1.0, float(r.abs().max())))
    print(f"[phase-fold] {H}x{W}: unrounded fold, scaled max-abs {e:.2e}")
    assert e <= 1e-12, e
    # folded in fp32 from the f16 weight and rounded once to f16
    w16 = w.half()
    wp16 = pack_conv_weight_ups(w16)
    assert wp16.dtype == torch.float16 and wp16.is_contiguous()
    r = ref(w16.double())
    e = float((_phase_conv(x, wp16) - r).abs().max() / max(1.0, float(r.abs().max())))
    print(f"[phase-fold] {H}x{W}: fold rounded to f16, scaled max-abs {e:.2e}")
    assert e <= 5e-4, e


@pytest.mark.skipif(not os.path.exists(CXX), reason="clang++ of the ROCm toolchain not available")
def test_phase_form_on_the_cpu_emulation(tmp_path):
    """the loader-wave kernel's phase form (row order (b, phase, y, x), 2x2 tap walk, per-phase weight block, scattered store
    pass with and without statistics, both tile widths, both weight layouts) against the double-precision nearest-2x + 3x3
    reference, and a request the dispatcher must decline"""
    env = dict(os.environ, EMU_ONLY="emu_gemm")
    subprocess.run([sys.executable, os.path.join(REPO, "tools", "cpu_emu", "build.py"), str(tmp_path)], check=True,
                   stdout=subprocess.DEVNULL, env=env)
    r = subprocess.run([os.path.join(str(tmp_path), "emu_gemm"), "phase-fold"], capture_output=True, text=True, timeout=900)
    lines = [l for l in r.stdout.splitlines() if l.startswith(("ok", "FAIL"))]
    assert r.returncode == 0 and len(lines) == EMU_CASES and all(l.startswith("ok") for l in lines), \
        r.stdout[-3000:] + r.stderr[-1000:]
