"""The boundary kernels of csrc/elementwise.hip on every fp16 input and at production extents: inputs, oracles, mutants, bounds
and cases (tests/test_boundary_kernels_cpu.py qualifies them and runs the kernels on the CPU emulation,
tests/test_boundary_kernels_gpu.py runs them on the device).  Everything here is torch / numpy on the CPU; nothing imports the
native library.  A plain module, not a conftest: the two test files import it by name."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

import kernel_refs as KR

ACT_NONE, ACT_GELU, ACT_RELU, ACT_SILU = 0, 1, 2, 3          # PFD_ACT_* of include/pfd_hip.h
ACT_NAMES = ("none", "gelu", "relu", "silu")
PFD_EINVAL, PFD_ESHAPE = -1, -2
GRID_CAP = 4096 * 256                                         # grid_for (csrc/pfd_common.h): at most 4096 blocks of 256 threads


# ------------------------------------------------------------------------------------------------
# inputs
# ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def all_f16(kind):
    """every fp16 bit pattern of one kind, in bit order (0x0000 .. 0xFFFF): 'non_nan' the 63 490 patterns that are not NaN
    (+-0, the subnormals, +-65504 and +-inf among them), 'finite' the 63 488 without the two infinities, 'nan' the 2046
    NaN patterns.  CPU, fp16.  Computed once; do not modify."""
    bits = np.arange(65536, dtype=np.int32)
    expo, man = (bits >> 10) & 31, bits & 1023
    keep = {"non_nan": (expo != 31) | (man == 0), "finite": expo != 31, "nan": (expo == 31) & (man != 0)}[kind]
    x = torch.from_numpy(bits[keep].astype(np.uint16).view(np.float16).copy())
    assert x.numel() == {"non_nan": 63490, "finite": 63488, "nan": 2046}[kind]
    return x


def bits_of(t):
    """the bit patterns of an fp16 tensor as int32 (CPU)"""
    return t.detach().cpu().contiguous().view(torch.int16).to(torch.int32) & 0xFFFF


# ------------------------------------------------------------------------------------------------
# pfd_image_u8_f16
# ------------------------------------------------------------------------------------------------
IMAGE_MUL_ADD = ((0.5, 0.5), (1.0, 0.0))


def image_u8_ref(x, mul, add, f16_image, dtype=torch.float64):
    """the reference's output stage on the CPU: clamp(x * mul + add, 0, 1) in `dtype`, held in the image's type (float16 or
    float32), `.mul(255)` in that type, `.byte()` (truncation).  Only (mul, add) in IMAGE_MUL_ADD are specified: the product
    x * mul is exact for both (a power of two, or one), so a fused multiply-add and a product and a sum rounded one after
    the other give the same value, and the fp32 and the fp64 evaluation agree on every input (the CPU file checks that).
    NaN inputs are outside the oracle: `.byte()` of a NaN is undefined."""
    assert (mul, add) in IMAGE_MUL_ADD
    return (x.to(dtype) * mul + add).clamp(0, 1).to(torch.float16 if f16_image else torch.float32).mul(255).byte()


def _mut_no_f16_rounding(x, mul, add, f16_image):
    return image_u8_ref(x, mul, add, False)


def _mut_product_not_rounded(x, mul, add, f16_image):
    return (x.double() * mul + add).clamp(0, 1).half().double().mul(255).byte()


def _mut_flag_swapped(x, mul, add, f16_image):
    return image_u8_ref(x, mul, add, not f16_image)


def _mut_round_to_nearest(x, mul, add, f16_image):
    return (x.double() * mul + add).clamp(0, 1).to(torch.float16 if f16_image else torch.float32).mul(255).round().byte()


# name -> (wrong variant of image_u8_ref, the f16_image requests it applies to)
IMAGE_U8_MUTANTS = {
    "no_f16_rounding": (_mut_no_f16_rounding, (True,)),              # an f16 request computed as fp32
    "product_not_rounded": (_mut_product_not_rounded, (True,)),      # the image rounded to f16, v * 255 not
    "flag_swapped": (_mut_flag_swapped, (False,)),                   # f16 arithmetic on an fp32 request
    "round_to_nearest": (_mut_round_to_nearest, (True, False)),      # in place of truncation
}


# ------------------------------------------------------------------------------------------------
# pfd_act_f16
# ------------------------------------------------------------------------------------------------
def half_ulp_f16(ref64):
    """half an fp16 ulp of each value: 2^(e - 11) for 2^e <= |ref| < 2^(e + 1), 2^-25 where |ref| < 2^-14 (subnormal)"""
    mag = ref64.double().abs()
    _, ex = torch.frexp(mag)                                       # |ref| = m 2^ex, m in [0.5, 1)
    hu = torch.ldexp(torch.ones_like(mag), (ex - 12).clamp_min(-25))
    return torch.where(mag < 2.0 ** -14, torch.full_like(mag, 2.0 ** -25), hu)


def act_bound(ref64, act):
    """the largest |got - ref| allowed per element, ref the fp64 value of kernel_refs.activation_ref:
      none  0: the bits of the input (act_violations compares bits)
      ReLU  0: equal as numbers; fmaxf does not fix the sign of a zero, so -0 may come out as either zero, everything else
            bit for bit (act_violations)
      SiLU  hu + 2^-20 |ref|: eight fp32 ulps for one rcp, one exp2 and two products, no absolute term
      GELU  hu + 5e-7: the figure is the source's own claim in csrc/pfd_common.h
    hu = half_ulp_f16(ref), the one rounding of the result to fp16."""
    ref64 = ref64.double()
    if act in (ACT_NONE, ACT_RELU):
        return torch.zeros_like(ref64)
    hu = half_ulp_f16(ref64)
    return hu + (2.0 ** -20 * ref64.abs() if act == ACT_SILU else 5e-7)


def act_violations(got, x, act):
    """got = the fp16 output for the fp16 input x -> (mask of the elements outside act_bound, error / bound per element
    where the bound is not zero).  A NaN or an infinity out of a finite input is a violation."""
    got, x = got.detach().cpu(), x.detach().cpu()
    assert got.dtype == torch.float16 and got.shape == x.shape
    ref = KR.activation_ref(x, act)
    if act == ACT_NONE:
        return bits_of(got) != bits_of(x), None
    if act == ACT_RELU:
        want = torch.relu(x)                                          # +0 for every negative input and for -0
        bad = bits_of(got) != bits_of(want)
        neg_zero = bits_of(x) == 0x8000
        bad = torch.where(neg_zero, got.double() != 0.0, bad)
        return bad, None
    bound = act_bound(ref, act)
    err = (got.double() - ref).abs()
    bad = ~(err <= bound)                                             # NaN -> violation
    return bad, err / bound


def _mut_gelu_tanh(x):
    return F.gelu(x.double(), approximate="tanh")


def _mut_silu_1702(x):
    return x.double() * torch.sigmoid(1.702 * x.double())


# name -> (the activation whose bound it must violate, the wrong fp64 formula)
ACT_MUTANTS = {"gelu_tanh": (ACT_GELU, _mut_gelu_tanh), "silu_1702": (ACT_SILU, _mut_silu_1702)}


def _f32(v):
    return np.asarray(v, dtype=np.float32)


def _fma32(a, b, c):
    """fmaf on float32 arrays: the product of two float32 is exact in float64; one more rounding to float32"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _exp2_32(v):
    return np.exp2(v.astype(np.float64)).astype(np.float32)


def gelu_form32(x):
    """pfd_gelu of csrc/pfd_common.h as written, in numpy float32, with a correctly rounded 1 / x and exp2 in place of the
    hardware's: what the FORMULA costs, before the two instructions add their error.  x: fp16 tensor -> float32 ndarray"""
    x = x.float().numpy()
    with np.errstate(over="ignore", invalid="ignore"):
        z = np.abs(x) * _f32(0.70710678118654752440)
        t = _f32(1.0) / _fma32(_f32(0.3275911), z, _f32(1.0))
        poly = _fma32(t, _f32(1.061405429), _f32(-1.453152027))
        poly = _fma32(t, poly, _f32(1.421413741))
        poly = _fma32(t, poly, _f32(-0.284496736))
        poly = _fma32(t, poly, _f32(0.254829592))
        half_erfc = _f32(0.5) * t * poly * _exp2_32(_f32(-1.4426950408889634) * z * z)
        return x * np.where(x >= 0, _f32(1.0) - half_erfc, half_erfc)


def silu_form32(x):
    """pfd_silu as written, the same way"""
    x = x.float().numpy()
    with np.errstate(over="ignore"):
        return x * (_f32(1.0) / (_f32(1.0) + _exp2_32(_f32(-1.4426950408889634) * x)))


# ------------------------------------------------------------------------------------------------
# cases past the grid: the smallest of each kernel whose element count exceeds GRID_CAP
# ------------------------------------------------------------------------------------------------
TO_NHWC_PAST_GRID = (1, 3, 592, 592)                                  # 1 051 392 elements; mul = 1, add = 0
IM2COL_PAST_GRID = dict(shape=(1, 130, 130, 3), ks=3, stride=1, pad=1, kpad=64)      # 130 * 130 * 64 = 1 081 600
ADD_ROWVEC_PAST_GRID = (6554, 1280)                                   # 6554 * 160 = 1 048 640 vectors
IMAGE_U8_PAST_GRID = 8 * 256 * 4096 + 13                              # the SIZES[-1] of test_encoder_kernels_gpu.py
IMAGE_U8_SIZES = (1, 7, 8, 9, 2049, IMAGE_U8_PAST_GRID)

assert TO_NHWC_PAST_GRID[1] * TO_NHWC_PAST_GRID[2] * TO_NHWC_PAST_GRID[3] == 1051392 > GRID_CAP
assert 130 * 130 * 64 == 1081600 > GRID_CAP and ADD_ROWVEC_PAST_GRID[0] * (ADD_ROWVEC_PAST_GRID[1] // 8) == 1048640 > GRID_CAP
assert (ADD_ROWVEC_PAST_GRID[0] - 1) * (ADD_ROWVEC_PAST_GRID[1] // 8) <= GRID_CAP and IMAGE_U8_PAST_GRID // 8 + 1 > GRID_CAP


def image_u8_operand(n):
    """n fp16 values for pfd_image_u8_f16: the non-NaN patterns over and over (so every size holds every kind of input its
    length allows), started at an offset that depends on n"""
    x = all_f16("non_nan")
    idx = (torch.arange(n, dtype=torch.int64) + 7919 * (n % 13)) % x.numel()
    return x[idx]


# ------------------------------------------------------------------------------------------------
# the shapes of the aliasing / bad-argument cases on the emulation and the device
# ------------------------------------------------------------------------------------------------
ROW_SHAPES = ((5, 160), (3, 320))


def row_operands(R, C, seed):
    """x [R, C], b [R, C], v [C] fp16 (CPU): unit Gaussians with a mean, so that sums round"""
    g = torch.Generator().manual_seed(1000 * R + C + seed)
    return ((torch.randn((R, C), generator=g) + 0.3).half(), torch.randn((R, C), generator=g).half(),
            torch.randn((C,), generator=g).half())
