// What the fused CFG + sampler step kernels share (elementwise.hip: cfg_ddim_kernel, cfg_dpmpp_kernel,
// cfg_ddim_rng_kernel; inpaint.hip: cfg_masked_kernel): ONE copy of what they compute per element -- the guided eps,
// pred_x0 and the emit of the next UNet input -- and of what their entry points check alike.  That the kernels agree
// bit for bit on these is a property of the functions below.  Each kernel keeps its own decode of the thread index.
#pragma once
#include "pfd_common.h"

namespace {

// NHWC index of element (b, c, yh, xw) of an NCHW [B, C, h, w] tensor
__device__ __forceinline__ long nhwc_index(int b, int c, int yh, int xw, int C, int h, int w) {
  return (((long)b * h + yh) * w + xw) * C + c;
}

// the guided eps of the element at NHWC index ei: eps holds nb batches of n elements, unconditional first
__device__ __forceinline__ float guided_eps(const half_t* __restrict__ eps, int nb, long n, long ei, float scale) {
  if (nb == 2) {
    const float eu = (float)eps[ei];
    const float ec = (float)eps[n + ei];
    return eu + scale * (ec - eu);
  }
  return (float)eps[ei] * scale;
}

__device__ __forceinline__ float pred_x0_of(float xv, float e, float s1mat, float isq_at) {
  return (xv - s1mat * e) * isq_at;
}

// `rep` fp16 copies of the next UNet input at NHWC index ei (nothing without xin_next)
__device__ __forceinline__ void emit_next(half_t* __restrict__ xin_next, int rep, long n, long ei, float v) {
  if (xin_next) {
    const half_t hv = (half_t)v;
    for (int r = 0; r < rep; ++r) xin_next[(long)r * n + ei] = hv;
  }
}

// Sums of products with the rounding spelled out.  Under the default contraction a sum of two products has two ways to
// become an fma, and which one the compiler takes -- or neither -- depends on the kernel the expression is inlined into: the
// unmasked step kernels, compiled from one source expression, round it in three ways (see cfg_masked_kernel).  A kernel that
// has to reproduce the bits of another takes these.
// a*b + c*d, both products rounded before the sum
__device__ __forceinline__ float sum_of_products(float a, float b, float c, float d) {
#pragma clang fp contract(off)
  const float p = a * b, q = c * d;
  return p + q;
}
// x + a*b, the product rounded before the sum
__device__ __forceinline__ float add_rounded_product(float x, float a, float b) {
#pragma clang fp contract(off)
  const float p = a * b;
  return x + p;
}

// the per-step numbers of a DDIM row {a_t, a_prev, sigma_t, sqrt(1-a_t), guidance scale}
struct DdimStep {
  float sigma, s1mat, isq_at, sq_aprev, dir;
  __device__ __forceinline__ explicit DdimStep(const float* __restrict__ coef) {
    const float a_t = coef[0], a_prev = coef[1];
    sigma = coef[2];
    s1mat = coef[3];
    isq_at = 1.0f / sqrtf(a_t);
    sq_aprev = sqrtf(a_prev);
    dir = sqrtf(fmaxf(1.0f - a_prev - sigma * sigma, 0.f));
  }
  // x_prev without the noise term
  __device__ __forceinline__ float update(float p0, float e) const { return sq_aprev * p0 + dir * e; }
};

inline int grid_for(long n, int block) {
  long g = (n + block - 1) / block;
  if (g > 4096) g = 4096;
  if (g < 1) g = 1;
  return (int)g;
}

// what all step entry points check alike
inline bool step_args_ok(int nb, int B, int C, int h, int w, const void* xin_next, int rep) {
  return nb >= 1 && nb <= 2 && B > 0 && C > 0 && h > 0 && w > 0 && !(xin_next && (rep < 1 || rep > 2));
}

// a thread's quad is one 16-byte access of x / x_prev / pred_x0 (cfg_ddim_rng_kernel<VEC = true>)
inline bool quad_vec_ok(int w, const float* x, const float* x_prev, const float* pred_x0) {
  return !(w & 3) && !((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(x_prev) |
                        reinterpret_cast<uintptr_t>(pred_x0)) & 15);
}

}  // namespace
