// ControlNet strength (lib/control.py is the same specification in fp64 on the host): the add of a
// ControlNet residual into the UNet with one fp32 scale per sample,
//   y[b, e] = (half) fmaf(scale[b * scale_stride], (float) r[b, e], (float) x[b, e]).
// Streaming and memory-bound.  The sample index comes from the grid (blockIdx.y), the scale is read once per block and is
// block-uniform: a sample whose scale is exactly 0 copies x and never touches r (the unconditional half of a
// cond-only request: a third of the traffic saved).  At scale 1.0f the result is bit for bit add_kernel's
// (elementwise.hip): fmaf(1, r, x) and x + r round the same exact sum once.
// y may be x or r: a lane reads both of its 16-byte operands before it writes, and no other lane touches them -- hence
// no __restrict__ on the three pointers.  Plain stores: the next kernel reads y.
#include "pfd_common.h"

namespace {

__global__ __launch_bounds__(256) void add_scaled_rows_kernel(const half_t* x, const half_t* r,
                                                              const float* __restrict__ scale, long scale_stride, half_t* y,
                                                              long nv) {
  const long b = blockIdx.y;
  const uint4* xv = reinterpret_cast<const uint4*>(x) + b * nv;
  const uint4* rv = reinterpret_cast<const uint4*>(r) + b * nv;
  uint4* yv = reinterpret_cast<uint4*>(y) + b * nv;
  const long stride = (long)gridDim.x * blockDim.x;
  long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nv) return;
  // x is needed whatever the scale is: its first load is in flight while the scale arrives; r waits for the branch
  Pack16 p;
  p.u = xv[i];
  const float s = scale[b * scale_stride];
  if (s == 0.0f) {
    if (xv == yv) return;      // in place on x: nothing to do
    for (;;) {
      yv[i] = p.u;
      i += stride;
      if (i >= nv) return;
      p.u = xv[i];
    }
  }
  for (;;) {
    Pack16 q, o;
    q.u = rv[i];
#pragma unroll
    for (int e = 0; e < 8; ++e) o.e[e] = (half_t)fmaf(s, (float)q.e[e], (float)p.e[e]);
    yv[i] = o.u;
    i += stride;
    if (i >= nv) return;
    p.u = xv[i];
  }
}

int refuse(int code, const char* msg) {
  pfd_set_error(msg);
  return code;
}

}  // namespace

extern "C" int pfd_add_scaled_rows_f16(const void* x, const void* r, const float* scale, int64_t scale_stride, void* y,
                                       int32_t B, int64_t n_per_sample, pfd_stream_t stream) {
  if (!x || !r || !scale || !y) return refuse(PFD_EINVAL, "pfd_add_scaled_rows_f16: x, r, scale and y must not be NULL");
  if (B < 1 || scale_stride < 1 || n_per_sample < 1)
    return refuse(PFD_EINVAL, "pfd_add_scaled_rows_f16: B, scale_stride and n_per_sample must be positive");
  if (n_per_sample % 8 != 0 || !aligned16(x) || !aligned16(r) || !aligned16(y))
    return refuse(PFD_ESHAPE, "pfd_add_scaled_rows_f16: n_per_sample must be a multiple of 8 and x, r, y 16-byte aligned");
  if (B > 65535) return refuse(PFD_ESHAPE, "pfd_add_scaled_rows_f16: at most 65535 samples");
  if (reinterpret_cast<uintptr_t>(scale) & 3) return refuse(PFD_EINVAL, "pfd_add_scaled_rows_f16: scale must be 4-byte aligned");
  const long nv = (long)(n_per_sample / 8);
  // at most 4096 blocks over the launch (grid_for's cap), every block of a sample the same number of rounds
  long per_sample = 4096 / B;
  if (per_sample < 1) per_sample = 1;
  long gx = (nv + 255) / 256;
  if (gx > per_sample) {
    const long rounds = (gx + per_sample - 1) / per_sample;
    gx = (gx + rounds - 1) / rounds;
  }
  PfdProfScope prof_scope(15, 0.0, 0.0, (hipStream_t)stream);
  hipLaunchKernelGGL(add_scaled_rows_kernel, dim3((unsigned)gx, (unsigned)B), dim3(256), 0, (hipStream_t)stream,
                     (const half_t*)x, (const half_t*)r, scale, (long)scale_stride, (half_t*)y, nv);
  return pfd_check_launch("pfd_add_scaled_rows_f16");
}
