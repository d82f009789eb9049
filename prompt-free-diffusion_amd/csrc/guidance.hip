// Guidance rescale (lib/guidance.py is the same specification in fp64 on the host): Lin et al. 2023, "Common
// Diffusion Noise Schedules and Sample Steps are Flawed", section 3.4.  For sample b of a CFG batch, with eu / ec its
// unconditional / conditional eps (f16, n elements each), s its guidance scale and phi in [0, 1]:
//   g      = fl32(fma(s, fl32(ec - eu), eu))               the guided eps exactly as guided_eps of step.hip rounds it
//   mul[b] = phi * std(ec) / std(g) + (1 - phi)            std over the n elements of the sample, mean removed
// The step kernel then multiplies its guided eps by mul[b] (StepArgs::eps_mul, pfd_cfg_step_mul).
//
// ONE block of kThreads threads per sample; no workspace, no atomics, nothing read back.  OWNERSHIP: the sample is cut into
// groups of 8 consecutive elements (the last one short when n % 8 != 0); thread t owns the groups t, t + kThreads, ... and
// adds their elements in ascending order into ONE serial fp32 sum per statistic.  The 64 sums of a wave meet in wave_sum (six
// butterfly levels, every lane ends with the same bits), the kWaves wave sums in LDS, where every thread adds them in the
// same fixed tree (four levels).  Two sweeps: the sums of ec and g, then -- with the two means -- the sums of the squared
// deviations (the second sweep reads L2).  The count cancels in std(ec) / std(g): the ratio is sqrt(q_c / q_g).
//
// What the bits of mul[b] depend on: the sample's data, s, phi and n -- not B, not the grid (one block per sample whatever
// B is), not the alignment: a base that is not 16-byte aligned, or n % 8 != 0, reads the same groups element by element
// (VEC = false) and adds them in the same order.
// A sample whose phi is exactly 0 writes 1.0f and reads nothing of its eps; that branch, like q_g == 0, is uniform over
// the block, and every thread of a block that passes it reaches both barriers.
//
// The whole file is compiled with floating-point contraction OFF: every rounding is written out.
#include "pfd_common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / PFD_WAVE;
static_assert(kWaves == 16, "block_sum2 adds sixteen wave sums");

// the guided eps of an element: guided_eps of step.hip at nb = 2
__device__ __forceinline__ float guided(float eu, float ec, float s) { return __builtin_fmaf(s, ec - eu, eu); }

// the 8 (or, in the sample's last group, `cnt`) elements at element offset `at` of p, as floats; absent ones are not read
template <bool VEC>
__device__ __forceinline__ void load_group(const half_t* p, long at, int cnt, float v[8]) {
  if (VEC) {
    Pack16 k;
    k.u = *reinterpret_cast<const uint4*>(p + at);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = (float)k.e[j];
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = j < cnt ? (float)p[at + j] : 0.f;
  }
}

// two block sums at once: wave_sum, one LDS slot per wave, then the same fixed tree in every thread -- one barrier
__device__ __forceinline__ void block_sum2(float& a, float& b, float (*slot)[2]) {
  a = wave_sum(a);
  b = wave_sum(b);
  if ((threadIdx.x & (PFD_WAVE - 1)) == 0) {
    slot[threadIdx.x / PFD_WAVE][0] = a;
    slot[threadIdx.x / PFD_WAVE][1] = b;
  }
  __syncthreads();
  float r[2];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    float t[kWaves];
#pragma unroll
    for (int i = 0; i < kWaves; ++i) t[i] = slot[i][k];
#pragma unroll
    for (int o = kWaves / 2; o > 0; o >>= 1)
#pragma unroll
      for (int i = 0; i < o; ++i) t[i] = t[i] + t[i + o];
    r[k] = t[0];
  }
  a = r[0];
  b = r[1];
}

template <bool VEC>
__global__ __launch_bounds__(kThreads) void guidance_rescale_kernel(const half_t* eps, const float* scale, long scale_stride,
                                                                    const float* phi, long phi_stride, float* mul, long n) {
  __shared__ float sums[kWaves][2];     // first sweep
  __shared__ float sqs[kWaves][2];      // second sweep (its own slots: no barrier between the sweeps' uses)
  const long b = blockIdx.x, B = gridDim.x;
  const float ph = phi[b * phi_stride];
  if (ph == 0.f) {                      // uniform over the block: nothing of this sample's eps is read
    if (threadIdx.x == 0) mul[b] = 1.0f;
    return;
  }
  const float s = scale[b * scale_stride];
  const half_t* pu = eps + b * n;
  const half_t* pc = eps + (B + b) * n;
  const long groups = (n + 7) >> 3;
  float sum_c = 0.f, sum_g = 0.f;
  for (long g = threadIdx.x; g < groups; g += kThreads) {
    const long at = g << 3;
    const int cnt = n - at < 8 ? (int)(n - at) : 8;
    float u[8], c[8];
    load_group<VEC>(pu, at, cnt, u);
    load_group<VEC>(pc, at, cnt, c);
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (VEC || j < cnt) {
        sum_c = sum_c + c[j];
        sum_g = sum_g + guided(u[j], c[j], s);
      }
  }
  block_sum2(sum_c, sum_g, sums);
  const float fn = (float)n;
  const float mean_c = sum_c / fn, mean_g = sum_g / fn;
  float q_c = 0.f, q_g = 0.f;
  for (long g = threadIdx.x; g < groups; g += kThreads) {
    const long at = g << 3;
    const int cnt = n - at < 8 ? (int)(n - at) : 8;
    float u[8], c[8];
    load_group<VEC>(pu, at, cnt, u);
    load_group<VEC>(pc, at, cnt, c);
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (VEC || j < cnt) {
        const float dc = c[j] - mean_c;
        const float dg = guided(u[j], c[j], s) - mean_g;
        q_c = __builtin_fmaf(dc, dc, q_c);
        q_g = __builtin_fmaf(dg, dg, q_g);
      }
  }
  block_sum2(q_c, q_g, sqs);
  if (threadIdx.x == 0) {
    // q_g == 0 (a constant guided eps): the factor is 1; else one division, one square root, one fma
    mul[b] = q_g == 0.f ? 1.0f : __builtin_fmaf(ph, sqrtf(q_c / q_g), 1.0f - ph);
  }
}

int bad_args(int code, const char* msg) {
  pfd_set_error(msg);
  return code;
}

}  // namespace

extern "C" int pfd_guidance_rescale_f32(const void* eps, const float* scale, int32_t scale_stride, const float* phi,
                                        int32_t phi_stride, float* mul, int32_t B, int64_t n, pfd_stream_t stream) {
  if (!eps || !scale || !phi || !mul) return bad_args(PFD_EINVAL, "pfd_guidance_rescale_f32: eps, scale, phi and mul must not be NULL");
  if (B <= 0 || n <= 0 || scale_stride < 0 || phi_stride < 0)
    return bad_args(PFD_EINVAL, "pfd_guidance_rescale_f32: B and n must be positive, the strides not negative");
  hipStream_t s = (hipStream_t)stream;
  PfdProfScope prof_scope(15, 0.0, 0.0, s);
  // (n % 8 == 0 and an aligned base: every sample's base is aligned, both halves)
  if (n % 8 == 0 && aligned16(eps))
    hipLaunchKernelGGL((guidance_rescale_kernel<true>), dim3((unsigned)B), dim3(kThreads), 0, s, (const half_t*)eps, scale,
                       (long)scale_stride, phi, (long)phi_stride, mul, (long)n);
  else
    hipLaunchKernelGGL((guidance_rescale_kernel<false>), dim3((unsigned)B), dim3(kThreads), 0, s, (const half_t*)eps, scale,
                       (long)scale_stride, phi, (long)phi_stride, mul, (long)n);
  return pfd_check_launch("pfd_guidance_rescale_f32");
}
