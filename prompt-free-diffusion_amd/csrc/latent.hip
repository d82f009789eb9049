// The seeded latent start of an image-to-image request (lib/img2img.py is the same function in fp64 on
// the host): the VAE posterior's sample (distributions.py:24-62), its scaling (pfd.py vae_encode) and the forward
// noising q(x_t | x_0) (pfd.py:204-207, the x0 branch of ddim.py:213-219) in ONE launch, straight from the f16 NHWC
// moments the quant_conv GEMM leaves behind -- no NCHW copy of the moments, no noise tensors, no generator state:
//
//   std = exp(0.5 * clamp(logvar, -30, 20));  x0 = scale_factor * (mean + posterior_mul * std * z_p)
//   x_t = sqrt(a_t) * x0 + sqrt(1 - a_t) * z_q
//
// z_q / z_p of element e = (c*h + y)*w + x of sample key[b] = (seed, sample_id) are the counter-based normals of
// philox.h at step 0 in streams 1 / 2, so a sample's start is a function of its key and its picture only.
#include "pfd_common.h"
#include "philox.h"

namespace {

// One thread = four consecutive NCHW elements of ONE sample = one Philox call per stream.  VEC (C*h*w % 4 == 0, 16-byte
// aligned outputs): 16-byte stores; otherwise scalar stores, the tail of a sample's last quad dropped.  The moments are
// gathered element by element (NHWC: 2C halves per pixel, the mean of channel c at [c], its logvar at [C + c]); with
// `bcast` one picture's moments serve every sample.
template <bool VEC>
__global__ __launch_bounds__(256) void latent_start_kernel(const half_t* __restrict__ mom, int bcast,
                                                           const int64_t* __restrict__ key, float sf, float sq_at,
                                                           float sq_1mat, float pmul, float* __restrict__ x0,
                                                           float* __restrict__ xt, int B, int C, int h, int w) {
  const long hw = (long)h * w;
  const long ns = (long)C * hw;
  const long nq = (ns + 3) >> 2;
  const long total = (long)B * nq;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int b = (int)(i / nq);
    const long q = i - (long)b * nq;
    const long e0 = q * 4;
    const long base = (long)b * ns + e0;
    const half_t* mb = mom + (bcast ? 0 : (long)b * hw * 2 * C);
    const int64_t seed = key[2 * b], sid = key[2 * b + 1];
    float zq[4], zp[4], v0[4], vt[4];
    pfd_philox_normal4(seed, sid, 0, (uint32_t)q, PFD_STREAM_Q, zq);
    pfd_philox_normal4(seed, sid, 0, (uint32_t)q, PFD_STREAM_POSTERIOR, zp);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      v0[j] = vt[j] = 0.f;
      if (!VEC && e0 + j >= ns) continue;
      const long el = e0 + j;       // (c*h + y)*w + x inside the sample
      const int c = (int)(el / hw);
      const long pix = el - (long)c * hw;
      const half_t* m = mb + pix * 2 * C + c;
      const float mean = (float)m[0];
      const float lv = fminf(fmaxf((float)m[C], -30.0f), 20.0f);
      const float sd = expf(0.5f * lv);
      const float s0 = sf * (mean + (pmul * sd) * zp[j]);
      v0[j] = s0;
      vt[j] = sq_at * s0 + sq_1mat * zq[j];
    }
    if (VEC) {
      *reinterpret_cast<float4*>(xt + base) = make_float4(vt[0], vt[1], vt[2], vt[3]);
      if (x0) *reinterpret_cast<float4*>(x0 + base) = make_float4(v0[0], v0[1], v0[2], v0[3]);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (e0 + j < ns) {
          xt[base + j] = vt[j];
          if (x0) x0[base + j] = v0[j];
        }
    }
  }
}

// 1024 blocks of 256 threads = four per CU of a 256-CU part; a larger start walks the grid-stride loop
constexpr long kMaxBlocks = 1024;

}  // namespace

extern "C" int pfd_latent_start(const void* moments, int32_t Bm, const int64_t* key, float scale_factor, float sq_at,
                                float sq_1mat, float posterior_mul, float* x0, float* xt, int32_t B, int32_t C, int32_t h,
                                int32_t w, pfd_stream_t stream) {
  if (!moments || !key || !xt) {
    pfd_set_error("pfd_latent_start: moments, key and xt must not be NULL");
    return PFD_EINVAL;
  }
  if (B <= 0 || C <= 0 || h <= 0 || w <= 0) {
    pfd_set_error("pfd_latent_start: B, C, h, w must be positive");
    return PFD_EINVAL;
  }
  if (Bm != 1 && Bm != B) {
    pfd_set_error("pfd_latent_start: Bm must be 1 (one picture for all samples) or B");
    return PFD_EINVAL;
  }
  const long ns = (long)C * h * w;
  if (ns > ((long)1 << 34)) {   // the quad index is one 32-bit counter word
    pfd_set_error("pfd_latent_start: more than 2^34 elements per sample");
    return PFD_ESHAPE;
  }
  const long nq = (ns + 3) >> 2;
  long grid = ((long)B * nq + 255) / 256;
  if (grid > kMaxBlocks) grid = kMaxBlocks;
  const bool vec = !(ns & 3) && aligned16(xt) && (!x0 || aligned16(x0));
  PfdProfScope prof_scope(15, 0.0, 0.0, (hipStream_t)stream);
  if (vec)
    hipLaunchKernelGGL(latent_start_kernel<true>, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream,
                       (const half_t*)moments, Bm == 1 && B > 1 ? 1 : 0, key, scale_factor, sq_at, sq_1mat, posterior_mul,
                       x0, xt, B, C, h, w);
  else
    hipLaunchKernelGGL(latent_start_kernel<false>, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream,
                       (const half_t*)moments, Bm == 1 && B > 1 ? 1 : 0, key, scale_factor, sq_at, sq_1mat, posterior_mul,
                       x0, xt, B, C, h, w);
  return pfd_check_launch("pfd_latent_start");
}
