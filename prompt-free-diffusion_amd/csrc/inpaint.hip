// Masked regeneration (inpainting; lib/inpaint.py is the same specification in fp64 on the host):
//   * cfg_masked_kernel: the fused CFG + sampler step (DDIM or DPM-Solver++) with the blend that keeps the unmasked
//     region on the init picture's trajectory, in ONE launch per step like the unmasked kernels -- no noise tensor, no
//     generator state, so a masked loop is captured as a hipGraph and a sample's result depends on its key row alone;
//   * mask_grid_kernel: a uint8 mask of any size -> the binary grid at latent or pixel resolution (dilating);
//   * composite_kernel: decoded pixels inside the selection, the init picture's bytes outside.
#include "pfd_common.h"
#include "philox.h"
#include "step_common.h"

namespace {

constexpr int kSolverDdim = 0, kSolverDpmpp = 1;

// One thread = four consecutive NCHW elements of ONE sample = one Philox call per stream in use (the decode of
// cfg_ddim_rng_kernel).  For element e of sample b:
//   xp    = the unmasked update: SOLVER 0 the DDIM step of cfg_ddim_kernel / cfg_ddim_rng_kernel (the seeded stream-0
//           noise when sigma != 0), SOLVER 1 the DPM-Solver++ step of cfg_dpmpp_kernel -- the shared functions of
//           step_common.h and the unmasked kernels' rounding, so mask = 1 gives the unmasked kernels' bits
//   known = ksq * x0_keep[e] + ks * z_keep,  z_keep the stream-3 normal of (key[b], step, e)
//   x_out = m * xp + (1 - m) * known,  m = mask[b or 0, y, x]
// pred_x0 is the unmasked one; the next UNet input is half(x_out).  sigma == 0 and ks == 0 skip their Philox call on a
// branch that is uniform over the launch.  VEC (w % 4 == 0, 16-byte aligned x / x_out / pred_x0 / x0_keep / x0_prev):
// 16-byte accesses; otherwise the scalar path computes the same values.  PS: scale_ps[b] in place of the row's scale.
template <bool VEC, int SOLVER, bool PS>
__global__ __launch_bounds__(256) void cfg_masked_kernel(
    const half_t* __restrict__ eps, int nb, const float* __restrict__ x, const float* __restrict__ x0_prev,
    const int64_t* __restrict__ key, int step, float noise_mul, const float* __restrict__ coef,
    const float* __restrict__ scale_ps, const float* __restrict__ x0_keep, const float* __restrict__ mask, int mask_bcast,
    float ksq, float ks, float* __restrict__ x_out, float* __restrict__ pred_x0, half_t* __restrict__ xin_next, int rep,
    int B, int C, int h, int w) {
  const long hw = (long)h * w;
  const long ns = (long)C * hw;
  const long n = (long)B * ns;
  const long nq = (ns + 3) >> 2;
  const long total = (long)B * nq;
  // DDIM: the row {a_t, a_prev, sigma, sqrt(1-a_t), scale}; DPM-Solver++: {a_t, sqrt(1-a_t), c_x, c_d, w_cur, w_prev, scale, 0}
  const DdimStep k(coef);   // (read as a DDIM row; only its fields are used under SOLVER 0)
  const float a_t = coef[0], s1mat = coef[1], c_x = coef[2], c_d = coef[3];
  const float w_cur = x0_prev ? coef[4] : 1.f, w_prev = x0_prev ? coef[5] : 0.f;
  const float isq_at = 1.0f / sqrtf(a_t);
  const float scale_all = PS ? 0.f : coef[SOLVER == kSolverDdim ? 4 : 6];
  const bool step_noise = SOLVER == kSolverDdim && k.sigma != 0.f;
  const bool keep_noise = ks != 0.f;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int b = (int)(i / nq);
    const long q = i - (long)b * nq;
    const long e0 = q * 4;
    const long base = (long)b * ns + e0;
    const float scale = PS ? scale_ps[b] : scale_all;
    const float* mb = mask + (mask_bcast ? 0 : (long)b * hw);
    float z[4] = {0.f, 0.f, 0.f, 0.f}, zk[4] = {0.f, 0.f, 0.f, 0.f}, xv[4], kv[4], hv[4] = {0.f, 0.f, 0.f, 0.f}, xo4[4], p04[4];
    if (step_noise) pfd_philox_normal4(key[2 * b], key[2 * b + 1], step, (uint32_t)q, PFD_STREAM_STEP, z);
    if (keep_noise) pfd_philox_normal4(key[2 * b], key[2 * b + 1], step, (uint32_t)q, PFD_STREAM_KEEP, zk);
    if (VEC) {
      const float4 v = *reinterpret_cast<const float4*>(x + base);
      xv[0] = v.x; xv[1] = v.y; xv[2] = v.z; xv[3] = v.w;
      const float4 u = *reinterpret_cast<const float4*>(x0_keep + base);
      kv[0] = u.x; kv[1] = u.y; kv[2] = u.z; kv[3] = u.w;
      if (SOLVER == kSolverDpmpp && x0_prev) {
        const float4 t = *reinterpret_cast<const float4*>(x0_prev + base);
        hv[0] = t.x; hv[1] = t.y; hv[2] = t.z; hv[3] = t.w;
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool in = e0 + j < ns;
        xv[j] = in ? x[base + j] : 0.f;
        kv[j] = in ? x0_keep[base + j] : 0.f;
        if (SOLVER == kSolverDpmpp && x0_prev) hv[j] = in ? x0_prev[base + j] : 0.f;
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      xo4[j] = p04[j] = 0.f;
      if (!VEC && e0 + j >= ns) continue;
      const long el = e0 + j;   // (c*h + y)*w + x inside the sample
      const int xw = (int)(el % w);
      const long t = el / w;
      const int yh = (int)(t % h);
      const int c = (int)(t / h);
      const long ei = nhwc_index(b, c, yh, xw, C, h, w);
      const float e = guided_eps(eps, nb, n, ei, scale);
      float p0, xp;
      if (SOLVER == kSolverDdim) {
        p0 = pred_x0_of(xv[j], e, k.s1mat, k.isq_at);
        // DdimStep::update and the noise term, with the rounding of the unmasked kernel that serves the same request spelled
        // out (their one source expression compiles three ways): cfg_ddim_kernel sums two rounded products; the seeded
        // cfg_ddim_rng_kernel contracts dir * e onto the rounded sq_aprev * p0, then its 16-byte form contracts the noise
        // term too while its scalar form adds the rounded sigma * noise
        if (!step_noise) {
          xp = sum_of_products(k.sq_aprev, p0, k.dir, e);
        } else {
          const float nz = noise_mul * z[j];
          xp = __builtin_fmaf(k.dir, e, k.sq_aprev * p0);
          xp = VEC ? __builtin_fmaf(k.sigma, nz, xp) : add_rounded_product(xp, k.sigma, nz);
        }
      } else {
        p0 = pred_x0_of(xv[j], e, s1mat, isq_at);
        // cfg_dpmpp_kernel's rounding, spelled out: D is a sum of two rounded products, x_next one fma on the rounded c_d D
        float d = p0;
        if (x0_prev) d = sum_of_products(w_cur, p0, w_prev, hv[j]);
        xp = __builtin_fmaf(c_x, xv[j], c_d * d);
      }
      float known = ksq * kv[j];
      if (keep_noise) known = ksq * kv[j] + ks * zk[j];
      const float m = mb[(long)yh * w + xw];
      const float xo = m * xp + (1.0f - m) * known;
      xo4[j] = xo;
      p04[j] = p0;
      emit_next(xin_next, rep, n, ei, xo);
    }
    if (VEC) {
      *reinterpret_cast<float4*>(x_out + base) = make_float4(xo4[0], xo4[1], xo4[2], xo4[3]);
      *reinterpret_cast<float4*>(pred_x0 + base) = make_float4(p04[0], p04[1], p04[2], p04[3]);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (e0 + j < ns) {
          x_out[base + j] = xo4[j];
          pred_x0[base + j] = p04[j];
        }
    }
  }
}

// One output cell per thread; it loops over its footprint: rows lo = (y*Hm)/gh .. hi = max(lo + 1, ceil((y+1)*Hm/gh)),
// columns alike -- never empty, together covering the mask, so a marked pixel always lies in a marked cell.
template <bool F32>
__global__ __launch_bounds__(256) void mask_grid_kernel(const uint8_t* __restrict__ mask, void* __restrict__ out, int Bm,
                                                        int Hm, int Wm, int gh, int gw) {
  const long total = (long)Bm * gh * gw;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int gx = (int)(i % gw);
    const long t = i / gw;
    const int gy = (int)(t % gh);
    const int b = (int)(t / gh);
    const int y0 = (int)(((long)gy * Hm) / gh), x0 = (int)(((long)gx * Wm) / gw);
    const int y1 = max(y0 + 1, (int)((((long)gy + 1) * Hm + gh - 1) / gh));
    const int x1 = max(x0 + 1, (int)((((long)gx + 1) * Wm + gw - 1) / gw));
    const uint8_t* mb = mask + (long)b * Hm * Wm;
    int any = 0;
    for (int y = y0; y < y1 && !any; ++y)
      for (int xx = x0; xx < x1; ++xx)
        if (mb[(long)y * Wm + xx] >= 128) {
          any = 1;
          break;
        }
    if (F32) ((float*)out)[i] = any ? 1.0f : 0.0f;
    else ((uint8_t*)out)[i] = (uint8_t)any;
  }
}

// One pixel per thread: its C bytes from `decoded` where sel is set, from `init` elsewhere.
__global__ __launch_bounds__(256) void composite_kernel(const uint8_t* __restrict__ decoded, const uint8_t* __restrict__ init,
                                                        int init_bcast, const uint8_t* __restrict__ sel, int sel_bcast,
                                                        uint8_t* __restrict__ out, int n, long hw, int C) {
  const long total = (long)n * hw;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long b = i / hw;
    const long p = i - b * hw;
    const bool s = sel[(sel_bcast ? 0 : b * hw) + p] != 0;
    const uint8_t* src = s ? decoded + i * C : init + ((init_bcast ? 0 : b * hw) + p) * C;
    for (int c = 0; c < C; ++c) out[i * C + c] = src[c];
  }
}

constexpr int kMaxSide = 8192;   // the bound of the picture kernels (image.hip)

template <int SOLVER, bool PS>
void launch_masked(bool vec, int grid, hipStream_t stream, const half_t* eps, int nb, const float* x, const float* x0_prev,
                   const int64_t* key, int step, float noise_mul, const float* coef, const float* scale,
                   const float* x0_keep, const float* mask, int mask_bcast, float ksq, float ks, float* x_out,
                   float* pred_x0, half_t* xin_next, int rep, int B, int C, int h, int w) {
  if (vec)
    hipLaunchKernelGGL((cfg_masked_kernel<true, SOLVER, PS>), dim3(grid), dim3(256), 0, stream, eps, nb, x, x0_prev, key,
                       step, noise_mul, coef, scale, x0_keep, mask, mask_bcast, ksq, ks, x_out, pred_x0, xin_next, rep, B,
                       C, h, w);
  else
    hipLaunchKernelGGL((cfg_masked_kernel<false, SOLVER, PS>), dim3(grid), dim3(256), 0, stream, eps, nb, x, x0_prev, key,
                       step, noise_mul, coef, scale, x0_keep, mask, mask_bcast, ksq, ks, x_out, pred_x0, xin_next, rep, B,
                       C, h, w);
}

int refuse(int code, const char* msg) {
  pfd_set_error(msg);
  return code;
}

}  // namespace

extern "C" int pfd_cfg_step_masked(const void* eps, int32_t nb, const float* x, int32_t solver, const float* x0_prev,
                                   const int64_t* key, int32_t step, float noise_mul, const float* coef,
                                   const float* scale, const float* x0_keep, const float* mask, int32_t Bm, float ksq,
                                   float ks, float* x_out, float* pred_x0, void* xin_next, int32_t rep, int32_t B,
                                   int32_t C, int32_t h, int32_t w, pfd_stream_t stream) {
  if (!eps || !x || !key || !coef || !x0_keep || !mask || !x_out || !pred_x0)
    return refuse(PFD_EINVAL, "pfd_cfg_step_masked: eps, x, key, coef, x0_keep, mask, x_out and pred_x0 must not be NULL");
  if (solver != kSolverDdim && solver != kSolverDpmpp)
    return refuse(PFD_EINVAL, "pfd_cfg_step_masked: solver must be 0 (DDIM) or 1 (DPM-Solver++)");
  if (step < 0) return refuse(PFD_EINVAL, "pfd_cfg_step_masked: step must not be negative");
  if (!step_args_ok(nb, B, C, h, w, xin_next, rep))
    return refuse(PFD_EINVAL, "pfd_cfg_step_masked: nb in {1, 2}, positive B, C, h, w and rep in {1, 2} with xin_next");
  if (Bm != 1 && Bm != B) return refuse(PFD_EINVAL, "pfd_cfg_step_masked: Bm must be 1 (one mask for all samples) or B");
  if (x0_keep == x_out || x0_keep == pred_x0)
    return refuse(PFD_EINVAL, "pfd_cfg_step_masked: x0_keep must not alias x_out or pred_x0");
  if (x0_prev && (solver != kSolverDpmpp || x0_prev == x_out || x0_prev == pred_x0))
    return refuse(PFD_EINVAL, "pfd_cfg_step_masked: x0_prev goes with solver 1 and must not alias x_out or pred_x0");
  const long ns = (long)C * h * w;
  if (ns > ((long)1 << 34))   // the quad index is one 32-bit counter word
    return refuse(PFD_ESHAPE, "pfd_cfg_step_masked: more than 2^34 elements per sample");
  const long nq = (ns + 3) >> 2;
  const bool vec = quad_vec_ok(w, x, x_out, pred_x0) && aligned16(x0_keep) && (!x0_prev || aligned16(x0_prev));
  const int grid = grid_for((long)B * nq, 256);
  const int bcast = Bm == 1 && B > 1 ? 1 : 0;
  PfdProfScope prof_scope(15, 0.0, 0.0, (hipStream_t)stream);
#define PFD_MASKED(SOLVER, PS)                                                                                          \
  launch_masked<SOLVER, PS>(vec, grid, (hipStream_t)stream, (const half_t*)eps, nb, x, x0_prev, key, step, noise_mul,  \
                            coef, scale, x0_keep, mask, bcast, ksq, ks, x_out, pred_x0, (half_t*)xin_next, rep, B, C,  \
                            h, w)
  if (solver == kSolverDdim) {
    if (scale) PFD_MASKED(kSolverDdim, true);
    else PFD_MASKED(kSolverDdim, false);
  } else {
    if (scale) PFD_MASKED(kSolverDpmpp, true);
    else PFD_MASKED(kSolverDpmpp, false);
  }
#undef PFD_MASKED
  return pfd_check_launch("pfd_cfg_step_masked");
}

extern "C" int pfd_mask_grid_u8(const void* mask, int32_t Bm, int32_t Hm, int32_t Wm, void* out, int32_t out_f32,
                                int32_t gh, int32_t gw, pfd_stream_t stream) {
  if (!mask || !out) return refuse(PFD_EINVAL, "pfd_mask_grid_u8: mask and out must not be NULL");
  if (Bm <= 0 || Hm <= 0 || Wm <= 0 || gh <= 0 || gw <= 0)
    return refuse(PFD_EINVAL, "pfd_mask_grid_u8: Bm, Hm, Wm, gh, gw must be positive");
  if (Hm > kMaxSide || Wm > kMaxSide || gh > kMaxSide || gw > kMaxSide)
    return refuse(PFD_ESHAPE, "pfd_mask_grid_u8: sides up to 8192");
  const int grid = grid_for((long)Bm * gh * gw, 256);
  PfdProfScope prof_scope(15, 0.0, 0.0, (hipStream_t)stream);
  if (out_f32)
    hipLaunchKernelGGL(mask_grid_kernel<true>, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const uint8_t*)mask, out, Bm,
                       Hm, Wm, gh, gw);
  else
    hipLaunchKernelGGL(mask_grid_kernel<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const uint8_t*)mask, out, Bm,
                       Hm, Wm, gh, gw);
  return pfd_check_launch("pfd_mask_grid_u8");
}

extern "C" int pfd_composite_u8(const void* decoded, const void* init, int32_t Bi, const void* sel, int32_t Bs, void* out,
                                int32_t n, int32_t H, int32_t W, int32_t C, pfd_stream_t stream) {
  if (!decoded || !init || !sel || !out) return refuse(PFD_EINVAL, "pfd_composite_u8: decoded, init, sel and out must not be NULL");
  if (n <= 0 || H <= 0 || W <= 0 || C <= 0) return refuse(PFD_EINVAL, "pfd_composite_u8: n, H, W, C must be positive");
  if ((Bi != 1 && Bi != n) || (Bs != 1 && Bs != n))
    return refuse(PFD_EINVAL, "pfd_composite_u8: init and sel have leading dimension 1 or n");
  if (H > kMaxSide || W > kMaxSide || C > 4) return refuse(PFD_ESHAPE, "pfd_composite_u8: sides up to 8192, at most 4 channels");
  if (out == decoded || out == init || out == sel)
    return refuse(PFD_EINVAL, "pfd_composite_u8: out must not alias decoded, init or sel");
  const long hw = (long)H * W;
  PfdProfScope prof_scope(15, 0.0, 0.0, (hipStream_t)stream);
  hipLaunchKernelGGL(composite_kernel, dim3(grid_for((long)n * hw, 256)), dim3(256), 0, (hipStream_t)stream,
                     (const uint8_t*)decoded, (const uint8_t*)init, Bi == 1 && n > 1 ? 1 : 0, (const uint8_t*)sel,
                     Bs == 1 && n > 1 ? 1 : 0, (uint8_t*)out, n, hw, C);
  return pfd_check_launch("pfd_composite_u8");
}
