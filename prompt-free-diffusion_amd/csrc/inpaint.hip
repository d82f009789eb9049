// Masked regeneration (inpainting; lib/inpaint.py is the same specification in fp64 on the host) around the
// sampler's loop -- the masked step itself, pfd_cfg_step_masked, is the MASKED form of the one step kernel (step.hip):
//   * mask_grid_kernel: a uint8 mask of any size -> the binary grid at latent or pixel resolution (dilating);
//   * composite_kernel: decoded pixels inside the selection, the init picture's bytes outside.
#include "pfd_common.h"

namespace {

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

int refuse(int code, const char* msg) {
  pfd_set_error(msg);
  return code;
}

}  // namespace

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
