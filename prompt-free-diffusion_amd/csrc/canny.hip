// Canny edge hints on the device: packed uint8 pictures [B, H, W, C] -> the edge map the reference's only non-neural
// annotator builds on the host, `cv2.Canny(img, low, high)` (controlnet_annotator/canny/__init__.py:5, behind
// ControlNet.preprocess, controlnet.py:332-360), as uint8 [B, H, W] or as the hint [B, 3, H, W] of `ToTensor` +
// `repeat(1, 3, 1, 1)` (controlnet.py:357-359).
//
// The algorithm is the numpy statement in lib/canny.py, to the byte: 3x3 Sobel on a replicated border, L1 magnitude, the
// channel with the largest magnitude (lowest index on a tie), non-maximum suppression in 15-bit fixed point
// (tan 22.5 = 13573 / 2^15) on magnitudes with a border of ZEROS, hysteresis over 8-connected candidates.  All integer.
// That statement restates OpenCV's published algorithm; its byte equality with cv2.Canny has not been measured.
//
// Four launches per call, whatever the picture holds:
//   1. canny_nms_kernel      tile + halo in LDS -> one state byte per pixel (0 | 1 weak | 2 strong); parent[i] = i
//   2. canny_link_kernel     union-find over the candidates: every candidate unites with its E, SW, S, SE candidate
//                            neighbours (atomicMin on the larger root, retried until both roots agree)
//   3. canny_resolve_kernel  every candidate is compressed to its root; a strong one marks strong[root]
//   4. canny_emit_kernel     edge = candidate whose root is marked
// The hysteresis is exact for any picture (a component is found whole, however it winds), needs no flag read by the
// host, and can be captured in a hipGraph.  Workgroups of one launch talk through relaxed agent-scope atomics on parent[]
// only; the kernel boundaries order everything else.  No MFMA, no inline assembly, no scratch (tests/test_canny_cpu.py).
#include "pfd_common.h"

namespace {

constexpr int kMaxSide = 4096;
constexpr int kTW = 64, kTH = 16;               // pixels of one tile
constexpr int kPW = kTW + 4, kPH = kTH + 4;     // staged picture: halo of two (Sobel of the magnitude halo)
constexpr int kMW = kTW + 2, kMH = kTH + 2;     // magnitudes: halo of one (the NMS neighbours)
constexpr int kMaxGrid = 1 << 20;               // tiles beyond that are walked by a grid-stride loop

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ int absi(int v) { return v < 0 ? -v : v; }

// ---- 1. Sobel + channel choice + non-maximum suppression -----------------------------------------------------------
template <int C>
__global__ __launch_bounds__(256) void canny_nms_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ states,
                                                        int* __restrict__ parent, uint8_t* __restrict__ strong, int H,
                                                        int W, int tiles_x, int tiles_y, long ntiles, int low, int high) {
  __shared__ uint8_t pix[kPH * kPW * C];
  __shared__ int mag[kMH][kMW];
  __shared__ int grad[kMH][kMW];                // the chosen channel's signed gx (low half) and gy (high half)
  const int tid = threadIdx.x;
  for (long t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int x0 = (int)(t % tiles_x) * kTW;
    const int y0 = (int)((t / tiles_x) % tiles_y) * kTH;
    const long b = t / ((long)tiles_x * tiles_y);
    const uint8_t* img = src + b * H * W * C;
    // every load is unconditional: the address is clamped to the picture, which IS the replicated border; threads past
    // the end of the staged block repeat its last pixel
    constexpr int NP = kPH * kPW;
#pragma unroll
    for (int k = 0; k < (NP + 255) / 256; ++k) {
      const int i = min(k * 256 + tid, NP - 1);
      const int py = clampi(y0 - 2 + i / kPW, 0, H - 1), px = clampi(x0 - 2 + i % kPW, 0, W - 1);
      const uint8_t* g = img + ((long)py * W + px) * C;
      uint8_t v[C];
#pragma unroll
      for (int c = 0; c < C; ++c) v[c] = g[c];
#pragma unroll
      for (int c = 0; c < C; ++c) pix[i * C + c] = v[c];
    }
    __syncthreads();
    for (int i = tid; i < kMH * kMW; i += 256) {
      const int r = i / kMW, c = i % kMW;       // pixel (y0 - 1 + r, x0 - 1 + c) = staged (r + 1, c + 1)
      int bm = -1, bx = 0, by = 0;
#pragma unroll
      for (int ch = 0; ch < C; ++ch) {
        auto a = [&](int dr, int dc) { return (int)pix[((r + 1 + dr) * kPW + (c + 1 + dc)) * C + ch]; };
        const int gx = (a(-1, 1) + 2 * a(0, 1) + a(1, 1)) - (a(-1, -1) + 2 * a(0, -1) + a(1, -1));
        const int gy = (a(1, -1) + 2 * a(1, 0) + a(1, 1)) - (a(-1, -1) + 2 * a(-1, 0) + a(-1, 1));
        const int m = absi(gx) + absi(gy);
        if (m > bm) {                           // strictly larger: the lowest channel keeps a tie
          bm = m;
          bx = gx;
          by = gy;
        }
      }
      const int y = y0 - 1 + r, x = x0 - 1 + c;
      mag[r][c] = (y >= 0 && y < H && x >= 0 && x < W) ? bm : 0;       // the suppression sees zeros outside the picture
      grad[r][c] = (int)(((unsigned)bx & 0xffffu) | ((unsigned)by << 16));
    }
    __syncthreads();
    for (int i = tid; i < kTW * kTH; i += 256) {
      const int r = i / kTW, c = i % kTW;
      const int y = y0 + r, x = x0 + c;
      if (y < H && x < W) {
        const int m = mag[r + 1][c + 1], g = grad[r + 1][c + 1];
        const int xs = (int)(int16_t)(g & 0xffff), ys = g >> 16;
        int state = 0;
        if (m > low) {
          const int ax = absi(xs), ay = absi(ys) << 15;
          const int t22 = ax * 13573, t67 = t22 + (ax << 16);
          bool keep;
          if (ay < t22) {
            keep = m > mag[r + 1][c] && m >= mag[r + 1][c + 2];
          } else if (ay > t67) {
            keep = m > mag[r][c + 1] && m >= mag[r + 2][c + 1];
          } else {
            const int s = (xs ^ ys) < 0 ? -1 : 1;
            keep = m > mag[r][c + 1 - s] && m > mag[r + 2][c + 1 + s];
          }
          state = keep ? (m > high ? 2 : 1) : 0;
        }
        const long idx = (b * H + y) * W + x;
        states[idx] = (uint8_t)state;
        parent[idx] = (int)idx;
        strong[idx] = 0;
      }
    }
    __syncthreads();                            // the next tile of this block restages the LDS
  }
}

// ---- 2. - 4. hysteresis: connected components of the candidates ----------------------------------------------------
// parent[i] <= i at all times and only ever decreases, so a walk towards the root ends, whoever else is linking.
__device__ __forceinline__ int uf_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ int uf_root(const int* parent, int i) {
  int p = uf_load(parent + i);
  while (p != i) {
    i = p;
    p = uf_load(parent + i);
  }
  return i;
}

__device__ __forceinline__ void uf_unite(int* parent, int a, int b) {
  for (;;) {
    a = uf_root(parent, a);
    b = uf_root(parent, b);
    if (a == b) return;
    if (a < b) {
      const int t = a;
      a = b;
      b = t;
    }
    // a is the larger root: hang it under b.  Somebody may have hung it elsewhere meanwhile (old != a): a now points to
    // the smaller of the two, and the other one still has to meet b
    const int old = __hip_atomic_fetch_min(parent + a, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (old == a) return;
    a = old;
  }
}

__global__ __launch_bounds__(256) void canny_link_kernel(const uint8_t* __restrict__ states, int* __restrict__ parent,
                                                         int H, int W, int total) {
  const long gl = (long)blockIdx.x * 256 + threadIdx.x;
  if (gl >= total) return;
  const int gid = (int)gl;
  const int rem = gid % (H * W), y = rem / W, x = rem % W;
  const long last = total - 1;
  // unconditional loads at clamped indices; what lies outside the picture is masked afterwards
  const int s = states[gid];
  const int e = states[min(gl + 1, last)], sw = states[min(gl + W - 1, last)], so = states[min(gl + W, last)],
            se = states[min(gl + W + 1, last)];
  if (!s) return;
  const bool right = x + 1 < W, down = y + 1 < H;
  if (right && e) uf_unite(parent, gid, gid + 1);
  if (down && x > 0 && sw) uf_unite(parent, gid, gid + W - 1);
  if (down && so) uf_unite(parent, gid, gid + W);
  if (down && right && se) uf_unite(parent, gid, gid + W + 1);
}

__global__ __launch_bounds__(256) void canny_resolve_kernel(const uint8_t* __restrict__ states, int* __restrict__ parent,
                                                            uint8_t* __restrict__ strong, int total) {
  const long gl = (long)blockIdx.x * 256 + threadIdx.x;
  if (gl >= total) return;
  const int gid = (int)gl;
  const int s = states[gid];
  if (!s) return;
  const int r = uf_root(parent, gid);
  // (another thread's walk through gid reads the old ancestor or the root: both lead to the root)
  __hip_atomic_store(parent + gid, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (s == 2) strong[r] = 1;
}

__global__ __launch_bounds__(256) void canny_emit_kernel(const uint8_t* __restrict__ states, const int* __restrict__ parent,
                                                         const uint8_t* __restrict__ strong, void* __restrict__ out,
                                                         int kind, int HW, int total) {
  const long gl = (long)blockIdx.x * 256 + threadIdx.x;
  if (gl >= total) return;
  const int gid = (int)gl;
  const int s = states[gid];
  const int root = clampi(parent[gid], 0, gid);     // a non-candidate is its own root
  const bool edge = s != 0 && strong[root] != 0;
  if (kind == PFD_IMG_U8) {
    reinterpret_cast<uint8_t*>(out)[gid] = edge ? 255 : 0;
  } else {
    const long o = (long)(gid / HW) * 3 * HW + gid % HW;
    if (kind == PFD_IMG_NCHW_F16) {
      const half_t v = edge ? (half_t)1.0f : (half_t)0.0f;
      half_t* p = reinterpret_cast<half_t*>(out) + o;
      p[0] = v;
      p[HW] = v;
      p[2 * (long)HW] = v;
    } else {
      const float v = edge ? 1.0f : 0.0f;
      float* p = reinterpret_cast<float*>(out) + o;
      p[0] = v;
      p[HW] = v;
      p[2 * (long)HW] = v;
    }
  }
}

int shape_error(const char* what) {
  pfd_set_error(what);
  return PFD_ESHAPE;
}

}  // namespace

extern "C" int pfd_canny_check(int32_t B, int32_t H, int32_t W, int32_t C) {
  if (B < 1 || (C != 1 && C != 3)) return shape_error("pfd_canny: B >= 1 and C in {1, 3}");
  if (H < 1 || H > kMaxSide || W < 1 || W > kMaxSide) return shape_error("pfd_canny: sides 1 ... 4096");
  if ((long)B * H * W >= (1L << 31)) return shape_error("pfd_canny: B * H * W must stay below 2^31 (int32 labels)");
  return PFD_OK;
}

extern "C" int pfd_canny_u8(const void* src, int32_t B, int32_t H, int32_t W, int32_t C, int32_t low, int32_t high,
                            void* states, void* parent, void* strong, void* out, int32_t out_kind, pfd_stream_t stream) {
  if (!src || !states || !parent || !strong || !out) return PFD_EINVAL;
  if (out_kind != PFD_IMG_U8 && out_kind != PFD_IMG_NCHW_F16 && out_kind != PFD_IMG_NCHW_F32) return PFD_EINVAL;
  if (const int rc = pfd_canny_check(B, H, W, C)) return rc;
  if (low > high) {
    const int32_t t = low;
    low = high;
    high = t;
  }
  const int total = (int)((long)B * H * W);
  const int tiles_x = (W + kTW - 1) / kTW, tiles_y = (H + kTH - 1) / kTH;
  const long ntiles = (long)B * tiles_x * tiles_y;
  const dim3 tgrid((unsigned)(ntiles < kMaxGrid ? ntiles : kMaxGrid)), pgrid((unsigned)(((long)total + 255) / 256));
  hipStream_t st = (hipStream_t)stream;
  const int esz = out_kind == PFD_IMG_U8 ? 1 : out_kind == PFD_IMG_NCHW_F32 ? 12 : 6;
  PfdProfScope prof_scope(15, 0.0, (double)total * (C + 6 + 5 + 10 + 6 + esz), st);
  if (C == 3)
    hipLaunchKernelGGL(canny_nms_kernel<3>, tgrid, dim3(256), 0, st, (const uint8_t*)src, (uint8_t*)states, (int*)parent,
                       (uint8_t*)strong, H, W, tiles_x, tiles_y, ntiles, low, high);
  else
    hipLaunchKernelGGL(canny_nms_kernel<1>, tgrid, dim3(256), 0, st, (const uint8_t*)src, (uint8_t*)states, (int*)parent,
                       (uint8_t*)strong, H, W, tiles_x, tiles_y, ntiles, low, high);
  hipLaunchKernelGGL(canny_link_kernel, pgrid, dim3(256), 0, st, (const uint8_t*)states, (int*)parent, H, W, total);
  hipLaunchKernelGGL(canny_resolve_kernel, pgrid, dim3(256), 0, st, (const uint8_t*)states, (int*)parent,
                     (uint8_t*)strong, total);
  hipLaunchKernelGGL(canny_emit_kernel, pgrid, dim3(256), 0, st, (const uint8_t*)states, (const int*)parent,
                     (const uint8_t*)strong, out, out_kind, H * W, total);
  return pfd_check_launch("pfd_canny_u8");
}
