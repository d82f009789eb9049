// Request front door: packed uint8 pictures [B, H, W, C] -> what the reference builds on the host in front of the model,
// `imctl.resize([w, h], Image.Resampling.BICUBIC)` (app.py:232) and `tvtrans.ToTensor()(im)[None].to(dtype)` (app.py:234,244).
//
// The resize is Pillow's ImagingResample for 8-bit channels: two separable passes in 32-bit fixed point (coefficients scaled
// by 2^22, half added before the arithmetic shift, clamp to a byte), the horizontal one first, with a ROUNDED uint8 picture
// between them -- the vertical pass reads bytes, not the wide sums, which is what makes the result Pillow's byte for byte.
// The coefficient tables depend on (in, out) only and come from the host (lib/image_io.py: doubles, as in Pillow).
// ToTensor is (float)u8 / 255.0f with a correctly rounded division (u8 * (1 / 255.f) differs in 126 of the 256 values),
// then ONE rounding to f16 for an fp16 model; there is no _Float16 arithmetic here, so the excess-precision trap of
// elementwise.hip (round_f16) does not arise: the only narrowing is the final conversion of an fp32 value.
//
// All of it is byte shuffling, bound by memory: no MFMA, no inline assembly, no scratch (tests/test_image_ingest_cpu.py).
#include "pfd_common.h"

namespace {

constexpr int kMaxSide = 8192;
constexpr int kMaxRatio = 16;                        // in / out per axis
constexpr int kMaxTaps = 4 * kMaxRatio + 2;          // window of 2 * support + 1 = 65 samples at the largest ratio
constexpr int kHalf = 1 << (PFD_IMG_PRECISION_BITS - 1);

// ---- horizontal pass ------------------------------------------------------------------------------------------------
// A block is four waves; a wave owns 64 consecutive output pixels of ONE row and stages the input bytes their windows
// cover in LDS (at most 63 window starts of <= 16 pixels each + one window).  The row pitch W * C is not 16-byte aligned in
// general: the span is placed in LDS at the same offset mod 16 as in memory, so that its aligned middle moves as 16-byte
// loads / LDS stores and only the head and the tail move as bytes.  A thread then produces one whole pixel.
constexpr int kHPix = 64, kHRows = 4;
constexpr int kHSpan = (kHPix - 1) * kMaxRatio + 1 + kMaxTaps;             // input pixels
constexpr int kHRowBytes = ((kHSpan * 3 + 15 + 15) / 16) * 16;             // + the alignment offset, in 16-byte units

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

template <int C>
__global__ __launch_bounds__(256) void image_resample_h_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                               long rows, int Win, int Wout,
                                                               const int* __restrict__ kk, const int* __restrict__ xmin,
                                                               const int* __restrict__ klen, int ktaps) {
  __shared__ uint4 stage[kHRows][kHRowBytes / 16];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int x0 = blockIdx.y * kHPix;
  const int xl = min(x0 + kHPix, Wout) - 1;
  const long row = (long)blockIdx.x * kHRows + wave;
  const bool live = row < rows;
  // the tables are the caller's: every index derived from them is clamped to the row and to the staged span
  const int lo = clampi(xmin[x0], 0, Win);
  const int hi = min(clampi(xmin[xl] + klen[xl], lo, Win), lo + kHSpan);
  uint8_t* lds = reinterpret_cast<uint8_t*>(stage[wave]);
  const uint8_t* g = src + (row * Win + lo) * C;
  const int off = (int)(reinterpret_cast<uintptr_t>(g) & 15);
  if (live) {
    const int n = (hi - lo) * C;
    const int head = min(n, (16 - off) & 15);
    const int nvec = (n - head) >> 4;
    const int tail = head + nvec * 16;
    if (lane < head) lds[off + lane] = g[lane];
    for (int i = lane; i < nvec; i += 64)
      *reinterpret_cast<uint4*>(lds + off + head + 16 * i) = *reinterpret_cast<const uint4*>(g + head + 16 * i);
    if (lane < n - tail) lds[off + tail + lane] = g[tail + lane];
  }
  __syncthreads();
  const int x = x0 + lane;
  if (live && x < Wout) {
    const int s = clampi(xmin[x], lo, hi) - lo;
    const int kl = min(min(klen[x], ktaps), hi - lo - s);
    const int* __restrict__ w = kk + (long)x * ktaps;
    const uint8_t* p = lds + off + s * C;
    int acc[C];
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = kHalf;
    for (int t = 0; t < kl; ++t) {
      const int wt = w[t];
#pragma unroll
      for (int c = 0; c < C; ++c) acc[c] += (int)p[t * C + c] * wt;
    }
    uint8_t* o = dst + (row * Wout + x) * C;
#pragma unroll
    for (int c = 0; c < C; ++c) o[c] = (uint8_t)clampi(acc[c] >> PFD_IMG_PRECISION_BITS, 0, 255);
  }
}

// ---- vertical pass + ToTensor ---------------------------------------------------------------------------------------
// Threads run along the row: a thread owns V consecutive pixels (V * C bytes) of one output row and walks the taps down
// the column; V = 4 (dword loads, 8- / 16-byte stores) where the width and the pointers allow it, else V = 1 (bytes).  No
// LDS: neighbouring lanes read neighbouring bytes of the same input rows.  kk == NULL: no resampling (Hin == Hout), the
// bytes of row y go straight to the store -- ToTensor alone, or a copy.
__device__ __forceinline__ float to_unit(int u) { return (float)u / 255.0f; }   // IEEE division: ToTensor's .div(255)

template <int C, int V>
__global__ __launch_bounds__(256) void image_resample_v_kernel(const uint8_t* __restrict__ src, void* __restrict__ dst,
                                                               int kind, long total, int Hin, int Hout, int W,
                                                               const int* __restrict__ kk, const int* __restrict__ ymin,
                                                               const int* __restrict__ klen, int ktaps) {
  constexpr int N = C * V;
  const long gid = (long)blockIdx.x * 256 + threadIdx.x;
  if (gid >= total) return;
  const int nch = W / V;
  const int xq = (int)(gid % nch);
  const long t1 = gid / nch;
  const int y = (int)(t1 % Hout);
  const long b = t1 / Hout;
  const long pitch = (long)W * C;
  const uint8_t* col = src + b * Hin * pitch + (long)xq * N;
  int u[N];
  auto load = [&](const uint8_t* p, int* v) {
    if constexpr (V == 4) {
#pragma unroll
      for (int j = 0; j < N / 4; ++j) {
        const uint32_t d = reinterpret_cast<const uint32_t*>(p)[j];
#pragma unroll
        for (int e = 0; e < 4; ++e) v[4 * j + e] = (int)((d >> (8 * e)) & 255u);
      }
    } else {
#pragma unroll
      for (int j = 0; j < N; ++j) v[j] = (int)p[j];
    }
  };
  if (kk) {
    const int s = clampi(ymin[y], 0, Hin);
    const int kl = min(min(klen[y], ktaps), Hin - s);
    const int* __restrict__ w = kk + (long)y * ktaps;
    const uint8_t* p = col + s * pitch;
#pragma unroll
    for (int j = 0; j < N; ++j) u[j] = kHalf;
    for (int t = 0; t < kl; ++t, p += pitch) {
      const int wt = w[t];
      int v[N];
      load(p, v);
#pragma unroll
      for (int j = 0; j < N; ++j) u[j] += v[j] * wt;
    }
#pragma unroll
    for (int j = 0; j < N; ++j) u[j] = clampi(u[j] >> PFD_IMG_PRECISION_BITS, 0, 255);
  } else {
    load(col + y * pitch, u);
  }
  const long x = (long)xq * V;
  if (kind == PFD_IMG_U8) {
    uint8_t* o = reinterpret_cast<uint8_t*>(dst) + ((b * Hout + y) * W + x) * C;
    if constexpr (V == 4) {
#pragma unroll
      for (int j = 0; j < N / 4; ++j)
        reinterpret_cast<uint32_t*>(o)[j] = (uint32_t)u[4 * j] | ((uint32_t)u[4 * j + 1] << 8) |
                                            ((uint32_t)u[4 * j + 2] << 16) | ((uint32_t)u[4 * j + 3] << 24);
    } else {
#pragma unroll
      for (int j = 0; j < N; ++j) o[j] = (uint8_t)u[j];
    }
  } else if (kind == PFD_IMG_NHWC_F16) {
    half_t* o = reinterpret_cast<half_t*>(dst) + ((b * Hout + y) * W + x) * C;
    if constexpr (V == 4) {
#pragma unroll
      for (int j = 0; j < N / 4; ++j) {
        Pack8 q;
#pragma unroll
        for (int e = 0; e < 4; ++e) q.e[e] = (half_t)to_unit(u[4 * j + e]);
        reinterpret_cast<uint2*>(o)[j] = q.u;
      }
    } else {
#pragma unroll
      for (int j = 0; j < N; ++j) o[j] = (half_t)to_unit(u[j]);
    }
  } else {   // NCHW: channel c of the thread's pixels is V consecutive elements of plane (b, c)
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const long di = ((b * C + c) * Hout + y) * W + x;
      if (kind == PFD_IMG_NCHW_F16) {
        half_t* o = reinterpret_cast<half_t*>(dst) + di;
        if constexpr (V == 4) {
          Pack8 q;
#pragma unroll
          for (int e = 0; e < 4; ++e) q.e[e] = (half_t)to_unit(u[e * C + c]);
          *reinterpret_cast<uint2*>(o) = q.u;
        } else {
          o[0] = (half_t)to_unit(u[c]);
        }
      } else {
        float* o = reinterpret_cast<float*>(dst) + di;
        if constexpr (V == 4) {
          *reinterpret_cast<uint4*>(o) = make_uint4(__builtin_bit_cast(unsigned, to_unit(u[c])),
                                                    __builtin_bit_cast(unsigned, to_unit(u[C + c])),
                                                    __builtin_bit_cast(unsigned, to_unit(u[2 * C + c])),
                                                    __builtin_bit_cast(unsigned, to_unit(u[3 * C + c])));
        } else {
          o[0] = to_unit(u[c]);
        }
      }
    }
  }
}

int shape_error(const char* what) {
  pfd_set_error(what);
  return PFD_ESHAPE;
}

int check_axis(int in, int out) {
  return in >= 1 && in <= kMaxSide && out >= 1 && out <= kMaxSide && in <= kMaxRatio * out;
}

}  // namespace

extern "C" int pfd_image_resample_check(int32_t B, int32_t Hin, int32_t Win, int32_t Hout, int32_t Wout, int32_t C) {
  if (B < 1 || (C != 1 && C != 3)) return shape_error("pfd_image_resample: B >= 1 and C in {1, 3} (RGBA is premultiplied by Image.resize: another algorithm)");
  if (!check_axis(Hin, Hout) || !check_axis(Win, Wout))
    return shape_error("pfd_image_resample: sides 1 ... 8192, in / out <= 16 per axis");
  // (the flat thread index of the vertical pass and the row index of the horizontal one are 64-bit; the grids are not)
  const long hmax = Hin > Hout ? Hin : Hout, wmax = Win > Wout ? Win : Wout;
  if ((long)B * hmax > (1L << 30) || (long)B * hmax * wmax > (1L << 36))
    return shape_error("pfd_image_resample: more than 2^30 rows or 2^36 pixels");
  return PFD_OK;
}

extern "C" int pfd_image_resample_h_u8(const void* src, void* dst, int32_t B, int32_t H, int32_t Win, int32_t Wout,
                                       int32_t C, const int32_t* kk, const int32_t* xmin, const int32_t* klen,
                                       int32_t ktaps, pfd_stream_t stream) {
  if (!src || !dst || !kk || !xmin || !klen) return PFD_EINVAL;
  if (const int rc = pfd_image_resample_check(B, H, Win, H, Wout, C)) return rc;
  if (ktaps < 1 || ktaps > kMaxTaps) return shape_error("pfd_image_resample_h_u8: ktaps outside 1 ... 66");
  const long rows = (long)B * H;
  const dim3 grid((unsigned)((rows + kHRows - 1) / kHRows), (unsigned)((Wout + kHPix - 1) / kHPix));
  PfdProfScope prof_scope(15, 0.0, (double)rows * (Win + Wout) * C, (hipStream_t)stream);
  if (C == 3)
    hipLaunchKernelGGL(image_resample_h_kernel<3>, grid, dim3(256), 0, (hipStream_t)stream, (const uint8_t*)src,
                       (uint8_t*)dst, rows, Win, Wout, kk, xmin, klen, ktaps);
  else
    hipLaunchKernelGGL(image_resample_h_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, (const uint8_t*)src,
                       (uint8_t*)dst, rows, Win, Wout, kk, xmin, klen, ktaps);
  return pfd_check_launch("pfd_image_resample_h_u8");
}

extern "C" int pfd_image_resample_v_u8(const void* src, void* dst, int32_t out_kind, int32_t B, int32_t Hin,
                                       int32_t Hout, int32_t W, int32_t C, const int32_t* kk, const int32_t* ymin,
                                       const int32_t* klen, int32_t ktaps, pfd_stream_t stream) {
  if (!src || !dst || (kk && (!ymin || !klen))) return PFD_EINVAL;
  if (out_kind < PFD_IMG_U8 || out_kind > PFD_IMG_NHWC_F16) return PFD_EINVAL;
  if (const int rc = pfd_image_resample_check(B, Hin, W, Hout, W, C)) return rc;
  if (kk && (ktaps < 1 || ktaps > kMaxTaps)) return shape_error("pfd_image_resample_v_u8: ktaps outside 1 ... 66");
  if (!kk && Hin != Hout) return shape_error("pfd_image_resample_v_u8: no tap table, but Hin != Hout");
  const int esz = out_kind == PFD_IMG_U8 ? 1 : out_kind == PFD_IMG_NCHW_F32 ? 4 : 2;
  const bool vec = (W % 4) == 0 && (reinterpret_cast<uintptr_t>(src) & 3) == 0 &&
                   (reinterpret_cast<uintptr_t>(dst) & (uintptr_t)(4 * esz - 1)) == 0;
  const long total = (long)B * Hout * (vec ? W / 4 : W);
  const dim3 grid((unsigned)((total + 255) / 256));
  PfdProfScope prof_scope(15, 0.0, (double)B * W * C * ((double)Hin + (double)Hout * esz), (hipStream_t)stream);
#define PFD_IMG_LAUNCH_V(CC, VV)                                                                                        \
  hipLaunchKernelGGL((image_resample_v_kernel<CC, VV>), grid, dim3(256), 0, (hipStream_t)stream, (const uint8_t*)src,   \
                     dst, out_kind, total, Hin, Hout, W, kk, ymin, klen, ktaps)
  if (C == 3 && vec) PFD_IMG_LAUNCH_V(3, 4);
  else if (C == 3) PFD_IMG_LAUNCH_V(3, 1);
  else if (vec) PFD_IMG_LAUNCH_V(1, 4);
  else PFD_IMG_LAUNCH_V(1, 1);
#undef PFD_IMG_LAUNCH_V
  return pfd_check_launch("pfd_image_resample_v_u8");
}
