// The bit-pinned stages of the GroupNorm family (norm.hip) and of the split-K reduction tails (gemm_glds.hip), each written
// once.  Several kernels are documented as producing the same bits -- the fused split-K reduction + GroupNorm and the
// separate pair, the table and the apply kernel, the PAR and the plain producer-statistics form, a sample whatever its
// batch -- and tests/golden/norm_bits.txt holds every one of them to the bits it had.  Those relations hold because the
// kernels call the functions below, not because the same lines were typed alike.
//
// Rounding (DESIGN.md 3.22 has the table and the measurements).  The affine map switches contraction off and spells its
// fma.  The variance of gn_finalise and the fma of gn_normalise are still contracted by the compiler -- to one fma at every
// call site, in the parent's gfx950 assembly and in this one: spelled as __builtin_fmaf they compute the same, but
// gn_small_kernel takes 65 registers instead of 61 and gn_apply_pstats_kernel<true> 160 instead of 97, and
// tests/test_store_policy_cpu.py pins both.  Every other product of these kernels (the slab accumulation `acc += slab * w`,
// the producer-partial gather, the squares of the slab statistics) has a factor that is exactly 0 or 1, or is the square
// of an f16 value: exact in fp32, so the bits are the same fused or not.
//
// Everything sits in the unnamed namespace of the including file: the kernels' symbols (GnSrc is part of four of them) are
// pinned by tests/test_store_policy_cpu.py.  __shared__ arrays stay declared in the kernels and come in as pointers.
#pragma once
#include "pfd_common.h"

namespace {

constexpr int GN_MAX_G = 64;
// threads of a block that keeps one (sample, group) slab in registers (gn_small_kernel, splitk_reduce_gnorm_kernel), and the
// 4-half chunks each of them holds: 1024 since round 5 -- the launch is one round trip of the slab, so its time is set by the
// loads a block has in flight; with 256 the fused reduction took as long as the pair it replaces (profiles/r05_fused_gnorm_ab.log)
#ifndef PFD_GN_THREADS
#define PFD_GN_THREADS 1024   // (-DPFD_GN_THREADS=256: A/B builds)
#endif
constexpr int GNS_T = PFD_GN_THREADS;
constexpr int GNS_MAX = 8192 / GNS_T;

struct GnSrc {
  const half_t* x1;
  const half_t* x2;
  long ld1, ld2;
  int C1, C2;
};

__device__ __forceinline__ uint4 gn_load(const GnSrc& s, long row, int v) {
  const int c = v * 8;
  if (c < s.C1) return *reinterpret_cast<const uint4*>(s.x1 + row * s.ld1 + c);
  return *reinterpret_cast<const uint4*>(s.x2 + row * s.ld2 + (c - s.C1));
}

// ---- finalise: mean = r(sum / count), rstd = rsqrt(max(var, 0) + eps); var is contracted by the compiler, in each of
// the six kernels that end here, to fma(-mean, mean, r(sumsq / count))
__device__ __forceinline__ void gn_finalise(float sum, float sumsq, float count, float eps, float& mean, float& rstd) {
  mean = sum / count;
  rstd = rsqrtf(fmaxf(sumsq / count - mean * mean, 0.f) + eps);
}

// ---- affine map of one channel: scale = r(rstd gamma), shift = fma(-mean, scale, beta)
__device__ __forceinline__ void gn_affine(float mean, float rstd, float gamma, float beta, float& scale, float& shift) {
#pragma clang fp contract(off)
  scale = rstd * gamma;
  shift = __builtin_fmaf(-mean, scale, beta);
}

// one element: f16(act(x scale + shift)), contracted by the compiler at every call site to fma(x, scale, shift)
__device__ __forceinline__ half_t gn_normalise(float x, float scale, float shift, int act) {
  float t = x * scale + shift;
  if (act == PFD_ACT_SILU) t = pfd_silu(t);
  return (half_t)t;
}

// the maps of all C channels of one sample, by the 256 threads of a block: into LDS (the apply kernels) or into the two
// planes of the table
__device__ __forceinline__ void gn_channel_maps(const half_t* __restrict__ gamma, const half_t* __restrict__ beta,
                                                const float* gmean, const float* grstd, int C, int cpg, float* scale,
                                                float* shift) {
  for (int c = threadIdx.x; c < C; c += 256) {
    const int g = c / cpg;
    float w, o;
    gn_affine(gmean[g], grstd[g], (float)gamma[c], (float)beta[c], w, o);
    scale[c] = w;
    shift[c] = o;
  }
}

// ---- partials fold, LDS second stage: thread (part, g) of a 256-thread block brings the sums (a, q) of its share of group
// g; threads 0 .. G-1 add the P = 256 / G shares in order and finalise into gmean / grstd
__device__ __forceinline__ void gn_fold_lds(float a, float q, int G, float count, float eps, float* ra, float* rq,
                                            float* gmean, float* grstd) {
  const int tid = threadIdx.x, P = 256 / G;
  ra[tid] = a;
  rq[tid] = q;
  __syncthreads();
  if (tid < G) {
    for (int k = 1; k < P; ++k) {
      a += ra[k * G + tid];
      q += rq[k * G + tid];
    }
    gn_finalise(a, q, count, eps, gmean[tid], grstd[tid]);
  }
  __syncthreads();
}

// the whole fold of the nchunks x G partial sums gn_stats_kernel wrote for sample b (<= 64 KB, L2 resident): thread
// (part, g) sums chunks part, part + P, ..., then the LDS stage
__device__ __forceinline__ void gn_fold_partials(const float* __restrict__ partial, int b, int nchunks, int G, float count,
                                                 float eps, float* ra, float* rq, float* gmean, float* grstd) {
  const int tid = threadIdx.x, P = 256 / G;
  const int g = tid % G, part = tid / G;
  float a = 0.f, q = 0.f;
  if (part < P) {
    for (int k = part; k < nchunks; k += P) {
      const float2 v = *reinterpret_cast<const float2*>(partial + (((long)b * nchunks + k) * G + g) * 2);
      a += v.x;
      q += v.y;
    }
  }
  gn_fold_lds(a, q, G, count, eps, ra, rq, gmean, grstd);
}

// ---- apply loop: the rows of chunk `chunk` of sample b, U rows requested per round trip.  Thread (v, rt) owns the 8
// channels v*8.. (two vec slots when C > 2048) and rows rt, rt + RT, ...; sc / sh: the channel maps in LDS
template <int U>
__device__ __forceinline__ void gn_apply_rows(const GnSrc& s, const float* sc, const float* sh, half_t* __restrict__ y,
                                              long ldy, int HW, int b, int chunk, int rows_per_chunk, int act) {
  const int tid = threadIdx.x;
  const int nvec = (s.C1 + s.C2) / 8;
  const int VT = nvec < 256 ? nvec : 256;
  const int RT = 256 / VT;
  const int v0 = tid % VT, rt = tid / VT;
  if (rt >= RT) return;
  const int r_beg = chunk * rows_per_chunk;
  const int r_end = min(HW, r_beg + rows_per_chunk);
  for (int v = v0; v < nvec; v += 256) {
    float w[8], o[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      w[e] = sc[v * 8 + e];
      o[e] = sh[v * 8 + e];
    }
    for (int r = r_beg + rt; r < r_end; r += U * RT) {
      Pack16 p[U];
#pragma unroll
      for (int u = 0; u < U; ++u)
        if (r + u * RT < r_end) p[u].u = gn_load(s, (long)b * HW + r + u * RT, v);
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (r + u * RT >= r_end) break;
        const long row = (long)b * HW + r + u * RT;
        Pack16 q;
#pragma unroll
        for (int e = 0; e < 8; ++e) q.e[e] = gn_normalise((float)p[u].e[e], w[e], o[e], act);
        gst_t<PFD_ST_NORM>(reinterpret_cast<uint4*>(y + row * ldy + v * 8), q.u);
      }
    }
  }
}

// ---- slab statistics of a GNS_T-thread block: (sm, sq) = the sums a thread formed over its GNS_MAX chunks of 4 halves
// (chunk k, element e in order; padding slots zero) -> wave_sum -> red[2 * GNS_T / 64] -> every thread adds the wave totals
// in order -> finalise.  The eight-line thread loop itself stays in the two kernels: as a function here it costs
// gn_small_kernel a register (62 for 61).
__device__ __forceinline__ void gn_slab_stats(float sm, float sq, int HW, int cpg, float eps, float* red, float& mean,
                                              float& rstd) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  sm = wave_sum(sm);
  sq = wave_sum(sq);
  constexpr int NWV = GNS_T / 64;
  if (lane == 0) {
    red[wave] = sm;
    red[NWV + wave] = sq;
  }
  __syncthreads();
  const float count = (float)HW * (float)cpg;
  float ts = red[0], tq = red[NWV];
#pragma unroll
  for (int w = 1; w < NWV; ++w) {
    ts += red[w];
    tq += red[NWV + w];
  }
  gn_finalise(ts, tq, count, eps, mean, rstd);
}

// ---- split-K epilogue tail of one element: accumulator + bias, + row vector, activation, + residual, one rounding to f16
__device__ __forceinline__ half_t splitk_tail(float acc, half_t bias, half_t rowvec, half_t residual, int act) {
  float x = acc + (float)bias;
  x += (float)rowvec;
  if (act == PFD_ACT_GELU) x = pfd_gelu(x);
  else if (act == PFD_ACT_RELU) x = fmaxf(x, 0.f);
  else if (act == PFD_ACT_SILU) x = pfd_silu(x);
  return (half_t)(x + (float)residual);
}

}  // namespace
