// Shared device-side helpers for the gfx950 kernels of libpfd_hip.so.
// Wavefront = 64 lanes, MFMA f16 shapes 32x32x16 / 16x16x32, fp32 accumulate.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pfd_hip.h"

typedef _Float16 half_t;
typedef _Float16 half2_t __attribute__((ext_vector_type(2)));
typedef _Float16 half4_t __attribute__((ext_vector_type(4)));
typedef _Float16 half8_t __attribute__((ext_vector_type(8)));
typedef float float4_t __attribute__((ext_vector_type(4)));
typedef float float16_t __attribute__((ext_vector_type(16)));

#define PFD_WAVE 64

// MFMA C/D layouts (guide §3):
//   32x32: col = lane & 31, row = (r & 3) + 8*(r >> 2) + 4*(lane >> 5), r in [0,16)
//   16x16: col = lane & 15, row = 4*(lane >> 4) + r,                   r in [0,4)
// A operand: lane holds 8 consecutive k of row (lane & 31 | lane & 15); B likewise for a column.
// The k owned by (lane-group, j) only has to agree between A and B.
__device__ __forceinline__ int mfma32_row(int r, int hi) { return (r & 3) + 8 * (r >> 2) + 4 * hi; }

// exact-erf GELU (torch F.gelu default) evaluated with the Abramowitz-Stegun 7.1.26 erfc form:
// erfc(z) = t*P4(t)*exp(-z^2), t = 1/(1 + p z); |abs error| < 5e-7 in gelu(x), far inside one fp16 ulp of
// the stored result, and ~13 VALU ops instead of ocml erff's branchy ~40 -- the GEGLU epilogue of the
// 64^2 feed-forward evaluates 42 M of these per launch. The negative side uses erfc directly, so there
// is no 1 - erf cancellation in the tail.
__device__ __forceinline__ float pfd_gelu(float x) {
  const float z = fabsf(x) * 0.70710678118654752440f;
  const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f, z, 1.0f));
  float poly = fmaf(t, 1.061405429f, -1.453152027f);
  poly = fmaf(t, poly, 1.421413741f);
  poly = fmaf(t, poly, -0.284496736f);
  poly = fmaf(t, poly, 0.254829592f);
  const float half_erfc = 0.5f * t * poly * __builtin_amdgcn_exp2f(-1.4426950408889634f * z * z);
  return x * (x >= 0.0f ? 1.0f - half_erfc : half_erfc);
}
__device__ __forceinline__ float pfd_silu(float x) {
  return x * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.4426950408889634f * x));
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

union Pack16 {
  uint4 u;
  half8_t h;
  half_t e[8];
};

union Pack8 {
  uint2 u;
  half_t e[4];
};

// Global-memory accesses with the address space spelled out at the access: a pointer the compiler cannot trace to a kernel
// argument (gemm_glds.hip, reload_params) is generic to it (flat_load / flat_store, which also tick lgkmcnt and order against
// LDS reads); through these they are global_load / global_store whatever the pointer's provenance.
template <int BYTES> struct GRaw;
template <> struct GRaw<2>  { typedef unsigned short type; };
template <> struct GRaw<4>  { typedef unsigned int type; };
template <> struct GRaw<8>  { typedef unsigned int type __attribute__((ext_vector_type(2))); };
template <> struct GRaw<16> { typedef unsigned int type __attribute__((ext_vector_type(4))); };
template <class T>
__device__ __forceinline__ T gld(const void* ptr) {
  typedef typename GRaw<sizeof(T)>::type V;
  const V v = *reinterpret_cast<const __attribute__((address_space(1))) V*>((unsigned long)ptr);
  T out;
  __builtin_memcpy(&out, &v, sizeof(T));
  return out;
}

// Cache policy of an output store.  A policy changes where the line lives after the store, never the value
// and never the visibility rules: consumers are later launches, ordered by the kernel boundary as before.
//   ST_PLAIN  the line stays dirty in the XCD's L2 until something writes it back (at the latest the end of the kernel)
//   ST_WT     write-through (sc1): the bytes leave the L2 as they are stored, the kernel ends with nothing left to write back
//   ST_NT     non-temporal (nt): kept in L2, marked for early eviction
enum StorePolicy { ST_PLAIN = 0, ST_WT = 1, ST_NT = 2 };
// The policy of each family of stores, decided family by family on end-to-end pairs (profiles/store_policy.md): the final
// store passes of the GEMM / convolution kernels write through (-1.45 % / -0.87 % per batch on two machines, nothing on a third); every
// other family's write-through and non-temporal arms were inside the run-to-run spread or slower and stay plain.
constexpr int PFD_ST_SLAB = ST_PLAIN;      // split-K partial sums (epilogue_store, slab branch): sc1 +0.15 %, nt -0.4 % (inside the spread)
constexpr int PFD_ST_REDUCE = ST_PLAIN;    // outputs of the split-K reduction kernels: sc1 -0.04 %
constexpr int PFD_ST_OUT = ST_WT;          // final outputs of the GEMM / convolution store passes (with ln_out; not the 2-byte tail)
constexpr int PFD_ST_ATTN = ST_PLAIN;      // attention outputs: sc1 +0.6 %
constexpr int PFD_ST_NORM = ST_PLAIN;      // GroupNorm / LayerNorm apply kernels: sc1 -0.06 %

template <int POLICY = ST_PLAIN, class T>
__device__ __forceinline__ void gst(void* ptr, T val) {
  typedef typename GRaw<sizeof(T)>::type V;
  V v;
  __builtin_memcpy(&v, &val, sizeof(T));
  typedef __attribute__((address_space(1))) V* GPtr;
  GPtr g = reinterpret_cast<GPtr>((unsigned long)ptr);
#if defined(PFD_CPU_EMU)
  *g = v;
#else
  if constexpr (POLICY == ST_NT) {
    __builtin_nontemporal_store(v, g);
  } else if constexpr (POLICY == ST_WT && sizeof(T) == 16) {
    // (the trailing s_nop keeps the data registers from being rewritten in the store's issue shadow; "memory": the compiler
    //  must not move other accesses of these bytes across a store it cannot see)
    asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" ::"v"(g), "v"(v) : "memory");
  } else if constexpr (POLICY == ST_WT && sizeof(T) == 8) {
    unsigned long bits;   // a relaxed agent-scope atomic store is the compiler-visible spelling of an 8-byte sc1 store
    __builtin_memcpy(&bits, &val, 8);
    __hip_atomic_store(reinterpret_cast<__attribute__((address_space(1))) unsigned long*>((unsigned long)ptr), bits,
                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  } else {
    static_assert(POLICY == ST_PLAIN, "write-through stores are 8 or 16 bytes wide");
    *g = v;
  }
#endif
}
// The same for a store through a pointer the compiler can trace to a kernel argument: under ST_PLAIN it is the ordinary typed
// store (type-based alias information and __restrict__ intact, so the schedule around it is what it always was)
template <int POLICY = ST_PLAIN, class T>
__device__ __forceinline__ void gst_t(T* ptr, T val) {
  if constexpr (POLICY == ST_PLAIN) *ptr = val;
  else gst<POLICY>(ptr, val);
}

// XCD-aware, bijective remap of a linear block id: the dispatcher places block b on XCD
// b % 8; give every XCD one contiguous chunk of the tile space so neighbouring tiles
// (which share an operand panel) meet in the same L2.  Speed only, never correctness.
__device__ __forceinline__ int xcd_remap(int bid, int nblk) {
  const int q = nblk >> 3, r = nblk & 7;
  const int xcd = bid & 7, idx = bid >> 3;
  const int start = xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q;
  return start + idx;
}

// optional per-launch event timing (capi.hip); buckets: 0-7 gemm <TM,TN,CONV>, 8 attention,
// 9 swin attention, 10 groupnorm, 11 layernorm
bool pfd_prof_on();
void pfd_prof_begin(int bucket, double flops, double bytes, hipStream_t stream);
void pfd_prof_end(hipStream_t stream);
// event pair around every launch of the enclosing scope (no-op unless pfd_prof_enable(1)); the destructor runs after the
// `return pfd_check_launch(...)` expression, i.e. after the launches
struct PfdProfScope {
  hipStream_t s;
  bool on;
  PfdProfScope(int bucket, double flops, double bytes, hipStream_t st) : s(st), on(pfd_prof_on()) {
    if (on) pfd_prof_begin(bucket, flops, bytes, s);
  }
  ~PfdProfScope() {
    if (on) pfd_prof_end(s);
  }
  PfdProfScope(const PfdProfScope&) = delete;
  PfdProfScope& operator=(const PfdProfScope&) = delete;
};

// pointer alignment the 16-byte (8-byte) vector accesses of the kernels need
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
inline bool aligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) == 0; }

// blocks of a grid-stride launch over n items: at most 4096
inline int grid_for(long n, int block) {
  long g = (n + block - 1) / block;
  if (g > 4096) g = 4096;
  if (g < 1) g = 1;
  return (int)g;
}

// host-side error plumbing (defined in capi.cpp)
int pfd_check_launch(const char* what);
void pfd_set_error(const char* msg);
