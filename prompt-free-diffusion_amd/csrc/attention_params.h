// Kernel-side argument block of pfd_attention_f16 (attention.hip, attention3.hip).
#pragma once
#include "pfd_common.h"

typedef unsigned u32x4 __attribute__((ext_vector_type(4)));

struct AttnParams {
  const half_t* Q;
  const half_t* K;
  const half_t* Vt;
  half_t* O;
  long ldq, ldk, ldvt, ldo;
  long q_bs, k_bs, vt_bs, o_bs;
  int B, H, Nq, Nk, D;
  float scale_log2;
};

// pfd_attention_kbias_f16: the same block followed by the per-key logits (fp32, log2 units; element (b, j) at kbias[b * kb_bs + j]).
// A type of its own, so that the argument block -- and with it the code -- of the kernels without the operand stays what it is.
struct AttnParamsKB : AttnParams {
  const float* kbias;
  long kb_bs;
  float inv_scale_log2;   // 1 / scale_log2: the unfolded builds stage kbias / (scale log2 e), the units of their raw scores
};
// (the kernel text is compiled for both blocks: what only the second one has is read through these)
__device__ __forceinline__ const float* attn_kbias_row(const AttnParams&, int) { return nullptr; }
__device__ __forceinline__ const float* attn_kbias_row(const AttnParamsKB& p, int b) { return p.kbias + (long)b * p.kb_bs; }
__device__ __forceinline__ float attn_inv_scale_log2(const AttnParams&) { return 0.f; }
__device__ __forceinline__ float attn_inv_scale_log2(const AttnParamsKB& p) { return p.inv_scale_log2; }

// pfd_attention_rbias_f16: the logits depend on the REGION of the query.  A table of nr <= ATTN_MAX_REGIONS rows per sample
// (element (b, g, j) at rbias[b * rb_bs + g * rb_rs + j]) and one region id per query (qregion[b * qr_bs + i]; qr_bs = 0: one
// map for the batch).  Again a type of its own: the two blocks above, and the code compiled over them, stay what they are.
constexpr int ATTN_MAX_REGIONS = 8;
struct AttnParamsRB : AttnParams {
  const float* rbias;
  long rb_rs, rb_bs;
  const unsigned char* qregion;
  long qr_bs;
  int nr;
  float inv_scale_log2;
  float m_start;          // the running maximum before the first live key: -2^100 log2 units in the units of the raw score
};
__device__ __forceinline__ const float* attn_kbias_row(const AttnParamsRB& p, int b) { return p.rbias + (long)b * p.rb_bs; }
__device__ __forceinline__ float attn_inv_scale_log2(const AttnParamsRB& p) { return p.inv_scale_log2; }
// (what only the third block has; the other two never reach these calls: `if constexpr (RBIAS)`)
template <class P> __device__ __forceinline__ int attn_nr(const P&) { return 1; }
__device__ __forceinline__ int attn_nr(const AttnParamsRB& p) { return p.nr; }
template <class P> __device__ __forceinline__ long attn_rb_rs(const P&) { return 0; }
__device__ __forceinline__ long attn_rb_rs(const AttnParamsRB& p) { return p.rb_rs; }
template <class P> __device__ __forceinline__ const unsigned char* attn_qregion(const P&, int) { return nullptr; }
__device__ __forceinline__ const unsigned char* attn_qregion(const AttnParamsRB& p, int b) { return p.qregion + (long)b * p.qr_bs; }
template <class P> __device__ __forceinline__ float attn_m_start(const P&) { return -__builtin_inff(); }
__device__ __forceinline__ float attn_m_start(const AttnParamsRB& p) { return p.m_start; }

// attention3.hip: the software-pipelined d = 40 kernel (64 queries per wave); `takes` = shapes it is built for
bool pfd_attention3_takes(const AttnParams& p);
void pfd_attention3_launch(const AttnParams& p, hipStream_t s);
