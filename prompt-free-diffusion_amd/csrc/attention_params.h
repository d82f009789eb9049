// Kernel-side argument blocks of the attention entry points (attention.hip, attention3.hip) and, at the end, the host's
// dispatch plan over them.
#pragma once
#include <stdlib.h>

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

// ------------------------------------------------------------------------------------------------
// The dispatch plan: which kernel a launch of the three entry points takes.  Plain host code without device types -- the
// launcher of attention.hip, tools/cpu_emu and tests/kernel_refs.py (attention_kernel_class) all follow this one function;
// `emu_attn --dispatch` pins what it decides as tests/golden/attention_dispatch.txt.
// ------------------------------------------------------------------------------------------------
enum AttnOperand { ATTN_PLAIN, ATTN_KBIAS, ATTN_RBIAS };   // pfd_attention_f16 | pfd_attention_kbias_f16 | pfd_attention_rbias_f16
enum AttnClass {
  ATTN_A3,     // attention3_kernel: the software-pipelined d = 40 kernel, 4 waves x 64 queries
  ATTN_W8,     // <40, 8, true, true>: 8 waves, PV on 16x16x32 + the maximum folded into the QK^T MFMA (the 4-wave PV16 build
               // spills 24 bytes at 128 VGPRs)
  ATTN_W4,     // <D, 4, false>: every head dim but 512
  ATTN_D512,   // attention512_kernel<slices>
};
struct AttnPlan {
  int rc;                    // PFD_OK, or PFD_ESHAPE: no kernel is built for the request
  AttnClass cls;
  int qb, threads, slices;   // queries per block, threads per block, blocks per query tile (the V column slices of d = 512, else 1)
};

// The test hooks, read here and nowhere else.
struct AttnHooks {
  bool force8;   // PFD_ATTN_FORCE8=1: the 8-wave form for every d = 40 problem that has one (selftest --attn, tools/cpu_emu)
  bool force3;   // PFD_ATTN3_FORCE=1: attention3_kernel for small grids too (selftest --attn, tools/cpu_emu); Nk % 64 == 0, Nk >= 128 stay
  // PFD_ATTN512_SLICES: 2 (default since round 4) or 4 -- two 256-column slices recompute QK^T twice instead of four times
  // and keep 128 accumulator registers per wave in AGPRs (256 + 129 registers, no scratch): 0.363 vs 0.547 ms at the C2
  // shape, 1.39 vs 1.61 ms at 96^2 (profiles/r03_k18_vae_attention512.log).  One 512-column slice (256 accumulator
  // registers) crashes hipcc 7.2's register allocator, so it is not instantiated.  Read per launch (once per decoded
  // batch), so the GPU suite exercises both instantiations in one process.
  int slices512;
};
inline AttnHooks attn_hooks(int D) {
  static const bool force8 = getenv("PFD_ATTN_FORCE8") && atoi(getenv("PFD_ATTN_FORCE8")) != 0;
  static const bool force3 = getenv("PFD_ATTN3_FORCE") && atoi(getenv("PFD_ATTN3_FORCE")) != 0;
  const char* nsl = D == 512 ? getenv("PFD_ATTN512_SLICES") : nullptr;
  return {force8, force3, nsl && atoi(nsl) == 4 ? 4 : 2};
}

inline AttnPlan attn_plan(int B, int H, int Nq, int Nk, int D, AttnOperand op, const AttnHooks& hk) {
  const AttnPlan eshape = {PFD_ESHAPE, ATTN_W4, 0, 0, 0};
  if (D == 512)   // the plain operand only; one head, whole 32-key tiles
    return op == ATTN_PLAIN && H == 1 && Nk % 32 == 0 ? AttnPlan{PFD_OK, ATTN_D512, 128, 256, hk.slices512} : eshape;
  if (D != 40 && D != 80 && D != 160 && !(D == 96 && op == ATTN_PLAIN)) return eshape;
  const long blocks256 = (long)B * H * ((Nq + 255) / 256);
  if (D == 40 && op == ATTN_PLAIN && Nk % 64 == 0 && Nk >= 128) {
    // round 6: the software-pipelined 64-queries-per-wave kernel (attention3.hip) for self-attention-sized problems (decided on
    // hardware against the 8-wave kernel: 260 vs 284 us at B 8 / 64^2, profiles/r06_bench_attn_*.log; the A/B switch is gone).
    // Whole 64-key tiles, at least two of them; enough 256-query blocks to give every CU one.  It has no logit operand.
    if (hk.force3 || (Nq >= 256 && blocks256 >= 256)) return {PFD_OK, ATTN_A3, 256, 256, 1};
  }
  // 8-wave blocks pay when a block has many queries to amortise the staging over and the grid still fills the chip twice.
  // Not compiled with a row per region: the 4-wave d = 40 build takes those shapes too.
  if (D == 40 && op != ATTN_RBIAS && ((Nq >= 1024 && blocks256 >= 512) || hk.force8)) return {PFD_OK, ATTN_W8, 256, 512, 1};
  // (round 5: 64-query blocks of two waves for the grids that fill less than the chip -- d = 160 at 16^2 / 8^2 -- measured
  //  the same or slightly slower, profiles/r05_e2e_ab_candidates.log)
  return {PFD_OK, ATTN_W4, 128, 256, 1};
}

// attention3.hip: the way into the translation unit of ATTN_A3 (built with its own flags)
void pfd_attention3_launch(const AttnParams& p, dim3 grid, hipStream_t s);
