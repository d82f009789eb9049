// pfd_attention_f16: fused QK^T -> online softmax -> PV on v_mfma_f32_32x32x16_f16.
//
// The kernel works on the TRANSPOSED problem so that the softmax reduction axis is
// (almost) lane-local and P never leaves registers:
//     S^T[kv, q] = sum_d K[kv, d] Q[q, d]        A = K tile (LDS), B = Q (registers)
//     O^T[d,  q] = sum_kv V^T[d, kv] P^T[kv, q]   A = V^T tile (LDS), B = P^T (registers)
// A 32x32 S^T accumulator has col = q = lane&31 and rows kv = (r&3) + 8(r>>2) + 4(lane>>5):
// one q column is split over lanes l and l^32, so the row max needs exactly one cross-lane
// exchange.  Registers 8b..8b+7 of that accumulator are, for 16-kv block b, the 8 values an MFMA
// B operand wants -- in the k order pi(hi, j) = (j&3) + 8(j>>2) + 4hi.  MFMA only needs A and B
// to agree on which k a (lane-group, j) slot means, so the V^T A operand is read in the same pi
// order: two 8-byte LDS reads per fragment, no permutation of P.
// V arrives already transposed from its producer GEMM (see pfd_hip.h), K row-major.
//
// Block = 4 waves x 32 query rows; KV tile = 64 keys, two LDS stages: the global loads of tile
// t+1 are issued (to registers) before the MFMAs of tile t and written to the other stage after
// them -- one barrier per tile, HBM/L2 latency hidden under compute.
//
// The path is VALU-bound at head dim 40 (160 MFMA flops per score vs ~4 VALU ops), so the softmax
// is kept to max / fma / v_exp / cvt per score:
//   * scores stay raw; p = exp2(s*c - m*c) with c = scale*log2(e) is one fma + one v_exp_f32;
//   * the row sum costs nothing when the V^T tile has padding rows (D = 40, 80): row D of the LDS
//     tile is set to 1.0, so O^T[D, q] accumulates sum_kv P -- with exactly the fp16-rounded P that
//     multiplies V, and it is rescaled with the rest of the accumulator;
//   * the accumulator is rescaled only when some row of the wave actually raised its running max
//     (exact: alpha == 1 otherwise).
// Per tile per wave: 2*DQK/16 + 4*DV/32 MFMAs (DQK = D rounded to 16, DV = D rounded to 32).
#include <type_traits>

#include "pfd_common.h"
#include "attention_params.h"

namespace {

// Occupancy: D = 40 needs 136 VGPRs when left alone (3 waves per SIMD); asked for 4 waves per SIMD the
// allocation fits 128 without scratch and self-attention at N = 4096 gains 4.6 % (452 -> 473 TF), the 148-key
// cross-attention 16 % (profiles/r02_attention_ablation.log).  A 128-key tile (half the barriers, 62 KB LDS,
// 184 VGPRs) measured 2 % slower.  Larger head dims keep their natural allocation.
// (The round-2 kernel this describes -- attention_kernel<D, 64>, PFD_ATTN=0 -- and the intermediate stages PFD_ATTN=1..5 were
//  removed in round 5; git history and profiles/r03_attention_modes.log hold their measurements.)
// ------------------------------------------------------------------------------------------------
// The attention kernel (round 3 on; same math, same LDS K image, same transposed formulation as the round-2 kernel):
//  * the ragged last KV tile is PEELED: the loop over full tiles has no key masking, no clamped row indices and no
//    64-bit address arithmetic (per-thread source pointers advance by a constant per tile).  The ISA of the old loop
//    spent ~60 of its ~200 VALU instructions per tile on that, and the softmax path is VALU bound at d = 40.
//  * NWAVES = 8: 256 queries per block share one staged K / V^T tile (the global loads, ds_writes and the barrier of
//    a tile are paid once per 256 queries instead of per 128; the "no loads / staging" ablation of the old kernel
//    was -29 %).  Same 4 waves per SIMD (two 512-thread blocks per CU).
//  * PV16 (d = 40): O^T = V^T . P^T on v_mfma_f32_16x16x32_f16, so the head dim pads 40 -> 48 instead of 64 (12
//    MFMAs x 16 cycles per tile instead of 8 x 32).  The 32x32 S^T accumulator holds query l & 31 in lane l; a
//    16x16x32 B operand wants the SAME 16 queries in all four 16-lane rows.  One v_permlane16_swap per packed
//    register pair (16-key blocks bb = 0 / 1 of a 32-key half) does it: afterwards the first register holds queries
//    0-15 in every row (row kg = 2 hi + bb), the second queries 16-31.  MFMA only needs A and B to agree on which key a
//    (row, slot) pair means, so the V^T A operand is read in that order: keys 32 u + 16 bb + 4 hi + {0..3} and + 8.
//    The V^T image is 64 halfs per row without padding; 8-byte slot s of row d is stored at s ^ sigma(d),
//    sigma = d[1] | d[2] << 1 | d[3] << 3, which makes both ds_read_b64 of a fragment conflict free (rows of equal
//    parity share a bank half; {sigma} and {sigma ^ 4} partition its 16 slots).
// ------------------------------------------------------------------------------------------------
//  * FOLD (d = 40): the running maximum is subtracted BY THE QK^T MFMA.  D pads 40 -> 48 in the contraction, so slot 40
//    is free: K's LDS image carries 1.0 there, the (pre-scaled, Q' = scale log2(e) Q) query fragment carries -m, and the
//    accumulator comes out as s' - m -- the per-score fma in front of v_exp_f32 (31 of the ~105 VALU instructions of a
//    tile) disappears.  m is kept as an f16 value (it lives in an f16 operand slot); every use of it -- the fold, the
//    accumulator rescale -- sees the same rounded number, so the rounding cancels in O / l exactly like any other
//    common factor.  The maximum is only RAISED when a row's tile maximum exceeds the folded one by more than 6 (P <= 64
//    in f16; the guide's T13 deferred rescale), or on the first tile; that path subtracts the increment explicitly.
// The LDS image (K / V^T tiles incl. padding) is cleared with 16-byte stores before the first tile (round 5: the rolled loop of
// ds_write_b16 it replaces was 169 trips per thread at d = 160, ~2 us of an 18 us launch; -0.95 % per batch, same bits --
// profiles/r05_e2e_ab_candidates.log.  s_setprio(1) around the two MFMA clusters of a tile, the guide's T5, measured +0.2 %
// here and is not compiled in.)
//  * KBIAS (pfd_attention_kbias_f16): an additive per-key logit kbias[b, j] in log2 units -- log2 of a key's weight, or -inf for
//    a key that is not there.  The 64 values of a tile are STAGED WITH ITS K TILE (one float per thread of the first wave, 256
//    bytes per LDS stage behind the V^T images; one LDS-DMA dword load of the first wave) and read back as four broadcast ds_read_b128 per 32-key half right where the
//    scores leave the QK^T MFMAs: rows (r & 3) + 8 (r >> 2) + 4 hi of the accumulator are four runs of four consecutive keys.
//    (Four 16-byte global loads per half issued ahead of the MFMAs would hold 32 more registers live across them; the d = 40
//    builds have none to spare at 128.)  The logit meets the score in the score's units -- kbias itself in the FOLD build, whose
//    accumulator is in log2 units, kbias (1 / c) with c = scale log2 e where the score is raw (one multiply) -- and it meets
//    it as the START VALUE of the QK^T accumulator instead of 0: the MFMAs add it, s + kbias / c = (s c + kbias) / c, in front
//    of the tile maximum -- no add per score and no register of its own; the multiply by 1 / c is the one VALU instruction
//    per score of the builds with raw scores, the FOLD build has none.  Everything behind the MFMAs -- maximum, rescale,
//    exp2(fma(s, c, -m c)) -- is the code of the kernel without the operand: an all-zero kbias starts the accumulator at 0.0
//    and gives the bits of pfd_attention_f16.  A tile whose keys are all -inf has mx = -inf: it raises nothing,
//    every p is exp2(-inf) = 0 and -- K and V being finite by contract -- the accumulators and the row sum stay as they were.
//    Key 0 is finite by contract, so the running maximum is finite from the first tile on and (-inf) - (-inf) never occurs.
//    Without KBIAS nothing of this is compiled: the kernels of pfd_attention_f16 are the code they were (tools/isa_diff.py).
//  * RBIAS (pfd_attention_rbias_f16): the logit row depends on the REGION of the query -- a table rbias[b, g, j] of nr <= 8 rows and
//    one region id per query.  In the S^T layout a lane IS a query (l31), so the only change to the arithmetic is WHICH row the
//    accumulator start reads: all nr rows of a tile are staged (row g by wave g % NWAVES, one LDS-DMA dword load each, 2 x 8 x 256
//    bytes of LDS), and the four 16-byte reads per 32-key half go to row `region of this lane` -- no broadcasts any more (lanes of
//    one region still share an address).  The block's QB region ids are staged into LDS once (as row offsets, clamped to nr - 1)
//    and the lane re-reads its own per tile from an opaque index: kept live across the loop it would cost the d = 40 build a
//    register it does not have.  Built for the unfolded classes only (4 waves at d = 40, d = 80, d = 160); the 4-wave build
//    serves the shapes the folded 8-wave one takes elsewhere.
//    Fully masked LEADING tiles are legal here (a region that uses only the second reference masks the whole first tile), so
//    "key 0 is finite" is replaced by "every region that occurs keeps one finite key somewhere", and the running maximum starts
//    at a finite -2^100 log2 units instead of -inf: see the comment at m_run in the kernel text for why no (-inf) - (-inf) occurs,
//    lane by lane (one wave holds queries of regions that start on different tiles).  For a region whose key 0 is finite every
//    value of the lane's column is what attention_kbias_kernel computes from that row: alpha of the first tile is exp2(-huge) = 0
//    there and exp2(-inf) = 0 here, and a rescale another lane of the wave asks for multiplies this lane by alpha = 1.
// (the kernel text is attention2_kernel.inc, compiled once without the key logits, once with them and once with a row per region)
#define ATTN2_KERNEL_NAME attention2_kernel
#define ATTN2_PARAMS AttnParams
#define ATTN2_KBIAS false
#define ATTN2_RBIAS false
#include "attention2_kernel.inc"
#undef ATTN2_KERNEL_NAME
#undef ATTN2_PARAMS
#undef ATTN2_KBIAS
#define ATTN2_KERNEL_NAME attention_kbias_kernel
#define ATTN2_PARAMS AttnParamsKB
#define ATTN2_KBIAS true
#include "attention2_kernel.inc"
#undef ATTN2_KERNEL_NAME
#undef ATTN2_PARAMS
#undef ATTN2_RBIAS
#define ATTN2_KERNEL_NAME attention_rbias_kernel
#define ATTN2_PARAMS AttnParamsRB
#define ATTN2_RBIAS true
#include "attention2_kernel.inc"
#undef ATTN2_KERNEL_NAME
#undef ATTN2_PARAMS
#undef ATTN2_KBIAS
#undef ATTN2_RBIAS

// ------------------------------------------------------------------------------------------------
// d = 512, one head: the VAE mid-block attention (autokl_modules.py:186-197).  Same transposed formulation
// (S^T = K Q^T, O^T = V^T P^T on v_mfma_f32_32x32x16_f16, online softmax per query = per lane column), but the head does
// not fit one wave's registers as a whole: a wave keeps the Q fragments of its 32 queries for the full contraction
// (32 k-steps x 4 VGPRs = 128) and the O^T accumulators of ONE 128-column slice of V (4 tiles x 16 = 64); the four
// slices are four blocks (blockIdx -> (batch, query tile, slice)), each of which recomputes QK^T -- 4 x 34 + 34 GFLOP per
// 512^2 image instead of 68, for no [N, N] score matrix in HBM at any resolution.  KV tile = 32 keys: the K image
// (32 x 520 halfs) and the V^T slice image (128 x 36 halfs) are double buffered in 85 KB of LDS; one block per CU,
// four waves on four SIMDs, up to 512 unified registers per wave (accumulators in AGPRs).
// Requires Nk % 32 == 0 (the VAE's token counts are multiples of 64).
// ------------------------------------------------------------------------------------------------
template <int NSL>   // V column slices per query tile: 4 (128 columns, 64 accumulator registers) or 2 (256 columns, 128)
__global__ __launch_bounds__(256, 1) void attention512_kernel(const AttnParams p) {
  constexpr int D = 512, DVC = D / NSL, KV_TILE = 32, NTHR = 256, QB = 128;
  constexpr int K_LD = D + 8;           // 1040-B rows: an odd multiple of 16 B, conflict-free ds_read_b128 over 32 rows
  constexpr int VT_LD = KV_TILE + 4;    // 72-B rows: 18 dwords, conflict-free ds_read_b64 over 32 rows
  constexpr int NS = D / 16;            // 32 k-steps of the QK^T contraction
  constexpr int ND = DVC / 32;          // 4 O^T tiles
  constexpr int K_PT = KV_TILE * (D / 8) / NTHR;        // 8 16-byte chunks of K per thread and tile
  constexpr int V_PT = DVC * (KV_TILE / 8) / NTHR;      // 2 of V^T
  constexpr int K_TILE_HALFS = KV_TILE * K_LD;
  constexpr int V_TILE_HALFS = DVC * VT_LD;
  __shared__ __attribute__((aligned(16))) half_t lds[2 * K_TILE_HALFS + 2 * V_TILE_HALFS];
  half_t* const Ks = lds;
  half_t* const Vts = lds + 2 * K_TILE_HALFS;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, hi = lane >> 5;
  const int nqb = (p.Nq + QB - 1) / QB;
  const int lin = xcd_remap(blockIdx.x, gridDim.x);
  constexpr int SL_SH = NSL == 4 ? 2 : 1;
  const int slice = lin & (NSL - 1);             // the slices of a query tile are neighbours: they read the same K stream
  const int qb = (lin >> SL_SH) % nqb;
  const int b = (lin >> SL_SH) / nqb;
  const int q_row = qb * QB + wave * 32 + l31;

  half8_t qf[NS];
  {
    const half_t* qp = p.Q + (long)b * p.q_bs + (long)min(q_row, p.Nq - 1) * p.ldq + hi * 8;
#pragma unroll
    for (int s = 0; s < NS; ++s) qf[s] = *reinterpret_cast<const half8_t*>(qp + s * 16);
  }
  float16_t o32[ND];
#pragma unroll
  for (int i = 0; i < ND; ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) o32[i][r] = 0.f;
  float m_run = -INFINITY, l_run = 0.f;
  const float c = p.scale_log2;

  // staging: thread t moves K chunks t + 256 j (row = chunk / 64, 16-byte column = chunk % 64) and V^T chunks t + 256 j
  // (row = chunk / 4 of the slice, 8-key column = chunk % 4); the source pointers advance by a constant per tile
  const half_t* kptr[K_PT];
  const half_t* vptr[V_PT];
  int k_lds[K_PT], v_lds[V_PT];
#pragma unroll
  for (int j = 0; j < K_PT; ++j) {
    const int ch = tid + NTHR * j, row = ch >> 6, cc = ch & 63;
    k_lds[j] = row * K_LD + cc * 8;
    kptr[j] = p.K + (long)b * p.k_bs + (long)row * p.ldk + cc * 8;
  }
#pragma unroll
  for (int j = 0; j < V_PT; ++j) {
    const int ch = tid + NTHR * j, d = ch >> 2, cc = ch & 3;
    v_lds[j] = d * VT_LD + cc * 8;
    vptr[j] = p.Vt + (long)(slice * DVC + d) * p.ldvt + (long)b * p.vt_bs + cc * 8;
  }
  u32x4 kreg[K_PT], vreg[V_PT];
  auto load_tile = [&]() __attribute__((always_inline)) {
#pragma unroll
    for (int j = 0; j < K_PT; ++j) {
      kreg[j] = *reinterpret_cast<const u32x4*>(kptr[j]);
      kptr[j] += (long)KV_TILE * p.ldk;
    }
#pragma unroll
    for (int j = 0; j < V_PT; ++j) {
      vreg[j] = *reinterpret_cast<const u32x4*>(vptr[j]);
      vptr[j] += KV_TILE;
    }
  };
  auto store_tile = [&](int stage) __attribute__((always_inline)) {
    half_t* Kd = Ks + stage * K_TILE_HALFS;
    half_t* Vd = Vts + stage * V_TILE_HALFS;
#pragma unroll
    for (int j = 0; j < K_PT; ++j) *reinterpret_cast<u32x4*>(Kd + k_lds[j]) = kreg[j];
#pragma unroll
    for (int j = 0; j < V_PT; ++j) {   // 72-byte rows are 8-byte aligned only
      *reinterpret_cast<uint2*>(Vd + v_lds[j]) = make_uint2(vreg[j][0], vreg[j][1]);
      *reinterpret_cast<uint2*>(Vd + v_lds[j] + 4) = make_uint2(vreg[j][2], vreg[j][3]);
    }
  };
  auto compute_tile = [&](int stage) __attribute__((always_inline)) {
    const half_t* Kt = Ks + stage * K_TILE_HALFS;
    const half_t* Vt = Vts + stage * V_TILE_HALFS;
    float16_t st;
#pragma unroll
    for (int r = 0; r < 16; ++r) st[r] = 0.f;
    const half_t* kp = Kt + l31 * K_LD + hi * 8;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const half8_t kf = *reinterpret_cast<const half8_t*>(kp + s * 16);
      st = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf, qf[s], st, 0, 0, 0);
    }
    float mx = st[0];
#pragma unroll
    for (int r = 1; r < 16; ++r) mx = fmaxf(mx, st[r]);
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float m_new = fmaxf(m_run, mx);
    if (__any(m_new > m_run)) {
      const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * c);   // 0 on the first tile, 1 where the maximum stayed
      l_run *= alpha;
#pragma unroll
      for (int i = 0; i < ND; ++i)
#pragma unroll
        for (int r = 0; r < 16; ++r) o32[i][r] *= alpha;
      m_run = m_new;
    }
    const float mc = m_run * c;
    float rs = 0.f;
    half8_t pf[2];
#pragma unroll
    for (int bb = 0; bb < 2; ++bb)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float e = __builtin_amdgcn_exp2f(fmaf(st[bb * 8 + j], c, -mc));
        rs += e;
        pf[bb][j] = (half_t)e;
      }
    rs += __shfl_xor(rs, 32, 64);
    l_run += rs;
    // P^T slot j of lane half hi in 16-key block bb is key 16 bb + 8 (j / 4) + 4 hi + j % 4: read V^T in that order
#pragma unroll
    for (int i = 0; i < ND; ++i) {
      const half_t* vp = Vt + (i * 32 + l31) * VT_LD + 4 * hi;
#pragma unroll
      for (int bb = 0; bb < 2; ++bb) {
        const half4_t lo4 = *reinterpret_cast<const half4_t*>(vp + bb * 16);
        const half4_t hi4 = *reinterpret_cast<const half4_t*>(vp + bb * 16 + 8);
        half8_t vf;
        vf[0] = lo4[0]; vf[1] = lo4[1]; vf[2] = lo4[2]; vf[3] = lo4[3];
        vf[4] = hi4[0]; vf[5] = hi4[1]; vf[6] = hi4[2]; vf[7] = hi4[3];
        o32[i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf, pf[bb], o32[i], 0, 0, 0);
      }
    }
  };

  const int ntiles = p.Nk / KV_TILE;
  load_tile();
  store_tile(0);
  __syncthreads();
  for (int t = 0; t + 1 < ntiles; ++t) {
    load_tile();
    __builtin_amdgcn_sched_barrier(0);   // the next tile's loads stay in front of this tile's MFMAs (left alone, the
    compute_tile(t & 1);                 // scheduler sinks them behind the QK^T chain to shorten their live ranges)
    store_tile((t & 1) ^ 1);
    __syncthreads();
  }
  compute_tile((ntiles - 1) & 1);

  if (q_row < p.Nq) {
    const float inv = 1.0f / l_run;
    half_t* op = p.O + (long)b * p.o_bs + (long)q_row * p.ldo + slice * DVC;
#pragma unroll
    for (int i = 0; i < ND; ++i)
#pragma unroll
      for (int rq = 0; rq < 4; ++rq) {
        half4_t o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = (half_t)(o32[i][rq * 4 + e] * inv);
        *reinterpret_cast<half4_t*>(op + i * 32 + 8 * rq + 4 * hi) = o;
      }
  }
}

// One launch of a (D, waves) build of the kernel text over the caller's parameter block
template <int D, int NWAVES, bool PV16, bool FOLD, class P>
void launch2(const P& p, dim3 grid, hipStream_t s) {
  if constexpr (std::is_same_v<P, AttnParamsKB>)
    hipLaunchKernelGGL((attention_kbias_kernel<D, NWAVES, PV16, FOLD>), grid, dim3(64 * NWAVES), 0, s, p);
  else if constexpr (std::is_same_v<P, AttnParamsRB>)
    hipLaunchKernelGGL((attention_rbias_kernel<D, NWAVES, PV16, FOLD>), grid, dim3(64 * NWAVES), 0, s, p);
  else
    hipLaunchKernelGGL((attention2_kernel<D, NWAVES, PV16, FOLD>), grid, dim3(64 * NWAVES), 0, s, p);
}

// The class the plan chose at head dim D.  Only the builds attn_plan() can name are instantiated: attention3_kernel, d = 96 and
// d = 512 for the plain block only, no 8-wave build for the block with a row per region.
template <int D, class P>
void launch_class(const P& p, const AttnPlan& pl, dim3 grid, hipStream_t s) {
  constexpr bool plain = std::is_same_v<P, AttnParams>, regions = std::is_same_v<P, AttnParamsRB>;
  if constexpr (!plain && (D == 96 || D == 512)) {
    // (never reached: the plan declines these)
  } else if constexpr (D == 512) {
    if (pl.slices == 2) hipLaunchKernelGGL(attention512_kernel<2>, grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL(attention512_kernel<4>, grid, dim3(256), 0, s, p);
  } else {
    if constexpr (D == 40 && plain)
      if (pl.cls == ATTN_A3) return pfd_attention3_launch(p, grid, s);
    if constexpr (D == 40 && !regions)
      if (pl.cls == ATTN_W8) return launch2<D, 8, true, true>(p, grid, s);
    launch2<D, 4, false, false>(p, grid, s);
  }
}

// The launcher of the three entry points: plan, one profiling bracket, one grid, the kernel, the launch check under `label`
template <class P>
int launch(const P& p, const char* label, hipStream_t s) {
  constexpr AttnOperand op = std::is_same_v<P, AttnParamsKB> ? ATTN_KBIAS : std::is_same_v<P, AttnParamsRB> ? ATTN_RBIAS : ATTN_PLAIN;
  const AttnPlan pl = attn_plan(p.B, p.H, p.Nq, p.Nk, p.D, op, attn_hooks(p.D));
  if (pl.rc != PFD_OK) return pl.rc;
  const bool prof = pfd_prof_on();
  if (prof)
    pfd_prof_begin(8, 4.0 * p.B * p.H * (double)p.Nq * p.Nk * p.D,
                   2.0 * p.B * p.H * p.D * (2.0 * p.Nq + 2.0 * p.Nk), s);
  dim3 grid(((p.Nq + pl.qb - 1) / pl.qb) * pl.slices * p.H * p.B);
  switch (p.D) {   // (the plan has declined every other D)
    case 40: launch_class<40>(p, pl, grid, s); break;
    case 80: launch_class<80>(p, pl, grid, s); break;
    case 96: launch_class<96>(p, pl, grid, s); break;
    case 160: launch_class<160>(p, pl, grid, s); break;
    case 512: launch_class<512>(p, pl, grid, s); break;
  }
  if (prof) pfd_prof_end(s);
  return pfd_check_launch(label);
}

int check_desc(const PfdAttnDesc* d) {
  if (!d || !d->Q || !d->K || !d->Vt || !d->O) return PFD_EINVAL;
  if (d->B <= 0 || d->H <= 0 || d->Nq <= 0 || d->Nk <= 0) return PFD_EINVAL;
  if ((d->ldq & 7) || (d->ldk & 7) || (d->ldo & 7) || (d->ldvt & 7) || (d->vt_bs & 7) || (d->q_bs & 7) ||
      (d->k_bs & 7) || (d->o_bs & 7))
    return PFD_EINVAL;
  if ((reinterpret_cast<uintptr_t>(d->Q) & 15) || (reinterpret_cast<uintptr_t>(d->K) & 15) ||
      (reinterpret_cast<uintptr_t>(d->Vt) & 15) || (reinterpret_cast<uintptr_t>(d->O) & 15))
    return PFD_EINVAL;
  return PFD_OK;
}

void fill_params(const PfdAttnDesc* d, AttnParams& p) {
  p.Q = (const half_t*)d->Q; p.K = (const half_t*)d->K; p.Vt = (const half_t*)d->Vt; p.O = (half_t*)d->O;
  p.ldq = d->ldq; p.ldk = d->ldk; p.ldvt = d->ldvt; p.ldo = d->ldo;
  p.q_bs = d->q_bs; p.k_bs = d->k_bs; p.vt_bs = d->vt_bs; p.o_bs = d->o_bs;
  p.B = d->B; p.H = d->H; p.Nq = d->Nq; p.Nk = d->Nk; p.D = d->D;
  p.scale_log2 = d->scale * 1.4426950408889634f;
}

}  // namespace

extern "C" int pfd_attention_kbias_f16(const PfdAttnDesc* d, const float* kbias, int64_t kb_bs, pfd_stream_t stream) {
  if (const int rc = check_desc(d)) return rc;
  if (!kbias || (reinterpret_cast<uintptr_t>(kbias) & 15) || (kb_bs & 3) || kb_bs < d->Nk) return PFD_EINVAL;
  if (!(d->scale > 0.f)) return PFD_EINVAL;   // the logits are divided by scale log2(e) where the score is raw
  AttnParamsKB p;
  fill_params(d, p);
  p.kbias = kbias;
  p.kb_bs = kb_bs;
  p.inv_scale_log2 = 1.0f / p.scale_log2;
  return launch(p, "pfd_attention_kbias_f16", (hipStream_t)stream);
}

extern "C" int pfd_attention_rbias_f16(const PfdAttnDesc* d, const float* rbias, int64_t rb_rs, int64_t rb_bs, int nr,
                                       const uint8_t* qregion, int64_t qr_bs, pfd_stream_t stream) {
  if (const int rc = check_desc(d)) return rc;
  if (nr < 1 || nr > ATTN_MAX_REGIONS) return PFD_EINVAL;
  if (!rbias || (reinterpret_cast<uintptr_t>(rbias) & 15) || (rb_rs & 3) || rb_rs < d->Nk) return PFD_EINVAL;
  if ((rb_bs & 3) || (rb_bs != 0 && rb_bs < (int64_t)nr * rb_rs)) return PFD_EINVAL;   // 0: one table for the batch
  if (!qregion || (qr_bs != 0 && qr_bs < d->Nq)) return PFD_EINVAL;
  if (!(d->scale > 0.f)) return PFD_EINVAL;
  AttnParamsRB p;
  fill_params(d, p);
  p.rbias = rbias;
  p.rb_rs = rb_rs;
  p.rb_bs = rb_bs;
  p.qregion = qregion;
  p.qr_bs = qr_bs;
  p.nr = nr;
  p.inv_scale_log2 = 1.0f / p.scale_log2;
  p.m_start = -0x1p100f * p.inv_scale_log2;   // -2^100 log2 units as a raw score
  // (the start value must be finite as a raw score, 2^100 / (scale log2 e) < 2^128, and far below every real score; the header
  //  states the range it promises, 2^-28 < scale log2 e < 2^10 -- the head sizes served have scale = d^-1/2)
  if (!(p.scale_log2 > 0x1p-28f) || !(p.scale_log2 < 0x1p10f)) return PFD_EINVAL;
  return launch(p, "pfd_attention_rbias_f16", (hipStream_t)stream);
}

extern "C" int pfd_attention_f16(const PfdAttnDesc* d, pfd_stream_t stream) {
  if (const int rc = check_desc(d)) return rc;
  AttnParams p;
  fill_params(d, p);
  return launch(p, "pfd_attention_f16", (hipStream_t)stream);
}
