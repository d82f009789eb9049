// The body of attention2_kernel (csrc/attention.hip holds its description), compiled three times from there:
//   ATTN2_KERNEL_NAME = attention2_kernel,      ATTN2_PARAMS = AttnParams,   ATTN2_KBIAS = false                      (pfd_attention_f16)
//   ATTN2_KERNEL_NAME = attention_kbias_kernel, ATTN2_PARAMS = AttnParamsKB, ATTN2_KBIAS = true                       (pfd_attention_kbias_f16)
//   ATTN2_KERNEL_NAME = attention_rbias_kernel, ATTN2_PARAMS = AttnParamsRB, ATTN2_KBIAS = true, ATTN2_RBIAS = true   (pfd_attention_rbias_f16)
// (why two __global__ templates from one text and not a fifth template parameter: DESIGN.md 3.20)
template <int D, int NWAVES, bool PV16, bool FOLD = false>
__global__ __launch_bounds__(NWAVES * 64, (D <= 40 ? 4 : 1)) void ATTN2_KERNEL_NAME(const ATTN2_PARAMS p) {
  constexpr bool KBIAS = ATTN2_KBIAS;
  constexpr bool RBIAS = ATTN2_RBIAS;   // the logits of a key depend on the region of the query: KBIAS with a row per region
  static_assert(!RBIAS || (KBIAS && !FOLD), "the regional build stages rows like KBIAS; no folded form of it is built");
  static_assert(!PV16 || D == 40, "the 16x16x32 PV path is laid out for d = 40 (48 padded rows, row 40 = ones)");
  static_assert(!FOLD || D == 40, "the folded maximum uses contraction slot 40 of the d = 40 build (DQK = 48)");
  constexpr int KV_TILE = 64, NU = 2;
  constexpr int NTHR = NWAVES * 64;
  constexpr int QB = NWAVES * 32;
  constexpr int DQK = (D + 15) / 16 * 16;
  constexpr int DV = PV16 ? 48 : (D + 31) / 32 * 32;
  constexpr int VT_LD = PV16 ? KV_TILE : KV_TILE + 4;
  constexpr int K_LD = DQK + 8;
  constexpr int NS = DQK / 16;
  constexpr int ND = DV / 32;        // 32-row O^T tiles (PV on 32x32x16)
  constexpr int NDT = DV / 16;       // 16-row O^T tiles (PV on 16x16x32)
  constexpr bool SUM_MFMA = DV > D;
  constexpr int KCH = D / 8;
  constexpr int K_CHUNKS = KV_TILE * KCH;
  constexpr int V_CHUNKS = D * (KV_TILE / 8);
  constexpr int K_PT = (K_CHUNKS + NTHR - 1) / NTHR;
  constexpr int V_PT = (V_CHUNKS + NTHR - 1) / NTHR;
  constexpr int K_TILE_HALFS = KV_TILE * K_LD;
  constexpr int V_TILE_HALFS = DV * VT_LD;
  constexpr int KB_ROWS = RBIAS ? ATTN_MAX_REGIONS : 1;
  constexpr int KB_HALFS = KBIAS ? 2 * KB_ROWS * KV_TILE * 2 : 0;   // two stages of (rows of) 64 fp32 key logits behind the V^T images
  constexpr int RG_HALFS = RBIAS ? QB * 2 : 0;            // RBIAS: per query of the block, where its region's row starts in a stage
  __shared__ __attribute__((aligned(16))) half_t lds[2 * K_TILE_HALFS + 2 * V_TILE_HALFS + KB_HALFS + RG_HALFS];
  half_t* const Ks = lds;
  half_t* const Vts = lds + 2 * K_TILE_HALFS;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, hi = lane >> 5;
  const int nqb = (p.Nq + QB - 1) / QB;
  const int lin = xcd_remap(blockIdx.x, gridDim.x);
  const int bh = lin / nqb;
  const int qb = lin - bh * nqb;
  const int b = bh / p.H, h = bh - b * p.H;
  const int q_row = qb * QB + wave * 32 + l31;

  if constexpr (RBIAS) {
    // the region of each of the block's QB queries, once, as the float offset of its row inside a stage (ids are clamped to the
    // rows that are staged: the host refuses others, and a wild byte must not read LDS nobody wrote).  Visible behind the barrier
    // of the clear below; compute_tile re-reads its lane's entry per tile instead of keeping it live across the loop.
    int* const Rg = reinterpret_cast<int*>(lds + 2 * K_TILE_HALFS + 2 * V_TILE_HALFS + KB_HALFS);
    if (tid < QB) Rg[tid] = min((int)attn_qregion(p, b)[min(qb * QB + tid, p.Nq - 1)], attn_nr(p) - 1) * KV_TILE;
  }
  static_assert((2 * K_TILE_HALFS + 2 * V_TILE_HALFS) % 8 == 0, "16-byte clears");
  for (int i = tid; i < (2 * K_TILE_HALFS + 2 * V_TILE_HALFS) / 8; i += NTHR)
    reinterpret_cast<uint4*>(lds)[i] = make_uint4(0, 0, 0, 0);
  __syncthreads();
  if (SUM_MFMA) {   // row D of V^T = 1: O^T[D, q] accumulates sum_kv P (every slot of the row, so the swizzle is moot)
    for (int i = tid; i < 2 * KV_TILE; i += NTHR)
      Vts[(i / KV_TILE) * V_TILE_HALFS + D * VT_LD + (i % KV_TILE)] = (half_t)1.f;
  }
  if (FOLD) {       // column D of K = 1 in both stages (the staging writes columns 0 .. D - 1 only)
    for (int i = tid; i < 2 * KV_TILE; i += NTHR)
      Ks[(i / KV_TILE) * K_TILE_HALFS + (i % KV_TILE) * K_LD + D] = (half_t)1.f;
  }

  half8_t qf[NS];
  {
    const half_t* qp = p.Q + (long)b * p.q_bs + (long)min(q_row, p.Nq - 1) * p.ldq + h * D;
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      const int d = s * 16 + hi * 8;
      Pack16 t;
      t.u = *reinterpret_cast<const uint4*>(qp + min(d, D - 8));   // unconditional; padding slots zeroed below
      if (d >= D) t.u = make_uint4(0, 0, 0, 0);
      qf[s] = t.h;
      if (FOLD) {
#pragma unroll
        for (int e = 0; e < 8; ++e) qf[s][e] = (half_t)((float)qf[s][e] * p.scale_log2);
      }
    }
  }
  bool first_tile = true;   // FOLD: the first tile always sets the folded maximum

  float16_t o32[PV16 ? 1 : ND];          // PV on 32x32x16: O^T tile i, col = q = l31
  float4_t o16[PV16 ? NDT : 1][2];       // PV on 16x16x32: [d tile][q tile], col = q % 16 = lane & 15, rows 4 (lane >> 4) + r
#pragma unroll
  for (int i = 0; i < (PV16 ? 1 : ND); ++i)
#pragma unroll
    for (int r = 0; r < 16; ++r) o32[i][r] = 0.f;
#pragma unroll
  for (int i = 0; i < (PV16 ? NDT : 1); ++i)
#pragma unroll
    for (int q = 0; q < 2; ++q) o16[i][q] = (float4_t){0.f, 0.f, 0.f, 0.f};
  // RBIAS: a query whose region masks the leading key tiles meets mx = -inf there.  Its running maximum therefore starts at a
  // large FINITE negative value (p.m_start, -2^100 log2 units) and is finite ever after: m_new = fmaxf(finite, .) is finite, a
  // masked tile leaves it alone and gives p = exp2(fma(-inf, c, finite)) = 0, the first live tile rescales the (zero)
  // accumulators by exp2(-huge) = 0 exactly as the start at -inf does.  No (-inf) - (-inf) can be formed, per lane.
  float m_run = FOLD ? 0.f : (RBIAS ? attn_m_start(p) : -INFINITY), l_run = 0.f;

  const half_t* kbase = p.K + (long)b * p.k_bs + h * D;
  const half_t* vbase = p.Vt + (long)h * D * p.ldvt + (long)b * p.vt_bs;
  const float c = p.scale_log2;
  float inv_c = 0.f;        // KBIAS, raw scores: kbias / c is in their units (-inf stays -inf: c > 0)
  if constexpr (KBIAS) inv_c = attn_inv_scale_log2(p);

  // ---- staging: chunk = 16 bytes; thread t moves K chunks t + NTHR j and V^T chunks (t + NTHR / 2) % NTHR + NTHR j ----
  // (inactive slots load a clamped, valid chunk and do not store it: no branch around a load.  Row / chunk indices are
  //  recomputed where the ragged tile needs them: kept live they cost the d = 40 build its 128-register budget.)
  auto k_chunk = [&](int j, int& row, int& cc, int tid) __attribute__((always_inline)) {
    const int chc = min(tid + NTHR * j, K_CHUNKS - 1);
    row = chc / KCH;
    cc = chc - row * KCH;
  };
  auto v_chunk = [&](int j, int& d, int& cc, int tid) __attribute__((always_inline)) {
    const int chc = min(((tid + NTHR / 2) & (NTHR - 1)) + NTHR * j, V_CHUNKS - 1);
    d = chc / (KV_TILE / 8);
    cc = chc % (KV_TILE / 8);
  };
  int k_lds[K_PT], v_lds0[V_PT];
  bool k_on[K_PT], v_on[V_PT];
  const half_t* kptr[K_PT];
  const half_t* vptr[V_PT];
#pragma unroll
  for (int j = 0; j < K_PT; ++j) {
    int row, cc;
    k_chunk(j, row, cc, tid);
    k_on[j] = tid + NTHR * j < K_CHUNKS;
    k_lds[j] = row * K_LD + cc * 8;
    kptr[j] = kbase + (long)row * p.ldk + cc * 8;
  }
#pragma unroll
  for (int j = 0; j < V_PT; ++j) {
    int d, cc;
    v_chunk(j, d, cc, tid);
    v_on[j] = ((tid + NTHR / 2) & (NTHR - 1)) + NTHR * j < V_CHUNKS;
    if (PV16) {
      const int dl_ = d & 15;
      const int sg_ = ((dl_ >> 1) & 3) | (((dl_ >> 3) & 1) << 3);
      v_lds0[j] = d * VT_LD + 4 * ((2 * cc) ^ sg_);   // second 8-byte half: slot (2 cc + 1) ^ sigma = this address ^ 4 halfs
    } else {
      v_lds0[j] = d * VT_LD + cc * 8;                 // second half: + 4 halfs
    }
    vptr[j] = vbase + (long)d * p.ldvt + cc * 8;
  }
  const int v_last = max(0, ((p.Nk + 7) & ~7) - 8);
  // (first-class vector values, not the uint4 struct: a struct copy global -> private -> LDS is folded by the compiler's
  //  memcpy forwarding into ONE copy at the store point, i.e. the prefetch load lands right in front of its ds_write)
  u32x4 kregA[K_PT], vregA[V_PT];
  // KBIAS: the 64 logits of a tile go global -> LDS by ONE LDS-DMA instruction of the first wave (lane l's dword lands at
  // base + 4 l), issued with the tile's K / V^T loads into the stage that tile will occupy -- nobody reads that stage before
  // the barrier behind this tile's compute, and the DMA needs no register to wait in (the d = 40 builds have none to spare).
  // It completes in issue order with the loads behind it; the vmcnt(0) in front of each barrier says so explicitly.
  float* const Kbs = reinterpret_cast<float*>(lds + 2 * K_TILE_HALFS + 2 * V_TILE_HALFS);
  const float* kbrow = nullptr;
  int kb_next = 0;          // wave-uniform: the first key of the tile load_full stands on
  if constexpr (KBIAS) kbrow = attn_kbias_row(p, b);
  // (src = a wave-uniform base + a lane offset taken from an opaque value at every call: otherwise the loop carries a
  //  per-thread 64-bit pointer and a per-thread tile counter -- three registers the d = 40 build spills for)
  auto stage_kbias = [&](const float* base, int off_max, int kv0) __attribute__((always_inline)) {
    if constexpr (RBIAS) {   // row g of the table by wave g % NWAVES: one LDS-DMA dword load per row, into row g of the stage
      int ln = tid;
      asm volatile("" : "+v"(ln));
      const int w0 = __builtin_amdgcn_readfirstlane(ln >> 6);
#pragma unroll
      for (int i = 0; i < (ATTN_MAX_REGIONS + NWAVES - 1) / NWAVES; ++i) {
        const int g = w0 + i * NWAVES;
        if (g < attn_nr(p))
          __builtin_amdgcn_global_load_lds(
              (const __attribute__((address_space(1))) void*)(base + (long)g * attn_rb_rs(p) + min(ln & 63, off_max)),
              (__attribute__((address_space(3))) void*)(Kbs + (((kv0 >> 6) & 1) * KB_ROWS + g) * KV_TILE), 4, 0, 0);
      }
    } else if (__builtin_amdgcn_readfirstlane(wave) == 0) {
      int ln = tid;
      asm volatile("" : "+v"(ln));
      __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(base + min(ln & 63, off_max)),
                                       (__attribute__((address_space(3))) void*)(Kbs + ((kv0 >> 6) & 1) * KV_TILE), 4, 0, 0);
    }
  };

  auto load_full = [&](u32x4* kreg, u32x4* vreg) __attribute__((always_inline)) {   // the tile the pointers stand on
    if constexpr (KBIAS) {
      stage_kbias(kbrow + kb_next, KV_TILE - 1, kb_next);
      kb_next += KV_TILE;
    }
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
  auto load_ragged = [&](u32x4* kreg, u32x4* vreg, int kv0) __attribute__((always_inline)) {   // clamped to valid rows / chunks
    // KBIAS: the thread index of the ragged tile is opaque, so its row / chunk arithmetic is done here, behind the loop, instead
    // of being hoisted in front of it and kept live across it (the d = 40 build has no register for that: it went to scratch)
    int tr = tid;
    if constexpr (KBIAS) {
      asm volatile("" : "+v"(tr));
      stage_kbias(kbrow + kv0, p.Nk - 1 - kv0, kv0);   // keys past Nk: the last valid address, masked in compute_tile
    }
#pragma unroll
    for (int j = 0; j < K_PT; ++j) {
      int row, cc;
      k_chunk(j, row, cc, tr);
      kreg[j] = *reinterpret_cast<const u32x4*>(kbase + (long)min(kv0 + row, p.Nk - 1) * p.ldk + cc * 8);
    }
#pragma unroll
    for (int j = 0; j < V_PT; ++j) {
      int d, cc;
      v_chunk(j, d, cc, tr);
      vreg[j] = *reinterpret_cast<const u32x4*>(vbase + (long)d * p.ldvt + min(kv0 + cc * 8, v_last));
    }
  };
  // RAG is a constant at every call site (the lambdas are not generic on purpose: a generic lambda is inlined too late
  // for the staging arrays to be promoted to registers)
  auto store_tile = [&](const u32x4* kreg, const u32x4* vreg, int stage, const bool RAG, int kv0) __attribute__((always_inline)) {
    half_t* Kd = Ks + stage * K_TILE_HALFS;
    half_t* Vd = Vts + stage * V_TILE_HALFS;
#pragma unroll
    for (int j = 0; j < K_PT; ++j)
      if (k_on[j]) *reinterpret_cast<u32x4*>(Kd + k_lds[j]) = kreg[j];
#pragma unroll
    for (int j = 0; j < V_PT; ++j) {
      unsigned w0 = vreg[j][0], w1 = vreg[j][1], w2 = vreg[j][2], w3 = vreg[j][3];
      if (RAG) {   // keys past Nk: P is 0 there, but 0 x NaN garbage must not reach the accumulator
        int d, cc, tr = tid;
        if constexpr (KBIAS) asm volatile("" : "+v"(tr));
        v_chunk(j, d, cc, tr);
        const int valid = p.Nk - (kv0 + cc * 8);
        w0 = valid >= 2 ? w0 : (valid == 1 ? (w0 & 0xFFFFu) : 0u);
        w1 = valid >= 4 ? w1 : (valid == 3 ? (w1 & 0xFFFFu) : 0u);
        w2 = valid >= 6 ? w2 : (valid == 5 ? (w2 & 0xFFFFu) : 0u);
        w3 = valid >= 8 ? w3 : (valid == 7 ? (w3 & 0xFFFFu) : 0u);
      }
      if (v_on[j]) {
        *reinterpret_cast<uint2*>(Vd + v_lds0[j]) = make_uint2(w0, w1);
        *reinterpret_cast<uint2*>(Vd + (PV16 ? v_lds0[j] ^ 4 : v_lds0[j] + 4)) = make_uint2(w2, w3);
      }
    }
  };

  // V^T fragment addressing of the 16x16x32 path (halfs, relative to the tile): row dl, slots (4 bb + hi) and + 2
  const int dl = lane & 15, kg = lane >> 4;
  const int sg = ((dl >> 1) & 3) | (((dl >> 3) & 1) << 3);
  const int x0 = (4 * (kg & 1) + (kg >> 1)) ^ (sg & 7), x1 = (4 * (kg & 1) + (kg >> 1) + 2) ^ (sg & 7);
  const int u_flip = sg >> 3;
  const int vrow16 = dl * VT_LD;

  auto compute_tile = [&](int stage, const bool RAG, int kv0) __attribute__((always_inline)) {
    const half_t* Kt = Ks + stage * K_TILE_HALFS;
    const half_t* Vt = Vts + stage * V_TILE_HALFS;
    float16_t st[NU];
    int roff = 0;             // RBIAS: the row of the lane's own region (the reads below are then no broadcasts)
    if constexpr (RBIAS) {
      int tq = tid;
      asm volatile("" : "+v"(tq));
      roff = reinterpret_cast<const int*>(Kbs + 2 * KB_ROWS * KV_TILE)[(tq >> 6) * 32 + (tq & 31)];
    }
#pragma unroll
    for (int u = 0; u < NU; ++u) {
      if constexpr (KBIAS) {
        // the accumulator STARTS at the key's logit, in the units of the score: the QK^T MFMAs add it for nothing, and the
        // four broadcast 16-byte reads land in the registers that are the accumulator anyway (rows (r & 3) + 8 (r >> 2) + 4 hi
        // are four runs of four consecutive keys).  RBIAS: the same four reads from the row of the lane's region -- a broadcast
        // only among the lanes of one region; rows are 256 bytes apart, so lanes of different regions meet in the same banks
        // and a read takes up to as many passes as there are regions in the half-wave (measured: profiles/regions.md)
        const float* kb = Kbs + stage * (KB_ROWS * KV_TILE) + roff + u * 32 + 4 * hi;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
          const float4_t bv = *reinterpret_cast<const float4_t*>(kb + 8 * g);
#pragma unroll
          for (int e = 0; e < 4; ++e) st[u][4 * g + e] = FOLD ? bv[e] : bv[e] * inv_c;
        }
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) st[u][r] = 0.f;
      }
      const half_t* kp = Kt + (u * 32 + l31) * K_LD + hi * 8;
#pragma unroll
      for (int s = 0; s < NS; ++s) {
        const half8_t kf = *reinterpret_cast<const half8_t*>(kp + s * 16);
        st[u] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf, qf[s], st[u], 0, 0, 0);
      }
    }
    if (RAG) {
#pragma unroll
      for (int u = 0; u < NU; ++u)
#pragma unroll
        for (int r = 0; r < 16; ++r)
          if (kv0 + u * 32 + mfma32_row(r, hi) >= p.Nk) st[u][r] = -INFINITY;
    }
    float mx = st[0][0];
#pragma unroll
    for (int u = 0; u < NU; ++u)
#pragma unroll
      for (int r = 0; r < 16; ++r) mx = fmaxf(mx, st[u][r]);
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    auto rescale_o = [&](float alpha) __attribute__((always_inline)) {
      if constexpr (PV16) {
        const float a0 = __shfl(alpha, dl, 64), a1 = __shfl(alpha, dl + 16, 64);   // accumulator columns: q = dl + 16 qt
#pragma unroll
        for (int i = 0; i < NDT; ++i)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            o16[i][0][r] *= a0;
            o16[i][1][r] *= a1;
          }
      } else {
#pragma unroll
        for (int i = 0; i < ND; ++i)
#pragma unroll
          for (int r = 0; r < 16; ++r) o32[i][r] *= alpha;
      }
    };
    float rs = 0.f;
    half8_t pf[NU][2];
    if constexpr (FOLD) {
      // st = s' - m_run already (m_run: the f16-representable maximum folded into the query fragment; 0 before the first tile)
      if (first_tile || __any(mx > 6.0f)) {
        const bool up = first_tile || mx > 0.f;
        const float m_new = up ? (float)(half_t)(m_run + mx) : m_run;
        const float delta = m_new - m_run;                       // exact: both are f16 values
        rescale_o(__builtin_amdgcn_exp2f(-delta));               // (accumulators are 0 on the first tile)
#pragma unroll
        for (int u = 0; u < NU; ++u)
#pragma unroll
          for (int r = 0; r < 16; ++r) st[u][r] -= delta;
        m_run = m_new;
        if (hi) qf[NS - 1][0] = (half_t)(-m_new);                // contraction slot D = 40: k block 2, upper lane half, element 0
        first_tile = false;
      }
#pragma unroll
      for (int u = 0; u < NU; ++u)
#pragma unroll
        for (int bb = 0; bb < 2; ++bb)
#pragma unroll
          for (int j = 0; j < 8; ++j) pf[u][bb][j] = (half_t)__builtin_amdgcn_exp2f(st[u][bb * 8 + j]);
    } else {
      const float m_new = fmaxf(m_run, mx);
      if (__any(m_new > m_run)) {
        const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * c);   // 1 for rows whose max did not move; 0 at the start
        l_run *= alpha;
        rescale_o(alpha);
        m_run = m_new;
      }
      const float mc = m_run * c;
#pragma unroll
      for (int u = 0; u < NU; ++u)
#pragma unroll
        for (int bb = 0; bb < 2; ++bb)
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const float e = __builtin_amdgcn_exp2f(fmaf(st[u][bb * 8 + j], c, -mc));
            if (!SUM_MFMA) rs += e;
            pf[u][bb][j] = (half_t)e;
          }
    }
    if (!SUM_MFMA) {
      rs += __shfl_xor(rs, 32, 64);
      l_run += rs;
    }
    if constexpr (PV16) {
      union H8 {
        half8_t h;
        unsigned w[4];
      };
      half8_t pb[NU][2];   // [32-key half][q tile]
#pragma unroll
      for (int u = 0; u < NU; ++u) {
        H8 a, bq, r0, r1;
        a.h = pf[u][0];
        bq.h = pf[u][1];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const auto sw = __builtin_amdgcn_permlane16_swap(a.w[k], bq.w[k], false, false);
          r0.w[k] = sw[0];   // rows: (q 0-15, hi 0, bb 0) (q 0-15, hi 0, bb 1) (q 0-15, hi 1, bb 0) (q 0-15, hi 1, bb 1)
          r1.w[k] = sw[1];   // the same for q 16-31
        }
        pb[u][0] = r0.h;
        pb[u][1] = r1.h;
      }
  #pragma unroll
      for (int i = 0; i < NDT; ++i)
#pragma unroll
        for (int u = 0; u < NU; ++u) {
          const half_t* vp = Vt + i * 16 * VT_LD + vrow16 + 32 * (u ^ u_flip);
          const half4_t lo4 = *reinterpret_cast<const half4_t*>(vp + 4 * x0);
          const half4_t hi4 = *reinterpret_cast<const half4_t*>(vp + 4 * x1);
          half8_t vf;
          vf[0] = lo4[0]; vf[1] = lo4[1]; vf[2] = lo4[2]; vf[3] = lo4[3];
          vf[4] = hi4[0]; vf[5] = hi4[1]; vf[6] = hi4[2]; vf[7] = hi4[3];
          o16[i][0] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vf, pb[u][0], o16[i][0], 0, 0, 0);
          o16[i][1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vf, pb[u][1], o16[i][1], 0, 0, 0);
        }
      } else {
#pragma unroll
      for (int i = 0; i < ND; ++i) {
        const half_t* vp = Vt + (i * 32 + l31) * VT_LD + 4 * hi;
#pragma unroll
        for (int u = 0; u < NU; ++u)
#pragma unroll
          for (int bb = 0; bb < 2; ++bb) {
            const half4_t lo4 = *reinterpret_cast<const half4_t*>(vp + u * 32 + bb * 16);
            const half4_t hi4 = *reinterpret_cast<const half4_t*>(vp + u * 32 + bb * 16 + 8);
            half8_t vf;
            vf[0] = lo4[0]; vf[1] = lo4[1]; vf[2] = lo4[2]; vf[3] = lo4[3];
            vf[4] = hi4[0]; vf[5] = hi4[1]; vf[6] = hi4[2]; vf[7] = hi4[3];
            o32[i] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf, pf[u][bb], o32[i], 0, 0, 0);
          }
      }
    }
  };

  const int nfull = p.Nk / KV_TILE;
  const bool rag = (p.Nk % KV_TILE) != 0;
  // first tile
  if (nfull > 0) {
    load_full(kregA, vregA);
    store_tile(kregA, vregA, 0, false, 0);
  } else {
    load_ragged(kregA, vregA, 0);
    store_tile(kregA, vregA, 0, true, 0);
  }
  __builtin_amdgcn_s_waitcnt(0x0F70);   // vmcnt(0) on every path into the loop (Q fragments included)
  __syncthreads();
  int t = 0;
  for (; t + 1 < nfull; ++t) {          // full tile followed by a full tile: the hot loop
    load_full(kregA, vregA);
    compute_tile(t & 1, false, 0);
    store_tile(kregA, vregA, (t & 1) ^ 1, false, 0);
    if constexpr (KBIAS) __builtin_amdgcn_s_waitcnt(0x0F70);
    __syncthreads();
  }
  if (nfull > 0) {                      // last full tile; its successor is the ragged tile or nothing
    if (rag) load_ragged(kregA, vregA, (t + 1) * KV_TILE);
    compute_tile(t & 1, false, 0);
    if (rag) store_tile(kregA, vregA, (t & 1) ^ 1, true, (t + 1) * KV_TILE);
    if constexpr (KBIAS) __builtin_amdgcn_s_waitcnt(0x0F70);
    __syncthreads();
    ++t;
  }
  if (rag) compute_tile(t & 1, true, t * KV_TILE);

  // ---- epilogue: O[q, d] = O^T[d, q] / l ----
  if constexpr (PV16) {
    // row 40 of O^T (d tile 2, local row 8 = lane row 2, register 0) = sum_kv P of query (lane & 15) + 16 qt
    const float l0 = __shfl(o16[2][0][0], 32 + dl, 64), l1 = __shfl(o16[2][1][0], 32 + dl, 64);
#pragma unroll
    for (int qt = 0; qt < 2; ++qt) {
      const int q = qb * QB + wave * 32 + qt * 16 + dl;
      const float inv = 1.0f / (qt ? l1 : l0);
      if (q < p.Nq) {
        half_t* op = p.O + (long)b * p.o_bs + (long)q * p.ldo + h * D;
#pragma unroll
        for (int i = 0; i < NDT; ++i) {
          const int d0 = i * 16 + 4 * kg;
          if (d0 < D) {
            half4_t o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = (half_t)(o16[i][qt][e] * inv);
            gst_t<PFD_ST_ATTN>(reinterpret_cast<half4_t*>(op + d0), o);
          }
        }
      }
    }
  } else {
    if (SUM_MFMA) {
      constexpr int lr = D % 32;
      constexpr int src_hi = (lr >> 2) & 1;
      constexpr int reg = (lr & 3) + 4 * (lr >> 3);
      const float v = o32[D / 32][reg];
      l_run = __shfl(v, src_hi * 32 + l31, 64);
    }
    int q_out = q_row;
    int hi_out = hi;
    if constexpr (KBIAS) {   // from an opaque thread index: row and offsets are formed here, not kept live across the loop
      int te = tid;
      asm volatile("" : "+v"(te));
      q_out = qb * QB + (te >> 6) * 32 + (te & 31);
      hi_out = (te >> 5) & 1;
    }
    if (q_out < p.Nq) {
      const float inv = 1.0f / l_run;
      half_t* op = p.O + (long)b * p.o_bs + (long)q_out * p.ldo + h * D;
#pragma unroll
      for (int i = 0; i < ND; ++i)
#pragma unroll
        for (int rq = 0; rq < 4; ++rq) {
          const int d0 = i * 32 + 8 * rq + 4 * hi_out;
          if (d0 < D) {
            half4_t o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = (half_t)(o32[i][rq * 4 + e] * inv);
            gst_t<PFD_ST_ATTN>(reinterpret_cast<half4_t*>(op + d0), o);
          }
        }
    }
  }
}

