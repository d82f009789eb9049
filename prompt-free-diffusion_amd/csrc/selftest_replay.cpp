// The launch-list replay of build/selftest (modes: selftest.cpp).
#include <array>

#include "selftest_util.h"

__global__ void count_mismatch_kernel(const unsigned short* a, const unsigned short* b, size_t n, unsigned* cnt) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  unsigned bad = 0;
  for (; i < n; i += (size_t)gridDim.x * blockDim.x) bad += a[i] != b[i];
  if (bad) atomicAdd(cnt, bad);
}

// --replay <file>: relaunch a recorded GEMM/conv launch list (tools/dump_unet_shapes.py) once each, in
// order, on random operands -- the torch-free workload rocprofv3 --pmc is pointed at.
int replay(const char* path, bool timed, int force_tile) {
  FILE* f = fopen(path, "r");
  if (!f) { printf("cannot open %s\n", path); return 1; }
  // one launch per line: 19 fields (rounds 1-3), 22 (+ k_split, zero_rows, gn_out != NULL) or 24 (+ gnf = 0 | 1 | 2 = fused
  // GroupNorm in the split-K reduction keeping / skipping the raw result, res_rows); shorter lines are padded with zeros
  std::vector<std::array<long, 24>> rows;
  char line[512];
  while (fgets(line, sizeof(line), f)) {
    std::array<long, 24> r{};
    int n = 0, off = 0, adv = 0;
    while (n < 24 && sscanf(line + off, "%ld%n", &r[n], &adv) == 1) { ++n; off += adv; }
    if (n != 19 && n != 22 && n != 24) break;
    rows.push_back(r);
  }
  fclose(f);
  size_t maxA = 0, maxW = 0, maxC = 0, maxV = 0;
  for (auto& q : rows) {
    const long M = q[0], N = q[1], K = q[2], ks = q[8];
    const size_t a = ks > 0 ? (size_t)q[12] * q[13] * q[14] * q[15] : (size_t)M * K;
    maxA = std::max(maxA, a); maxW = std::max(maxW, (size_t)N * K * (ks > 0 && q[11] == 2 ? 4 : 1)); maxC = std::max(maxC, (size_t)M * N);
    maxV = std::max(maxV, (size_t)std::max(M, N) * 4);
  }
  Dev<h16> dA(rand_h(maxA)), dW(rand_h(maxW, 0.05f)), dB(rand_h(maxV)), dRV(rand_h(maxC)), dR(rand_h(maxC)), dC(maxC), dY(maxC);
  Dev<float> dWS((size_t)24 << 20);
  size_t maxM = 1;
  for (auto& q : rows) maxM = std::max(maxM, (size_t)q[0]);
  Dev<float> dGnO((maxM / 64 + 1) * 8 * 16 * 2);   // PfdGemmDesc.gn_out: [M / 64][N / 160 <= 8][16] float2
  Dev<float> dLnS(rand_f(maxM * 16, 1.0f)), dLnC(rand_f(16384, 1.0f)), dLnO(maxM * 16);   // [M][<= 8][2] statistics, column sums
  {  // plausible statistics: sum ~ 0, sum of squares ~ K (so that rstd is finite)
    std::vector<float> st(maxM * 16);
    for (size_t i = 0; i < st.size(); i += 2) { st[i] = 0.5f; st[i + 1] = 200.f; }
    HIP_OK(hipMemcpy(dLnS.p, st.data(), st.size() * sizeof(float), hipMemcpyHostToDevice));
  }
  int bad = 0;
  // --replay-time: every launch reads its weights from a fresh slice of a 2 GB pool (as in the UNet,
  // where 1.7 GB of other layers' weights pass through the caches between two uses of a layer) and is
  // bracketed by its own pair of events; the table lists, per distinct problem, the time against the
  // per-problem roofline max(flops / 2.5 PF, algorithmic bytes / 8 TB/s).
  const size_t pool_elems = timed ? (size_t)1 << 30 : 0;
  Dev<h16> dPool(pool_elems ? pool_elems : 8);
  if (timed) HIP_OK(hipMemset(dPool.p, 0x11, pool_elems * 2));
  size_t pool_off = 0;
  const int reps = timed ? 4 : 2;
  std::vector<hipEvent_t> ev(timed ? rows.size() + 1 : 0);
  for (auto& e : ev) HIP_OK(hipEventCreate(&e));
  std::vector<double> acc_ms(rows.size(), 0.0);
  for (int rep = 0; rep < reps; ++rep) {  // first pass warms caches / code objects
    size_t li = 0;
    if (timed) HIP_OK(hipEventRecord(ev[0], nullptr));
    for (auto& q : rows) {
      PfdGemmDesc d = gemm_desc(dWS);
      d.M = q[0]; d.N = q[1]; d.K = q[2]; d.act = q[3];
      d.A = dA.p; d.W = dW.p; d.C = dC.p;
      d.bias = q[4] ? dB.p : nullptr; d.rowvec = q[5] ? dRV.p : nullptr; d.R = q[6] ? dR.p : nullptr;
      d.bias_per_row = q[7];
      d.ksize = q[8]; d.stride = q[9]; d.pad = q[10]; d.ups = q[11];
      d.B = q[12]; d.H = q[13]; d.Wd = q[14]; d.Cin = q[15]; d.Ho = q[16]; d.Wo = q[17];
      d.rows_per_rv = (int)std::min<long>(q[18], 1 << 30);
      const long nout = d.act == PFD_ACT_GEGLU ? d.N / 2 : d.N;
      d.lda = d.ksize > 0 ? d.Cin : d.K; d.ldw = d.K; d.ldc = nout; d.ldr = nout; d.ldrv = d.N;
      if (q[19] > 0) { d.k_split = (int)q[19]; d.A2 = dA.p + (size_t)d.M * d.k_split; d.lda = d.k_split; d.lda2 = d.K - d.k_split; }
      d.zero_rows = (int)q[20];
      if (q[21]) d.gn_out = dGnO.p;
      if (q[22]) {   // GroupNorm(+SiLU) of the output inside the split-K reduction (PfdGemmDesc.gnf_y); the residual then wraps never
        d.gnf_gamma = dB.p; d.gnf_beta = dB.p + d.N; d.gnf_y = dY.p; d.gnf_ldy = nout; d.gnf_eps = 1e-5f; d.gnf_act = PFD_ACT_SILU;
        d.gnf_rows = d.ksize > 0 ? d.Ho * d.Wo : (int)std::min<long>(q[18], d.M);
        d.gnf_skip_raw = q[22] == 2;
      }
      if (q[23] > 0 && d.R && !q[22]) d.res_rows = (int)q[23];
      static const bool replay_warm = getenv("PFD_REPLAY_WARM") && atoi(getenv("PFD_REPLAY_WARM")) != 0;   // weights of every launch from ONE buffer (cache-warm): the bound of any weight prefetch
      if (timed && !replay_warm) {
        const size_t wn = ((size_t)d.N * d.K * (d.ksize > 0 && d.ups == 2 ? 4 : 1) + 4095) & ~(size_t)4095;   // (ups = 2: four phase blocks)
        if (pool_off + wn > pool_elems) pool_off = 0;
        d.W = dPool.p + pool_off;
        pool_off += wn;
      }
      // PFD_REPLAY_LN=1: the launches that carry a folded LayerNorm in the UNet do so here too (q|k|v, q and GEGLU
      // projections consume row statistics; proj_in / out-projections emit them) -- prices the fold per shape
      static const bool replay_ln = getenv("PFD_REPLAY_LN") && atoi(getenv("PFD_REPLAY_LN")) != 0;
      if (replay_ln && d.ksize == 0 && d.N % 160 == 0 && !d.bias_per_row) {
        const bool cwidth = d.K == 320 || d.K == 640 || d.K == 1280;
        if (cwidth && (d.act == PFD_ACT_GEGLU || d.N == 3 * d.K || (d.N == d.K && !d.R && !d.bias))) {
          d.ln_stats = dLnS.p; d.ln_colsum = dLnC.p; d.ln_parts = d.K / 160; d.ln_eps = 1e-5f;
        } else if ((d.N == 320 || d.N == 640 || d.N == 1280) && d.act == 0 && d.bias && d.K == d.N) {   // out-projections, proj_in
          d.ln_out = dLnO.p;
        }
      }
      static const bool replay_tiled = getenv("PFD_REPLAY_TILED") && atoi(getenv("PFD_REPLAY_TILED")) != 0;
      if (replay_tiled && (d.N % 160 == 0 || d.N % 128 == 0) && d.K % 64 == 0 && !d.bias_per_row) d.w_tiled = 1;
      if (force_tile == 0 || pfd_gemm_f16_ex(&d, force_tile, nullptr) != 0) {
        int rc = pfd_gemm_f16(&d, nullptr);
        if (rc == PFD_ESHAPE && d.gnf_y) {   // declined (this build does not split the shape): the two-call form's first call
          d.gnf_y = nullptr;
          rc = pfd_gemm_f16(&d, nullptr);
        }
        bad += rc != 0;
      }
      // PFD_REPLAY_DET=1: every launch twice on the same operands into two buffers; the results must be the same bits
      static const bool replay_det = getenv("PFD_REPLAY_DET") && atoi(getenv("PFD_REPLAY_DET")) != 0;
      if (replay_det && rep == 0) {
        static Dev<h16>* dC2 = nullptr;
        static Dev<unsigned>* dCnt = nullptr;
        if (!dC2) { dC2 = new Dev<h16>(maxC); dCnt = new Dev<unsigned>(1); }
        PfdGemmDesc d2 = d;
        d2.C = dC2->p;
        HIP_OK(hipMemset(dCnt->p, 0, sizeof(unsigned)));
        bad += pfd_gemm_f16(&d2, nullptr) != 0;
        const size_t nel = (size_t)d.M * nout;
        hipLaunchKernelGGL(count_mismatch_kernel, dim3(1024), dim3(256), 0, nullptr, (const unsigned short*)dC.p,
                           (const unsigned short*)dC2->p, nel, dCnt->p);
        const unsigned nb = dCnt->get()[0];
        if (nb) {
          ++bad;
          printf("NONDETERMINISTIC: M%ld N%ld K%ld ksize%ld stride%ld ups%ld act%ld rv%d R%d: %u of %zu elements differ between two launches\n",
                 (long)d.M, (long)d.N, (long)d.K, (long)d.ksize, (long)d.stride, (long)d.ups, (long)d.act, d.rowvec != nullptr, d.R != nullptr, nb, nel);
        }
      }
      if (timed) HIP_OK(hipEventRecord(ev[++li], nullptr));
    }
    HIP_OK(hipDeviceSynchronize());
    if (timed && rep > 0)
      for (size_t i = 0; i < rows.size(); ++i) {
        float ms = 0;
        HIP_OK(hipEventElapsedTime(&ms, ev[i], ev[i + 1]));
        acc_ms[i] += ms / (reps - 1);
      }
  }
  HIP_OK(hipDeviceSynchronize());
  printf("replayed %zu launches x%d, %d errors\n", rows.size(), reps, bad);
  if (timed) {
    struct Agg { std::array<long, 24> q; int n; double ms; };
    std::vector<Agg> aggs;
    for (size_t i = 0; i < rows.size(); ++i) {
      bool found = false;
      for (auto& a : aggs) if (a.q == rows[i]) { a.n++; a.ms += acc_ms[i]; found = true; break; }
      if (!found) aggs.push_back({rows[i], 1, acc_ms[i]});
    }
    std::sort(aggs.begin(), aggs.end(), [](const Agg& a, const Agg& b) { return a.ms > b.ms; });
    double tot = 0, tot_ideal = 0;
    printf("%7s %6s %6s k s u act rv R ks zrows gn | %3s %9s %8s %8s %8s %8s\n", "M", "N", "K", "n", "us/launch", "TF/s", "GB/s", "ideal_us", "sum_ms");
    for (auto& a : aggs) {
      const auto& q = a.q;
      const double M = q[0], N = q[1], K = q[2];
      const double nout = q[3] == PFD_ACT_GEGLU ? N / 2 : N;
      const double Mz = M - q[20];   // rows with a non-zero operand (PfdGemmDesc.zero_rows)
      const double abytes = q[8] > 0 ? 2.0 * q[12] * q[13] * q[14] * q[15] : 2.0 * Mz * K;
      const double bytes = abytes + 2.0 * N * K + 2.0 * M * nout + (q[6] ? 2.0 * M * nout : 0) + (q[5] ? 2.0 * M * N / std::max<double>(1, std::min<long>(q[18], M)) : 0);
      const double flops = 2.0 * Mz * N * K;
      const double us = a.ms / a.n * 1e3;
      const double ideal = std::max(flops / 2.5e15, bytes / 8e12) * 1e6;
      tot += a.ms; tot_ideal += ideal * a.n * 1e-3;
      printf("%7ld %6ld %6ld %ld %ld %ld %3ld %2ld %ld %4ld %5ld %ld | %3d %9.1f %8.1f %8.1f %8.1f %8.2f\n", q[0], q[1], q[2], q[8], q[9], q[11], q[3], q[5], q[6],
             q[19], q[20], q[21], a.n, us, flops / us * 1e-6, bytes / us * 1e-3, ideal, a.ms);
    }
    printf("total %.2f ms per UNet pass (GEMM/conv only); roofline-ideal %.2f ms\n", tot, tot_ideal);
  }
  return bad;
}
