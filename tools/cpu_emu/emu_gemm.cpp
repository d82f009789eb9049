// CPU emulation of the wide-tile GEMM / convolution kernels of csrc/gemm_glds.hip (test infrastructure; see hip/hip_runtime.h
// in this directory for the execution model).  tools/cpu_emu/build.py writes gemm_glds_emu.inc -- the kernel file with its
// gfx950 inline-asm statements replaced by their C meaning -- and compiles this file for the host.  The same host dispatcher
// (pfd_gemm160_try: tile choice, split-K, forced variants) and the same device code (index arithmetic, LDS images and
// swizzles, ring slots, barriers, epilogues, the split-K reductions) then run on CPU threads, and the result is
// compared with a double-precision reference.  What it cannot see: s_waitcnt counts (a copy lands when it is issued),
// register allocation, timing.
//   usage: emu_gemm [case ...]      no argument = the built-in list; exit code = number of failed cases
//          emu_gemm --dispatch [--sweep] FILE...    what the dispatcher decides, one text line per call, nothing executed
//                                                   (tests/golden/gemm_dispatch.txt; see "dispatch probe" below)
#include <stdio.h>

#include <array>
#include <random>
#include <set>
#include <string>

#include "hip/hip_runtime.h"


// ---- what the kernel file expects from the rest of the library ----
#include "pfd_common.h"
bool pfd_prof_on() { return false; }
void pfd_prof_begin(int, double, double, hipStream_t) {}
void pfd_prof_end(hipStream_t) {}
static std::string g_err;
int pfd_check_launch(const char*) { return 0; }
void pfd_set_error(const char* m) { g_err = m; }
int pfd_ln_rowstats_launch(const half_t*, long, int, int, float*, hipStream_t, bool) {   // (norm.hip: not part of this build)
  if (emu::dry_run) emu::launch_log.push_back({"pfd_ln_rowstats_launch (norm.hip)", 0, 0, 0, {}});
  return PFD_ESHAPE;
}

#include "gemm_glds_emu.inc"

// ---- cases ----
typedef _Float16 h16;
static std::mt19937 rng(99);
static std::vector<h16> rand_h(size_t n, float scale) {
  std::uniform_real_distribution<float> d(-1.f, 1.f);
  std::vector<h16> v(n);
  for (auto& x : v) x = (h16)(d(rng) * scale);
  return v;
}

struct Case {
  const char* what;
  int M, N, K, variant, splits;
  bool res = false, rowvec = false;
  int act = 0, k_split = 0, zero_rows = 0;
  int ksize = 0, stride = 1, pad = 0, ups = 0, B = 0, H = 0, W = 0, Cin = 0;
  int base_variant = -1;   // >= 0: additionally demand the same bits as this variant
  bool w_tiled = false;    // the weight is handed over K-tile-contiguous (PfdGemmDesc.w_tiled)
  bool gn_stats = false;   // the launch emits GroupNorm statistics (PfdGemmDesc.gn_out): checked against the sums of what it stored
  int gnf = 0;             // 1 / 2: GroupNorm(+SiLU) fused into the split-K reduction (PfdGemmDesc.gnf_y), raw tensor skipped / kept
  int res_rows = 0;        // > 0: the residual holds that many rows, read with one wrap (PfdGemmDesc.res_rows)
  bool declined = false;   // the library must not serve the request: return value 1, nothing written
  int gn_pro = 0;          // 1 / 2: GroupNorm affine map (+ SiLU) in the staging path of the patch kernel (PfdGemmDesc.gn_table)
  int contract = 0;        // 1 / 2: the slab contract of PfdGemmDesc.ws on integer operands whose two slab partials cancel, inside / beyond the f16 range
};

// PfdGemmDesc.ups = 2: the 3x3 weight [N][9 Cin] folded (fp32, rounded once) into four 2x2-tap phase blocks [py][px][N][4 Cin]:
// phase tap (ty, tx) sums the 3x3 taps that read the same low-res pixel, rows R(0,0) = {0}, R(0,1) = {1,2}, R(1,0) = {0,1}, R(1,1) = {2}
static std::vector<_Float16> fold_phase_weight(const std::vector<_Float16>& Wt, int N, int Cin) {
  auto taps = [](int ph, int t, int* lo, int* hi) { *lo = ph == 0 ? (t == 0 ? 0 : 1) : (t == 0 ? 0 : 2); *hi = ph == 0 ? (t == 0 ? 0 : 2) : (t == 0 ? 1 : 2); };
  std::vector<_Float16> out((size_t)4 * N * 4 * Cin);
  for (int py = 0; py < 2; ++py)
    for (int px = 0; px < 2; ++px)
      for (int n = 0; n < N; ++n)
        for (int ty = 0; ty < 2; ++ty)
          for (int tx = 0; tx < 2; ++tx) {
            int y0, y1, x0, x1;
            taps(py, ty, &y0, &y1);
            taps(px, tx, &x0, &x1);
            for (int ci = 0; ci < Cin; ++ci) {
              float a = 0.f;
              for (int ky = y0; ky <= y1; ++ky)
                for (int kx = x0; kx <= x1; ++kx) a += (float)Wt[(size_t)n * 9 * Cin + (ky * 3 + kx) * Cin + ci];
              out[(((size_t)(py * 2 + px) * N + n) * 4 + ty * 2 + tx) * Cin + ci] = (_Float16)a;
            }
          }
  return out;
}

static int run_variant(const Case& c, int variant, const std::vector<h16>& A, const std::vector<h16>& A2, const std::vector<h16>& Wt,
                       const std::vector<h16>& bias, const std::vector<h16>& rv, const std::vector<h16>& R, int M, int K, int Ho, int Wo,
                       std::vector<h16>& C, std::vector<float>& ws, std::vector<float>* gn = nullptr, std::vector<h16>* gnf_y = nullptr,
                       const std::vector<h16>* gnf_gb = nullptr, int gnf_skip_raw = 0, const std::vector<float>* gn_table = nullptr) {
  const bool conv = c.ksize > 0;
  PfdGemmDesc d;
  memset(&d, 0, sizeof(d));
  d.M = M; d.N = c.N; d.K = K;
  std::vector<h16> Wtiled, Wfold;
  const std::vector<h16>* Wsrc = &Wt;
  int nblk = 1;                       // weight blocks of [N][K] each
  if (c.ups == 2) { Wfold = fold_phase_weight(Wt, c.N, c.Cin); Wsrc = &Wfold; K = 4 * c.Cin; d.K = K; nblk = 4; }
  if (c.w_tiled) {   // (n, k) -> (((n / T) * (K / 64) + k / 64) * T + n % T) * 64 + k % 64, T = the tile width
    const int T = c.N % 160 == 0 ? 160 : 128;
    Wtiled.resize(Wsrc->size());
    for (int bl = 0; bl < nblk; ++bl)
      for (int n = 0; n < c.N; ++n)
        for (int k = 0; k < K; ++k)
          Wtiled[(size_t)bl * c.N * K + (((size_t)(n / T) * (K / 64) + k / 64) * T + n % T) * 64 + k % 64] = (*Wsrc)[((size_t)bl * c.N + n) * K + k];
  }
  d.A = A.data(); d.W = c.w_tiled ? Wtiled.data() : Wsrc->data(); d.bias = bias.data(); d.C = C.data();
  d.w_tiled = c.w_tiled ? 1 : 0;
  d.R = c.res ? R.data() : nullptr;
  d.rowvec = c.rowvec ? rv.data() : nullptr;
  d.lda = conv ? c.Cin : (c.k_split ? c.k_split : K);
  d.ldw = K; d.ldc = c.N; d.ldr = c.N; d.ldrv = c.N;
  d.rows_per_rv = conv ? Ho * Wo : 64;
  d.act = c.act;
  d.ksize = c.ksize; d.stride = c.stride; d.pad = c.pad; d.ups = c.ups;
  d.B = c.B; d.H = c.H; d.Wd = c.W; d.Cin = c.Cin; d.Ho = Ho; d.Wo = Wo;
  if (c.k_split) { d.k_split = c.k_split; d.A2 = A2.data(); d.lda2 = K - c.k_split; }
  d.zero_rows = c.zero_rows;
  d.res_rows = c.res_rows;
  d.ws = ws.data(); d.ws_bytes = ws.size() * sizeof(float);
  if (gn) d.gn_out = gn->data();
  if (gnf_y) {
    d.gnf_gamma = gnf_gb->data(); d.gnf_beta = gnf_gb->data() + c.N; d.gnf_y = gnf_y->data(); d.gnf_ldy = c.N; d.gnf_eps = 1e-5f;
    d.gnf_act = PFD_ACT_SILU; d.gnf_rows = conv ? Ho * Wo : M; d.gnf_skip_raw = gnf_skip_raw;
  }
  if (gn_table) { d.gn_table = gn_table->data(); d.gn_c1 = c.Cin; d.gn_act = c.gn_pro == 2 ? PFD_ACT_SILU : PFD_ACT_NONE; }
  return pfd_gemm160_try(&d, variant, c.splits, nullptr);
}

static int run_case(const Case& c) {
  const bool conv = c.ksize > 0;
  int M = c.M, K = c.K, Ho = 0, Wo = 0;
  if (conv) {
    const int Hin = c.ups ? 2 * c.H : c.H, Win = c.ups ? 2 * c.W : c.W;
    Ho = (Hin + 2 * c.pad - c.ksize) / c.stride + 1;
    Wo = (Win + 2 * c.pad - c.ksize) / c.stride + 1;
    M = c.B * Ho * Wo;
    K = c.ksize * c.ksize * c.Cin;
  }
  const int N = c.N;
  const long a_rows = conv ? (long)c.B * c.H * c.W : M, lda_full = conv ? c.Cin : K;
  auto Afull = rand_h((size_t)a_rows * lda_full, 1.f);
  auto Wt = rand_h((size_t)N * K, 1.7f / sqrtf((float)K)), bias = rand_h(N, 0.5f), R = rand_h((size_t)M * N, 1.f);
  const int rows_per_rv = conv ? Ho * Wo : 64;
  auto rv = rand_h((size_t)((M + rows_per_rv - 1) / rows_per_rv) * N, 0.5f);
  for (long r = 0; r < c.zero_rows; ++r)
    for (long k = 0; k < lda_full; ++k) Afull[r * lda_full + k] = (h16)0;
  if (c.contract) {
    // split-K 2 over five K tiles: slabs [0, 192) and [192, K).  A = 4 {-2..2} + 8 s_k, W = 8 {-1, 0, 1} + 8 s_k in the first slab
    // and - 12 s_k in the second, bias 16 {-4..4}: every product is a multiple of 16, the two partials are about +-12288 and
    // nothing rounds; contract 2 doubles A and the noise of W and triples its common part (multiples of 32, partials about
    // +-73728: most beyond 65504, a few per cent of them back inside)
    std::uniform_int_distribution<int> d2(-2, 2), d1(-1, 1), d4(-4, 4), sg(0, 1);
    const float mul = c.contract == 2 ? 2.f : 1.f;
    std::vector<float> sk(K);
    for (auto& v : sk) v = sg(rng) ? 1.f : -1.f;
    for (int m = 0; m < M; ++m)
      for (int k = 0; k < K; ++k) Afull[(size_t)m * K + k] = (h16)(mul * (4.f * d2(rng) + 8.f * sk[k]));
    for (int n = 0; n < N; ++n)
      for (int k = 0; k < K; ++k) Wt[(size_t)n * K + k] = (h16)(mul * 8.f * d1(rng) + (c.contract == 2 ? 3.f : 1.f) * (k < 192 ? 8.f : -12.f) * sk[k]);
    for (auto& v : bias) v = (h16)(16.f * d4(rng));
  }
  // device operands: rows below zero_rows are not stored; columns >= k_split live in a second buffer
  const int K1 = c.k_split ? c.k_split : (int)lda_full, K2 = c.k_split ? K - c.k_split : 0;
  const long Mz = a_rows - c.zero_rows;
  std::vector<h16> A1((size_t)Mz * K1 + 64), A2((size_t)Mz * std::max(K2, 1) + 64);
  for (long m = 0; m < Mz; ++m) {
    for (int k = 0; k < K1; ++k) A1[(size_t)m * K1 + k] = Afull[(size_t)(m + c.zero_rows) * lda_full + k];
    for (int k = 0; k < K2; ++k) A2[(size_t)m * K2 + k] = Afull[(size_t)(m + c.zero_rows) * lda_full + K1 + k];
  }
  std::vector<h16> C((size_t)M * N, (h16)-77.f);
  std::vector<float> ws((size_t)8 * M * N + 64);
  g_err.clear();
  std::vector<float> gn1((size_t)(M / 64 + 1) * (N / 160) * 32, -1.f), gn2 = gn1;
  // GroupNorm prologue: a per-sample {scale[Cin], shift[Cin]} table; the operand of the contraction is the f16 rounding of
  // act(x * scale + shift), and the zero padding pads THAT image
  std::vector<float> table;
  std::vector<h16> Apro;
  if (c.gn_pro) {
    std::uniform_real_distribution<float> d(-1.f, 1.f);
    table.resize((size_t)c.B * 2 * c.Cin);
    for (int b = 0; b < c.B; ++b)
      for (int ch = 0; ch < c.Cin; ++ch) { table[((size_t)b * 2) * c.Cin + ch] = 1.f + 0.3f * d(rng); table[((size_t)b * 2 + 1) * c.Cin + ch] = 0.4f * d(rng); }
    Apro.resize(Afull.size());
    for (size_t i = 0; i < Afull.size(); ++i) {
      const int ch = (int)(i % c.Cin), b = (int)(i / ((size_t)c.H * c.W * c.Cin));
      double v = (double)Afull[i] * (double)table[((size_t)b * 2) * c.Cin + ch] + (double)table[((size_t)b * 2 + 1) * c.Cin + ch];
      if (c.gn_pro == 2) v = v / (1.0 + exp(-v));
      Apro[i] = (h16)v;
    }
  }
  const std::vector<h16>& Aref = c.gn_pro ? Apro : Afull;
  const int rc = run_variant(c, c.variant, A1, A2, Wt, bias, rv, R, M, K, Ho, Wo, C, ws, c.gn_stats ? &gn1 : nullptr, nullptr, nullptr, 0,
                             c.gn_pro ? &table : nullptr);
  if (c.declined) {
    size_t touched = 0;
    for (const auto& v : C) touched += (float)v != -77.f;
    const bool ok = rc == 1 && touched == 0;
    printf("%s %-70s rc %d, %zu elements written (declined requests launch nothing)\n", ok ? "ok  " : "FAIL", c.what, rc, touched);
    return ok ? 0 : 1;
  }
  if (rc != 0) { printf("FAIL %-70s rc=%d %s\n", c.what, rc, g_err.c_str()); return 1; }
  if (c.contract) {
    // include/pfd_hip.h, PfdGemmDesc.ws: epi(sum_s f16(P_s)), the slabs summed in fp32 in slab order, IEEE throughout -- here every
    // finite quantity is exact, so the whole output is held to the bits (a NaN to being one)
    size_t bad = 0, n_nan = 0, n_inf = 0;
    double pmax = 0;
    for (int m = 0; m < M; ++m)
      for (int n = 0; n < N; ++n) {
        double P[2] = {0, 0};
        for (int k = 0; k < K; ++k) P[k >= 192] += (double)Afull[(size_t)m * K + k] * (double)Wt[(size_t)n * K + k];
        pmax = std::max(pmax, std::max(fabs(P[0]), fabs(P[1])));
        float v = (float)(h16)P[0] + (float)(h16)P[1];
        v += (float)(h16)P[1] * 0.f;   // the group of four is filled up with the last slab weighted by 0: NaN where that slab is +-inf
        v += (float)bias[n];
        if (c.act == PFD_ACT_RELU) v = fmaxf(v, 0.f);
        const h16 want = (h16)v, got = C[(size_t)m * N + n];
        if (c.contract == 1 && (double)want != P[0] + P[1] + (double)bias[n]) ++bad;   // (the double-precision sum itself)
        n_nan += v != v; n_inf += std::isinf(v);
        if (v != v ? !((float)got != (float)got) : memcmp(&want, &got, sizeof(h16)) != 0) {
          if (++bad <= 4) printf("     (%d, %d): partials %.0f %.0f bias %.0f -> %g, expected %g\n", m, n, P[0], P[1], (double)bias[n], (double)got, (double)want);
        }
      }
    bool ok = bad == 0 && (c.contract == 1 ? pmax < 32768 && n_nan + n_inf == 0 : n_nan > 0 && n_inf > 0);
    std::string extra;
    if (ok && c.gn_stats) {   // the statistics are the sums of the stored values (all finite here)
      const int cpg = N / 32, tn = N / 160, ngl = 160 / cpg;
      double worst = 0;
      for (int sl = 0; sl < M / 64; ++sl)
        for (int t = 0; t < tn; ++t)
          for (int gl = 0; gl < ngl; ++gl) {
            double a = 0, q = 0;
            for (int r = 0; r < 64; ++r)
              for (int cc = 0; cc < cpg; ++cc) { const double v = (double)C[(size_t)(sl * 64 + r) * N + t * 160 + gl * cpg + cc]; a += v; q += v * v; }
            const size_t o = (((size_t)sl * tn + t) * 16 + gl) * 2;
            worst = std::max(worst, std::max(fabs(a - gn1[o]) / (1 + fabs(a)), fabs(q - gn1[o + 1]) / (1 + fabs(q))));
          }
      ok = ok && worst <= 1e-3;
      extra = " | statistics err " + std::to_string(worst);
    }
    if (c.contract == 1)
      printf("%s %-70s bit-equal to the double-precision sum: %zu elements differ, max |partial| %.0f%s\n", ok ? "ok  " : "FAIL", c.what, bad, pmax, extra.c_str());
    else
      printf("%s %-70s IEEE pattern of sum_s f16(P_s): %zu elements differ, %zu NaN, %zu inf, max |partial| %.0f\n", ok ? "ok  " : "FAIL", c.what, bad, n_nan, n_inf, pmax);
    fflush(stdout);
    return ok ? 0 : 1;
  }
  // double-precision reference
  double max_err = 0, max_ref = 0;
  for (int m = 0; m < M; ++m) {
    int b = 0, oy = 0, ox = 0;
    if (conv) { b = m / (Ho * Wo); oy = (m % (Ho * Wo)) / Wo; ox = m % Wo; }
    for (int n = 0; n < N; ++n) {
      double s = 0;
      if (!conv) {
        for (int k = 0; k < K; ++k) s += (double)Afull[(size_t)m * K + k] * (double)Wt[(size_t)n * K + k];
      } else {
        const int Hin = c.ups ? 2 * c.H : c.H, Win = c.ups ? 2 * c.W : c.W;
        for (int ky = 0; ky < c.ksize; ++ky)
          for (int kx = 0; kx < c.ksize; ++kx) {
            int iy = oy * c.stride + ky - c.pad, ix = ox * c.stride + kx - c.pad;
            if (iy < 0 || iy >= Hin || ix < 0 || ix >= Win) continue;
            if (c.ups) { iy /= 2; ix /= 2; }
            const h16* ap = &Aref[(((size_t)b * c.H + iy) * c.W + ix) * c.Cin];
            const h16* wp = &Wt[(size_t)n * K + (ky * c.ksize + kx) * c.Cin];
            for (int ci = 0; ci < c.Cin; ++ci) s += (double)ap[ci] * (double)wp[ci];
          }
      }
      s += (double)bias[n];
      if (c.rowvec) s += (double)rv[(size_t)(m / rows_per_rv) * N + n];
      if (c.act == PFD_ACT_SILU) s = s / (1.0 + exp(-s));
      else if (c.act == PFD_ACT_RELU) s = s > 0 ? s : 0;
      if (c.res) s += (double)R[(size_t)(c.res_rows > 0 && m >= c.res_rows ? m - c.res_rows : m) * N + n];
      max_ref = std::max(max_ref, fabs(s));
      max_err = std::max(max_err, fabs(s - (double)C[(size_t)m * N + n]));
    }
  }
  const bool ok = max_err <= 4e-3 * std::max(1.0, max_ref);
  int fails = ok ? 0 : 1;
  std::string extra;
  if (ok && c.base_variant >= 0) {
    std::vector<h16> C2((size_t)M * N, (h16)-55.f);
    const int rc2 = run_variant(c, c.base_variant, A1, A2, Wt, bias, rv, R, M, K, Ho, Wo, C2, ws, nullptr, nullptr, nullptr, 0,
                                c.gn_pro ? &table : nullptr);
    size_t nd = 0;
    for (size_t i = 0; i < C.size(); ++i) nd += memcmp(&C[i], &C2[i], sizeof(h16)) != 0;
    if (rc2 != 0 || nd) { fails = 1; extra = " | vs variant " + std::to_string(c.base_variant) + ": rc " + std::to_string(rc2) + ", " + std::to_string(nd) + " elements differ"; }
    else extra = " | == variant " + std::to_string(c.base_variant) + " bitwise";
  }
  if (ok && c.gn_stats) {
    // the statistics are the sums of the f16 values the launch stored, per 64-row slab and group of N / 32 channels
    const int cpg = N / 32, tn = N / 160, ngl = 160 / cpg;
    double worst = 0;
    if (c.ups == 2) {
      // the phase form's slabs are 64 rows of the (b, phase, y, x) order: what the consumer uses are the per-sample totals
      const int spS = Ho * Wo / 64;
      for (int b = 0; b < c.B; ++b)
        for (int t = 0; t < tn; ++t)
          for (int gl = 0; gl < ngl; ++gl) {
            double a = 0, q = 0, ga = 0, gq = 0;
            for (int r = 0; r < Ho * Wo; ++r)
              for (int cc = 0; cc < cpg; ++cc) { const double v = (double)C[((size_t)b * Ho * Wo + r) * N + t * 160 + gl * cpg + cc]; a += v; q += v * v; }
            for (int sl = b * spS; sl < (b + 1) * spS; ++sl) { const size_t o = (((size_t)sl * tn + t) * 16 + gl) * 2; ga += gn1[o]; gq += gn1[o + 1]; }
            worst = std::max(worst, std::max(fabs(a - ga) / (1 + fabs(a)), fabs(q - gq) / (1 + fabs(q))));
          }
      if (worst > 1e-3) fails = 1;
      extra += std::string(" | per-sample group sums err ") + std::to_string(worst);
    } else {
    for (int sl = 0; sl < M / 64; ++sl)
      for (int t = 0; t < tn; ++t)
        for (int gl = 0; gl < ngl; ++gl) {
          double a = 0, q = 0;
          for (int r = 0; r < 64; ++r)
            for (int cc = 0; cc < cpg; ++cc) { const double v = (double)C[(size_t)(sl * 64 + r) * N + t * 160 + gl * cpg + cc]; a += v; q += v * v; }
          const size_t o = (((size_t)sl * tn + t) * 16 + gl) * 2;
          worst = std::max(worst, std::max(fabs(a - gn1[o]) / (1 + fabs(a)), fabs(q - gn1[o + 1]) / (1 + fabs(q))));
        }
    if (worst > 1e-3) fails = 1;
    extra += std::string(" | statistics err ") + std::to_string(worst);
    }
  }
  if (ok && c.gnf) {
    // the same launch with the fused GroupNorm request: raw result (when kept) bit for bit the plain reduction's, the normalised
    // tensor against a double-precision GroupNorm(32) + SiLU of that raw result
    auto gb = rand_h((size_t)2 * N, 1.f);
    std::vector<h16> C2((size_t)M * N, (h16)-55.f), Y((size_t)M * N, (h16)-33.f);
    const int rc2 = run_variant(c, c.variant, A1, A2, Wt, bias, rv, R, M, K, Ho, Wo, C2, ws, nullptr, &Y, &gb, c.gnf == 1 ? 1 : 0);
    size_t nd = 0, untouched = 0;
    for (size_t i = 0; i < C.size(); ++i) { nd += memcmp(&C[i], &C2[i], sizeof(h16)) != 0; untouched += (float)C2[i] == -55.f; }
    const int HW = conv ? Ho * Wo : M, Bn = M / HW, cpg = N / 32;
    double werr = 0;
    for (int b = 0; b < Bn; ++b)
      for (int g = 0; g < 32; ++g) {
        double a = 0, q = 0;
        for (int p = 0; p < HW; ++p)
          for (int ch = g * cpg; ch < (g + 1) * cpg; ++ch) { const double v = (double)C[((size_t)b * HW + p) * N + ch]; a += v; q += v * v; }
        const double n = (double)HW * cpg, mean = a / n, rstd = 1.0 / sqrt(q / n - mean * mean + 1e-5);
        for (int p = 0; p < HW; ++p)
          for (int ch = g * cpg; ch < (g + 1) * cpg; ++ch) {
            double v = ((double)C[((size_t)b * HW + p) * N + ch] - mean) * rstd * (double)gb[ch] + (double)gb[N + ch];
            v = v / (1.0 + exp(-v));
            werr = std::max(werr, fabs(v - (double)Y[((size_t)b * HW + p) * N + ch]) / std::max(1.0, fabs(v)));
          }
      }
    const bool raw_ok = c.gnf == 2 ? nd == 0 : untouched == C2.size();
    if (rc2 != 0 || !raw_ok || werr > 4e-3) fails = 1;
    extra += " | fused GroupNorm: rc " + std::to_string(rc2) + (c.gnf == 2 ? ", raw differs in " + std::to_string(nd) : ", raw elements written " + std::to_string(C2.size() - untouched)) +
             ", normalised err " + std::to_string(werr);
    if (!fails) {   // and a request the library must decline without launching: the same problem unsplit
      Case u = c; u.splits = 1;
      std::vector<h16> C3((size_t)M * N, (h16)-55.f), Y3((size_t)M * N, (h16)-33.f);
      const int rc3 = run_variant(u, c.variant, A1, A2, Wt, bias, rv, R, M, K, Ho, Wo, C3, ws, nullptr, &Y3, &gb, 0);
      size_t touched = 0;
      for (size_t i = 0; i < C3.size(); ++i) touched += ((float)C3[i] != -55.f) + ((float)Y3[i] != -33.f);
      if (rc3 != 1 || touched) { fails = 1; extra += " | UNSPLIT REQUEST NOT DECLINED (rc " + std::to_string(rc3) + ", " + std::to_string(touched) + " written)"; }
      else extra += " | unsplit request declined, nothing written";
    }
  }
  printf("%s %-70s max err %.2e (max |ref| %.2f)%s\n", fails ? "FAIL" : "ok  ", c.what, max_err, max_ref, extra.c_str());
  fflush(stdout);
  return fails;
}

// ---- dispatch probe: emu_gemm --dispatch FILE... ----
// A dry run of pfd_gemm160_try (emu::dry_run: launches are recorded, nothing executes, no pointer is dereferenced) over
//  (a) every distinct record of the given PFD_TRACE_GEMM files (TRACE_FIELDS of lib/hip/ops.py: 19, 22 or 24 integers, short
//      ones zero-padded) under the heuristic (variant 0, splits 0);
//  (b) hand-written requests for what a record does not carry (LayerNorm fold, transposed tail, GroupNorm prologue, tiled
//      weights, 128-wide problems, requests that must be declined);
//  (c) a dozen records under every forced variant that serves them, splits 0 and 2.
// One line per call: the record, "v <variant> s <splits> -> <return value>", then per launch the instantiated kernel, grid x / z,
// block x, the named integer fields of the G160Params it was handed (the rarely set ones only where they are set), its non-null
// pointers and whether A2 == A.  Named fields only: the struct is filled field by field and has padding.  --sweep: every record under variant 0 and every
// variant code with splits 0 1 2 3 4 8 instead (comparing two builds of the dispatcher).
typedef std::array<long, 24> Rec;
static void* fake(int i) { return reinterpret_cast<void*>((uintptr_t)0x10000 * (i + 1)); }   // 16-byte aligned, never dereferenced
enum { P_A, P_W, P_BIAS, P_RV, P_R, P_C, P_WS, P_A2, P_GNO, P_GAMMA, P_BETA, P_Y, P_CT, P_LNS, P_LNC, P_LNO, P_TABLE };

static PfdGemmDesc desc_of(const Rec& q) {   // as selftest --replay and ops.gemm / ops.conv fill it
  PfdGemmDesc d;
  memset(&d, 0, sizeof(d));
  d.M = q[0]; d.N = q[1]; d.K = q[2]; d.act = q[3];
  d.A = fake(P_A); d.W = fake(P_W); d.C = fake(P_C);
  d.bias = q[4] ? fake(P_BIAS) : nullptr; d.rowvec = q[5] ? fake(P_RV) : nullptr; d.R = q[6] ? fake(P_R) : nullptr;
  d.bias_per_row = q[7];
  d.ksize = q[8]; d.stride = q[9]; d.pad = q[10]; d.ups = q[11];
  d.B = q[12]; d.H = q[13]; d.Wd = q[14]; d.Cin = q[15]; d.Ho = q[16]; d.Wo = q[17];
  d.rows_per_rv = (int)std::min<long>(q[18], 1 << 30);
  const long nout = d.act == PFD_ACT_GEGLU ? d.N / 2 : d.N;
  d.lda = d.ksize > 0 ? d.Cin : d.K; d.ldw = d.K; d.ldc = nout; d.ldr = nout; d.ldrv = d.N;
  d.ws = fake(P_WS); d.ws_bytes = (size_t)96 << 20;   // ops._WS_BYTES
  if (q[19] > 0) { d.k_split = (int)q[19]; d.A2 = fake(P_A2); d.lda = d.k_split; d.lda2 = d.K - d.k_split; }
  d.zero_rows = (int)q[20];
  if (q[21]) d.gn_out = fake(P_GNO);
  if (q[22]) {
    d.gnf_gamma = fake(P_GAMMA); d.gnf_beta = fake(P_BETA); d.gnf_y = fake(P_Y); d.gnf_ldy = nout; d.gnf_eps = 1e-5f; d.gnf_act = PFD_ACT_SILU;
    d.gnf_rows = d.ksize > 0 ? d.Ho * d.Wo : (int)std::min<long>(q[18], d.M);
    d.gnf_skip_raw = q[22] == 2;
  }
  if (q[23] > 0 && d.R && !q[22]) d.res_rows = (int)q[23];
  return d;
}

static std::string launches_text() {
  std::string out, prev;
  char b[1024];
  for (const auto& l : emu::launch_log) {
    snprintf(b, sizeof(b), " | %s grid %ux%u block %u", l.kernel.c_str(), l.grid_x, l.grid_z, l.block_x);
    out += b;
    if (l.args.empty() || l.args[0].size() != sizeof(G160Params)) continue;
    G160Params p;
    memcpy(&p, l.args[0].data(), sizeof(p));
    snprintf(b, sizeof(b), " tiles_m=%d tiles_n=%d splits=%d kt_per_split=%d k_split=%d rows_per_rv=%d", p.tiles_m, p.tiles_n, p.splits, p.kt_per_split,
             p.k_split, p.rows_per_rv);
    std::string t = b;
    // the other named fields where they differ from kFieldDefaults (the first line of the output)
    const struct { const char* name; long v, dflt; } opt[] = {{"nmajor", p.nmajor, 0}, {"krot", p.krot, 0}, {"pt_w", p.pt_w, 0}, {"pt_sh", p.pt_sh, 0},
        {"w_tu", p.w_tu, 0}, {"w_kstep", p.w_kstep, 64}, {"zero_rows", p.zero_rows, 0}, {"r_wrap", p.r_wrap, 0x7fffffff}, {"gn_c1", p.gn_c1, 0},
        {"gn_act", p.gn_act, 0}, {"ln_P", p.ln_P, 0}};
    for (const auto& o : opt)
      if (o.v != o.dflt) t += std::string(" ") + o.name + "=" + std::to_string(o.v);
    t += " ptr";   // the non-null pointer fields (every other pointer of the struct is null)
    const std::pair<const char*, const void*> ptrs[] = {{"A", p.A}, {"W", p.W}, {"bias", p.bias}, {"rowvec", p.rowvec}, {"R", p.R}, {"C", p.C},
        {"ws", p.ws}, {"Ct", p.Ct}, {"ln_in", p.ln_in}, {"ln_cs", p.ln_cs}, {"ln_out", p.ln_out}, {"gn_table", p.gn_table}, {"A2", p.A2}, {"gn_out", p.gn_out}};
    for (const auto& q : ptrs)
      if (q.second) t += std::string(" ") + q.first;
    t += p.A2 == p.A ? " A2==A" : " A2!=A";
    out += t == prev ? " (the same parameters)" : t;
    prev = t;
    if (l.args.size() > 1 && l.args[1].size() == sizeof(GnFuse)) {
      GnFuse f;
      memcpy(&f, l.args[1].data(), sizeof(f));
      snprintf(b, sizeof(b), " gnf: ldy=%ld act=%d rows=%d skip_raw=%d ptr%s%s%s", f.ldy, f.act, f.rows, f.skip_raw, f.gamma ? " gamma" : "",
               f.beta ? " beta" : "", f.y ? " y" : "");
      out += b;
    }
  }
  return out;
}
static const char kFieldDefaults[] = "# fields printed only where they differ: nmajor=0 krot=0 pt_w=0 pt_sh=0 w_tu=0 w_kstep=64 zero_rows=0 r_wrap=2147483647 "
                                     "gn_c1=0 gn_act=0 ln_P=0; pointers not listed after \"ptr\" are null";

// one call, one line; served_only: print nothing unless the call returned 0
static void probe(const std::string& what, const PfdGemmDesc& d, int variant, int splits, bool served_only = false) {
  emu::launch_log.clear();
  emu::launched.clear();
  const int rc = pfd_gemm160_try(&d, variant, splits, nullptr);
  if (served_only && rc != 0) return;
  printf("%s v %d s %d -> %d%s\n", what.c_str(), variant, splits, rc, launches_text().c_str());
}

static std::string rec_text(const Rec& q) {
  std::string s;
  for (long v : q) s += (s.empty() ? "" : " ") + std::to_string(v);
  return s;
}
static Rec rec_of(const char* line, int* nfields = nullptr) {
  Rec r{};
  int n = 0, off = 0, adv = 0;
  while (n < 24 && sscanf(line + off, "%ld%n", &r[n], &adv) == 1) { ++n; off += adv; }
  if (nfields) *nfields = n;
  return r;
}

static const int kVariants[] = {22, 23, 24, 25, 41, 43, 44, 47, 48, 82, 83, 84, 96, 98, 99};

static int dispatch_probe(int argc, char** argv) {
  emu::dry_run = true;
  bool sweep = false;
  puts(kFieldDefaults);
  for (int i = 0; i < argc; ++i) {
    if (!strcmp(argv[i], "--sweep")) { sweep = true; continue; }
    FILE* f = fopen(argv[i], "r");
    if (!f) { fprintf(stderr, "emu_gemm: cannot open %s\n", argv[i]); return 2; }
    const char* base = strrchr(argv[i], '/');
    printf("# %s\n", base ? base + 1 : argv[i]);
    std::set<Rec> seen;
    char line[512];
    for (int ln = 1; fgets(line, sizeof(line), f); ++ln) {
      int n;
      const Rec q = rec_of(line, &n);
      if (n == 0) continue;
      if (n != 19 && n != 22 && n != 24) { fprintf(stderr, "emu_gemm: %s:%d: %d fields\n", argv[i], ln, n); return 2; }
      if (!seen.insert(q).second) continue;
      const PfdGemmDesc d = desc_of(q);
      probe(rec_text(q), d, 0, 0);
      if (sweep)
        for (int v : {0, 22, 23, 24, 25, 41, 43, 44, 47, 48, 82, 83, 84, 96, 98, 99})
          for (int s : {0, 1, 2, 3, 4, 8})
            if (v || s) probe(rec_text(q), d, v, s);
    }
    fclose(f);
  }
  if (sweep) return 0;

  // (b) what a launch record does not carry, named after the model shape it stands for
  printf("# hand-written requests\n");
  auto lin = [](int M, int N, int K, int act, bool bias, bool res) { return desc_of(Rec{M, N, K, act, bias, 0, res, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1}); };
  auto conv3 = [](int B, int H, int Cin, int N, int ups = 0, bool res = false) {
    const int Ho = ups ? 2 * H : H;
    return desc_of(Rec{(long)B * Ho * Ho, N, (ups == 2 ? 4 : 9) * Cin, 0, 1, 0, res, 0, 3, 1, 1, ups, B, H, H, Cin, Ho, Ho, (long)Ho * Ho});
  };
  auto ln_in = [](PfdGemmDesc d) { d.ln_stats = fake(P_LNS); d.ln_colsum = fake(P_LNC); d.ln_parts = d.K / 160; d.ln_eps = 1e-5f; return d; };
  auto ln_out = [](PfdGemmDesc d) { d.ln_out = fake(P_LNO); return d; };
  auto tail = [](PfdGemmDesc d, int n_split) { d.Ct = fake(P_CT); d.ldct = d.M; d.n_split = n_split; d.ldc = n_split; return d; };
  auto gn_pro = [](PfdGemmDesc d, int c1, int act) {
    d.gn_table = fake(P_TABLE); d.gn_c1 = c1; d.gn_act = act;
    if (c1 < d.Cin) { d.lda = c1; d.A2 = fake(P_A2); d.lda2 = d.Cin - c1; }
    return d;
  };
  auto tiled = [](PfdGemmDesc d) { d.w_tiled = 1; return d; };
  probe("64^2 norm1 -> q|k|v 32768x960x320, LayerNorm fold (ln_stats + ln_colsum)", ln_in(lin(32768, 960, 320, 0, false, false)), 0, 0);
  probe("32^2 norm3 -> GEGLU projection 8192x5120x640, LayerNorm fold", ln_in(lin(8192, 5120, 640, PFD_ACT_GEGLU, true, false)), 0, 0);
  probe("64^2 norm2 -> to_q 32768x320x320, LayerNorm fold, also emits ln_out", ln_out(ln_in(lin(32768, 320, 320, 0, false, false))), 0, 0);
  probe("16^2 norm2 -> to_q 2048x1280x1280, LayerNorm fold, also emits ln_out", ln_out(ln_in(lin(2048, 1280, 1280, 0, false, false))), 0, 0);
  probe("64^2 out-projection 32768x320x320 + residual, emits ln_out", ln_out(lin(32768, 320, 320, 0, true, true)), 0, 0);
  probe("8^2 ff-out 512x1280x5120 + residual, emits ln_out (split K: statistics by the stand-alone kernel)", ln_out(lin(512, 1280, 5120, 0, true, true)), 0, 0);
  probe("32^2 fused q|k|v 8192x1920x640, v transposed (Ct, n_split 1280), LayerNorm fold", tail(ln_in(lin(8192, 1920, 640, 0, false, false)), 1280), 0, 0);
  probe("16^2 fused q|k|v 2048x3840x1280, v transposed (Ct, n_split 2560)", tail(lin(2048, 3840, 1280, 0, false, false), 2560), 0, 0);
  probe("SeeCoder q|k|v 4096x384x128 (128-wide), v transposed (Ct, n_split 256)", tail(lin(4096, 384, 128, 0, true, false), 256), 0, 0);
  probe("32^2 ResBlock conv 640 -> 640, GroupNorm + SiLU prologue (gn_table, one source)", gn_pro(conv3(8, 32, 640, 640), 640, PFD_ACT_SILU), 0, 0);
  probe("32^2 output ResBlock conv 1280|640 -> 640, GroupNorm + SiLU prologue over the skip concat (gn_table, A2)", gn_pro(conv3(8, 32, 1920, 640), 1280, PFD_ACT_SILU), 0, 0);
  probe("64^2 conv 320 -> 320, GroupNorm prologue without SiLU (gn_table, one source)", gn_pro(conv3(8, 64, 320, 320), 320, PFD_ACT_NONE), 0, 0);
  probe("64^2 conv 320|320 -> 320, GroupNorm prologue without SiLU (gn_table, A2), variant 98 named", gn_pro(conv3(8, 64, 640, 320), 320, PFD_ACT_NONE), 98, 0);
  probe("64^2 conv 320 -> 320 on a 48-wide image, GroupNorm prologue (pixel tiles)", gn_pro(desc_of(Rec{8 * 64 * 48, 320, 2880, 0, 1, 0, 0, 0, 3, 1, 1, 0, 8, 64, 48, 320, 64, 48, 64 * 48}), 320, PFD_ACT_SILU), 0, 0);
  probe("16^2 linear 2048x1280x1280, K-tile-contiguous weight (w_tiled)", tiled(lin(2048, 1280, 1280, 0, true, true)), 0, 0);
  probe("16^2 conv 1280 -> 1280, K-tile-contiguous weight (w_tiled)", tiled(conv3(8, 16, 1280, 1280)), 0, 0);
  probe("VAE 512 -> 512 linear 4096x512x512, K-tile-contiguous weight (w_tiled, 128-wide)", tiled(lin(4096, 512, 512, 0, true, false)), 0, 0);
  probe("VAE mid attention projection 4096x512x512 (128-wide, 64-row tile)", lin(4096, 512, 512, 0, true, true), 0, 0);
  probe("VAE 64^2 conv 512 -> 512 (128-wide, 128-row tile)", conv3(1, 64, 512, 512), 0, 0);
  probe("VAE 256^2 conv 256 -> 128 (128-wide, 256-row tile, loader waves)", conv3(1, 256, 256, 128), 0, 0);
  probe("Swin linear 65536x256x4096 (128-wide, 256-row tile)", lin(65536, 256, 4096, 0, true, false), 0, 0);
  printf("# requests that must be declined (return value 1)\n");
  {
    PfdGemmDesc d = conv3(16, 32, 640, 640);   // 256 patch tiles: not split
    d.gnf_gamma = fake(P_GAMMA); d.gnf_beta = fake(P_BETA); d.gnf_y = fake(P_Y); d.gnf_ldy = d.N; d.gnf_eps = 1e-5f; d.gnf_act = PFD_ACT_SILU; d.gnf_rows = 1024;
    probe("fused GroupNorm (gnf_y) on 32^2 conv 640 -> 640 with 16 samples: a problem that does not split", d, 0, 0);
    d = lin(32768, 1280, 320, 0, true, true);
    d.gnf_gamma = fake(P_GAMMA); d.gnf_beta = fake(P_BETA); d.gnf_y = fake(P_Y); d.gnf_ldy = d.N; d.gnf_eps = 1e-5f; d.gnf_act = PFD_ACT_SILU; d.gnf_rows = 512;
    probe("fused GroupNorm (gnf_y) on linear 32768x1280x320: a problem that does not split", d, 0, 0);
  }
  probe("phase-folded upsample conv (ups = 2) 16^2 1280 -> 1280 with a residual", conv3(8, 16, 1280, 1280, 2, true), 0, 0);
  probe("skip conv 32768x320x640 over two sources (k_split 320) under variant 47", desc_of(Rec{32768, 320, 640, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 320, 0, 0, 0, 0}), 47, 0);
  probe("linear 2080x1280x1280 with GroupNorm statistics (gn_out), M % 64 != 0", desc_of(Rec{2080, 1280, 1280, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 1, 0, 0}), 0, 0);

  // (c) every case of the two variant switches and every branch of the loader-wave / patch launchers
  printf("# forced variants that serve the request (splits 0 and 2)\n");
  static const char* forced[] = {
      "8192 640 2560 0 1 0 1 0 0 0 0 0 0 0 0 0 0 0 1",                              // linear, 160-wide
      "2048 1280 5120 0 1 0 1 0 0 0 0 0 0 0 0 0 0 0 1 0 0 1 0 0",                   // linear + GroupNorm statistics
      "8192 5120 640 4 1 0 0 0 0 0 0 0 0 0 0 0 0 0 1",                              // GEGLU projection (84)
      "32768 320 640 0 1 0 0 0 0 0 0 0 0 0 0 0 0 0 1 320 0 0 0 0",                  // two-source contraction
      "16384 640 640 0 1 0 1 0 0 0 0 0 0 0 0 0 0 0 1 0 8192 0 0 8192",              // zero rows + residual stored once
      "4096 512 512 0 1 0 1 0 0 0 0 0 0 0 0 0 0 0 1",                               // linear, 128-wide
      "8192 640 5760 0 1 1 0 0 3 1 1 0 8 32 32 640 32 32 1024",                     // 3x3 conv, patch kernel
      "2048 1280 11520 0 1 1 0 0 3 1 1 0 8 16 16 1280 16 16 256 0 0 0 1 0",         // 3x3 conv + fused GroupNorm (raw kept)
      "2048 640 5760 0 1 0 0 0 3 2 1 0 8 32 32 640 16 16 256",                      // stride-2 conv (implicit GEMM)
      "8192 1280 11520 0 1 0 0 0 3 1 1 1 8 16 16 1280 32 32 1024 0 0 1 0 0",        // upsample conv, 9-tap gather
      "8192 1280 5120 0 1 0 0 0 3 1 1 2 8 16 16 1280 32 32 1024 0 0 1 0 0",         // upsample conv, phase form
      "4096 512 4608 0 1 0 0 0 3 1 1 0 1 64 64 512 64 64 4096",                     // 3x3 conv, 128-wide
      "4096 256 1024 0 1 0 0 0 3 1 1 2 1 32 32 256 64 64 4096",                     // phase form, 128-wide
  };
  for (const char* r : forced) {
    const Rec q = rec_of(r);
    const PfdGemmDesc d = desc_of(q);
    for (int v : kVariants)
      for (int s : {0, 2}) probe(rec_text(q), d, v, s, true);
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc > 1 && !strcmp(argv[1], "--dispatch")) return dispatch_probe(argc - 2, argv + 2);
  std::vector<Case> cases;
  auto lin = [&](const char* w, int M, int N, int K, int v, int sp, bool res, int base) {
    Case c{w, M, N, K, v, sp}; c.res = res; c.base_variant = base; cases.push_back(c); return &cases.back();
  };
  auto conv = [&](const char* w, int N, int v, int sp, int ks, int st, int pad, int ups, int B, int H, int W, int Cin, bool res, int base) {
    Case c{w, 0, N, 0, v, sp}; c.res = res; c.ksize = ks; c.stride = st; c.pad = pad; c.ups = ups; c.B = B; c.H = H; c.W = W; c.Cin = Cin;
    c.base_variant = base; cases.push_back(c); return &cases.back();
  };
  // the hardware-validated LDS-ring kernels (sanity of the emulation itself)
  lin("variant 23 (64x160, 4-stage LDS ring) 200x160x512", 200, 160, 512, 23, 1, true, -1);
  lin("variant 83 (128x160, 8 waves, 3-stage LDS ring) 200x160x320", 200, 160, 320, 83, 1, false, -1);
  // residual stored once for a doubled batch (PfdGemmDesc.res_rows, round 5): store pass and plain split-K reduction, + zero rows
  { auto c = lin("residual read with one wrap (res_rows 128), 8-wave 128-row tile", 256, 160, 256, 82, 1, true, -1); c->res_rows = 128; }
  { auto c = lin("residual read with one wrap + zero rows (the CFG re-join), 64-row ring", 256, 320, 512, 23, 1, true, -1); c->res_rows = 128; c->zero_rows = 128; }
  { auto c = lin("residual read with one wrap, split-K 2 (plain reduction)", 256, 160, 1024, 23, 2, true, -1); c->res_rows = 128; }
  // split-K reduction that also emits the GroupNorm statistics (three row sweeps in flight)
  { auto c = lin("split-K 4 + GroupNorm statistics (N 320: cpg 10), residual", 128, 320, 1024, 23, 4, true, -1); c->gn_stats = true; }
  { auto c = conv("split-K 2 conv 8x8x128 -> 1280 + statistics (cpg 40), SiLU-free", 1280, 83, 2, 3, 1, 1, 0, 2, 8, 8, 128, true, -1); c->gn_stats = true; }
  // the transformer tail fold (proj_out over [h1 | g]): two sources + residual with one wrap + group sums of the output in one
  // launch, on the store pass of the 128-row and 64-row eight-wave tiles and through the split-K reduction (slab 0 holds K tiles
  // of both sources)
  { auto c = lin("tail fold: k_split 64 of K 320, res_rows 128, group sums (cpg 10), 8-wave 128-row tile", 256, 320, 320, 82, 1, true, -1); c->k_split = 64; c->res_rows = 128; c->gn_stats = true; }
  { auto c = lin("tail fold: k_split 64 of K 320, res_rows 64, group sums, 8-wave 64-row ring", 128, 320, 320, 43, 1, true, -1); c->k_split = 64; c->res_rows = 64; c->gn_stats = true; }
  { auto c = lin("tail fold: k_split 128 of K 640, res_rows 64, split-K 2 through the reduction that emits group sums", 128, 320, 640, 43, 2, true, -1); c->k_split = 128; c->res_rows = 64; c->gn_stats = true; }
  // split-K reduction that also NORMALISES (PfdGemmDesc.gnf_y, round 5): 8 samples so that B * 32 >= 128 blocks as the host demands
  { auto c = conv("fused GroupNorm: split-K 2 conv 4x4x128 -> 1280 (cpg 40), row vector, raw skipped", 1280, 83, 2, 3, 1, 1, 0, 8, 4, 4, 128, false, -1); c->rowvec = true; c->gnf = 1; }
  { auto c = conv("fused GroupNorm: split-K 3 conv 4x4x192 -> 1280, residual, raw kept", 1280, 23, 3, 3, 1, 1, 0, 4, 4, 4, 192, true, -1); c->gnf = 2; }
  { auto c = conv("fused GroupNorm: split-K 2 patch conv 16x16x128 -> 1280, raw skipped", 1280, 98, 2, 3, 1, 1, 0, 4, 16, 16, 128, false, -1); c->rowvec = true; c->gnf = 1; }
  // the slab contract of PfdGemmDesc.ws (include/pfd_hip.h) on the real split-K paths: partial sums that cancel, and one that leaves the range
  { auto c = lin("slab contract: exact cancelling partials, split-K 2, 128x160x320", 128, 160, 320, 23, 2, false, -1); c->contract = 1; }
  { auto c = lin("slab contract: the same, 128x320x320, through the reduction that emits group sums", 128, 320, 320, 23, 2, false, -1); c->contract = 1; c->gn_stats = true; }
  { auto c = lin("slab contract: a partial beyond the range, split-K 2, 128x160x320", 128, 160, 320, 23, 2, false, -1); c->contract = 2; }
  // the barrier forms of the patch kernel (sanity of the emulation on the hardware-validated kernels)
  conv("variant 98 patch conv 16x16 (loader waves, barrier per tap), 2 channel blocks", 160, 98, 1, 3, 1, 1, 0, 1, 16, 16, 128, true, -1);
  conv("variant 96 patch conv 16x16 (3-stage weight ring), 2 channel blocks", 160, 96, 1, 3, 1, 1, 0, 1, 16, 16, 128, true, 98);
  { auto c = conv("variant 96 patch conv 16x16, K-tile-contiguous weights, two column tiles", 320, 96, 1, 3, 1, 1, 0, 1, 16, 16, 128, true, -1); c->w_tiled = true; }
  { auto c = conv("variant 83 implicit-GEMM conv, K-tile-contiguous weights, two column tiles", 320, 83, 1, 3, 1, 1, 0, 1, 8, 8, 128, false, -1); c->w_tiled = true; }
  conv("variant 99 patch conv 16x16 (8-wave form), 2 channel blocks", 160, 99, 1, 3, 1, 1, 0, 1, 16, 16, 128, true, 98);
  // upsample convolution as four folded 2x2-tap phase convolutions (PfdGemmDesc.ups = 2) against the nearest-2x + 3x3 reference:
  // 16x16 -> 32x32, one 256-row tile per phase
  { auto c = conv("phase-fold: upsample conv 16x16x64 -> 320, group sums of the output (cpg 10)", 320, 0, 0, 3, 1, 1, 2, 1, 16, 16, 64, false, -1); c->gn_stats = true; }
  conv("phase-fold: upsample conv 16x16x64 -> 160, two-stage form forced", 160, 48, 0, 3, 1, 1, 2, 1, 16, 16, 64, false, -1);
  conv("phase-fold: upsample conv 16x16x64 -> 128 (128-wide tile)", 128, 0, 0, 3, 1, 1, 2, 1, 16, 16, 64, false, -1);
  { auto c = conv("phase-fold: upsample conv 16x16x128 -> 160, K-tile-contiguous phase blocks", 160, 0, 0, 3, 1, 1, 2, 1, 16, 16, 128, false, -1); c->w_tiled = true; }
  { auto c = conv("phase-fold: upsample conv 8x8x64 -> 160 is declined (a tile would straddle two phases)", 160, 0, 0, 3, 1, 1, 2, 1, 8, 8, 64, false, -1); c->declined = true; }
  // the fragment pipeline of the loader-wave patch kernel: A fragments read one half step ahead, those of
  // taps 1..8 before the tap's barrier.  (The emulation checks the index arithmetic and the order of the sums -- same bits as
  // the 8-wave kernel, whose loop reads every fragment behind the barrier -- not the hazard: a copy lands when it is issued.)
  // Three channel blocks: both buffer hand-overs and one buffer reuse.
  conv("fragment pipeline: 3-stage ring form, 16x16x192 -> 160, three channel blocks", 160, 96, 1, 3, 1, 1, 0, 1, 16, 16, 192, true, 99);
  conv("fragment pipeline: two-stage form, 16x16x192 -> 160, three channel blocks", 160, 98, 1, 3, 1, 1, 0, 1, 16, 16, 192, true, 99);
  // split-K 3 over five channel blocks: slices [0, 2), [2, 4), [4, 5) -- the last has one block and no early read
  conv("fragment pipeline: 3-stage ring form, split-K 3 over 16x16x320 -> 160", 160, 96, 3, 3, 1, 1, 0, 1, 16, 16, 320, true, 99);
  conv("fragment pipeline: two-stage form, split-K 3 over 16x16x320 -> 160", 160, 98, 3, 3, 1, 1, 0, 1, 16, 16, 320, true, 99);
  { auto c = conv("fragment pipeline: GroupNorm + SiLU prologue form, 16x16x128 -> 160", 160, 98, 1, 3, 1, 1, 0, 1, 16, 16, 128, true, 0); c->gn_pro = 2; }
  int fails = 0, n = 0;
  for (const auto& c : cases) {
    if (argc > 1) {
      bool hit = false;
      for (int i = 1; i < argc; ++i) hit = hit || strstr(c.what, argv[i]);
      if (!hit) continue;
    }
    fails += run_case(c);
    ++n;
  }
  printf("%d cases, %d failed\n", n, fails);
  return fails;
}
