// Torch-free self test + micro benchmark of libpfd_hip.so (runs in seconds on a GPU box).
// Every kernel is checked against a straightforward fp64/fp32 CPU loop over the SAME fp16
// inputs.  This is test infrastructure: nothing here is linked into the product library.
//   build/selftest            -> correctness (exit code = number of failed cases)
//   build/selftest --bench    -> also time the UNet-shaped problems and print TFLOP/s
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <functional>
#include <random>
#include <string>
#include <array>
#include <atomic>
#include <thread>
#include <vector>

#include "pfd_hip.h"

typedef _Float16 h16;

#define HIP_OK(x)                                                                 \
  do {                                                                            \
    hipError_t e_ = (x);                                                          \
    if (e_ != hipSuccess) {                                                       \
      fprintf(stderr, "HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); \
      exit(99);                                                                   \
    }                                                                             \
  } while (0)

static std::mt19937 rng(1234);
static int g_fail = 0, g_total = 0;

static std::vector<h16> rand_h(size_t n, float scale = 1.f) {
  std::uniform_real_distribution<float> d(-1.f, 1.f);
  std::vector<h16> v(n);
  for (auto& x : v) x = (h16)(d(rng) * scale);
  return v;
}
static std::vector<float> rand_f(size_t n, float scale = 1.f) {
  std::uniform_real_distribution<float> d(-1.f, 1.f);
  std::vector<float> v(n);
  for (auto& x : v) x = d(rng) * scale;
  return v;
}
template <class T>
struct Dev {
  T* p = nullptr;
  size_t n = 0;
  Dev() {}
  explicit Dev(size_t n_) : n(n_) { HIP_OK(hipMalloc(&p, std::max<size_t>(n, 1) * sizeof(T))); HIP_OK(hipMemset(p, 0, std::max<size_t>(n,1) * sizeof(T))); }
  explicit Dev(const std::vector<T>& h) : n(h.size()) {
    HIP_OK(hipMalloc(&p, std::max<size_t>(n, 1) * sizeof(T)));
    HIP_OK(hipMemcpy(p, h.data(), n * sizeof(T), hipMemcpyHostToDevice));
  }
  ~Dev() { if (p) hipFree(p); }
  std::vector<T> get() const {
    std::vector<T> h(n);
    HIP_OK(hipDeviceSynchronize());
    HIP_OK(hipMemcpy(h.data(), p, n * sizeof(T), hipMemcpyDeviceToHost));
    return h;
  }
  Dev(const Dev&) = delete;
  Dev& operator=(const Dev&) = delete;
};

template <class T>
static void report(const std::string& name, const std::vector<T>& got, const std::vector<double>& ref,
                   double atol, double rtol) {
  double worst = 0, maxabs = 0;
  size_t bad = 0, worst_i = 0;
  for (size_t i = 0; i < ref.size(); ++i) {
    const double g = (double)got[i];
    const double d = fabs(g - ref[i]);
    const double lim = atol + rtol * fabs(ref[i]);
    if (!(d <= lim) || !std::isfinite(g)) ++bad;
    if (d / lim > worst || !std::isfinite(g)) { worst = std::isfinite(g) ? d / lim : 1e30; worst_i = i; }
    maxabs = std::max(maxabs, d);
  }
  ++g_total;
  if (bad) {
    ++g_fail;
    printf("FAIL %-58s bad=%zu/%zu max|d|=%.4g worst@%zu got=%.5g ref=%.5g\n", name.c_str(), bad, ref.size(),
           maxabs, worst_i, (double)got[worst_i], ref[worst_i]);
  } else {
    printf("ok   %-58s max|d|=%.3g\n", name.c_str(), maxabs);
  }
  fflush(stdout);
}

static double act_ref(double v, int act) {
  switch (act) {
    case PFD_ACT_GELU: return 0.5 * v * (1.0 + erf(v / sqrt(2.0)));
    case PFD_ACT_RELU: return v > 0 ? v : 0;
    case PFD_ACT_SILU: return v / (1.0 + exp(-v));
    default: return v;
  }
}



// the host references are plain fp64 loops: rows are independent, so they run on the box's host threads (the round-5
// candidate list took > 400 s single-threaded -- 6 s per case -- and was cut off by its GPU-call limit)
template <class F>
static void parallel_rows(int M, F&& body) {
  unsigned nt = std::thread::hardware_concurrency();
  nt = std::max(1u, std::min(nt ? nt : 1u, 48u));
  if (M < 64 || nt == 1) { for (int m = 0; m < M; ++m) body(m); return; }
  std::vector<std::thread> th;
  std::atomic<int> next{0};
  for (unsigned t = 0; t < nt; ++t)
    th.emplace_back([&]() { for (int m; (m = next.fetch_add(8)) < M;) for (int i = m; i < std::min(M, m + 8); ++i) body(i); });
  for (auto& t : th) t.join();
}

// ------------------------------------------------------------------ GEMM / conv
struct GemmCase {
  int M, N, K;
  int act = 0;
  bool bias = true, res = false, rowvec = false, bias_row = false;
  int tile = 0;
  int extra_ld = 0;  // added to every leading dimension
  int ksize = 0, stride = 1, pad = 0, ups = 0, B = 0, H = 0, W = 0, Cin = 0;
  int n_split = 0;  // > 0: columns >= n_split go transposed to Ct
  int w_tiled = 0;  // 1: the weight is uploaded K-tile-contiguous (PfdGemmDesc.w_tiled)
  int k_split = 0;  // > 0: columns >= k_split of the operand come from a second buffer (PfdGemmDesc.k_split)
  int zero_rows = 0;  // > 0: the first rows of the operand are all zero and not stored (PfdGemmDesc.zero_rows)
  int gn_out = 0;     // 1: the launch also emits the GroupNorm statistics of its output (PfdGemmDesc.gn_out)
  int res_rows = 0;   // > 0: the residual holds that many rows and is read with one wrap (PfdGemmDesc.res_rows)
  int declined = 0;   // 1: the library must answer PFD_ESHAPE and leave the output untouched
};

// PfdGemmDesc.ups = 2: the 3x3 weight [N][ldw >= 9 Cin] folded in fp32 and rounded once into four 2x2-tap phase blocks
// [py][px][N][ldf >= 4 Cin]; phase tap (ty, tx) sums the 3x3 taps that read the same low-res pixel
static std::vector<h16> fold_phase_weight(const std::vector<h16>& W, int N, int Cin, long ldw, long ldf) {
  auto taps = [](int ph, int t, int* lo, int* hi) { *lo = ph == 0 ? (t == 0 ? 0 : 1) : (t == 0 ? 0 : 2); *hi = ph == 0 ? (t == 0 ? 0 : 2) : (t == 0 ? 1 : 2); };
  std::vector<h16> out((size_t)4 * N * ldf, (h16)0);
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
                for (int kx = x0; kx <= x1; ++kx) a += (float)W[(size_t)n * ldw + (ky * 3 + kx) * Cin + ci];
              out[((size_t)(py * 2 + px) * N + n) * ldf + (ty * 2 + tx) * Cin + ci] = (h16)a;
            }
          }
  return out;
}

static void run_gemm_case(const GemmCase& c) {
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
  const long lda = (conv ? c.Cin : K) + c.extra_ld, ldw = K + c.extra_ld;
  const int Nout = c.act == PFD_ACT_GEGLU ? N / 2 : N;
  const long ldc = Nout + c.extra_ld, ldr = Nout + c.extra_ld, ldrv = N + c.extra_ld;
  const long a_rows = conv ? (long)c.B * c.H * c.W : M;
  const float ws = 1.0f / sqrtf((float)K);
  auto A = rand_h(a_rows * lda), W = rand_h((size_t)N * ldw, ws * 1.7f);
  auto bias = rand_h(c.bias_row ? M : N, 0.5f);
  const int rows_per_rv = conv ? Ho * Wo : 64;
  const int n_rv = (M + rows_per_rv - 1) / rows_per_rv;
  auto rv = rand_h((size_t)n_rv * ldrv, 0.5f);
  auto R = rand_h((size_t)M * ldr, 1.0f);
  std::vector<h16> Wup = W;
  // what the device contracts over: the four folded phase blocks of ups = 2 (the reference keeps the 9-tap weight)
  const int Kd = c.ups == 2 ? 4 * c.Cin : K, nblk = c.ups == 2 ? 4 : 1;
  const long ldwd = Kd + c.extra_ld;
  if (c.ups == 2) Wup = fold_phase_weight(W, N, c.Cin, ldw, ldwd);
  if (c.w_tiled) {   // (n, k) -> (((n / T) * (K / 64) + k / 64) * T + n % T) * 64 + k % 64, per weight block
    const int T = N % 160 == 0 ? 160 : 128, nkt = Kd / 64;
    const std::vector<h16> Wsrc = Wup;
    Wup.assign((size_t)nblk * N * Kd, (h16)0);
    for (int bl = 0; bl < nblk; ++bl)
      for (int n = 0; n < N; ++n)
        for (int k = 0; k < Kd; ++k)
          Wup[(size_t)bl * N * Kd + (((size_t)(n / T) * nkt + k / 64) * T + n % T) * 64 + k % 64] = Wsrc[((size_t)bl * N + n) * ldwd + k];
  }
  for (long r = 0; r < c.zero_rows; ++r)                     // the reference sees zero rows ...
    for (long k = 0; k < lda; ++k) A[r * lda + k] = (h16)0;
  // ... the device sees the operand without them, and split in two buffers at k_split (second one with its own stride)
  const long lda2 = c.k_split ? (K - c.k_split) + 8 : 8;
  std::vector<h16> Adev(A.begin() + (long)c.zero_rows * lda, A.end()), A2dev((size_t)std::max<long>(1, M - c.zero_rows) * lda2);
  if (c.k_split)
    for (long r = 0; r < M - c.zero_rows; ++r)
      for (long k = c.k_split; k < K; ++k) {
        A2dev[r * lda2 + (k - c.k_split)] = Adev[r * lda + k];
        Adev[r * lda + k] = (h16)7.0f;                        // must never be read
      }
  Dev<h16> dA(Adev), dA2(A2dev), dW(Wup), dB(bias), dRV(rv), dR(R), dC((size_t)M * ldc);
  Dev<float> dWS((size_t)8 * M * N + 64);
  PfdGemmDesc d;
  memset(&d, 0, sizeof(d));
  d.ws = dWS.p; d.ws_bytes = ((size_t)8 * M * N + 64) * sizeof(float);
  d.A = dA.p; d.W = dW.p; d.bias = c.bias ? dB.p : nullptr; d.rowvec = c.rowvec ? dRV.p : nullptr;
  d.R = c.res ? dR.p : nullptr; d.C = dC.p;
  d.lda = lda; d.ldw = ldwd; d.ldr = ldr; d.ldc = ldc; d.ldrv = ldrv;
  d.M = M; d.N = N; d.K = Kd; d.rows_per_rv = rows_per_rv; d.act = c.act; d.bias_per_row = c.bias_row;
  d.ksize = c.ksize; d.stride = c.stride; d.pad = c.pad; d.ups = c.ups;
  d.B = c.B; d.H = c.H; d.Wd = c.W; d.Cin = c.Cin; d.Ho = Ho; d.Wo = Wo;
  const long ldct = (M + 7) / 8 * 8 + 8;
  Dev<h16> dCt(c.n_split > 0 ? (size_t)(N - c.n_split) * ldct : 8);
  if (c.n_split > 0) { d.Ct = dCt.p; d.ldct = ldct; d.n_split = c.n_split; }
  d.w_tiled = c.w_tiled;
  if (c.k_split) { d.A2 = dA2.p; d.lda2 = lda2; d.k_split = c.k_split; }
  d.zero_rows = c.zero_rows;
  d.res_rows = c.res_rows;
  Dev<float> dGn(c.gn_out ? (size_t)(M / 64) * (N / 160) * 32 : 2);
  if (c.gn_out) {
    HIP_OK(hipMemset(dGn.p, 0xFF, dGn.n * sizeof(float)));   // NaN pattern: every used slot must be written
    d.gn_out = dGn.p;
  }
  const int rc = pfd_gemm_f16_ex(&d, c.tile, nullptr);
  char name[256];
  snprintf(name, sizeof(name), "gemm M%d N%d K%d act%d b%d r%d rv%d br%d tile%d%s ks%d zr%d%s%s ld+%d %s", M, N, K, c.act,
           c.bias, c.res, c.rowvec, c.bias_row, c.tile, c.w_tiled ? "T" : "", c.k_split, c.zero_rows, c.gn_out ? " gn" : "",
           c.res_rows ? (" rr" + std::to_string(c.res_rows)).c_str() : "", c.extra_ld,
           conv ? (std::string("conv k") + std::to_string(c.ksize) + " s" + std::to_string(c.stride) + " p" +
                   std::to_string(c.pad) + " u" + std::to_string(c.ups))
                      .c_str()
                : "");
  if (c.declined) {   // nothing launched, nothing written (the output buffer is zero-filled at allocation)
    auto got = dC.get();
    size_t touched = 0;
    for (const auto& v : got) touched += (float)v != 0.f;
    ++g_total;
    const bool ok = rc == PFD_ESHAPE && touched == 0;
    if (!ok) ++g_fail;
    printf("%s %-58s declined: rc=%d, %zu elements written\n", ok ? "ok  " : "FAIL", name, rc, touched);
    return;
  }
  if (rc != 0) {
    ++g_total; ++g_fail;
    printf("FAIL %-58s rc=%d (%s)\n", name, rc, pfd_last_error());
    return;
  }
  auto got = dC.get();
  // CPU reference
  std::vector<double> pre((size_t)M * N);
  parallel_rows(M, [&](int m) {
    int b = 0, oy = 0, ox = 0;
    if (conv) { b = m / (Ho * Wo); oy = (m % (Ho * Wo)) / Wo; ox = m % Wo; }
    for (int n = 0; n < N; ++n) {
      double s = 0;
      if (!conv) {
        for (int k = 0; k < K; ++k) s += (double)A[m * lda + k] * (double)W[n * ldw + k];
      } else {
        const int Hin = c.ups ? 2 * c.H : c.H, Win = c.ups ? 2 * c.W : c.W;
        for (int ky = 0; ky < c.ksize; ++ky)
          for (int kx = 0; kx < c.ksize; ++kx) {
            int iy = oy * c.stride + ky - c.pad, ix = ox * c.stride + kx - c.pad;
            if (iy < 0 || iy >= Hin || ix < 0 || ix >= Win) continue;
            if (c.ups) { iy /= 2; ix /= 2; }
            const h16* ap = &A[(((long)b * c.H + iy) * c.W + ix) * lda];
            const h16* wp = &W[n * ldw + (ky * c.ksize + kx) * c.Cin];
            for (int ci = 0; ci < c.Cin; ++ci) s += (double)ap[ci] * (double)wp[ci];
          }
      }
      if (c.bias) s += (double)bias[c.bias_row ? m : n];
      if (c.rowvec) s += (double)rv[(m / rows_per_rv) * ldrv + n];
      pre[(size_t)m * N + n] = s;
    }
  });
  std::vector<double> ref((size_t)M * ldc, 0.0);
  std::vector<h16> gotc((size_t)M * ldc, (h16)0);
  if (c.n_split > 0) {  // transposed tail: [N - n_split, ldct], pad columns untouched
    auto gt = dCt.get();
    std::vector<double> rt(gt.size(), 0.0);
    for (int n = c.n_split; n < N; ++n)
      for (int m = 0; m < M; ++m) rt[(size_t)(n - c.n_split) * ldct + m] = pre[(size_t)m * N + n];
    report((std::string(name) + " [Ct]").c_str(), gt, rt, 4e-3, 3e-3);
  }
  for (int m = 0; m < M; ++m)
    for (int n = 0; n < (c.n_split > 0 ? c.n_split : Nout); ++n) {
      double v;
      if (c.act == PFD_ACT_GEGLU) {
        const int gr = (N % 160 == 0) ? 2 : 32;  // packing granularity of the kernel that serves this N
        const int blk = n / gr, j = n % gr;
        const double x = pre[(size_t)m * N + blk * 2 * gr + j], g = pre[(size_t)m * N + blk * 2 * gr + gr + j];
        v = x * act_ref(g, PFD_ACT_GELU);
      } else {
        v = act_ref(pre[(size_t)m * N + n], c.act);
      }
      if (c.res) v += (double)R[(c.res_rows > 0 && m >= c.res_rows ? m - c.res_rows : m) * ldr + n];
      ref[(size_t)m * ldc + n] = v;
      gotc[(size_t)m * ldc + n] = got[(size_t)m * ldc + n];
    }
  // the pad columns (ld+extra) must stay untouched (zero)
  for (int m = 0; m < M; ++m)
    for (long n = c.n_split > 0 ? c.n_split : Nout; n < ldc; ++n) gotc[(size_t)m * ldc + n] = got[(size_t)m * ldc + n];
  report(name, gotc, ref, 4e-3, 3e-3);
  if (c.gn_out) {   // the statistics must be the sums of the f16 values the launch stored, per 64-row slab and group of N / 32
    auto st = dGn.get();
    const int cpg = N / 32, tn = N / 160, ngl = 160 / cpg;
    std::vector<double> sref((size_t)(M / 64) * tn * 32, 0.0);
    std::vector<float> sgot(sref.size(), 0.f);
    for (int sl = 0; sl < M / 64; ++sl)
      for (int t = 0; t < tn; ++t)
        for (int gl = 0; gl < ngl; ++gl) {
          double a = 0, q = 0;
          for (int r = 0; r < 64; ++r)
            for (int cc = 0; cc < cpg; ++cc) {
              const double v = (double)got[(size_t)(sl * 64 + r) * ldc + t * 160 + gl * cpg + cc];
              a += v; q += v * v;
            }
          const size_t o = (((size_t)sl * tn + t) * 16 + gl) * 2;
          sref[o] = a; sref[o + 1] = q; sgot[o] = st[o]; sgot[o + 1] = st[o + 1];
        }
    // 2-D patch tiles (48- / 96-wide images) partition a sample into slabs of 64 tile-local rows, not 64 consecutive pixels:
    // what the consumer uses -- and what is compared then -- are the per-sample totals
    // (the phase form of the upsample convolution, ups = 2, orders a sample's rows (phase, y, x): per-sample totals as well)
    const bool tile2d = conv && c.ksize == 3 && c.stride == 1 && ((!c.ups && c.W != 16 && c.W != 32 && c.W != 64) || c.ups == 2);
    if (tile2d) {
      const int spS = Ho * Wo / 64;
      std::vector<double> tref((size_t)c.B * tn * 32, 0.0);
      std::vector<float> tgot(tref.size(), 0.f);
      for (int sl = 0; sl < M / 64; ++sl)
        for (int t = 0; t < tn; ++t)
          for (int k = 0; k < 2 * ngl; ++k) {
            const size_t o = (((size_t)sl * tn + t) * 16) * 2 + k, od = (((size_t)(sl / spS) * tn + t) * 16) * 2 + k;
            tref[od] += sref[o]; tgot[od] += sgot[o];
          }
      report((std::string(name) + " [gn_out, per sample]").c_str(), tgot, tref, 5e-2, 1e-4);
    } else {
      report((std::string(name) + " [gn_out]").c_str(), sgot, sref, 2e-2, 1e-4);
    }
  }
}

// K-tile-contiguous weights (PfdGemmDesc.w_tiled): every wide-tile kernel family, both tile widths, conv K walks, split-K
// conv3x3_narrow_kernel (round 6): 3x3 convolutions with N <= 16 output channels
static void run_narrow_conv_cases() {
  run_gemm_case({0, 4, 0, 0, true, false, false, false, 0, 0, 3, 1, 1, 0, 2, 16, 64, 320});    // the UNet head: 320 -> 4 on a 64-wide image
  run_gemm_case({0, 3, 0, 0, true, false, false, false, 0, 0, 3, 1, 1, 0, 1, 12, 40, 128});    // N = 3 (VAE conv_out), one ragged segment
  run_gemm_case({0, 4, 0, 0, false, false, false, false, 0, 8, 3, 1, 1, 0, 1, 9, 96, 64});     // no bias, ld + 8, 64 + 32 pixel segments
  run_gemm_case({0, 8, 0, 0, true, false, false, false, 0, 0, 3, 1, 1, 0, 1, 8, 16, 512});     // N = 8: two row groups store
  run_gemm_case({0, 13, 0, 0, true, false, false, false, 0, 0, 3, 1, 1, 0, 1, 5, 130, 64});    // N = 13: element stores, three segments
  run_gemm_case({0, 4, 0, PFD_ACT_SILU, true, false, false, false, 0, 0, 3, 1, 1, 0, 1, 8, 64, 64});   // an activation: the general kernel
}

// PfdGemmDesc.ups = 2 against the nearest-2x + 3x3 reference: one 256-row tile per phase, both tile widths, both forms of the
// loader-wave kernel, statistics, K-tile-contiguous phase blocks, several samples, a 4x16 image, and a declined request
static void run_ups_fold_cases() {
  { GemmCase c{0, 320, 0, 0, true, false, false, false, 0, 0, 3, 1, 1, 2, 1, 16, 16, 64}; c.gn_out = 1; run_gemm_case(c); }
  run_gemm_case({0, 160, 0, 0, true, false, false, false, 5800, 0, 3, 1, 1, 2, 1, 16, 16, 64});
  run_gemm_case({0, 128, 0, PFD_ACT_SILU, true, false, false, false, 0, 8, 3, 1, 1, 2, 1, 16, 16, 64});
  { GemmCase c{0, 160, 0, 0, false, false, false, false, 0, 0, 3, 1, 1, 2, 3, 8, 32, 128}; c.w_tiled = 1; run_gemm_case(c); }
  run_gemm_case({0, 320, 0, 0, true, false, false, false, 0, 0, 3, 1, 1, 2, 2, 16, 48, 64});
  { GemmCase c{0, 160, 0, 0, true, false, false, false, 0, 0, 3, 1, 1, 2, 1, 8, 8, 64}; c.declined = 1; run_gemm_case(c); }
  { GemmCase c{0, 160, 0, 0, true, true, false, false, 0, 0, 3, 1, 1, 2, 1, 16, 16, 64}; c.declined = 1; run_gemm_case(c); }   // residual: not served
}

static void run_tiled_weight_cases() {
  for (int v : {0, 3200, 3300, 3400, 3500, 5400, 5800, 5100, 5300, 9200, 9300}) {
    GemmCase a{700, 320, 1024, 0, true, true, true, false, v}; a.w_tiled = 1; run_gemm_case(a);
    GemmCase b{0, 320, 0, 0, true, true, false, false, v, 0, 3, 1, 1, 0, 3, 16, 16, 128}; b.w_tiled = 1; run_gemm_case(b);
  }
  { GemmCase c{600, 640, 320, PFD_ACT_GEGLU, true, false, false, false, 9400}; c.w_tiled = 1; run_gemm_case(c); }
  { GemmCase c{520, 960, 320, 0, false, false, false, false, 0}; c.n_split = 640; c.w_tiled = 1; run_gemm_case(c); }
  { GemmCase c{900, 320, 1536, 0, true, false, false, false, 3203}; c.w_tiled = 1; run_gemm_case(c); }
  { GemmCase c{600, 256, 512, 0, true, true, false, false, 5400}; c.w_tiled = 1; run_gemm_case(c); }          // 128-wide tiles
  { GemmCase c{0, 256, 0, PFD_ACT_SILU, true, true, true, false, 0, 0, 3, 1, 1, 0, 2, 9, 7, 128}; c.w_tiled = 1; run_gemm_case(c); }
  for (int v : {10800, 10600, 10900, 10802}) {   // patch kernels (tap / channel-block walk over the tiled K axis)
    GemmCase c{0, 320, 0, 0, true, true, true, false, v, 0, 3, 1, 1, 0, 2, 32, 32, 128}; c.w_tiled = 1; run_gemm_case(c);
    GemmCase e{0, 160, 0, PFD_ACT_SILU, true, false, true, false, v, 0, 3, 1, 1, 0, 1, 64, 64, 256}; e.w_tiled = 1; run_gemm_case(e);
  }
  { GemmCase c{0, 160, 0, PFD_ACT_SILU, true, false, true, false, 5800, 0, 3, 2, 1, 0, 5, 20, 16, 64}; c.w_tiled = 1; run_gemm_case(c); }   // stride 2
  { GemmCase c{0, 160, 0, 0, true, false, false, false, 5800, 0, 3, 1, 1, 1, 2, 9, 12, 64}; c.w_tiled = 1; run_gemm_case(c); }               // upsample
}

// ------------------------------------------------------------------ LayerNorm folded into the GEMM (ABI 7)
// x = producer GEMM output (+ residual) with ln_out; y = LN(x; gamma, beta) W^T + b computed by the consumer GEMM over
// the un-normalised x with the gamma-scaled weight, the column sums and b' -- against an fp64 LayerNorm -> Linear
// over the same f16 x.  Also: producer partial sums == pfd_ln_rowstats_f16 of the stored x.
static void run_ln_fold_case(int M, int C, int N, int act, int tile_prod, int tile_cons, int n_split) {
  const int Kp = 192;                       // producer contraction length
  const int P = C / 160;
  auto A0 = rand_h((size_t)M * Kp), W0 = rand_h((size_t)C * Kp, 0.12f), b0 = rand_h(C, 0.5f), R0 = rand_h((size_t)M * C, 2.0f);
  for (int m = 0; m < M; ++m)               // a per-row offset so that mean^2 >> var on some rows (cancellation check)
    for (int c = 0; c < C; ++c) R0[(size_t)m * C + c] = (h16)((float)R0[(size_t)m * C + c] + (m % 7 == 0 ? 6.0f : 0.3f));
  auto gam = rand_f(C, 0.5f), bet = rand_f(C, 0.3f);
  for (auto& g : gam) g += 1.0f;
  auto W1 = rand_h((size_t)N * C, 0.08f), b1 = rand_h(N, 0.5f);
  const float eps = 1e-5f;
  // packed operands of the fold: W' = f16(W o gamma), s_n = sum_k W'[n][k], b'_n = sum_k beta_k W[n][k] + b_n
  std::vector<h16> Wg((size_t)N * C), bp(N);
  std::vector<float> cs(N);
  for (int n = 0; n < N; ++n) {
    double sacc = 0, bacc = (double)b1[n];
    for (int k = 0; k < C; ++k) {
      const h16 w = (h16)((float)W1[(size_t)n * C + k] * gam[k]);
      Wg[(size_t)n * C + k] = w;
      sacc += (double)w;
      bacc += (double)bet[k] * (double)W1[(size_t)n * C + k];
    }
    cs[n] = (float)sacc;
    bp[n] = (h16)bacc;
  }
  Dev<h16> dA0(A0), dW0(W0), db0(b0), dR0(R0), dX((size_t)M * C), dWg(Wg), dbp(bp);
  Dev<float> dcs(cs), dst((size_t)M * P * 2), dst2((size_t)M * P * 2), dWS((size_t)8 * M * std::max(N, C) + 64);
  const int Nout = act == PFD_ACT_GEGLU ? N / 2 : (n_split > 0 ? n_split : N);
  Dev<h16> dY((size_t)M * Nout);
  const long ldct = (M + 7) / 8 * 8;
  Dev<h16> dCt(n_split > 0 ? (size_t)(N - n_split) * ldct : 8);
  char name[200];
  snprintf(name, sizeof(name), "ln-fold M%d C%d N%d act%d prod%d cons%d split%d", M, C, N, act, tile_prod, tile_cons, n_split);
  PfdGemmDesc d;
  memset(&d, 0, sizeof(d));
  d.A = dA0.p; d.W = dW0.p; d.bias = db0.p; d.R = dR0.p; d.C = dX.p;
  d.lda = Kp; d.ldw = Kp; d.ldr = C; d.ldc = C; d.M = M; d.N = C; d.K = Kp; d.rows_per_rv = 1;
  d.ws = dWS.p; d.ws_bytes = dWS.n * sizeof(float);
  d.ln_out = dst.p;
  int rc = pfd_gemm_f16_ex(&d, tile_prod, nullptr);
  if (rc == 0) rc = pfd_ln_rowstats_f16(dX.p, C, M, C, dst2.p, nullptr);
  PfdGemmDesc e;
  memset(&e, 0, sizeof(e));
  e.A = dX.p; e.W = dWg.p; e.bias = dbp.p; e.C = dY.p;
  e.lda = C; e.ldw = C; e.ldc = Nout; e.M = M; e.N = N; e.K = C; e.rows_per_rv = 1; e.act = act;
  e.ws = dWS.p; e.ws_bytes = dWS.n * sizeof(float);
  e.ln_stats = dst.p; e.ln_colsum = dcs.p; e.ln_parts = P; e.ln_eps = eps;
  if (n_split > 0) { e.Ct = dCt.p; e.ldct = ldct; e.n_split = n_split; }
  if (rc == 0) rc = pfd_gemm_f16_ex(&e, tile_cons, nullptr);
  if (rc != 0) { ++g_total; ++g_fail; printf("FAIL %-58s rc=%d (%s)\n", name, rc, pfd_last_error()); return; }
  auto X = dX.get();
  auto st = dst.get(), st2 = dst2.get();
  {  // statistics: producer epilogue vs stand-alone kernel vs fp64 over the stored x
    std::vector<double> ref(st.size());
    for (int m = 0; m < M; ++m)
      for (int p = 0; p < P; ++p) {
        double a = 0, q = 0;
        for (int c = 0; c < 160; ++c) { const double v = (double)X[(size_t)m * C + p * 160 + c]; a += v; q += v * v; }
        ref[((size_t)m * P + p) * 2] = a; ref[((size_t)m * P + p) * 2 + 1] = q;
      }
    report((std::string(name) + " [stats: epilogue]").c_str(), st, ref, 2e-2, 2e-5);
    report((std::string(name) + " [stats: kernel]").c_str(), st2, ref, 2e-2, 2e-5);
  }
  std::vector<double> pre((size_t)M * N);
  std::vector<double> xn(C);
  for (int m = 0; m < M; ++m) {
    double mu = 0, var = 0;
    for (int c = 0; c < C; ++c) mu += (double)X[(size_t)m * C + c];
    mu /= C;
    for (int c = 0; c < C; ++c) { const double dlt = (double)X[(size_t)m * C + c] - mu; var += dlt * dlt; }
    const double rstd = 1.0 / sqrt(var / C + eps);
    for (int c = 0; c < C; ++c) xn[c] = ((double)X[(size_t)m * C + c] - mu) * rstd * gam[c] + bet[c];
    for (int n = 0; n < N; ++n) {
      double a = (double)b1[n];
      for (int c = 0; c < C; ++c) a += xn[c] * (double)W1[(size_t)n * C + c];
      pre[(size_t)m * N + n] = a;
    }
  }
  auto got = dY.get();
  std::vector<double> ref((size_t)M * Nout);
  for (int m = 0; m < M; ++m)
    for (int n = 0; n < Nout; ++n) {
      if (act == PFD_ACT_GEGLU) {
        const int blk = n / 2, j = n % 2;
        ref[(size_t)m * Nout + n] = pre[(size_t)m * N + blk * 4 + j] * act_ref(pre[(size_t)m * N + blk * 4 + 2 + j], PFD_ACT_GELU);
      } else {
        ref[(size_t)m * Nout + n] = act_ref(pre[(size_t)m * N + n], act);
      }
    }
  report(name, got, ref, 1e-2, 6e-3);
  if (n_split > 0) {
    auto gt = dCt.get();
    std::vector<double> rt(gt.size(), 0.0);
    for (int n = n_split; n < N; ++n)
      for (int m = 0; m < M; ++m) rt[(size_t)(n - n_split) * ldct + m] = pre[(size_t)m * N + n];
    report((std::string(name) + " [Ct]").c_str(), gt, rt, 1e-2, 6e-3);
  }
}

// the same 3x3 / s1 / p1 convolution under two forced tile codes: the results must be the same bits, on every one of
// `reps` launches of the second code (a hand-over protocol that races shows up as a launch that differs)
static void run_conv_same_case(int B, int H, int W, int Cin, int N, int tile_a, int tile_b, bool res, int reps = 8) {
  const long M = (long)B * H * W, K = 9L * Cin;
  auto A = rand_h((size_t)M * Cin), Wt = rand_h((size_t)N * K, 1.7f / sqrtf((float)K)), Bv = rand_h(N), R = rand_h((size_t)M * N);
  Dev<h16> dA(A), dW(Wt), dB(Bv), dR(R), dC1((size_t)M * N), dC2((size_t)M * N);
  Dev<float> dWS((size_t)8 * M * N);
  PfdGemmDesc d;
  memset(&d, 0, sizeof(d));
  d.M = (int)M; d.N = N; d.K = (int)K; d.A = dA.p; d.W = dW.p; d.bias = dB.p; d.R = res ? dR.p : nullptr;
  d.lda = Cin; d.ldw = K; d.ldc = N; d.ldr = N; d.ldrv = N; d.rows_per_rv = 1;
  d.ksize = 3; d.stride = 1; d.pad = 1; d.B = B; d.H = H; d.Wd = W; d.Cin = Cin; d.Ho = H; d.Wo = W;
  d.ws = dWS.p; d.ws_bytes = (size_t)8 * M * N * sizeof(float);
  char name[160];
  snprintf(name, sizeof(name), "conv3x3 B%d %dx%d %d->%d tile %d == tile %d (bitwise, %d launches)%s", B, H, W, Cin, N, tile_a, tile_b, reps, res ? " +res" : "");
  ++g_total;
  d.C = dC1.p;
  int rc = pfd_gemm_f16_ex(&d, tile_a, nullptr);
  if (rc != 0) { ++g_fail; printf("FAIL %-58s rc=%d (%s)\n", name, rc, pfd_last_error()); return; }
  auto y1 = dC1.get();
  d.C = dC2.p;
  for (int r = 0; r < reps; ++r) {
    HIP_OK(hipMemset(dC2.p, 0xFF, (size_t)M * N * sizeof(h16)));
    rc = pfd_gemm_f16_ex(&d, tile_b, nullptr);
    if (rc != 0) { ++g_fail; printf("FAIL %-58s rc=%d (%s)\n", name, rc, pfd_last_error()); return; }
    auto y2 = dC2.get();
    if (memcmp(y1.data(), y2.data(), y1.size() * sizeof(h16))) {
      size_t nd = 0;
      for (size_t i = 0; i < y1.size(); ++i) nd += memcmp(&y1[i], &y2[i], sizeof(h16)) != 0;
      ++g_fail;
      printf("FAIL %-58s launch %d: %zu of %zu elements differ\n", name, r, nd, y1.size());
      return;
    }
  }
  printf("ok   %-58s\n", name);
}

// the same linear layer (bias, optional residual / split-K / two-source contraction / zero rows) under two forced tile
// codes: same bits, on every one of `reps` launches of the second code
static void run_lin_same_case(int M, int N, int K, int tile_a, int tile_b, bool res, int k_split = 0, int zero_rows = 0, int reps = 8) {
  auto A = rand_h((size_t)M * K), Wt = rand_h((size_t)N * K, 1.7f / sqrtf((float)K)), Bv = rand_h(N), R = rand_h((size_t)M * N);
  const int K1 = k_split > 0 ? k_split : K, K2 = K - K1, Mz = M - zero_rows;
  // operand rows below zero_rows are not stored; columns >= k_split live in a second buffer
  std::vector<h16> A1((size_t)Mz * K1), A2((size_t)Mz * (K2 > 0 ? K2 : 1));
  for (int m = 0; m < Mz; ++m) {
    for (int k = 0; k < K1; ++k) A1[(size_t)m * K1 + k] = A[(size_t)(m + zero_rows) * K + k];
    for (int k = 0; k < K2; ++k) A2[(size_t)m * K2 + k] = A[(size_t)(m + zero_rows) * K + K1 + k];
  }
  Dev<h16> dA(A1), dA2(A2), dW(Wt), dB(Bv), dR(R), dC1((size_t)M * N), dC2((size_t)M * N);
  Dev<float> dWS((size_t)8 * M * N);
  PfdGemmDesc d;
  memset(&d, 0, sizeof(d));
  d.M = M; d.N = N; d.K = K; d.A = dA.p; d.W = dW.p; d.bias = dB.p; d.R = res ? dR.p : nullptr;
  d.lda = K1; d.ldw = K; d.ldc = N; d.ldr = N; d.ldrv = N; d.rows_per_rv = 1;
  if (k_split > 0) { d.k_split = k_split; d.A2 = dA2.p; d.lda2 = K2; }
  d.zero_rows = zero_rows;
  d.ws = dWS.p; d.ws_bytes = (size_t)8 * M * N * sizeof(float);
  char name[200];
  snprintf(name, sizeof(name), "linear %dx%dx%d tile %d == tile %d (bitwise, %d launches)%s ks%d zr%d", M, N, K, tile_a, tile_b, reps,
           res ? " +res" : "", k_split, zero_rows);
  ++g_total;
  d.C = dC1.p;
  int rc = pfd_gemm_f16_ex(&d, tile_a, nullptr);
  if (rc != 0) { ++g_fail; printf("FAIL %-58s rc=%d (%s)\n", name, rc, pfd_last_error()); return; }
  auto y1 = dC1.get();
  d.C = dC2.p;
  for (int r = 0; r < reps; ++r) {
    HIP_OK(hipMemset(dC2.p, 0xFF, (size_t)M * N * sizeof(h16)));
    rc = pfd_gemm_f16_ex(&d, tile_b, nullptr);
    if (rc != 0) { ++g_fail; printf("FAIL %-58s rc=%d (%s)\n", name, rc, pfd_last_error()); return; }
    auto y2 = dC2.get();
    if (memcmp(y1.data(), y2.data(), y1.size() * sizeof(h16))) {
      size_t nd = 0;
      for (size_t i = 0; i < y1.size(); ++i) nd += memcmp(&y1[i], &y2[i], sizeof(h16)) != 0;
      ++g_fail;
      printf("FAIL %-58s launch %d: %zu of %zu elements differ\n", name, r, nd, y1.size());
      return;
    }
  }
  printf("ok   %-58s\n", name);
}

// pfd_add_rowvec_lnstats_f16 == pfd_add_rowvec_f16 followed by pfd_ln_rowstats_f16, bit for bit (values and statistics)
static void run_add_rowvec_lnstats_case(int R, int C) {
  auto X = rand_h((size_t)R * C, 3.0f), V = rand_h(C, 1.0f);
  Dev<h16> dX(X), dV(V), dY1((size_t)R * C), dY2((size_t)R * C);
  const int P = C / 160;
  Dev<float> s1((size_t)R * P * 2), s2((size_t)R * P * 2);
  int rc = pfd_add_rowvec_lnstats_f16(dX.p, C, dV.p, dY1.p, C, R, C, s1.p, nullptr);
  if (rc == 0) rc = pfd_add_rowvec_f16(dX.p, C, dV.p, dY2.p, C, R, C, nullptr);
  if (rc == 0) rc = pfd_ln_rowstats_f16(dY2.p, C, R, C, s2.p, nullptr);
  char name[128];
  snprintf(name, sizeof(name), "add_rowvec + row statistics R%d C%d (bitwise vs two launches)", R, C);
  ++g_total;
  if (rc != 0) { ++g_fail; printf("FAIL %-58s rc=%d (%s)\n", name, rc, pfd_last_error()); return; }
  auto y1 = dY1.get(), y2 = dY2.get();
  auto a = s1.get(), b = s2.get();
  const bool same = !memcmp(y1.data(), y2.data(), y1.size() * sizeof(h16)) && !memcmp(a.data(), b.data(), a.size() * sizeof(float));
  if (!same) { ++g_fail; printf("FAIL %-58s outputs differ\n", name); }
  else printf("ok   %-58s\n", name);
}

static void run_ln_fold_suite() {
  run_add_rowvec_lnstats_case(130, 320);
  run_add_rowvec_lnstats_case(77, 1280);
  run_ln_fold_case(300, 320, 960, 0, 0, 0, 640);            // fused q | k | v^T of a 320-wide block (transposed tail)
  run_ln_fold_case(700, 320, 320, 0, 3400, 3400, 0);        // 128-row tiles, 4 waves
  run_ln_fold_case(520, 640, 640, 0, 9200, 9200, 0);        // 128-row tiles, 8 waves
  run_ln_fold_case(300, 640, 1280, PFD_ACT_GEGLU, 5400, 5400, 0);   // GEGLU, 256-row tiles
  run_ln_fold_case(600, 320, 640, PFD_ACT_GEGLU, 3200, 9400, 0);    // 256 x 320 GEGLU tile; 64-row producer
  run_ln_fold_case(130, 1280, 320, 0, 3204, 3204, 0);       // split-K on both sides (stats by the stand-alone kernel)
  run_ln_fold_case(200, 1280, 1280, PFD_ACT_GELU, 5300, 3300, 0);   // 8-wave 64-row ring producer, 4-wave ring consumer
  run_ln_fold_case(77, 960, 160, 0, 9300, 3500, 0);         // ragged M, 6 partials
}

// ------------------------------------------------------------------ attention
// spike > 0: key `spike` of every (b, h) is set to 4 x query (spike % Nq) -- its score jumps far above everything before
// it, which forces the running-maximum update (and the deferred-rescale path of the folded form) in the middle of the stream
static void run_attn_case(int B, int H, int Nq, int Nk, int D, bool fused_layout, int spike = 0) {
  const int C = H * D;
  const float scale = 1.0f / sqrtf((float)D);
  // fused_layout: Q and K are column slices of one [B*N, 2C] matrix (self-attention producer layout)
  const long ldq = fused_layout ? 2 * C : C, ldk = ldq, ldo = C;
  const int Nkp = (Nk + 7) / 8 * 8;
  const long ldvt = (long)B * Nkp;
  auto Qh = rand_h((size_t)B * Nq * ldq, 1.5f), Kh = rand_h((size_t)B * Nk * ldk, 1.5f), Vt = rand_h((size_t)C * ldvt, 1.0f);
  if (spike > 0 && spike < Nk) {
    const int koff0 = fused_layout ? C : 0;
    for (int b = 0; b < B; ++b)
      for (int c = 0; c < C; ++c)
        Kh[(size_t)b * Nk * ldk + (size_t)spike * ldk + koff0 + c] =
            (h16)(4.0f * (float)Qh[(size_t)b * Nq * ldq + (size_t)(spike % Nq) * ldq + c]);
  }
  Dev<h16> dQ(Qh), dK(Kh), dV(Vt), dO((size_t)B * Nq * ldo);
  PfdAttnDesc d;
  memset(&d, 0, sizeof(d));
  d.Q = dQ.p; d.K = fused_layout ? dK.p + C : dK.p; d.Vt = dV.p; d.O = dO.p;
  d.ldq = ldq; d.ldk = ldk; d.ldvt = ldvt; d.ldo = ldo;
  d.q_bs = (long)Nq * ldq; d.k_bs = (long)Nk * ldk; d.vt_bs = Nkp; d.o_bs = (long)Nq * ldo;
  d.B = B; d.H = H; d.Nq = Nq; d.Nk = Nk; d.D = D; d.scale = scale;
  const int rc = pfd_attention_f16(&d, nullptr);
  char name[128];
  snprintf(name, sizeof(name), "attention B%d H%d Nq%d Nk%d D%d fused%d spike%d", B, H, Nq, Nk, D, (int)fused_layout, spike);
  if (rc != 0) { ++g_total; ++g_fail; printf("FAIL %-58s rc=%d (%s)\n", name, rc, pfd_last_error()); return; }
  auto got = dO.get();
  std::vector<double> ref(got.size(), 0.0);
  const int koff = fused_layout ? C : 0;
  std::vector<double> s(Nk);
  for (int b = 0; b < B; ++b)
    for (int h = 0; h < H; ++h)
      for (int i = 0; i < Nq; ++i) {
        double mx = -1e300;
        for (int j = 0; j < Nk; ++j) {
          double a = 0;
          for (int e = 0; e < D; ++e)
            a += (double)Qh[(size_t)b * Nq * ldq + i * ldq + h * D + e] * (double)Kh[(size_t)b * Nk * ldk + j * ldk + koff + h * D + e];
          s[j] = a * scale;
          mx = std::max(mx, s[j]);
        }
        double sum = 0;
        for (int j = 0; j < Nk; ++j) { s[j] = exp(s[j] - mx); sum += s[j]; }
        for (int e = 0; e < D; ++e) {
          double o = 0;
          for (int j = 0; j < Nk; ++j) o += s[j] * (double)Vt[(size_t)(h * D + e) * ldvt + b * Nkp + j];
          ref[(size_t)b * Nq * ldo + i * ldo + h * D + e] = o / sum;
        }
      }
  report(name, got, ref, 3e-3, 5e-3);
}

// ------------------------------------------------------------------ swin window attention
static void run_swin_case(int B, int H, int W, int nH, int shift) {
  const int C = nH * 32, ws = 12, NT = 144;
  const float scale = 1.0f / sqrtf(32.f);
  auto qkv = rand_h((size_t)B * H * W * 3 * C, 1.5f), qb = rand_h(3 * C, 0.5f), rpb = rand_h(529 * nH, 1.0f);
  Dev<h16> dq(qkv), db(qb), dr(rpb), dout((size_t)B * H * W * C);
  PfdSwinAttnDesc d;
  memset(&d, 0, sizeof(d));
  d.qkv = dq.p; d.qkv_bias = db.p; d.rpb = dr.p; d.out = dout.p;
  d.B = B; d.H = H; d.W = W; d.C = C; d.nH = nH; d.ws = ws; d.shift = shift; d.scale = scale;
  const int rc = pfd_swin_window_attention_f16(&d, nullptr);
  char name[128];
  snprintf(name, sizeof(name), "swin_attn B%d H%d W%d nH%d shift%d", B, H, W, nH, shift);
  if (rc != 0) { ++g_total; ++g_fail; printf("FAIL %-58s rc=%d (%s)\n", name, rc, pfd_last_error()); return; }
  auto got = dout.get();
  std::vector<double> ref(got.size(), 0.0);
  const int Hp = (H + ws - 1) / ws * ws, Wp = (W + ws - 1) / ws * ws;
  // reference algorithm, literally: pad -> roll(-shift) -> partition -> attention -> reverse -> roll(+shift) -> crop
  auto src = [&](int b, int y, int x, int col) -> double {  // padded qkv
    if (y < H && x < W) return (double)qkv[((size_t)(b * H + y) * W + x) * 3 * C + col];
    return (double)qb[col];
  };
  std::vector<int> img_mask((size_t)Hp * Wp, 0);
  if (shift > 0) {
    int hs[4] = {0, Hp - ws, Hp - shift, Hp}, wsl[4] = {0, Wp - ws, Wp - shift, Wp}, cnt = 0;
    for (int a = 0; a < 3; ++a)
      for (int c2 = 0; c2 < 3; ++c2) {
        for (int y = hs[a]; y < hs[a + 1]; ++y)
          for (int x = wsl[c2]; x < wsl[c2 + 1]; ++x) img_mask[(size_t)y * Wp + x] = cnt;
        ++cnt;
      }
  }
  std::vector<double> sc(NT);
  for (int b = 0; b < B; ++b)
    for (int wy = 0; wy < Hp / ws; ++wy)
      for (int wx = 0; wx < Wp / ws; ++wx)
        for (int h = 0; h < nH; ++h)
          for (int i = 0; i < NT; ++i) {
            const int iy = i / ws, ix = i % ws;
            const int piy = wy * ws + iy, pix = wx * ws + ix;           // rolled frame
            const int oy = (piy + shift) % Hp, ox = (pix + shift) % Wp;  // original padded frame
            double mx = -1e300;
            for (int j = 0; j < NT; ++j) {
              const int jy = j / ws, jx = j % ws;
              const int pjy = wy * ws + jy, pjx = wx * ws + jx;
              const int ky = (pjy + shift) % Hp, kx = (pjx + shift) % Wp;
              double a = 0;
              for (int e = 0; e < 32; ++e)
                a += src(b, oy, ox, h * 32 + e) * scale * src(b, ky, kx, C + h * 32 + e);
              a += (double)rpb[((iy - jy + ws - 1) * (2 * ws - 1) + (ix - jx + ws - 1)) * nH + h];
              if (shift > 0 && img_mask[(size_t)piy * Wp + pix] != img_mask[(size_t)pjy * Wp + pjx]) a += -100.0;
              sc[j] = a;
              mx = std::max(mx, a);
            }
            double sum = 0;
            for (int j = 0; j < NT; ++j) { sc[j] = exp(sc[j] - mx); sum += sc[j]; }
            if (oy < H && ox < W)
              for (int e = 0; e < 32; ++e) {
                double o = 0;
                for (int j = 0; j < NT; ++j) {
                  const int jy = j / ws, jx = j % ws;
                  const int ky = (wy * ws + jy + shift) % Hp, kx = (wx * ws + jx + shift) % Wp;
                  o += sc[j] * src(b, ky, kx, 2 * C + h * 32 + e);
                }
                ref[((size_t)(b * H + oy) * W + ox) * C + h * 32 + e] = o / sum;
              }
          }
  report(name, got, ref, 3e-3, 5e-3);
}

// ------------------------------------------------------------------ norms
static void run_gn_case(int B, int HW, int C1, int C2, int G, int act, float eps) {
  const int C = C1 + C2;
  auto x1 = rand_h((size_t)B * HW * C1, 2.f), x2 = rand_h((size_t)B * HW * std::max(C2, 8), 1.f);
  for (auto& v : x1) v = (h16)((float)v + 0.7f);
  auto gm = rand_h(C, 1.f), bt = rand_h(C, 0.5f);
  Dev<h16> d1(x1), d2(x2), dg(gm), db(bt), dy((size_t)B * HW * C);
  const size_t wsb = pfd_groupnorm_ws_bytes(B, C, HW);
  Dev<char> dws(wsb);
  const int rc = pfd_groupnorm_f16(d1.p, C1, C1, C2 ? d2.p : nullptr, C2, C2, dg.p, db.p, dy.p, C, B, HW, G, eps, act,
                                   dws.p, wsb, nullptr);
  char name[128];
  snprintf(name, sizeof(name), "groupnorm B%d HW%d C%d+%d G%d act%d", B, HW, C1, C2, G, act);
  if (rc != 0) { ++g_total; ++g_fail; printf("FAIL %-58s rc=%d (%s)\n", name, rc, pfd_last_error()); return; }
  auto got = dy.get();
  std::vector<double> ref(got.size());
  const int cpg = C / G;
  auto X = [&](int b, int p, int c) -> double {
    return c < C1 ? (double)x1[((size_t)b * HW + p) * C1 + c] : (double)x2[((size_t)b * HW + p) * C2 + (c - C1)];
  };
  for (int b = 0; b < B; ++b)
    for (int g = 0; g < G; ++g) {
      double s = 0, q = 0;
      for (int p = 0; p < HW; ++p)
        for (int c = g * cpg; c < (g + 1) * cpg; ++c) { const double v = X(b, p, c); s += v; q += v * v; }
      const double n = (double)HW * cpg, mean = s / n, var = q / n - mean * mean, rstd = 1.0 / sqrt(var + eps);
      for (int p = 0; p < HW; ++p)
        for (int c = g * cpg; c < (g + 1) * cpg; ++c) {
          double v = (X(b, p, c) - mean) * rstd * (double)gm[c] + (double)bt[c];
          ref[((size_t)b * HW + p) * C + c] = act_ref(v, act);
        }
    }
  report(name, got, ref, 4e-3, 3e-3);
}

// conv3x3(act(GroupNorm([x1 | x2]))) two ways: pfd_groupnorm_f16 + plain patch conv vs pfd_groupnorm_table_f16 + the
// conv's GroupNorm prologue.  Same statistics code, same fp32 affine map, same kernel behind it: the outputs must be
// identical, not merely close.
// PfdGemmDesc.gnf_y (ABI 9): GroupNorm(32)(+SiLU) of a convolution's output inside its split-K reduction launch vs the two-call
// form (the same convolution without the request, then pfd_groupnorm_f16 on its output): the same bits, raw and normalised
static void run_gnf_case(int B, int H, int W, int Cin, int N, int act_gn, float eps, bool res, bool rowvec, bool keep_raw, int tile = 0) {
  const int HW = H * W, M = B * HW, K = 9 * Cin;
  auto A = rand_h((size_t)M * Cin), Wt = rand_h((size_t)N * K, 1.7f / sqrtf((float)K)), bias = rand_h(N, 0.5f);
  auto rv = rand_h((size_t)B * N, 0.5f), R = rand_h((size_t)M * N, 1.0f), gm = rand_h(N, 1.f), bt = rand_h(N, 0.5f);
  Dev<h16> dA(A), dW(Wt), dB(bias), dRV(rv), dR(R), dG(gm), dBt(bt), dC((size_t)M * N), dC2((size_t)M * N), dY((size_t)M * N), dY2((size_t)M * N);
  Dev<float> dWS((size_t)8 * M * N + 64);
  PfdGemmDesc d;
  memset(&d, 0, sizeof(d));
  d.A = dA.p; d.W = dW.p; d.bias = dB.p; d.rowvec = rowvec ? dRV.p : nullptr; d.R = res ? dR.p : nullptr; d.C = dC.p;
  d.lda = Cin; d.ldw = K; d.ldc = N; d.ldr = N; d.ldrv = N;
  d.M = M; d.N = N; d.K = K; d.rows_per_rv = HW; d.act = 0;
  d.ksize = 3; d.stride = 1; d.pad = 1; d.B = B; d.H = H; d.Wd = W; d.Cin = Cin; d.Ho = H; d.Wo = W;
  d.ws = dWS.p; d.ws_bytes = ((size_t)8 * M * N + 64) * sizeof(float);
  char name[200];
  snprintf(name, sizeof(name), "conv3x3 B%d %dx%d %d->%d + fused GroupNorm act%d res%d rv%d raw%d tile%d", B, H, W, Cin, N, act_gn, res, rowvec, keep_raw, tile);
  HIP_OK(hipMemset(dC.p, 0x3C, (size_t)M * N * sizeof(h16)));     // 1.0 pattern: an unwritten raw tensor stays recognisable
  PfdGemmDesc f = d;
  f.gnf_gamma = dG.p; f.gnf_beta = dBt.p; f.gnf_y = dY.p; f.gnf_ldy = N; f.gnf_eps = eps; f.gnf_act = act_gn; f.gnf_rows = HW;
  f.gnf_skip_raw = keep_raw ? 0 : 1;
  const int rc = tile ? pfd_gemm_f16_ex(&f, tile, nullptr) : pfd_gemm_f16(&f, nullptr);
  ++g_total;
  if (rc != 0) { ++g_fail; printf("FAIL %-58s rc=%d (%s)\n", name, rc, pfd_last_error()); return; }
  d.C = dC2.p;
  const size_t wsb = pfd_groupnorm_ws_bytes(B, N, HW);
  Dev<char> dws(wsb);
  const int rc2 = tile ? pfd_gemm_f16_ex(&d, tile, nullptr) : pfd_gemm_f16(&d, nullptr);
  const int rc3 = pfd_groupnorm_f16(dC2.p, N, N, nullptr, 0, 0, dG.p, dBt.p, dY2.p, N, B, HW, 32, eps, act_gn, dws.p, wsb, nullptr);
  auto y = dY.get(), y2 = dY2.get(), c = dC.get(), c2 = dC2.get();
  size_t ny = 0, nc = 0, nraw_written = 0;
  for (size_t i = 0; i < y.size(); ++i) {
    ny += memcmp(&y[i], &y2[i], sizeof(h16)) != 0;
    nc += memcmp(&c[i], &c2[i], sizeof(h16)) != 0;
    const unsigned short one = 0x3C3C;
    nraw_written += memcmp(&c[i], &one, sizeof(h16)) != 0;
  }
  // 20 channels per group (N = 640, round 6): pfd_groupnorm_f16 takes its two-launch form there, whose statistics are summed in another
  // order -- the normalised tensors then agree except for last-bit roundings (< 0.1 % of the elements); the raw tensor stays bitwise
  const bool bitwise = N / 32 >= 32;
  const bool ok = rc2 == 0 && rc3 == 0 && (bitwise ? ny == 0 : ny * 1000 < y.size()) && (keep_raw ? nc == 0 : nraw_written == 0);
  if (!ok) {
    ++g_fail;
    printf("FAIL %-58s rc %d %d: normalised %zu of %zu elements differ, raw %zu differ, raw written %zu\n", name, rc2, rc3, ny, y.size(), nc, nraw_written);
  } else {
    printf("ok   %-58s == conv + groupnorm (%s)%s\n", name, bitwise ? "bitwise" : "last-bit roundings of the statistics order only",
           keep_raw ? ", raw too (bitwise)" : ", raw tensor not written");
  }
  // and the two-call form itself against fp64 (so that "the same bits" is not the same wrong bits): GroupNorm of the stored raw tensor
  std::vector<double> ref(y2.size());
  const int cpg = N / 32;
  for (int b = 0; b < B; ++b)
    for (int g = 0; g < 32; ++g) {
      double sm = 0, q = 0;
      for (int p = 0; p < HW; ++p)
        for (int ch = g * cpg; ch < (g + 1) * cpg; ++ch) { const double v = (double)c2[((size_t)b * HW + p) * N + ch]; sm += v; q += v * v; }
      const double n = (double)HW * cpg, mean = sm / n, rstd = 1.0 / sqrt(q / n - mean * mean + eps);
      for (int p = 0; p < HW; ++p)
        for (int ch = g * cpg; ch < (g + 1) * cpg; ++ch)
          ref[((size_t)b * HW + p) * N + ch] = act_ref(((double)c2[((size_t)b * HW + p) * N + ch] - mean) * rstd * (double)gm[ch] + (double)bt[ch], act_gn);
    }
  report((std::string(name) + " [vs fp64]").c_str(), y, ref, 4e-3, 3e-3);
}

// a request the library must decline with NOTHING launched (a problem it does not split / a width without the fused form)
static void run_gnf_decline_case(int B, int H, int W, int Cin, int N) {
  const int HW = H * W, M = B * HW, K = 9 * Cin;
  Dev<h16> dA(rand_h((size_t)M * Cin)), dW(rand_h((size_t)N * K, 0.02f)), dB(rand_h(N, 0.5f)), dG(rand_h(N, 1.f)), dBt(rand_h(N, 0.5f));
  Dev<h16> dC((size_t)M * N), dY((size_t)M * N);
  Dev<float> dWS((size_t)8 * M * N + 64);
  HIP_OK(hipMemset(dC.p, 0x3C, (size_t)M * N * sizeof(h16)));
  HIP_OK(hipMemset(dY.p, 0x3C, (size_t)M * N * sizeof(h16)));
  PfdGemmDesc d;
  memset(&d, 0, sizeof(d));
  d.A = dA.p; d.W = dW.p; d.bias = dB.p; d.C = dC.p; d.lda = Cin; d.ldw = K; d.ldc = N; d.M = M; d.N = N; d.K = K; d.rows_per_rv = HW;
  d.ksize = 3; d.stride = 1; d.pad = 1; d.B = B; d.H = H; d.Wd = W; d.Cin = Cin; d.Ho = H; d.Wo = W;
  d.ws = dWS.p; d.ws_bytes = ((size_t)8 * M * N + 64) * sizeof(float);
  d.gnf_gamma = dG.p; d.gnf_beta = dBt.p; d.gnf_y = dY.p; d.gnf_ldy = N; d.gnf_eps = 1e-5f; d.gnf_act = PFD_ACT_SILU; d.gnf_rows = HW;
  const int rc = pfd_gemm_f16(&d, nullptr);
  HIP_OK(hipDeviceSynchronize());
  auto c = dC.get(), y = dY.get();
  size_t touched = 0;
  const unsigned short one = 0x3C3C;
  for (size_t i = 0; i < c.size(); ++i) touched += (memcmp(&c[i], &one, 2) != 0) + (memcmp(&y[i], &one, 2) != 0);
  ++g_total;
  char name[160];
  snprintf(name, sizeof(name), "conv3x3 B%d %dx%d %d->%d fused GroupNorm request declined", B, H, W, Cin, N);
  if (rc != PFD_ESHAPE || touched) { ++g_fail; printf("FAIL %-58s rc=%d, %zu elements written\n", name, rc, touched); }
  else printf("ok   %-58s PFD_ESHAPE, nothing written\n", name);
}

// pfd_groupnorm_pstats_f16: statistics handed over in the producers' layout (host-computed here) vs a plain fp64 GroupNorm
static void run_gn_pstats_case(int B, int HW, int C1, int C2, int act, float eps) {
  const int C = C1 + C2, G = 32, cpg = C / G;
  auto x1 = rand_h((size_t)B * HW * C1), x2 = rand_h((size_t)B * HW * std::max(C2, 8)), gm = rand_h(C), bt = rand_h(C);
  for (auto& v : x1) v = (h16)((float)v * 1.5f + 0.3f);
  auto mk_stats = [&](const std::vector<h16>& x, int Cs) {
    const int cpp = Cs / 32, tn = Cs / 160;
    std::vector<float> st((size_t)(B * HW / 64) * tn * 32, 0.f);
    for (int sl = 0; sl < B * HW / 64; ++sl)
      for (int c = 0; c < Cs; ++c) {
        double a = 0, q = 0;
        for (int r = 0; r < 64; ++r) { const double v = (double)x[(size_t)(sl * 64 + r) * Cs + c]; a += v; q += v * v; }
        const size_t o = (((size_t)sl * tn + c / 160) * 16 + (c % 160) / cpp) * 2;
        st[o] += (float)a; st[o + 1] += (float)q;
      }
    return st;
  };
  auto s1 = mk_stats(x1, C1);
  std::vector<float> s2 = C2 ? mk_stats(x2, C2) : std::vector<float>(2, 0.f);
  Dev<h16> d1(x1), d2(x2), dg(gm), db(bt), dy((size_t)B * HW * C);
  Dev<float> ds1(s1), ds2(s2);
  char name[160];
  snprintf(name, sizeof(name), "groupnorm pstats B%d HW%d C%d+%d act%d", B, HW, C1, C2, act);
  if (!pfd_groupnorm_takes_pstats(B, C1, C2, HW, G)) { ++g_total; ++g_fail; printf("FAIL %s: shape refused\n", name); return; }
  const int rc = pfd_groupnorm_pstats_f16(d1.p, C1, C1, ds1.p, C2 ? d2.p : nullptr, C2, C2, C2 ? ds2.p : nullptr, dg.p, db.p, dy.p, C,
                                          B, HW, G, eps, act, nullptr);
  if (rc != 0) { ++g_total; ++g_fail; printf("FAIL %s rc=%d (%s)\n", name, rc, pfd_last_error()); return; }
  auto got = dy.get();
  std::vector<double> ref((size_t)B * HW * C);
  auto at = [&](int b, int r, int c) { return c < C1 ? (double)x1[((size_t)b * HW + r) * C1 + c] : (double)x2[((size_t)b * HW + r) * C2 + c - C1]; };
  for (int b = 0; b < B; ++b)
    for (int g = 0; g < G; ++g) {
      double a = 0, q = 0;
      for (int r = 0; r < HW; ++r)
        for (int c = g * cpg; c < (g + 1) * cpg; ++c) { const double v = at(b, r, c); a += v; q += v * v; }
      const double n = (double)HW * cpg, mean = a / n, rstd = 1.0 / sqrt(std::max(q / n - mean * mean, 0.0) + eps);
      for (int r = 0; r < HW; ++r)
        for (int c = g * cpg; c < (g + 1) * cpg; ++c)
          ref[((size_t)b * HW + r) * C + c] = act_ref((at(b, r, c) - mean) * rstd * (double)gm[c] + (double)bt[c], act);
    }
  report(name, got, ref, 6e-3, 4e-3);
}

static void run_gn_conv_case(int B, int H, int W, int C1, int C2, int N, int act, bool with_res) {
  const int C = C1 + C2, HW = H * W, G = 32, M = B * HW, K = 9 * C;
  const float eps = 1e-5f;
  auto x1 = rand_h((size_t)M * C1, 2.f), x2 = rand_h((size_t)M * std::max(C2, 8), 1.f);
  for (auto& v : x1) v = (h16)((float)v + 0.7f);
  auto gm = rand_h(C, 1.f), bt = rand_h(C, 0.5f);
  auto Wt = rand_h((size_t)N * K, 0.05f), bias = rand_h(N, 0.5f), R = rand_h((size_t)M * N, 1.f);
  auto rv = rand_h((size_t)B * N, 0.5f);
  Dev<h16> d1(x1), d2(x2), dg(gm), db(bt), dy((size_t)M * C), dW(Wt), dB(bias), dR(R), dRV(rv);
  Dev<h16> dC0((size_t)M * N), dC1((size_t)M * N);
  Dev<float> dT((size_t)B * C * 2);
  const size_t wsb = pfd_groupnorm_ws_bytes(B, C, HW);
  Dev<char> dws(wsb);
  Dev<float> dWS((size_t)8 * M * N + 64);
  char name[160];
  snprintf(name, sizeof(name), "gn-prologue conv B%d %dx%d C%d+%d N%d act%d res%d", B, H, W, C1, C2, N, act, (int)with_res);
  int rc = pfd_groupnorm_f16(d1.p, C1, C1, C2 ? d2.p : nullptr, C2, C2, dg.p, db.p, dy.p, C, B, HW, G, eps, act, dws.p,
                             wsb, nullptr);
  PfdGemmDesc d;
  memset(&d, 0, sizeof(d));
  d.ws = dWS.p; d.ws_bytes = ((size_t)8 * M * N + 64) * sizeof(float);
  d.A = dy.p; d.W = dW.p; d.bias = dB.p; d.rowvec = dRV.p; d.R = with_res ? dR.p : nullptr; d.C = dC0.p;
  d.lda = C; d.ldw = K; d.ldr = N; d.ldc = N; d.ldrv = N;
  d.M = M; d.N = N; d.K = K; d.rows_per_rv = HW;
  d.ksize = 3; d.stride = 1; d.pad = 1; d.B = B; d.H = H; d.Wd = W; d.Cin = C; d.Ho = H; d.Wo = W;
  if (rc == 0) rc = pfd_gemm_f16_ex(&d, 10800, nullptr);
  if (rc == 0)
    rc = pfd_groupnorm_table_f16(d1.p, C1, C1, C2 ? d2.p : nullptr, C2, C2, dg.p, db.p, dT.p, B, HW, G, eps, dws.p, wsb,
                                 nullptr);
  d.A = d1.p; d.lda = C1; d.A2 = C2 ? d2.p : nullptr; d.lda2 = C2; d.gn_c1 = C1; d.gn_table = dT.p; d.gn_act = act;
  d.C = dC1.p;
  if (rc == 0) rc = pfd_gemm_f16(&d, nullptr);
  ++g_total;
  if (rc != 0) { ++g_fail; printf("FAIL %-58s rc=%d (%s)\n", name, rc, pfd_last_error()); return; }
  auto c0 = dC0.get(), c1 = dC1.get();
  size_t bad = 0;
  double worst = 0, mag = 0;
  for (size_t i = 0; i < c0.size(); ++i) {
    const double a = (double)c0[i], b = (double)c1[i];
    if (!(a == b)) { ++bad; worst = std::max(worst, fabs(a - b)); }
    mag = std::max(mag, fabs(a));
  }
  if (bad) { ++g_fail; printf("FAIL %-58s %zu of %zu differ, max |d| %.4g (max |ref| %.3g)\n", name, bad, c0.size(), worst, mag); }
  else printf("ok   %-58s identical (%zu values, max |ref| %.3g)\n", name, c0.size(), mag);
  // a shape the patch kernel does not take must be refused, not served by something else
  d.Wd = 8; d.H = H * W / 8; d.Ho = d.H; d.Wo = 8;
  ++g_total;
  const int rc2 = pfd_gemm_f16(&d, nullptr);
  if (rc2 != PFD_ESHAPE) { ++g_fail; printf("FAIL %-58s W=8 with gn_table: rc=%d, expected PFD_ESHAPE\n", name, rc2); }
}

static void run_ln_case(int M, int C, int gather4, int B, int H, int W) {
  const int Cq = C / 4;
  auto x = rand_h(gather4 ? (size_t)B * H * W * Cq : (size_t)M * C, 2.f);
  for (auto& v : x) v = (h16)((float)v - 0.4f);
  auto gm = rand_h(C, 1.f), bt = rand_h(C, 0.5f);
  Dev<h16> dx(x), dg(gm), db(bt), dy((size_t)M * C);
  const int rc = pfd_layernorm_f16(dx.p, gather4 ? Cq : C, dg.p, db.p, dy.p, C, M, C, 1e-5f, gather4, B, H, W, nullptr);
  char name[128];
  snprintf(name, sizeof(name), "layernorm M%d C%d gather%d", M, C, gather4);
  if (rc != 0) { ++g_total; ++g_fail; printf("FAIL %-58s rc=%d (%s)\n", name, rc, pfd_last_error()); return; }
  auto got = dy.get();
  std::vector<double> ref(got.size());
  const int Ho = (H + 1) / 2, Wo = (W + 1) / 2;
  for (int m = 0; m < M; ++m) {
    std::vector<double> row(C);
    for (int c = 0; c < C; ++c) {
      if (!gather4) row[c] = (double)x[(size_t)m * C + c];
      else {
        const int b = m / (Ho * Wo), oy = (m % (Ho * Wo)) / Wo, ox = m % Wo, part = c / Cq;
        const int iy = 2 * oy + (part & 1), ix = 2 * ox + (part >> 1);
        row[c] = (iy < H && ix < W) ? (double)x[(((size_t)b * H + iy) * W + ix) * Cq + c % Cq] : 0.0;
      }
    }
    double s = 0; for (double v : row) s += v;
    const double mean = s / C;
    double q = 0; for (double v : row) q += (v - mean) * (v - mean);
    const double rstd = 1.0 / sqrt(q / C + 1e-5);
    for (int c = 0; c < C; ++c) ref[(size_t)m * C + c] = (row[c] - mean) * rstd * (double)gm[c] + (double)bt[c];
  }
  report(name, got, ref, 4e-3, 3e-3);
}

static void run_softmax_case(int R, int N, float scale) {
  auto x = rand_h((size_t)R * N, 8.f);
  Dev<h16> dx(x), dy((size_t)R * N);
  const int rc = pfd_softmax_rows_f16(dx.p, N, dy.p, N, R, N, scale, nullptr);
  char name[128];
  snprintf(name, sizeof(name), "softmax_rows R%d N%d", R, N);
  if (rc != 0) { ++g_total; ++g_fail; printf("FAIL %-58s rc=%d\n", name, rc); return; }
  auto got = dy.get();
  std::vector<double> ref(got.size());
  for (int r = 0; r < R; ++r) {
    double mx = -1e300, s = 0;
    for (int j = 0; j < N; ++j) mx = std::max(mx, (double)x[(size_t)r * N + j] * scale);
    for (int j = 0; j < N; ++j) s += exp((double)x[(size_t)r * N + j] * scale - mx);
    for (int j = 0; j < N; ++j) ref[(size_t)r * N + j] = exp((double)x[(size_t)r * N + j] * scale - mx) / s;
  }
  report(name, got, ref, 1e-4, 5e-3);
}

// ------------------------------------------------------------------ elementwise
static void run_elementwise() {
  {  // layout conversions
    const int B = 2, C = 4, H = 9, W = 7, rep = 2;
    auto x = rand_f((size_t)B * C * H * W, 3.f);
    Dev<float> dx(x);
    Dev<h16> dy((size_t)rep * B * C * H * W);
    int rc = pfd_nchw_to_nhwc_f16(dx.p, 1, dy.p, B, C, H, W, 0.5f, 0.25f, rep, nullptr);
    auto got = dy.get();
    std::vector<double> ref(got.size());
    for (int r = 0; r < rep; ++r)
      for (int b = 0; b < B; ++b) for (int c = 0; c < C; ++c) for (int y = 0; y < H; ++y) for (int xx = 0; xx < W; ++xx)
        ref[(size_t)r * B * C * H * W + (((size_t)b * H + y) * W + xx) * C + c] = x[(((size_t)b * C + c) * H + y) * W + xx] * 0.5 + 0.25;
    report(std::string("nchw_to_nhwc f32 rep2 rc=") + std::to_string(rc), got, ref, 2e-3, 2e-3);
    auto xh = rand_h((size_t)B * H * W * 70, 2.f);
    Dev<h16> dxh(xh);
    Dev<float> dyf((size_t)B * 70 * H * W);
    rc = pfd_nhwc_to_nchw(dxh.p, dyf.p, 1, B, 70, H, W, 0.5f, 0.5f, 0.f, 1.f, nullptr);
    auto gotf = dyf.get();
    std::vector<double> reff(gotf.size());
    for (int b = 0; b < B; ++b) for (int c = 0; c < 70; ++c) for (int p = 0; p < H * W; ++p)
      reff[((size_t)b * 70 + c) * H * W + p] = std::min(1.0, std::max(0.0, (double)xh[((size_t)b * H * W + p) * 70 + c] * 0.5 + 0.5));
    report(std::string("nhwc_to_nchw f32 clamp rc=") + std::to_string(rc), gotf, reff, 1e-6, 1e-6);
  }
  {  // im2col
    const int B = 2, H = 6, W = 5, Cin = 4, ks = 3, st = 1, pad = 1, Ho = 6, Wo = 5, Kpad = 64;
    auto x = rand_h((size_t)B * H * W * Cin);
    Dev<h16> dx(x), dc((size_t)B * Ho * Wo * Kpad);
    int rc = pfd_im2col_f16(dx.p, Cin, dc.p, B, H, W, Cin, ks, st, pad, Ho, Wo, Kpad, nullptr);
    auto got = dc.get();
    std::vector<double> ref(got.size(), 0.0);
    for (int b = 0; b < B; ++b) for (int oy = 0; oy < Ho; ++oy) for (int ox = 0; ox < Wo; ++ox)
      for (int ky = 0; ky < ks; ++ky) for (int kx = 0; kx < ks; ++kx) for (int ci = 0; ci < Cin; ++ci) {
        const int iy = oy * st + ky - pad, ix = ox * st + kx - pad;
        if (iy < 0 || iy >= H || ix < 0 || ix >= W) continue;
        ref[(((size_t)b * Ho + oy) * Wo + ox) * Kpad + (ky * ks + kx) * Cin + ci] = (double)x[(((size_t)b * H + iy) * W + ix) * Cin + ci];
      }
    report(std::string("im2col k3 rc=") + std::to_string(rc), got, ref, 0, 0);
  }
  {  // timestep embedding
    const int B = 3, dim = 320;
    std::vector<int64_t> t = {1, 481, 981};
    Dev<int64_t> dt(t);
    Dev<h16> de((size_t)B * dim);
    int rc = pfd_timestep_embedding_f16(dt.p, de.p, B, dim, 10000.f, nullptr);
    auto got = de.get();
    std::vector<double> ref(got.size());
    for (int b = 0; b < B; ++b) for (int j = 0; j < dim; ++j) {
      const int f = j % 160;
      const double fr = exp(-log(10000.0) * f / 160.0);
      ref[b * dim + j] = j < 160 ? cos(t[b] * fr) : sin(t[b] * fr);
    }
    report(std::string("timestep_embedding rc=") + std::to_string(rc), got, ref, 2e-3, 1e-3);
  }
  {  // cfg + ddim
    const int B = 2, C = 4, h = 5, w = 6;
    const size_t n = (size_t)B * C * h * w;
    auto eps = rand_h(2 * n, 1.5f);
    auto x = rand_f(n, 2.f), nz = rand_f(n, 1.f);
    std::vector<float> coef = {0.45f, 0.52f, 0.1f, sqrtf(1 - 0.45f), 2.0f};
    Dev<h16> de(eps), dxin(2 * n);
    Dev<float> dx(x), dn(nz), dc(coef), dxp(n), dp0(n);
    int rc = pfd_cfg_ddim_step(de.p, 2, dx.p, dn.p, dc.p, dxp.p, dp0.p, dxin.p, 2, B, C, h, w, nullptr);
    auto gxp = dxp.get(), gp0 = dp0.get();
    auto gxin = dxin.get();
    std::vector<double> rxp(n), rp0(n), rxin(2 * n);
    for (int b = 0; b < B; ++b) for (int c = 0; c < C; ++c) for (int y = 0; y < h; ++y) for (int xx = 0; xx < w; ++xx) {
      const size_t i = (((size_t)b * C + c) * h + y) * w + xx, ei = (((size_t)b * h + y) * w + xx) * C + c;
      const double eu = (double)eps[ei], ec = (double)eps[n + ei], e = eu + 2.0 * (ec - eu);
      const double p0 = (x[i] - sqrt(1 - 0.45) * e) / sqrt(0.45);
      const double xp = sqrt(0.52) * p0 + sqrt(1 - 0.52 - 0.01) * e + 0.1 * nz[i];
      rxp[i] = xp; rp0[i] = p0; rxin[ei] = xp; rxin[n + ei] = xp;
    }
    report(std::string("cfg_ddim x_prev rc=") + std::to_string(rc), gxp, rxp, 2e-5, 2e-5);
    report("cfg_ddim pred_x0", gp0, rp0, 2e-5, 2e-5);
    report("cfg_ddim xin_next", gxin, rxin, 3e-3, 2e-3);
  }
  {  // seeded noise (Philox4x32-10 + Box-Muller, include/pfd_hip.h) alone and inside the cfg + ddim step; host reference = the specification in fp64
    auto philox = [](uint32_t c[4], uint32_t k0, uint32_t k1) {
      for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = 0xD2511F53ull * c[0], p1 = 0xCD9E8D57ull * c[2];
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
        c[0] = n0; c[1] = (uint32_t)p1; c[2] = n2; c[3] = (uint32_t)p0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
      }
    };
    auto normal = [&](int64_t seed, int64_t sid, int step, long e) {
      uint32_t c[4] = {(uint32_t)(e >> 2), (uint32_t)step, (uint32_t)((uint64_t)sid & 0xffffffffu), 0u};
      philox(c, (uint32_t)((uint64_t)seed & 0xffffffffu), (uint32_t)((uint64_t)seed >> 32));
      const int j = (int)(e & 3);
      const double u = ((c[j & 2] >> 8) + 1) * ldexp(1.0, -24), v = (c[(j & 2) + 1] >> 8) * ldexp(1.0, -24);
      const double rad = sqrt(-2.0 * log(u)), ang = 2.0 * 3.14159265358979323846 * v;
      return rad * ((j & 1) ? sin(ang) : cos(ang));
    };
    uint32_t kat[4] = {0x243f6a88u, 0x85a308d3u, 0x13198a2eu, 0x03707344u};
    philox(kat, 0xa4093822u, 0x299f31d0u);
    ++g_total;
    if (!(kat[0] == 0xd16cfe09u && kat[1] == 0x94fdccebu && kat[2] == 0x5001e420u && kat[3] == 0x24126ea1u)) {
      ++g_fail;
      printf("FAIL %-58s %08x %08x %08x %08x\n", "philox4x32_10 host reference, known answer", kat[0], kat[1], kat[2], kat[3]);
    }
    std::vector<int64_t> key = {-1, 3, (1ll << 40) + 12345, 7};
    Dev<int64_t> dk(key);
    for (long ns : {7l, 4100l}) {
      Dev<float> dz((size_t)2 * ns);
      int rc = pfd_philox_normal_f32(dk.p, 49, dz.p, 2, ns, nullptr);
      auto got = dz.get();
      std::vector<double> ref(got.size());
      for (int b = 0; b < 2; ++b) for (long e = 0; e < ns; ++e) ref[b * ns + e] = normal(key[2 * b], key[2 * b + 1], 49, e);
      report(std::string("philox_normal n=") + std::to_string(ns) + " rc=" + std::to_string(rc), got, ref, 1e-5, 0);
    }
    for (int w : {6, 8}) {   // scalar path, 16-byte path
      const int B = 2, C = 4, h = 5;
      const long ns = (long)C * h * w;
      const size_t n = (size_t)B * ns;
      auto eps = rand_h(2 * n, 1.5f);
      auto x = rand_f(n, 2.f);
      std::vector<float> coef = {0.45f, 0.52f, 0.1f, sqrtf(1 - 0.45f), 2.0f};
      Dev<h16> de(eps), dxin(2 * n);
      Dev<float> dx(x), dc(coef), dxp(n), dp0(n);
      int rc = pfd_cfg_ddim_step_rng(de.p, 2, dx.p, dk.p, 7, 0.5f, dc.p, dxp.p, dp0.p, dxin.p, 2, B, C, h, w, nullptr);
      const int rc_null = pfd_cfg_ddim_step_rng(de.p, 2, dx.p, nullptr, 7, 0.5f, dc.p, dxp.p, dp0.p, dxin.p, 2, B, C, h, w, nullptr);
      auto gxp = dxp.get(), gp0 = dp0.get();
      auto gxin = dxin.get();
      std::vector<double> rxp(n), rp0(n), rxin(2 * n);
      for (int b = 0; b < B; ++b) for (int c = 0; c < C; ++c) for (int y = 0; y < h; ++y) for (int xx = 0; xx < w; ++xx) {
        const long el = ((long)c * h + y) * w + xx;
        const size_t i = (size_t)b * ns + el, ei = (((size_t)b * h + y) * w + xx) * C + c;
        const double eu = (double)eps[ei], ec = (double)eps[n + ei], e = eu + 2.0 * (ec - eu);
        const double p0 = (x[i] - sqrt(1 - 0.45) * e) / sqrt(0.45);
        const double xp = sqrt(0.52) * p0 + sqrt(1 - 0.52 - 0.01) * e + 0.1 * 0.5 * normal(key[2 * b], key[2 * b + 1], 7, el);
        rxp[i] = xp; rp0[i] = p0; rxin[ei] = xp; rxin[n + ei] = xp;
      }
      const std::string tag = std::string("cfg_ddim_rng w=") + std::to_string(w);
      ++g_total;
      if (rc_null != PFD_EINVAL) { ++g_fail; printf("FAIL %-58s rc=%d\n", (tag + " key=NULL").c_str(), rc_null); }
      report(tag + " x_prev rc=" + std::to_string(rc), gxp, rxp, 2e-5, 2e-5);
      report(tag + " pred_x0", gp0, rp0, 2e-5, 2e-5);
      report(tag + " xin_next", gxin, rxin, 3e-3, 2e-3);
    }
  }
  {  // add, add_rowvec
    const long n = 1003;
    auto a = rand_h(n + 5), b = rand_h(n + 5);
    Dev<h16> da(a), db(b), dy(n + 5);
    int rc = pfd_add_f16(da.p, db.p, dy.p, n, nullptr);
    auto got = dy.get();
    std::vector<double> ref(n + 5, 0.0);
    for (long i = 0; i < n; ++i) ref[i] = (double)a[i] + (double)b[i];
    report(std::string("add_f16 rc=") + std::to_string(rc), got, ref, 1e-3, 1e-3);
    Dev<h16> dxy(n + 5);
    rc = pfd_axpby_f16(da.p, 0.7f, db.p, -1.25f, dxy.p, n, nullptr);
    auto gxy = dxy.get();
    for (long i = 0; i < n; ++i) ref[i] = 0.7 * (double)a[i] - 1.25 * (double)b[i];
    report(std::string("axpby_f16 rc=") + std::to_string(rc), gxy, ref, 1e-3, 1e-3);
    rc = pfd_axpby_f16(da.p, 0.3f, nullptr, 0.f, dxy.p, n, nullptr);
    gxy = dxy.get();
    for (long i = 0; i < n; ++i) ref[i] = 0.3 * (double)a[i];
    report(std::string("axpby_f16 (b = NULL) rc=") + std::to_string(rc), gxy, ref, 1e-3, 1e-3);
    const int R = 37, C = 96;
    auto x = rand_h((size_t)R * C), v = rand_h(C);
    Dev<h16> dx(x), dv(v), dz((size_t)R * C);
    rc = pfd_add_rowvec_f16(dx.p, C, dv.p, dz.p, C, R, C, nullptr);
    auto gz = dz.get();
    std::vector<double> rz(gz.size());
    for (int r = 0; r < R; ++r) for (int c = 0; c < C; ++c) rz[r * C + c] = (double)x[r * C + c] + (double)v[c];
    report(std::string("add_rowvec rc=") + std::to_string(rc), gz, rz, 1e-3, 1e-3);
  }
}

// ------------------------------------------------------------------ uint8 picture ingest (image.hip)
// Pillow's tap table of one axis, restated in doubles (the product builds it in lib/image_io.py)
struct ImgTaps {
  std::vector<int32_t> xmin, klen, kk;
  int ktaps = 0;
};
static ImgTaps image_taps(int in, int out) {
  auto cubic = [](double t) {
    const double a = -0.5;
    t = fabs(t);
    if (t < 1.0) return ((a + 2.0) * t - (a + 3.0)) * t * t + 1;
    if (t < 2.0) return (((t - 5) * t + 8) * t - 4) * a;
    return 0.0;
  };
  const double scale = (double)in / out, fs = scale > 1.0 ? scale : 1.0, support = 2.0 * fs, ss = 1.0 / fs;
  ImgTaps t;
  std::vector<std::vector<int32_t>> rows(out);
  for (int xx = 0; xx < out; ++xx) {
    const double center = (xx + 0.5) * scale;
    const int x0 = std::max((int)(center - support + 0.5), 0), x1 = std::min((int)(center + support + 0.5), in);
    std::vector<double> k(x1 - x0);
    double ww = 0;
    for (int x = 0; x < x1 - x0; ++x) ww += k[x] = cubic((x + x0 - center + 0.5) * ss);
    for (double& v : k) {
      if (ww != 0.0) v /= ww;
      rows[xx].push_back(v < 0 ? (int)(-0.5 + v * (1 << PFD_IMG_PRECISION_BITS)) : (int)(0.5 + v * (1 << PFD_IMG_PRECISION_BITS)));
    }
    t.xmin.push_back(x0);
    t.klen.push_back(x1 - x0);
    t.ktaps = std::max(t.ktaps, x1 - x0);
  }
  t.kk.assign((size_t)out * t.ktaps, 0);
  for (int xx = 0; xx < out; ++xx) std::copy(rows[xx].begin(), rows[xx].end(), t.kk.begin() + (size_t)xx * t.ktaps);
  return t;
}

static void report_bytes(const std::string& name, size_t bad, size_t n) {
  ++g_total;
  if (bad) ++g_fail;
  printf("%s %-58s %zu of %zu values differ\n", bad ? "FAIL" : "ok  ", name.c_str(), bad, n);
  fflush(stdout);
}

// one case per pass against a scalar host loop (int32 sums, arithmetic shift, clamp), then ToTensor of the result: exact
static void run_image_case(int B, int H, int W, int C, int Ho, int Wo) {
  std::vector<uint8_t> src((size_t)B * H * W * C);
  for (size_t i = 0; i < src.size(); ++i) src[i] = (i / 7 + i / 31) % 5 == 0 ? (i & 1 ? 255 : 0) : (uint8_t)((i * 2654435761u) >> 13);
  auto clamp8 = [](int v) { return (uint8_t)std::min(std::max(v, 0), 255); };
  const ImgTaps th = image_taps(W, Wo), tv = image_taps(H, Ho);
  std::vector<uint8_t> mid((size_t)B * H * Wo * C), ref((size_t)B * Ho * Wo * C);
  for (int b = 0; b < B; ++b) for (int y = 0; y < H; ++y) for (int x = 0; x < Wo; ++x) for (int c = 0; c < C; ++c) {
    int acc = 1 << (PFD_IMG_PRECISION_BITS - 1);
    for (int t = 0; t < th.klen[x]; ++t) acc += (int)src[(((size_t)b * H + y) * W + th.xmin[x] + t) * C + c] * th.kk[(size_t)x * th.ktaps + t];
    mid[(((size_t)b * H + y) * Wo + x) * C + c] = clamp8(acc >> PFD_IMG_PRECISION_BITS);
  }
  for (int b = 0; b < B; ++b) for (int y = 0; y < Ho; ++y) for (int x = 0; x < Wo; ++x) for (int c = 0; c < C; ++c) {
    int acc = 1 << (PFD_IMG_PRECISION_BITS - 1);
    for (int t = 0; t < tv.klen[y]; ++t) acc += (int)mid[(((size_t)b * H + tv.xmin[y] + t) * Wo + x) * C + c] * tv.kk[(size_t)y * tv.ktaps + t];
    ref[(((size_t)b * Ho + y) * Wo + x) * C + c] = clamp8(acc >> PFD_IMG_PRECISION_BITS);
  }
  Dev<uint8_t> dsrc(src), dmid(mid.size()), du8(ref.size());
  Dev<int32_t> hk(th.kk), hx(th.xmin), hl(th.klen), vk(tv.kk), vx(tv.xmin), vl(tv.klen);
  Dev<float> df32(ref.size());
  Dev<h16> df16(ref.size());
  char tag[96];
  snprintf(tag, sizeof(tag), "%dx%dx%dx%d -> %dx%d", B, H, W, C, Ho, Wo);
  int rc = pfd_image_resample_h_u8(dsrc.p, dmid.p, B, H, W, Wo, C, hk.p, hx.p, hl.p, th.ktaps, nullptr);
  auto gmid = dmid.get();
  size_t bad = 0;
  for (size_t i = 0; i < mid.size(); ++i) bad += gmid[i] != mid[i];
  report_bytes(std::string("image horizontal pass ") + tag + " rc=" + std::to_string(rc), bad + (rc != 0), mid.size());
  rc = pfd_image_resample_v_u8(dmid.p, du8.p, PFD_IMG_U8, B, H, Ho, Wo, C, vk.p, vx.p, vl.p, tv.ktaps, nullptr);
  auto gu8 = du8.get();
  bad = 0;
  for (size_t i = 0; i < ref.size(); ++i) bad += gu8[i] != ref[i];
  report_bytes(std::string("image vertical pass ") + tag + " rc=" + std::to_string(rc), bad + (rc != 0), ref.size());
  rc = pfd_image_resample_v_u8(dmid.p, df32.p, PFD_IMG_NCHW_F32, B, H, Ho, Wo, C, vk.p, vx.p, vl.p, tv.ktaps, nullptr);
  rc |= pfd_image_resample_v_u8(du8.p, df16.p, PFD_IMG_NCHW_F16, B, Ho, Ho, Wo, C, nullptr, nullptr, nullptr, 0, nullptr);   // ToTensor alone
  auto g32 = df32.get();
  auto g16 = df16.get();
  bad = 0;
  for (int b = 0; b < B; ++b) for (int c = 0; c < C; ++c) for (int y = 0; y < Ho; ++y) for (int x = 0; x < Wo; ++x) {
    const float want = (float)ref[(((size_t)b * Ho + y) * Wo + x) * C + c] / 255.0f;
    const h16 want16 = (h16)want;
    const size_t i = (((size_t)b * C + c) * Ho + y) * Wo + x;
    bad += memcmp(&g32[i], &want, 4) != 0;
    bad += memcmp(&g16[i], &want16, 2) != 0;
  }
  report_bytes(std::string("image ToTensor f32 (fused) / f16 (alone) ") + tag + " rc=" + std::to_string(rc), bad + (rc != 0), 2 * ref.size());
}

static void run_image() {
  run_image_case(2, 37, 53, 3, 64, 96);     // enlarging: 4 taps, odd row pitch (byte heads and tails), 4-pixel vertical form
  run_image_case(1, 200, 333, 3, 50, 70);   // shrinking by 4 and 4.8, 1-pixel vertical form (70 % 4 != 0)
  run_image_case(1, 300, 300, 1, 20, 20);   // one channel, ratio 15
  const int rc = pfd_image_resample_check(1, 1025, 64, 64, 64, 3);
  report_bytes("image resample bounds: ratio above 16 is PFD_ESHAPE rc=" + std::to_string(rc), rc != PFD_ESHAPE, 1);
}

// ------------------------------------------------------------------ bench
static float time_ms(const std::function<void()>& f, int iters) {
  hipEvent_t a, b;
  HIP_OK(hipEventCreate(&a)); HIP_OK(hipEventCreate(&b));
  for (int i = 0; i < 3; ++i) f();
  HIP_OK(hipEventRecord(a, 0));
  for (int i = 0; i < iters; ++i) f();
  HIP_OK(hipEventRecord(b, 0));
  HIP_OK(hipEventSynchronize(b));
  float ms = 0;
  HIP_OK(hipEventElapsedTime(&ms, a, b));
  return ms / iters;
}

static void bench_gemm(const char* label, int M, int N, int K, int ksize, int B, int H, int Cin, int tile) {
  const bool conv = ksize > 0;
  if (conv) { M = B * H * H; K = ksize * ksize * Cin; }
  auto A = rand_h(conv ? (size_t)B * H * H * Cin : (size_t)M * K), W = rand_h((size_t)N * K, 0.05f), bias = rand_h(N);
  Dev<h16> dA(A), dW(W), dB(bias), dC((size_t)M * N);
  Dev<float> dWS((size_t)16 << 20);
  PfdGemmDesc d;
  memset(&d, 0, sizeof(d));
  d.ws = dWS.p; d.ws_bytes = (size_t)64 << 20;
  d.A = dA.p; d.W = dW.p; d.bias = dB.p; d.C = dC.p;
  d.lda = conv ? Cin : K; d.ldw = K; d.ldc = N; d.M = M; d.N = N; d.K = K; d.rows_per_rv = 1;
  d.ksize = ksize; d.stride = 1; d.pad = ksize / 2; d.B = B; d.H = H; d.Wd = H; d.Cin = Cin; d.Ho = H; d.Wo = H;
  int rc = 0;
  const float ms = time_ms([&] { rc |= pfd_gemm_f16_ex(&d, tile, nullptr); }, 20);
  const double tf = 2.0 * M * N * K / (ms * 1e-3) / 1e12;
  printf("bench %-34s M%-6d N%-5d K%-6d tile%-2d rc=%d %8.3f ms %8.1f TFLOP/s\n", label, M, N, K, tile, rc, ms, tf);
  fflush(stdout);
}

static void bench_gn_conv(const char* label, int B, int H, int C1, int C2, int N) {
  const int C = C1 + C2, HW = H * H, M = B * HW, K = 9 * C, G = 32;
  auto x1 = rand_h((size_t)M * C1), x2 = rand_h((size_t)M * std::max(C2, 8)), gm = rand_h(C), bt = rand_h(C);
  auto Wt = rand_h((size_t)N * K, 0.05f), bias = rand_h(N);
  Dev<h16> d1(x1), d2(x2), dg(gm), db(bt), dy((size_t)M * C), dW(Wt), dB(bias), dC((size_t)M * N);
  Dev<float> dT((size_t)B * C * 2);
  const size_t wsb = pfd_groupnorm_ws_bytes(B, C, HW);
  Dev<char> dws(wsb);
  PfdGemmDesc d;
  memset(&d, 0, sizeof(d));
  d.W = dW.p; d.bias = dB.p; d.C = dC.p; d.ldw = K; d.ldc = N; d.M = M; d.N = N; d.K = K; d.rows_per_rv = 1;
  d.ksize = 3; d.stride = 1; d.pad = 1; d.B = B; d.H = H; d.Wd = H; d.Cin = C; d.Ho = H; d.Wo = H;
  int rc = 0;
  d.A = dy.p; d.lda = C;
  const float gn = time_ms([&] {
    rc |= pfd_groupnorm_f16(d1.p, C1, C1, C2 ? d2.p : nullptr, C2, C2, dg.p, db.p, dy.p, C, B, HW, G, 1e-5f, PFD_ACT_SILU,
                            dws.p, wsb, nullptr); }, 20);
  const float conv = time_ms([&] { rc |= pfd_gemm_f16(&d, nullptr); }, 20);
  const float two = time_ms([&] {
    rc |= pfd_groupnorm_f16(d1.p, C1, C1, C2 ? d2.p : nullptr, C2, C2, dg.p, db.p, dy.p, C, B, HW, G, 1e-5f, PFD_ACT_SILU,
                            dws.p, wsb, nullptr);
    rc |= pfd_gemm_f16(&d, nullptr); }, 20);
  d.A = d1.p; d.lda = C1; d.A2 = C2 ? d2.p : nullptr; d.lda2 = C2; d.gn_c1 = C1; d.gn_table = dT.p; d.gn_act = PFD_ACT_SILU;
  const float tab = time_ms([&] {
    rc |= pfd_groupnorm_table_f16(d1.p, C1, C1, C2 ? d2.p : nullptr, C2, C2, dg.p, db.p, dT.p, B, HW, G, 1e-5f, dws.p, wsb,
                                  nullptr); }, 20);
  const float pconv = time_ms([&] { rc |= pfd_gemm_f16(&d, nullptr); }, 20);
  const float fused = time_ms([&] {
    rc |= pfd_groupnorm_table_f16(d1.p, C1, C1, C2 ? d2.p : nullptr, C2, C2, dg.p, db.p, dT.p, B, HW, G, 1e-5f, dws.p, wsb,
                                  nullptr);
    rc |= pfd_gemm_f16(&d, nullptr); }, 20);
  printf("bench gn+conv %-30s rc=%d  groupnorm %.1f + conv %.1f = %.1f us | table %.1f + prologue conv %.1f = %.1f us\n",
         label, rc, gn * 1e3, conv * 1e3, two * 1e3, tab * 1e3, pconv * 1e3, fused * 1e3);
}

static void bench_attn(const char* label, int B, int H, int Nq, int Nk, int D) {
  const int C = H * D, Nkp = (Nk + 7) / 8 * 8;
  auto Q = rand_h((size_t)B * Nq * C), K = rand_h((size_t)B * Nk * C), Vt = rand_h((size_t)C * B * Nkp);
  Dev<h16> dQ(Q), dK(K), dV(Vt), dO((size_t)B * Nq * C);
  PfdAttnDesc d;
  memset(&d, 0, sizeof(d));
  d.Q = dQ.p; d.K = dK.p; d.Vt = dV.p; d.O = dO.p;
  d.ldq = C; d.ldk = C; d.ldvt = (long)B * Nkp; d.ldo = C;
  d.q_bs = (long)Nq * C; d.k_bs = (long)Nk * C; d.vt_bs = Nkp; d.o_bs = (long)Nq * C;
  d.B = B; d.H = H; d.Nq = Nq; d.Nk = Nk; d.D = D; d.scale = 1.f / sqrtf((float)D);
  int rc = 0;
  const float ms = time_ms([&] { rc |= pfd_attention_f16(&d, nullptr); }, 20);
  const double tf = 4.0 * B * H * (double)Nq * Nk * D / (ms * 1e-3) / 1e12;
  printf("bench %-34s B%d H%d Nq%d Nk%d D%d rc=%d %8.3f ms %8.1f TFLOP/s\n", label, B, H, Nq, Nk, D, rc, ms, tf);
  fflush(stdout);
}

static void bench_gn(const char* label, int B, int HW, int C) {
  auto x = rand_h((size_t)B * HW * C), g = rand_h(C), bt = rand_h(C);
  Dev<h16> dx(x), dg(g), db(bt), dy((size_t)B * HW * C);
  const size_t wsb = pfd_groupnorm_ws_bytes(B, C, HW);
  Dev<char> dws(wsb);
  int rc = 0;
  const float ms = time_ms([&] { rc |= pfd_groupnorm_f16(dx.p, C, C, nullptr, 0, 0, dg.p, db.p, dy.p, C, B, HW, 32, 1e-5f, PFD_ACT_SILU, dws.p, wsb, nullptr); }, 20);
  const double gbs = 6.0 * B * HW * C / (ms * 1e-3) / 1e9;
  printf("bench %-34s B%d HW%d C%d rc=%d %8.3f ms %8.1f GB/s (6 B/elem)\n", label, B, HW, C, rc, ms, gbs);
  fflush(stdout);
}

static void bench_ln(const char* label, int M, int C) {
  auto x = rand_h((size_t)M * C), g = rand_h(C), b = rand_h(C);
  Dev<h16> dx(x), dg(g), db(b), dy((size_t)M * C);
  int rc = 0;
  const float ms = time_ms([&] { rc |= pfd_layernorm_f16(dx.p, C, dg.p, db.p, dy.p, C, M, C, 1e-5f, 0, 0, 0, 0, nullptr); }, 20);
  printf("bench %-34s M%d C%d rc=%d %8.3f ms %8.1f GB/s (4 B/elem)\n", label, M, C, rc, ms, 4.0 * M * C / (ms * 1e-3) / 1e9);
  fflush(stdout);
}

// ------------------------------------------------------------------------------------------------
// --winograd: Winograd F(2x2, 3x3) PROTOTYPE (selftest only; nothing here is linked into libpfd_hip.so).
// the one exact-in-real-arithmetic lever on the 3x3 convolutions (2.25x fewer MACs).  Built the
// way a product version would have to start: input transform V = B^T d B (4x4 tiles with stride 2, zero padding; one
// pass, fp32 math, fp16 out), 16 GEMMs M_k = V_k U_k^T on the library's own wide-tile kernels (U = G g G^T transformed in
// fp64 on the host and rounded to fp16), inverse transform Y = A^T M A (+ bias) -- measured against the patch kernel on
// the same operands, with the error of both against an fp64 direct convolution at a shape the CPU can check.
// ------------------------------------------------------------------------------------------------
typedef _Float16 h16x8 __attribute__((ext_vector_type(8)));

// x [B,H,W,C] f16 -> V [16][T][C] f16, T = B * (H/2) * (W/2); one thread = one tile x 8 channels
__global__ void wino_input_kernel(const h16* __restrict__ x, h16* __restrict__ V, int B, int H, int W, int C) {
  const int cv = C / 8;
  const long T = (long)B * (H / 2) * (W / 2);
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= T * cv) return;
  const long t = i / cv;
  const int c0 = (int)(i - t * cv) * 8;
  const int tw = W / 2, th = H / 2;
  const int b = (int)(t / (th * tw));
  const int ty = (int)((t / tw) % th), tx = (int)(t % tw);
  float d[4][4][8];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int y = 2 * ty - 1 + r, xx = 2 * tx - 1 + q;
      h16x8 v = {0, 0, 0, 0, 0, 0, 0, 0};
      if (y >= 0 && y < H && xx >= 0 && xx < W) v = *reinterpret_cast<const h16x8*>(x + (((long)b * H + y) * W + xx) * C + c0);
#pragma unroll
      for (int e = 0; e < 8; ++e) d[r][q][e] = (float)v[e];
    }
  // B^T d B, B^T = [1 0 -1 0; 0 1 1 0; 0 -1 1 0; 0 1 0 -1]
  float tmp[4][4][8];
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      tmp[0][q][e] = d[0][q][e] - d[2][q][e];
      tmp[1][q][e] = d[1][q][e] + d[2][q][e];
      tmp[2][q][e] = d[2][q][e] - d[1][q][e];
      tmp[3][q][e] = d[1][q][e] - d[3][q][e];
    }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    h16x8 o[4];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      o[0][e] = (h16)(tmp[r][0][e] - tmp[r][2][e]);
      o[1][e] = (h16)(tmp[r][1][e] + tmp[r][2][e]);
      o[2][e] = (h16)(tmp[r][2][e] - tmp[r][1][e]);
      o[3][e] = (h16)(tmp[r][1][e] - tmp[r][3][e]);
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) *reinterpret_cast<h16x8*>(V + ((long)(r * 4 + q) * T + t) * C + c0) = o[q];
  }
}

// Mk [16][T][N] f16 -> y [B,H,W,N] f16 (+ bias); one thread = one tile x 8 channels.  A^T = [1 1 1 0; 0 1 -1 -1]
__global__ void wino_output_kernel(const h16* __restrict__ Mk, const h16* __restrict__ bias, h16* __restrict__ y, int B, int H,
                                   int W, int N) {
  const int nv = N / 8;
  const long T = (long)B * (H / 2) * (W / 2);
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= T * nv) return;
  const long t = i / nv;
  const int n0 = (int)(i - t * nv) * 8;
  const int tw = W / 2, th = H / 2;
  const int b = (int)(t / (th * tw));
  const int ty = (int)((t / tw) % th), tx = (int)(t % tw);
  float m[4][4][8];
#pragma unroll
  for (int k = 0; k < 16; ++k) {
    const h16x8 v = *reinterpret_cast<const h16x8*>(Mk + ((long)k * T + t) * N + n0);
#pragma unroll
    for (int e = 0; e < 8; ++e) m[k >> 2][k & 3][e] = (float)v[e];
  }
  const h16x8 bv = *reinterpret_cast<const h16x8*>(bias + n0);
  float tmp[2][4][8];
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      tmp[0][q][e] = m[0][q][e] + m[1][q][e] + m[2][q][e];
      tmp[1][q][e] = m[1][q][e] - m[2][q][e] - m[3][q][e];
    }
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    h16x8 o0, o1;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      o0[e] = (h16)(tmp[r][0][e] + tmp[r][1][e] + tmp[r][2][e] + (float)bv[e]);
      o1[e] = (h16)(tmp[r][1][e] - tmp[r][2][e] - tmp[r][3][e] + (float)bv[e]);
    }
    h16* row = y + (((long)b * H + 2 * ty + r) * W + 2 * tx) * N + n0;
    *reinterpret_cast<h16x8*>(row) = o0;
    *reinterpret_cast<h16x8*>(row + N) = o1;
  }
}

// one shape: times (and, if check, verifies against fp64) the direct patch-kernel convolution and the Winograd pipeline
static void winograd_case(const char* label, int B, int H, int Cin, int N, bool check) {
  const int W = H, M = B * H * W, K = 9 * Cin;
  const long T = (long)B * (H / 2) * (W / 2);
  auto x = rand_h((size_t)M * Cin), wt = rand_h((size_t)N * K, 1.7f / sqrtf((float)K)), bias = rand_h(N, 0.5f);
  // U_k[n][c] = (G g G^T)[k], G = [1 0 0; .5 .5 .5; .5 -.5 .5; 0 0 1]; direct weight layout is [N][ky][kx][Cin]
  std::vector<h16> U((size_t)16 * N * Cin);
  static const double G[4][3] = {{1, 0, 0}, {0.5, 0.5, 0.5}, {0.5, -0.5, 0.5}, {0, 0, 1}};
  for (int n = 0; n < N; ++n)
    for (int c = 0; c < Cin; ++c) {
      double g[3][3], t1[4][3];
      for (int a = 0; a < 3; ++a)
        for (int b2 = 0; b2 < 3; ++b2) g[a][b2] = (double)wt[(size_t)n * K + (a * 3 + b2) * Cin + c];
      for (int a = 0; a < 4; ++a)
        for (int b2 = 0; b2 < 3; ++b2) t1[a][b2] = G[a][0] * g[0][b2] + G[a][1] * g[1][b2] + G[a][2] * g[2][b2];
      for (int a = 0; a < 4; ++a)
        for (int b2 = 0; b2 < 4; ++b2)
          U[((size_t)(a * 4 + b2) * N + n) * Cin + c] = (h16)(t1[a][0] * G[b2][0] + t1[a][1] * G[b2][1] + t1[a][2] * G[b2][2]);
    }
  Dev<h16> dx(x), dw(wt), db(bias), dU(U), dV((size_t)16 * T * Cin), dM((size_t)16 * T * N), dy((size_t)M * N), dyw((size_t)M * N);
  Dev<float> dWS((size_t)24 << 20);
  PfdGemmDesc d;
  memset(&d, 0, sizeof(d));
  d.A = dx.p; d.W = dw.p; d.bias = db.p; d.C = dy.p; d.lda = Cin; d.ldw = K; d.ldc = N; d.M = M; d.N = N; d.K = K; d.rows_per_rv = 1;
  d.ksize = 3; d.stride = 1; d.pad = 1; d.B = B; d.H = H; d.Wd = W; d.Cin = Cin; d.Ho = H; d.Wo = W;
  d.ws = dWS.p; d.ws_bytes = (size_t)96 << 20;
  int rc = 0;
  const float t_direct = time_ms([&] { rc |= pfd_gemm_f16(&d, nullptr); }, 20) * 1e3f;
  PfdGemmDesc g;
  memset(&g, 0, sizeof(g));
  g.lda = Cin; g.ldw = Cin; g.ldc = N; g.M = (int)T; g.N = N; g.K = Cin; g.rows_per_rv = 1; g.ws = dWS.p; g.ws_bytes = (size_t)96 << 20;
  const unsigned gi = (unsigned)((T * (Cin / 8) + 255) / 256), go = (unsigned)((T * (N / 8) + 255) / 256);
  auto in_t = [&] { hipLaunchKernelGGL(wino_input_kernel, dim3(gi), dim3(256), 0, nullptr, dx.p, dV.p, B, H, W, Cin); };
  auto gemms = [&] {
    for (int k = 0; k < 16; ++k) {
      g.A = dV.p + (size_t)k * T * Cin; g.W = dU.p + (size_t)k * N * Cin; g.C = dM.p + (size_t)k * T * N;
      rc |= pfd_gemm_f16(&g, nullptr);
    }
  };
  auto out_t = [&] { hipLaunchKernelGGL(wino_output_kernel, dim3(go), dim3(256), 0, nullptr, dM.p, db.p, dyw.p, B, H, W, N); };
  const float t_in = time_ms(in_t, 20) * 1e3f, t_g = time_ms(gemms, 10) * 1e3f, t_out = time_ms(out_t, 20) * 1e3f;
  const float t_all = time_ms([&] { in_t(); gemms(); out_t(); }, 10) * 1e3f;
  // optimistic bound for a batched / fused product kernel: the same MACs and activation traffic as ONE launch (16 T rows
  // against one weight matrix: 1/16 of the weight traffic, no launch boundaries between the 16 GEMMs)
  PfdGemmDesc o = g;
  o.A = dV.p; o.W = dU.p; o.C = dM.p; o.M = (int)(16 * T);
  const float t_one = time_ms([&] { rc |= pfd_gemm_f16(&o, nullptr); }, 10) * 1e3f;
  printf("winograd %-26s M%-6d N%-5d K%-6d rc=%d | direct %7.1f us (%6.1f TF/s) | F(2x2,3x3): transform %6.1f + 16 GEMMs %7.1f "
         "+ inverse %6.1f = %7.1f us (x%.2f of direct); 16 GEMMs as one launch %7.1f us -> lower bound %7.1f us (x%.2f)\n",
         label, M, N, K, rc, t_direct, 2.0 * M * N * K / t_direct * 1e-6, t_in, t_g, t_out, t_all, t_all / t_direct, t_one,
         t_in + t_one + t_out, (t_in + t_one + t_out) / t_direct);
  // the two results must agree with each other at the shape being timed (fp16 noise)
  {
    in_t(); gemms(); out_t();
    rc |= pfd_gemm_f16(&d, nullptr);
    auto a = dy.get(), b2 = dyw.get();
    double worst = 0, rms = 0;
    for (size_t i = 0; i < a.size(); ++i) { const double e = fabs((double)a[i] - (double)b2[i]); worst = std::max(worst, e); rms += e * e; }
    printf("         winograd vs direct on the GPU: max |diff| %.3e, rms %.3e\n", worst, sqrt(rms / a.size()));
  }
  if (check) {   // fp64 direct convolution on the host
    std::vector<double> ref((size_t)M * N);
    for (int m = 0; m < M; ++m) {
      const int b = m / (H * W), oy = (m / W) % H, ox = m % W;
      for (int n = 0; n < N; ++n) {
        double sacc = (double)bias[n];
        for (int ky = 0; ky < 3; ++ky)
          for (int kx = 0; kx < 3; ++kx) {
            const int iy = oy + ky - 1, ix = ox + kx - 1;
            if (iy < 0 || iy >= H || ix < 0 || ix >= W) continue;
            const h16* ap = &x[(((size_t)b * H + iy) * W + ix) * Cin];
            const h16* wp = &wt[(size_t)n * K + (ky * 3 + kx) * Cin];
            for (int c = 0; c < Cin; ++c) sacc += (double)ap[c] * (double)wp[c];
          }
        ref[(size_t)m * N + n] = sacc;
      }
    }
    auto a = dy.get(), b2 = dyw.get();
    double ed = 0, ew = 0, rd = 0, rw = 0, rr = 0;
    for (size_t i = 0; i < ref.size(); ++i) {
      const double e1 = fabs((double)a[i] - ref[i]), e2 = fabs((double)b2[i] - ref[i]);
      ed = std::max(ed, e1); ew = std::max(ew, e2); rd += e1 * e1; rw += e2 * e2; rr += ref[i] * ref[i];
    }
    printf("         error vs fp64 direct convolution (output rms %.3f): direct max %.3e rel-L2 %.3e | winograd max %.3e rel-L2 %.3e "
           "(x%.1f)\n", sqrt(rr / ref.size()), ed, sqrt(rd / rr), ew, sqrt(rw / rr), sqrt(rw / rd));
    ++g_total;
    if (!(sqrt(rw / rr) < 1e-2)) { ++g_fail; printf("FAIL winograd prototype is not a convolution\n"); }
  }
  fflush(stdout);
}

static int winograd_main() {
  // numerics at a shape the host can check (same K structure as the UNet's 320 -> 320 convolutions)
  winograd_case("check 320->320 @16^2", 1, 16, 320, 320, true);
  winograd_case("check 1280->1280 @8^2", 1, 8, 1280, 1280, true);
  // the four dominant 3x3 shapes of a C2 UNet pass (UNet batch 8)
  winograd_case("320->320 @64^2", 8, 64, 320, 320, false);
  winograd_case("960->320 @64^2", 8, 64, 960, 320, false);
  winograd_case("640->640 @32^2", 8, 32, 640, 640, false);
  winograd_case("1280->1280 @16^2", 8, 16, 1280, 1280, false);
  printf("%d checks, %d failed\n", g_total, g_fail);
  return g_fail ? 1 : 0;
}

// Per-launch floor of the runtime: N dependent launches of a kernel with ~no work, in-stream and as one
// hipGraph -- what every one of the ~500 launches of a UNet pass pays on top of its own duration.
static void bench_launch_floor() {
  Dev<h16> a(std::vector<h16>(4096)), b(std::vector<h16>(4096)), c(4096);
  const int N = 2000;
  hipStream_t st;
  HIP_OK(hipStreamCreate(&st));
  hipEvent_t e0, e1;
  HIP_OK(hipEventCreate(&e0)); HIP_OK(hipEventCreate(&e1));
  auto run = [&] { for (int i = 0; i < N; ++i) pfd_add_f16(a.p, b.p, c.p, 4096, st); };
  run();
  HIP_OK(hipStreamSynchronize(st));
  HIP_OK(hipEventRecord(e0, st)); run(); HIP_OK(hipEventRecord(e1, st));
  HIP_OK(hipEventSynchronize(e1));
  float ms = 0;
  HIP_OK(hipEventElapsedTime(&ms, e0, e1));
  printf("bench launch floor: in-stream      %6.2f us/launch (%d dependent tiny launches)\n", ms * 1e3 / N, N);
  hipGraph_t g; hipGraphExec_t ge;
  HIP_OK(hipStreamBeginCapture(st, hipStreamCaptureModeGlobal));
  run();
  HIP_OK(hipStreamEndCapture(st, &g));
  HIP_OK(hipGraphInstantiate(&ge, g, nullptr, nullptr, 0));
  HIP_OK(hipGraphLaunch(ge, st));
  HIP_OK(hipStreamSynchronize(st));
  HIP_OK(hipEventRecord(e0, st)); HIP_OK(hipGraphLaunch(ge, st)); HIP_OK(hipEventRecord(e1, st));
  HIP_OK(hipEventSynchronize(e1));
  HIP_OK(hipEventElapsedTime(&ms, e0, e1));
  printf("bench launch floor: hipGraph replay %6.2f us/launch\n", ms * 1e3 / N);
  HIP_OK(hipGraphExecDestroy(ge)); HIP_OK(hipGraphDestroy(g)); HIP_OK(hipStreamDestroy(st));
  fflush(stdout);
}

__global__ void count_mismatch_kernel(const unsigned short* a, const unsigned short* b, size_t n, unsigned* cnt) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  unsigned bad = 0;
  for (; i < n; i += (size_t)gridDim.x * blockDim.x) bad += a[i] != b[i];
  if (bad) atomicAdd(cnt, bad);
}

// --replay <file>: relaunch a recorded GEMM/conv launch list (tools/dump_unet_shapes.py) once each, in
// order, on random operands -- the torch-free workload rocprofv3 --pmc is pointed at.
static int replay(const char* path, bool timed = false, int force_tile = 0) {
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
      PfdGemmDesc d;
      memset(&d, 0, sizeof(d));
      d.M = q[0]; d.N = q[1]; d.K = q[2]; d.act = q[3];
      d.A = dA.p; d.W = dW.p; d.C = dC.p;
      d.bias = q[4] ? dB.p : nullptr; d.rowvec = q[5] ? dRV.p : nullptr; d.R = q[6] ? dR.p : nullptr;
      d.bias_per_row = q[7];
      d.ksize = q[8]; d.stride = q[9]; d.pad = q[10]; d.ups = q[11];
      d.B = q[12]; d.H = q[13]; d.Wd = q[14]; d.Cin = q[15]; d.Ho = q[16]; d.Wo = q[17];
      d.rows_per_rv = (int)std::min<long>(q[18], 1 << 30);
      const long nout = d.act == PFD_ACT_GEGLU ? d.N / 2 : d.N;
      d.lda = d.ksize > 0 ? d.Cin : d.K; d.ldw = d.K; d.ldc = nout; d.ldr = nout; d.ldrv = d.N;
      d.ws = dWS.p; d.ws_bytes = (size_t)96 << 20;
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

int main(int argc, char** argv) {
  if (argc > 2 && !strcmp(argv[1], "--replay")) return replay(argv[2]);
  if (argc > 1 && !strcmp(argv[1], "--launch-floor")) { bench_launch_floor(); return 0; }
  if (argc > 1 && !strcmp(argv[1], "--winograd")) return winograd_main();
  if (argc > 1 && !strcmp(argv[1], "--bench-patch")) {   // one 3x3 conv per image width the patch kernel serves
    bench_gemm("conv3x3 320->320 @64^2", 0, 320, 0, 3, 8, 64, 320, 0);
    bench_gemm("conv3x3 640->640 @32^2", 0, 640, 0, 3, 8, 32, 640, 0);
    bench_gemm("conv3x3 1280->1280 @16^2", 0, 1280, 0, 3, 8, 16, 1280, 0);
    bench_gemm("conv3x3 320->320 @64^2 implicit GEMM", 0, 320, 0, 3, 8, 64, 320, 5400);
    return 0;
  }
  if (argc > 1 && !strcmp(argv[1], "--bench-gn-conv")) {   // GroupNorm + conv: two launches + a tensor vs table + prologue
    bench_gn_conv("320->320 @64^2", 16, 64, 320, 0, 320);
    bench_gn_conv("640->320 @64^2 (skip concat)", 16, 64, 320, 320, 320);
    bench_gn_conv("960->320 @64^2 (skip concat)", 16, 64, 640, 320, 320);
    bench_gn_conv("640->640 @32^2", 16, 32, 640, 0, 640);
    bench_gn_conv("1280->640 @32^2 (skip concat)", 16, 32, 640, 640, 640);
    bench_gn_conv("1920->640 @32^2 (skip concat)", 16, 32, 1280, 640, 640);
    return 0;
  }
  if (argc > 1 && !strcmp(argv[1], "--gemm-new")) {   // quick correctness pass over the round-3 tile variants only
    for (int v : {5100, 5300, 9200, 9300}) {
      run_gemm_case({1100, 320, 1024, 0, true, true, true, false, v});
      run_gemm_case({300, 320, 192, PFD_ACT_SILU, true, true, true, false, v});
      run_gemm_case({77, 160, 64, 0, true, false, false, false, v, 8});
      run_gemm_case({0, 160, 0, 0, true, true, false, false, v, 0, 3, 1, 1, 0, 3, 16, 16, 128});
      run_gemm_case({900, 320, 1536, 0, true, false, false, false, v + 3});
      run_gemm_case({200, 320, 128, PFD_ACT_GEGLU, true, false, false, false, v});
    }
    { GemmCase t{520, 480, 128, 0, false, false, false, false, 5100}; t.n_split = 320; run_gemm_case(t); }
    { GemmCase t{520, 480, 128, 0, false, false, false, false, 9200}; t.n_split = 320; run_gemm_case(t); }
    run_gemm_case({600, 640, 320, PFD_ACT_GEGLU, true, false, false, false, 9400});
    run_gemm_case({300, 320, 64, PFD_ACT_GEGLU, false, false, false, false, 9400});
    run_tiled_weight_cases();
    printf("SELFTEST %d/%d passed, %d failed\n", g_total - g_fail, g_total, g_fail);
    return g_fail;
  }
  if (argc > 1 && !strcmp(argv[1], "--r5")) {   // round 5: the kernels adopted this round
    // adopted: the split-K reduction that also normalises (PfdGemmDesc.gnf_y) at the shapes the UNet / ControlNet give it
    run_gnf_case(8, 16, 16, 1280, 1280, PFD_ACT_SILU, 1e-5f, false, true, false);       // ResBlock conv1 @16^2 (patch kernel, split 4)
    run_gnf_case(8, 8, 8, 1280, 1280, PFD_ACT_SILU, 1e-5f, false, true, false);         // @8^2 (ring kernel, split 4)
    run_gnf_case(8, 8, 8, 2560, 1280, PFD_ACT_SILU, 1e-5f, false, true, false);         // over the skip concat width, split 8
    run_gnf_case(8, 16, 16, 640, 1280, PFD_ACT_SILU, 1e-5f, false, true, false);        // 640 -> 1280
    run_gnf_case(8, 16, 16, 1280, 1280, PFD_ACT_NONE, 1e-6f, true, false, true);        // + residual, raw kept, no activation
    run_gnf_case(4, 8, 8, 1280, 1280, PFD_ACT_SILU, 1e-5f, true, true, true);           // UNet batch 4
    run_gnf_case(8, 16, 16, 1280, 1280, PFD_ACT_SILU, 1e-5f, false, true, false, 10802);   // forced patch kernel, split 2
    run_gnf_case(8, 8, 8, 1280, 1280, PFD_ACT_SILU, 1e-5f, false, true, false, 3308);        // forced 4-stage ring, split 8
    run_gnf_decline_case(8, 64, 64, 320, 320);                                          // 64^2: not split, cpg 10
    // round 6: the 640-channel norms of the 32^2 level (20 channels per group, 1024 x 5 chunks per slab)
    run_gnf_case(8, 32, 32, 640, 640, PFD_ACT_SILU, 1e-5f, false, true, false);         // ResBlock conv1 @32^2 (patch kernel, split 2)
    run_gnf_case(8, 32, 32, 640, 640, PFD_ACT_SILU, 1e-5f, true, false, true);          // conv2: + residual, raw kept for the skip
    run_gnf_case(8, 32, 32, 1280, 640, PFD_ACT_SILU, 1e-5f, false, true, false);        // over a skip concat width
    run_gnf_case(4, 32, 32, 320, 640, PFD_ACT_SILU, 1e-5f, false, true, false);         // first ResBlock of the level, UNet batch 4
    // residual stored once for a doubled batch (PfdGemmDesc.res_rows): every store pass and both plain reductions
    for (int v : {0, 9200, 9300, 3200, 3300, 5400, 5800}) {
      { GemmCase c{1024, 320, 256, 0, true, true, true, false, v}; c.res_rows = 512; run_gemm_case(c); }                      // plain store pass
      if (v != 5800) { GemmCase c{1024, 320, 256, 0, true, true, false, false, v}; c.res_rows = 512; c.zero_rows = 512; run_gemm_case(c); }  // + zero rows: the cross-attention re-join (not on the loader-wave kernel)
      { GemmCase c{1024, 320, 320, 0, true, true, false, false, v}; c.res_rows = 512; c.gn_out = 1; run_gemm_case(c); }       // statistics-emitting store pass: proj_out
    }
    { GemmCase c{1024, 320, 2048, 0, true, true, false, false, 3304}; c.res_rows = 512; run_gemm_case(c); }                    // split-K 4: plain reduction
    { GemmCase c{1024, 320, 2048, 0, true, true, false, false, 3304}; c.res_rows = 512; c.gn_out = 1; run_gemm_case(c); }      // ... statistics-emitting reduction
    // the statistics-emitting split-K reduction and the GroupNorm apply from producer statistics
    { GemmCase c{512, 1280, 2048, 0, true, true, true, false, 3304}; c.gn_out = 1; run_gemm_case(c); }                          // split-K 4, cpg 40
    { GemmCase c{0, 320, 0, 0, true, true, true, false, 9302, 0, 3, 1, 1, 0, 2, 16, 16, 128}; c.gn_out = 1; run_gemm_case(c); }   // conv, split-K 2
    run_gn_case(8, 64, 1280, 0, 32, PFD_ACT_SILU, 1e-5f);
    run_gn_case(8, 256, 1280, 1280, 32, PFD_ACT_SILU, 1e-5f);
    run_gn_pstats_case(8, 4096, 320, 0, PFD_ACT_SILU, 1e-5f);
    run_gn_pstats_case(8, 4096, 320, 320, PFD_ACT_SILU, 1e-5f);
    run_gn_pstats_case(3, 1024, 640, 0, PFD_ACT_NONE, 1e-6f);
    run_gn_pstats_case(2, 256, 1280, 1280, PFD_ACT_SILU, 1e-5f);
    printf("SELFTEST %d/%d passed, %d failed\n", g_total - g_fail, g_total, g_fail);
    return g_fail;
  }
  if (argc > 1 && !strcmp(argv[1], "--ups-fold")) {   // upsample convolution as four 2x2-tap phase convolutions (PfdGemmDesc.ups = 2)
    run_ups_fold_cases();
    if (argc > 2 && !strcmp(argv[2], "full")) {       // the two large upsample convolutions of a C2 UNet pass against fp64 (a minute of host time)
      { GemmCase c{0, 640, 0, 0, true, false, false, false, 0, 0, 3, 1, 1, 2, 8, 32, 32, 640}; c.gn_out = 1; run_gemm_case(c); }
      { GemmCase c{0, 1280, 0, 0, true, false, false, false, 0, 0, 3, 1, 1, 2, 8, 16, 16, 1280}; c.gn_out = 1; run_gemm_case(c); }
    }
    printf("SELFTEST %d/%d passed, %d failed\n", g_total - g_fail, g_total, g_fail);
    return g_fail;
  }
  if (argc > 1 && !strcmp(argv[1], "--patch-wide")) {   // 3x3 patch kernels on 48- / 96-wide images (2-D output tiles)
    for (int v : {0, 10800, 10900}) {
      run_gemm_case({0, 160, 0, PFD_ACT_SILU, true, true, true, false, v, 0, 3, 1, 1, 0, 1, 16, 48, 128});   // 16 x 16 tiles
      run_gemm_case({0, 320, 0, 0, true, true, true, false, v, 0, 3, 1, 1, 0, 2, 8, 96, 64});                 // 8 x 32 tiles
      run_gemm_case({0, 160, 0, 0, true, false, true, false, v, 0, 3, 1, 1, 0, 1, 32, 96, 128});              // 4 x 3 tiles
      run_gemm_case({0, 160, 0, 0, true, true, false, false, v, 0, 3, 1, 1, 0, 3, 32, 48, 64});               // several samples
    }
    run_gemm_case({0, 160, 0, 0, true, true, true, false, 10802, 0, 3, 1, 1, 0, 1, 16, 96, 256});             // split over channel blocks
    { GemmCase c{0, 320, 0, 0, true, true, true, false, 0, 0, 3, 1, 1, 0, 2, 16, 96, 128}; c.w_tiled = 1; run_gemm_case(c); }
    run_gemm_case({0, 160, 0, 0, true, true, false, false, 5400, 0, 3, 1, 1, 0, 1, 16, 48, 128});             // same shape, implicit GEMM
    printf("SELFTEST %d/%d passed, %d failed\n", g_total - g_fail, g_total, g_fail);
    return g_fail;
  }
  if (argc > 1 && !strcmp(argv[1], "--narrow")) {   // conv3x3_narrow_kernel: cases + the two shapes of the pipeline
    run_narrow_conv_cases();
    bench_gemm("unet head conv 320->4 @64^2 B8", 8 * 4096, 4, 2880, 3, 8, 64, 320, 0);
    bench_gemm("unet head conv 320->4 @96^2 B4", 4 * 9216, 4, 2880, 3, 4, 96, 320, 0);
    bench_gemm("vae conv_out 128->3 @512^2 B4", 4 * 262144, 3, 1152, 3, 4, 512, 128, 0);
    bench_gemm("unet head conv, round-5 kernel", 8 * 4096, 4, 2880, 3, 8, 64, 320, 11);
    bench_gemm("vae conv_out, round-5 kernel", 4 * 262144, 3, 1152, 3, 4, 512, 128, 21);
    printf("SELFTEST %d/%d passed, %d failed\n", g_total - g_fail, g_total, g_fail);
    return g_fail;
  }
  if (argc > 1 && !strcmp(argv[1], "--image")) {   // the uint8 picture ingest only
    run_image();
    printf("SELFTEST %d/%d passed, %d failed\n", g_total - g_fail, g_total, g_fail);
    return g_fail;
  }
  if (argc > 1 && !strcmp(argv[1], "--elementwise")) {   // boundary / elementwise kernels only (the seeded noise among them)
    run_elementwise();
    printf("SELFTEST %d/%d passed, %d failed\n", g_total - g_fail, g_total, g_fail);
    return g_fail;
  }
  if (argc > 1 && !strcmp(argv[1], "--ln")) {
    run_ln_fold_suite();
    printf("SELFTEST %d/%d passed, %d failed\n", g_total - g_fail, g_total, g_fail);
    return g_fail;
  }
  if (argc > 1 && !strcmp(argv[1], "--attn")) {   // attention correctness cases only (seconds; run once per PFD_ATTN mode)
    run_attn_case(2, 2, 128, 128, 40, true);
    run_attn_case(1, 2, 300, 148, 40, false);
    run_attn_case(2, 2, 512, 256, 40, true);
    run_attn_case(1, 1, 256, 40, 40, false);
    run_attn_case(1, 2, 520, 1000, 40, false);
    run_attn_case(1, 2, 77, 64, 40, true);
    run_attn_case(1, 2, 200, 148, 40, false);
    run_attn_case(2, 2, 64, 64, 80, true);
    run_attn_case(1, 2, 144, 256, 96, false);
    run_attn_case(1, 3, 148, 148, 96, false);
    run_attn_case(2, 2, 64, 148, 160, false);
    run_attn_case(1, 1, 256, 320, 160, true);
    run_attn_case(1, 2, 520, 1000, 40, false, 700);   // maximum jumps at key 700 (tile 10 of 16)
    run_attn_case(2, 2, 512, 256, 40, true, 130);
    run_attn_case(1, 2, 300, 148, 40, false, 140);    // ... inside the ragged tile
    run_attn_case(1, 2, 512, 1024, 40, true, 700);    // round 6: whole 64-key tiles (attention3_kernel when PFD_ATTN3_FORCE=1 or the grid is big)
    run_attn_case(1, 1, 700, 640, 40, false, 333);    // ragged last query block
    run_attn_case(8, 8, 1024, 1024, 40, true, 500);   // 256 blocks: attention3_kernel by the dispatcher's own rule
    printf("SELFTEST %d/%d passed, %d failed\n", g_total - g_fail, g_total, g_fail);
    return g_fail;
  }
  if (argc > 1 && !strcmp(argv[1], "--attn512")) {   // VAE mid-block attention (d = 512, one head): cases + bench
    run_attn_case(2, 1, 256, 256, 512, false);
    run_attn_case(1, 1, 200, 96, 512, false);          // ragged query tile, 3 key tiles
    run_attn_case(1, 1, 128, 32, 512, false);          // a single key tile
    run_attn_case(2, 1, 128, 512, 512, true);          // Q / K as column slices of one matrix
    run_attn_case(1, 1, 128, 512, 512, false, 300);    // the maximum jumps in the middle of the stream
    bench_attn("vae mid attention 64^2 d512", 4, 1, 4096, 4096, 512);
    bench_attn("vae mid attention 96^2 d512", 2, 1, 9216, 9216, 512);
    printf("%d checks, %d failed\n", g_total, g_fail);
    return g_fail ? 1 : 0;
  }
  if (argc > 1 && !strcmp(argv[1], "--bench-attn")) {
    bench_attn("self-attn 64^2 d40", 8, 8, 4096, 4096, 40);
    bench_attn("self-attn 64^2 d40 (CFG prefix)", 4, 8, 4096, 4096, 40);
    bench_attn("self-attn 96^2 d40 (C5)", 4, 8, 9216, 9216, 40);
    bench_attn("self-attn 32^2 d80", 8, 8, 1024, 1024, 80);
    bench_attn("self-attn 16^2 d160", 8, 8, 256, 256, 160);
    bench_attn("cross-attn 64^2 d40", 4, 8, 4096, 148, 40);
    bench_attn("seecoder cross d96", 1, 8, 144, 4096, 96);
    // fixed cost of the short launches: the same problems with fewer keys
    bench_attn("cross-attn 64^2 d40, 64 keys", 4, 8, 4096, 64, 40);
    bench_attn("cross-attn 64^2 d40, 8 keys", 4, 8, 4096, 8, 40);
    bench_attn("cross-attn 32^2 d80", 4, 8, 1024, 148, 80);
    bench_attn("cross-attn 32^2 d80, 8 keys", 4, 8, 1024, 8, 80);
    bench_attn("cross-attn 16^2 d160", 4, 8, 256, 148, 160);
    bench_attn("cross-attn 16^2 d160, 8 keys", 4, 8, 256, 8, 160);
    bench_attn("self-attn 16^2 d160, 64 keys", 8, 8, 256, 64, 160);
    return 0;
  }
  if (argc > 1 && !strcmp(argv[1], "--bench-gn")) {
    bench_gn("groupnorm+silu 320 @64^2", 8, 4096, 320);
    bench_gn("groupnorm+silu 640 @64^2", 8, 4096, 640);
    bench_gn("groupnorm+silu 640 @32^2", 8, 1024, 640);
    bench_gn("groupnorm+silu 1280 @32^2", 8, 1024, 1280);
    bench_gn("groupnorm+silu 1280 @16^2", 8, 256, 1280);
    bench_gn("groupnorm+silu 2560 @16^2", 8, 256, 2560);
    bench_gn("groupnorm+silu 1280 @8^2", 8, 64, 1280);
    bench_gn("groupnorm+silu 128 @512^2", 4, 262144, 128);
    bench_ln("layernorm 320 @64^2", 32768, 320);
    bench_ln("layernorm 640 @32^2", 8192, 640);
    bench_ln("layernorm 1280 @16^2", 2048, 1280);
    return 0;
  }
  if (argc > 2 && !strcmp(argv[1], "--replay-time")) return replay(argv[2], true, argc > 3 ? atoi(argv[3]) : 0);
  const bool bench = argc > 1 && !strcmp(argv[1], "--bench");
  const bool only_bench = argc > 1 && !strcmp(argv[1], "--only-bench");
  hipDeviceProp_t prop;
  HIP_OK(hipGetDeviceProperties(&prop, 0));
  printf("device: %s  CUs=%d  abi=%d\n", prop.name, prop.multiProcessorCount, pfd_abi_version());

  if (!only_bench) {
    const int tiles[] = {22, 21, 12, 11};
    for (int t : tiles) {
      run_gemm_case({256, 256, 128, 0, true, false, false, false, t});
      run_gemm_case({301, 203 - 3, 192, PFD_ACT_GELU, true, true, true, false, t});
      run_gemm_case({77, 72, 64, PFD_ACT_SILU, true, true, false, true, t, 8});
    }
    run_gemm_case({130, 4, 128, 0, true, true, false, false, 0});          // N = 4 (UNet head)
    run_gemm_case({64, 37, 64, PFD_ACT_RELU, false, false, false, false, 0});  // odd N -> scalar stores
    run_gemm_case({200, 256, 128, PFD_ACT_GEGLU, true, true, false, false, 0});
    run_gemm_case({512, 1280, 320, 0, true, false, true, false, 0});
    for (int t : tiles) {
      GemmCase c{0, 96, 0, 0, true, true, true, false, t, 0, 3, 1, 1, 0, 2, 9, 7, 64};
      run_gemm_case(c);
    }
    run_gemm_case({0, 128, 0, PFD_ACT_SILU, true, false, false, false, 0, 0, 3, 2, 1, 0, 2, 10, 8, 64});  // stride 2
    run_gemm_case({0, 64, 0, 0, true, true, false, false, 0, 0, 3, 1, 1, 1, 1, 5, 6, 128});             // upsample
    run_gemm_case({0, 64, 0, 0, true, false, false, false, 0, 8, 3, 2, 0, 0, 1, 9, 9, 64});             // pad 0, stride 2, ld+8
    run_gemm_case({0, 80, 0, 0, true, false, false, false, 0, 0, 1, 1, 0, 0, 2, 6, 6, 128});            // 1x1 as conv

    // wide-tile LDS-DMA kernel (N % 160 == 0): variants 256x160 / 128x160 / 64x160, split-K, conv gather
    for (int v : {0, 5400, 3400, 3200}) {
      run_gemm_case({300, 320, 192, PFD_ACT_SILU, true, true, true, false, v});
      run_gemm_case({77, 160, 64, 0, true, false, false, false, v, 8});
      GemmCase c{0, 320, 0, 0, true, true, true, false, v, 0, 3, 1, 1, 0, 2, 9, 7, 64};
      run_gemm_case(c);
    }
    // patch conv kernel: W in {16,32,64}, whole image rows per tile, halo zero padding, split over channel blocks
    run_gemm_case({0, 160, 0, PFD_ACT_SILU, true, true, true, false, 10900, 0, 3, 1, 1, 0, 2, 16, 16, 64});
    run_gemm_case({0, 320, 0, 0, true, true, false, false, 10900, 0, 3, 1, 1, 0, 1, 32, 32, 128});
    run_gemm_case({0, 160, 0, 0, true, false, true, false, 10902, 0, 3, 1, 1, 0, 1, 64, 64, 128});
    run_gemm_case({0, 320, 0, 0, true, false, false, false, 0, 0, 3, 1, 1, 0, 3, 16, 16, 192});
    run_gemm_case({520, 160, 1024, PFD_ACT_GELU, true, true, true, false, 3204});   // 64x160 tiles, split-K 4
    run_gemm_case({130, 320, 2048, 0, true, true, false, false, 5403});             // 256x160, split-K 3
    run_gemm_case({200, 320, 128, PFD_ACT_GEGLU, true, false, false, false, 0});     // GEGLU, 40-row packing
    // 128-wide tiles of the wide kernel (N % 128 == 0, N % 160 != 0: VAE / Swin / SeeCoder widths)
    run_gemm_case({300, 256, 192, PFD_ACT_SILU, true, true, true, false, 5400});
    run_gemm_case({77, 128, 64, 0, true, false, false, false, 3400, 8});
    run_gemm_case({130, 384, 320, PFD_ACT_GELU, true, true, false, false, 3200});
    run_gemm_case({520, 256, 2048, 0, true, true, false, false, 3404});
    run_gemm_case({0, 256, 0, PFD_ACT_SILU, true, true, true, false, 0, 0, 3, 1, 1, 0, 2, 9, 7, 128});
    run_gemm_case({0, 128, 0, 0, true, false, false, false, 5400, 0, 3, 1, 1, 1, 1, 5, 6, 128});   // upsample
    run_gemm_case({0, 512, 0, 0, true, false, false, false, 0, 0, 3, 2, 0, 0, 1, 9, 9, 64});       // stride 2, pad 0
    {
      GemmCase t{200, 384, 128, 0, true, false, false, false, 0}; t.n_split = 256; run_gemm_case(t);
    }
    // transposed tail (fused q|k|v projection): all three tile heights, ragged M, bias
    {
      GemmCase t{520, 480, 128, 0, false, false, false, false, 0}; t.n_split = 320; run_gemm_case(t);
      GemmCase u{301, 320, 192, 0, true, false, false, false, 5400}; u.n_split = 160; run_gemm_case(u);
      GemmCase v{77, 960, 320, 0, false, false, false, false, 3400}; v.n_split = 640; run_gemm_case(v);
      GemmCase w{130, 480, 64, 0, true, false, false, false, 3200}; w.n_split = 320; run_gemm_case(w);
    }
    // deep operand rings (counted vmcnt + raw barrier): K shorter than, equal to and longer than the ring, split-K, conv
    run_gemm_case({130, 320, 128, 0, true, true, false, false, 3300});
    run_gemm_case({300, 160, 256, PFD_ACT_GELU, true, true, true, false, 3500});
    run_gemm_case({300, 320, 1024, 0, true, true, true, false, 3300});
    run_gemm_case({77, 160, 1344, 0, true, false, false, false, 3500});
    run_gemm_case({520, 320, 2048, 0, true, true, false, false, 3304});
    run_gemm_case({130, 160, 1536, 0, true, false, false, false, 3503});
    run_gemm_case({0, 320, 0, 0, true, true, false, false, 3302, 0, 3, 1, 1, 0, 2, 8, 8, 256});
    run_gemm_case({0, 160, 0, PFD_ACT_SILU, true, false, true, false, 3500, 0, 3, 2, 1, 0, 2, 10, 8, 128});
    // wave-specialised forms: 256-row tile with loader waves (48), patch kernel with loader waves (98) / without (99)
    run_gemm_case({300, 320, 1024, 0, true, true, true, false, 5800});
    run_gemm_case({0, 320, 0, 0, true, true, false, false, 5800, 0, 3, 1, 1, 0, 2, 8, 8, 256});
    run_gemm_case({0, 160, 0, PFD_ACT_SILU, true, false, true, false, 5800, 0, 3, 2, 1, 0, 2, 10, 8, 128});
    run_gemm_case({0, 320, 0, 0, true, true, false, false, 10800, 0, 3, 1, 1, 0, 1, 32, 32, 128});
    run_gemm_case({0, 160, 0, 0, true, false, true, false, 10802, 0, 3, 1, 1, 0, 1, 64, 64, 128});
    // round 3: rotated K walk (several M tiles, K tiles >= M tiles and < M tiles, split-K, conv wrap-around) and the
    // loader-wave kernels (5800 / 5700 = 256-row tile, 10800 / 10600 = patch kernel with two / three weight stages)
    for (int v : {5800, 5700}) {   // 58 = two operand stages, 57 = the 3-stage ring (the default)
      run_gemm_case({1100, 320, 1024, 0, true, true, true, false, v});
      run_gemm_case({700, 640, 192, PFD_ACT_GELU, true, false, true, false, v});
      run_gemm_case({600, 320, 2048, 0, true, true, false, false, v + 2});                       // split-K 2
      run_gemm_case({0, 320, 0, 0, true, true, false, false, v, 0, 3, 1, 1, 0, 3, 16, 16, 128});   // conv, 3 M tiles
      run_gemm_case({0, 160, 0, PFD_ACT_SILU, true, false, true, false, v, 0, 3, 2, 1, 0, 5, 20, 16, 64});  // stride 2
      run_gemm_case({0, 160, 0, 0, true, false, false, false, v, 0, 3, 1, 1, 1, 2, 9, 12, 64});   // upsample
      run_gemm_case({600, 256, 512, 0, true, true, false, false, v});                            // 128-wide tiles
    }
    for (int v : {10800, 10600}) {
      run_gemm_case({0, 320, 0, 0, true, true, true, false, v, 0, 3, 1, 1, 0, 2, 32, 32, 128});
      run_gemm_case({0, 160, 0, PFD_ACT_SILU, true, false, true, false, v, 0, 3, 1, 1, 0, 1, 64, 64, 256});
      run_gemm_case({0, 320, 0, 0, true, true, false, false, v, 0, 3, 1, 1, 0, 3, 16, 16, 320});
      run_gemm_case({0, 160, 0, 0, true, false, false, false, v + 2, 0, 3, 1, 1, 0, 2, 16, 16, 512});  // split over cb
    }
    run_gemm_case({600, 640, 320, PFD_ACT_GEGLU, true, false, false, false, 9400});   // 256 x 320 GEGLU tile
    run_gemm_case({300, 320, 64, PFD_ACT_GEGLU, false, false, false, false, 9400});
    for (int v : {3200, 3300, 3400, 3500, 5400, 5100, 5300, 9200, 9300}) {   // rotated walk over several M tiles; 8-wave small tiles
      run_gemm_case({1100, 320, 1024, 0, true, true, true, false, v});
      run_gemm_case({0, 160, 0, 0, true, true, false, false, v, 0, 3, 1, 1, 0, 3, 16, 16, 128});
      run_gemm_case({900, 320, 1536, 0, true, false, false, false, v + 3});
    }
    // GroupNorm(+SiLU) prologue of the patch kernel == pfd_groupnorm_f16 followed by the plain convolution, bit for bit
    run_gn_conv_case(2, 16, 16, 64, 0, 160, PFD_ACT_SILU, false);
    run_gn_conv_case(1, 32, 32, 128, 64, 320, PFD_ACT_SILU, true);
    run_gn_conv_case(2, 64, 64, 64, 128, 160, PFD_ACT_NONE, true);
    run_gn_conv_case(3, 32, 32, 320, 0, 320, PFD_ACT_SILU, true);
    run_gemm_case({0, 160, 0, PFD_ACT_SILU, true, false, false, false, 0, 0, 3, 2, 1, 0, 2, 10, 8, 128});  // stride 2
    run_gemm_case({0, 160, 0, 0, true, true, false, false, 3402, 0, 3, 1, 1, 1, 1, 5, 6, 128});           // upsample + split
    run_gemm_case({0, 320, 0, 0, true, false, false, false, 0, 8, 3, 2, 0, 0, 1, 9, 9, 64});               // pad 0, ld+8
    run_gemm_case({0, 160, 0, 0, true, false, false, false, 0, 0, 1, 1, 0, 0, 2, 6, 6, 128});              // 1x1 as conv
    run_ups_fold_cases();
    run_narrow_conv_cases();

    run_gemm_case({0, 160, 0, PFD_ACT_SILU, true, true, true, false, 0, 0, 3, 1, 1, 0, 1, 16, 48, 128});   // patch kernel, 2-D tiles
    run_gemm_case({0, 320, 0, 0, true, true, true, false, 0, 0, 3, 1, 1, 0, 2, 8, 96, 64});
    run_ln_fold_suite();
    run_attn_case(2, 2, 128, 128, 40, true);
    run_attn_case(1, 2, 300, 148, 40, false);    // ragged queries and keys (2 full tiles + 20 keys)
    run_attn_case(2, 2, 512, 256, 40, true);     // full tiles only
    run_attn_case(1, 1, 256, 40, 40, false);     // a single ragged tile
    run_attn_case(1, 2, 520, 1000, 40, false);   // 15 full tiles + 40 keys
    run_attn_case(1, 2, 77, 64, 40, true);       // exactly one full tile
    run_attn_case(1, 2, 200, 148, 40, false);
    run_attn_case(2, 2, 64, 64, 80, true);
    run_attn_case(1, 2, 144, 256, 96, false);
    run_attn_case(1, 3, 148, 148, 96, false);
    run_attn_case(2, 2, 64, 148, 160, false);
    run_attn_case(1, 1, 256, 320, 160, true);
    run_attn_case(2, 1, 256, 256, 512, false);   // VAE mid-block attention (attention512_kernel)
    run_attn_case(1, 1, 200, 96, 512, false);

    run_swin_case(1, 14, 17, 2, 0);
    run_swin_case(1, 14, 17, 2, 6);
    run_swin_case(2, 24, 24, 1, 6);
    run_swin_case(1, 8, 8, 3, 6);

    run_gn_case(2, 64, 320, 0, 32, PFD_ACT_SILU, 1e-5f);
    run_gn_case(2, 100, 64, 32, 32, PFD_ACT_NONE, 1e-6f);   // groups straddle the concat seam
    run_gn_case(1, 50, 1280, 1280, 32, PFD_ACT_SILU, 1e-5f);  // two vec slots per thread
    run_gn_case(2, 1024, 128, 0, 32, PFD_ACT_SILU, 1e-6f);
    run_gn_case(1, 16, 1920, 0, 32, PFD_ACT_SILU, 1e-5f);
    // single-launch small-slab form ((C/G) % 4 == 0, slab <= 32 K elements, >= 128 blocks)
    run_gn_case(4, 64, 1280, 0, 32, PFD_ACT_SILU, 1e-5f);
    run_gn_case(4, 256, 1280, 1280, 32, PFD_ACT_SILU, 1e-5f);
    run_gn_case(8, 128, 1024, 0, 32, PFD_ACT_NONE, 1e-6f);
    run_gn_case(4, 100, 1280, 640, 32, PFD_ACT_SILU, 1e-5f);   // cpg 60: groups straddle the seam

    run_ln_case(37, 320, 0, 0, 0, 0);
    run_ln_case(10, 1280, 0, 0, 0, 0);
    run_ln_case(5, 3072, 0, 0, 0, 0);
    run_ln_case(2 * 4 * 3, 4 * 96, 1, 2, 7, 5);
    run_ln_case(8195, 320, 0, 0, 0, 0);    // multi-row form (M >= 8192), ragged last wave
    run_ln_case(8192, 640, 0, 0, 0, 0);
    run_ln_case(8193, 1280, 0, 0, 0, 0);
    run_softmax_case(5, 4096, 0.044f);
    run_softmax_case(3, 1152, 0.1f);
    run_softmax_case(2, 36864, 0.044f);   // long-row form (N > 16384)
    run_softmax_case(2, 16392, 0.05f);
    run_elementwise();
    run_image();
    printf("SELFTEST %d/%d passed, %d failed\n", g_total - g_fail, g_total, g_fail);
  }

  if (bench || only_bench) {
    // UNet-shaped problems at C2 (UNet batch 8)
    for (int t : {5400, 10900, 5400, 10900}) {   // gather conv vs patch conv
      bench_gemm("PATCH conv3x3 320->320 @64^2", 0, 320, 0, 3, 8, 64, 320, t);
      bench_gemm("PATCH conv3x3 960->320 @64^2", 0, 320, 0, 3, 8, 64, 960, t);
      bench_gemm("PATCH conv3x3 640->640 @32^2", 0, 640, 0, 3, 8, 32, 640, t == 5400 ? 5402 : t);
      bench_gemm("PATCH conv3x3 1280->1280 @16^2", 0, 1280, 0, 3, 8, 16, 1280, t == 5400 ? 3404 : t);
    }
    for (int rep = 0; rep < 1; ++rep)
      for (int t : {5400, 3400}) {
        bench_gemm("conv3x3 320->320 @64^2", 0, 320, 0, 3, 8, 64, 320, t);
        bench_gemm("linear qkv 320->960 @64^2", 32768, 960, 320, 0, 0, 0, 0, t);
        bench_gemm("linear 1280->320 @64^2", 32768, 320, 1280, 0, 0, 0, 0, t);
        bench_gemm("conv3x3 640->640 @32^2", 0, 640, 0, 3, 8, 32, 640, t);
      }
    for (int t : {5400, 5402, 5403, 3402, 0}) bench_gemm("conv3x3 640->640 @32^2", 0, 640, 0, 3, 8, 32, 640, t);
    for (int t : {5400, 5402, 0}) bench_gemm("conv3x3 1920->640 @32^2", 0, 640, 0, 3, 8, 32, 1920, t);
    for (int t : {3400, 3200, 3402, 3404, 3202, 0}) bench_gemm("conv3x3 1280->1280 @16^2", 0, 1280, 0, 3, 8, 16, 1280, t);
    for (int t : {3200, 3204, 3208, 3404, 3408, 0}) bench_gemm("conv3x3 1280->1280 @8^2", 0, 1280, 0, 3, 8, 8, 1280, t);
    for (int t : {5400, 3400, 0}) bench_gemm("linear qkv 320->960 @64^2", 32768, 960, 320, 0, 0, 0, 0, t);
    for (int t : {5400, 3400, 0}) bench_gemm("linear 1280->320 @64^2", 32768, 320, 1280, 0, 0, 0, 0, t);
    for (int t : {5400, 3400, 0}) bench_gemm("linear 320->2560 @64^2", 32768, 2560, 320, 0, 0, 0, 0, t);
    for (int t : {5400, 3400, 3200, 0}) bench_gemm("linear 1280->10240 @16^2", 2048, 10240, 1280, 0, 0, 0, 0, t);
    bench_gemm("square-ish 8192x5120x4096", 8192, 5120, 4096, 0, 0, 0, 0, 5400);
    for (int t : {22, 21}) {
      bench_gemm("conv3x3 640->640 @32^2", 0, 640, 0, 3, 8, 32, 640, t);
      bench_gemm("conv3x3 1280->1280 @16^2", 0, 1280, 0, 3, 8, 16, 1280, t);
    }
    for (int t : {22, 21, 12, 11}) bench_gemm("conv3x3 1280->1280 @8^2", 0, 1280, 0, 3, 8, 8, 1280, t);
    bench_gemm("conv3x3 2560->1280 @16^2", 0, 1280, 0, 3, 8, 16, 2560, 0);
    bench_gemm("conv3x3 960->320 @64^2", 0, 320, 0, 3, 8, 64, 960, 0);
    bench_gemm("linear qk 320->640 @64^2", 32768, 640, 320, 0, 0, 0, 0, 0);
    bench_gemm("linear geglu-in 320->2560", 32768, 2560, 320, 0, 0, 0, 0, 0);
    bench_gemm("linear ff-out 1280->320", 32768, 320, 1280, 0, 0, 0, 0, 0);
    bench_gemm("linear 640->5120 @32^2", 8192, 5120, 640, 0, 0, 0, 0, 0);
    bench_gemm("linear 1280->10240 @16^2", 2048, 10240, 1280, 0, 0, 0, 0, 0);
    bench_gemm("vae conv3x3 128->128 @512^2 (B1)", 0, 128, 0, 3, 1, 512, 128, 0);
    bench_gemm("vae conv3x3 512->512 @64^2 (B4)", 0, 512, 0, 3, 4, 64, 512, 0);
    bench_gemm("square 4096^3", 4096, 4096, 4096, 0, 0, 0, 0, 22);
    bench_attn("self-attn 64^2 d40", 8, 8, 4096, 4096, 40);
    bench_attn("self-attn 32^2 d80", 8, 8, 1024, 1024, 80);
    bench_attn("self-attn 16^2 d160", 8, 8, 256, 256, 160);
    bench_attn("cross-attn 64^2 d40", 8, 8, 4096, 148, 40);
    bench_attn("seecoder cross d96", 1, 8, 144, 4096, 96);
    bench_gn("groupnorm+silu 320 @64^2", 8, 4096, 320);
    bench_gn("groupnorm+silu 1280 @16^2", 8, 256, 1280);
    bench_gn("groupnorm+silu 128 @512^2", 4, 262144, 128);
  }
  return g_fail;
}
