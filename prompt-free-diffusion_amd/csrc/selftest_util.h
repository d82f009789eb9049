// What the three selftest sources share: HIP error check, the one random stream, device buffers, the pass / fail counters
// and reporters, descriptor helpers, and the few entry points that cross files.  Test infrastructure only.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <atomic>
#include <random>
#include <string>
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

// every operand of every mode is drawn from this one stream: a case's inputs depend on all draws before it
inline std::mt19937 rng(1234);
inline int g_fail = 0, g_total = 0;

inline std::vector<h16> rand_h(size_t n, float scale = 1.f) {
  std::uniform_real_distribution<float> d(-1.f, 1.f);
  std::vector<h16> v(n);
  for (auto& x : v) x = (h16)(d(rng) * scale);
  return v;
}
inline std::vector<float> rand_f(size_t n, float scale = 1.f) {
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
  ~Dev() { if (p) (void)hipFree(p); }
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
void report(const std::string& name, const std::vector<T>& got, const std::vector<double>& ref, double atol, double rtol) {
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

// a library call answered rc != 0 before anything could be compared: the case is counted here, once, as failed
inline void fail_rc(const char* name, int rc) {
  ++g_total; ++g_fail;
  printf("FAIL %-58s rc=%d (%s)\n", name, rc, pfd_last_error());
}

inline double act_ref(double v, int act) {
  switch (act) {
    case PFD_ACT_GELU: return 0.5 * v * (1.0 + erf(v / sqrt(2.0)));
    case PFD_ACT_RELU: return v > 0 ? v : 0;
    case PFD_ACT_SILU: return v / (1.0 + exp(-v));
    default: return v;
  }
}

// the host references are plain fp64 loops: rows are independent, so they run on host threads and the result does not
// depend on how many.  OMP_NUM_THREADS when set and positive (a shared machine reports far more CPUs than a command may use),
// else at most 16
template <class F>
void parallel_rows(int M, F&& body) {
  const char* env = getenv("OMP_NUM_THREADS");
  const unsigned nt = env && atoi(env) > 0 ? (unsigned)atoi(env) : std::min(std::max(1u, std::thread::hardware_concurrency()), 16u);
  if (M < 64 || nt == 1) { for (int m = 0; m < M; ++m) body(m); return; }
  std::vector<std::thread> th;
  std::atomic<int> next{0};
  for (unsigned t = 0; t < nt; ++t)
    th.emplace_back([&]() { for (int m; (m = next.fetch_add(8)) < M;) for (int i = m; i < std::min(M, m + 8); ++i) body(i); });
  for (auto& t : th) t.join();
}

// an all-zero descriptor with the whole of `ws` as its workspace
inline PfdGemmDesc gemm_desc(const Dev<float>& ws) {
  PfdGemmDesc d;
  memset(&d, 0, sizeof(d));
  d.ws = ws.p; d.ws_bytes = ws.n * sizeof(float);
  return d;
}
// geometry of a 3x3 / stride 1 / pad 1 convolution over a [B, H, W, Cin] image (the output has the same H x W)
inline void conv3x3_geometry(PfdGemmDesc& d, int B, int H, int W, int Cin) {
  d.ksize = 3; d.stride = 1; d.pad = 1; d.B = B; d.H = H; d.Wd = W; d.Cin = Cin; d.Ho = H; d.Wo = W;
}

// selftest_bench.cpp: the two timers the correctness modes use, and the bench modes
void bench_gemm(const char* label, int M, int N, int K, int ksize, int B, int H, int Cin, int tile);
void bench_attn(const char* label, int B, int H, int Nq, int Nk, int D);
int bench_unet_list(int, char**);
int bench_patch(int, char**);
int bench_gn_conv_list(int, char**);
int bench_attn_list(int, char**);
int bench_gn_list(int, char**);
int bench_launch_floor(int, char**);
// selftest_boundary.cpp
int bench_boundary(int, char**);
// selftest_replay.cpp
int replay(const char* path, bool timed, int force_tile);
