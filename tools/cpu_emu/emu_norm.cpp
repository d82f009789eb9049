// CPU emulation of csrc/norm.hip (test infrastructure; see hip/hip_runtime.h in this directory for the execution model): the
// single-launch small-slab GroupNorm and the GroupNorm apply from producer statistics (eight slabs' partials / eight rows in
// flight) against a double-precision GroupNorm.  --forms: the two-launch form with both vector slots and with constant groups,
// the table kernel and the plain-loop apply from producer statistics.  --dispatch FILE: a dry run of the three entry points.
#include <stdio.h>

#include <random>
#include <string>

#include "hip/hip_runtime.h"


#include "pfd_common.h"
bool pfd_prof_on() { return false; }
void pfd_prof_begin(int, double, double, hipStream_t) {}
void pfd_prof_end(hipStream_t) {}
int pfd_check_launch(const char*) { return 0; }
void pfd_set_error(const char*) {}

#include "norm_emu.inc"

typedef _Float16 h16;
static std::mt19937 rng(5);
static std::vector<h16> rand_h(size_t n, float scale, float off = 0.f) {
  std::uniform_real_distribution<float> d(-1.f, 1.f);
  std::vector<h16> v(n);
  for (auto& x : v) x = (h16)(d(rng) * scale + off);
  return v;
}
static int g_fail = 0, g_total = 0;

static void check(const char* name, const std::vector<h16>& got, const std::vector<double>& ref, const std::vector<h16>* same, const char* same_what) {
  double me = 0, mr = 0;
  for (size_t i = 0; i < got.size(); ++i) { me = std::max(me, fabs((double)got[i] - ref[i])); mr = std::max(mr, fabs(ref[i])); }
  bool ok = me <= 6e-3 * std::max(1.0, mr);
  std::string extra;
  if (same) {
    size_t nd = 0;
    for (size_t i = 0; i < got.size(); ++i) nd += memcmp(&got[i], &(*same)[i], sizeof(h16)) != 0;
    if (nd) { ok = false; extra = std::string(" | ") + same_what + ": " + std::to_string(nd) + " elements differ"; }
    else extra = std::string(" | == ") + same_what + " bitwise";
  }
  ++g_total;
  g_fail += !ok;
  printf("%s %-64s max err %.2e (max |ref| %.2f)%s\n", ok ? "ok  " : "FAIL", name, me, mr, extra.c_str());
  fflush(stdout);
}

static std::vector<double> gn_ref(const std::vector<h16>& x1, const std::vector<h16>& x2, const std::vector<h16>& gm, const std::vector<h16>& bt,
                                  int B, int HW, int C1, int C2, int G, float eps, int act) {
  const int C = C1 + C2, cpg = C / G;
  std::vector<double> ref((size_t)B * HW * C);
  auto at = [&](int b, int r, int c) { return c < C1 ? (double)x1[((size_t)b * HW + r) * C1 + c] : (double)x2[((size_t)b * HW + r) * C2 + c - C1]; };
  for (int b = 0; b < B; ++b)
    for (int g = 0; g < G; ++g) {
      double a = 0, q = 0;
      for (int r = 0; r < HW; ++r)
        for (int c = g * cpg; c < (g + 1) * cpg; ++c) { const double v = at(b, r, c); a += v; q += v * v; }
      const double n = (double)HW * cpg, mean = a / n, rstd = 1.0 / sqrt(std::max(q / n - mean * mean, 0.0) + eps);
      for (int r = 0; r < HW; ++r)
        for (int c = g * cpg; c < (g + 1) * cpg; ++c) {
          double v = (at(b, r, c) - mean) * rstd * (double)gm[c] + (double)bt[c];
          if (act == PFD_ACT_SILU) v = v / (1.0 + exp(-v));
          ref[((size_t)b * HW + r) * C + c] = v;
        }
    }
  return ref;
}

// pfd_groupnorm_f16 (small-slab single launch where the shape qualifies) against double precision
static void small_case(int B, int HW, int C1, int C2, int act) {
  const int C = C1 + C2, G = 32;
  auto x1 = rand_h((size_t)B * HW * C1, 2.f, 0.7f), x2 = rand_h((size_t)B * HW * std::max(C2, 8), 1.f), gm = rand_h(C, 1.f), bt = rand_h(C, 0.5f);
  std::vector<h16> y((size_t)B * HW * C, (h16)-7.f);
  const size_t wsb = pfd_groupnorm_ws_bytes(B, C, HW);
  std::vector<char> ws(wsb);
  int rc = pfd_groupnorm_f16(x1.data(), C1, C1, C2 ? x2.data() : nullptr, C2, C2, gm.data(), bt.data(), y.data(), C, B, HW, G, 1e-5f, act, ws.data(), wsb, nullptr);
  char name[160];
  snprintf(name, sizeof(name), "groupnorm B%d HW%d C%d+%d act%d (rc %d)", B, HW, C1, C2, act, rc);
  check(name, y, gn_ref(x1, x2, gm, bt, B, HW, C1, C2, G, 1e-5f, act), nullptr, "");
}

// pfd_groupnorm_pstats_f16 (statistics in the producers' layout, computed on the host here; grouped partial loads where a
// group is at most two producer groups per source) against double precision
static void pstats_case(int B, int HW, int C1, int C2, int act) {
  const int C = C1 + C2, G = 32;
  auto x1 = rand_h((size_t)B * HW * C1, 1.5f, 0.3f), x2 = rand_h((size_t)B * HW * std::max(C2, 8), 1.f), gm = rand_h(C, 1.f), bt = rand_h(C, 0.5f);
  auto mk = [&](const std::vector<h16>& x, int Cs) {
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
  auto s1 = mk(x1, C1);
  std::vector<float> s2 = C2 ? mk(x2, C2) : std::vector<float>(2, 0.f);
  std::vector<h16> y((size_t)B * HW * C, (h16)-7.f);
  char name[160];
  if (!pfd_groupnorm_takes_pstats(B, C1, C2, HW, G)) { ++g_total; ++g_fail; printf("FAIL pstats B%d HW%d C%d+%d: shape refused\n", B, HW, C1, C2); return; }
  int rc = pfd_groupnorm_pstats_f16(x1.data(), C1, C1, s1.data(), C2 ? x2.data() : nullptr, C2, C2, C2 ? s2.data() : nullptr, gm.data(), bt.data(), y.data(), C, B, HW, G, 1e-5f, act, nullptr);
  snprintf(name, sizeof(name), "groupnorm pstats B%d HW%d C%d+%d act%d (rc %d)", B, HW, C1, C2, act, rc);
  check(name, y, gn_ref(x1, x2, gm, bt, B, HW, C1, C2, G, 1e-5f, act), nullptr, "");
}

// ---- emu_norm --forms: the forms no other CPU check runs (tests/test_norm_kernels_cpu.py) ----
// x = uniform values around an offset; const_groups: group 0 holds 3.0 (every sum exact) and group 1 fp16(2.7) (sums that round)
static std::vector<h16> forms_x(int B, int HW, int C, int G, bool const_groups) {
  auto x = rand_h((size_t)B * HW * C, 2.f, 0.7f);
  if (const_groups) {
    const int cpg = C / G;
    for (size_t r = 0; r < (size_t)B * HW; ++r)
      for (int c = 0; c < 2 * cpg; ++c) x[r * C + c] = c < cpg ? (h16)3.f : (h16)2.7f;
  }
  return x;
}

// pfd_groupnorm_f16 in the two-launch form for any G, one source, against double precision; every output finite
static void two_launch_case(const char* what, int B, int HW, int C, int G, int act, bool const_groups) {
  auto x = forms_x(B, HW, C, G, const_groups), gm = rand_h(C, 1.f), bt = rand_h(C, 0.5f);
  std::vector<h16> none, y((size_t)B * HW * C, (h16)-7.f);
  const size_t wsb = pfd_groupnorm_ws_bytes(B, C, HW);
  std::vector<char> ws(wsb);
  emu::launched.clear();
  int rc = pfd_groupnorm_f16(x.data(), C, C, nullptr, 0, 0, gm.data(), bt.data(), y.data(), C, B, HW, G, 1e-5f, act, ws.data(), wsb, nullptr);
  char name[200];
  snprintf(name, sizeof(name), "%s: groupnorm B%d HW%d C%d G%d act%d (rc %d, %s)", what, B, HW, C, G, act, rc,
           emu::launched.size() == 2 ? "two launches" : "NOT the two-launch form");
  bool finite = emu::launched.size() == 2 && rc == 0;
  for (h16 v : y) finite = finite && std::isfinite((float)v);
  if (!finite) { ++g_total; ++g_fail; printf("FAIL %s: not finite / wrong form\n", name); return; }
  check(name, y, gn_ref(x, none, gm, bt, B, HW, C, 0, G, 1e-5f, act), nullptr, "");
}

// pfd_groupnorm_table_f16 against the double-precision scale = rstd gamma, shift = beta - mean scale
static void table_case(int B, int HW, int C, int G) {
  auto x = forms_x(B, HW, C, G, false), gm = rand_h(C, 1.f), bt = rand_h(C, 0.5f);
  const size_t wsb = pfd_groupnorm_ws_bytes(B, C, HW);
  std::vector<char> ws(wsb);
  std::vector<float> table((size_t)B * 2 * C + 4, -7.f);
  float* tab = table.data() + ((16 - (reinterpret_cast<uintptr_t>(table.data()) & 15)) & 15) / 4;   // 16-byte aligned
  int rc = pfd_groupnorm_table_f16(x.data(), C, C, nullptr, 0, 0, gm.data(), bt.data(), tab, B, HW, G, 1e-5f, ws.data(), wsb, nullptr);
  const int cpg = C / G;
  double me = 0, mr = 0;
  for (int b = 0; b < B; ++b)
    for (int g = 0; g < G; ++g) {
      double a = 0, q = 0;
      for (int r = 0; r < HW; ++r)
        for (int c = g * cpg; c < (g + 1) * cpg; ++c) { const double v = (double)x[((size_t)b * HW + r) * C + c]; a += v; q += v * v; }
      const double n = (double)HW * cpg, mean = a / n, rstd = 1.0 / sqrt(std::max(q / n - mean * mean, 0.0) + 1e-5);
      for (int c = g * cpg; c < (g + 1) * cpg; ++c) {
        const double sc = rstd * (double)gm[c], sh = (double)bt[c] - mean * sc;
        me = std::max({me, fabs(tab[(size_t)b * 2 * C + c] - sc), fabs(tab[(size_t)b * 2 * C + C + c] - sh)});
        mr = std::max({mr, fabs(sc), fabs(sh)});
      }
    }
  const bool ok = rc == 0 && me <= 1e-5 * std::max(1.0, mr);
  ++g_total;
  g_fail += !ok;
  printf("%s groupnorm table B%d HW%d C%d G%d (rc %d)   max err %.2e (max |scale|, |shift| %.2f)\n", ok ? "ok  " : "FAIL", B, HW, C, G, rc, me, mr);
  fflush(stdout);
}

// pfd_groupnorm_pstats_f16 with G != 32 (a group spans more than two producer groups: the plain loop of the fold)
static void pstats_plain_case(int B, int HW, int C1, int G, int act) {
  auto x1 = rand_h((size_t)B * HW * C1, 1.5f, 0.3f), gm = rand_h(C1, 1.f), bt = rand_h(C1, 0.5f);
  const int cpp = C1 / 32, tn = C1 / 160;
  std::vector<float> st((size_t)(B * HW / 64) * tn * 32, NAN);   // the slots no producer writes stay NaN
  for (int sl = 0; sl < B * HW / 64; ++sl)
    for (int pg = 0; pg < 32; ++pg) {
      double a = 0, q = 0;
      for (int r = 0; r < 64; ++r)
        for (int c = pg * cpp; c < (pg + 1) * cpp; ++c) { const double v = (double)x1[(size_t)(sl * 64 + r) * C1 + c]; a += v; q += v * v; }
      const int c0 = pg * cpp;
      const size_t o = (((size_t)sl * tn + c0 / 160) * 16 + (c0 % 160) / cpp) * 2;
      st[o] = (float)a; st[o + 1] = (float)q;
    }
  std::vector<h16> none, y((size_t)B * HW * C1, (h16)-7.f);
  emu::launched.clear();
  int rc = pfd_groupnorm_pstats_f16(x1.data(), C1, C1, st.data(), nullptr, 0, 0, nullptr, gm.data(), bt.data(), y.data(), C1, B, HW, G, 1e-5f, act, nullptr);
  const std::string kern = emu::launched.empty() ? "nothing" : emu::launched[0];
  char name[200];
  snprintf(name, sizeof(name), "groupnorm pstats B%d HW%d C%d G%d act%d (rc %d, %s)", B, HW, C1, G, act, rc, kern.c_str());
  bool finite = rc == 0 && kern == "gn_apply_pstats_kernel<false>";
  for (h16 v : y) finite = finite && std::isfinite((float)v);
  if (!finite) { ++g_total; ++g_fail; printf("FAIL %s: not finite / not the plain loop\n", name); return; }
  check(name, y, gn_ref(x1, none, gm, bt, B, HW, C1, 0, G, 1e-5f, act), nullptr, "");
}

// ---- emu_norm --dispatch FILE: a dry run (emu::dry_run: launches are recorded, nothing executes, no pointer is dereferenced) of
// the three GroupNorm entry points.  One request per line of FILE: "<id> gn|pstats|table B HW C1 C2 G"; one line out per request:
// the request, "-> <return value>", then per launch the instantiated kernel, grid x x y and block x. ----
static int dispatch_probe(const char* path) {
  emu::dry_run = true;
  FILE* f = fopen(path, "r");
  if (!f) { fprintf(stderr, "emu_norm: cannot open %s\n", path); return 2; }
  auto fake = [](int i) { return reinterpret_cast<void*>((uintptr_t)0x10000 * (i + 1)); };   // 16-byte aligned, never dereferenced
  char line[512], id[256], api[16];
  for (int ln = 1; fgets(line, sizeof(line), f); ++ln) {
    int B, HW, C1, C2, G;
    if (sscanf(line, "%255s %15s %d %d %d %d %d", id, api, &B, &HW, &C1, &C2, &G) != 7) { fprintf(stderr, "emu_norm: %s:%d: not a request\n", path, ln); return 2; }
    emu::launch_log.clear();
    emu::launched.clear();
    const size_t wsb = pfd_groupnorm_ws_bytes(B, C1 + C2, HW);
    void* x2 = C2 ? fake(1) : nullptr;
    int rc;
    if (!strcmp(api, "gn"))
      rc = pfd_groupnorm_f16(fake(0), C1, C1, x2, C2, C2, fake(2), fake(3), fake(4), C1 + C2, B, HW, G, 1e-5f, PFD_ACT_SILU, fake(5), wsb, nullptr);
    else if (!strcmp(api, "pstats"))
      rc = pfd_groupnorm_pstats_f16(fake(0), C1, C1, fake(6), x2, C2, C2, C2 ? fake(7) : nullptr, fake(2), fake(3), fake(4), C1 + C2, B, HW, G, 1e-5f,
                                    PFD_ACT_SILU, nullptr);
    else if (!strcmp(api, "table"))
      rc = pfd_groupnorm_table_f16(fake(0), C1, C1, x2, C2, C2, fake(2), fake(3), fake(8), B, HW, G, 1e-5f, fake(5), wsb, nullptr);
    else { fprintf(stderr, "emu_norm: %s:%d: entry point %s\n", path, ln, api); return 2; }
    printf("%s %s %d %d %d %d %d -> %d", id, api, B, HW, C1, C2, G, rc);
    // (the kernel as the launch expression spells it: no launch of norm.hip sits in a template, and the C++ runtime's demangler
    //  does not read the _Float16 parameters of these kernels' linkage names)
    for (size_t i = 0; i < emu::launch_log.size(); ++i) {
      const auto& l = emu::launch_log[i];
      printf(" | %s grid %ux%u block %u", emu::launched[i].c_str(), l.grid_x, l.grid_y, l.block_x);
    }
    printf("\n");
  }
  fclose(f);
  return 0;
}

int main(int argc, char** argv) {
  if (argc > 2 && !strcmp(argv[1], "--dispatch")) return dispatch_probe(argv[2]);
  if (argc > 1 && !strcmp(argv[1], "--forms")) {
    two_launch_case("both vector slots", 1, 5, 4096, 32, PFD_ACT_SILU, false);   // chunks of 3 and 2 rows
    table_case(2, 33, 192, 24);                                                  // P = 10, two chunks
    pstats_plain_case(2, 128, 320, 8, PFD_ACT_SILU);                             // four producer groups per group
    two_launch_case("constant groups", 3, 37, 256, 32, PFD_ACT_NONE, true);
    printf("%d cases, %d failed\n", g_total, g_fail);
    return g_fail;
  }
  const bool quick = argc > 1 && !strcmp(argv[1], "--quick");   // the CPU suite's subset
  small_case(8, 64, 1280, 0, PFD_ACT_SILU);      // 8^2: 640 chunks per group slab, 3 slots per thread
  small_case(4, 64, 1280, 1280, PFD_ACT_NONE);   // skip concat, cpg 80
  small_case(4, 100, 1408, 0, PFD_ACT_SILU);     // cpg 44, cpr 11 (carries in the index walk), ragged HW
  if (!quick) {
    small_case(4, 256, 1280, 0, PFD_ACT_SILU);   // 16^2 (B x G = 128): 2560 chunks
    small_case(4, 64, 1024, 0, PFD_ACT_SILU);    // cpg 32, cpr 8: no carries
    small_case(4, 64, 1280, 640, PFD_ACT_SILU);  // cpg 60 straddles the two sources: the plain form both times
  }
  pstats_case(1, 4096, 320, 0, PFD_ACT_SILU);    // 64^2: 64 slabs, 8 per thread
  pstats_case(1, 1024, 320, 320, PFD_ACT_SILU);  // skip concat: two producer groups per group
  if (!quick) {
    pstats_case(1, 4608, 320, 0, PFD_ACT_NONE);  // 72 slabs: a second trip of the chunked fold
    pstats_case(2, 256, 640, 0, PFD_ACT_SILU);   // 4 slabs, six clamped slots
  }
  printf("%d cases, %d failed\n", g_total, g_fail);
  return g_fail;
}
