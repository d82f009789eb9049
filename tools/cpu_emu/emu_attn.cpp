// CPU emulation of csrc/attention.hip (see hip/hip_runtime.h): the fused attention kernels (8-wave d = 40 form with the PV
// product on 16x16x32 and the maximum folded into the QK^T MFMA; 4-wave form for every head dim) against a double-precision
// softmax(scale Q K^T) V.
//   usage: emu_attn [--quick] [--w4] [--kbias]     (--w4: the 4-wave d = 40 form; prints one line per case with a checksum of the output bits;
//                                                    --kbias: pfd_attention_kbias_f16, the per-key logit operand, every kernel class it has)
//          emu_attn --rbias                        (pfd_attention_rbias_f16, a logit row per region of the query: d = 40, 80, 160)
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

#include "attention_emu.inc"
#include "attention3_kernel.h"   // round 6: the software-pipelined d = 40 kernel (no inline asm: included as it is)

typedef _Float16 h16;
static std::mt19937 rng(11);
static std::vector<h16> rand_h(size_t n, float scale) {
  std::uniform_real_distribution<float> d(-1.f, 1.f);
  std::vector<h16> v(n);
  for (auto& x : v) x = (h16)(d(rng) * scale);
  return v;
}
static int g_fail = 0, g_total = 0;

static void run_case(int B, int H, int Nq, int Nk, int D, int spike = 0) {
  const int C = H * D;
  const long nkp = (Nk + 7) / 8 * 8;
  auto Q = rand_h((size_t)B * Nq * C, 1.5f), K = rand_h((size_t)B * Nk * C, 1.5f), V = rand_h((size_t)B * Nk * C, 1.f);
  if (spike > 0 && spike < Nk)   // key `spike` = 4 x query (spike % Nq): the row maximum jumps in the middle of the stream
    for (int b = 0; b < B; ++b)
      for (int c = 0; c < C; ++c) K[((size_t)b * Nk + spike) * C + c] = (h16)(4.0f * (float)Q[((size_t)b * Nq + spike % Nq) * C + c]);
  std::vector<h16> Vt((size_t)C * B * nkp, (h16)0.f), O((size_t)B * Nq * C, (h16)-9.f);
  for (int b = 0; b < B; ++b)
    for (int j = 0; j < Nk; ++j)
      for (int c = 0; c < C; ++c) Vt[(size_t)c * B * nkp + (size_t)b * nkp + j] = V[((size_t)b * Nk + j) * C + c];
  PfdAttnDesc d;
  memset(&d, 0, sizeof(d));
  d.Q = Q.data(); d.K = K.data(); d.Vt = Vt.data(); d.O = O.data();
  d.ldq = C; d.ldk = C; d.ldo = C; d.ldvt = (long)B * nkp;
  d.q_bs = (long)Nq * C; d.k_bs = (long)Nk * C; d.o_bs = (long)Nq * C; d.vt_bs = nkp;
  d.B = B; d.H = H; d.Nq = Nq; d.Nk = Nk; d.D = D;
  d.scale = 1.0f / sqrtf((float)D);
  const int rc = pfd_attention_f16(&d, nullptr);
  double me = 0, mr = 0;
  std::vector<double> s(Nk);
  for (int b = 0; b < B && rc == 0; ++b)
    for (int h = 0; h < H; ++h)
      for (int i = 0; i < Nq; ++i) {
        double mx = -1e300;
        for (int j = 0; j < Nk; ++j) {
          double a = 0;
          for (int e = 0; e < D; ++e) a += (double)Q[((size_t)b * Nq + i) * C + h * D + e] * (double)K[((size_t)b * Nk + j) * C + h * D + e];
          s[j] = a * d.scale;
          mx = std::max(mx, s[j]);
        }
        double den = 0;
        for (int j = 0; j < Nk; ++j) { s[j] = exp(s[j] - mx); den += s[j]; }
        for (int e = 0; e < D; ++e) {
          double o = 0;
          for (int j = 0; j < Nk; ++j) o += s[j] * (double)V[((size_t)b * Nk + j) * C + h * D + e];
          o /= den;
          mr = std::max(mr, fabs(o));
          me = std::max(me, fabs(o - (double)O[((size_t)b * Nq + i) * C + h * D + e]));
        }
      }
  uint64_t sum = 1469598103934665603ull;   // FNV-1a over the output bits
  for (auto& x : O) { unsigned short u; memcpy(&u, &x, 2); sum = (sum ^ u) * 1099511628211ull; }
  const bool ok = rc == 0 && me <= 4e-3 * std::max(1.0, mr);
  ++g_total;
  g_fail += !ok;
  printf("%s attention B%d H%d Nq%d Nk%d D%d  rc %d  max err %.2e (max |ref| %.2f)  bits %016llx\n", ok ? "ok  " : "FAIL", B, H, Nq, Nk, D, rc, me,
         mr, (unsigned long long)sum);
  fflush(stdout);
}

// pfd_attention_kbias_f16: per-key logits in log2 units (rows of kb_bs > Nk floats, NaN behind the keys), against the weighted
// softmax in double precision.  pattern 0: two references 0.7 / 0.3; 1: sample b keeps 1 + b % 2 halves, the rest is -inf (whole
// trailing tiles masked); 2: -inf on keys 64..127 and on every fifth key, key 0 finite, random logits in [-12, 0] elsewhere
static void run_case_kbias(int B, int H, int Nq, int Nk, int D, int pattern) {
  const int C = H * D;
  const long nkp = (Nk + 7) / 8 * 8, kb_bs = (Nk + 3) / 4 * 4 + 4;
  auto Q = rand_h((size_t)B * Nq * C, 1.5f), K = rand_h((size_t)B * Nk * C, 1.5f), V = rand_h((size_t)B * Nk * C, 1.f);
  std::vector<h16> Vt((size_t)C * B * nkp, (h16)0.f), O((size_t)B * Nq * C, (h16)-9.f);
  for (int b = 0; b < B; ++b)
    for (int j = 0; j < Nk; ++j)
      for (int c = 0; c < C; ++c) Vt[(size_t)c * B * nkp + (size_t)b * nkp + j] = V[((size_t)b * Nk + j) * C + c];
  float* kb = (float*)aligned_alloc(16, sizeof(float) * B * kb_bs);
  std::uniform_real_distribution<float> u(-12.f, 0.f);
  const int half = Nk / 2;
  for (int b = 0; b < B; ++b)
    for (long j = 0; j < kb_bs; ++j) {
      float v = NAN;
      if (j < Nk) {
        if (pattern == 0) v = j < half ? 0.f : log2f(0.3f / 0.7f);
        else if (pattern == 1) v = (j < half || (b % 2) == 1) ? 0.f : -INFINITY;
        else v = (j > 0 && ((j >= 64 && j < 128) || j % 5 == 0)) ? -INFINITY : u(rng);
      }
      kb[b * kb_bs + j] = v;
    }
  PfdAttnDesc d;
  memset(&d, 0, sizeof(d));
  d.Q = Q.data(); d.K = K.data(); d.Vt = Vt.data(); d.O = O.data();
  d.ldq = C; d.ldk = C; d.ldo = C; d.ldvt = (long)B * nkp;
  d.q_bs = (long)Nq * C; d.k_bs = (long)Nk * C; d.o_bs = (long)Nq * C; d.vt_bs = nkp;
  d.B = B; d.H = H; d.Nq = Nq; d.Nk = Nk; d.D = D;
  d.scale = 1.0f / sqrtf((float)D);
  const int rc = pfd_attention_kbias_f16(&d, kb, kb_bs, nullptr);
  // the bound of the GPU tests (tests/refmix_refs.py kbias_bound): (3 2^-11 + Nk 2^-25 + 2^-16 + 2 ln2 2^-11 A) vmax for the
  // fp16 P, the fp16 result and, in the folded 8-wave form, the fp16 Q' (A = max sum_e |q'_e k_e| in log2 units), plus
  // 2 ln2 (ceil(D / 16) + 1) 2^-24 (Bmax + T) vmax for the accumulator that starts at the logit (T = max |biased score|)
  double me = 0, mr = 0, vmax = 0, Amax = 0, Tmax = 0, Bmax = 0;
  const double LOG2E = 1.4426950408889634;
  for (auto& x : V) vmax = std::max(vmax, fabs((double)x));
  std::vector<double> s(Nk);
  for (int b = 0; b < B && rc == 0; ++b)
    for (int h = 0; h < H; ++h)
      for (int i = 0; i < Nq; ++i) {
        double mx = -1e300;
        for (int j = 0; j < Nk; ++j) {
          double a = 0, aa = 0;
          for (int e = 0; e < D; ++e) {
            const double pr = (double)Q[((size_t)b * Nq + i) * C + h * D + e] * (double)K[((size_t)b * Nk + j) * C + h * D + e];
            a += pr;
            aa += fabs(pr);
          }
          const double bj = (double)kb[b * kb_bs + j];
          s[j] = a * d.scale + bj * 0.6931471805599453;
          if (bj > -1e300) {
            Amax = std::max(Amax, aa * d.scale * LOG2E);
            Tmax = std::max(Tmax, fabs(s[j] * LOG2E));
            Bmax = std::max(Bmax, fabs(bj));
          }
          mx = std::max(mx, s[j]);
        }
        double den = 0;
        for (int j = 0; j < Nk; ++j) { s[j] = exp(s[j] - mx); den += s[j]; }
        for (int e = 0; e < D; ++e) {
          double o = 0;
          for (int j = 0; j < Nk; ++j) o += s[j] * (double)V[((size_t)b * Nk + j) * C + h * D + e];
          o /= den;
          mr = std::max(mr, fabs(o));
          const double got = (double)O[((size_t)b * Nq + i) * C + h * D + e];
          me = std::max(me, got == got ? fabs(o - got) : 1e30);
        }
      }
  free(kb);
  const bool folded = D == 40 && getenv("PFD_ATTN_FORCE8") && atoi(getenv("PFD_ATTN_FORCE8")) != 0;
  const double bound = (3 * ldexp(1.0, -11) + Nk * ldexp(1.0, -25) + ldexp(1.0, -16) + (folded ? 2 * 0.6931471805599453 * ldexp(1.0, -11) * Amax : 0.0) +
                        2 * 0.6931471805599453 * ((D + 15) / 16 + 1) * ldexp(1.0, -24) * (Bmax + Tmax)) * vmax;
  const bool ok = rc == 0 && me <= bound;
  ++g_total;
  g_fail += !ok;
  printf("%s attention kbias pattern %d B%d H%d Nq%d Nk%d D%d  rc %d  max err %.2e = %.3f of the bound (max |ref| %.2f)\n", ok ? "ok  " : "FAIL",
         pattern, B, H, Nq, Nk, D, rc, me, me / bound, mr);
  fflush(stdout);
}

// pfd_attention_rbias_f16: nr rows of logits per sample and a region per query, against the weighted softmax in double precision.
// Row 0 masks reference 0 (keys 0 .. Nk / 2 - 1: the whole first key tile and more), row 1 masks reference 1 (the trailing
// tiles), row 2 masks keys 64 .. 127 (a middle tile) and every fifth key, rows 3 .. are random logits in [-12, 0].  Regions
// change every five queries (inside a wave's 32) and start at b, so the samples differ; shared: one map for the batch (qr_bs = 0).
static void run_case_rbias(int B, int H, int Nq, int Nk, int D, int nr, bool shared) {
  const int C = H * D;
  const long nkp = (Nk + 7) / 8 * 8, rb_rs = (Nk + 3) / 4 * 4 + 4, rb_bs = nr * rb_rs;
  auto Q = rand_h((size_t)B * Nq * C, 1.5f), K = rand_h((size_t)B * Nk * C, 1.5f), V = rand_h((size_t)B * Nk * C, 1.f);
  std::vector<h16> Vt((size_t)C * B * nkp, (h16)0.f), O((size_t)B * Nq * C, (h16)-9.f);
  for (int b = 0; b < B; ++b)
    for (int j = 0; j < Nk; ++j)
      for (int c = 0; c < C; ++c) Vt[(size_t)c * B * nkp + (size_t)b * nkp + j] = V[((size_t)b * Nk + j) * C + c];
  float* rb = (float*)aligned_alloc(16, sizeof(float) * B * rb_bs);
  std::uniform_real_distribution<float> u(-12.f, 0.f);
  const int half = Nk / 2;
  for (int b = 0; b < B; ++b)
    for (int g = 0; g < nr; ++g)
      for (long j = 0; j < rb_rs; ++j) {
        float v = NAN;
        if (j < Nk) {
          if (g == 0) v = j < half ? -INFINITY : u(rng);
          else if (g == 1) v = j < half ? (b ? -1.f : 0.f) : -INFINITY;
          else if (g == 2) v = ((j >= 64 && j < 128) || j % 5 == 0) ? -INFINITY : u(rng);
          else v = u(rng);
        }
        rb[b * rb_bs + g * rb_rs + j] = v;
      }
  std::vector<uint8_t> qr((size_t)B * Nq);
  for (int b = 0; b < B; ++b)
    for (int i = 0; i < Nq; ++i) qr[(size_t)b * Nq + i] = (uint8_t)((i / 5 + (shared ? 0 : b)) % nr);
  PfdAttnDesc d;
  memset(&d, 0, sizeof(d));
  d.Q = Q.data(); d.K = K.data(); d.Vt = Vt.data(); d.O = O.data();
  d.ldq = C; d.ldk = C; d.ldo = C; d.ldvt = (long)B * nkp;
  d.q_bs = (long)Nq * C; d.k_bs = (long)Nk * C; d.o_bs = (long)Nq * C; d.vt_bs = nkp;
  d.B = B; d.H = H; d.Nq = Nq; d.Nk = Nk; d.D = D;
  d.scale = 1.0f / sqrtf((float)D);
  const int rc = pfd_attention_rbias_f16(&d, rb, rb_rs, rb_bs, nr, qr.data(), shared ? 0 : Nq, nullptr);
  // the bound of the GPU tests (tests/refmix_refs.py kbias_bound, unfolded classes), Bmax and T over the table
  double me = 0, mr = 0, vmax = 0, Tmax = 0, Bmax = 0;
  const double LOG2E = 1.4426950408889634;
  for (auto& x : V) vmax = std::max(vmax, fabs((double)x));
  std::vector<double> s(Nk);
  for (int b = 0; b < B && rc == 0; ++b)
    for (int h = 0; h < H; ++h)
      for (int i = 0; i < Nq; ++i) {
        const float* row = rb + b * rb_bs + qr[(size_t)(shared ? 0 : b) * Nq + i] * rb_rs;
        double mx = -1e300;
        for (int j = 0; j < Nk; ++j) {
          double a = 0;
          for (int e = 0; e < D; ++e) a += (double)Q[((size_t)b * Nq + i) * C + h * D + e] * (double)K[((size_t)b * Nk + j) * C + h * D + e];
          const double bj = (double)row[j];
          s[j] = a * d.scale + bj * 0.6931471805599453;
          if (bj > -1e300) {
            Tmax = std::max(Tmax, fabs(s[j] * LOG2E));
            Bmax = std::max(Bmax, fabs(bj));
          }
          mx = std::max(mx, s[j]);
        }
        double den = 0;
        for (int j = 0; j < Nk; ++j) { s[j] = exp(s[j] - mx); den += s[j]; }
        for (int e = 0; e < D; ++e) {
          double o = 0;
          for (int j = 0; j < Nk; ++j) o += s[j] * (double)V[((size_t)b * Nk + j) * C + h * D + e];
          o /= den;
          mr = std::max(mr, fabs(o));
          const double got = (double)O[((size_t)b * Nq + i) * C + h * D + e];
          me = std::max(me, got == got ? fabs(o - got) : 1e30);
        }
      }
  free(rb);
  const double bound = (3 * ldexp(1.0, -11) + Nk * ldexp(1.0, -25) + ldexp(1.0, -16) +
                        2 * 0.6931471805599453 * ((D + 15) / 16 + 1) * ldexp(1.0, -24) * (Bmax + Tmax)) * vmax;
  const bool ok = rc == 0 && me <= bound;
  ++g_total;
  g_fail += !ok;
  printf("%s attention rbias nr %d %s B%d H%d Nq%d Nk%d D%d  rc %d  max err %.2e = %.3f of the bound (max |ref| %.2f)\n", ok ? "ok  " : "FAIL",
         nr, shared ? "shared" : "per-sample", B, H, Nq, Nk, D, rc, me, me / bound, mr);
  fflush(stdout);
}

// The operands on which the named mutants of lib/regions.py are a thousand bounds from the specification (the construction of
// tests/regions_refs.py `discriminating`, with a sign vector of its own): every query and key along one sign vector, so that
// the score of key j is t_j log2 units for every query; keys 0 .. 73 are reference 0 (V = +1), 74 .. 147 reference 1 (V = -1);
// row 0 of the table masks reference 1, row 1 masks reference 0 -- the whole first key tile.  The specification says +1 in
// region 0 and -1 in region 1, exactly.  kind 0: regions alternate from query to query (region_ignored, region_of_next_query);
// 1: sample 1 has its rows swapped (table_of_sample0); 2: the live keys of region 1 at -12 (masked_leading_tile_scored_zero);
// 3: a left / right map on the 6 x 6 grid (grid_transposed); 4: every query in region 1 (grid_top_left).
static void run_case_rbias_disc(int D, int kind) {
  const int B = 2, H = 1, Nq = 36, Nk = 148, C = D, nr = 2, tref = Nk / 2;
  const long nkp = (Nk + 7) / 8 * 8, rb_rs = (Nk + 3) / 4 * 4 + 4, rb_bs = nr * rb_rs;
  const float scale = 1.0f / sqrtf((float)D);
  const double c = (double)scale * 1.4426950408889634;
  std::vector<float> u(D);
  for (int e = 0; e < D; ++e) u[e] = ((e * 7 + e / 3) % 3 == 0) ? -1.f : 1.f;
  std::vector<h16> Q((size_t)B * Nq * C), K((size_t)B * Nk * C), Vt((size_t)C * B * nkp, (h16)0.f), O((size_t)B * Nq * C, (h16)-9.f);
  for (size_t i = 0; i < Q.size(); ++i) Q[i] = (h16)u[i % C];
  for (int b = 0; b < B; ++b)
    for (int j = 0; j < Nk; ++j) {
      const double t = (kind == 2 && j >= tref) ? -12.0 : 0.0;
      for (int e = 0; e < C; ++e) {
        K[((size_t)b * Nk + j) * C + e] = (h16)(float)(t / (D * c) * u[e]);
        Vt[(size_t)e * B * nkp + (size_t)b * nkp + j] = (h16)(j < tref ? 1.f : -1.f);
      }
    }
  float* rb = (float*)aligned_alloc(16, sizeof(float) * B * rb_bs);
  for (int b = 0; b < B; ++b)
    for (int g = 0; g < nr; ++g)
      for (long j = 0; j < rb_rs; ++j) {
        const bool rowA = (g == 0) != (kind == 1 && b == 1);          // this row listens to reference 0
        rb[b * rb_bs + g * rb_rs + j] = j >= Nk ? NAN : ((j < tref) == rowA ? 0.f : -INFINITY);
      }
  std::vector<uint8_t> qr((size_t)B * Nq);
  for (int b = 0; b < B; ++b)
    for (int i = 0; i < Nq; ++i) qr[(size_t)b * Nq + i] = (uint8_t)(kind == 3 ? (i % 6 >= 3) : kind == 4 ? 1 : i % 2);
  PfdAttnDesc d;
  memset(&d, 0, sizeof(d));
  d.Q = Q.data(); d.K = K.data(); d.Vt = Vt.data(); d.O = O.data();
  d.ldq = C; d.ldk = C; d.ldo = C; d.ldvt = (long)B * nkp;
  d.q_bs = (long)Nq * C; d.k_bs = (long)Nk * C; d.o_bs = (long)Nq * C; d.vt_bs = nkp;
  d.B = B; d.H = H; d.Nq = Nq; d.Nk = Nk; d.D = D;
  d.scale = scale;
  const int rc = pfd_attention_rbias_f16(&d, rb, rb_rs, rb_bs, nr, qr.data(), Nq, nullptr);
  double me = 0;
  for (int b = 0; b < B && rc == 0; ++b)
    for (int i = 0; i < Nq; ++i) {
      const bool rowA = (qr[(size_t)b * Nq + i] == 0) != (kind == 1 && b == 1);
      for (int e = 0; e < C; ++e) {
        const double got = (double)O[((size_t)b * Nq + i) * C + e];
        me = std::max(me, got == got ? fabs(got - (rowA ? 1.0 : -1.0)) : 1e30);
      }
    }
  free(rb);
  // the bound of the GPU tests with vmax = 1, Bmax = 0 and T = 12 (every live score is 0 or -12)
  const double bound = 3 * ldexp(1.0, -11) + Nk * ldexp(1.0, -25) + ldexp(1.0, -16) + 2 * 0.6931471805599453 * ((D + 15) / 16 + 1) * ldexp(1.0, -24) * 12.0;
  const bool ok = rc == 0 && me <= bound;
  ++g_total;
  g_fail += !ok;
  printf("%s attention rbias mutant-operands kind %d D%d  rc %d  max err %.2e = %.3f of the bound\n", ok ? "ok  " : "FAIL", kind, D, rc, me, me / bound);
  fflush(stdout);
}

int main(int argc, char** argv) {
  bool quick = false, force8 = true, kbias = false;
  for (int i = 1; i < argc; ++i) {
    if (!strcmp(argv[i], "--rbias")) {    // every class pfd_attention_rbias_f16 has: the 4-wave d = 40 form, d = 80, d = 160
      run_case_rbias(2, 1, 130, 200, 40, 8, false);   // two blocks, ragged queries and keys, every row kind, 8 regions
      run_case_rbias(2, 2, 70, 148, 40, 3, true);
      run_case_rbias(1, 1, 40, 148, 40, 1, true);     // one region whose first tile is masked in full
      run_case_rbias(2, 1, 64, 148, 80, 5, false);
      run_case_rbias(2, 1, 40, 200, 160, 4, false);
      for (int D : {40, 80, 160})           // the operands of the named mutants, every class
        for (int kind = 0; kind < 5; ++kind) run_case_rbias_disc(D, kind);
      printf("%d cases, %d failed\n", g_total, g_fail);
      return g_fail;
    }
    kbias = kbias || !strcmp(argv[i], "--kbias");
    if (!strcmp(argv[i], "--a3")) {       // attention3_kernel: whole 64-key tiles; one block / ragged queries / three heads
      setenv("PFD_ATTN3_FORCE", "1", 1);
      run_case(1, 1, 256, 192, 40);
      run_case(1, 2, 300, 128, 40);
      run_case(2, 1, 256, 320, 40);
      run_case(1, 1, 256, 320, 40, 200);   // deferred rescale taken in tile 3 (sub-block A or B by the query's position)
      run_case(1, 1, 256, 256, 40, 100);   // ... in tile 1, query 100 = sub-block B of wave 1
      run_case(1, 1, 256, 704, 40, 500);   // 11 tiles: both rings wrap twice (odd count: single-tile interval + five pairs)
      run_case(1, 1, 256, 768, 40);        // 12 tiles: pairs only
      printf("%d cases, %d failed\n", g_total, g_fail);
      return g_fail;
    }
    quick = quick || !strcmp(argv[i], "--quick");
    if (!strcmp(argv[i], "--w4")) force8 = false;   // the 4-wave d = 40 form (what small launches take)
  }
  if (force8) setenv("PFD_ATTN_FORCE8", "1", 1);      // the 8-wave d = 40 form at these (small) sizes
  else unsetenv("PFD_ATTN_FORCE8");
  if (kbias) {   // --kbias: the 8-wave folded d = 40 form, d = 80 and d = 160; --kbias --w4: the 4-wave d = 40 form
    run_case_kbias(2, 1, 130, 200, 40, 1);  // sample 0: keys 100.. masked = tile 2 and the peeled tile in full
    run_case_kbias(1, 2, 70, 148, 40, 2);   // holes: tile 1 masked in full between two live tiles
    run_case_kbias(1, 1, 40, 148, 40, 0);
    if (force8) {
      run_case_kbias(2, 1, 64, 148, 80, 1);
      run_case_kbias(1, 1, 40, 148, 80, 2);
      run_case_kbias(2, 1, 40, 200, 160, 1);
      run_case_kbias(1, 1, 40, 148, 160, 2);
    }
    printf("%d cases, %d failed\n", g_total, g_fail);
    return g_fail;
  }
  run_case(1, 2, 300, 200, 40);           // ragged queries and keys, 4 KV tiles (3 full + 1 peeled)
  run_case(1, 1, 256, 148, 40);           // the cross-attention length (148 context tokens)
  if (!quick) {
    run_case(2, 1, 64, 64, 160);          // 8^2 level
    run_case(1, 1, 100, 77, 80);
    run_case(1, 1, 130, 96, 96);          // SeeCoder
  }
  printf("%d cases, %d failed\n", g_total, g_fail);
  return g_fail;
}
