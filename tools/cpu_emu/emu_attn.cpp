// CPU emulation of csrc/attention.hip (see hip/hip_runtime.h): the fused attention kernels (8-wave d = 40 form with the PV
// product on 16x16x32 and the maximum folded into the QK^T MFMA; 4-wave form for every head dim) against a double-precision
// softmax(scale Q K^T) V.
//   usage: emu_attn [--quick] [--w4] [--kbias]     (--w4: the 4-wave d = 40 form; prints one line per case with a checksum of the output bits;
//                                                    --kbias: pfd_attention_kbias_f16, the per-key logit operand, every kernel class it has)
//          emu_attn --rbias                        (pfd_attention_rbias_f16, a logit row per region of the query: d = 40, 80, 160)
//          emu_attn --dispatch FILE                (a dry run of the three entry points: what they decide, one text line per request)
#include <stdio.h>

#include <functional>
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

// the dense descriptor of the drivers: channels-last Q / K / O, V^T rows of B x (Nk rounded up to 8) keys
static PfdAttnDesc dense_desc(const void* Q, const void* K, const void* Vt, void* O, int B, int H, int Nq, int Nk, int D) {
  const long C = (long)H * D, nkp = (Nk + 7) / 8 * 8;
  PfdAttnDesc d;
  memset(&d, 0, sizeof(d));
  d.Q = Q; d.K = K; d.Vt = Vt; d.O = O;
  d.ldq = C; d.ldk = C; d.ldo = C; d.ldvt = (long)B * nkp;
  d.q_bs = (long)Nq * C; d.k_bs = (long)Nk * C; d.o_bs = (long)Nq * C; d.vt_bs = nkp;
  d.B = B; d.H = H; d.Nq = Nq; d.Nk = Nk; d.D = D;
  d.scale = 1.0f / sqrtf((float)D);
  return d;
}

// One problem: random Q, K, V (drawn from rng in this order; the logits of a case come after them), the padded V^T, the output
// (preset to -9) and the descriptor.  spike > 0: key `spike` = 4 x query (spike % Nq), the row maximum jumps in the middle of the stream
struct Problem {
  const int B, H, Nq, Nk, D, C;
  std::vector<h16> Q, K, V, Vt, O;
  PfdAttnDesc d;
  Problem(int B, int H, int Nq, int Nk, int D, int spike = 0)
      : B(B), H(H), Nq(Nq), Nk(Nk), D(D), C(H * D), Q(rand_h((size_t)B * Nq * C, 1.5f)), K(rand_h((size_t)B * Nk * C, 1.5f)),
        V(rand_h((size_t)B * Nk * C, 1.f)), O((size_t)B * Nq * C, (h16)-9.f) {
    const long nkp = (Nk + 7) / 8 * 8;
    if (spike > 0 && spike < Nk)
      for (int b = 0; b < B; ++b)
        for (int c = 0; c < C; ++c) K[((size_t)b * Nk + spike) * C + c] = (h16)(4.0f * (float)Q[((size_t)b * Nq + spike % Nq) * C + c]);
    Vt.assign((size_t)C * B * nkp, (h16)0.f);
    for (int b = 0; b < B; ++b)
      for (int j = 0; j < Nk; ++j)
        for (int c = 0; c < C; ++c) Vt[(size_t)c * B * nkp + (size_t)b * nkp + j] = V[((size_t)b * Nk + j) * C + c];
    d = dense_desc(Q.data(), K.data(), Vt.data(), O.data(), B, H, Nq, Nk, D);
  }
};

// softmax(scale Q K^T + ln2 row) V in double precision against p.O (a NaN there, or what a declined call left, is an error); row(b, i): the Nk logits of
// query i of sample b in log2 units, or no function at all.  Returns the maxima the bounds need: the error, |ref|, |V|, and over
// the live keys A = sum_e |q'_e k_e|, T = |biased score| (both in log2 units) and |logit|
struct RefMax { double me = 0, mr = 0, vmax = 0, A = 0, T = 0, Bm = 0; };
static RefMax reference(const Problem& p, const std::function<const float*(int, int)>& row = nullptr) {
  const double LOG2E = 1.4426950408889634, LN2 = 0.6931471805599453;
  const int Nq = p.Nq, Nk = p.Nk, D = p.D, C = p.C;
  RefMax m;
  for (auto& x : p.V) m.vmax = std::max(m.vmax, fabs((double)x));
  std::vector<double> s(Nk);
  for (int b = 0; b < p.B; ++b)
    for (int h = 0; h < p.H; ++h)
      for (int i = 0; i < Nq; ++i) {
        const float* logit = row ? row(b, i) : nullptr;
        double mx = -1e300;
        for (int j = 0; j < Nk; ++j) {
          double a = 0, aa = 0;
          for (int e = 0; e < D; ++e) {
            const double pr = (double)p.Q[((size_t)b * Nq + i) * C + h * D + e] * (double)p.K[((size_t)b * Nk + j) * C + h * D + e];
            a += pr;
            aa += fabs(pr);
          }
          const double bj = logit ? (double)logit[j] : 0.0;
          s[j] = a * p.d.scale + bj * LN2;
          if (bj > -1e300) {
            m.A = std::max(m.A, aa * p.d.scale * LOG2E);
            m.T = std::max(m.T, fabs(s[j] * LOG2E));
            m.Bm = std::max(m.Bm, fabs(bj));
          }
          mx = std::max(mx, s[j]);
        }
        double den = 0;
        for (int j = 0; j < Nk; ++j) { s[j] = exp(s[j] - mx); den += s[j]; }
        for (int e = 0; e < D; ++e) {
          double o = 0;
          for (int j = 0; j < Nk; ++j) o += s[j] * (double)p.V[((size_t)b * Nk + j) * C + h * D + e];
          o /= den;
          m.mr = std::max(m.mr, fabs(o));
          const double got = (double)p.O[((size_t)b * Nq + i) * C + h * D + e];
          m.me = std::max(m.me, got == got ? fabs(o - got) : 1e30);
        }
      }
  return m;
}

// the bound of the GPU tests (tests/refmix_refs.py kbias_bound): (3 2^-11 + Nk 2^-25 + 2^-16 + 2 ln2 2^-11 A) vmax for the
// fp16 P, the fp16 result and, in the folded 8-wave form, the fp16 Q' (A = max sum_e |q'_e k_e| in log2 units), plus
// 2 ln2 (ceil(D / 16) + 1) 2^-24 (Bmax + T) vmax for the accumulator that starts at the logit (T = max |biased score|)
static double bias_bound(int Nk, int D, bool folded, double A, double BT, double vmax) {
  return (3 * ldexp(1.0, -11) + Nk * ldexp(1.0, -25) + ldexp(1.0, -16) + (folded ? 2 * 0.6931471805599453 * ldexp(1.0, -11) * A : 0.0) +
          2 * 0.6931471805599453 * ((D + 15) / 16 + 1) * ldexp(1.0, -24) * BT) * vmax;
}

static bool tally(bool ok) {
  ++g_total;
  g_fail += !ok;
  return ok;
}

static void run_case(int B, int H, int Nq, int Nk, int D, int spike = 0) {
  Problem p(B, H, Nq, Nk, D, spike);
  const int rc = pfd_attention_f16(&p.d, nullptr);
  const RefMax m = reference(p);
  uint64_t sum = 1469598103934665603ull;   // FNV-1a over the output bits
  for (auto& x : p.O) { unsigned short u; memcpy(&u, &x, 2); sum = (sum ^ u) * 1099511628211ull; }
  const bool ok = tally(rc == 0 && m.me <= 4e-3 * std::max(1.0, m.mr));
  printf("%s attention B%d H%d Nq%d Nk%d D%d  rc %d  max err %.2e (max |ref| %.2f)  bits %016llx\n", ok ? "ok  " : "FAIL", B, H, Nq, Nk, D, rc, m.me,
         m.mr, (unsigned long long)sum);
  fflush(stdout);
}

// pfd_attention_kbias_f16: per-key logits in log2 units (rows of kb_bs > Nk floats, NaN behind the keys), against the weighted
// softmax in double precision.  pattern 0: two references 0.7 / 0.3; 1: sample b keeps 1 + b % 2 halves, the rest is -inf (whole
// trailing tiles masked); 2: -inf on keys 64..127 and on every fifth key, key 0 finite, random logits in [-12, 0] elsewhere
static void run_case_kbias(int B, int H, int Nq, int Nk, int D, int pattern) {
  Problem p(B, H, Nq, Nk, D);
  const long kb_bs = (Nk + 3) / 4 * 4 + 4;
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
  const int rc = pfd_attention_kbias_f16(&p.d, kb, kb_bs, nullptr);
  const RefMax m = reference(p, [&](int b, int) { return kb + b * kb_bs; });
  free(kb);
  const bool folded = attn_plan(B, H, Nq, Nk, D, ATTN_KBIAS, attn_hooks(D)).cls == ATTN_W8;   // the class with an fp16 Q'
  const double bound = bias_bound(Nk, D, folded, m.A, m.Bm + m.T, m.vmax);
  const bool ok = tally(rc == 0 && m.me <= bound);
  printf("%s attention kbias pattern %d B%d H%d Nq%d Nk%d D%d  rc %d  max err %.2e = %.3f of the bound (max |ref| %.2f)\n", ok ? "ok  " : "FAIL",
         pattern, B, H, Nq, Nk, D, rc, m.me, m.me / bound, m.mr);
  fflush(stdout);
}

// pfd_attention_rbias_f16: nr rows of logits per sample and a region per query, against the weighted softmax in double precision.
// Row 0 masks reference 0 (keys 0 .. Nk / 2 - 1: the whole first key tile and more), row 1 masks reference 1 (the trailing
// tiles), row 2 masks keys 64 .. 127 (a middle tile) and every fifth key, rows 3 .. are random logits in [-12, 0].  Regions
// change every five queries (inside a wave's 32) and start at b, so the samples differ; shared: one map for the batch (qr_bs = 0).
static void run_case_rbias(int B, int H, int Nq, int Nk, int D, int nr, bool shared) {
  Problem p(B, H, Nq, Nk, D);
  const long rb_rs = (Nk + 3) / 4 * 4 + 4, rb_bs = nr * rb_rs;
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
  const int rc = pfd_attention_rbias_f16(&p.d, rb, rb_rs, rb_bs, nr, qr.data(), shared ? 0 : Nq, nullptr);
  // the bound of the unfolded classes, Bmax and T over the table
  const RefMax m = reference(p, [&](int b, int i) { return rb + b * rb_bs + qr[(size_t)(shared ? 0 : b) * Nq + i] * rb_rs; });
  free(rb);
  const double bound = bias_bound(Nk, D, false, 0.0, m.Bm + m.T, m.vmax);
  const bool ok = tally(rc == 0 && m.me <= bound);
  printf("%s attention rbias nr %d %s B%d H%d Nq%d Nk%d D%d  rc %d  max err %.2e = %.3f of the bound (max |ref| %.2f)\n", ok ? "ok  " : "FAIL",
         nr, shared ? "shared" : "per-sample", B, H, Nq, Nk, D, rc, m.me, m.me / bound, m.mr);
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
  PfdAttnDesc d = dense_desc(Q.data(), K.data(), Vt.data(), O.data(), B, H, Nq, Nk, D);
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
  const double bound = bias_bound(Nk, D, false, 0.0, 12.0, 1.0);
  const bool ok = tally(rc == 0 && me <= bound);
  printf("%s attention rbias mutant-operands kind %d D%d  rc %d  max err %.2e = %.3f of the bound\n", ok ? "ok  " : "FAIL", kind, D, rc, me, me / bound);
  fflush(stdout);
}

// ---- emu_attn --dispatch FILE: a dry run (emu::dry_run: launches are recorded, nothing executes, no pointer is dereferenced) of
// the three entry points.  One request per line of FILE: "plain|kbias|rbias B H Nq Nk D [key=value ...]" on dense operands with
// fake aligned pointers; the keys change one thing each: null=<operand>, misalign=<operand> (Q K Vt O bias qregion), ldk, kb_bs,
// nr, rb_rs, rb_bs, qr_bs (numbers), scale (a float), slices (PFD_ATTN512_SLICES for this call; unset without the key).
// One line out per request: the request, "-> <return value>", then the instantiated kernel, grid x and block x of the launch.
// PFD_ATTN_FORCE8 / PFD_ATTN3_FORCE are read once per process: one run of the probe per setting. ----
static int dispatch_probe(const char* path) {
  emu::dry_run = true;
  FILE* f = fopen(path, "r");
  if (!f) { fprintf(stderr, "emu_attn: cannot open %s\n", path); return 2; }
  char line[512], api[16];
  for (int ln = 1; fgets(line, sizeof(line), f); ++ln) {
    line[strcspn(line, "\n")] = 0;
    int B, H, Nq, Nk, D, at = 0;
    if (sscanf(line, "%15s %d %d %d %d %d%n", api, &B, &H, &Nq, &Nk, &D, &at) != 6) { fprintf(stderr, "emu_attn: %s:%d: not a request\n", path, ln); return 2; }
    const std::string req = line;
    uintptr_t ptr[6];   // Q K Vt O bias qregion: 16-byte aligned, never dereferenced
    for (int i = 0; i < 6; ++i) ptr[i] = (uintptr_t)0x10000 * (i + 1);
    const char* names[6] = {"Q", "K", "Vt", "O", "bias", "qregion"};
    PfdAttnDesc d = dense_desc(nullptr, nullptr, nullptr, nullptr, B, H, Nq, Nk, D);
    long kb_bs = (Nk + 3) / 4 * 4 + 4, rb_rs = kb_bs, rb_bs = -1, qr_bs = Nq, nr = 2;
    unsetenv("PFD_ATTN512_SLICES");
    for (char* tok = strtok(line + at, " "); tok; tok = strtok(nullptr, " ")) {
      char key[16], val[32];
      if (sscanf(tok, "%15[^=]=%31s", key, val) != 2) { fprintf(stderr, "emu_attn: %s:%d: %s\n", path, ln, tok); return 2; }
      long* num = !strcmp(key, "kb_bs") ? &kb_bs : !strcmp(key, "rb_rs") ? &rb_rs : !strcmp(key, "rb_bs") ? &rb_bs : !strcmp(key, "qr_bs") ? &qr_bs :
                  !strcmp(key, "nr") ? &nr : nullptr;
      int op = 0;
      while (op < 6 && strcmp(val, names[op])) ++op;
      if (num) *num = atol(val);
      else if (!strcmp(key, "ldk")) d.ldk = atol(val);
      else if (!strcmp(key, "scale")) d.scale = strtof(val, nullptr);
      else if (!strcmp(key, "slices")) setenv("PFD_ATTN512_SLICES", val, 1);
      else if (!strcmp(key, "null") && op < 6) ptr[op] = 0;
      else if (!strcmp(key, "misalign") && op < 6) ptr[op] += 8;
      else { fprintf(stderr, "emu_attn: %s:%d: %s\n", path, ln, tok); return 2; }
    }
    if (rb_bs < 0) rb_bs = nr * rb_rs;
    d.Q = (const void*)ptr[0]; d.K = (const void*)ptr[1]; d.Vt = (const void*)ptr[2]; d.O = (void*)ptr[3];
    emu::launch_log.clear();
    int rc;
    char sizes[128] = "";   // the operand sizes the request left to the probe
    if (!strcmp(api, "plain")) rc = pfd_attention_f16(&d, nullptr);
    else if (!strcmp(api, "kbias")) {
      snprintf(sizes, sizeof(sizes), " (kb_bs %ld)", kb_bs);
      rc = pfd_attention_kbias_f16(&d, (const float*)ptr[4], kb_bs, nullptr);
    } else if (!strcmp(api, "rbias")) {
      snprintf(sizes, sizeof(sizes), " (nr %ld rb_rs %ld rb_bs %ld qr_bs %ld)", nr, rb_rs, rb_bs, qr_bs);
      rc = pfd_attention_rbias_f16(&d, (const float*)ptr[4], rb_rs, rb_bs, (int)nr, (const uint8_t*)ptr[5], qr_bs, nullptr);
    } else { fprintf(stderr, "emu_attn: %s:%d: entry point %s\n", path, ln, api); return 2; }
    printf("%s%s -> %d", req.c_str(), sizes, rc);
    for (const auto& l : emu::launch_log) printf(" | %s grid %u block %u", l.kernel.c_str(), l.grid_x, l.block_x);
    printf("\n");
  }
  fclose(f);
  return 0;
}

int main(int argc, char** argv) {
  if (argc > 2 && !strcmp(argv[1], "--dispatch")) return dispatch_probe(argv[2]);
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
