// CPU emulation of the element-wise entry points of csrc/elementwise.hip (test infrastructure; see hip/hip_runtime.h in this
// directory for the execution model): pfd_image_u8_f16, pfd_act_f16, pfd_add_f16, pfd_axpby_f16, pfd_add_rowvec_f16 and
// pfd_add_rowvec_lnstats_f16 run through the library's own entry points on cases given on the command line.  Every buffer
// has a 0xA5 guard band on both sides.  The driver checks the return code against the one the case expects, that exactly
// one kernel was launched (none where the call is refused) and the guard bands, prints one line per case and leaves the
// output next to the input for the test to judge (tests/test_boundary_kernels_cpu.py).
//
// usage: emu_elementwise <case> ...     every case: op,p0,p1,p2,alias,offin,offout,null,rc,path
//   op      p0, p1, p2               <path> holds                     <path>.out receives
//   image   n, f16_image, k          f16 x [n]                        u8 [n]   (mul, add) = (0.5, 0.5) for k = 0, (1, 0) for k = 1
//   act     n, act, 0                f16 x [n]                        f16 [n]
//   add     n, 0, 0                  f16 a [n], f16 b [n]             f16 [n]
//   axpby   n, 0, 0                  f16 a [n], f16 b [n]             f16 [n]  alpha = 0.75, beta = -1.25
//   rowvec  R, C, 0                  f16 x [R][C], f16 v [C]          f16 [R][C]
//   rowstat R, C, 0                  f16 x [R][C], f16 v [C]          f16 [R][C], then f32 [R][C / 160][2]
//   alias   0: y apart, 1: y = the first input (x / a), 2: y = the second (b)
//   offin   the first input starts that many bytes behind a 16-byte boundary;  offout: the same for y (alias 0)
//   null    0: none, 1: the first input is NULL, 2: y is NULL, 3: the second input (b / v) is NULL (legal for add / axpby)
//   rc      the return code expected (0: one launch)
// Where the call is refused the output file holds the untouched 0xA5 bytes of y.
#include <stdio.h>

#include <string>

#include "hip/hip_runtime.h"


#include "pfd_common.h"
bool pfd_prof_on() { return false; }
void pfd_prof_begin(int, double, double, hipStream_t) {}
void pfd_prof_end(hipStream_t) {}
int pfd_check_launch(const char*) { return 0; }
static std::string g_err;
void pfd_set_error(const char* m) { g_err = m ? m : ""; }

#include "elementwise_emu.inc"

// a buffer whose payload starts `offset` bytes behind a 16-byte boundary, with a guard band on both sides
struct Guarded {
  std::vector<unsigned char> mem;
  size_t off, n;
  Guarded(size_t bytes, int offset) : mem(bytes + 160, 0xA5), n(bytes) {
    off = 48;
    while (((uintptr_t)(mem.data() + off) & 15) != (uintptr_t)(offset & 15)) ++off;
  }
  unsigned char* p() { return mem.data() + off; }
  bool intact() const {
    for (size_t i = 0; i < mem.size(); ++i)
      if ((i < off || i >= off + n) && mem[i] != 0xA5) return false;
    return true;
  }
};

static void write_file(const std::string& path, const void* a, size_t na, const void* b = nullptr, size_t nb = 0) {
  FILE* f = fopen(path.c_str(), "wb");
  if (!f || fwrite(a, 1, na, f) != na || fwrite(b, 1, nb, f) != nb) { fprintf(stderr, "emu_elementwise: cannot write %s\n", path.c_str()); exit(2); }
  fclose(f);
}

static void read_exact(FILE* in, void* p, size_t bytes, const std::string& path) {
  if (bytes && fread(p, 1, bytes, in) != bytes) { fprintf(stderr, "emu_elementwise: %s is too short for its case\n", path.c_str()); exit(2); }
}

static std::vector<std::string> split(const std::string& s, size_t nfields, std::string* rest) {
  std::vector<std::string> f;
  size_t at = 0;
  for (size_t c; f.size() < nfields && (c = s.find(',', at)) != std::string::npos; at = c + 1) f.push_back(s.substr(at, c - at));
  *rest = s.substr(at);      // the rest, commas included
  return f;
}

static std::string kernel_and_reset() {
  const std::string k = emu::launch_log.empty() ? "" : emu::launch_log[0].kernel;
  emu::launched.clear();
  emu::launch_log.clear();
  return k;
}

static int run_case(const std::string& s) {
  std::string path;
  const std::vector<std::string> f = split(s, 9, &path);
  if (f.size() != 9) { fprintf(stderr, "emu_elementwise: malformed case %s\n", s.c_str()); exit(2); }
  const std::string op = f[0];
  const long p0 = atol(f[1].c_str());
  const int p1 = atoi(f[2].c_str()), p2 = atoi(f[3].c_str()), alias = atoi(f[4].c_str()), offin = atoi(f[5].c_str()),
            offout = atoi(f[6].c_str()), null = atoi(f[7].c_str()), want = atoi(f[8].c_str());
  const bool rows = op == "rowvec" || op == "rowstat", two = op == "add" || op == "axpby";
  if (!(rows || two || op == "image" || op == "act") || p0 < 0 || alias < 0 || alias > (two ? 2 : 1) || null < 0 || null > 3 ||
      (op == "image" && alias) || (rows && p1 < 0)) {
    fprintf(stderr, "emu_elementwise: %s: bad case\n", s.c_str());
    exit(2);
  }
  // sizes in bytes: the first input, the second input, the output, the statistics
  const size_t n = rows ? (size_t)p0 * p1 : (size_t)p0;
  const size_t b0 = n * 2, b1 = rows ? (size_t)p1 * 2 : two ? n * 2 : 0, by = op == "image" ? n : n * 2;
  const size_t bs = op == "rowstat" ? (size_t)p0 * (p1 / 160) * 8 : 0;
  Guarded in0(b0, offin), in1(b1, 0), y(by, offout), st(bs, 0);
  FILE* in = fopen(path.c_str(), "rb");
  if (!in) { fprintf(stderr, "emu_elementwise: cannot read %s\n", path.c_str()); exit(2); }
  read_exact(in, in0.p(), b0, path);
  read_exact(in, in1.p(), b1, path);
  if (fgetc(in) != EOF) { fprintf(stderr, "emu_elementwise: %s is longer than its case\n", path.c_str()); exit(2); }
  fclose(in);
  unsigned char* out = alias == 1 ? in0.p() : alias == 2 ? in1.p() : y.p();
  const void* a0 = null == 1 ? nullptr : in0.p();
  const void* a1 = null == 3 ? nullptr : in1.p();
  void* ay = null == 2 ? nullptr : out;
  int rc;
  if (op == "image") rc = pfd_image_u8_f16(a0, ay, p0, p2 ? 1.0f : 0.5f, p2 ? 0.0f : 0.5f, p1, nullptr);
  else if (op == "act") rc = pfd_act_f16(a0, ay, p0, p1, nullptr);
  else if (op == "add") rc = pfd_add_f16(a0, a1, ay, p0, nullptr);
  else if (op == "axpby") rc = pfd_axpby_f16(a0, 0.75f, a1, -1.25f, ay, p0, nullptr);
  else if (op == "rowvec") rc = pfd_add_rowvec_f16(a0, p1, a1, ay, p1, (int32_t)p0, p1, nullptr);
  else rc = pfd_add_rowvec_lnstats_f16(a0, p1, a1, ay, p1, (int32_t)p0, p1, st.p(), nullptr);
  const bool guards = in0.intact() && in1.intact() && y.intact() && st.intact();
  const bool ok = rc == want && guards && emu::launch_log.size() == (rc == 0 ? 1u : 0u);
  printf("%s %s %ld %d %d alias %d offin %d offout %d null %d  rc %d (expected %d)%s | %s\n", ok ? "ok  " : "FAIL", op.c_str(), p0, p1,
         p2, alias, offin, offout, null, rc, want, guards ? "" : ", WRITE OUTSIDE A BUFFER", kernel_and_reset().c_str());
  fflush(stdout);
  write_file(path + ".out", out, by, st.p(), bs);
  return !ok;
}

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: emu_elementwise op,p0,p1,p2,alias,offin,offout,null,rc,path ... (see the head of emu_elementwise.cpp)\n"); return 2; }
  int fail = 0;
  for (int a = 1; a < argc; ++a) fail += run_case(argv[a]);
  return fail != 0;
}
