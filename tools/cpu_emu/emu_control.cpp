// CPU emulation of csrc/control.hip (test infrastructure; see hip/hip_runtime.h in this directory for the execution model):
// pfd_add_scaled_rows_f16 runs through the library's own entry point on cases given on the command line, and pfd_add_f16
// of csrc/elementwise.hip next to it, so that a test can hold the two against each other bit for bit.  The driver checks
// the return code against the one the case expects and the guard bands around every buffer, prints one line per case
// (with the kernel launched) and leaves the output next to the input for the test to judge against lib/control.py.
//
// usage: emu_control <case> ...
//   scaled,B,n,stride,alias,offset,rc,path   <path>: f16 x [B][n], f16 r [B][n], f32 scale [(B-1)*stride + 1];
//                                            alias 0: y apart, 1: y = x, 2: y = r;  offset: x starts that many halves
//                                            behind a 16-byte boundary;  rc: the return code expected (0: one launch);
//                                            written: <path>.out (f16 [B][n]; untouched 0xA5 bytes where rc != 0)
//   add,n,path                               <path>: f16 a [n], f16 b [n];  written: <path>.out = pfd_add_f16
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
#include "control_emu.inc"

// a buffer whose payload starts `offset` halves behind a 16-byte boundary, with a guard band on both sides
struct Guarded {
  std::vector<unsigned char> mem;
  size_t off, n;
  Guarded(size_t bytes, int offset) : mem(bytes + 160, 0xA5), n(bytes) {
    off = 48;
    while (((uintptr_t)(mem.data() + off) & 15) != (uintptr_t)(offset & 7) * 2) ++off;
  }
  unsigned char* p() { return mem.data() + off; }
  bool intact() const {
    for (size_t i = 0; i < mem.size(); ++i)
      if ((i < off || i >= off + n) && mem[i] != 0xA5) return false;
    return true;
  }
};

static void write_file(const std::string& path, const void* p, size_t bytes) {
  FILE* f = fopen(path.c_str(), "wb");
  if (!f || fwrite(p, 1, bytes, f) != bytes) { fprintf(stderr, "emu_control: cannot write %s\n", path.c_str()); exit(2); }
  fclose(f);
}

static void read_exact(FILE* in, void* p, size_t bytes, const std::string& path) {
  if (bytes && fread(p, 1, bytes, in) != bytes) { fprintf(stderr, "emu_control: %s is too short for its case\n", path.c_str()); exit(2); }
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

static int run_scaled(const std::string& s) {
  std::string path;
  const std::vector<std::string> f = split(s, 7, &path);
  if (f.size() != 7) { fprintf(stderr, "emu_control: malformed case %s\n", s.c_str()); exit(2); }
  const int B = atoi(f[1].c_str()), stride = atoi(f[3].c_str()), alias = atoi(f[4].c_str()), offset = atoi(f[5].c_str());
  const long n = atol(f[2].c_str());
  const int want = atoi(f[6].c_str());
  if (B < 1 || n < 1 || stride < 1 || alias < 0 || alias > 2) { fprintf(stderr, "emu_control: %s: bad case\n", s.c_str()); exit(2); }
  const size_t bytes = (size_t)B * n * 2, ns = (size_t)(B - 1) * stride + 1;
  Guarded x(bytes, offset), r(bytes, 0), y(bytes, 0), sc(ns * 4, 0);
  FILE* in = fopen(path.c_str(), "rb");
  if (!in) { fprintf(stderr, "emu_control: cannot read %s\n", path.c_str()); exit(2); }
  read_exact(in, x.p(), bytes, path);
  read_exact(in, r.p(), bytes, path);
  read_exact(in, sc.p(), ns * 4, path);
  if (fgetc(in) != EOF) { fprintf(stderr, "emu_control: %s is longer than its case\n", path.c_str()); exit(2); }
  fclose(in);
  unsigned char* out = alias == 1 ? x.p() : alias == 2 ? r.p() : y.p();
  const int rc = pfd_add_scaled_rows_f16(x.p(), r.p(), (const float*)sc.p(), stride, out, B, n, nullptr);
  const bool guards = x.intact() && r.intact() && y.intact() && sc.intact();
  const bool ok = rc == want && guards && emu::launch_log.size() == (rc == 0 ? 1u : 0u);
  printf("%s scaled B %d n %ld stride %d alias %d offset %d  rc %d (expected %d)%s | %s\n", ok ? "ok  " : "FAIL", B, n, stride,
         alias, offset, rc, want, guards ? "" : ", WRITE OUTSIDE A BUFFER", kernel_and_reset().c_str());
  fflush(stdout);
  write_file(path + ".out", out, bytes);
  return !ok;
}

static int run_add(const std::string& s) {
  std::string path;
  const std::vector<std::string> f = split(s, 2, &path);
  if (f.size() != 2) { fprintf(stderr, "emu_control: malformed case %s\n", s.c_str()); exit(2); }
  const long n = atol(f[1].c_str());
  if (n < 1) { fprintf(stderr, "emu_control: %s: bad case\n", s.c_str()); exit(2); }
  Guarded a((size_t)n * 2, 0), b((size_t)n * 2, 0), y((size_t)n * 2, 0);
  FILE* in = fopen(path.c_str(), "rb");
  if (!in) { fprintf(stderr, "emu_control: cannot read %s\n", path.c_str()); exit(2); }
  read_exact(in, a.p(), (size_t)n * 2, path);
  read_exact(in, b.p(), (size_t)n * 2, path);
  if (fgetc(in) != EOF) { fprintf(stderr, "emu_control: %s is longer than its case\n", path.c_str()); exit(2); }
  fclose(in);
  const int rc = pfd_add_f16(a.p(), b.p(), y.p(), n, nullptr);
  const bool guards = a.intact() && b.intact() && y.intact();
  const bool ok = rc == 0 && guards && emu::launch_log.size() == 1;
  printf("%s add n %ld  rc %d%s | %s\n", ok ? "ok  " : "FAIL", n, rc, guards ? "" : ", WRITE OUTSIDE A BUFFER",
         kernel_and_reset().c_str());
  fflush(stdout);
  write_file(path + ".out", y.p(), (size_t)n * 2);
  return !ok;
}

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: emu_control scaled,...|add,... (see the head of emu_control.cpp)\n"); return 2; }
  int fail = 0;
  for (int a = 1; a < argc; ++a) {
    const std::string s = argv[a];
    if (s.rfind("scaled,", 0) == 0) fail += run_scaled(s);
    else if (s.rfind("add,", 0) == 0) fail += run_add(s);
    else { fprintf(stderr, "emu_control: unknown case %s\n", argv[a]); return 2; }
  }
  return fail != 0;
}
