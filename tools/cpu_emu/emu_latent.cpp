// CPU emulation of csrc/latent.hip (test infrastructure; see hip/hip_runtime.h in this directory for the execution model): the
// kernel runs through the library's own entry point, Philox rounds, Box-Muller and all, on cases given on the command line.
// The driver checks the return code and the guard bands around both outputs, prints one line per case and leaves x0 and x_t
// (fp32 NCHW, raw) next to the input for the test to judge against lib/img2img.py.
//
// usage: emu_latent <case> ...     <case> = B,Bm,C,h,w,scale_factor,sq_at,sq_1mat,posterior_mul,offset,want_x0,path
//   <path>: int64 [B][2] key rows, then f16 [Bm][h][w][2C] moments;  written: <path>.xt and (want_x0) <path>.x0
// The four numbers are read with strtof (hex floats pass exactly).  offset: the outputs start that many floats behind a
// 16-byte boundary (0: the 16-byte stores where the sample length allows them; 1: the scalar path).
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

#include "latent_emu.inc"

// an fp32 buffer whose payload starts `offset` floats behind a 16-byte boundary, with a guard band on both sides
struct Guarded {
  std::vector<float> mem;
  size_t off, n;
  Guarded(size_t count, int offset) : mem(count + 32), n(count) {
    off = 8;
    while (((uintptr_t)(mem.data() + off) & 15) != (uintptr_t)(offset & 3) * 4) ++off;
    for (auto& v : mem) memcpy(&v, "\xA5\xA5\xA5\xA5", 4);
  }
  float* p() { return mem.data() + off; }
  bool intact() const {
    for (size_t i = 0; i < mem.size(); ++i)
      if ((i < off || i >= off + n) && memcmp(&mem[i], "\xA5\xA5\xA5\xA5", 4)) return false;
    return true;
  }
};

static void write_file(const std::string& path, const void* p, size_t bytes) {
  FILE* f = fopen(path.c_str(), "wb");
  if (!f || fwrite(p, 1, bytes, f) != bytes) { fprintf(stderr, "emu_latent: cannot write %s\n", path.c_str()); exit(2); }
  fclose(f);
}

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: emu_latent B,Bm,C,h,w,scale_factor,sq_at,sq_1mat,posterior_mul,offset,want_x0,path ...\n"); return 2; }
  int fail = 0;
  for (int a = 1; a < argc; ++a) {
    std::vector<std::string> f;
    const std::string s = argv[a];
    size_t at = 0;
    for (size_t c; f.size() < 11 && (c = s.find(',', at)) != std::string::npos; at = c + 1) f.push_back(s.substr(at, c - at));
    if (f.size() != 11) { fprintf(stderr, "emu_latent: malformed case %s\n", argv[a]); return 2; }
    const std::string path = s.substr(at);      // the rest, commas included
    const int B = atoi(f[0].c_str()), Bm = atoi(f[1].c_str()), C = atoi(f[2].c_str()), h = atoi(f[3].c_str()), w = atoi(f[4].c_str());
    const float sf = strtof(f[5].c_str(), nullptr), sq_at = strtof(f[6].c_str(), nullptr), sq_1mat = strtof(f[7].c_str(), nullptr);
    const float pmul = strtof(f[8].c_str(), nullptr);
    const int offset = atoi(f[9].c_str()), want_x0 = atoi(f[10].c_str());
    if (B < 1 || Bm < 1 || C < 1 || h < 1 || w < 1) { fprintf(stderr, "emu_latent: %s: dimensions must be positive\n", argv[a]); return 2; }
    const size_t nkey = (size_t)B * 2, nmom = (size_t)Bm * h * w * 2 * C, nout = (size_t)B * C * h * w;
    std::vector<int64_t> key(nkey);
    std::vector<half_t> mom(nmom);
    FILE* in = fopen(path.c_str(), "rb");
    if (!in || fread(key.data(), 8, nkey, in) != nkey || fread(mom.data(), 2, nmom, in) != nmom || fgetc(in) != EOF) {
      fprintf(stderr, "emu_latent: %s does not hold the case's keys and moments\n", path.c_str());
      return 2;
    }
    fclose(in);
    Guarded x0(nout, offset), xt(nout, offset);
    const int rc = pfd_latent_start(mom.data(), Bm, key.data(), sf, sq_at, sq_1mat, pmul, want_x0 ? x0.p() : nullptr, xt.p(), B, C, h, w, nullptr);
    const bool guards = x0.intact() && xt.intact();
    const bool ok = rc == 0 && guards && emu::launched.size() == 1;
    fail += !ok;
    printf("%s %dx%dx%dx%d Bm %d offset %d  rc %d%s | %s\n", ok ? "ok  " : "FAIL", B, C, h, w, Bm, offset, rc,
           guards ? "" : ", WRITE OUTSIDE A BUFFER", emu::launched.empty() ? "" : emu::launched[0].c_str());
    fflush(stdout);
    emu::launched.clear();
    emu::launch_log.clear();
    write_file(path + ".xt", xt.p(), nout * 4);
    if (want_x0) write_file(path + ".x0", x0.p(), nout * 4);
  }
  return fail != 0;
}
