// CPU emulation of csrc/inpaint.hip (test infrastructure; see hip/hip_runtime.h in this directory for the execution model): the
// two kernels run through the library's own entry points on cases given on the command line (the masked step: emu_step.cpp).  The driver checks the return code and the guard bands around every output, prints one line per case (with the
// instantiated kernel) and leaves the outputs next to the input for the test to judge against lib/inpaint.py.
//
// usage: emu_inpaint <case> ...
//   grid,Bm,Hm,Wm,gh,gw,f32,path      <path>: u8 [Bm][Hm][Wm];  written: <path>.out (f32 or u8 [Bm][gh][gw])
//   comp,n,Bi,Bs,H,W,C,path           <path>: u8 decoded [n][H][W][C], init [Bi][H][W][C], sel [Bs][H][W];  written: <path>.out
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

#include "inpaint_emu.inc"

// a buffer of T whose payload starts `offset` floats behind a 16-byte boundary, with a guard band on both sides
template <class T>
struct Guarded {
  std::vector<unsigned char> mem;
  size_t off, n;
  Guarded(size_t count, int offset) : mem(count * sizeof(T) + 128, 0xA5), n(count * sizeof(T)) {
    off = 32;
    while (((uintptr_t)(mem.data() + off) & 15) != (uintptr_t)(offset & 3) * 4) ++off;
  }
  T* p() { return reinterpret_cast<T*>(mem.data() + off); }
  bool intact() const {
    for (size_t i = 0; i < mem.size(); ++i)
      if ((i < off || i >= off + n) && mem[i] != 0xA5) return false;
    return true;
  }
};

static void write_file(const std::string& path, const void* p, size_t bytes) {
  FILE* f = fopen(path.c_str(), "wb");
  if (!f || fwrite(p, 1, bytes, f) != bytes) { fprintf(stderr, "emu_inpaint: cannot write %s\n", path.c_str()); exit(2); }
  fclose(f);
}

static void read_exact(FILE* in, void* p, size_t bytes, const std::string& path) {
  if (bytes && fread(p, 1, bytes, in) != bytes) { fprintf(stderr, "emu_inpaint: %s is too short for its case\n", path.c_str()); exit(2); }
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

static int run_grid(const std::string& s) {
  std::string path;
  const std::vector<std::string> f = split(s, 7, &path);
  if (f.size() != 7) { fprintf(stderr, "emu_inpaint: malformed case %s\n", s.c_str()); exit(2); }
  const int Bm = atoi(f[1].c_str()), Hm = atoi(f[2].c_str()), Wm = atoi(f[3].c_str()), gh = atoi(f[4].c_str()), gw = atoi(f[5].c_str());
  const int f32 = atoi(f[6].c_str());
  if (Bm < 1 || Hm < 1 || Wm < 1 || gh < 1 || gw < 1) { fprintf(stderr, "emu_inpaint: %s: bad dimensions\n", s.c_str()); exit(2); }
  const size_t nin = (size_t)Bm * Hm * Wm, nout = (size_t)Bm * gh * gw * (f32 ? 4 : 1);
  Guarded<unsigned char> mask(nin, 0), out(nout, 0);
  FILE* in = fopen(path.c_str(), "rb");
  if (!in) { fprintf(stderr, "emu_inpaint: cannot read %s\n", path.c_str()); exit(2); }
  read_exact(in, mask.p(), nin, path);
  if (fgetc(in) != EOF) { fprintf(stderr, "emu_inpaint: %s is longer than its case\n", path.c_str()); exit(2); }
  fclose(in);
  const int rc = pfd_mask_grid_u8(mask.p(), Bm, Hm, Wm, out.p(), f32, gh, gw, nullptr);
  const bool guards = mask.intact() && out.intact();
  const bool ok = rc == 0 && guards && emu::launch_log.size() == 1;
  printf("%s grid %dx%dx%d -> %dx%d f32 %d  rc %d%s | %s\n", ok ? "ok  " : "FAIL", Bm, Hm, Wm, gh, gw, f32, rc,
         guards ? "" : ", WRITE OUTSIDE A BUFFER", kernel_and_reset().c_str());
  fflush(stdout);
  write_file(path + ".out", out.p(), nout);
  return !ok;
}

static int run_comp(const std::string& s) {
  std::string path;
  const std::vector<std::string> f = split(s, 7, &path);
  if (f.size() != 7) { fprintf(stderr, "emu_inpaint: malformed case %s\n", s.c_str()); exit(2); }
  const int n = atoi(f[1].c_str()), Bi = atoi(f[2].c_str()), Bs = atoi(f[3].c_str()), H = atoi(f[4].c_str()), W = atoi(f[5].c_str());
  const int C = atoi(f[6].c_str());
  if (n < 1 || Bi < 1 || Bs < 1 || H < 1 || W < 1 || C < 1) { fprintf(stderr, "emu_inpaint: %s: bad dimensions\n", s.c_str()); exit(2); }
  const size_t px = (size_t)H * W;
  Guarded<unsigned char> dec(n * px * C, 0), init(Bi * px * C, 0), sel(Bs * px, 0), out(n * px * C, 0);
  FILE* in = fopen(path.c_str(), "rb");
  if (!in) { fprintf(stderr, "emu_inpaint: cannot read %s\n", path.c_str()); exit(2); }
  read_exact(in, dec.p(), n * px * C, path);
  read_exact(in, init.p(), Bi * px * C, path);
  read_exact(in, sel.p(), Bs * px, path);
  if (fgetc(in) != EOF) { fprintf(stderr, "emu_inpaint: %s is longer than its case\n", path.c_str()); exit(2); }
  fclose(in);
  const int rc = pfd_composite_u8(dec.p(), init.p(), Bi, sel.p(), Bs, out.p(), n, H, W, C, nullptr);
  const bool guards = dec.intact() && init.intact() && sel.intact() && out.intact();
  const bool ok = rc == 0 && guards && emu::launch_log.size() == 1;
  printf("%s comp %dx%dx%dx%d Bi %d Bs %d  rc %d%s | %s\n", ok ? "ok  " : "FAIL", n, H, W, C, Bi, Bs, rc,
         guards ? "" : ", WRITE OUTSIDE A BUFFER", kernel_and_reset().c_str());
  fflush(stdout);
  write_file(path + ".out", out.p(), n * px * C);
  return !ok;
}

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: emu_inpaint grid,...|comp,... (see the head of emu_inpaint.cpp)\n"); return 2; }
  int fail = 0;
  for (int a = 1; a < argc; ++a) {
    const std::string s = argv[a];
    if (s.rfind("grid,", 0) == 0) fail += run_grid(s);
    else if (s.rfind("comp,", 0) == 0) fail += run_comp(s);
    else { fprintf(stderr, "emu_inpaint: unknown case %s\n", argv[a]); return 2; }
  }
  return fail != 0;
}
