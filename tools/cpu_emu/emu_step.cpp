// CPU emulation of csrc/step.hip (test infrastructure; see hip/hip_runtime.h in this directory for the execution model): the
// one step kernel runs through any of the library's five entry points, Philox rounds, Box-Muller and all, on cases given on
// the command line.  The driver checks the return code and the guard bands around every tensor, prints one line per case
// (with the instantiated kernel) and leaves the outputs next to the input for the test to judge.
//
// usage: emu_step <case> ...
//   entry,B,Bm,C,h,w,nb,rep,solver,ps,hist,noise,keyed,index,noise_mul,ksq,ks,offset,path
//     entry: ddim | rng | ps | dpmpp | masked (pfd_cfg_ddim_step, _step_rng, _step_ps, pfd_cfg_dpmpp_step, pfd_cfg_step_masked)
//     <path>: int64 [B][2] key rows (keyed), f32 [8] coefficient row, f32 [B] scales (ps), f16 [nb*B][h][w][C] eps, f32 x,
//     f32 noise (noise), f32 x0_prev (hist), and for masked f32 x0_keep, f32 [Bm][h][w] mask
//     written: <path>.xout, <path>.pred (f32 NCHW), <path>.xin (f16 [rep*B][h][w][C])
// Floats are read with strtof (hex floats pass exactly).  offset: the fp32 tensors start that many floats behind a 16-byte
// boundary (0: the 16-byte accesses where w allows them; 1: the scalar path).
#include <stdio.h>
#include <string.h>

#include <string>

#include "hip/hip_runtime.h"


#include "pfd_common.h"
bool pfd_prof_on() { return false; }
void pfd_prof_begin(int, double, double, hipStream_t) {}
void pfd_prof_end(hipStream_t) {}
int pfd_check_launch(const char*) { return 0; }
static std::string g_err;
void pfd_set_error(const char* m) { g_err = m ? m : ""; }

#include "step_emu.inc"

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
  if (!f || fwrite(p, 1, bytes, f) != bytes) { fprintf(stderr, "emu_step: cannot write %s\n", path.c_str()); exit(2); }
  fclose(f);
}

static void read_exact(FILE* in, void* p, size_t bytes, const std::string& path) {
  if (bytes && fread(p, 1, bytes, in) != bytes) { fprintf(stderr, "emu_step: %s is too short for its case\n", path.c_str()); exit(2); }
}

static std::vector<std::string> split(const std::string& s, size_t nfields, std::string* rest) {
  std::vector<std::string> f;
  size_t at = 0;
  for (size_t c; f.size() < nfields && (c = s.find(',', at)) != std::string::npos; at = c + 1) f.push_back(s.substr(at, c - at));
  *rest = s.substr(at);      // the rest, commas included
  return f;
}

static std::string kernel_and_reset() {
  std::string k = emu::launch_log.empty() ? "" : emu::launch_log[0].kernel;
  // the demangler of the host's C++ runtime does not know _Float16 parameters: read the template arguments off the mangled
  // name ("cfg_step_kernelILi0ELb1ELb1ELb0EE" -> "cfg_step_kernel<0, true, true, false>": solver, keyed, masked, 16-byte)
  int solver = 0, keyed = 0, masked = 0, vec = 0;
  const size_t at = k.find("cfg_step_kernelI");
  if (at != std::string::npos && sscanf(k.c_str() + at, "cfg_step_kernelILi%dELb%dELb%dELb%dEE", &solver, &keyed, &masked, &vec) == 4) {
    auto tf = [](int v) { return v ? "true" : "false"; };
    k = "cfg_step_kernel<" + std::to_string(solver) + ", " + tf(keyed) + ", " + tf(masked) + ", " + tf(vec) + ">";
  }
  emu::launched.clear();
  emu::launch_log.clear();
  return k;
}

static int run_case(const std::string& s) {
  std::string path;
  const std::vector<std::string> f = split(s, 18, &path);
  if (f.size() != 18) { fprintf(stderr, "emu_step: malformed case %s\n", s.c_str()); exit(2); }
  auto I = [&](int i) { return atoi(f[i].c_str()); };
  const std::string entry = f[0];
  const int B = I(1), Bm = I(2), C = I(3), h = I(4), w = I(5), nb = I(6), rep = I(7), solver = I(8), ps = I(9), hist = I(10), noise = I(11);
  const int keyed = I(12), index = I(13);
  const float noise_mul = strtof(f[14].c_str(), nullptr), ksq = strtof(f[15].c_str(), nullptr), ks = strtof(f[16].c_str(), nullptr);
  const int offset = I(17);
  const bool masked = entry == "masked";
  if (B < 1 || Bm < 1 || C < 1 || h < 1 || w < 1 || nb < 1 || nb > 2 || rep < 1 || rep > 2) { fprintf(stderr, "emu_step: %s: bad dimensions\n", s.c_str()); exit(2); }
  const size_t n = (size_t)B * C * h * w;
  std::vector<int64_t> key((size_t)B * 2);
  std::vector<float> coef(8), scale(B);
  std::vector<half_t> eps((size_t)nb * n);
  Guarded<float> x(n, offset), nz(n, offset), hprev(n, offset), x0(n, offset), xout(n, offset), pred(n, offset), mask((size_t)Bm * h * w, 0);
  Guarded<half_t> xin((size_t)rep * n, 0);
  FILE* in = fopen(path.c_str(), "rb");
  if (!in) { fprintf(stderr, "emu_step: cannot read %s\n", path.c_str()); exit(2); }
  if (keyed) read_exact(in, key.data(), key.size() * 8, path);
  read_exact(in, coef.data(), 32, path);
  if (ps) read_exact(in, scale.data(), (size_t)B * 4, path);
  read_exact(in, eps.data(), eps.size() * 2, path);
  read_exact(in, x.p(), n * 4, path);
  if (noise) read_exact(in, nz.p(), n * 4, path);
  if (hist) read_exact(in, hprev.p(), n * 4, path);
  if (masked) {
    read_exact(in, x0.p(), n * 4, path);
    read_exact(in, mask.p(), (size_t)Bm * h * w * 4, path);
  }
  if (fgetc(in) != EOF) { fprintf(stderr, "emu_step: %s is longer than its case\n", path.c_str()); exit(2); }
  fclose(in);
  const float* sc = ps ? scale.data() : nullptr;
  const float* nzp = noise ? nz.p() : nullptr;
  const float* hp = hist ? hprev.p() : nullptr;
  const int64_t* kp = keyed ? key.data() : nullptr;
  int rc;
  if (entry == "ddim")
    rc = pfd_cfg_ddim_step(eps.data(), nb, x.p(), nzp, coef.data(), xout.p(), pred.p(), xin.p(), rep, B, C, h, w, nullptr);
  else if (entry == "rng")
    rc = pfd_cfg_ddim_step_rng(eps.data(), nb, x.p(), kp, index, noise_mul, coef.data(), xout.p(), pred.p(), xin.p(), rep, B, C, h, w, nullptr);
  else if (entry == "ps")
    rc = pfd_cfg_ddim_step_ps(eps.data(), nb, x.p(), nzp, kp, index, noise_mul, coef.data(), sc, xout.p(), pred.p(), xin.p(), rep, B, C, h, w, nullptr);
  else if (entry == "dpmpp")
    rc = pfd_cfg_dpmpp_step(eps.data(), nb, x.p(), hp, coef.data(), sc, xout.p(), pred.p(), xin.p(), rep, B, C, h, w, nullptr);
  else if (masked)
    rc = pfd_cfg_step_masked(eps.data(), nb, x.p(), solver, hp, kp, index, noise_mul, coef.data(), sc, x0.p(), mask.p(), Bm, ksq, ks,
                             xout.p(), pred.p(), xin.p(), rep, B, C, h, w, nullptr);
  else { fprintf(stderr, "emu_step: unknown entry point %s\n", entry.c_str()); exit(2); }
  const bool guards = x.intact() && nz.intact() && hprev.intact() && x0.intact() && xout.intact() && pred.intact() && mask.intact() && xin.intact();
  const bool ok = rc == 0 && guards && emu::launch_log.size() == 1;
  printf("%s %s %dx%dx%dx%d Bm %d nb %d rep %d solver %d offset %d  rc %d launches %d%s | %s\n", ok ? "ok  " : "FAIL", entry.c_str(), B, C,
         h, w, Bm, nb, rep, solver, offset, rc, (int)emu::launch_log.size(), guards ? "" : ", WRITE OUTSIDE A BUFFER", kernel_and_reset().c_str());
  fflush(stdout);
  write_file(path + ".xout", xout.p(), n * 4);
  write_file(path + ".pred", pred.p(), n * 4);
  write_file(path + ".xin", xin.p(), (size_t)rep * n * 2);
  return !ok;
}

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: emu_step entry,... (see the head of emu_step.cpp)\n"); return 2; }
  int fail = 0;
  for (int a = 1; a < argc; ++a) fail += run_case(argv[a]);
  return fail != 0;
}
