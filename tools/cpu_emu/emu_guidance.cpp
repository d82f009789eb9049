// CPU emulation of csrc/guidance.hip and of pfd_cfg_step_mul in csrc/step.hip (test infrastructure; see hip/hip_runtime.h in
// this directory for the execution model): both run through the library's own entry points on cases given on the command
// line.  The driver checks the return code against the one the case expects and the guard bands around every tensor,
// prints one line per case (with the kernel launched) and leaves the outputs next to the input for the test to judge
// against lib/guidance.py and tests/golden/step_bits.npz.
//
// usage: emu_guidance <case> ...
//   stats,B,n,sstride,pstride,offset,null,rc,path
//       <path>: f16 eps [2B][n], f32 scale [(B-1)*sstride + 1], f32 phi [(B-1)*pstride + 1];  offset: eps starts that many
//       halves behind a 16-byte boundary;  null: a bit per pointer passed as NULL (1 eps, 2 scale, 4 phi, 8 mul);  rc: the
//       return code expected (0: one launch);  written: <path>.mul (f32 [B]; untouched 0xA5 bytes where rc != 0)
//   step,rc,<a case of emu_step: entry,B,Bm,C,h,w,nb,rep,solver,ps,hist,noise,keyed,index,noise_mul,ksq,ks,offset,path>
//       the inputs of that case in emu_step's layout in <path>, the factors f32 [B] in <path>.mulin (no such file: eps_mul
//       is NULL); the case runs through pfd_cfg_step_mul with the pointers its entry point would get;
//       written: <path>.xout, <path>.pred, <path>.xin as emu_step writes them
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
#include "guidance_emu.inc"

// a buffer whose payload starts `offset` bytes behind a 16-byte boundary, with a guard band on both sides
struct Guarded {
  std::vector<unsigned char> mem;
  size_t off, n;
  Guarded(size_t bytes, int offset) : mem(bytes + 160, 0xA5), n(bytes) {
    off = 48;
    while (((uintptr_t)(mem.data() + off) & 15) != (uintptr_t)(offset & 15)) ++off;
  }
  unsigned char* p() { return mem.data() + off; }
  float* f() { return reinterpret_cast<float*>(p()); }
  bool intact() const {
    for (size_t i = 0; i < mem.size(); ++i)
      if ((i < off || i >= off + n) && mem[i] != 0xA5) return false;
    return true;
  }
};

static void write_file(const std::string& path, const void* p, size_t bytes) {
  FILE* f = fopen(path.c_str(), "wb");
  if (!f || fwrite(p, 1, bytes, f) != bytes) { fprintf(stderr, "emu_guidance: cannot write %s\n", path.c_str()); exit(2); }
  fclose(f);
}

static void read_exact(FILE* in, void* p, size_t bytes, const std::string& path) {
  if (bytes && fread(p, 1, bytes, in) != bytes) { fprintf(stderr, "emu_guidance: %s is too short for its case\n", path.c_str()); exit(2); }
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
  // (the host's demangler does not know _Float16 parameters: read the template arguments off the mangled name, as emu_step does)
  int solver = 0, keyed = 0, masked = 0, vec = 0;
  size_t at = k.find("cfg_step_kernelI");
  auto tf = [](int v) { return v ? "true" : "false"; };
  if (at != std::string::npos && sscanf(k.c_str() + at, "cfg_step_kernelILi%dELb%dELb%dELb%dEE", &solver, &keyed, &masked, &vec) == 4)
    k = "cfg_step_kernel<" + std::to_string(solver) + ", " + tf(keyed) + ", " + tf(masked) + ", " + tf(vec) + ">";
  at = k.find("guidance_rescale_kernelI");
  if (at != std::string::npos && sscanf(k.c_str() + at, "guidance_rescale_kernelILb%dEE", &vec) == 1)
    k = std::string("guidance_rescale_kernel<") + tf(vec) + ">";
  emu::launched.clear();
  emu::launch_log.clear();
  return k;
}

static int run_stats(const std::string& s) {
  std::string path;
  const std::vector<std::string> f = split(s, 8, &path);
  if (f.size() != 8) { fprintf(stderr, "emu_guidance: malformed case %s\n", s.c_str()); exit(2); }
  auto I = [&](int i) { return atoi(f[i].c_str()); };
  const int B = I(1), ss = I(3), ps = I(4), offset = I(5), null = I(6), want = I(7);
  const long n = atol(f[2].c_str());
  // (a case that must be refused may carry B, n or a stride <= 0: the buffers then hold one sample of one element)
  const size_t Bb = B > 0 ? B : 1, nn = n > 0 ? n : 1;
  const size_t nsc = (Bb - 1) * (ss > 0 ? ss : 0) + 1, nph = (Bb - 1) * (ps > 0 ? ps : 0) + 1;
  Guarded eps(2 * Bb * nn * 2, offset * 2), sc(nsc * 4, 0), ph(nph * 4, 0), mul(Bb * 4, 0);
  FILE* in = fopen(path.c_str(), "rb");
  if (!in) { fprintf(stderr, "emu_guidance: cannot read %s\n", path.c_str()); exit(2); }
  read_exact(in, eps.p(), eps.n, path);
  read_exact(in, sc.p(), sc.n, path);
  read_exact(in, ph.p(), ph.n, path);
  if (fgetc(in) != EOF) { fprintf(stderr, "emu_guidance: %s is longer than its case\n", path.c_str()); exit(2); }
  fclose(in);
  std::vector<unsigned char> mul_before(mul.p(), mul.p() + mul.n);
  const int rc = pfd_guidance_rescale_f32(null & 1 ? nullptr : eps.p(), null & 2 ? nullptr : sc.f(), ss, null & 4 ? nullptr : ph.f(), ps,
                                          null & 8 ? nullptr : mul.f(), B, n, nullptr);
  const bool guards = eps.intact() && sc.intact() && ph.intact() && mul.intact();
  const bool untouched = rc == 0 || !memcmp(mul_before.data(), mul.p(), mul.n);
  const bool ok = rc == want && guards && untouched && emu::launch_log.size() == (rc == 0 ? 1u : 0u);
  printf("%s stats B %d n %ld strides %d %d offset %d null %d  rc %d (expected %d)%s | %s\n", ok ? "ok  " : "FAIL", B, n, ss, ps, offset,
         null, rc, want, guards ? "" : ", WRITE OUTSIDE A BUFFER", kernel_and_reset().c_str());
  fflush(stdout);
  write_file(path + ".mul", mul.p(), mul.n);
  return !ok;
}

static int run_step(const std::string& s) {
  std::string path;
  const std::vector<std::string> f = split(s, 20, &path);
  if (f.size() != 20) { fprintf(stderr, "emu_guidance: malformed case %s\n", s.c_str()); exit(2); }
  auto I = [&](int i) { return atoi(f[i].c_str()); };
  const int want = I(1);
  const std::string entry = f[2];
  const int B = I(3), Bm = I(4), C = I(5), h = I(6), w = I(7), nb = I(8), rep = I(9), solver = I(10), ps = I(11), hist = I(12), noise = I(13);
  const int keyed = I(14), index = I(15);
  const float noise_mul = strtof(f[16].c_str(), nullptr), ksq = strtof(f[17].c_str(), nullptr), ks = strtof(f[18].c_str(), nullptr);
  const int offset = I(19);
  const bool masked = entry == "masked";
  if (B < 1 || Bm < 1 || C < 1 || h < 1 || w < 1 || nb < 1 || nb > 2 || rep < 1 || rep > 2) { fprintf(stderr, "emu_guidance: %s: bad dimensions\n", s.c_str()); exit(2); }
  const size_t n = (size_t)B * C * h * w;
  std::vector<int64_t> key((size_t)B * 2);
  std::vector<float> coef(8), scale(B);
  std::vector<half_t> eps((size_t)nb * n);
  const int ob = (offset & 3) * 4;
  Guarded x(n * 4, ob), nz(n * 4, ob), hprev(n * 4, ob), x0(n * 4, ob), xout(n * 4, ob), pred(n * 4, ob), mask((size_t)Bm * h * w * 4, 0);
  Guarded xin((size_t)rep * n * 2, 0), mulin((size_t)B * 4, 0);
  FILE* in = fopen(path.c_str(), "rb");
  if (!in) { fprintf(stderr, "emu_guidance: cannot read %s\n", path.c_str()); exit(2); }
  if (keyed) read_exact(in, key.data(), key.size() * 8, path);
  read_exact(in, coef.data(), 32, path);
  if (ps) read_exact(in, scale.data(), (size_t)B * 4, path);
  read_exact(in, eps.data(), eps.size() * 2, path);
  read_exact(in, x.p(), n * 4, path);
  if (noise) read_exact(in, nz.p(), n * 4, path);
  if (hist) read_exact(in, hprev.p(), n * 4, path);
  if (masked) {
    read_exact(in, x0.p(), n * 4, path);
    read_exact(in, mask.p(), mask.n, path);
  }
  if (fgetc(in) != EOF) { fprintf(stderr, "emu_guidance: %s is longer than its case\n", path.c_str()); exit(2); }
  fclose(in);
  const float* mp = nullptr;
  if (FILE* m = fopen((path + ".mulin").c_str(), "rb")) {
    read_exact(m, mulin.p(), mulin.n, path + ".mulin");
    fclose(m);
    mp = mulin.f();
  }
  const int rc = pfd_cfg_step_mul(eps.data(), nb, x.f(), solver, noise ? nz.f() : nullptr, hist ? hprev.f() : nullptr,
                                  keyed ? key.data() : nullptr, index, noise_mul, coef.data(), ps ? scale.data() : nullptr, mp,
                                  masked ? x0.f() : nullptr, masked ? mask.f() : nullptr, masked ? Bm : 0, ksq, ks, xout.f(), pred.f(),
                                  xin.p(), rep, B, C, h, w, nullptr);
  const bool guards = x.intact() && nz.intact() && hprev.intact() && x0.intact() && xout.intact() && pred.intact() && mask.intact() &&
                      xin.intact() && mulin.intact();
  const bool ok = rc == want && guards && emu::launch_log.size() == (rc == 0 ? 1u : 0u);
  printf("%s step %s %dx%dx%dx%d Bm %d nb %d rep %d solver %d offset %d  rc %d (expected %d) launches %d%s | %s\n", ok ? "ok  " : "FAIL",
         entry.c_str(), B, C, h, w, Bm, nb, rep, solver, offset, rc, want, (int)emu::launch_log.size(), guards ? "" : ", WRITE OUTSIDE A BUFFER",
         kernel_and_reset().c_str());
  fflush(stdout);
  write_file(path + ".xout", xout.p(), n * 4);
  write_file(path + ".pred", pred.p(), n * 4);
  write_file(path + ".xin", xin.p(), (size_t)rep * n * 2);
  return !ok;
}

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: emu_guidance stats,...|step,... (see the head of emu_guidance.cpp)\n"); return 2; }
  int fail = 0;
  for (int a = 1; a < argc; ++a) {
    const std::string s = argv[a];
    if (s.rfind("stats,", 0) == 0) fail += run_stats(s);
    else if (s.rfind("step,", 0) == 0) fail += run_step(s);
    else { fprintf(stderr, "emu_guidance: unknown case %s\n", argv[a]); return 2; }
  }
  return fail != 0;
}
