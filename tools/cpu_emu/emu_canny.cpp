// CPU emulation of csrc/canny.hip (test infrastructure; see hip/hip_runtime.h in this directory for the execution model): the
// four kernels run through the library's own entry point on pictures that tests/test_canny_cpu.py writes into a directory.
// The 256 threads of a block are OS threads, so the union-find of the link kernel really runs concurrently (blocks follow
// one another).  The driver checks the return code and the guard bands around every buffer and leaves the state bytes and
// every output (uint8, f16 hint, f32 hint) next to the inputs for the test to judge.
//
// usage: emu_canny <dir>     <dir>/cases.txt: one line per case, `name b h w c low high src_offset forms`;
//   <dir>/<name>.src   uint8 [b][h][w][c]
// src_offset: the picture is placed that many bytes behind a 16-byte boundary.  forms: 1 = the uint8 output only,
// 3 = the two hint forms as well (each form is one more call).
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

#include "canny_emu.inc"

static std::vector<uint8_t> read_file(const std::string& path) {
  std::vector<uint8_t> v;
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) { fprintf(stderr, "emu_canny: cannot read %s\n", path.c_str()); exit(2); }
  fseek(f, 0, SEEK_END);
  v.resize((size_t)ftell(f));
  fseek(f, 0, SEEK_SET);
  if (!v.empty() && fread(v.data(), 1, v.size(), f) != v.size()) exit(2);
  fclose(f);
  return v;
}
static void write_file(const std::string& path, const void* p, size_t n) {
  FILE* f = fopen(path.c_str(), "wb");
  if (!f || fwrite(p, 1, n, f) != n) { fprintf(stderr, "emu_canny: cannot write %s\n", path.c_str()); exit(2); }
  fclose(f);
}

// a buffer whose payload starts `offset` bytes behind a 16-byte boundary, with a guard band on both sides
struct Guarded {
  std::vector<uint8_t> mem;
  size_t off, n;
  Guarded(size_t bytes, int offset) : mem(bytes + 96, 0xA5), n(bytes) {
    off = 32;
    while (((uintptr_t)(mem.data() + off) & 15) != (uintptr_t)offset) ++off;
  }
  uint8_t* p() { return mem.data() + off; }
  bool intact() const {
    for (size_t i = 0; i < off; ++i) if (mem[i] != 0xA5) return false;
    for (size_t i = off + n; i < mem.size(); ++i) if (mem[i] != 0xA5) return false;
    return true;
  }
};

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: emu_canny <dir>\n"); return 2; }
  const std::string dir = std::string(argv[1]) + "/";
  FILE* f = fopen((dir + "cases.txt").c_str(), "r");
  if (!f) { fprintf(stderr, "emu_canny: no cases.txt in %s\n", argv[1]); return 2; }
  char name[64];
  int b, h, w, c, low, high, soff, forms, fail = 0, total = 0;
  while (fscanf(f, "%63s %d %d %d %d %d %d %d %d", name, &b, &h, &w, &c, &low, &high, &soff, &forms) == 9) {
    const std::string base = dir + name;
    const auto src = read_file(base + ".src");
    const size_t npix = (size_t)b * h * w;
    if (src.size() != npix * c) { fprintf(stderr, "emu_canny: %s: file size does not match the case\n", name); return 2; }
    Guarded in(src.size(), soff), states(npix, 0), parent(npix * 4, 0), strong(npix, 0), u8(npix, 0), f16(npix * 6, 0), f32(npix * 12, 0);
    memcpy(in.p(), src.data(), src.size());
    int rc = pfd_canny_u8(in.p(), b, h, w, c, low, high, states.p(), parent.p(), strong.p(), u8.p(), PFD_IMG_U8, nullptr);
    write_file(base + ".states", states.p(), npix);
    if (forms & 2) {
      rc |= pfd_canny_u8(in.p(), b, h, w, c, low, high, states.p(), parent.p(), strong.p(), f16.p(), PFD_IMG_NCHW_F16, nullptr);
      rc |= pfd_canny_u8(in.p(), b, h, w, c, low, high, states.p(), parent.p(), strong.p(), f32.p(), PFD_IMG_NCHW_F32, nullptr);
    }
    const bool guards = in.intact() && states.intact() && parent.intact() && strong.intact() && u8.intact() && f16.intact() && f32.intact();
    const bool ok = rc == 0 && guards;
    ++total;
    fail += !ok;
    std::string kernels;
    for (auto& k : emu::launched) if (kernels.find(k) == std::string::npos) kernels += (kernels.empty() ? "" : " ") + k;
    const size_t launches = emu::launched.size();
    emu::launched.clear();
    printf("%s %-22s %dx%dx%dx%d (%d, %d)  rc %d, %zu launches%s | %s\n", ok ? "ok  " : "FAIL", name, b, h, w, c, low, high, rc, launches,
           guards ? "" : ", WRITE OUTSIDE A BUFFER", kernels.c_str());
    fflush(stdout);
    write_file(base + ".out_u8", u8.p(), npix);
    if (forms & 2) {
      write_file(base + ".out_f16", f16.p(), npix * 6);
      write_file(base + ".out_f32", f32.p(), npix * 12);
    }
  }
  fclose(f);
  printf("%d cases, %d failed\n", total, fail);
  return fail || !total;
}
