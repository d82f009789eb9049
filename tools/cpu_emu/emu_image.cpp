// CPU emulation of csrc/image.hip (test infrastructure; see hip/hip_runtime.h in this directory for the execution model): the
// two resampling passes and the fused ToTensor run through the library's own entry points on pictures, tap tables and
// expected bytes that tests/test_image_ingest_cpu.py writes into a directory.  The driver compares the uint8 result with the
// expected bytes itself and leaves every output (uint8, f32 NCHW, f16 NCHW, f16 NHWC) next to the inputs for the test to judge.
//
// usage: emu_image <dir>     <dir>/cases.txt: one line per case, `name h w c oh ow src_offset`;
//   <dir>/<name>.src   uint8 [h][w][c]          <dir>/<name>.exp   uint8 [oh][ow][c] (Pillow's bytes)
//   <dir>/<name>.htaps / .vtaps   int32: ktaps, xmin[out], klen[out], kk[out][ktaps]   (absent: that axis keeps its size)
// src_offset: the picture is placed that many bytes behind a 16-byte boundary (pointer alignment decides the load width).
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

#include "image_emu.inc"

static std::vector<uint8_t> read_file(const std::string& path, bool required = true) {
  std::vector<uint8_t> v;
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) {
    if (required) { fprintf(stderr, "emu_image: cannot read %s\n", path.c_str()); exit(2); }
    return v;
  }
  fseek(f, 0, SEEK_END);
  v.resize((size_t)ftell(f));
  fseek(f, 0, SEEK_SET);
  if (!v.empty() && fread(v.data(), 1, v.size(), f) != v.size()) exit(2);
  fclose(f);
  return v;
}
static void write_file(const std::string& path, const void* p, size_t n) {
  FILE* f = fopen(path.c_str(), "wb");
  if (!f || fwrite(p, 1, n, f) != n) { fprintf(stderr, "emu_image: cannot write %s\n", path.c_str()); exit(2); }
  fclose(f);
}

struct Taps {
  std::vector<uint8_t> raw;
  int ktaps = 0, n = 0;
  const int32_t* xmin() const { return (const int32_t*)raw.data() + 1; }
  const int32_t* klen() const { return xmin() + n; }
  const int32_t* kk() const { return klen() + n; }
  bool load(const std::string& path, int out) {
    raw = read_file(path, false);
    if (raw.empty()) return false;
    n = out;
    ktaps = *(const int32_t*)raw.data();
    if (raw.size() != sizeof(int32_t) * (1 + 2 * (size_t)out + (size_t)out * ktaps)) { fprintf(stderr, "emu_image: %s has the wrong size\n", path.c_str()); exit(2); }
    return true;
  }
};

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
  if (argc < 2) { fprintf(stderr, "usage: emu_image <dir>\n"); return 2; }
  const std::string dir = std::string(argv[1]) + "/";
  FILE* f = fopen((dir + "cases.txt").c_str(), "r");
  if (!f) { fprintf(stderr, "emu_image: no cases.txt in %s\n", argv[1]); return 2; }
  char name[64];
  int h, w, c, oh, ow, soff, fail = 0, total = 0;
  while (fscanf(f, "%63s %d %d %d %d %d %d", name, &h, &w, &c, &oh, &ow, &soff) == 7) {
    const std::string base = dir + name;
    const auto src = read_file(base + ".src"), exp = read_file(base + ".exp");
    const size_t npix = (size_t)oh * ow * c;
    if (src.size() != (size_t)h * w * c || exp.size() != npix) { fprintf(stderr, "emu_image: %s: file sizes do not match the case\n", name); return 2; }
    Taps ht, vt;
    const bool hpass = ht.load(base + ".htaps", ow), vpass = vt.load(base + ".vtaps", oh);
    Guarded in(src.size(), soff), mid((size_t)h * ow * c, soff), u8(npix, 0), f32(npix * 4, 0), f16(npix * 2, 0), nhwc(npix * 2, 0);
    memcpy(in.p(), src.data(), src.size());
    int rc = 0;
    const uint8_t* vsrc = in.p();
    if (hpass) {
      rc |= pfd_image_resample_h_u8(in.p(), mid.p(), 1, h, w, ow, c, ht.kk(), ht.xmin(), ht.klen(), ht.ktaps, nullptr);
      vsrc = mid.p();
    }
    struct { int kind; Guarded* dst; } outs[4] = {{PFD_IMG_U8, &u8}, {PFD_IMG_NCHW_F32, &f32}, {PFD_IMG_NCHW_F16, &f16}, {PFD_IMG_NHWC_F16, &nhwc}};
    for (auto& o : outs)
      rc |= pfd_image_resample_v_u8(vsrc, o.dst->p(), o.kind, 1, h, oh, ow, c, vpass ? vt.kk() : nullptr, vpass ? vt.xmin() : nullptr,
                                    vpass ? vt.klen() : nullptr, vt.ktaps, nullptr);
    size_t nd = 0;
    for (size_t i = 0; i < npix; ++i) nd += u8.p()[i] != exp[i];
    const bool guards = in.intact() && mid.intact() && u8.intact() && f32.intact() && f16.intact() && nhwc.intact();
    const bool ok = rc == 0 && nd == 0 && guards;
    ++total;
    fail += !ok;
    std::string kernels;
    for (auto& k : emu::launched) if (kernels.find(k) == std::string::npos) kernels += (kernels.empty() ? "" : " ") + k;
    emu::launched.clear();
    printf("%s %-14s %dx%dx%d -> %dx%d  rc %d, %zu of %zu bytes differ%s | %s\n", ok ? "ok  " : "FAIL", name, h, w, c, oh, ow, rc, nd, npix,
           guards ? "" : ", WRITE OUTSIDE A BUFFER", kernels.c_str());
    fflush(stdout);
    write_file(base + ".out_u8", u8.p(), npix);
    write_file(base + ".out_f32", f32.p(), npix * 4);
    write_file(base + ".out_f16", f16.p(), npix * 2);
    write_file(base + ".out_nhwc_f16", nhwc.p(), npix * 2);
  }
  fclose(f);
  printf("%d cases, %d failed\n", total, fail);
  return fail || !total;
}
