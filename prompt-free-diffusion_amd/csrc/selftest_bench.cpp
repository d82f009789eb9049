// The timed runs of build/selftest (modes: selftest.cpp): UNet- / VAE-shaped problems and the runtime's launch floor.
#include <functional>

#include "selftest_util.h"

static float time_ms(const std::function<void()>& f, int iters) {
  hipEvent_t a, b;
  HIP_OK(hipEventCreate(&a)); HIP_OK(hipEventCreate(&b));
  for (int i = 0; i < 3; ++i) f();
  HIP_OK(hipEventRecord(a, 0));
  for (int i = 0; i < iters; ++i) f();
  HIP_OK(hipEventRecord(b, 0));
  HIP_OK(hipEventSynchronize(b));
  float ms = 0;
  HIP_OK(hipEventElapsedTime(&ms, a, b));
  return ms / iters;
}

// ksize: 0 = a linear layer, 3 = a 3x3 / stride 1 / pad 1 convolution over B square H x H images
void bench_gemm(const char* label, int M, int N, int K, int ksize, int B, int H, int Cin, int tile) {
  const bool conv = ksize > 0;
  if (conv) { M = B * H * H; K = ksize * ksize * Cin; }
  auto A = rand_h(conv ? (size_t)B * H * H * Cin : (size_t)M * K), W = rand_h((size_t)N * K, 0.05f), bias = rand_h(N);
  Dev<h16> dA(A), dW(W), dB(bias), dC((size_t)M * N);
  Dev<float> dWS((size_t)16 << 20);
  PfdGemmDesc d = gemm_desc(dWS);
  d.A = dA.p; d.W = dW.p; d.bias = dB.p; d.C = dC.p;
  d.lda = conv ? Cin : K; d.ldw = K; d.ldc = N; d.M = M; d.N = N; d.K = K; d.rows_per_rv = 1;
  if (conv) conv3x3_geometry(d, B, H, H, Cin);
  int rc = 0;
  const float ms = time_ms([&] { rc |= pfd_gemm_f16_ex(&d, tile, nullptr); }, 20);
  const double tf = 2.0 * M * N * K / (ms * 1e-3) / 1e12;
  printf("bench %-34s M%-6d N%-5d K%-6d tile%-2d rc=%d %8.3f ms %8.1f TFLOP/s\n", label, M, N, K, tile, rc, ms, tf);
  fflush(stdout);
}

static void bench_gn_conv(const char* label, int B, int H, int C1, int C2, int N) {
  const int C = C1 + C2, HW = H * H, M = B * HW, K = 9 * C, G = 32;
  auto x1 = rand_h((size_t)M * C1), x2 = rand_h((size_t)M * std::max(C2, 8)), gm = rand_h(C), bt = rand_h(C);
  auto Wt = rand_h((size_t)N * K, 0.05f), bias = rand_h(N);
  Dev<h16> d1(x1), d2(x2), dg(gm), db(bt), dy((size_t)M * C), dW(Wt), dB(bias), dC((size_t)M * N);
  Dev<float> dT((size_t)B * C * 2);
  const size_t wsb = pfd_groupnorm_ws_bytes(B, C, HW);
  Dev<char> dws(wsb);
  PfdGemmDesc d = gemm_desc(Dev<float>());   // no workspace
  d.W = dW.p; d.bias = dB.p; d.C = dC.p; d.ldw = K; d.ldc = N; d.M = M; d.N = N; d.K = K; d.rows_per_rv = 1;
  conv3x3_geometry(d, B, H, H, C);
  int rc = 0;
  auto norm = [&] { rc |= pfd_groupnorm_f16(d1.p, C1, C1, C2 ? d2.p : nullptr, C2, C2, dg.p, db.p, dy.p, C, B, HW, G, 1e-5f, PFD_ACT_SILU, dws.p, wsb, nullptr); };
  auto table = [&] { rc |= pfd_groupnorm_table_f16(d1.p, C1, C1, C2 ? d2.p : nullptr, C2, C2, dg.p, db.p, dT.p, B, HW, G, 1e-5f, dws.p, wsb, nullptr); };
  auto launch = [&] { rc |= pfd_gemm_f16(&d, nullptr); };
  d.A = dy.p; d.lda = C;
  const float gn = time_ms(norm, 20);
  const float conv = time_ms(launch, 20);
  const float two = time_ms([&] { norm(); launch(); }, 20);
  d.A = d1.p; d.lda = C1; d.A2 = C2 ? d2.p : nullptr; d.lda2 = C2; d.gn_c1 = C1; d.gn_table = dT.p; d.gn_act = PFD_ACT_SILU;
  const float tab = time_ms(table, 20);
  const float pconv = time_ms(launch, 20);
  const float fused = time_ms([&] { table(); launch(); }, 20);
  printf("bench gn+conv %-30s rc=%d  groupnorm %.1f + conv %.1f = %.1f us | table %.1f + prologue conv %.1f = %.1f us\n",
         label, rc, gn * 1e3, conv * 1e3, two * 1e3, tab * 1e3, pconv * 1e3, fused * 1e3);
}

void bench_attn(const char* label, int B, int H, int Nq, int Nk, int D) {
  const int C = H * D, Nkp = (Nk + 7) / 8 * 8;
  auto Q = rand_h((size_t)B * Nq * C), K = rand_h((size_t)B * Nk * C), Vt = rand_h((size_t)C * B * Nkp);
  Dev<h16> dQ(Q), dK(K), dV(Vt), dO((size_t)B * Nq * C);
  PfdAttnDesc d;
  memset(&d, 0, sizeof(d));
  d.Q = dQ.p; d.K = dK.p; d.Vt = dV.p; d.O = dO.p;
  d.ldq = C; d.ldk = C; d.ldvt = (long)B * Nkp; d.ldo = C;
  d.q_bs = (long)Nq * C; d.k_bs = (long)Nk * C; d.vt_bs = Nkp; d.o_bs = (long)Nq * C;
  d.B = B; d.H = H; d.Nq = Nq; d.Nk = Nk; d.D = D; d.scale = 1.f / sqrtf((float)D);
  int rc = 0;
  const float ms = time_ms([&] { rc |= pfd_attention_f16(&d, nullptr); }, 20);
  const double tf = 4.0 * B * H * (double)Nq * Nk * D / (ms * 1e-3) / 1e12;
  printf("bench %-34s B%d H%d Nq%d Nk%d D%d rc=%d %8.3f ms %8.1f TFLOP/s\n", label, B, H, Nq, Nk, D, rc, ms, tf);
  fflush(stdout);
}

static void bench_gn(const char* label, int B, int HW, int C) {
  auto x = rand_h((size_t)B * HW * C), g = rand_h(C), bt = rand_h(C);
  Dev<h16> dx(x), dg(g), db(bt), dy((size_t)B * HW * C);
  const size_t wsb = pfd_groupnorm_ws_bytes(B, C, HW);
  Dev<char> dws(wsb);
  int rc = 0;
  const float ms = time_ms([&] { rc |= pfd_groupnorm_f16(dx.p, C, C, nullptr, 0, 0, dg.p, db.p, dy.p, C, B, HW, 32, 1e-5f, PFD_ACT_SILU, dws.p, wsb, nullptr); }, 20);
  const double gbs = 6.0 * B * HW * C / (ms * 1e-3) / 1e9;
  printf("bench %-34s B%d HW%d C%d rc=%d %8.3f ms %8.1f GB/s (6 B/elem)\n", label, B, HW, C, rc, ms, gbs);
  fflush(stdout);
}

static void bench_ln(const char* label, int M, int C) {
  auto x = rand_h((size_t)M * C), g = rand_h(C), b = rand_h(C);
  Dev<h16> dx(x), dg(g), db(b), dy((size_t)M * C);
  int rc = 0;
  const float ms = time_ms([&] { rc |= pfd_layernorm_f16(dx.p, C, dg.p, db.p, dy.p, C, M, C, 1e-5f, 0, 0, 0, 0, nullptr); }, 20);
  printf("bench %-34s M%d C%d rc=%d %8.3f ms %8.1f GB/s (4 B/elem)\n", label, M, C, rc, ms, 4.0 * M * C / (ms * 1e-3) / 1e9);
  fflush(stdout);
}

// Per-launch floor of the runtime: N dependent launches of a kernel with ~no work, in-stream and as one
// hipGraph -- what every one of the ~500 launches of a UNet pass pays on top of its own duration.
int bench_launch_floor(int, char**) {
  Dev<h16> a(std::vector<h16>(4096)), b(std::vector<h16>(4096)), c(4096);
  const int N = 2000;
  hipStream_t st;
  HIP_OK(hipStreamCreate(&st));
  hipEvent_t e0, e1;
  HIP_OK(hipEventCreate(&e0)); HIP_OK(hipEventCreate(&e1));
  auto run = [&] { for (int i = 0; i < N; ++i) pfd_add_f16(a.p, b.p, c.p, 4096, st); };
  run();
  HIP_OK(hipStreamSynchronize(st));
  HIP_OK(hipEventRecord(e0, st)); run(); HIP_OK(hipEventRecord(e1, st));
  HIP_OK(hipEventSynchronize(e1));
  float ms = 0;
  HIP_OK(hipEventElapsedTime(&ms, e0, e1));
  printf("bench launch floor: in-stream      %6.2f us/launch (%d dependent tiny launches)\n", ms * 1e3 / N, N);
  hipGraph_t g; hipGraphExec_t ge;
  HIP_OK(hipStreamBeginCapture(st, hipStreamCaptureModeGlobal));
  run();
  HIP_OK(hipStreamEndCapture(st, &g));
  HIP_OK(hipGraphInstantiate(&ge, g, nullptr, nullptr, 0));
  HIP_OK(hipGraphLaunch(ge, st));
  HIP_OK(hipStreamSynchronize(st));
  HIP_OK(hipEventRecord(e0, st)); HIP_OK(hipGraphLaunch(ge, st)); HIP_OK(hipEventRecord(e1, st));
  HIP_OK(hipEventSynchronize(e1));
  HIP_OK(hipEventElapsedTime(&ms, e0, e1));
  printf("bench launch floor: hipGraph replay %6.2f us/launch\n", ms * 1e3 / N);
  HIP_OK(hipGraphExecDestroy(ge)); HIP_OK(hipGraphDestroy(g)); HIP_OK(hipStreamDestroy(st));
  fflush(stdout);
  return 0;
}

// ------------------------------------------------------------------ the bench lists
int bench_patch(int, char**) {   // one 3x3 conv per image width the patch kernel serves
  bench_gemm("conv3x3 320->320 @64^2", 0, 320, 0, 3, 8, 64, 320, 0);
  bench_gemm("conv3x3 640->640 @32^2", 0, 640, 0, 3, 8, 32, 640, 0);
  bench_gemm("conv3x3 1280->1280 @16^2", 0, 1280, 0, 3, 8, 16, 1280, 0);
  bench_gemm("conv3x3 320->320 @64^2 implicit GEMM", 0, 320, 0, 3, 8, 64, 320, 5400);
  return 0;
}

int bench_gn_conv_list(int, char**) {   // GroupNorm + conv: two launches + a tensor vs table + prologue
  bench_gn_conv("320->320 @64^2", 16, 64, 320, 0, 320);
  bench_gn_conv("640->320 @64^2 (skip concat)", 16, 64, 320, 320, 320);
  bench_gn_conv("960->320 @64^2 (skip concat)", 16, 64, 640, 320, 320);
  bench_gn_conv("640->640 @32^2", 16, 32, 640, 0, 640);
  bench_gn_conv("1280->640 @32^2 (skip concat)", 16, 32, 640, 640, 640);
  bench_gn_conv("1920->640 @32^2 (skip concat)", 16, 32, 1280, 640, 640);
  return 0;
}

int bench_attn_list(int, char**) {
  bench_attn("self-attn 64^2 d40", 8, 8, 4096, 4096, 40);
  bench_attn("self-attn 64^2 d40 (CFG prefix)", 4, 8, 4096, 4096, 40);
  bench_attn("self-attn 96^2 d40 (C5)", 4, 8, 9216, 9216, 40);
  bench_attn("self-attn 32^2 d80", 8, 8, 1024, 1024, 80);
  bench_attn("self-attn 16^2 d160", 8, 8, 256, 256, 160);
  bench_attn("cross-attn 64^2 d40", 4, 8, 4096, 148, 40);
  bench_attn("seecoder cross d96", 1, 8, 144, 4096, 96);
  // fixed cost of the short launches: the same problems with fewer keys
  bench_attn("cross-attn 64^2 d40, 64 keys", 4, 8, 4096, 64, 40);
  bench_attn("cross-attn 64^2 d40, 8 keys", 4, 8, 4096, 8, 40);
  bench_attn("cross-attn 32^2 d80", 4, 8, 1024, 148, 80);
  bench_attn("cross-attn 32^2 d80, 8 keys", 4, 8, 1024, 8, 80);
  bench_attn("cross-attn 16^2 d160", 4, 8, 256, 148, 160);
  bench_attn("cross-attn 16^2 d160, 8 keys", 4, 8, 256, 8, 160);
  bench_attn("self-attn 16^2 d160, 64 keys", 8, 8, 256, 64, 160);
  return 0;
}

int bench_gn_list(int, char**) {
  bench_gn("groupnorm+silu 320 @64^2", 8, 4096, 320);
  bench_gn("groupnorm+silu 640 @64^2", 8, 4096, 640);
  bench_gn("groupnorm+silu 640 @32^2", 8, 1024, 640);
  bench_gn("groupnorm+silu 1280 @32^2", 8, 1024, 1280);
  bench_gn("groupnorm+silu 1280 @16^2", 8, 256, 1280);
  bench_gn("groupnorm+silu 2560 @16^2", 8, 256, 2560);
  bench_gn("groupnorm+silu 1280 @8^2", 8, 64, 1280);
  bench_gn("groupnorm+silu 128 @512^2", 4, 262144, 128);
  bench_ln("layernorm 320 @64^2", 32768, 320);
  bench_ln("layernorm 640 @32^2", 8192, 640);
  bench_ln("layernorm 1280 @16^2", 2048, 1280);
  return 0;
}

int bench_unet_list(int, char**) {
  // UNet-shaped problems at C2 (UNet batch 8)
  for (int t : {5400, 10900, 5400, 10900}) {   // gather conv vs patch conv
    bench_gemm("PATCH conv3x3 320->320 @64^2", 0, 320, 0, 3, 8, 64, 320, t);
    bench_gemm("PATCH conv3x3 960->320 @64^2", 0, 320, 0, 3, 8, 64, 960, t);
    bench_gemm("PATCH conv3x3 640->640 @32^2", 0, 640, 0, 3, 8, 32, 640, t == 5400 ? 5402 : t);
    bench_gemm("PATCH conv3x3 1280->1280 @16^2", 0, 1280, 0, 3, 8, 16, 1280, t == 5400 ? 3404 : t);
  }
  for (int t : {5400, 3400}) {
    bench_gemm("conv3x3 320->320 @64^2", 0, 320, 0, 3, 8, 64, 320, t);
    bench_gemm("linear qkv 320->960 @64^2", 32768, 960, 320, 0, 0, 0, 0, t);
    bench_gemm("linear 1280->320 @64^2", 32768, 320, 1280, 0, 0, 0, 0, t);
    bench_gemm("conv3x3 640->640 @32^2", 0, 640, 0, 3, 8, 32, 640, t);
  }
  for (int t : {5400, 5402, 5403, 3402, 0}) bench_gemm("conv3x3 640->640 @32^2", 0, 640, 0, 3, 8, 32, 640, t);
  for (int t : {5400, 5402, 0}) bench_gemm("conv3x3 1920->640 @32^2", 0, 640, 0, 3, 8, 32, 1920, t);
  for (int t : {3400, 3200, 3402, 3404, 3202, 0}) bench_gemm("conv3x3 1280->1280 @16^2", 0, 1280, 0, 3, 8, 16, 1280, t);
  for (int t : {3200, 3204, 3208, 3404, 3408, 0}) bench_gemm("conv3x3 1280->1280 @8^2", 0, 1280, 0, 3, 8, 8, 1280, t);
  for (int t : {5400, 3400, 0}) bench_gemm("linear qkv 320->960 @64^2", 32768, 960, 320, 0, 0, 0, 0, t);
  for (int t : {5400, 3400, 0}) bench_gemm("linear 1280->320 @64^2", 32768, 320, 1280, 0, 0, 0, 0, t);
  for (int t : {5400, 3400, 0}) bench_gemm("linear 320->2560 @64^2", 32768, 2560, 320, 0, 0, 0, 0, t);
  for (int t : {5400, 3400, 3200, 0}) bench_gemm("linear 1280->10240 @16^2", 2048, 10240, 1280, 0, 0, 0, 0, t);
  bench_gemm("square-ish 8192x5120x4096", 8192, 5120, 4096, 0, 0, 0, 0, 5400);
  for (int t : {22, 21}) {
    bench_gemm("conv3x3 640->640 @32^2", 0, 640, 0, 3, 8, 32, 640, t);
    bench_gemm("conv3x3 1280->1280 @16^2", 0, 1280, 0, 3, 8, 16, 1280, t);
  }
  for (int t : {22, 21, 12, 11}) bench_gemm("conv3x3 1280->1280 @8^2", 0, 1280, 0, 3, 8, 8, 1280, t);
  bench_gemm("conv3x3 2560->1280 @16^2", 0, 1280, 0, 3, 8, 16, 2560, 0);
  bench_gemm("conv3x3 960->320 @64^2", 0, 320, 0, 3, 8, 64, 960, 0);
  bench_gemm("linear qk 320->640 @64^2", 32768, 640, 320, 0, 0, 0, 0, 0);
  bench_gemm("linear geglu-in 320->2560", 32768, 2560, 320, 0, 0, 0, 0, 0);
  bench_gemm("linear ff-out 1280->320", 32768, 320, 1280, 0, 0, 0, 0, 0);
  bench_gemm("linear 640->5120 @32^2", 8192, 5120, 640, 0, 0, 0, 0, 0);
  bench_gemm("linear 1280->10240 @16^2", 2048, 10240, 1280, 0, 0, 0, 0, 0);
  bench_gemm("vae conv3x3 128->128 @512^2 (B1)", 0, 128, 0, 3, 1, 512, 128, 0);
  bench_gemm("vae conv3x3 512->512 @64^2 (B4)", 0, 512, 0, 3, 4, 64, 512, 0);
  bench_gemm("square 4096^3", 4096, 4096, 4096, 0, 0, 0, 0, 22);
  bench_attn("self-attn 64^2 d40", 8, 8, 4096, 4096, 40);
  bench_attn("self-attn 32^2 d80", 8, 8, 1024, 1024, 80);
  bench_attn("self-attn 16^2 d160", 8, 8, 256, 256, 160);
  bench_attn("cross-attn 64^2 d40", 8, 8, 4096, 148, 40);
  bench_attn("seecoder cross d96", 1, 8, 144, 4096, 96);
  bench_gn("groupnorm+silu 320 @64^2", 8, 4096, 320);
  bench_gn("groupnorm+silu 1280 @16^2", 8, 256, 1280);
  bench_gn("groupnorm+silu 128 @512^2", 4, 262144, 128);
  return 0;
}
