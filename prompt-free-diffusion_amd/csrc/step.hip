// The fused CFG combine + sampler step: ONE kernel behind the five entry points pfd_cfg_ddim_step,
// pfd_cfg_ddim_step_rng, pfd_cfg_ddim_step_ps, pfd_cfg_dpmpp_step and pfd_cfg_step_masked -- and pfd_cfg_step_mul, any of the
// five with a per-sample factor on the guided eps (guidance rescale) --, one launch per step.  Per element:
//   e      = the guided eps (nb = 2: eu + scale (ec - eu); nb = 1: eu scale), scale the row's or scale_ps[b]; times
//            eps_mul[b] where the entry point has one
//   pred   = (x - sqrt(1-a_t) e) / sqrt(a_t)
//   xp     = DDIM: sqrt(a_prev) pred + dir e [+ sigma noise], the noise a tensor or the seeded stream-0 normal times noise_mul
//            DPM-Solver++(2M): c_x x + c_d D, D = pred or w_cur pred + w_prev x0_prev
//   x_out  = xp, or masked: m xp + (1 - m) known, known = ksq x0_keep + ks z_keep (the stream-3 normal)
// pred_x0 is always the unmasked one; the next UNet input is `rep` f16 NHWC copies of x_out.  lib/solver.py, lib/noise.py and
// lib/inpaint.py are the same functions in fp64 on the host.
//
// The whole file is compiled with floating-point contraction OFF: every rounding of the step is written out below, a sum of
// products either as explicitly rounded products or through __builtin_fmaf.  The bits of an entry point therefore do not
// depend on what the compiler would fuse in one instantiation or another -- and what rests on them (graphed = eager, a
// sample does not depend on its company, mask = 1 is the unmasked step, the kept region ends as x0_keep, a per-sample scale
// vector is the batch-wide call) holds by construction.  tests/golden/step_bits.npz pins the bits of every form.
#include "pfd_common.h"
#include "philox.h"

#pragma clang fp contract(off)

namespace {

constexpr int kSolverDdim = 0, kSolverDpmpp = 1;

// what every entry point fills in; pointers an entry point does not have are NULL
struct StepArgs {
  const half_t* eps;       // f16 NHWC [nb*B, h, w, C], unconditional batch first
  const float* x;          // fp32 NCHW [B, C, h, w], like noise, x0_prev, x0_keep and the two fp32 outputs
  const float* noise;      // DDIM, un-keyed: the noise tensor, or NULL
  const float* x0_prev;    // DPM-Solver++: the history, or NULL for a first-order step
  const int64_t* key;      // KEYED: [B][2] (seed, sample_id)
  const float* coef;       // DDIM {a_t, a_prev, sigma, sqrt(1-a_t), scale}; DPM {a_t, sqrt(1-a_t), c_x, c_d, w_cur, w_prev, scale, 0}
  const float* scale_ps;   // [B] per-sample guidance scales in place of the row's, or NULL
  const float* eps_mul;    // [B] guidance rescale: the guided eps of sample b times eps_mul[b] (guidance.hip), or NULL
  const float* x0_keep;    // MASKED
  const float* mask;       // MASKED: [1 | B, h, w]
  float* x_out;
  float* pred_x0;
  half_t* xin_next;        // or NULL
  float noise_mul, ksq, ks;
  int nb, step, mask_bcast, rep, B, C, h, w;
};

// NHWC index of element (b, c, yh, xw) of an NCHW [B, C, h, w] tensor
__device__ __forceinline__ long nhwc_index(int b, int c, int yh, int xw, int C, int h, int w) {
  return (((long)b * h + yh) * w + xw) * C + c;
}

// the guided eps from the unconditional and (nb = 2) the conditional eps of an element (f16 values, exact in fp32): the
// difference is rounded, then one fma
__device__ __forceinline__ float guided_eps(float eu, float ec, int nb, float scale) {
  if (nb == 2) return __builtin_fmaf(scale, ec - eu, eu);
  return eu * scale;
}

// one fma, then the rounded product with 1 / sqrt(a_t)
__device__ __forceinline__ float pred_x0_of(float xv, float e, float s1mat, float isq_at) {
  return isq_at * __builtin_fmaf(-s1mat, e, xv);
}

// `rep` fp16 copies of the next UNet input at NHWC index ei (nothing without xin_next)
__device__ __forceinline__ void emit_next(half_t* xin_next, int rep, long n, long ei, float v) {
  if (xin_next) {
    const half_t hv = (half_t)v;
    for (int r = 0; r < rep; ++r) xin_next[(long)r * n + ei] = hv;
  }
}

// the per-launch numbers of a DDIM row: sqrtf and the division are correctly rounded, 1 - a_prev is rounded before sigma^2
// is taken off it in one fma
struct DdimStep {
  float sigma, sq_aprev, dir;
  __device__ __forceinline__ explicit DdimStep(const float* coef) {
    const float a_prev = coef[1];
    sigma = coef[2];
    sq_aprev = sqrtf(a_prev);
    dir = sqrtf(fmaxf(__builtin_fmaf(-sigma, sigma, 1.0f - a_prev), 0.f));
  }
};

__device__ __forceinline__ void load4(const float* p, float v[4]) {
  const float4 t = *reinterpret_cast<const float4*>(p);
  v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
}

// ROUNDING FORMS.  Inherited, not designed: before this file the step was four kernel templates whose sums of products the
// compiler contracted differently from one instantiation to the next, and requests have been served with those bits since.
// Each form below is what one of them compiled to (gfx950, ROCm 7.0), kept so that no entry point changes its results; with
// r(.) a rounding to fp32:
//                                      DDIM update xp                      + noise               pfd_cfg_ entry points
//   un-keyed, any access               r(sq_aprev p0) + r(dir e)           fma(sigma, noise, xp)  ddim_step, ddim_step_ps
//   keyed,  16-byte access             fma(dir, e, r(sq_aprev p0))         fma(sigma, nz, xp)     ddim_step_rng, ddim_step_ps
//   keyed,  scalar access              fma(dir, e, r(sq_aprev p0))         xp + r(sigma nz)       ddim_step_rng, ddim_step_ps
//   masked, sigma == 0                 the un-keyed form (that kernel served eta = 0)             step_masked, solver 0
//   masked, sigma != 0                 the keyed form of its access                               step_masked, solver 0
//   (nz = r(noise_mul z); the un-masked keyed form at sigma == 0 draws nothing and adds nothing)
//   DPM-Solver++, every entry point    D = r(w_cur p0) + r(w_prev x0_prev);  xp = fma(c_x, x, r(c_d D))
//                                      known                               blend
//   masked, 16-byte access             fma(ks, z_keep, r(ksq x0_keep))     solver 0: fma(m, xp, r((1-m) known))
//   masked, scalar access              r(ksq x0_keep) + r(ks z_keep)       solver 1: fma(1-m, known, r(m xp))
//   (ks == 0: known = r(ksq x0_keep) in both)
// The guided eps, pred_x0 and the per-launch numbers round alike everywhere (guided_eps, pred_x0_of, DdimStep).  Making the
// forms equal would be simpler still, and is a change of results: DESIGN.md 3.21 lists it as follow-up.
template <bool KEYED, bool MASKED, bool VEC>
struct Rounding {
  static constexpr bool kNoiseFused = VEC;   // keyed noise term: one fma, or a rounded product added
  static constexpr bool kKnownFused = VEC;   // known: one fma onto r(ksq x0_keep), or two rounded products
  // DDIM update: dir e fused onto r(sq_aprev p0), or two rounded products
  __device__ static __forceinline__ bool update_fused(bool step_noise) { return KEYED && (!MASKED || step_noise); }
};

// One thread = four consecutive NCHW elements of ONE sample = one Philox call per stream in use.  Compile-time: the solver,
// KEYED (a key row per sample: the seeded step noise of DDIM and the kept region's noise), MASKED, and VEC (w % 4 == 0 and
// every fp32 tensor 16-byte aligned: the four share a row, 16-byte accesses; otherwise the scalar path computes the same
// values and drops the tail of a sample's last quad).  A noise tensor, per-sample scales, a history, sigma == 0 and ks == 0
// are uniform over the launch: runtime branches.
template <int SOLVER, bool KEYED, bool MASKED, bool VEC>
__global__ __launch_bounds__(256) void cfg_step_kernel(const StepArgs a) {
  using R = Rounding<KEYED, MASKED, VEC>;
  const int C = a.C, h = a.h, w = a.w;
  const long hw = (long)h * w;
  const long ns = (long)C * hw;
  const long n = (long)a.B * ns;
  const long nq = (ns + 3) >> 2;
  const long total = (long)a.B * nq;
  const float* coef = a.coef;
  const DdimStep k(coef);   // (read as a DDIM row; used under the DDIM solver only)
  const float s1mat = coef[SOLVER == kSolverDdim ? 3 : 1];
  const float isq_at = 1.0f / sqrtf(coef[0]);
  const bool hist = SOLVER == kSolverDpmpp && a.x0_prev;
  // (a first-order step does not read the weights; a DDIM row has five numbers)
  const float c_x = coef[2], c_d = coef[3], w_cur = hist ? coef[4] : 1.f, w_prev = hist ? coef[5] : 0.f;
  const float scale_all = coef[SOLVER == kSolverDdim ? 4 : 6];
  const bool step_noise = KEYED && SOLVER == kSolverDdim && k.sigma != 0.f;
  const bool keep_noise = MASKED && a.ks != 0.f;
  const bool noise_tensor = !KEYED && SOLVER == kSolverDdim && a.noise;
  const bool update_fused = R::update_fused(step_noise);
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int b = (int)(i / nq);
    const long q = i - (long)b * nq;
    const long e0 = q * 4;
    const long base = (long)b * ns + e0;
    const float scale = a.scale_ps ? a.scale_ps[b] : scale_all;
    float z[4] = {0.f, 0.f, 0.f, 0.f}, zk[4] = {0.f, 0.f, 0.f, 0.f}, xv[4], nv[4] = {0.f, 0.f, 0.f, 0.f},
          hv[4] = {0.f, 0.f, 0.f, 0.f}, kv[4] = {0.f, 0.f, 0.f, 0.f}, xo4[4], p04[4];
    if (KEYED) {   // (the quad index is one 32-bit counter word: the entry points bound ns for the keyed forms)
      if (step_noise) pfd_philox_normal4(a.key[2 * b], a.key[2 * b + 1], a.step, (uint32_t)q, PFD_STREAM_STEP, z);
      if (keep_noise) pfd_philox_normal4(a.key[2 * b], a.key[2 * b + 1], a.step, (uint32_t)q, PFD_STREAM_KEEP, zk);
    }
    if (VEC) {
      load4(a.x + base, xv);
      if (noise_tensor) load4(a.noise + base, nv);
      if (hist) load4(a.x0_prev + base, hv);
      if (MASKED) load4(a.x0_keep + base, kv);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const bool in = e0 + j < ns;
        xv[j] = in ? a.x[base + j] : 0.f;
        if (noise_tensor) nv[j] = in ? a.noise[base + j] : 0.f;
        if (hist) hv[j] = in ? a.x0_prev[base + j] : 0.f;
        if (MASKED) kv[j] = in ? a.x0_keep[base + j] : 0.f;
      }
    }
    // the gathers of the four elements first (NHWC eps, the mask), so that they are in flight together.  VEC: the four share
    // a row, one decode serves them (the next element is C halves on in eps, one float on in the mask)
    long ei[4], mi = 0;
    float eu[4], ec[4] = {0.f, 0.f, 0.f, 0.f}, mk[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      ei[j] = 0;
      eu[j] = 0.f;
      if (!VEC && e0 + j >= ns) continue;
      if (!VEC || j == 0) {
        const long el = e0 + j;   // (c*h + y)*w + x inside the sample
        const int xw = (int)(el % w);
        const long t = el / w;
        const int yh = (int)(t % h);
        const int c = (int)(t / h);
        ei[j] = nhwc_index(b, c, yh, xw, C, h, w);
        mi = (a.mask_bcast ? 0 : (long)b * hw) + (long)yh * w + xw;
      } else {
        ei[j] = ei[j - 1] + C;
        mi += 1;
      }
      eu[j] = (float)a.eps[ei[j]];
      if (a.nb == 2) ec[j] = (float)a.eps[n + ei[j]];
      if (MASKED) mk[j] = a.mask[mi];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      xo4[j] = p04[j] = 0.f;
      if (!VEC && e0 + j >= ns) continue;
      float e = guided_eps(eu[j], ec[j], a.nb, scale);
      if (a.eps_mul) e = a.eps_mul[b] * e;   // a rounded product, for pred_x0 and the update alike; uniform over the launch
      const float p0 = pred_x0_of(xv[j], e, s1mat, isq_at);
      float xp;
      if (SOLVER == kSolverDdim) {
        const float sp = k.sq_aprev * p0;
        xp = update_fused ? __builtin_fmaf(k.dir, e, sp) : sp + k.dir * e;
        if (noise_tensor) xp = __builtin_fmaf(k.sigma, nv[j], xp);
        if (step_noise) {
          const float nz = a.noise_mul * z[j];
          xp = R::kNoiseFused ? __builtin_fmaf(k.sigma, nz, xp) : xp + k.sigma * nz;
        }
      } else {
        float d = p0;
        if (hist) d = w_cur * p0 + w_prev * hv[j];
        xp = __builtin_fmaf(c_x, xv[j], c_d * d);
      }
      float xo = xp;
      if (MASKED) {
        float known = a.ksq * kv[j];
        if (keep_noise) known = R::kKnownFused ? __builtin_fmaf(a.ks, zk[j], known) : known + a.ks * zk[j];
        const float m = mk[j];
        const float om = 1.0f - m;
        xo = SOLVER == kSolverDdim ? __builtin_fmaf(m, xp, om * known) : __builtin_fmaf(om, known, m * xp);
      }
      xo4[j] = xo;
      p04[j] = p0;
      emit_next(a.xin_next, a.rep, n, ei[j], xo);
    }
    if (VEC) {
      *reinterpret_cast<float4*>(a.x_out + base) = make_float4(xo4[0], xo4[1], xo4[2], xo4[3]);
      *reinterpret_cast<float4*>(a.pred_x0 + base) = make_float4(p04[0], p04[1], p04[2], p04[3]);
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (e0 + j < ns) {
          a.x_out[base + j] = xo4[j];
          a.pred_x0[base + j] = p04[j];
        }
    }
  }
}

// ---- the host side --------------------------------------------------------------------------------------------------------
// what an entry point may refuse, in the order the checks are made
enum StepFault { kStepOk, kNullArg, kBadSolver, kBadStep, kBadDims, kBadBm, kKeepAlias, kBadHistory, kTooLarge };

// The one validator.  `required`: the pointers this entry point cannot do without (eps, x, coef and the two fp32 outputs are
// required everywhere); solver: 0 / 1 as the caller gave it; Bm: the mask's leading dimension (MASKED only); bounded: the
// 2^34 elements per sample of the Philox counter apply (every keyed launch; pfd_cfg_dpmpp_step has answered it from the
// start, with its own code) -- the un-keyed DDIM forms have no such bound.
StepFault check_step(const StepArgs& a, bool required, int solver, bool masked, int Bm, bool bounded) {
  if (!a.eps || !a.x || !a.coef || !a.x_out || !a.pred_x0 || !required) return kNullArg;
  if (solver != kSolverDdim && solver != kSolverDpmpp) return kBadSolver;
  if (a.key && a.step < 0) return kBadStep;
  if (!(a.nb >= 1 && a.nb <= 2 && a.B > 0 && a.C > 0 && a.h > 0 && a.w > 0 && !(a.xin_next && (a.rep < 1 || a.rep > 2))))
    return kBadDims;
  if (masked && Bm != 1 && Bm != a.B) return kBadBm;
  if (masked && (a.x0_keep == a.x_out || a.x0_keep == a.pred_x0)) return kKeepAlias;
  // the history is read while both outputs are written
  if (a.x0_prev && (solver != kSolverDpmpp || a.x0_prev == a.x_out || a.x0_prev == a.pred_x0)) return kBadHistory;
  if (bounded && (long)a.C * a.h * a.w > ((long)1 << 34)) return kTooLarge;   // the quad index is one 32-bit counter word
  return kStepOk;
}

// every pointer the 16-byte form touches; a NULL one is aligned
bool quad_vec_ok(const StepArgs& a) {
  return !(a.w & 3) && aligned16(a.x) && aligned16(a.x_out) && aligned16(a.pred_x0) && aligned16(a.noise) &&
         aligned16(a.x0_prev) && aligned16(a.x0_keep);
}

template <int SOLVER, bool KEYED, bool MASKED>
void launch_form(const StepArgs& a, hipStream_t stream) {
  const long nq = ((long)a.C * a.h * a.w + 3) >> 2;
  const dim3 grid(grid_for((long)a.B * nq, 256));
  if (quad_vec_ok(a)) hipLaunchKernelGGL((cfg_step_kernel<SOLVER, KEYED, MASKED, true>), grid, dim3(256), 0, stream, a);
  else hipLaunchKernelGGL((cfg_step_kernel<SOLVER, KEYED, MASKED, false>), grid, dim3(256), 0, stream, a);
}

// the one launch of a step on checked arguments (profiler bucket 15); `name` for the launch check
int launch_step(const StepArgs& a, int solver, bool masked, pfd_stream_t stream, const char* name) {
  hipStream_t s = (hipStream_t)stream;
  PfdProfScope prof_scope(15, 0.0, 0.0, s);
  if (solver == kSolverDdim) {
    if (masked) launch_form<kSolverDdim, true, true>(a, s);
    else if (a.key) launch_form<kSolverDdim, true, false>(a, s);
    else launch_form<kSolverDdim, false, false>(a, s);
  } else {
    if (masked) launch_form<kSolverDpmpp, true, true>(a, s);
    else launch_form<kSolverDpmpp, false, false>(a, s);
  }
  return pfd_check_launch(name);
}

StepArgs step_args(const void* eps, int nb, const float* x, const float* coef, const float* scale, float* x_out, float* pred_x0,
                   void* xin_next, int rep, int B, int C, int h, int w) {
  StepArgs a = {};
  a.eps = (const half_t*)eps; a.nb = nb; a.x = x; a.coef = coef; a.scale_ps = scale; a.x_out = x_out; a.pred_x0 = pred_x0;
  a.xin_next = (half_t*)xin_next; a.rep = rep; a.B = B; a.C = C; a.h = h; a.w = w;
  a.noise_mul = 1.0f; a.ksq = 1.0f;
  return a;
}

int refuse(int code, const char* msg) {
  pfd_set_error(msg);
  return code;
}

}  // namespace

extern "C" int pfd_cfg_ddim_step(const void* eps, int32_t nb, const float* x, const float* noise, const float* coef,
                                 float* x_prev, float* pred_x0, void* xin_next, int32_t rep, int32_t B, int32_t C,
                                 int32_t h, int32_t w, pfd_stream_t stream) {
  StepArgs a = step_args(eps, nb, x, coef, nullptr, x_prev, pred_x0, xin_next, rep, B, C, h, w);
  a.noise = noise;
  if (check_step(a, true, kSolverDdim, false, 0, false) != kStepOk) return PFD_EINVAL;
  return launch_step(a, kSolverDdim, false, stream, "pfd_cfg_ddim_step");
}

extern "C" int pfd_cfg_ddim_step_rng(const void* eps, int32_t nb, const float* x, const int64_t* key, int32_t step,
                                     float noise_mul, const float* coef, float* x_prev, float* pred_x0, void* xin_next,
                                     int32_t rep, int32_t B, int32_t C, int32_t h, int32_t w, pfd_stream_t stream) {
  StepArgs a = step_args(eps, nb, x, coef, nullptr, x_prev, pred_x0, xin_next, rep, B, C, h, w);
  a.key = key; a.step = step; a.noise_mul = noise_mul;
  const StepFault f = check_step(a, key, kSolverDdim, false, 0, true);
  if (f != kStepOk) return f == kTooLarge ? PFD_ESHAPE : PFD_EINVAL;
  return launch_step(a, kSolverDdim, false, stream, "pfd_cfg_ddim_step_rng");
}

extern "C" int pfd_cfg_ddim_step_ps(const void* eps, int32_t nb, const float* x, const float* noise, const int64_t* key,
                                    int32_t step, float noise_mul, const float* coef, const float* scale,
                                    float* x_prev, float* pred_x0, void* xin_next, int32_t rep, int32_t B, int32_t C,
                                    int32_t h, int32_t w, pfd_stream_t stream) {
  StepArgs a = step_args(eps, nb, x, coef, scale, x_prev, pred_x0, xin_next, rep, B, C, h, w);
  a.noise = noise; a.key = key; a.step = step; a.noise_mul = noise_mul;
  const StepFault f = check_step(a, scale && !(noise && key), kSolverDdim, false, 0, key != nullptr);
  if (f != kStepOk) return f == kTooLarge ? PFD_ESHAPE : PFD_EINVAL;
  return launch_step(a, kSolverDdim, false, stream, "pfd_cfg_ddim_step_ps");
}

extern "C" int pfd_cfg_dpmpp_step(const void* eps, int32_t nb, const float* x, const float* x0_prev, const float* coef,
                                  const float* scale, float* x_next, float* pred_x0, void* xin_next, int32_t rep,
                                  int32_t B, int32_t C, int32_t h, int32_t w, pfd_stream_t stream) {
  StepArgs a = step_args(eps, nb, x, coef, scale, x_next, pred_x0, xin_next, rep, B, C, h, w);
  a.x0_prev = x0_prev;
  // (more than 2^34 elements per sample: PFD_EINVAL here, where the seeded siblings answer PFD_ESHAPE -- pfd_hip.h)
  if (check_step(a, true, kSolverDpmpp, false, 0, true) != kStepOk) return PFD_EINVAL;
  return launch_step(a, kSolverDpmpp, false, stream, "pfd_cfg_dpmpp_step");
}

extern "C" int pfd_cfg_step_masked(const void* eps, int32_t nb, const float* x, int32_t solver, const float* x0_prev,
                                   const int64_t* key, int32_t step, float noise_mul, const float* coef,
                                   const float* scale, const float* x0_keep, const float* mask, int32_t Bm, float ksq,
                                   float ks, float* x_out, float* pred_x0, void* xin_next, int32_t rep, int32_t B,
                                   int32_t C, int32_t h, int32_t w, pfd_stream_t stream) {
  StepArgs a = step_args(eps, nb, x, coef, scale, x_out, pred_x0, xin_next, rep, B, C, h, w);
  a.x0_prev = x0_prev; a.key = key; a.step = step; a.noise_mul = noise_mul; a.x0_keep = x0_keep; a.mask = mask;
  a.mask_bcast = Bm == 1 && B > 1 ? 1 : 0; a.ksq = ksq; a.ks = ks;
  switch (check_step(a, key && x0_keep && mask, solver, true, Bm, true)) {
    case kStepOk: break;
    case kNullArg: return refuse(PFD_EINVAL, "pfd_cfg_step_masked: eps, x, key, coef, x0_keep, mask, x_out and pred_x0 must not be NULL");
    case kBadSolver: return refuse(PFD_EINVAL, "pfd_cfg_step_masked: solver must be 0 (DDIM) or 1 (DPM-Solver++)");
    case kBadStep: return refuse(PFD_EINVAL, "pfd_cfg_step_masked: step must not be negative");
    case kBadDims: return refuse(PFD_EINVAL, "pfd_cfg_step_masked: nb in {1, 2}, positive B, C, h, w and rep in {1, 2} with xin_next");
    case kBadBm: return refuse(PFD_EINVAL, "pfd_cfg_step_masked: Bm must be 1 (one mask for all samples) or B");
    case kKeepAlias: return refuse(PFD_EINVAL, "pfd_cfg_step_masked: x0_keep must not alias x_out or pred_x0");
    case kBadHistory: return refuse(PFD_EINVAL, "pfd_cfg_step_masked: x0_prev goes with solver 1 and must not alias x_out or pred_x0");
    case kTooLarge: return refuse(PFD_ESHAPE, "pfd_cfg_step_masked: more than 2^34 elements per sample");
  }
  return launch_step(a, solver, true, stream, "pfd_cfg_step_masked");
}

// Any of the five above with the guidance-rescale factor eps_mul [B] (pfd_guidance_rescale_f32) on the guided eps.  The
// arguments are the union of the five signatures, NULL where the entry point stood for has none; which one that is follows
// from them: a mask -> pfd_cfg_step_masked; else solver 1 -> pfd_cfg_dpmpp_step; else a scale -> pfd_cfg_ddim_step_ps, a key
// -> pfd_cfg_ddim_step_rng, neither -> pfd_cfg_ddim_step.  Its rules for which pointers go together, its check_step and its
// instantiation apply, so eps_mul of ones gives that entry point's bits.  There is no rescale without an unconditional half.
extern "C" int pfd_cfg_step_mul(const void* eps, int32_t nb, const float* x, int32_t solver, const float* noise,
                                const float* x0_prev, const int64_t* key, int32_t step, float noise_mul, const float* coef,
                                const float* scale, const float* eps_mul, const float* x0_keep, const float* mask, int32_t Bm,
                                float ksq, float ks, float* x_out, float* pred_x0, void* xin_next, int32_t rep, int32_t B,
                                int32_t C, int32_t h, int32_t w, pfd_stream_t stream) {
  if (!eps_mul) return refuse(PFD_EINVAL, "pfd_cfg_step_mul: eps_mul must not be NULL (without it, call the entry point itself)");
  if (nb != 2) return refuse(PFD_EINVAL, "pfd_cfg_step_mul: nb must be 2: there is no rescale without an unconditional half");
  StepArgs a = step_args(eps, nb, x, coef, scale, x_out, pred_x0, xin_next, rep, B, C, h, w);
  a.eps_mul = eps_mul;
  const bool masked = mask != nullptr;
  StepFault f;
  if (masked) {
    if (noise) return refuse(PFD_EINVAL, "pfd_cfg_step_mul: the masked step has no form with a noise tensor");
    a.x0_prev = x0_prev; a.key = key; a.step = step; a.noise_mul = noise_mul; a.x0_keep = x0_keep; a.mask = mask;
    a.mask_bcast = Bm == 1 && B > 1 ? 1 : 0; a.ksq = ksq; a.ks = ks;
    f = check_step(a, key && x0_keep, solver, true, Bm, true);
  } else if (x0_keep) {
    return refuse(PFD_EINVAL, "pfd_cfg_step_mul: x0_keep comes with a mask");
  } else if (solver == kSolverDpmpp) {
    if (noise || key) return refuse(PFD_EINVAL, "pfd_cfg_step_mul: DPM-Solver++ is deterministic: no noise tensor, no key");
    a.x0_prev = x0_prev;
    f = check_step(a, true, kSolverDpmpp, false, 0, true);
  } else {
    a.noise = noise; a.key = key; a.step = step; a.noise_mul = noise_mul; a.x0_prev = x0_prev;   // (a history: refused below)
    f = check_step(a, !(noise && key), solver, false, 0, key != nullptr);
  }
  if (f != kStepOk) return refuse(f == kTooLarge ? PFD_ESHAPE : PFD_EINVAL, "pfd_cfg_step_mul: arguments the entry point it stands for refuses");
  return launch_step(a, solver, masked, stream, "pfd_cfg_step_mul");
}
