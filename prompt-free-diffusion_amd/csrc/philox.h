// Counter-based noise of the stochastic DDIM step (eta > 0, ddim.py:166-169): Philox4x32-10 + Box-Muller.
// The noise of element e of a sample at DDIM step `step` is a pure function of (seed, sample_id, step, e): no noise
// tensor, no generator state, so the draw is capturable in a hipGraph, independent of the batch a sample rides in and
// of the number of ranks the batch is cut over.  lib/noise.py restates this file in numpy (the oracle of the tests);
// DESIGN.md ("Seeded on-device noise") has the specification.
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

#define PFD_HD __device__ __forceinline__

#define PFD_PHILOX_M0 0xD2511F53u
#define PFD_PHILOX_M1 0xCD9E8D57u
#define PFD_PHILOX_W0 0x9E3779B9u
#define PFD_PHILOX_W1 0xBB67AE85u

// c[0..3] <- Philox4x32-10(counter c, key (k0, k1))
PFD_HD void pfd_philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)PFD_PHILOX_M0 * c[0];
    const uint64_t p1 = (uint64_t)PFD_PHILOX_M1 * c[2];
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
    c[0] = n0;
    c[1] = (uint32_t)p1;
    c[2] = n2;
    c[3] = (uint32_t)p0;
    k0 += PFD_PHILOX_W0;
    k1 += PFD_PHILOX_W1;
  }
}

// two standard normals from two 32-bit words: u in (0, 1] and v in [0, 1) are exact in fp32 (24 bits each); the
// accurate logf / sinpif / cospif, never the __ fast intrinsics (the host oracle is compared at 1e-5 absolute)
PFD_HD void pfd_box_muller(uint32_t ra, uint32_t rb, float* z0, float* z1) {
  const float u = (float)((ra >> 8) + 1u) * 0x1p-24f;
  const float v = (float)(rb >> 8) * 0x1p-24f;
  const float rad = sqrtf(-2.0f * logf(u));
  *z0 = rad * cospif(2.0f * v);
  *z1 = rad * sinpif(2.0f * v);
}

// the fourth counter word names the stream a draw belongs to: the same (seed, sample_id, step, element) gives unrelated
// normals in different streams.  0: the step noise (what the word always was); 1 / 2: the forward-noising noise and the
// posterior noise of an img2img start (latent.hip), both at step 0; 3: the noise the kept region of a masked step is
// re-noised with (step.hip), at the step's index
#define PFD_STREAM_STEP 0u
#define PFD_STREAM_Q 1u
#define PFD_STREAM_POSTERIOR 2u
#define PFD_STREAM_KEEP 3u

// the normals of elements 4q .. 4q+3 of sample (seed, sample_id) at DDIM step `step` in stream `stream`
PFD_HD void pfd_philox_normal4(int64_t seed, int64_t sample_id, int32_t step, uint32_t q, uint32_t stream, float z[4]) {
  uint32_t c[4] = {q, (uint32_t)step, (uint32_t)((uint64_t)sample_id & 0xffffffffu), stream};
  pfd_philox4x32_10(c, (uint32_t)((uint64_t)seed & 0xffffffffu), (uint32_t)(((uint64_t)seed >> 32) & 0xffffffffu));
  pfd_box_muller(c[0], c[1], &z[0], &z[1]);
  pfd_box_muller(c[2], c[3], &z[2], &z[3]);
}
