// Philox4x32-10 + Box-Muller of the sample-indexed generator (rng.hip), shared with the fused DDP step of sampler.hip,
// which draws the same values itself: one definition, so that both compile to the same arithmetic.
#pragma once
#include "common.h"

// (the includers say the same: u01 below must stay a rounded multiply and a rounded add, never one FMA)
#pragma clang fp contract(off)

namespace dmh_philox {

struct U4 {
  uint32_t x, y, z, w;
};

__device__ __forceinline__ U4 philox4x32_10(U4 c, uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c.x), lo0 = 0xD2511F53u * c.x;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c.z), lo1 = 0xCD9E8D57u * c.z;
    c = U4{hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0};
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return c;
}

// (0, 1]-open-at-zero uniform of a 32-bit word, as cuRAND / torch's CUDA generator place it: x * 2^-32 + 2^-33
__device__ __forceinline__ float u01(uint32_t x) { return (float)x * 2.3283064365386963e-10f + 1.1641532182693481e-10f; }

// Box-Muller: two words -> two standard normals
__device__ __forceinline__ void box_muller(uint32_t a, uint32_t b, float& n0, float& n1) {
  const float r = sqrtf(-2.0f * logf(u01(a)));
  float s, c;
  sincospif(2.0f * u01(b), &s, &c);
  n0 = r * c;
  n1 = r * s;
}

// the four N(0,1) values of counter quad q (elements 4q .. 4q+3 of a row) at draw `draw` of sample `sid`
__device__ __forceinline__ void normal4(uint64_t seed, uint64_t draw, uint64_t sid, uint64_t q, float v[4]) {
  const U4 r = philox4x32_10(U4{(uint32_t)q, (uint32_t)draw, (uint32_t)sid, (uint32_t)(sid >> 32)}, (uint32_t)seed,
                             (uint32_t)(seed >> 32));
  box_muller(r.x, r.y, v[0], v[1]);
  box_muller(r.z, r.w, v[2], v[3]);
}

// The end of a launch that consumes one draw of the keyed generator (state: seed, draw index, tickets, reserved).  Every
// workgroup has read the draw index before it takes a ticket; the last one to arrive advances it and puts the ticket counter
// back, both visible to the next launch on the stream.  All threads of the workgroup call it.
__device__ __forceinline__ void advance_draw(unsigned long long* state, unsigned long long draw) {
  __syncthreads();
  if (threadIdx.x == 0) {
    const unsigned long long total = (unsigned long long)gridDim.x * gridDim.y;
    const unsigned long long t = atomicAdd(&state[2], 1ull);
    if (t == total - 1) {
      state[2] = 0;
      state[1] = draw + 1;
    }
  }
}

// workgroups per sample of such a launch over B rows of nq counter quads, 256 threads each.  Every workgroup ends with a
// returning atomic on ONE word (the arrival ticket): at 2400 workgroups those tickets were most of the launch (33 us for 2.4 M
// normals).  About two workgroups per CU in total, each looping over its share
static inline unsigned draw_grid_x(int B, int64_t nq) {
  int64_t gx = cdiv64(nq, 256);
  const int64_t cap = B >= 512 ? 1 : 512 / B;
  return (unsigned)(gx < 1 ? 1 : (gx > cap ? cap : gx));
}

}  // namespace dmh_philox
