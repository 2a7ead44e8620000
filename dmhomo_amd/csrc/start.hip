// Starting the sampler from a given pair (cfg.GaussianDiffusion.sample_from; not in the reference): the start image
//   x = ca * (2 * init - 1) + cb * eps
// in one launch (include/dmhomo_hip_start.h has the definition).  Two arms.  Given noise: eps is read (torch's stream
// generator drew it), out may be the noise tensor itself.  Keyed: eps is the keyed generator's next draw, computed here with
// rng_indexed_kernel's own mapping (philox.h: normal4, the grid plan and the arrival ticket are the shared definitions), so the
// noise tensor never exists in memory and the generator is left where one dmh_rng_indexed launch would have left it.
// Every operation is rounded separately: the result is bit for bit dmh_q_sample(dmh_affine(init, 2, -1), eps).
#include "common.h"
#include "flat_range.h"
#include "philox.h"
#include "../../include/dmhomo_hip_start.h"

#pragma clang fp contract(off)

namespace {

using namespace dmh_philox;

// one rounding per operation: dmh_affine's x * 2 + (-1), then dmh_q_sample's ca * k + cb * eps
__device__ __forceinline__ float start_mix(float x, float eps, float ca, float cb) {
  float k = x * 2.0f;
  k = k + (-1.0f);
  const float a = ca * k;
  const float b = cb * eps;
  return a + b;
}

__device__ __forceinline__ float4 start_mix4(float4 x, float4 e, float ca, float cb) {
  return make_float4(start_mix(x.x, e.x, ca, cb), start_mix(x.y, e.y, ca, cb), start_mix(x.z, e.z, ca, cb),
                     start_mix(x.w, e.w, ca, cb));
}

// grid: (blocks per sample, B), as rng_indexed_kernel; thread t of a row owns the counter quads t, t + stride, ... of the row.
// vec: per % 4 == 0 and init, out 16-byte aligned (uniform over the launch)
__global__ __launch_bounds__(256) void start_mix_keyed_kernel(const float* __restrict__ init, const int64_t* __restrict__ ids,
                                                              unsigned long long* state, float ca, float cb,
                                                              float* __restrict__ out, int64_t per, bool vec) {
  const unsigned long long seed = state[0], draw = state[1];
  const int b = blockIdx.y;
  const unsigned long long sid = (unsigned long long)ids[b];
  const float* x = init + (size_t)b * per;
  float* o = out + (size_t)b * per;
  const int64_t nq = (per + 3) >> 2;
  for (int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x; q < nq; q += (int64_t)gridDim.x * 256) {
    float v[4];
    normal4(seed, draw, sid, (uint64_t)q, v);
    const int64_t e = q << 2;
    if (vec) {   // (per % 4 == 0: e + 4 <= per)
      st4(o + e, start_mix4(ld4(x + e), make_float4(v[0], v[1], v[2], v[3]), ca, cb));
    } else {
      for (int j = 0; j < 4 && e + j < per; ++j) o[e + j] = start_mix(x[e + j], v[j], ca, cb);
    }
  }
  advance_draw(state, draw);
}

// the flat range of B * per elements (flat_range.h).  No __restrict__ on noise and out: in place (out == noise), every element
// is read and written by one thread
__global__ __launch_bounds__(FT) void start_mix_noise_kernel(const float* __restrict__ init, const float* noise, float ca, float cb,
                                                             float* out, int64_t total, FlatSplit sp) {
  const int64_t g = (int64_t)blockIdx.x * FT + threadIdx.x, stride = (int64_t)gridDim.x * FT;
  for (int64_t i = g; i < sp.head; i += stride) out[i] = start_mix(init[i], noise[i], ca, cb);
  for (int64_t v = g; v < sp.nv; v += stride) {
    const int64_t i = sp.head + v * 4;
    st4(out + i, start_mix4(ld4(init + i), ld4(noise + i), ca, cb));
  }
  for (int64_t i = sp.t0 + g; i < total; i += stride) out[i] = start_mix(init[i], noise[i], ca, cb);
}

bool finite_f(float v) { return v >= -3.402823466e38f && v <= 3.402823466e38f; }

}  // namespace

extern "C" int dmh_start_mix(const float* init01, const float* noise, const int64_t* sample_ids, uint64_t* state, float ca,
                             float cb, float* out, int B, int64_t per_sample, void* stream) {
  // ---- every check in front of the launch
  DMH_REQUIRE(init01 && out, "dmh_start_mix: null pointer (init01 and out are needed)");
  const bool keyed = !noise;
  if (keyed)
    DMH_REQUIRE(sample_ids && state, "dmh_start_mix: no noise source: give noise, or sample_ids and state (exactly one of the two)");
  else
    DMH_REQUIRE(!sample_ids && !state,
                "dmh_start_mix: two noise sources: give noise, or sample_ids and state (exactly one of the two)");
  DMH_REQUIRE(B >= 1 && B <= 65535 && per_sample >= 1 && per_sample < ((int64_t)1 << 31),
              "dmh_start_mix: B=%d rows of per_sample=%lld elements (1 <= B <= 65535, 1 <= per_sample < 2^31)", B,
              (long long)per_sample);
  DMH_REQUIRE(finite_f(ca) && finite_f(cb), "dmh_start_mix: ca=%g, cb=%g: not finite numbers", (double)ca, (double)cb);
  DMH_REQUIRE((((uintptr_t)init01 | (uintptr_t)noise | (uintptr_t)out) & 3u) == 0, "dmh_start_mix: a pointer is not 4-byte aligned");
  DMH_REQUIRE((((uintptr_t)sample_ids | (uintptr_t)state) & 7u) == 0, "dmh_start_mix: sample_ids / state are not 8-byte aligned");
  const int64_t total = (int64_t)B * per_sample;   // (B < 2^16, per_sample < 2^31)
  const uintptr_t bytes = (uintptr_t)total * 4u;
  DMH_REQUIRE(!overlaps(out, init01, bytes), "dmh_start_mix: out overlaps init01");
  DMH_REQUIRE(out == noise || !overlaps(out, noise, bytes),
              "dmh_start_mix: out overlaps noise in part (in place means out == noise)");
  if (keyed) {
    const uintptr_t po = (uintptr_t)out, ps = (uintptr_t)state, pi = (uintptr_t)sample_ids;
    DMH_REQUIRE(!(po < ps + 32u && ps < po + bytes) && !(po < pi + (uintptr_t)B * 8u && pi < po + bytes),
                "dmh_start_mix: out overlaps sample_ids or state");
  }
  // ---- the launch
  if (keyed) {
    const int64_t nq = (per_sample + 3) >> 2;
    const bool vec = (per_sample & 3) == 0 && (((uintptr_t)init01 | (uintptr_t)out) & 15u) == 0;
    hipLaunchKernelGGL(start_mix_keyed_kernel, dim3(draw_grid_x(B, nq), (unsigned)B), dim3(256), 0, (hipStream_t)stream, init01,
                       sample_ids, (unsigned long long*)state, ca, cb, out, per_sample, vec);
  } else {
    const FlatSplit sp = flat_split(out, total, same_phase(out, init01) && same_phase(out, noise));
    hipLaunchKernelGGL(start_mix_noise_kernel, dim3(flat_grid(sp, total)), dim3(FT), 0, (hipStream_t)stream, init01, noise, ca, cb,
                       out, total, sp);
  }
  DMH_CHECK_LAUNCH("dmh_start_mix");
  return DMH_OK;
}
