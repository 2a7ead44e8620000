// Re-labelling a batch of real pairs (ddpm.relabel_batch, Trainer.relabel; not in the reference) in one launch: per sample a new
// homography drawn on the device, its flow and flow image, the source warped by it as a first target, the validity of every
// target pixel (include/dmhomo_hip_relabel.h has the definition).  What it stands for is dmh_homography_flow +
// dmh_homography_warp + a where / cat that assemble the batch, behind a host-side draw; the per-pixel bodies are those kernels'
// own (geometry_dev.h), so flow, flow image and warp are theirs bit for bit.
#include "common.h"
#include "flat_range.h"
#include "geometry_dev.h"
#include "philox.h"
#include "../../include/dmhomo_hip_relabel.h"

#pragma clang fp contract(off)

namespace {

using namespace dmh_philox;

struct RelabelArgs {
  unsigned long long seed;
  double a, t, p;      // max_affine, max_shift, max_persp
  float max_flow;
  int H, W, use_fill;
};

// u_i = 2.0 * (double)u01(w_i) - 1.0
__device__ __forceinline__ double relabel_uniform(uint32_t w) {
  const double d = 2.0 * (double)u01(w);
  return d - 1.0;
}

// H_new of sample sid into h[9] (row-major), every operation rounded separately.  hb: the base homography or nullptr
__device__ void relabel_homography(const RelabelArgs& g, unsigned long long sid, const double* __restrict__ hb, double* h) {
  const uint32_t k0 = (uint32_t)g.seed, k1 = (uint32_t)(g.seed >> 32);
  const uint32_t s0 = (uint32_t)sid, s1 = (uint32_t)(sid >> 32);
  const U4 q0 = philox4x32_10(U4{0u, 0xFFFFFFFFu, s0, s1}, k0, k1);
  const U4 q1 = philox4x32_10(U4{1u, 0xFFFFFFFFu, s0, s1}, k0, k1);
  const double u[8] = {relabel_uniform(q0.x), relabel_uniform(q0.y), relabel_uniform(q0.z), relabel_uniform(q0.w),
                       relabel_uniform(q1.x), relabel_uniform(q1.y), relabel_uniform(q1.z), relabel_uniform(q1.w)};
  double P[9];
  P[0] = 1.0 + u[0] * g.a, P[1] = u[1] * g.a, P[2] = u[2] * g.t;
  P[3] = u[3] * g.a, P[4] = 1.0 + u[4] * g.a, P[5] = u[5] * g.t;
  P[6] = u[6] * g.p, P[7] = u[7] * g.p, P[8] = 1.0;
  const double s[3] = {(double)g.W / 640.0, (double)g.H / 360.0, 1.0};
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) P[i * 3 + j] = (P[i * 3 + j] * s[i]) / s[j];
  if (!hb) {
#pragma unroll
    for (int k = 0; k < 9; ++k) h[k] = P[k];
    return;
  }
  double M[9];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) M[i * 3 + j] = (P[i * 3] * hb[j] + P[i * 3 + 1] * hb[3 + j]) + P[i * 3 + 2] * hb[6 + j];
#pragma unroll
  for (int k = 0; k < 9; ++k) h[k] = M[k] / M[8];
}

// grid: (cdiv(H * W, 256), B); one pixel per thread, planes of H * W floats
__global__ __launch_bounds__(256) void relabel_batch_kernel(const float* __restrict__ data, const int64_t* __restrict__ ids,
                                                            const double* __restrict__ base, float* __restrict__ out,
                                                            double* __restrict__ Hm, unsigned char* __restrict__ valid,
                                                            RelabelArgs g) {
  __shared__ double sh[18];      // H_new, then its inverse (adjugate times 1 / det)
  const int b = blockIdx.y;
  if (threadIdx.x == 0) {
    relabel_homography(g, (unsigned long long)ids[b], base ? base + (size_t)b * 9 : nullptr, sh);
    homography_inverse(sh, sh + 9);
  }
  __syncthreads();
  if (blockIdx.x == 0 && threadIdx.x < 9) Hm[(size_t)b * 9 + threadIdx.x] = sh[threadIdx.x];
  const int H = g.H, W = g.W;
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= H * W) return;
  const int yi = p / W, xi = p % W;
  const size_t hw = (size_t)H * W;
  const float* d = data + (size_t)b * 12 * hw;
  float* o = out + (size_t)b * 12 * hw;
  // the copies: img1, mask
  o[0 * hw + p] = d[0 * hw + p];
  o[1 * hw + p] = d[1 * hw + p];
  o[2 * hw + p] = d[2 * hw + p];
  o[6 * hw + p] = d[6 * hw + p];
  // the label: flow and its image
  float u, v, r, gr, bl;
  homography_flow_pixel(sh, xi, yi, u, v);
  flow_pixel_to_rgb(u, v, g.max_flow, r, gr, bl);
  o[7 * hw + p] = r;
  o[8 * hw + p] = gr;
  o[9 * hw + p] = bl;
  o[10 * hw + p] = u;
  o[11 * hw + p] = v;
  // the first target: img1 warped by H_new, or where it has no source pixel the batch's own img2
  double sx, sy;
  homography_warp_source(sh + 9, xi, yi, sx, sy);
  const bool ok = sx >= 0.0 && sx <= (double)(W - 1) && sy >= 0.0 && sy <= (double)(H - 1);
  valid[(size_t)b * hw + p] = ok ? 1 : 0;
  if (!ok && g.use_fill) {
    o[3 * hw + p] = d[3 * hw + p];
    o[4 * hw + p] = d[4 * hw + p];
    o[5 * hw + p] = d[5 * hw + p];
  } else {
    const HomographyWarpTaps t = homography_warp_taps(sx, sy, H, W);
    o[3 * hw + p] = homography_warp_sample(d + 0 * hw, t, W);
    o[4 * hw + p] = homography_warp_sample(d + 1 * hw, t, W);
    o[5 * hw + p] = homography_warp_sample(d + 2 * hw, t, W);
  }
}

bool range_ok(double v) { return v >= 0.0 && v <= 1.7976931348623157e308; }      // (false for NaN)

}  // namespace

extern "C" int dmh_relabel_batch(const float* data, const int64_t* sample_ids, uint64_t seed, double max_affine, double max_shift,
                                 double max_persp, float max_flow, const double* base, int use_fill, float* out, double* Hm,
                                 unsigned char* valid, int B, int H, int W, void* stream) {
  // ---- every check in front of the launch
  DMH_REQUIRE(data && sample_ids && out && Hm && valid,
              "dmh_relabel_batch: null pointer (data, sample_ids, out, Hm and valid are needed)");
  DMH_REQUIRE(dmh_dims_ok({H, W}, 2, 1 << 16) && B >= 1 && B <= 65535 && (long long)B * 12 * H * W < (1LL << 31),
              "dmh_relabel_batch: B=%d H=%d W=%d (H, W in [2, 2^16], 1 <= B <= 65535, B*12*H*W < 2^31)", B, H, W);
  DMH_REQUIRE(range_ok(max_affine) && range_ok(max_shift) && range_ok(max_persp),
              "dmh_relabel_batch: ranges (%g, %g, %g): each must be a finite number >= 0", max_affine, max_shift, max_persp);
  DMH_REQUIRE(max_affine < 0.25, "dmh_relabel_batch: max_affine=%g must be below 0.25 (the linear part stays diagonally dominant)",
              max_affine);
  DMH_REQUIRE(max_persp < 5e-4, "dmh_relabel_batch: max_persp=%g must be below 5e-4 (w' stays >= 0.5 inside the frame)", max_persp);
  DMH_REQUIRE(max_flow > 0.f && max_flow <= 3.402823466e38f, "dmh_relabel_batch: max_flow=%g must be a finite number > 0",
              (double)max_flow);
  DMH_REQUIRE((((uintptr_t)data | (uintptr_t)out) & 3u) == 0, "dmh_relabel_batch: data / out are not 4-byte aligned");
  DMH_REQUIRE((((uintptr_t)sample_ids | (uintptr_t)base | (uintptr_t)Hm) & 7u) == 0,
              "dmh_relabel_batch: sample_ids / base / Hm are not 8-byte aligned");
  const uintptr_t hw = (uintptr_t)H * (uintptr_t)W;
  const uintptr_t bytes = (uintptr_t)B * 12u * hw * 4u;
  DMH_REQUIRE(!overlaps(out, data, bytes), "dmh_relabel_batch: out overlaps data (out == data is refused: the warp reads img1 "
              "at other pixels than it writes)");
  // ---- the launch
  RelabelArgs g;
  g.seed = seed;
  g.a = max_affine, g.t = max_shift, g.p = max_persp;
  g.max_flow = max_flow;
  g.H = H, g.W = W, g.use_fill = use_fill != 0;
  hipLaunchKernelGGL(relabel_batch_kernel, dim3(cdiv(H * W, 256), (unsigned)B), dim3(256), 0, (hipStream_t)stream, data, sample_ids,
                     base, out, Hm, valid, g);
  DMH_CHECK_LAUNCH("dmh_relabel_batch");
  return DMH_OK;
}
