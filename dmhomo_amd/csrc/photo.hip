// Photometric-consistency guidance of the conditional sampler (not in the reference's sampler; the energy is the photometric
// term of its training loss, CFG:782-806): at every denoise step the predicted x_start is moved down the gradient of
//   E = (1 / (3 H W)) * sum_{c,p} mask[p] * (u[c,p] - x[c,p])^2,   u = flow_warp(x[3:], flow)
// preconditioned on the im2 side by 1 / max(1, s[q]), s[q] = sum_p mask[p] * w_p(q).  The definition (include/dmhomo_hip.h
// states it too), per sample, x the blended logits (6, H, W) as guided_logit reads them:
//   u[c,p]   = sum_q w_p(q) * x[3+c,q]                  the taps and weights of flow_warp_taps, the fma chain of flow_warp_sample
//   r[c,p]   = mask[p] * (u[c,p] - x[c,p])              fp32
//   lam      = w * (sqrt_ac * sqrt_ac), hl = lam / 2    fp32, from the DmhStep of the entry
//   y[c,p]   = x[c,p] + hl * r[c,p]                     (x[c,p] itself where r == 0)
//   g[c,q]   = sum_p w_p(q) * r[c,p]                    each product in fp32, the sum in Q31.32 fixed point (below)
//   y[3+c,q] = x[3+c,q] - hl * (g[c,q] / max(1, s[q]))  (x[3+c,q] itself where g == 0)
// The transposed warp is a scatter: several source pixels p add into one target q wherever the flow folds or is clamped at
// the border.  It is summed with 64-bit INTEGER atomics (global_atomic_add_x2), so the result of a launch does not depend on
// the order in which workgroups run: integer addition is associative.  A contribution v (fp32) becomes the integer
// rint(clamp(v, -2^30, 2^30) * 2^32); a NaN contributes 0 (it still shows in y[c,p] of its own pixel).  The sum is exact to
// 2^-33 per contribution while sum |v| < 2^31 at a target; beyond that it wraps (unsigned arithmetic: defined, and wrong).
#include "common.h"

#pragma clang fp contract(off)   // (in front of sampler_dev.h: the blend is the step kernels' expression, one rounding per operation)

#include "sampler_dev.h"
#include "geometry_dev.h"

typedef unsigned long long u64;

constexpr double PH_SCALE = 4294967296.0;        // 2^32: Q31.32
constexpr double PH_CLAMP = 1073741824.0;        // 2^30: one contribution
constexpr int ET = 256;                          // threads of an energy workgroup
constexpr int E_CHUNK = 1024;                    // pixels an energy workgroup should at least own
constexpr int E_MAX_WG = 1024;                   // energy workgroups over all rows: 4 per CU

__device__ __forceinline__ u64 ph_fixed(float v) {
  double d = (double)v;
  if (!(d == d)) return 0ull;
  d = fmin(fmax(d, -PH_CLAMP), PH_CLAMP);
  return (u64)__double2ll_rn(d * PH_SCALE);
}
__device__ __forceinline__ float ph_float(u64 t) { return (float)((double)(long long)t * (1.0 / PH_SCALE)); }
__device__ __forceinline__ void ph_add(u64* p, float v) {
  if (v != 0.f) atomicAdd(p, ph_fixed(v));       // (a NaN goes in and adds 0: no branch on it here)
}

__device__ __forceinline__ FlowWarpTaps ph_taps(const float* __restrict__ flow, int b, int p, int H, int W) {
  const size_t hw = (size_t)H * W;
  return flow_warp_taps(flow[((size_t)b * 2 + 0) * hw + p], flow[((size_t)b * 2 + 1) * hw + p], p % W, p / W, H, W);
}

// ---- dmh_photo_weights: s[b][q] = sum_p mask[b][p] * w_p(q).  Scatter into acc[b][q] (zero on entry), then s <- acc, acc <- 0
__global__ __launch_bounds__(256) void photo_weights_scatter_kernel(const float* __restrict__ flow, const float* __restrict__ mask,
                                                                    u64* __restrict__ acc, int H, int W) {
  const int b = blockIdx.y, p = blockIdx.x * 256 + threadIdx.x, hw = H * W;
  if (p >= hw) return;
  const float m = mask[(size_t)b * hw + p];
  if (m == 0.f) return;
  const FlowWarpTaps t = ph_taps(flow, b, p, H, W);
  u64* a = acc + (size_t)b * hw;
  ph_add(a + (size_t)t.y0 * W + t.x0, m * t.wnw);
  if (t.x1ok) ph_add(a + (size_t)t.y0 * W + t.x1, m * t.wne);
  if (t.y1ok) ph_add(a + (size_t)t.y1 * W + t.x0, m * t.wsw);
  if (t.x1ok && t.y1ok) ph_add(a + (size_t)t.y1 * W + t.x1, m * t.wse);
}

__global__ __launch_bounds__(256) void photo_weights_finish_kernel(u64* __restrict__ acc, float* __restrict__ s, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  s[i] = ph_float(acc[i]);
  acc[i] = 0ull;
}

// ---- dmh_photo_guide.  Pass 1, one thread per (sample, pixel p): blend, warp, residual, y[:3] and the scatter of w_p(q) * r
struct PhotoArgs {
  const float *mc, *mn;
  const uint8_t* keep;
  const float *flow, *mask, *sw;
  u64* acc;
  float* guided;
  float w;
  int H, W;
};

__device__ __forceinline__ float ph_half_lambda(const DmhStep& s, float w) {
  const float ac = s.sqrt_ac * s.sqrt_ac;
  return (w * ac) * 0.5f;
}

__device__ __forceinline__ void photo_im1_body(const PhotoArgs& a, float cond_scale, float hl) {
  const int b = blockIdx.y, p = blockIdx.x * 256 + threadIdx.x, H = a.H, W = a.W, hw = H * W;
  if (p >= hw) return;
  const int64_t per_row = (int64_t)6 * hw, base = (int64_t)b * per_row;
  const float m = a.mask[(size_t)b * hw + p];
  const FlowWarpTaps t = ph_taps(a.flow, b, p, H, W);
  const int qnw = t.y0 * W + t.x0, qne = t.y0 * W + t.x1, qsw = t.y1 * W + t.x0, qse = t.y1 * W + t.x1;
  for (int c = 0; c < 3; ++c) {
    const int64_t i1 = base + (int64_t)c * hw, i2 = base + (int64_t)(3 + c) * hw;
    const float x1 = guided_logit(a.mc, a.mn, a.keep, i1 + p, per_row, cond_scale);
    float r = 0.f;
    if (m != 0.f) {   // (mask == 0: r is an exact 0 whatever u is, and im2 is not read)
      const float nw = guided_logit(a.mc, a.mn, a.keep, i2 + qnw, per_row, cond_scale);
      const float ne = t.x1ok ? guided_logit(a.mc, a.mn, a.keep, i2 + qne, per_row, cond_scale) : 0.f;
      const float sw = t.y1ok ? guided_logit(a.mc, a.mn, a.keep, i2 + qsw, per_row, cond_scale) : 0.f;
      const float se = (t.x1ok && t.y1ok) ? guided_logit(a.mc, a.mn, a.keep, i2 + qse, per_row, cond_scale) : 0.f;
      float u = nw * t.wnw;
      u = fmaf(ne, t.wne, u);
      u = fmaf(sw, t.wsw, u);
      u = fmaf(se, t.wse, u);
      r = m * (u - x1);
    }
    float y = x1;
    if (r != 0.f) {
      const float step = hl * r;
      y = x1 + step;
      u64* ac = a.acc + ((size_t)b * 3 + c) * hw;
      ph_add(ac + qnw, r * t.wnw);
      if (t.x1ok) ph_add(ac + qne, r * t.wne);
      if (t.y1ok) ph_add(ac + qsw, r * t.wsw);
      if (t.x1ok && t.y1ok) ph_add(ac + qse, r * t.wse);
    }
    a.guided[i1 + p] = y;
  }
}

// Pass 2, one thread per (sample, channel, pixel q) of im2: y[3+c] from the sums, which it leaves zero for the next step
__device__ __forceinline__ void photo_im2_body(const PhotoArgs& a, float cond_scale, float hl, int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int64_t hw = (int64_t)a.H * a.W, per_row = 6 * hw;
  const int64_t b = i / (3 * hw), rem = i - b * 3 * hw;
  const int64_t gi = b * per_row + 3 * hw + rem;
  const float x2 = guided_logit(a.mc, a.mn, a.keep, gi, per_row, cond_scale);
  const u64 t = a.acc[i];
  float y = x2;
  if (t != 0ull) {
    a.acc[i] = 0ull;
    const float g = ph_float(t);
    const float q = g / fmaxf(1.f, a.sw[b * hw + rem % hw]);
    const float step = hl * q;
    y = x2 - step;
  }
  a.guided[gi] = y;
}

__global__ __launch_bounds__(256) void photo_im1_kernel(DmhStep s, PhotoArgs a) {
  photo_im1_body(a, s.cond_scale, ph_half_lambda(s, a.w));
}
__global__ __launch_bounds__(256) void photo_im1_dev_kernel(const DmhStep* __restrict__ sp, PhotoArgs a) {
  const DmhStep s = *sp;
  photo_im1_body(a, s.cond_scale, ph_half_lambda(s, a.w));
}
__global__ __launch_bounds__(256) void photo_im2_kernel(DmhStep s, PhotoArgs a, int64_t total) {
  photo_im2_body(a, s.cond_scale, ph_half_lambda(s, a.w), total);
}
__global__ __launch_bounds__(256) void photo_im2_dev_kernel(const DmhStep* __restrict__ sp, PhotoArgs a, int64_t total) {
  const DmhStep s = *sp;
  photo_im2_body(a, s.cond_scale, ph_half_lambda(s, a.w), total);
}

// ---- dmh_photo_energy: fp64 partial sums in a fixed order (grid (splits, B)), then one thread per row adds them in split order
static int energy_splits(int B, int H, int W) {
  const int64_t want = cdiv64((int64_t)H * W, E_CHUNK), cap = E_MAX_WG / B > 1 ? E_MAX_WG / B : 1;
  return (int)(want < cap ? want : cap);
}

__global__ __launch_bounds__(ET) void photo_energy_partial_kernel(const float* __restrict__ x, const float* __restrict__ flow,
                                                                  const float* __restrict__ mask, double* __restrict__ ws, int H,
                                                                  int W) {
  __shared__ double part[ET / 64];
  const int tid = threadIdx.x, split = blockIdx.x, splits = gridDim.x, b = blockIdx.y, hw = H * W;
  const int chunk = (hw + splits - 1) / splits;
  const int lo = split * chunk, hi = lo + chunk < hw ? lo + chunk : hw;
  const float* xb = x + (size_t)b * 6 * hw;
  double acc = 0.;
  for (int p = lo + tid; p < hi; p += ET) {
    const float m = mask[(size_t)b * hw + p];
    if (m == 0.f) continue;
    const FlowWarpTaps t = ph_taps(flow, b, p, H, W);
    double e = 0.;
    for (int c = 0; c < 3; ++c) {
      const float* x2 = xb + (size_t)(3 + c) * hw;
      double u = (double)x2[(size_t)t.y0 * W + t.x0] * (double)t.wnw;
      if (t.x1ok) u += (double)x2[(size_t)t.y0 * W + t.x1] * (double)t.wne;
      if (t.y1ok) u += (double)x2[(size_t)t.y1 * W + t.x0] * (double)t.wsw;
      if (t.x1ok && t.y1ok) u += (double)x2[(size_t)t.y1 * W + t.x1] * (double)t.wse;
      const double d = u - (double)xb[(size_t)c * hw + p];
      e += d * d;
    }
    acc += (double)m * e;
  }
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off);
  if ((tid & 63) == 0) part[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) ws[(size_t)b * splits + split] = ((part[0] + part[1]) + part[2]) + part[3];
}

__global__ __launch_bounds__(64) void photo_energy_finish_kernel(const double* __restrict__ ws, double* __restrict__ E, int B,
                                                                 int splits, double count) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  double sum = 0.;
  for (int j = 0; j < splits; ++j) sum += ws[(size_t)b * splits + j];
  E[b] = sum / count;
}

// ---- entry points
static bool dims_ok(const char* who, int B, int H, int W) {
  // p, q and H * W are ints in the kernels and B is a grid dimension: H * W <= 2^24 keeps 6 * H * W inside them
  if (B < 1 || B > 65535 || H < 2 || W < 2 || (int64_t)H * W > ((int64_t)1 << 24)) {
    dmh_set_error("%s: B=%d samples of %d x %d pixels (1 <= B <= 65535, H >= 2 and W >= 2: the warp divides by W - 1; H * W <= 2^24)",
                  who, B, H, W);
    return false;
  }
  return true;
}

static bool overlaps(const void* a, const void* b, uintptr_t bytes) {
  const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
  return b && pa < pb + bytes && pb < pa + bytes;
}

extern "C" int64_t dmh_photo_acc_words(int B, int H, int W) {
  return dims_ok("dmh_photo_acc_words", B, H, W) ? (int64_t)3 * B * H * W : -1;
}

extern "C" int dmh_photo_energy_splits(int B, int H, int W) {
  return dims_ok("dmh_photo_energy_splits", B, H, W) ? energy_splits(B, H, W) : -1;
}

extern "C" int dmh_photo_weights(const float* flow, const float* mask, uint64_t* acc, float* s, int B, int H, int W, void* stream) {
  DMH_REQUIRE(flow && mask && acc && s, "dmh_photo_weights: null pointer");
  if (!dims_ok("dmh_photo_weights", B, H, W)) return DMH_EINVAL;
  const int hw = H * W;
  const int64_t total = (int64_t)B * hw;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(photo_weights_scatter_kernel, dim3((unsigned)cdiv(hw, 256), (unsigned)B), dim3(256), 0, st, flow, mask,
                     (u64*)acc, H, W);
  DMH_CHECK_LAUNCH("dmh_photo_weights(scatter)");
  hipLaunchKernelGGL(photo_weights_finish_kernel, dim3((unsigned)cdiv64(total, 256)), dim3(256), 0, st, (u64*)acc, s, total);
  DMH_CHECK_LAUNCH("dmh_photo_weights(finish)");
  return DMH_OK;
}

static int guide_checks(const char* who, const void* s, const PhotoArgs& a, int B) {
  if (!s || !a.mc || !a.flow || !a.mask || !a.sw || !a.acc || !a.guided) {
    dmh_set_error("%s: null pointer", who);
    return DMH_EINVAL;
  }
  if (a.keep && !a.mn) {
    dmh_set_error("%s: keep needs model_null", who);
    return DMH_EINVAL;
  }
  if (!dims_ok(who, B, a.H, a.W)) return DMH_EINVAL;
  if (!(a.w > 0.f && a.w <= 1.f)) {
    dmh_set_error("%s: w=%g outside (0, 1] (the step is a descent of the energy for lambda = w * abar_t in (0, 1] only)", who,
                  (double)a.w);
    return DMH_EINVAL;
  }
  const uintptr_t bytes = (uintptr_t)B * 6u * (uintptr_t)a.H * (uintptr_t)a.W * 4u;
  if (overlaps(a.guided, a.mc, bytes) || overlaps(a.guided, a.mn, bytes)) {
    dmh_set_error("%s: guided overlaps an input (model_cond or model_null)", who);
    return DMH_EINVAL;
  }
  return DMH_OK;
}

static PhotoArgs photo_args(const float* mc, const float* mn, const uint8_t* keep, const float* flow, const float* mask,
                            const float* sw, float w, uint64_t* acc, float* guided, int H, int W) {
  PhotoArgs a;
  a.mc = mc, a.mn = mn, a.keep = keep, a.flow = flow, a.mask = mask, a.sw = sw;
  a.acc = (u64*)acc, a.guided = guided, a.w = w, a.H = H, a.W = W;
  return a;
}

extern "C" int dmh_photo_guide(const DmhStep* s, const float* model_cond, const float* model_null, const uint8_t* keep,
                               const float* flow, const float* mask, const float* sw, float w, uint64_t* acc, float* guided, int B,
                               int H, int W, void* stream) {
  const PhotoArgs a = photo_args(model_cond, model_null, keep, flow, mask, sw, w, acc, guided, H, W);
  const int rc = guide_checks("dmh_photo_guide", s, a, B);
  if (rc != DMH_OK) return rc;
  const int hw = H * W;
  const int64_t total = (int64_t)B * 3 * hw;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(photo_im1_kernel, dim3((unsigned)cdiv(hw, 256), (unsigned)B), dim3(256), 0, st, *s, a);
  DMH_CHECK_LAUNCH("dmh_photo_guide(im1)");
  hipLaunchKernelGGL(photo_im2_kernel, dim3((unsigned)cdiv64(total, 256)), dim3(256), 0, st, *s, a, total);
  DMH_CHECK_LAUNCH("dmh_photo_guide(im2)");
  return DMH_OK;
}

extern "C" int dmh_photo_guide_dev(const DmhStep* cur_dev, const float* model_cond, const float* model_null, const uint8_t* keep,
                                   const float* flow, const float* mask, const float* sw, float w, uint64_t* acc, float* guided,
                                   int B, int H, int W, void* stream) {
  const PhotoArgs a = photo_args(model_cond, model_null, keep, flow, mask, sw, w, acc, guided, H, W);
  const int rc = guide_checks("dmh_photo_guide_dev", cur_dev, a, B);
  if (rc != DMH_OK) return rc;
  const int hw = H * W;
  const int64_t total = (int64_t)B * 3 * hw;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(photo_im1_dev_kernel, dim3((unsigned)cdiv(hw, 256), (unsigned)B), dim3(256), 0, st, cur_dev, a);
  DMH_CHECK_LAUNCH("dmh_photo_guide_dev(im1)");
  hipLaunchKernelGGL(photo_im2_dev_kernel, dim3((unsigned)cdiv64(total, 256)), dim3(256), 0, st, cur_dev, a, total);
  DMH_CHECK_LAUNCH("dmh_photo_guide_dev(im2)");
  return DMH_OK;
}

extern "C" int dmh_photo_energy(const float* x, const float* flow, const float* mask, double* ws, double* E, int B, int H, int W,
                                void* stream) {
  DMH_REQUIRE(x && flow && mask && ws && E, "dmh_photo_energy: null pointer");
  if (!dims_ok("dmh_photo_energy", B, H, W)) return DMH_EINVAL;
  const int splits = energy_splits(B, H, W);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(photo_energy_partial_kernel, dim3((unsigned)splits, (unsigned)B), dim3(ET), 0, st, x, flow, mask, ws, H, W);
  DMH_CHECK_LAUNCH("dmh_photo_energy(partials)");
  hipLaunchKernelGGL(photo_energy_finish_kernel, dim3((unsigned)cdiv(B, 64)), dim3(64), 0, st, (const double*)ws, E, B, splits,
                     3.0 * (double)H * (double)W);
  DMH_CHECK_LAUNCH("dmh_photo_energy(finish)");
  return DMH_OK;
}
