// Guidance rescale of the conditional sampler (Lin et al. 2024, "Common Diffusion Noise Schedules and Sample Steps are
// Flawed", 3.4; not in the reference): per sample, the guided blend is brought back to the standard deviation of the
// conditional logits and mixed by a factor phi.  The definition (include/dmhomo_hip.h states it too), per row b of n values:
//   mo_c[i] = model_cond[i], or model_null[i] where keep[b] == 0          (the conditional logit as guided_logit reads it)
//   cfg[i]  = nl + (mo_c - nl) * cond_scale                               (guided_logit's own fp32 expression)
//   ratio   = std(mo_c) / std(cfg) over the row (population), 1 where std(cfg) == 0
//   g[b]    = 1 + phi * (ratio - 1), rounded to fp32 once
// and every step kernel here works on guided_logit(...) * g[b].  A row whose cond equals its null bitwise has cfg == mo_c, so
// ratio == 1 and g == 1.0f exactly; a NaN or an infinity in a row makes that row's g NaN and no other's.
#include "common.h"

#pragma clang fp contract(off)
#include "sampler_dev.h"

// ---- dmh_guidance_factor: two launches, no atomics, no arrival counter: the result is a pure function of the inputs.
// Pass A: grid (B, splits), split j of row b covers the elements [j * chunk, min(n, (j + 1) * chunk)) and writes the mean and
// the sum of squared deviations (M2) of mo_c and of cfg over them.  Each thread sums x - K and (x - K)^2 in fp64, K = the
// split's first element (so a constant split sums exact zeros, and an offset row loses nothing to E[x^2] - mean^2); the
// threads of a wave combine by shuffles, the four waves through LDS in wave order.  Pass B: one thread per row merges the
// row's partials in split order (Chan et al.'s pairwise update) and writes g.
constexpr int GT = 256;            // threads of a pass A workgroup
constexpr int64_t G_CHUNK = 4096;  // elements a workgroup should at least own: 4 float4 per thread and tensor
constexpr int G_MAX_WG = 1024;     // workgroups of pass A over all rows: 4 per CU

static int guidance_splits(int B, int64_t n) {
  const int64_t want = cdiv64(n, G_CHUNK), cap = G_MAX_WG / B > 1 ? G_MAX_WG / B : 1;
  return (int)(want < cap ? want : cap);
}

// elements per split: a multiple of 4, so that every split of a row meets the same 16 B phase
__host__ __device__ __forceinline__ int64_t guidance_chunk(int64_t n, int splits) {
  return ((n + splits - 1) / splits + 3) / 4 * 4;
}

struct GuidanceSums {
  double s1c, s2c, s1g, s2g;   // sums of (mo_c - Kc), (mo_c - Kc)^2, (cfg - Kg), (cfg - Kg)^2
};

__device__ __forceinline__ void guidance_add(GuidanceSums& a, float mo, float nl, float cond_scale, double kc, double kg) {
  const float cf = guided_blend(mo, nl, cond_scale);
  const double dc = (double)mo - kc, dg = (double)cf - kg;
  a.s1c += dc;
  a.s2c += dc * dc;
  a.s1g += dg;
  a.s2g += dg * dg;
}

// mean and M2 of cnt values from their shifted sums; a negative M2 can only be rounding (NaN stays NaN)
__device__ __forceinline__ void guidance_moments(double k, double s1, double s2, double cnt, double* out) {
  const double m2 = s2 - s1 * s1 / cnt;
  out[0] = k + s1 / cnt;
  out[1] = m2 < 0. ? 0. : m2;
}

__device__ __forceinline__ void guidance_partial_body(float cond_scale, const float* mc, const float* mn, const uint8_t* keep,
                                                      double* ws, int64_t n) {
  __shared__ double part[GT / 64][4];
  const int tid = threadIdx.x, b = blockIdx.x, split = blockIdx.y, splits = gridDim.y;
  const int64_t chunk = guidance_chunk(n, splits);
  const int64_t lo = (int64_t)split * chunk;
  const int64_t cnt = n - lo < chunk ? n - lo : chunk;
  double* out = ws + ((size_t)b * splits + split) * 4;
  if (cnt <= 0) {   // (an empty split: pass B skips it by its count)
    if (tid < 4) out[tid] = 0.;
    return;
  }
  const bool kept = !keep || keep[b];   // a dropped row's conditional logits ARE its null logits: model_cond is not read
  const float* pn = mn + (size_t)b * (size_t)n + lo;
  const float* pc = kept ? mc + (size_t)b * (size_t)n + lo : pn;
  const float nl0 = pn[0], mo0 = pc[0];
  const double kc = (double)mo0, kg = (double)guided_blend(mo0, nl0, cond_scale);
  GuidanceSums a = {0., 0., 0., 0.};
  if ((((uintptr_t)pn ^ (uintptr_t)pc) & 15u) == 0) {   // both rows meet 16 B boundaries together: scalar head, float4, tail
    int64_t head = (int64_t)(((16u - (unsigned)((uintptr_t)pn & 15u)) & 15u) >> 2);
    head = head < cnt ? head : cnt;
    const int64_t nv = (cnt - head) >> 2;
    if (tid < head) guidance_add(a, pc[tid], pn[tid], cond_scale, kc, kg);
    const float4* vn = reinterpret_cast<const float4*>(pn + head);
    const float4* vc = reinterpret_cast<const float4*>(pc + head);
    for (int64_t i = tid; i < nv; i += GT) {
      const float4 qn = vn[i], qc = vc[i];
      guidance_add(a, qc.x, qn.x, cond_scale, kc, kg);
      guidance_add(a, qc.y, qn.y, cond_scale, kc, kg);
      guidance_add(a, qc.z, qn.z, cond_scale, kc, kg);
      guidance_add(a, qc.w, qn.w, cond_scale, kc, kg);
    }
    const int64_t t0 = head + nv * 4;
    if (tid < cnt - t0) guidance_add(a, pc[t0 + tid], pn[t0 + tid], cond_scale, kc, kg);
  } else {
    for (int64_t i = tid; i < cnt; i += GT) guidance_add(a, pc[i], pn[i], cond_scale, kc, kg);
  }
  for (int off = 32; off > 0; off >>= 1) {
    a.s1c += __shfl_down(a.s1c, off);
    a.s2c += __shfl_down(a.s2c, off);
    a.s1g += __shfl_down(a.s1g, off);
    a.s2g += __shfl_down(a.s2g, off);
  }
  if ((tid & 63) == 0) {
    double* p = part[tid >> 6];
    p[0] = a.s1c, p[1] = a.s2c, p[2] = a.s1g, p[3] = a.s2g;
  }
  __syncthreads();
  if (tid == 0) {
    double s[4];
    for (int j = 0; j < 4; ++j) s[j] = ((part[0][j] + part[1][j]) + part[2][j]) + part[3][j];
    guidance_moments(kc, s[0], s[1], (double)cnt, out);
    guidance_moments(kg, s[2], s[3], (double)cnt, out + 2);
  }
}

__global__ __launch_bounds__(GT) void guidance_partial_kernel(DmhStep s, const float* __restrict__ mc,
                                                              const float* __restrict__ mn, const uint8_t* __restrict__ keep,
                                                              double* __restrict__ ws, int64_t n) {
  guidance_partial_body(s.cond_scale, mc, mn, keep, ws, n);
}

__global__ __launch_bounds__(GT) void guidance_partial_dev_kernel(const DmhStep* __restrict__ sp, const float* __restrict__ mc,
                                                                  const float* __restrict__ mn,
                                                                  const uint8_t* __restrict__ keep, double* __restrict__ ws,
                                                                  int64_t n) {
  guidance_partial_body(sp->cond_scale, mc, mn, keep, ws, n);
}

// (mean, M2) of na values <- merged with (mb, m2b) of nb values
__device__ __forceinline__ void guidance_merge(double& ma, double& m2a, double na, double mb, double m2b, double nb) {
  const double delta = mb - ma, tot = na + nb;
  ma = ma + delta * nb / tot;
  m2a = (m2a + m2b) + delta * delta * na * nb / tot;
}

__global__ __launch_bounds__(64) void guidance_finish_kernel(const double* __restrict__ ws, float phi, float* __restrict__ gfac,
                                                             int B, int64_t n, int splits) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  const int64_t chunk = guidance_chunk(n, splits);
  const double* p = ws + (size_t)b * splits * 4;
  double na = 0., mc = 0., m2c = 0., mg = 0., m2g = 0.;
  for (int j = 0; j < splits; ++j, p += 4) {
    const int64_t left = n - (int64_t)j * chunk;
    if (left <= 0) break;
    const double nb = (double)(left < chunk ? left : chunk);
    if (j == 0) {
      mc = p[0], m2c = p[1], mg = p[2], m2g = p[3];
    } else {
      guidance_merge(mc, m2c, na, p[0], p[1], nb);
      guidance_merge(mg, m2g, na, p[2], p[3], nb);
    }
    na += nb;
  }
  // population variances M2 / n: only their ratio is used.  m2g == 0 (a constant row, n == 1): nothing to rescale
  const double ratio = m2g == 0. ? 1. : sqrt(m2c / m2g);
  gfac[b] = (float)(1. + (double)phi * (ratio - 1.));
}

// ---- the step kernels with the factor: guided_logit(...) * g[row] in guided_logit's place, everything behind it unchanged
__device__ __forceinline__ void x0_raw_gr_body(const DmhStep& s, const float* mc, const float* mn, const float* x,
                                               const float* gfac, float* x0_raw, int64_t total, const uint8_t* keep,
                                               int64_t per_row) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256)
    x0_raw[i] = raw_x_start(s, rescaled_guided_logit(mc, mn, keep, i, per_row, s.cond_scale, gfac), x[i]);
}

__global__ __launch_bounds__(256) void x0_raw_gr_kernel(DmhStep s, const float* __restrict__ mc, const float* __restrict__ mn,
                                                        const float* __restrict__ x, const float* __restrict__ gfac,
                                                        float* __restrict__ x0_raw, int64_t total,
                                                        const uint8_t* __restrict__ keep, int64_t per_row) {
  x0_raw_gr_body(s, mc, mn, x, gfac, x0_raw, total, keep, per_row);
}

__global__ __launch_bounds__(256) void x0_raw_gr_dev_kernel(const DmhStep* __restrict__ sp, const float* __restrict__ mc,
                                                            const float* __restrict__ mn, const float* __restrict__ x,
                                                            const float* __restrict__ gfac, float* __restrict__ x0_raw,
                                                            int64_t total, const uint8_t* __restrict__ keep, int64_t per_row) {
  const DmhStep s = *sp;
  x0_raw_gr_body(s, mc, mn, x, gfac, x0_raw, total, keep, per_row);
}

// step_thr_body of threshold.hip with the factor; thr == nullptr: the static clamp (denoise_step itself).  No __restrict__ on
// x / img_out (in place: every element is read by the thread that writes it) nor on hist (read, then written, by one thread)
__device__ __forceinline__ void step_gr_body(const DmhStep& s, const float* mc, const float* mn, const float* x,
                                             const float* noise, float* hist, const float* thr, const float* gfac,
                                             float* img_out, float* x_start, int64_t total, const uint8_t* keep,
                                             int64_t per_row, float missing) {
  const bool history = hist && reads_history(s);
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const float mo = rescaled_guided_logit(mc, mn, keep, i, per_row, s.cond_scale, gfac);
    const float nz = (noise && s.mode != 1) ? noise[i] : missing;
    const float prev = history ? hist[i] : missing;
    float x0, pn, o;
    if (thr) {
      const float t = s.clip ? thr[i / per_row] : 1.f;
      denoise_step_t<true>(s, mo, x[i], nz, noise != nullptr, prev, t, x0, pn, o);
    } else {
      denoise_step(s, mo, x[i], nz, noise != nullptr, prev, x0, pn, o);
    }
    img_out[i] = o;
    if (x_start) x_start[i] = x0;
    if (hist) hist[i] = x0;
  }
}

__global__ __launch_bounds__(256) void step_gr_kernel(DmhStep s, const float* __restrict__ mc, const float* __restrict__ mn,
                                                      const float* x, const float* __restrict__ noise, float* hist,
                                                      const float* __restrict__ thr, const float* __restrict__ gfac,
                                                      float* img_out, float* __restrict__ x_start, int64_t total,
                                                      const uint8_t* __restrict__ keep, int64_t per_row) {
  step_gr_body(s, mc, mn, x, noise, hist, thr, gfac, img_out, x_start, total, keep, per_row, __builtin_nanf(""));
}

// (the device-resident entry cannot be checked at launch: an entry that needs noise or history it was not given yields NaN)
__global__ __launch_bounds__(256) void step_gr_dev_kernel(const DmhStep* __restrict__ sp, const float* __restrict__ mc,
                                                          const float* __restrict__ mn, const float* x,
                                                          const float* __restrict__ noise, float* hist,
                                                          const float* __restrict__ thr, const float* __restrict__ gfac,
                                                          float* img_out, float* __restrict__ x_start, int64_t total,
                                                          const uint8_t* __restrict__ keep, int64_t per_row) {
  const DmhStep s = *sp;
  step_gr_body(s, mc, mn, x, noise, hist, thr, gfac, img_out, x_start, total, keep, per_row, __builtin_nanf(""));
}

static unsigned grid_for(int64_t n) {
  const int64_t g = cdiv64(n, 256);
  return (unsigned)(g < 16384 ? (g > 0 ? g : 1) : 16384);
}

static bool rows_ok(const char* who, int B, int64_t n) {
  if (B < 1 || n < 1 || n >= ((int64_t)1 << 31)) {
    dmh_set_error("%s: B=%d rows of n=%lld elements (B >= 1, 1 <= n < 2^31)", who, B, (long long)n);
    return false;
  }
  return true;
}

extern "C" int dmh_guidance_splits(int B, int64_t n) {
  return rows_ok("dmh_guidance_splits", B, n) ? guidance_splits(B, n) : -1;
}

static int factor_checks(const char* who, const void* s, const float* mc, const float* mn, const uint8_t* keep, float phi,
                         const double* ws, const float* gfac, int B, int64_t n) {
  if (!s || !mc || !ws || !gfac) {
    dmh_set_error("%s: null pointer", who);
    return DMH_EINVAL;
  }
  if (!mn) {
    dmh_set_error(keep ? "%s: keep needs model_null" : "%s: model_null is NULL (without a null pass there is nothing to rescale)",
                  who);
    return DMH_EINVAL;
  }
  if (!rows_ok(who, B, n)) return DMH_EINVAL;
  if (!(phi >= 0.f && phi <= 1.f)) {
    dmh_set_error("%s: phi=%g outside [0, 1]", who, (double)phi);
    return DMH_EINVAL;
  }
  return DMH_OK;
}

extern "C" int dmh_guidance_factor(const DmhStep* s, const float* model_cond, const float* model_null, const uint8_t* keep,
                                   float phi, double* ws, float* gfac, int B, int64_t n, void* stream) {
  const int rc = factor_checks("dmh_guidance_factor", s, model_cond, model_null, keep, phi, ws, gfac, B, n);
  if (rc != DMH_OK) return rc;
  const int splits = guidance_splits(B, n);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(guidance_partial_kernel, dim3((unsigned)B, (unsigned)splits), dim3(GT), 0, st, *s, model_cond, model_null,
                     keep, ws, n);
  DMH_CHECK_LAUNCH("dmh_guidance_factor(partials)");
  hipLaunchKernelGGL(guidance_finish_kernel, dim3((unsigned)cdiv(B, 64)), dim3(64), 0, st, (const double*)ws, phi, gfac, B, n,
                     splits);
  DMH_CHECK_LAUNCH("dmh_guidance_factor(finish)");
  return DMH_OK;
}

extern "C" int dmh_guidance_factor_dev(const DmhStep* cur_dev, const float* model_cond, const float* model_null,
                                       const uint8_t* keep, float phi, double* ws, float* gfac, int B, int64_t n,
                                       void* stream) {
  const int rc = factor_checks("dmh_guidance_factor_dev", cur_dev, model_cond, model_null, keep, phi, ws, gfac, B, n);
  if (rc != DMH_OK) return rc;
  const int splits = guidance_splits(B, n);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(guidance_partial_dev_kernel, dim3((unsigned)B, (unsigned)splits), dim3(GT), 0, st, cur_dev, model_cond,
                     model_null, keep, ws, n);
  DMH_CHECK_LAUNCH("dmh_guidance_factor_dev(partials)");
  hipLaunchKernelGGL(guidance_finish_kernel, dim3((unsigned)cdiv(B, 64)), dim3(64), 0, st, (const double*)ws, phi, gfac, B, n,
                     splits);
  DMH_CHECK_LAUNCH("dmh_guidance_factor_dev(finish)");
  return DMH_OK;
}

static int threshold_gr_checks(const char* who, const void* s, const float* mc, const float* mn, const float* x,
                               const float* gfac, const float* x0_raw, const float* thr, int B, int64_t n, const uint8_t* keep) {
  if (!s || !mc || !x || !gfac || !x0_raw || !thr) {
    dmh_set_error("%s: null pointer", who);
    return DMH_EINVAL;
  }
  if (!rows_ok(who, B, n)) return DMH_EINVAL;
  if (keep && !mn) {
    dmh_set_error("%s: keep needs model_null", who);
    return DMH_EINVAL;
  }
  return DMH_OK;
}

// dmh_sampler_threshold[_dev] of threshold.hip with the factor: the raw x_start of the rescaled logits into the scratch, then
// the selector as it stands (dmh_row_quantile_abs launches row_quantile_abs_kernel with floor 1)
extern "C" int dmh_sampler_threshold_gr(const DmhStep* s, const float* model_cond, const float* model_null, const float* x,
                                        const uint8_t* keep, const float* gfac, float* x0_raw, float* thr, int B, int64_t n,
                                        int64_t k, float frac, void* stream) {
  const int rc = threshold_gr_checks("dmh_sampler_threshold_gr", s, model_cond, model_null, x, gfac, x0_raw, thr, B, n, keep);
  if (rc != DMH_OK) return rc;
  DMH_REQUIRE(s->objective >= 0 && s->objective <= 2, "dmh_sampler_threshold_gr: bad enum (objective)");
  DMH_REQUIRE(k >= 0 && k < n && frac >= 0.f && frac < 1.f && (frac == 0.f || k + 1 < n),
              "dmh_sampler_threshold_gr: rank k=%lld + frac=%g outside a row of n=%lld elements", (long long)k, (double)frac,
              (long long)n);
  const int64_t total = (int64_t)B * n;   // (B < 2^31, n < 2^31)
  hipLaunchKernelGGL(x0_raw_gr_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, *s, model_cond, model_null, x,
                     gfac, x0_raw, total, keep, n);
  DMH_CHECK_LAUNCH("dmh_sampler_threshold_gr(x0_raw)");
  return dmh_row_quantile_abs(x0_raw, thr, B, n, k, frac, 1.f, stream);
}

extern "C" int dmh_sampler_threshold_gr_dev(const DmhStep* cur_dev, const float* model_cond, const float* model_null,
                                            const float* x, const uint8_t* keep, const float* gfac, float* x0_raw, float* thr,
                                            int B, int64_t n, int64_t k, float frac, void* stream) {
  const int rc = threshold_gr_checks("dmh_sampler_threshold_gr_dev", cur_dev, model_cond, model_null, x, gfac, x0_raw, thr, B, n,
                                     keep);
  if (rc != DMH_OK) return rc;
  DMH_REQUIRE(k >= 0 && k < n && frac >= 0.f && frac < 1.f && (frac == 0.f || k + 1 < n),
              "dmh_sampler_threshold_gr_dev: rank k=%lld + frac=%g outside a row of n=%lld elements", (long long)k, (double)frac,
              (long long)n);
  const int64_t total = (int64_t)B * n;
  hipLaunchKernelGGL(x0_raw_gr_dev_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, cur_dev, model_cond,
                     model_null, x, gfac, x0_raw, total, keep, n);
  DMH_CHECK_LAUNCH("dmh_sampler_threshold_gr_dev(x0_raw)");
  return dmh_row_quantile_abs(x0_raw, thr, B, n, k, frac, 1.f, stream);
}

static int step_gr_checks(const char* who, const void* s, const float* mc, const float* mn, const float* x, const float* noise,
                          const float* hist, const float* gfac, const float* img_out, int64_t total, const uint8_t* keep,
                          int64_t per_row) {
  if (!s || !mc || !x || !gfac || !img_out) {
    dmh_set_error("%s: null pointer", who);
    return DMH_EINVAL;
  }
  if (total < 1 || per_row < 1 || total % per_row != 0) {
    dmh_set_error("%s: n=%lld elements in rows of per_row=%lld (gfac holds one value per row)", who, (long long)total,
                  (long long)per_row);
    return DMH_EINVAL;
  }
  if (keep && !mn) {
    dmh_set_error("%s: keep needs model_null", who);
    return DMH_EINVAL;
  }
  if (noise && hist) {
    dmh_set_error("%s: noise (a DDIM entry) and hist (a multistep entry) exclude each other", who);
    return DMH_EINVAL;
  }
  return DMH_OK;
}

extern "C" int dmh_sampler_step_gr(const DmhStep* s, const float* model_cond, const float* model_null, const float* x,
                                   const float* noise, float* hist, const float* thr, const float* gfac, float* img_out,
                                   float* x_start, int64_t n, const uint8_t* keep, int64_t per_row, void* stream) {
  const int rc = step_gr_checks("dmh_sampler_step_gr", s, model_cond, model_null, x, noise, hist, gfac, img_out, n, keep, per_row);
  if (rc != DMH_OK) return rc;
  DMH_REQUIRE(s->objective >= 0 && s->objective <= 2 && (s->mode == 0 || s->mode == 1 || s->mode == 3),
              "dmh_sampler_step_gr: bad enum (mode: 0 DDIM, 1 last step or 3 multistep)");
  DMH_REQUIRE(s->mode != 0 || noise, "dmh_sampler_step_gr: DDIM update needs noise");
  DMH_REQUIRE(s->mode != 3 || hist, "dmh_sampler_step_gr: multistep update needs hist");
  hipLaunchKernelGGL(step_gr_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, *s, model_cond, model_null, x, noise,
                     hist, thr, gfac, img_out, x_start, n, keep, per_row);
  DMH_CHECK_LAUNCH("dmh_sampler_step_gr");
  return DMH_OK;
}

extern "C" int dmh_sampler_step_gr_dev(const DmhStep* cur_dev, const float* model_cond, const float* model_null, const float* x,
                                       const float* noise, float* hist, const float* thr, const float* gfac, float* img_out,
                                       float* x_start, int64_t n, const uint8_t* keep, int64_t per_row, void* stream) {
  const int rc = step_gr_checks("dmh_sampler_step_gr_dev", cur_dev, model_cond, model_null, x, noise, hist, gfac, img_out, n, keep,
                                per_row);
  if (rc != DMH_OK) return rc;
  hipLaunchKernelGGL(step_gr_dev_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, cur_dev, model_cond, model_null, x,
                     noise, hist, thr, gfac, img_out, x_start, n, keep, per_row);
  DMH_CHECK_LAUNCH("dmh_sampler_step_gr_dev");
  return DMH_OK;
}

// ---- Guidance interval (Kynkaanniemi et al. 2024, "Applying Guidance in a Limited Interval Improves Sample and Distribution
// Quality in Diffusion Models"; not in the reference): ONE captured denoise step serves guided and unguided entries.  The host
// writes guided [S] (uint8, one flag per entry of the step table) and the step cursor of dmh_sampler_seek selects the entry;
// both new kernels read the flag with one uniform load.  A cursor outside [0, S) counts as guided: the full work, and no read
// outside the table.
__device__ __forceinline__ bool entry_guided(const int32_t* cursor, const uint8_t* guided, int S) {
  const int c = *cursor;
  return c < 0 || c >= S || guided[c] != 0;
}

// dmh_rows_from_keep with the flag in front of it (one wave, the same ballot compaction, ascending).  Guided: the conditional
// side lists the rows with keep != 0 (all B without keep), the null-only side all B, both followed by B .. B + extra - 1.
// Unguided: the conditional side lists ALL B rows (a dropped row has no null row to borrow from) and no extras, the null-only
// side nothing.  Slots behind 1 + n stay unwritten.
__global__ __launch_bounds__(64) void rows_gated_kernel(const uint8_t* __restrict__ keep, int B, int extra,
                                                        const int32_t* __restrict__ cursor,
                                                        const uint8_t* __restrict__ guided, int S, int null_side,
                                                        int32_t* __restrict__ rows) {
  const bool on = entry_guided(cursor, guided, S);
  if (!on && null_side) {
    if (threadIdx.x == 0) rows[0] = 0;
    return;
  }
  const bool masked = on && !null_side && keep;
  int n = 0;
  for (int b0 = 0; b0 < B; b0 += 64) {
    const int b = b0 + (int)threadIdx.x;
    const bool k = b < B && (!masked || keep[b] != 0);
    const unsigned long long m = __ballot(k);
    if (k) rows[1 + n + __popcll(m & ((1ull << threadIdx.x) - 1ull))] = b;
    n += __popcll(m);
  }
  const int ex = on ? extra : 0;
  for (int j = threadIdx.x; j < ex; j += 64) rows[1 + n + j] = B + j;
  if (threadIdx.x == 0) rows[0] = n + ex;
}

extern "C" int dmh_rows_gated(const uint8_t* keep, int B, int extra, const int32_t* cursor, const uint8_t* guided, int S,
                              int null_side, int32_t* rows, void* stream) {
  DMH_REQUIRE(cursor && guided && rows, "dmh_rows_gated: null pointer");
  DMH_REQUIRE(B > 0 && extra >= 0 && S > 0 && (int64_t)B + extra < ((int64_t)1 << 31),
              "dmh_rows_gated: B=%d rows, extra=%d, S=%d entries (B >= 1, extra >= 0, S >= 1)", B, extra, S);
  DMH_REQUIRE(null_side == 0 || null_side == 1, "dmh_rows_gated: null_side=%d (0 conditional side, 1 null-only side)", null_side);
  hipLaunchKernelGGL(rows_gated_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, keep, B, extra, cursor, guided, S, null_side,
                     rows);
  DMH_CHECK_LAUNCH("dmh_rows_gated");
  return DMH_OK;
}

// The gate behind the network.  Guided entry: every workgroup returns before it touches cond or null.  Unguided entry: null <-
// cond, bit for bit (32-bit words, no floating-point instruction sees them).  Where the two pointers meet 16 B boundaries
// together: a scalar head up to the boundary, 16 B vectors, a scalar tail; else words.
__global__ __launch_bounds__(256) void guidance_gate_kernel(const int32_t* __restrict__ cursor, const uint8_t* __restrict__ guided,
                                                            int S, const uint32_t* __restrict__ cond, uint32_t* __restrict__ null,
                                                            int64_t n) {
  if (entry_guided(cursor, guided, S)) return;
  const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, stride = (int64_t)gridDim.x * 256;
  if ((((uintptr_t)cond ^ (uintptr_t)null) & 15u) != 0) {
    for (int64_t i = tid; i < n; i += stride) null[i] = cond[i];
    return;
  }
  int64_t head = (int64_t)(((16u - (unsigned)((uintptr_t)null & 15u)) & 15u) >> 2);
  head = head < n ? head : n;
  const int64_t nv = (n - head) >> 2, t0 = head + nv * 4;
  if (tid < head) null[tid] = cond[tid];
  const uint4* vc = reinterpret_cast<const uint4*>(cond + head);
  uint4* vn = reinterpret_cast<uint4*>(null + head);
  for (int64_t i = tid; i < nv; i += stride) vn[i] = vc[i];
  if (tid < n - t0) null[t0 + tid] = cond[t0 + tid];
}

extern "C" int dmh_guidance_gate(const int32_t* cursor, const uint8_t* guided, int S, const float* cond, float* null, int64_t n,
                                 void* stream) {
  DMH_REQUIRE(cursor && guided && cond && null, "dmh_guidance_gate: null pointer");
  DMH_REQUIRE(n > 0 && S > 0, "dmh_guidance_gate: n=%lld elements, S=%d entries (n >= 1, S >= 1)", (long long)n, S);
  DMH_REQUIRE((((uintptr_t)cond | (uintptr_t)null) & 3u) == 0, "dmh_guidance_gate: cond / null are not 4-byte aligned");
  DMH_REQUIRE(n < ((int64_t)1 << 40), "dmh_guidance_gate: n=%lld elements (limit 2^40)", (long long)n);
  const uintptr_t pc = (uintptr_t)cond, pn = (uintptr_t)null, bytes = (uintptr_t)n * 4u;
  DMH_REQUIRE(pc + bytes <= pn || pn + bytes <= pc, "dmh_guidance_gate: cond and null overlap");
  hipLaunchKernelGGL(guidance_gate_kernel, dim3(grid_for(cdiv64(n, 4))), dim3(256), 0, (hipStream_t)stream, cursor, guided, S,
                     (const uint32_t*)cond, (uint32_t*)null, n);
  DMH_CHECK_LAUNCH("dmh_guidance_gate");
  return DMH_OK;
}
