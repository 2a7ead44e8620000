// Dynamic thresholding of the guided sampler (Saharia et al. 2022, "Imagen", 2.3; not in the reference): per sample, the
// p-th percentile of |x_start| before any clamp — an EXACT order-statistic selection, linearly interpolated as torch.quantile
// does — and the step kernels that clamp to max(1, that) and divide by it instead of clamping to [-1, 1].
#include "common.h"

#pragma clang fp contract(off)
#include "sampler_dev.h"

// ---- dmh_row_quantile_abs: radix select on the bit pattern of |x|.  Non-negative floats order as their uint32 patterns
// (denormals, -0.0 == +0.0 included); NaN patterns sort above infinity and are counted like any value, and a row that holds
// one answers NaN.  One workgroup of 1024 threads per row, three histogram passes over the 31 bits of the key (11 + 10 + 10,
// most significant first) with LDS integer atomics, each followed by a scan that finds the bin holding rank k and narrows the
// key prefix; after the third the key of v[k] is known exactly, with the number of elements below it and equal to it.
// v[k+1] is v[k] when more than k + 1 elements are <= v[k], else the smallest key above it (one more pass, only when frac
// != 0).  Integer counting only: the result does not depend on the order the atomics land in.
constexpr int QT = 1024;       // threads of the workgroup
constexpr int QBINS = 2048;    // bins of the first digit; the other two use the lower 1024

// f(key) for every element of the row, 16 B loads where the row allows them (any order: the callers count or take a minimum)
template <class F>
__device__ __forceinline__ void for_each_key(const float* row, int64_t n, F f) {
  const unsigned* u = reinterpret_cast<const unsigned*>(row);
  const int tid = threadIdx.x;
  int64_t head = (int64_t)(((16u - (unsigned)((uintptr_t)u & 15u)) & 15u) >> 2);   // elements in front of a 16 B boundary
  head = head < n ? head : n;
  const int64_t nv = (n - head) >> 2;
  if (tid < head) f(u[tid] & 0x7fffffffu);
  const uint4* v = reinterpret_cast<const uint4*>(u + head);
  for (int64_t i = tid; i < nv; i += QT) {
    const uint4 q = v[i];
    f(q.x & 0x7fffffffu);
    f(q.y & 0x7fffffffu);
    f(q.z & 0x7fffffffu);
    f(q.w & 0x7fffffffu);
  }
  const int64_t t0 = head + nv * 4;
  if (tid < n - t0) f(u[t0 + tid] & 0x7fffffffu);
}

__global__ __launch_bounds__(QT) void row_quantile_abs_kernel(const float* __restrict__ x, int64_t n, int64_t k, float frac,
                                                              float floor_, float* __restrict__ out) {
  __shared__ unsigned hist[QBINS];
  __shared__ unsigned wsum[QT / 64];
  __shared__ unsigned sel[3];        // the bin that holds the rank, the rank inside it, its count
  __shared__ unsigned has_nan, above;
  const int tid = threadIdx.x;
  const float* row = x + (size_t)blockIdx.x * (size_t)n;
  unsigned prefix = 0, krem = (unsigned)k, cnt = 0;
  if (tid == 0) has_nan = 0u, above = 0xffffffffu;
  for (int pass = 0; pass < 3; ++pass) {
    const int shift = pass == 0 ? 20 : (pass == 1 ? 10 : 0);
    const unsigned dmask = pass == 0 ? 2047u : 1023u;
    const unsigned pmask = pass == 0 ? 0u : (pass == 1 ? 0xfff00000u : 0xfffffc00u);   // the digits already decided
    for (int i = tid; i < QBINS; i += QT) hist[i] = 0u;
    __syncthreads();
    bool nan = false;
    for_each_key(row, n, [&](unsigned key) {
      nan = nan || key > 0x7f800000u;
      if ((key & pmask) == prefix) atomicAdd(&hist[(key >> shift) & dmask], 1u);
    });
    if (pass == 0 && nan) has_nan = 1u;   // (every writer stores the same value)
    __syncthreads();
    // exclusive scan over the bins, two per thread: within a wave by shuffles, across the 16 waves through LDS
    const unsigned h0 = hist[2 * tid], h1 = hist[2 * tid + 1];
    const unsigned c = h0 + h1;
    unsigned incl = c;
    const int lane = tid & 63;
    for (int off = 1; off < 64; off <<= 1) {
      const unsigned t = __shfl_up(incl, off);
      if (lane >= off) incl += t;
    }
    if (lane == 63) wsum[tid >> 6] = incl;
    __syncthreads();
    unsigned base = 0;
    for (int w = 0; w < (tid >> 6); ++w) base += wsum[w];
    const unsigned excl = base + incl - c;
    if (krem >= excl && krem < excl + c) {   // exactly one thread: the bins' counts sum to more than krem
      const bool second = krem >= excl + h0;
      sel[0] = 2u * tid + (second ? 1u : 0u);
      sel[1] = krem - excl - (second ? h0 : 0u);
      sel[2] = second ? h1 : h0;
    }
    __syncthreads();
    prefix |= sel[0] << shift;
    krem = sel[1];
    cnt = sel[2];
    __syncthreads();   // (sel, wsum and hist are free again)
  }
  // prefix: the key of v[k]; k - krem elements lie below it and cnt equal it
  const unsigned akey = prefix;
  unsigned bkey = akey;
  const int64_t le = (k - (int64_t)krem) + (int64_t)cnt;
  if (frac != 0.f && le <= k + 1) {   // v[k+1] is the smallest key above (k + 1 < n: checked at launch)
    unsigned m = 0xffffffffu;
    for_each_key(row, n, [&](unsigned key) { m = key > akey ? (key < m ? key : m) : m; });
    atomicMin(&above, m);
    __syncthreads();
    bkey = above;
  }
  if (tid == 0) {
    const float a = __uint_as_float(akey), b = __uint_as_float(bkey);
    const float q = (frac == 0.f || akey == bkey) ? a : fmaf(b - a, frac, a);
    out[blockIdx.x] = has_nan ? __builtin_nanf("") : fmaxf(floor_, q);
  }
}

// x0_raw[i] = x_start of the entry before any clamp: the guided blend and the objective branch of denoise_step
__device__ __forceinline__ void x0_raw_body(const DmhStep& s, const float* mc, const float* mn, const float* x, float* x0_raw,
                                            int64_t total, const uint8_t* keep, int64_t per_row) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256)
    x0_raw[i] = raw_x_start(s, guided_logit(mc, mn, keep, i, per_row, s.cond_scale), x[i]);
}

__global__ __launch_bounds__(256) void x0_raw_kernel(DmhStep s, const float* __restrict__ mc, const float* __restrict__ mn,
                                                     const float* __restrict__ x, float* __restrict__ x0_raw, int64_t total,
                                                     const uint8_t* __restrict__ keep, int64_t per_row) {
  x0_raw_body(s, mc, mn, x, x0_raw, total, keep, per_row);
}

__global__ __launch_bounds__(256) void x0_raw_dev_kernel(const DmhStep* __restrict__ sp, const float* __restrict__ mc,
                                                         const float* __restrict__ mn, const float* __restrict__ x,
                                                         float* __restrict__ x0_raw, int64_t total,
                                                         const uint8_t* __restrict__ keep, int64_t per_row) {
  const DmhStep s = *sp;
  x0_raw_body(s, mc, mn, x, x0_raw, total, keep, per_row);
}

// sampler_step_body of sampler.hip with a threshold per row: noise and hist are both optional (a DDIM entry reads noise, a
// multistep entry hist).  missing: what stands for either where the entry needs one that was not given.  No __restrict__ on
// x / img_out (in place: every element is read by the thread that writes it) nor on hist (read, then written, by one thread)
__device__ __forceinline__ void step_thr_body(const DmhStep& s, const float* mc, const float* mn, const float* x,
                                              const float* noise, float* hist, const float* thr, float* img_out, float* x_start,
                                              int64_t total, const uint8_t* keep, int64_t per_row, float missing) {
  const bool history = hist && reads_history(s);
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const float mo = guided_logit(mc, mn, keep, i, per_row, s.cond_scale);
    const float nz = (noise && s.mode != 1) ? noise[i] : missing;
    const float prev = history ? hist[i] : missing;
    const float t = s.clip ? thr[i / per_row] : 1.f;
    float x0, pn, o;
    denoise_step_t<true>(s, mo, x[i], nz, noise != nullptr, prev, t, x0, pn, o);
    img_out[i] = o;
    if (x_start) x_start[i] = x0;
    if (hist) hist[i] = x0;
  }
}

__global__ __launch_bounds__(256) void step_thr_kernel(DmhStep s, const float* __restrict__ mc, const float* __restrict__ mn,
                                                       const float* x, const float* __restrict__ noise, float* hist,
                                                       const float* __restrict__ thr, float* img_out,
                                                       float* __restrict__ x_start, int64_t total,
                                                       const uint8_t* __restrict__ keep, int64_t per_row) {
  step_thr_body(s, mc, mn, x, noise, hist, thr, img_out, x_start, total, keep, per_row, __builtin_nanf(""));
}

// (the device-resident entry cannot be checked at launch: an entry that needs noise or history it was not given yields NaN)
__global__ __launch_bounds__(256) void step_thr_dev_kernel(const DmhStep* __restrict__ sp, const float* __restrict__ mc,
                                                           const float* __restrict__ mn, const float* x,
                                                           const float* __restrict__ noise, float* hist,
                                                           const float* __restrict__ thr, float* img_out,
                                                           float* __restrict__ x_start, int64_t total,
                                                           const uint8_t* __restrict__ keep, int64_t per_row) {
  const DmhStep s = *sp;
  step_thr_body(s, mc, mn, x, noise, hist, thr, img_out, x_start, total, keep, per_row, __builtin_nanf(""));
}

static unsigned grid_for(int64_t n) {
  const int64_t g = cdiv64(n, 256);
  return (unsigned)(g < 16384 ? (g > 0 ? g : 1) : 16384);
}

// what every entry point here asks of (B, n, k, frac): rows of 1 .. 2^31 - 1 elements, rank k inside the row, and a v[k+1]
// to interpolate towards wherever frac != 0
static bool quantile_args_ok(const char* who, int B, int64_t n, int64_t k, float frac) {
  if (B < 1 || n < 1 || n >= ((int64_t)1 << 31)) {
    dmh_set_error("%s: B=%d rows of n=%lld elements (B >= 1, 1 <= n < 2^31)", who, B, (long long)n);
    return false;
  }
  if (k < 0 || k >= n || !(frac >= 0.f && frac < 1.f) || (frac != 0.f && k + 1 >= n)) {
    dmh_set_error("%s: rank k=%lld + frac=%g outside a row of n=%lld elements (0 <= k < n, 0 <= frac < 1, k + 1 < n where frac != 0)",
                  who, (long long)k, (double)frac, (long long)n);
    return false;
  }
  return true;
}

extern "C" int dmh_row_quantile_abs(const float* x, float* out, int B, int64_t n, int64_t k, float frac, float floor_,
                                    void* stream) {
  DMH_REQUIRE(x && out, "dmh_row_quantile_abs: null pointer");
  if (!quantile_args_ok("dmh_row_quantile_abs", B, n, k, frac)) return DMH_EINVAL;
  DMH_REQUIRE(floor_ == floor_, "dmh_row_quantile_abs: floor is NaN");
  hipLaunchKernelGGL(row_quantile_abs_kernel, dim3((unsigned)B), dim3(QT), 0, (hipStream_t)stream, x, n, k, frac, floor_, out);
  DMH_CHECK_LAUNCH("dmh_row_quantile_abs");
  return DMH_OK;
}

static int threshold_checks(const char* who, const void* s, const float* mc, const float* mn, const float* x, const float* x0_raw,
                            const float* thr, int B, int64_t n, int64_t k, float frac, const uint8_t* keep) {
  if (!s || !mc || !x || !x0_raw || !thr) {
    dmh_set_error("%s: null pointer", who);
    return DMH_EINVAL;
  }
  if (!quantile_args_ok(who, B, n, k, frac)) return DMH_EINVAL;
  if (keep && !mn) {
    dmh_set_error("%s: keep needs model_null", who);
    return DMH_EINVAL;
  }
  return DMH_OK;
}

extern "C" int dmh_sampler_threshold(const DmhStep* s, const float* model_cond, const float* model_null, const float* x,
                                     const uint8_t* keep, float* x0_raw, float* thr, int B, int64_t n, int64_t k, float frac,
                                     void* stream) {
  const int rc = threshold_checks("dmh_sampler_threshold", s, model_cond, model_null, x, x0_raw, thr, B, n, k, frac, keep);
  if (rc != DMH_OK) return rc;
  DMH_REQUIRE(s->objective >= 0 && s->objective <= 2, "dmh_sampler_threshold: bad enum (objective)");
  const int64_t total = (int64_t)B * n;   // (B < 2^31, n < 2^31)
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(x0_raw_kernel, dim3(grid_for(total)), dim3(256), 0, st, *s, model_cond, model_null, x, x0_raw, total, keep, n);
  DMH_CHECK_LAUNCH("dmh_sampler_threshold(x0_raw)");
  hipLaunchKernelGGL(row_quantile_abs_kernel, dim3((unsigned)B), dim3(QT), 0, st, (const float*)x0_raw, n, k, frac, 1.f, thr);
  DMH_CHECK_LAUNCH("dmh_sampler_threshold(quantile)");
  return DMH_OK;
}

extern "C" int dmh_sampler_threshold_dev(const DmhStep* cur_dev, const float* model_cond, const float* model_null,
                                         const float* x, const uint8_t* keep, float* x0_raw, float* thr, int B, int64_t n,
                                         int64_t k, float frac, void* stream) {
  const int rc = threshold_checks("dmh_sampler_threshold_dev", cur_dev, model_cond, model_null, x, x0_raw, thr, B, n, k, frac, keep);
  if (rc != DMH_OK) return rc;
  const int64_t total = (int64_t)B * n;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(x0_raw_dev_kernel, dim3(grid_for(total)), dim3(256), 0, st, cur_dev, model_cond, model_null, x, x0_raw, total,
                     keep, n);
  DMH_CHECK_LAUNCH("dmh_sampler_threshold_dev(x0_raw)");
  hipLaunchKernelGGL(row_quantile_abs_kernel, dim3((unsigned)B), dim3(QT), 0, st, (const float*)x0_raw, n, k, frac, 1.f, thr);
  DMH_CHECK_LAUNCH("dmh_sampler_threshold_dev(quantile)");
  return DMH_OK;
}

static int step_thr_checks(const char* who, const void* s, const float* mc, const float* mn, const float* x, const float* noise,
                           const float* hist, const float* thr, const float* img_out, int64_t total, const uint8_t* keep,
                           int64_t per_row) {
  if (!s || !mc || !x || !thr || !img_out) {
    dmh_set_error("%s: null pointer", who);
    return DMH_EINVAL;
  }
  if (total < 1 || per_row < 1 || total % per_row != 0) {
    dmh_set_error("%s: n=%lld elements in rows of per_row=%lld (thr holds one value per row)", who, (long long)total,
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

extern "C" int dmh_sampler_step_thr(const DmhStep* s, const float* model_cond, const float* model_null, const float* x,
                                    const float* noise, float* hist, const float* thr, float* img_out, float* x_start, int64_t n,
                                    const uint8_t* keep, int64_t per_row, void* stream) {
  const int rc = step_thr_checks("dmh_sampler_step_thr", s, model_cond, model_null, x, noise, hist, thr, img_out, n, keep, per_row);
  if (rc != DMH_OK) return rc;
  DMH_REQUIRE(s->objective >= 0 && s->objective <= 2 && (s->mode == 0 || s->mode == 1 || s->mode == 3),
              "dmh_sampler_step_thr: bad enum (mode: 0 DDIM, 1 last step or 3 multistep)");
  DMH_REQUIRE(s->mode != 0 || noise, "dmh_sampler_step_thr: DDIM update needs noise");
  DMH_REQUIRE(s->mode != 3 || hist, "dmh_sampler_step_thr: multistep update needs hist");
  hipLaunchKernelGGL(step_thr_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, *s, model_cond, model_null, x, noise,
                     hist, thr, img_out, x_start, n, keep, per_row);
  DMH_CHECK_LAUNCH("dmh_sampler_step_thr");
  return DMH_OK;
}

extern "C" int dmh_sampler_step_thr_dev(const DmhStep* cur_dev, const float* model_cond, const float* model_null, const float* x,
                                        const float* noise, float* hist, const float* thr, float* img_out, float* x_start,
                                        int64_t n, const uint8_t* keep, int64_t per_row, void* stream) {
  const int rc = step_thr_checks("dmh_sampler_step_thr_dev", cur_dev, model_cond, model_null, x, noise, hist, thr, img_out, n, keep,
                                 per_row);
  if (rc != DMH_OK) return rc;
  hipLaunchKernelGGL(step_thr_dev_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, cur_dev, model_cond, model_null, x,
                     noise, hist, thr, img_out, x_start, n, keep, per_row);
  DMH_CHECK_LAUNCH("dmh_sampler_step_thr_dev");
  return DMH_OK;
}
