// Sampling around known pixels (cfg.GaussianDiffusion.sample_known; not in the reference): the select that puts the kept
// elements into the logits a step reads, and the score of the last entry.  The definition (include/dmhomo_hip_known.h states
// it too), per element i of row b, m[i] = (kmask[i] != 0):
//   x[i]   = guided_logit(model_cond, model_null, keep, i, per_row, cond_scale)      the step kernels' own fp32 expression
//   out[i] = m[i] ? known[i] : x[i]                                                  a select: no arithmetic joins the two
//   err[b] = sum_i m[i] * (x[i] - known[i])^2 / max(1, sum_i m[i])                   float64, a fixed summation order
// In the loop `known` is K = 2 * known - 1 and out goes to the step kernels as a conditional output without a null pass; behind
// the unnormalise the same entry (model_null = NULL, cond_scale = 1, in place, the caller's own values) is the write-back.
#include "common.h"
#include "flat_range.h"
#include "../../include/dmhomo_hip_known.h"

#pragma clang fp contract(off)   // (in front of sampler_dev.h: the blend is the step kernels' expression, one rounding per operation)

#include "sampler_dev.h"

// the logit under an element that is not kept.  NULLP: there is a null pass; a row with keep == 0 has no conditional logits
template <bool NULLP>
__device__ __forceinline__ float known_logit(const float* cond, const float* null, const uint8_t* keep, float cs, int64_t i,
                                             int64_t n, bool small) {
  if (!NULLP) return cond[i];
  const float nl = null[i];
  const bool kept = !keep || keep[row_of(i, n, small)];
  return guided_blend(kept ? cond[i] : nl, nl, cs);
}

template <bool NULLP>
__device__ __forceinline__ void known_elem(const float* cond, const float* null, const uint8_t* keep, float cs,
                                           const float* known, const uint8_t* kmask, float* out, int64_t i, int64_t n,
                                           bool small) {
  out[i] = kmask[i] ? known[i] : known_logit<NULLP>(cond, null, keep, cs, i, n, small);
}

// no __restrict__ on cond and out: in place, every element is read and written by one thread.  mask32: the four mask bytes of
// a vector start on a 4-byte boundary (one 32-bit load), else four byte loads
template <bool NULLP>
__global__ __launch_bounds__(FT) void known_blend_kernel(const float* cond, const float* __restrict__ null,
                                                         const uint8_t* __restrict__ keep, float cs,
                                                         const float* __restrict__ known, const uint8_t* __restrict__ kmask,
                                                         float* out, int64_t total, int64_t n, FlatSplit sp, bool mask32) {
  const int64_t g = (int64_t)blockIdx.x * FT + threadIdx.x, stride = (int64_t)gridDim.x * FT;
  const bool small = total <= (int64_t)0xffffffffll;
  for (int64_t i = g; i < sp.head; i += stride) known_elem<NULLP>(cond, null, keep, cs, known, kmask, out, i, n, small);
  for (int64_t v = g; v < sp.nv; v += stride) {
    const int64_t i = sp.head + v * 4;
    bool kept = true;
    if (NULLP && keep) {
      const int64_t r0 = row_of(i, n, small), r3 = row_of(i + 3, n, small);
      if (r0 != r3) {   // the vector crosses a row boundary (n % 4 != 0): every element under its own row's bit
        for (int j = 0; j < 4; ++j) known_elem<NULLP>(cond, null, keep, cs, known, kmask, out, i + j, n, small);
        continue;
      }
      kept = keep[r0] != 0;
    }
    uint32_t m4;
    if (mask32)
      m4 = *reinterpret_cast<const uint32_t*>(kmask + i);
    else
      m4 = (uint32_t)kmask[i] | ((uint32_t)kmask[i + 1] << 8) | ((uint32_t)kmask[i + 2] << 16) | ((uint32_t)kmask[i + 3] << 24);
    const float4 k = ld4(known + i);
    float4 x;
    if (NULLP) {
      const float4 nl = ld4(null + i);
      const float4 c = kept ? ld4(cond + i) : nl;
      x = make_float4(guided_blend(c.x, nl.x, cs), guided_blend(c.y, nl.y, cs), guided_blend(c.z, nl.z, cs),
                      guided_blend(c.w, nl.w, cs));
    } else {
      x = ld4(cond + i);
    }
    st4(out + i, make_float4((m4 & 0xffu) ? k.x : x.x, (m4 & 0xff00u) ? k.y : x.y, (m4 & 0xff0000u) ? k.z : x.z,
                             (m4 & 0xff000000u) ? k.w : x.w));
  }
  for (int64_t i = sp.t0 + g; i < total; i += stride) known_elem<NULLP>(cond, null, keep, cs, known, kmask, out, i, n, small);
}

// ---- dmh_known_error: two launches, no atomics: the result is a pure function of the inputs.  Pass A: grid (B, splits), split
// j of row b covers the elements [j * chunk, min(n, (j + 1) * chunk)) and writes (sum of squared differences, count) over its
// kept elements: each thread sums in fp64 over its stride, the threads of a wave combine by shuffles, the four waves through
// LDS in wave order.  Pass B: one thread per row adds the row's partials in split order and divides.
constexpr int KT = 256;            // threads of a pass A workgroup
constexpr int64_t K_CHUNK = 4096;  // elements a workgroup should at least own
constexpr int K_MAX_WG = 1024;     // workgroups of pass A over all rows: 4 per CU

static int known_splits(int B, int64_t n) {
  const int64_t want = cdiv64(n, K_CHUNK), cap = K_MAX_WG / B > 1 ? K_MAX_WG / B : 1;
  return (int)(want < cap ? want : cap);
}

template <bool NULLP>
__global__ __launch_bounds__(KT) void known_error_partial_kernel(const float* __restrict__ cond, const float* __restrict__ null,
                                                                 const uint8_t* __restrict__ keep, float cs,
                                                                 const float* __restrict__ known,
                                                                 const uint8_t* __restrict__ kmask, double* __restrict__ ws,
                                                                 int64_t n) {
  __shared__ double part[KT / 64][2];
  const int tid = threadIdx.x, b = blockIdx.x, split = blockIdx.y, splits = gridDim.y;
  const int64_t chunk = (n + splits - 1) / splits;
  const int64_t lo = (int64_t)split * chunk, hi = lo + chunk < n ? lo + chunk : n;
  const int64_t base = (int64_t)b * n;
  double acc = 0., cnt = 0.;
  for (int64_t j = lo + tid; j < hi; j += KT) {
    const int64_t i = base + j;
    if (!kmask[i]) continue;   // (a logit that is not kept is not read: its NaN is not this score's business)
    const double d = (double)known_logit<NULLP>(cond, null, keep, cs, i, n, false) - (double)known[i];
    acc += d * d;
    cnt += 1.;
  }
  for (int off = 32; off > 0; off >>= 1) {
    acc += __shfl_down(acc, off);
    cnt += __shfl_down(cnt, off);
  }
  if ((tid & 63) == 0) part[tid >> 6][0] = acc, part[tid >> 6][1] = cnt;
  __syncthreads();
  if (tid == 0) {
    double* o = ws + ((size_t)b * splits + split) * 2;
    o[0] = ((part[0][0] + part[1][0]) + part[2][0]) + part[3][0];
    o[1] = ((part[0][1] + part[1][1]) + part[2][1]) + part[3][1];
  }
}

__global__ __launch_bounds__(64) void known_error_finish_kernel(const double* __restrict__ ws, double* __restrict__ out, int B,
                                                                int splits) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  double sum = 0., cnt = 0.;
  for (int j = 0; j < splits; ++j) {
    sum += ws[((size_t)b * splits + j) * 2];
    cnt += ws[((size_t)b * splits + j) * 2 + 1];
  }
  out[b] = cnt > 0. ? sum / cnt : 0.;   // (nothing kept: exactly 0, and no NaN of an empty sum)
}

// ---- entry points
static bool known_rows_ok(const char* who, int B, int64_t n) {
  // B is a grid dimension of the error's first launch; B * n < 2^47 stays far inside the 64-bit index arithmetic
  if (B < 1 || B > 65535 || n < 1 || n >= ((int64_t)1 << 31)) {
    dmh_set_error("%s: B=%d rows of per_row=%lld elements (1 <= B <= 65535, 1 <= per_row < 2^31)", who, B, (long long)n);
    return false;
  }
  return true;
}

static int known_checks(const char* who, const float* mc, const float* mn, const uint8_t* keep, float cs, const float* known,
                        const uint8_t* kmask, int B, int64_t n) {
  if (!mc || !known || !kmask) {
    dmh_set_error("%s: null pointer", who);
    return DMH_EINVAL;
  }
  if (keep && !mn) {
    dmh_set_error("%s: keep needs model_null (without a null pass every row was computed)", who);
    return DMH_EINVAL;
  }
  if (!known_rows_ok(who, B, n)) return DMH_EINVAL;
  if (!(cs >= -3.402823466e38f && cs <= 3.402823466e38f)) {
    dmh_set_error("%s: cond_scale=%g is not a finite number", who, (double)cs);
    return DMH_EINVAL;
  }
  if ((((uintptr_t)mc | (uintptr_t)mn | (uintptr_t)known) & 3u) != 0) {
    dmh_set_error("%s: a pointer is not 4-byte aligned", who);
    return DMH_EINVAL;
  }
  return DMH_OK;
}

extern "C" int dmh_known_blend(const float* model_cond, const float* model_null, const uint8_t* keep, float cond_scale,
                               const float* known, const uint8_t* kmask, float* out, int B, int64_t per_row, void* stream) {
  DMH_REQUIRE(out, "dmh_known_blend: null pointer");
  const int rc = known_checks("dmh_known_blend", model_cond, model_null, keep, cond_scale, known, kmask, B, per_row);
  if (rc != DMH_OK) return rc;
  DMH_REQUIRE(((uintptr_t)out & 3u) == 0, "dmh_known_blend: a pointer is not 4-byte aligned");
  const int64_t total = (int64_t)B * per_row;   // (B < 2^16, per_row < 2^31)
  const uintptr_t bytes = (uintptr_t)total * 4u;
  DMH_REQUIRE(!overlaps(out, model_null, bytes) && !overlaps(out, known, bytes),
              "dmh_known_blend: out overlaps model_null or known");
  {
    const uintptr_t po = (uintptr_t)out, pm = (uintptr_t)kmask;
    DMH_REQUIRE(!(po < pm + (uintptr_t)total && pm < po + bytes), "dmh_known_blend: out overlaps kmask");
  }
  DMH_REQUIRE(out == model_cond || !overlaps(out, model_cond, bytes),
              "dmh_known_blend: out overlaps model_cond in part (in place means out == model_cond)");
  const FlatSplit sp = flat_split(out, total, same_phase(out, model_cond) && same_phase(out, model_null) && same_phase(out, known));
  const bool mask32 = (((uintptr_t)kmask + (uintptr_t)sp.head) & 3u) == 0;
  const dim3 grid(flat_grid(sp, total));
  if (model_null)
    hipLaunchKernelGGL(known_blend_kernel<true>, grid, dim3(FT), 0, (hipStream_t)stream, model_cond, model_null, keep, cond_scale,
                       known, kmask, out, total, per_row, sp, mask32);
  else
    hipLaunchKernelGGL(known_blend_kernel<false>, grid, dim3(FT), 0, (hipStream_t)stream, model_cond, model_null, keep, cond_scale,
                       known, kmask, out, total, per_row, sp, mask32);
  DMH_CHECK_LAUNCH("dmh_known_blend");
  return DMH_OK;
}

extern "C" int dmh_known_error_splits(int B, int64_t per_row) {
  return known_rows_ok("dmh_known_error_splits", B, per_row) ? known_splits(B, per_row) : -1;
}

extern "C" int dmh_known_error(const float* model_cond, const float* model_null, const uint8_t* keep, float cond_scale,
                               const float* known, const uint8_t* kmask, double* ws, double* out, int B, int64_t per_row,
                               void* stream) {
  DMH_REQUIRE(ws && out, "dmh_known_error: null pointer");
  const int rc = known_checks("dmh_known_error", model_cond, model_null, keep, cond_scale, known, kmask, B, per_row);
  if (rc != DMH_OK) return rc;
  DMH_REQUIRE((((uintptr_t)ws | (uintptr_t)out) & 7u) == 0, "dmh_known_error: ws / out are not 8-byte aligned");
  const int splits = known_splits(B, per_row);
  {
    const uintptr_t pw = (uintptr_t)ws, po = (uintptr_t)out, wb = (uintptr_t)B * (uintptr_t)splits * 16u, ob = (uintptr_t)B * 8u;
    DMH_REQUIRE(!(pw < po + ob && po < pw + wb), "dmh_known_error: ws overlaps out");
  }
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)B, (unsigned)splits);
  if (model_null)
    hipLaunchKernelGGL(known_error_partial_kernel<true>, grid, dim3(KT), 0, st, model_cond, model_null, keep, cond_scale, known,
                       kmask, ws, per_row);
  else
    hipLaunchKernelGGL(known_error_partial_kernel<false>, grid, dim3(KT), 0, st, model_cond, model_null, keep, cond_scale, known,
                       kmask, ws, per_row);
  DMH_CHECK_LAUNCH("dmh_known_error(partials)");
  hipLaunchKernelGGL(known_error_finish_kernel, dim3((unsigned)cdiv(B, 64)), dim3(64), 0, st, (const double*)ws, out, B, splits);
  DMH_CHECK_LAUNCH("dmh_known_error(finish)");
  return DMH_OK;
}
