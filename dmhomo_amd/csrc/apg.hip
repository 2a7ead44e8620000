// Adaptive projected guidance of the conditional sampler (Sadat, Hilliges, Weber 2024, "Eliminating Oversaturation and
// Artifacts of High Guidance Scales in Diffusion Models", Algorithm 1; not in the reference): the guidance update cond - null is
// split into its parts parallel and orthogonal to the conditional prediction, the parallel part is down-weighted (eta), the
// update's norm is capped per sample (rho) and a negative-momentum average of it runs over the steps (beta).  The definition
// (include/dmhomo_hip.h states it too), per row b of n values:
//   c[i] = model_cond[i], or model_null[i] where keep[b] == 0           (the conditional logit as guided_logit reads it)
//   d[i] = c[i] - model_null[i]                                          fp32
//   beta != 0:  run[i] <- d[i] + beta * run[i]  (fp32, two roundings);  d <- run
//   Sdd = sum d^2, Sdc = sum d*c, Scc = sum c^2                          products and sums in fp64
//   s = 1 if rho == 0 or Sdd == 0, else min(1, rho / sqrt(Sdd));   p = 0 if Scc == 0, else Sdc / Scc
//   A[b] = 1 - (w - 1) * s * (1 - eta) * p,  Cc[b] = (w - 1) * s         fp64, each rounded to fp32 once; w = cond_scale
//   guided[i] = A[b] * c[i] + Cc[b] * d[i]                               fp32: two products, one add
// = c + (w - 1) * s * (d_orth + eta * d_par).  A row whose sums are not all finite (a NaN or an infinity in it) gets A = Cc =
// NaN, and no other row does.  A row whose cond equals its null bitwise has d == 0 at beta == 0: A == 1, guided == c exactly.
// The guided logits go to the existing step and threshold entries as model_cond with model_null == NULL (guided_logit hands
// them on), so no step kernel knows about any of this.
#include "common.h"

#pragma clang fp contract(off)

// ---- dmh_apg_coef: two launches, no atomics, no arrival counter: the result is a pure function of the inputs and the split
// count.  Pass A: grid (B, splits), split j of row b covers the elements [j * chunk, min(n, (j + 1) * chunk)), writes run there
// (beta != 0) and the three fp64 sums over them; the threads of a wave combine by shuffles, the four waves through LDS in wave
// order.  Pass B: one thread per row adds the row's partials in split order and writes A and Cc.
constexpr int AT = 256;            // threads of a pass A workgroup
constexpr int64_t A_CHUNK = 4096;  // elements a workgroup should at least own: 4 float4 per thread and tensor
constexpr int A_MAX_WG = 1024;     // workgroups of pass A over all rows: 4 per CU

static int apg_splits(int B, int64_t n) {
  const int64_t want = cdiv64(n, A_CHUNK), cap = A_MAX_WG / B > 1 ? A_MAX_WG / B : 1;
  return (int)(want < cap ? want : cap);
}

// elements per split: a multiple of 4, so that every split of a row meets the same 16 B phase
__host__ __device__ __forceinline__ int64_t apg_chunk(int64_t n, int splits) {
  return ((n + splits - 1) / splits + 3) / 4 * 4;
}

struct ApgSums {
  double dd, dc, cc;
};

// one element: the update d (through the running average where there is one; the new average is returned in r) into the sums
__device__ __forceinline__ void apg_add(ApgSums& a, float c, float u, bool momentum, float beta, float& r) {
  float d = c - u;
  if (momentum) {
    const float br = beta * r;
    d = d + br;
    r = d;
  }
  const double dd = (double)d, dc = (double)c;
  a.dd += dd * dd;
  a.dc += dd * dc;
  a.cc += dc * dc;
}

// no __restrict__ on run: in place, every element is read and written by one thread
__global__ __launch_bounds__(AT) void apg_partial_kernel(const float* __restrict__ mc, const float* __restrict__ mn,
                                                         const uint8_t* __restrict__ keep, float beta, float* run,
                                                         double* __restrict__ ws, int64_t n) {
  __shared__ double part[AT / 64][3];
  const int tid = threadIdx.x, b = blockIdx.x, split = blockIdx.y, splits = gridDim.y;
  const int64_t chunk = apg_chunk(n, splits);
  const int64_t lo = (int64_t)split * chunk;
  const int64_t cnt = n - lo < chunk ? n - lo : chunk;
  double* out = ws + ((size_t)b * splits + split) * 3;
  if (cnt <= 0) {   // (an empty split: pass B stops in front of it)
    if (tid < 3) out[tid] = 0.;
    return;
  }
  const bool kept = !keep || keep[b];   // a dropped row's conditional logits ARE its null logits: model_cond is not read
  const bool momentum = run != nullptr;
  const float* pn = mn + (size_t)b * (size_t)n + lo;
  const float* pc = kept ? mc + (size_t)b * (size_t)n + lo : pn;
  float* pr = momentum ? run + (size_t)b * (size_t)n + lo : nullptr;
  ApgSums a = {0., 0., 0.};
  const uintptr_t phase = ((uintptr_t)pn ^ (uintptr_t)pc) | (momentum ? (uintptr_t)pn ^ (uintptr_t)pr : 0);
  if ((phase & 15u) == 0) {   // the rows meet 16 B boundaries together: scalar head, float4, scalar tail
    int64_t head = (int64_t)(((16u - (unsigned)((uintptr_t)pn & 15u)) & 15u) >> 2);
    head = head < cnt ? head : cnt;
    const int64_t nv = (cnt - head) >> 2;
    if (tid < head) {
      float r = momentum ? pr[tid] : 0.f;
      apg_add(a, pc[tid], pn[tid], momentum, beta, r);
      if (momentum) pr[tid] = r;
    }
    const float4* vn = reinterpret_cast<const float4*>(pn + head);
    const float4* vc = reinterpret_cast<const float4*>(pc + head);
    float4* vr = momentum ? reinterpret_cast<float4*>(pr + head) : nullptr;
    for (int64_t i = tid; i < nv; i += AT) {
      const float4 qn = vn[i], qc = vc[i];
      float4 qr = momentum ? vr[i] : make_float4(0.f, 0.f, 0.f, 0.f);
      apg_add(a, qc.x, qn.x, momentum, beta, qr.x);
      apg_add(a, qc.y, qn.y, momentum, beta, qr.y);
      apg_add(a, qc.z, qn.z, momentum, beta, qr.z);
      apg_add(a, qc.w, qn.w, momentum, beta, qr.w);
      if (momentum) vr[i] = qr;
    }
    const int64_t t0 = head + nv * 4;
    if (tid < cnt - t0) {
      float r = momentum ? pr[t0 + tid] : 0.f;
      apg_add(a, pc[t0 + tid], pn[t0 + tid], momentum, beta, r);
      if (momentum) pr[t0 + tid] = r;
    }
  } else {
    for (int64_t i = tid; i < cnt; i += AT) {
      float r = momentum ? pr[i] : 0.f;
      apg_add(a, pc[i], pn[i], momentum, beta, r);
      if (momentum) pr[i] = r;
    }
  }
  for (int off = 32; off > 0; off >>= 1) {
    a.dd += __shfl_down(a.dd, off);
    a.dc += __shfl_down(a.dc, off);
    a.cc += __shfl_down(a.cc, off);
  }
  if ((tid & 63) == 0) {
    double* p = part[tid >> 6];
    p[0] = a.dd, p[1] = a.dc, p[2] = a.cc;
  }
  __syncthreads();
  if (tid < 3) out[tid] = ((part[0][tid] + part[1][tid]) + part[2][tid]) + part[3][tid];
}

__device__ __forceinline__ void apg_finish_body(float cond_scale, const double* ws, float eta, float rho, float* coef, int B,
                                                int64_t n, int splits) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  const int64_t chunk = apg_chunk(n, splits);
  const double* p = ws + (size_t)b * splits * 3;
  double sdd = 0., sdc = 0., scc = 0.;
  for (int j = 0; j < splits; ++j, p += 3) {
    if (n - (int64_t)j * chunk <= 0) break;
    sdd += p[0], sdc += p[1], scc += p[2];
  }
  double A = __builtin_nan(""), Cc = __builtin_nan("");
  if (isfinite(sdd) && isfinite(sdc) && isfinite(scc)) {
    const double q = (rho == 0.f || sdd == 0.) ? 1. : (double)rho / sqrt(sdd);
    const double s = q < 1. ? q : 1.;
    const double pr = scc == 0. ? 0. : sdc / scc;
    Cc = ((double)cond_scale - 1.) * s;
    A = 1. - Cc * (1. - (double)eta) * pr;
  }
  coef[2 * b] = (float)A;
  coef[2 * b + 1] = (float)Cc;
}

__global__ __launch_bounds__(64) void apg_finish_kernel(DmhStep s, const double* __restrict__ ws, float eta, float rho,
                                                        float* __restrict__ coef, int B, int64_t n, int splits) {
  apg_finish_body(s.cond_scale, ws, eta, rho, coef, B, n, splits);
}

__global__ __launch_bounds__(64) void apg_finish_dev_kernel(const DmhStep* __restrict__ sp, const double* __restrict__ ws,
                                                            float eta, float rho, float* __restrict__ coef, int B, int64_t n,
                                                            int splits) {
  apg_finish_body(sp->cond_scale, ws, eta, rho, coef, B, n, splits);
}

// ---- dmh_apg_apply: guided = A * c + Cc * d, d from run where there is a running average, else c - null again
__global__ __launch_bounds__(256) void apg_apply_kernel(const float* __restrict__ mc, const float* __restrict__ mn,
                                                        const uint8_t* __restrict__ keep, const float* __restrict__ run,
                                                        const float* __restrict__ coef, float* __restrict__ guided,
                                                        int64_t total, int64_t per_row) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) {
    const int64_t b = i / per_row;
    const float u = mn[i];
    const float c = (keep && !keep[b]) ? u : mc[i];
    const float d = run ? run[i] : c - u;
    const float ac = coef[2 * b] * c, cd = coef[2 * b + 1] * d;
    guided[i] = ac + cd;
  }
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

extern "C" int dmh_apg_splits(int B, int64_t n) { return rows_ok("dmh_apg_splits", B, n) ? apg_splits(B, n) : -1; }

static int coef_checks(const char* who, const void* s, const float* mc, const float* mn, const uint8_t* keep, float eta,
                       float rho, float beta, const float* run, const double* ws, const float* coef, int B, int64_t n) {
  if (!s || !mc || !ws || !coef) {
    dmh_set_error("%s: null pointer", who);
    return DMH_EINVAL;
  }
  if (!mn) {
    dmh_set_error(keep ? "%s: keep needs model_null" : "%s: model_null is NULL (without a null pass there is nothing to project)",
                  who);
    return DMH_EINVAL;
  }
  if (!rows_ok(who, B, n)) return DMH_EINVAL;
  if (!(eta >= 0.f && eta <= 1.f)) {
    dmh_set_error("%s: eta=%g outside [0, 1]", who, (double)eta);
    return DMH_EINVAL;
  }
  if (!(rho >= 0.f && rho <= 3.402823466e38f)) {
    dmh_set_error("%s: rho=%g (a finite norm threshold >= 0; 0: none)", who, (double)rho);
    return DMH_EINVAL;
  }
  if (!(beta > -1.f && beta < 1.f)) {
    dmh_set_error("%s: beta=%g outside (-1, 1)", who, (double)beta);
    return DMH_EINVAL;
  }
  if ((run != nullptr) != (beta != 0.f)) {
    dmh_set_error("%s: run is %s with beta=%g (the running average goes with beta != 0, and only with it)", who,
                  run ? "given" : "NULL", (double)beta);
    return DMH_EINVAL;
  }
  return DMH_OK;
}

extern "C" int dmh_apg_coef(const DmhStep* s, const float* model_cond, const float* model_null, const uint8_t* keep, float eta,
                            float rho, float beta, float* run, double* ws, float* coef, int B, int64_t n, void* stream) {
  const int rc = coef_checks("dmh_apg_coef", s, model_cond, model_null, keep, eta, rho, beta, run, ws, coef, B, n);
  if (rc != DMH_OK) return rc;
  const int splits = apg_splits(B, n);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(apg_partial_kernel, dim3((unsigned)B, (unsigned)splits), dim3(AT), 0, st, model_cond, model_null, keep, beta,
                     run, ws, n);
  DMH_CHECK_LAUNCH("dmh_apg_coef(partials)");
  hipLaunchKernelGGL(apg_finish_kernel, dim3((unsigned)cdiv(B, 64)), dim3(64), 0, st, *s, (const double*)ws, eta, rho, coef, B, n,
                     splits);
  DMH_CHECK_LAUNCH("dmh_apg_coef(finish)");
  return DMH_OK;
}

extern "C" int dmh_apg_coef_dev(const DmhStep* cur_dev, const float* model_cond, const float* model_null, const uint8_t* keep,
                                float eta, float rho, float beta, float* run, double* ws, float* coef, int B, int64_t n,
                                void* stream) {
  const int rc = coef_checks("dmh_apg_coef_dev", cur_dev, model_cond, model_null, keep, eta, rho, beta, run, ws, coef, B, n);
  if (rc != DMH_OK) return rc;
  const int splits = apg_splits(B, n);
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(apg_partial_kernel, dim3((unsigned)B, (unsigned)splits), dim3(AT), 0, st, model_cond, model_null, keep, beta,
                     run, ws, n);
  DMH_CHECK_LAUNCH("dmh_apg_coef_dev(partials)");
  hipLaunchKernelGGL(apg_finish_dev_kernel, dim3((unsigned)cdiv(B, 64)), dim3(64), 0, st, cur_dev, (const double*)ws, eta, rho,
                     coef, B, n, splits);
  DMH_CHECK_LAUNCH("dmh_apg_coef_dev(finish)");
  return DMH_OK;
}

static bool overlaps(const void* a, const void* b, uintptr_t bytes) {
  const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
  return b && pa < pb + bytes && pb < pa + bytes;
}

extern "C" int dmh_apg_apply(const float* model_cond, const float* model_null, const uint8_t* keep, const float* run,
                             const float* coef, float* guided, int B, int64_t n, void* stream) {
  DMH_REQUIRE(model_cond && coef && guided, "dmh_apg_apply: null pointer");
  DMH_REQUIRE(model_null, keep ? "dmh_apg_apply: keep needs model_null"
                               : "dmh_apg_apply: model_null is NULL (without a null pass there is nothing to project)");
  if (!rows_ok("dmh_apg_apply", B, n)) return DMH_EINVAL;
  const int64_t total = (int64_t)B * n;   // (B < 2^31, n < 2^31)
  const uintptr_t bytes = (uintptr_t)total * 4u;
  DMH_REQUIRE(!overlaps(guided, model_cond, bytes) && !overlaps(guided, model_null, bytes) && !overlaps(guided, run, bytes),
              "dmh_apg_apply: guided overlaps an input (model_cond, model_null or run)");
  hipLaunchKernelGGL(apg_apply_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, model_cond, model_null, keep, run,
                     coef, guided, total, n);
  DMH_CHECK_LAUNCH("dmh_apg_apply");
  return DMH_OK;
}
