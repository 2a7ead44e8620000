// Guidance on the homography condition (flow_guidance; not in the reference) and the training side's drop of that condition
// (flow_drop_prob).  The definition (include/dmhomo_hip.h states it too), per element i of row b, w = flow_guidance - 1:
//   u[i] = the logits of the no-flow pass (null class where there is a null pass, else the conditional pass's keep bits)
//   b[i] = model_null[i] where there is a null pass (case A), else model_cond[i] (case B)
//   e[i] = w * (b[i] - u[i])                                             fp32, the difference rounded before the product
//   case A:  model_null[i] <- b[i] + e[i];  model_cond[i] <- model_cond[i] + e[i]  where the conditional pass computed row b
//   case B:  model_cond[i] <- b[i] + e[i]
// so that the blend null' + (cond' - null') * cond_scale of the step kernels is u + s_f * (n - u) + s_c * (c - n) in exact
// arithmetic, and cond' - null' is cond - null up to rounding: no kernel behind this one knows about any of it.
// dmh_affine_rows_keep is dmh_affine with a keep bit per row: a dropped row is +0.0, the no-flow pass's own stem input.
#include "common.h"
#include "flat_range.h"

#pragma clang fp contract(off)

// (the flat-range helpers — FlatSplit, flat_split, flat_grid, row_of — and the argument checks: flat_range.h)

// ---- dmh_flow_guidance_shift
__device__ __forceinline__ float shift_e(float b, float u, float w) {
  const float d = b - u;
  return w * d;
}

// one element.  NULLP: there is a null pass (case A); a row with keep == 0 has no conditional logits: not read, not written
template <bool NULLP>
__device__ __forceinline__ void shift_elem(float* cond, float* null, const float* uncond, const uint8_t* keep, float w, int64_t i,
                                           int64_t n, bool small) {
  const float u = uncond[i];
  if (NULLP) {
    const float b = null[i];
    const float e = shift_e(b, u, w);
    null[i] = b + e;
    if (!keep || keep[row_of(i, n, small)]) cond[i] = cond[i] + e;
  } else {
    const float b = cond[i];
    cond[i] = b + shift_e(b, u, w);
  }
}

// no __restrict__ on cond and null: in place, every element is read and written by one thread
template <bool NULLP>
__global__ __launch_bounds__(FT) void flow_shift_kernel(float* cond, float* null, const float* __restrict__ uncond,
                                                        const uint8_t* __restrict__ keep, float w, int64_t total, int64_t n,
                                                        FlatSplit sp) {
  const int64_t g = (int64_t)blockIdx.x * FT + threadIdx.x, stride = (int64_t)gridDim.x * FT;
  const bool small = total <= (int64_t)0xffffffffll;
  for (int64_t i = g; i < sp.head; i += stride) shift_elem<NULLP>(cond, null, uncond, keep, w, i, n, small);
  for (int64_t v = g; v < sp.nv; v += stride) {
    const int64_t i = sp.head + v * 4;
    bool kept = true;
    if (NULLP && keep) {
      const int64_t r0 = row_of(i, n, small), r3 = row_of(i + 3, n, small);
      if (r0 != r3) {   // the vector crosses a row boundary (n % 4 != 0): every element under its own row's bit
        for (int j = 0; j < 4; ++j) shift_elem<NULLP>(cond, null, uncond, keep, w, i + j, n, small);
        continue;
      }
      kept = keep[r0] != 0;
    }
    const float4 u = ld4(uncond + i);
    if (NULLP) {
      const float4 b = ld4(null + i);
      const float4 e = make_float4(shift_e(b.x, u.x, w), shift_e(b.y, u.y, w), shift_e(b.z, u.z, w), shift_e(b.w, u.w, w));
      st4(null + i, make_float4(b.x + e.x, b.y + e.y, b.z + e.z, b.w + e.w));
      if (kept) {
        const float4 c = ld4(cond + i);
        st4(cond + i, make_float4(c.x + e.x, c.y + e.y, c.z + e.z, c.w + e.w));
      }
    } else {
      const float4 b = ld4(cond + i);
      st4(cond + i, make_float4(b.x + shift_e(b.x, u.x, w), b.y + shift_e(b.y, u.y, w), b.z + shift_e(b.z, u.z, w),
                                b.w + shift_e(b.w, u.w, w)));
    }
  }
  for (int64_t i = sp.t0 + g; i < total; i += stride) shift_elem<NULLP>(cond, null, uncond, keep, w, i, n, small);
}

// ---- dmh_affine_rows_keep: dmh_affine's expression (sampler.hip: the product rounded, then the sum) on kept rows
__device__ __forceinline__ float affine1(float x, float scale, float shift) {
  const float p = x * scale;
  return p + shift;
}

__device__ __forceinline__ void affine_keep_elem(const float* x, float* y, const uint8_t* keep, float scale, float shift,
                                                 int64_t i, int64_t n, bool small) {
  y[i] = keep[row_of(i, n, small)] ? affine1(x[i], scale, shift) : 0.f;
}

__global__ __launch_bounds__(FT) void affine_rows_keep_kernel(const float* __restrict__ x, float* __restrict__ y,
                                                              const uint8_t* __restrict__ keep,
                                                              float scale, float shift, int64_t total, int64_t n,
                                                              FlatSplit sp) {
  const int64_t g = (int64_t)blockIdx.x * FT + threadIdx.x, stride = (int64_t)gridDim.x * FT;
  const bool small = total <= (int64_t)0xffffffffll;
  for (int64_t i = g; i < sp.head; i += stride) affine_keep_elem(x, y, keep, scale, shift, i, n, small);
  for (int64_t v = g; v < sp.nv; v += stride) {
    const int64_t i = sp.head + v * 4;
    const int64_t r0 = row_of(i, n, small), r3 = row_of(i + 3, n, small);
    if (r0 != r3) {
      for (int j = 0; j < 4; ++j) affine_keep_elem(x, y, keep, scale, shift, i + j, n, small);
      continue;
    }
    float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
    if (keep[r0]) {   // (a dropped row's x is not read)
      const float4 a = ld4(x + i);
      q = make_float4(affine1(a.x, scale, shift), affine1(a.y, scale, shift), affine1(a.z, scale, shift),
                      affine1(a.w, scale, shift));
    }
    st4(y + i, q);
  }
  for (int64_t i = sp.t0 + g; i < total; i += stride) affine_keep_elem(x, y, keep, scale, shift, i, n, small);
}

// ---- the entries
extern "C" int dmh_flow_guidance_shift(float* model_cond, float* model_null, const float* uncond, const uint8_t* keep, float w,
                                       int B, int64_t n, void* stream) {
  DMH_REQUIRE(model_cond && uncond, "dmh_flow_guidance_shift: null pointer");
  DMH_REQUIRE(model_null || !keep, "dmh_flow_guidance_shift: keep needs model_null (without a null pass every row was computed)");
  if (!rows_ok("dmh_flow_guidance_shift", B, n)) return DMH_EINVAL;
  DMH_REQUIRE(w >= -3.402823466e38f && w <= 3.402823466e38f, "dmh_flow_guidance_shift: w=%g is not finite", (double)w);
  DMH_REQUIRE((((uintptr_t)model_cond | (uintptr_t)model_null | (uintptr_t)uncond) & 3u) == 0,
              "dmh_flow_guidance_shift: a pointer is not 4-byte aligned");
  const int64_t total = (int64_t)B * n;   // (B < 2^31, n < 2^31)
  const uintptr_t bytes = (uintptr_t)total * 4u;
  DMH_REQUIRE(!overlaps(uncond, model_cond, bytes) && !overlaps(uncond, model_null, bytes),
              "dmh_flow_guidance_shift: uncond overlaps model_cond or model_null");
  DMH_REQUIRE(!overlaps(model_cond, model_null, bytes), "dmh_flow_guidance_shift: model_cond overlaps model_null");
  const FlatSplit sp = flat_split(model_cond, total, same_phase(model_cond, uncond) && same_phase(model_cond, model_null));
  const dim3 grid(flat_grid(sp, total));
  if (model_null)
    hipLaunchKernelGGL(flow_shift_kernel<true>, grid, dim3(FT), 0, (hipStream_t)stream, model_cond, model_null, uncond, keep, w,
                       total, n, sp);
  else
    hipLaunchKernelGGL(flow_shift_kernel<false>, grid, dim3(FT), 0, (hipStream_t)stream, model_cond, model_null, uncond, keep, w,
                       total, n, sp);
  DMH_CHECK_LAUNCH("dmh_flow_guidance_shift");
  return DMH_OK;
}

extern "C" int dmh_affine_rows_keep(const float* x, float* y, float scale, float shift, const uint8_t* keep, int B, int64_t n,
                                    void* stream) {
  DMH_REQUIRE(x && y && keep, "dmh_affine_rows_keep: null pointer");
  if (!rows_ok("dmh_affine_rows_keep", B, n)) return DMH_EINVAL;
  DMH_REQUIRE((((uintptr_t)x | (uintptr_t)y) & 3u) == 0, "dmh_affine_rows_keep: a pointer is not 4-byte aligned");
  const int64_t total = (int64_t)B * n;
  DMH_REQUIRE(!overlaps(x, y, (uintptr_t)total * 4u), "dmh_affine_rows_keep: y overlaps x");
  const FlatSplit sp = flat_split(x, total, same_phase(x, y));
  hipLaunchKernelGGL(affine_rows_keep_kernel, dim3(flat_grid(sp, total)), dim3(FT), 0, (hipStream_t)stream, x, y, keep, scale,
                     shift, total, n, sp);
  DMH_CHECK_LAUNCH("dmh_affine_rows_keep");
  return DMH_OK;
}
