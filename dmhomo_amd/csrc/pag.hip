// Perturbed-attention guidance (pag_scale; Ahn et al. 2024; not in the reference): the shift of the logits.  The perturbed
// pass itself is the identity arm of attention_kernel (attention.hip, dmh_attention_pag).  The definition (include/dmhomo_hip.h
// states it too), per element i of row b, s = pag_scale >= 0:
//   p[i] = the logits of the perturbed pass (the conditional pass with mid_attn's attention map replaced by the identity)
//   c[i] = model_cond[i] where the conditional pass computed row b, else (keep[b] == 0) model_null[i]
//   e[i] = s * (c[i] - p[i])                                             fp32, the difference rounded before the product
//   case A (a null pass):  model_null[i] <- model_null[i] + e[i];  model_cond[i] <- model_cond[i] + e[i]  where row b was computed
//   case B (none):         model_cond[i] <- c[i] + e[i]
// so that the blend null' + (cond' - null') * cond_scale of the step kernels is n + cond_scale * (c - n) + s * (c - p) in exact
// arithmetic: no kernel behind this one knows about any of it.
#include "common.h"
#include "flat_range.h"

#pragma clang fp contract(off)

__device__ __forceinline__ float pag_e(float c, float p, float s) {
  const float d = c - p;
  return s * d;
}

// one element.  NULLP: there is a null pass (case A); a row with keep == 0 has no conditional logits: not read, not written
template <bool NULLP>
__device__ __forceinline__ void pag_elem(float* cond, float* null, const float* pert, const uint8_t* keep, float s, int64_t i,
                                         int64_t n, bool small) {
  const float p = pert[i];
  if (NULLP) {
    const float nl = null[i];
    const bool kept = !keep || keep[row_of(i, n, small)];
    const float c = kept ? cond[i] : nl;
    const float e = pag_e(c, p, s);
    null[i] = nl + e;
    if (kept) cond[i] = c + e;
  } else {
    const float c = cond[i];
    cond[i] = c + pag_e(c, p, s);
  }
}

// no __restrict__ on cond and null: in place, every element is read and written by one thread
template <bool NULLP>
__global__ __launch_bounds__(FT) void pag_shift_kernel(float* cond, float* null, const float* __restrict__ pert,
                                                       const uint8_t* __restrict__ keep, float s, int64_t total, int64_t n,
                                                       FlatSplit sp) {
  const int64_t g = (int64_t)blockIdx.x * FT + threadIdx.x, stride = (int64_t)gridDim.x * FT;
  const bool small = total <= (int64_t)0xffffffffll;
  for (int64_t i = g; i < sp.head; i += stride) pag_elem<NULLP>(cond, null, pert, keep, s, i, n, small);
  for (int64_t v = g; v < sp.nv; v += stride) {
    const int64_t i = sp.head + v * 4;
    bool kept = true;
    if (NULLP && keep) {
      const int64_t r0 = row_of(i, n, small), r3 = row_of(i + 3, n, small);
      if (r0 != r3) {   // the vector crosses a row boundary (n % 4 != 0): every element under its own row's bit
        for (int j = 0; j < 4; ++j) pag_elem<NULLP>(cond, null, pert, keep, s, i + j, n, small);
        continue;
      }
      kept = keep[r0] != 0;
    }
    const float4 p = ld4(pert + i);
    if (NULLP) {
      const float4 nl = ld4(null + i);
      const float4 c = kept ? ld4(cond + i) : nl;
      const float4 e = make_float4(pag_e(c.x, p.x, s), pag_e(c.y, p.y, s), pag_e(c.z, p.z, s), pag_e(c.w, p.w, s));
      st4(null + i, make_float4(nl.x + e.x, nl.y + e.y, nl.z + e.z, nl.w + e.w));
      if (kept) st4(cond + i, make_float4(c.x + e.x, c.y + e.y, c.z + e.z, c.w + e.w));
    } else {
      const float4 c = ld4(cond + i);
      st4(cond + i, make_float4(c.x + pag_e(c.x, p.x, s), c.y + pag_e(c.y, p.y, s), c.z + pag_e(c.z, p.z, s),
                                c.w + pag_e(c.w, p.w, s)));
    }
  }
  for (int64_t i = sp.t0 + g; i < total; i += stride) pag_elem<NULLP>(cond, null, pert, keep, s, i, n, small);
}

extern "C" int dmh_pag_shift(float* model_cond, float* model_null, const float* pert, const uint8_t* keep, float s, int B,
                             int64_t n, void* stream) {
  DMH_REQUIRE(model_cond && pert, "dmh_pag_shift: null pointer");
  DMH_REQUIRE(model_null || !keep, "dmh_pag_shift: keep needs model_null (without a null pass every row was computed)");
  if (!rows_ok("dmh_pag_shift", B, n)) return DMH_EINVAL;
  DMH_REQUIRE(s >= 0.f && s <= 3.402823466e38f, "dmh_pag_shift: s=%g is not a finite number >= 0", (double)s);
  DMH_REQUIRE((((uintptr_t)model_cond | (uintptr_t)model_null | (uintptr_t)pert) & 3u) == 0,
              "dmh_pag_shift: a pointer is not 4-byte aligned");
  const int64_t total = (int64_t)B * n;   // (B < 2^31, n < 2^31)
  const uintptr_t bytes = (uintptr_t)total * 4u;
  DMH_REQUIRE(!overlaps(pert, model_cond, bytes) && !overlaps(pert, model_null, bytes),
              "dmh_pag_shift: pert overlaps model_cond or model_null");
  DMH_REQUIRE(!overlaps(model_cond, model_null, bytes), "dmh_pag_shift: model_cond overlaps model_null");
  const FlatSplit sp = flat_split(model_cond, total, same_phase(model_cond, pert) && same_phase(model_cond, model_null));
  const dim3 grid(flat_grid(sp, total));
  if (model_null)
    hipLaunchKernelGGL(pag_shift_kernel<true>, grid, dim3(FT), 0, (hipStream_t)stream, model_cond, model_null, pert, keep, s,
                       total, n, sp);
  else
    hipLaunchKernelGGL(pag_shift_kernel<false>, grid, dim3(FT), 0, (hipStream_t)stream, model_cond, model_null, pert, keep, s,
                       total, n, sp);
  DMH_CHECK_LAUNCH("dmh_pag_shift");
  return DMH_OK;
}
