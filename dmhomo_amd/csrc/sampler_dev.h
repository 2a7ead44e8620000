// The denoise step on one element, shared by the step kernels of sampler.hip, the thresholding kernels of threshold.hip and
// the guidance-rescale kernels of guidance.hip.
// Mirrors the reference's fp32 op order: a file that includes this sets `#pragma clang fp contract(off)` first.
#pragma once
#include "common.h"

// torch.clamp(x, -1., 1.) (CFG:612,634): NaN stays NaN (fminf / fmaxf alone would turn it into -1 and hide a broken row)
__device__ __forceinline__ float clamp_pm1(float x) { return x != x ? x : fminf(fmaxf(x, -1.f), 1.f); }

// dynamic thresholding (Saharia et al. 2022, 2.3): clamp to the row's threshold, then back into [-1, 1].  thr == 1 is
// clamp_pm1 bit for bit (a division by 1 is exact); a NaN thr makes every element of its row NaN (the division)
__device__ __forceinline__ float clamp_thr(float x, float thr) { return x != x ? x : fminf(fmaxf(x, -thr), thr) / thr; }

// the network output a step works on: model_cond[i], or with model_null the guided null + (cond - null) * cond_scale (CFG:410).
// keep (with model_null): row i / per_row of model_cond was only computed where keep != 0 — a row whose class the conditional
// pass dropped (CFG:415-425) has the null pass's inputs, so its logits ARE the null logits and model_cond is never read there
__device__ __forceinline__ float guided_logit(const float* mc, const float* mn, const uint8_t* keep, int64_t i, int64_t per_row,
                                              float cond_scale) {
  if (!mn) return mc[i];
  const float nl = mn[i];
  const float mo = (keep && !keep[i / per_row]) ? nl : mc[i];
  return nl + (mo - nl) * cond_scale;
}

// guidance rescale (guidance.hip): the blend of guided_logit on values already read — the same fp32 expression, so that the
// row moments of dmh_guidance_factor are those of what the step kernels blend — and guided_logit times its row's factor
// gfac[i / per_row]; a factor of 1.0f leaves guided_logit's bits
__device__ __forceinline__ float guided_blend(float mo, float nl, float cond_scale) { return nl + (mo - nl) * cond_scale; }

__device__ __forceinline__ float rescaled_guided_logit(const float* mc, const float* mn, const uint8_t* keep, int64_t i,
                                                       int64_t per_row, float cond_scale, const float* gfac) {
  return guided_logit(mc, mn, keep, i, per_row, cond_scale) * gfac[i / per_row];
}

// x_start before any clamp (CFG:614-628): what the clamp of denoise_step and the row quantile of dmh_sampler_threshold see
__device__ __forceinline__ float raw_x_start(const DmhStep& s, float mo, float xt) {
  if (s.objective == 0) return s.sqrt_recip_ac * xt - s.sqrt_recipm1_ac * mo;  // pred_noise, CFG:614-617
  if (s.objective == 1) return mo;                                             // pred_x0, CFG:619-622
  return s.sqrt_ac * xt - s.sqrt_1m_ac * mo;                                   // pred_v, CFG:624-628
}

// ONE denoise step on one element, the only statement of it: every step kernel calls this, so the eager, the captured
// and the fused path cannot differ in a bit.  mo: guided_logit, xt: the current image, nz: the entry's noise value, has_noise:
// whether the DDPM update adds it (a DDIM update always does), prev: the previous step's x0 (read by a multistep entry with
// c2 != 0 only) -> x0 (x_start), pn (pred_noise), o (the next image).  THR: a clipping entry clamps to the row's threshold
// thr and divides by it (clamp_thr) instead of clamping to [-1, 1]
template <bool THR>
__device__ __forceinline__ void denoise_step_t(const DmhStep& s, float mo, float xt, float nz, bool has_noise, float prev,
                                               float thr, float& x0, float& pn, float& o) {
  x0 = raw_x_start(s, mo, xt);
  if (s.clip) x0 = THR ? clamp_thr(x0, thr) : clamp_pm1(x0);
  if (s.objective == 0) {  // pred_noise: the network output itself, whatever the clamp did to x0 (CFG:614-617)
    pn = mo;
  } else {  // pred_x0 / pred_v: re-derived from the clamped x0 (CFG:621,627)
    pn = (s.sqrt_recip_ac * xt - x0) / s.sqrt_recipm1_ac;
  }
  if (s.mode == 0) {  // DDIM, CFG:705-707
    o = x0 * s.c0 + s.c1 * pn + s.c2 * nz;
  } else if (s.mode == 1) {  // last DDIM step, CFG:693-695
    o = x0;
  } else if (s.mode == 2) {  // DDPM posterior step, DDP:604-611,660: mean + exp(.5 logvar) * noise (no noise at t == 0)
    o = s.c0 * x0 + s.c1 * xt;
    if (has_noise) o = o + s.c2 * nz;
  } else {  // multistep (DPM-Solver++ 2M, data prediction): c2 == 0 is its first-order update and leaves prev unread
    o = s.c0 * x0 + s.c1 * xt;
    if (s.c2 != 0.f) o = o + s.c2 * prev;
  }
}

__device__ __forceinline__ void denoise_step(const DmhStep& s, float mo, float xt, float nz, bool has_noise, float prev,
                                             float& x0, float& pn, float& o) {
  denoise_step_t<false>(s, mo, xt, nz, has_noise, prev, 1.f, x0, pn, o);
}

// whether an entry reads the x0 history of the multistep solver
__device__ __forceinline__ bool reads_history(const DmhStep& s) { return s.mode == 3 && s.c2 != 0.f; }
