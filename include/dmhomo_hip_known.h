/* Extension of the C ABI of libdmhomo_hip.so (include/dmhomo_hip.h): sampling around known pixels.
 *
 * The entries below are exported by the same library and answer through the same error channel (dmh_last_error), but they
 * are declared here and bound from their own table (dmhomo_amd/_lib.py: EXTENSIONS): the table of dmhomo_hip.h and its
 * version (DMH_ABI_VERSION 500) are left as they are.
 *
 * Known pixels (cfg.GaussianDiffusion.sample_known; not in the reference).  Given, per sample, the image pair `known`
 * (6, H, W) in [0, 1] and a mask of the same shape (nonzero: keep this element), with K = 2 * known - 1 the pair in the
 * sampler's own range:
 *
 *   at EVERY entry of the time list, with x the logits the update would read — guided_logit(cond, null, keep, cond_scale),
 *   behind the shifts of flow_guidance / pag_scale, behind apg_eta or photo_guidance where those are on —
 *       y[i] = mask[i] ? K[i] : x[i]                                  a SELECT: a NaN under a kept element does not survive
 *   and y goes through the existing step and threshold kernels as a conditional output without a null pass.  Under pred_x0
 *   the step's x_start on a kept element is clamp(K) = K and its pred_noise is the noise the current image implies relative
 *   to K, so the DDIM update keeps that element a valid draw of q(x_s | K) at every noise level: no re-noising launch and
 *   no extra random draw.
 *
 *   after the last entry's unnormalise (0.5 * x + 0.5) the kept elements of the returned image are overwritten with `known`
 *   itself: 0.5 * (2 k - 1) + 0.5 == k holds for 193 of the 256 values k = n / 255 only, and uint8(k * 255) of the other 63
 *   would come back as n - 1.  The write-back is the same entry: null = NULL, cond_scale = 1, in place on the image.
 *
 *   resampling (known_resample = r >= 1; RePaint's harmonisation with jump length 1, Lugmayr et al. 2022): every entry t -> s
 *   is preceded by r - 1 "stay" entries t -> t.  A step to s followed by re-noising back to t is, in distribution, ONE DDIM
 *   entry at time t with, a = abar_t, a' = abar_s (1 for the entry that returns x_0), (sigma, c) that entry's DDIM
 *   coefficients (0, 0 for the last):
 *       c0 = sqrt(a),  c1 = sqrt(a / a') * c,  c2 = sqrt((a / a') * sigma^2 + 1 - a / a'),     c1^2 + c2^2 = 1 - a
 *   so the stays are entries of the step table, and no kernel knows about them.
 *
 *   the score (score_known): per sample, sum m * (x - K)^2 / max(1, sum m) over the sample's elements, m = (mask != 0), x the
 *   last entry's own logits before the overwrite: how far the model's final prediction is from the pixels it was told to
 *   keep.  float64, a fixed summation order; 0 for a sample with nothing kept.
 */
#ifndef DMHOMO_HIP_KNOWN_H
#define DMHOMO_HIP_KNOWN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* dmh_known_blend: one launch, B rows of per_row elements.
 *   out[i] = kmask[i] ? known[i] : guided_logit(model_cond, model_null, keep, i, per_row, cond_scale)
 * guided_logit as the step kernels read it: model_cond[i], or with model_null the blend null + (c - null) * cond_scale, c =
 * model_cond[i] or — keep[i / per_row] == 0: a row the conditional pass did not compute — model_null[i]; model_cond is not
 * read there.  model_null and keep may be NULL (keep needs model_null).  kmask: one byte per element.  out may be model_cond
 * itself (in place); it must not overlap model_null, known or kmask, nor model_cond in part.  With an all-zero mask out is
 * guided_logit bit for bit.  It reads no DmhStep: the same call serves the eager and the replayed loop. */
int dmh_known_blend(const float* model_cond, const float* model_null, const uint8_t* keep, float cond_scale,
                    const float* known, const uint8_t* kmask, float* out, int B, int64_t per_row, void* stream);

/* dmh_known_error_splits: workgroups per row of the first launch of dmh_known_error, a pure function of (B, per_row);
 * <= 0 for arguments outside 1 <= B <= 65535, 1 <= per_row < 2^31. */
int dmh_known_error_splits(int B, int64_t per_row);

/* dmh_known_error: out[b] = sum_i m * (x[i] - known[i])^2 / max(1, sum_i m) over row b, m = (kmask[i] != 0), x =
 * guided_logit(...) as above (read under kept elements only), differences, squares and sums in float64.  Two launches, no
 * atomics: partial (sum, count) pairs into ws (2 * B * dmh_known_error_splits(B, per_row) doubles), then one thread per row
 * adds them in split order: two calls give the same bits.  out: B doubles. */
int dmh_known_error(const float* model_cond, const float* model_null, const uint8_t* keep, float cond_scale,
                    const float* known, const uint8_t* kmask, double* ws, double* out, int B, int64_t per_row, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DMHOMO_HIP_KNOWN_H */
