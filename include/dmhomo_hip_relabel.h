/* Extension of the C ABI of libdmhomo_hip.so (include/dmhomo_hip.h): re-labelling a batch of real pairs.
 *
 * The entry below is exported by the same library and answers through the same error channel (dmh_last_error), but it is
 * declared here and bound from its own table (dmhomo_amd/_lib.py: RELABEL_EXTENSIONS): the tables of dmhomo_hip.h,
 * dmhomo_hip_known.h and dmhomo_hip_start.h and the version (DMH_ABI_VERSION 500) are left as they are.
 *
 * Re-label (dmhomo_amd.ddpm.relabel_batch, Trainer.relabel; not in the reference).  A batch in the 12-channel layout
 *   img1(3) | img2(3) | mask(1) | rgb_flow(3) | flow(2)
 * keeps its source image and its mask and gets a NEW homography label, drawn per sample on the device, with the flow and the
 * flow image of that label and, as a first target, the source warped by it (for a plane, the target that realises the label
 * exactly).
 *
 * The draw.  For sample id sid (int64, global) and seed (uint64):
 *
 *   words        two Philox4x32-10 blocks (csrc/philox.h), counter {q, 0xFFFFFFFF, sid lo, sid hi} for q = 0, 1, key (seed lo,
 *                seed hi).  The noise of the keyed generator (dmh_rng_indexed) uses the same counter layout with the draw index
 *                in the second word, counting up from 0: the draw word 0xFFFFFFFF keeps these eight words apart from every noise
 *                draw of the same seed and sample.  w0..w3 are x, y, z, w of q = 0, w4..w7 those of q = 1.
 *   uniforms     u_i = 2.0 * (double)u01(w_i) - 1.0,  u01 the fp32 uniform of philox.h (x * 2^-32 + 2^-33, a rounded multiply and
 *                a rounded add), widened to double; the multiply and the subtraction are rounded separately (both are exact).
 *   perturbation in the 360 x 640 frame, SyntheticConditions' own parameterisation, with (a, t, p) = (max_affine, max_shift,
 *                max_persp), whose defaults (.03, 8, 3e-5) are the constants of SyntheticConditions:
 *                  P0 = I + [[u0 a, u1 a, u2 t], [u3 a, u4 a, u5 t], [u6 p, u7 p, 0]]
 *   to H x W     P[i][j] = P0[i][j] * s_i / s_j  with s = (W / 640, H / 360, 1) in double: the product first, then the quotient.
 *                This is adapt_homography_to_preprocessing_v3(360, 640, P0, H, W) in closed form (M1 M0^-1 is diagonal); the
 *                closed form is the definition.
 *   base         NULL ('identity'):  H_new = P
 *                given ('batch'):    M = P . H_b,  M[i][j] = (P[i][0] H_b[0][j] + P[i][1] H_b[1][j]) + P[i][2] H_b[2][j]  in
 *                                    float64, row-major, every operation rounded separately;  H_new = M / M[2][2]
 *
 * Refused: a range that is negative or not finite; max_affine >= 0.25 (below it the linear part of P0 is strictly diagonally
 * dominant, hence invertible); max_persp >= 5e-4 (below it w' >= 1 - 5e-4 (640 + 360) = 0.5 inside the frame for the identity
 * base).
 *
 * Per pixel (x, y) of sample b, out being laid out as data:
 *   channels 0-2, 6   copied from data
 *   channels 10-11    the flow of H_new, dmh_homography_flow's arithmetic: H_new . (x, y, 1) in float64, w' + 1e-6, the
 *                     subtraction in float64, then the cast to fp32
 *   channels 7-9      dmh_homography_flow's flow image of that flow (max_flow as there)
 *   channels 3-5      img1 sampled at H_new^-1 . (x, y, 1), dmh_homography_warp's arithmetic: adjugate times 1 / det, float64
 *                     bilinear weights, taps outside the image read 0, rounded once
 *   valid             1 iff that source coordinate lies in the closed [0, W - 1] x [0, H - 1]
 *   where valid == 0 and use_fill, channels 3-5 take data's own img2 at that pixel instead.
 * flow, flow image and warp are bit for bit what dmh_homography_flow(Hm) and dmh_homography_warp(img1, Hm) write: the per-pixel
 * bodies are one definition (csrc/geometry_dev.h).
 */
#ifndef DMHOMO_HIP_RELABEL_H
#define DMHOMO_HIP_RELABEL_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* dmh_relabel_batch: one launch, 256 threads per workgroup, grid (ceil(H W / 256), B).  Thread 0 of every workgroup draws and
 * builds H_new and its inverse into LDS (18 doubles; every workgroup of a sample computes the same doubles, so there are no
 * atomics and no handshake), workgroup x == 0 writes Hm.
 *   data (B,12,H,W) fp32, sample_ids (B) int64, base (B,9) f64 row-major or NULL — all on the device;
 *   out (B,12,H,W) fp32, Hm (B,9) f64, valid (B,H,W) uint8.  out must not overlap data (out == data is refused).
 * H, W in [2, 2^16], 1 <= B <= 65535, B * 12 * H * W < 2^31; max_flow finite and > 0; float pointers 4-byte aligned, sample_ids,
 * base and Hm 8-byte aligned.  Every check runs before anything is launched. */
int dmh_relabel_batch(const float* data, const int64_t* sample_ids, uint64_t seed, double max_affine, double max_shift,
                      double max_persp, float max_flow, const double* base, int use_fill, float* out, double* Hm,
                      unsigned char* valid, int B, int H, int W, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DMHOMO_HIP_RELABEL_H */
