/* Extension of the C ABI of libdmhomo_hip.so (include/dmhomo_hip.h): starting the sampler from a given pair.
 *
 * The entry below is exported by the same library and answers through the same error channel (dmh_last_error), but it is
 * declared here and bound from its own table (dmhomo_amd/_lib.py: START_EXTENSIONS): the tables of dmhomo_hip.h and
 * dmhomo_hip_known.h and the version (DMH_ABI_VERSION 500) are left as they are.
 *
 * Start from a pair (cfg.GaussianDiffusion.sample_from; SDEdit, Meng et al. 2022; not in the reference).  With S =
 * sampling_timesteps, pairs = ddim_pairs(num_timesteps, S) the time list and strength a float in (0, 1]:
 *
 *   entries run     n  = min(S, floor(S * strength + 1e-9)),  n == 0 is refused        (schedule.start_entry)
 *   start entry     k0 = S - n,   start time t* = pairs[k0][0]
 *   start image     x  = ca * (2 * init - 1) + cb * eps
 *                   ca = sqrt_alphas_cumprod[t*], cb = sqrt_one_minus_alphas_cumprod[t*], the fp32 buffer values q_sample reads;
 *                   eps the generator's first draw of the call, the draw sample() uses as its initial image
 *
 * and from there the loop is the existing loop over pairs[k0:].  Every operation of the start image is rounded separately in
 * fp32 (no fused multiply-add):  k = init * 2;  k = k + (-1);  a = ca * k;  b = cb * eps;  x = a + b  — bit for bit
 * q_sample(affine(init, 2, -1), t*, eps) of the existing kernels.  strength = 1 is no special case: all S entries from
 * q(x_{T-1} | init).
 */
#ifndef DMHOMO_HIP_START_H
#define DMHOMO_HIP_START_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* dmh_start_mix: one launch, B rows of per_sample elements:  out[i] = ca * (2 * init01[i] - 1) + cb * eps[i]  as above.
 * Exactly one noise source is given.
 *   noise != NULL (sample_ids == state == NULL): eps = noise.  out may be noise itself (in place); any other overlap of out
 *     with init01 or noise is refused.  Where the three pointers share their 16-byte phase the body moves 16-byte vectors.
 *   noise == NULL (sample_ids and state given): the keyed generator's next draw, computed in registers — value (seed =
 *     state[0], sample_ids[b], draw = state[1], element) exactly as dmh_rng_indexed(kind 0) gives it: Philox4x32-10, counter
 *     (element / 4, draw, sample id lo, sample id hi), key = seed, two Box-Muller calls for the four values of a counter.  Same
 *     grid plan and arrival ticket as dmh_rng_indexed: the last workgroup sets state[1] = draw + 1 and state[2] = 0, so the
 *     generator is left where one dmh_rng_indexed launch would have left it.  The noise never exists in memory.  The counter
 *     quads are anchored at element 0 of a row: 16-byte vectors where per_sample % 4 == 0 and init01 and out are 16-byte
 *     aligned, else element by element.
 * 1 <= B <= 65535, 1 <= per_sample < 2^31, ca and cb finite, float pointers 4-byte aligned (sample_ids, state: 8-byte).
 * Every check runs before anything is launched. */
int dmh_start_mix(const float* init01, const float* noise, const int64_t* sample_ids, uint64_t* state, float ca, float cb,
                  float* out, int B, int64_t per_sample, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* DMHOMO_HIP_START_H */
