/* mipnerf_preview_tune_360.h -- C ABI of libmipnerf_preview_tune_360.so: TUNING A LATTICE OVER THE CONTRACTED SPACE THROUGH ITS OWN MARCH.
 * A ninth library: the gradient of mipnerf_preview_360_march (include/mipnerf_preview_360.h) with respect to the rows.  The other eight
 * libraries keep their entry points; the Adam pass (mipnerf_preview_tune_adam) and the regulariser of the tuning (the eighth library's
 * one entry point) are indifferent to the space a lattice lives in and are called unchanged.
 *
 * Built by `python -m mipnerf_pl_amd.build` from csrc/kernels_preview_tune_360.hip + csrc/preview_tune_360_capi.hip;
 * csrc/preview_tune_360.hpp states the rules below once, for the device and for a host compiler, and takes C1 - C5 from
 * csrc/preview_march_360.hpp and rules 8 / 10 from csrc/preview_tune.hpp by call.  Conventions of mipnerf_preview_tune.h: raw device
 * pointers, the stream as void*, 0 = ok, 1 = invalid argument, 2 = unsupported, 3 = HIP error, the message from the last-error call
 * (thread-local); the library never allocates and never synchronises; every argument is validated before any HIP call.
 *
 * THE GRADIENT (C1 - C5 are mipnerf_preview_360.h's, rules 5 - 7 mipnerf_preview.h's).  Along one ray the evaluated samples i = 0, 1, ...
 * have alpha_i, the clamped colour colour_i, the transmittance T_i before the sample (T_0 = 1, T_{i+1} = T_i (1 - alpha_i)) and the weight
 * w_i = T_i alpha_i; Y_k is the basis value k of the ray's WORLD direction, delta_i the sample's world length of C4.  G is the gradient of
 * the loss with respect to the ray's rgb, g_a the one with respect to its acc.  `distance` is not differentiated.
 * C6. q_i = sum_c G_c (colour_{i,c} - background_c) + g_a.                                                          (rule 8)
 * C7. The gradient of the BLENDED row of sample i (rule 9 with the sample's own world length):
 *       d row[0]          = delta_i (T_{i+1} q_i - S_i)  where row[0] > 0, else 0, with S_i = sum_{j > i} w_j q_j (no division);
 *                           delta_i = max(e_{i+1} - e_i, 0) is the number the forward formed alpha_i with,
 *       d row[1 + 3k + c] = w_i G_c Y_k                  where the colour before its clamp lies strictly inside (0, 1), else 0,
 *       d row[pad]        = 0.
 * C8. Corner (a, b, c) of the cell of z = contract(x) receives (wx_a wy_b) wz_c * d row, the weights (1 - f, f) per axis from the
 *     fractions of that cell (rule 10).
 * Sample positions, delta_i, the warp and the contraction depend on the ray only: no gradient flows through them.  Samples outside the
 * box, samples in clear cells, samples behind the early stop, rays that miss (C2) and rays whose rgb, acc, G or g_a is not finite add
 * nothing: a NaN row spoils the outputs of the rays through it, as in the march, and receives and causes no gradient.
 *
 * NOT BITWISE REPRODUCIBLE: the contributions of different rays to one row entry are added with float atomics and arrive in no fixed
 * order, so grad_rows of two runs on the same inputs may differ in the last bits; rgb and acc do not depend on it.  The contributions of
 * ONE ray arrive in a fixed order. */
#ifndef MIPNERF_PREVIEW_TUNE_360_H
#define MIPNERF_PREVIEW_TUNE_360_H

#include <stdint.h>

#include "mipnerf_preview.h"

#ifdef __cplusplus
extern "C" {
#endif

int mipnerf_preview_tune_360_abi_version(void);      /* 1 */
const char* mipnerf_preview_tune_360_last_error(void);
/* The march of one DENSE lattice over a box of the contracted space and its gradient with respect to the rows, in one launch.  field,
 * far_radius, params and the rays: as for mipnerf_preview_360_march (field.occupancy may be NULL; far_radius finite and > 1), everything
 * it checks is checked.  The loss side is exactly one of
 *     grad_rgb fp32 [n_rays, 3]:  G = grad_rgb                                      (then target must be NULL; loss_scale is ignored)
 *     target   fp32 [n_rays, 3]:  G_c = loss_scale * (rgb_c - target_c), rgb this launch's own output; loss_scale finite
 * grad_acc fp32 [n_rays] or NULL (g_a = 0).  rgb fp32 [n_rays, 3] and acc fp32 [n_rays], never NULL, receive the bytes
 * mipnerf_preview_360_march writes for the same inputs.  grad_rows fp32 [nz, ny, nx, W], 16-byte aligned, is ADDED INTO: the caller zeroes
 * it; its pad entries are never written.  counters: NULL, or two device uint64 that are added to: [0] the samples that added something,
 * [1] the flushes (runs of consecutive samples of a ray in one cell; each flush is 1 / 2 / 4 atomic wave instructions for degree
 * 0 / 1 / 2).  n_rays == 0 is ok whatever the ray pointers. */
int mipnerf_preview_tune_360_grad(const mipnerf_preview_field_t* field, float far_radius, const mipnerf_preview_params_t* params,
                                  int64_t n_rays, const float* origins, const float* directions, const float* near, const float* far,
                                  const float* grad_rgb, const float* target, float loss_scale, const float* grad_acc, float* rgb, float* acc,
                                  float* grad_rows, uint64_t* counters, void* stream);

#ifdef __cplusplus
}
#endif
#endif
