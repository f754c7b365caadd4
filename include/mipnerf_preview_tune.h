/* mipnerf_preview_tune.h -- C ABI of libmipnerf_preview_tune.so: FINE-TUNING THE BAKED LATTICE THROUGH ITS OWN RENDERER.  A sixth library:
 * libmipnerf_preview.so (include/mipnerf_preview.h) keeps its 4 entry points, libmipnerf_preview_mip.so (include/mipnerf_preview_mip.h) its
 * 3, libmipnerf_preview_sparse.so (include/mipnerf_preview_sparse.h) its 7 and the drop-in library (include/mipnerf_hip.h) its 93.
 *
 * Built by `python -m mipnerf_pl_amd.build` from csrc/kernels_preview_tune.hip + csrc/preview_tune_capi.hip; csrc/preview_tune.hpp states
 * rules 8 - 10 and the Adam rule once, for the device and for a host compiler, and takes rules 1 - 5 from csrc/preview_march.hpp by call.
 * Conventions of mipnerf_preview.h: raw device pointers, the stream as void*, 0 = ok, 1 = invalid argument, 2 = unsupported, 3 = HIP
 * error, the message from the last-error call (thread-local); the library never allocates and never synchronises; every argument is
 * validated before any HIP call.
 *
 * THE GRADIENT (rules 1 - 7 are mipnerf_preview.h's).  Along one ray the evaluated samples i = 0, 1, ... have alpha_i, the clamped colour
 * colour_i, the transmittance T_i before the sample (T_0 = 1, T_{i+1} = T_i (1 - alpha_i)) and the weight w_i = T_i alpha_i; Y_k is the
 * ray's basis value k, s the world step of rule 1.  G is the gradient of the loss with respect to the ray's rgb, g_a the one with respect
 * to its acc.  `distance` is not differentiated.
 *  8. q_i = sum_c G_c (colour_{i,c} - background_c) + g_a.
 *  9. The gradient of the BLENDED row of sample i:
 *       d row[0]          = s (T_{i+1} q_i - S_i)  where row[0] > 0, else 0, with S_i = sum_{j > i} w_j q_j (no division),
 *       d row[1 + 3k + c] = w_i G_c Y_k            where the colour before its clamp lies strictly inside (0, 1), else 0,
 *       d row[pad]        = 0.
 * 10. Corner (a, b, c) of the sample's cell receives (wx_a wy_b) wz_c * d row, the weights (1 - f, f) per axis from the fractions of rule 4.
 *     Samples in clear cells, samples behind the early stop, rays that miss and rays whose rgb, acc, G or g_a is not finite add nothing:
 *     a NaN row spoils the outputs of the rays through it, as in the march, and receives and causes no gradient.
 *
 * NOT BITWISE REPRODUCIBLE: the contributions of different rays to one row entry are added with float atomics and arrive in no fixed
 * order, so grad_rows of two runs on the same inputs may differ in the last bits.  This is the only entry point of the preview libraries
 * for which that is so; rgb and acc do not depend on it.  The contributions of ONE ray arrive in a fixed order. */
#ifndef MIPNERF_PREVIEW_TUNE_H
#define MIPNERF_PREVIEW_TUNE_H

#include <stdint.h>

#include "mipnerf_preview.h"

#ifdef __cplusplus
extern "C" {
#endif

int mipnerf_preview_tune_abi_version(void);      /* 1 */
const char* mipnerf_preview_tune_last_error(void);
/* The march of one dense lattice and its gradient with respect to the rows, in one launch.  field, params and the rays: as for
 * mipnerf_preview_march (field.occupancy may be NULL), everything it checks is checked.  The loss side is exactly one of
 *     grad_rgb fp32 [n_rays, 3]:  G = grad_rgb                                      (then target must be NULL; loss_scale is ignored)
 *     target   fp32 [n_rays, 3]:  G_c = loss_scale * (rgb_c - target_c), rgb this launch's own output; loss_scale finite
 * grad_acc fp32 [n_rays] or NULL (g_a = 0).  rgb fp32 [n_rays, 3] and acc fp32 [n_rays], never NULL, receive the bytes
 * mipnerf_preview_march writes for the same inputs.  grad_rows fp32 [nz, ny, nx, W], 16-byte aligned, is ADDED INTO: the caller zeroes it;
 * its pad entries are never written.  counters: NULL, or two device uint64 that are added to: [0] the samples that added something, [1]
 * the flushes (runs of consecutive samples of a ray in one cell; each flush is 1 / 2 / 4 atomic wave instructions for degree 0 / 1 / 2).
 * n_rays == 0 is ok whatever the ray pointers. */
int mipnerf_preview_tune_grad(const mipnerf_preview_field_t* field, const mipnerf_preview_params_t* params, int64_t n_rays,
                              const float* origins, const float* directions, const float* near, const float* far, const float* grad_rgb,
                              const float* target, float loss_scale, const float* grad_acc, float* rgb, float* acc, float* grad_rows,
                              uint64_t* counters, void* stream);
/* One Adam step on n_points rows and their repack to fp16, in one pass.  master, m, v, grad: fp32 [n_points, W], 16-byte aligned; rows:
 * fp16 [n_points, W], 8-byte aligned; mask: one byte per point or NULL.  Per used entry e < 1 + 3 (degree + 1)^2 of a point whose mask
 * byte is not 0, in this order, every operation rounded once:
 *     m = beta1 m + (1 - beta1) g;   v = beta2 v + (1 - beta2) (g g);   p = p - lr ((m c1) / (sqrtf(v c2) + eps)), lr = lr_sigma for
 *     e == 0, else lr_colour;   rows[e] = p rounded to fp16 as mipnerf_preview_pack rounds it (sigma saturates at 65504);   g = 0.
 * A point whose mask byte is 0 gets g = 0 only.  Pad entries keep their values in all five arrays.  c1 = 1 / (1 - beta1^t) and
 * c2 = 1 / (1 - beta2^t) are the bias corrections of step t, formed by the caller.  n_points == 0 is ok whatever the pointers. */
int mipnerf_preview_tune_adam(int64_t n_points, int32_t degree, float* master, float* m, float* v, float* grad, void* rows,
                              const uint8_t* mask, float lr_sigma, float lr_colour, float beta1, float beta2, float eps, float c1, float c2,
                              void* stream);

#ifdef __cplusplus
}
#endif
#endif
