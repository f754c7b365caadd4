/* mipnerf_preview_360.h -- C ABI of libmipnerf_preview_360.so: the baked preview of the UNBOUNDED-SCENE model.  The lattice of
 * mipnerf_preview.h (or the compact one of mipnerf_preview_sparse.h) spans a box of the CONTRACTED space z = contract(x) and is marched
 * along straight WORLD rays.  A seventh library: the other preview libraries and the drop-in library keep their entry points.
 *
 * Built by `python -m mipnerf_pl_amd.build` from csrc/kernels_preview_360.hip + csrc/preview_360_capi.hip; csrc/preview_march_360.hpp
 * states the rules below once, for the device and for a host compiler.  Conventions of mipnerf_preview.h: raw device pointers, the stream
 * as void*, 0 = ok, 1 = invalid argument, 2 = unsupported, 3 = HIP error, the message from the last-error call (thread-local); the
 * library never allocates and never synchronises, so every call can be captured into a hipGraph; every argument is validated before
 * any HIP call.
 *
 * Rows, the SH basis, the occupancy words, mipnerf_preview_params_t and the outputs of a miss are those of mipnerf_preview.h; its rules
 * 5 to 7 (early stop, outputs, determinism) hold unchanged.  A straight world ray is a curve in the contracted space, density is per
 * unit of WORLD length, and the step follows the lattice's cells in the CONTRACTED space:
 *
 * C1. Step.  s = step_scale * min(hx, hy, hz) of the lattice.  It is a length in the contracted space, formed on the host.
 * C2. Ray constants (directions are NOT normalised; t is in units of d; fp32 arithmetic, no contraction of products and sums).
 *     len = |d|, u = d / len, tc = -(o . u), m = o + tc u (the point nearest the centre), p2 = m . m, p = sqrt(p2),
 *     c = sqrt(4 p2 + 1), ts = sqrt(max(c - p2, 0)), half = sqrt(R^2 - p2), la = max(near len, tc - half), lb = min(far len, tc + half),
 *     R = far_radius.  The ray is a MISS when rule 2's finiteness, |d| or far <= near tests fail, or p2 >= R^2, or not la < lb; a miss is
 *     written exactly as rule 2 writes it.  There is no slab test: the interval is [near, far] cut by the ball of radius R.
 * C3. Warp.  tau is the world arclength from m.  W is odd.  For a = |tau| <= ts: W = tau.  Beyond: g = (a - ts) / (p2 + a ts),
 *     W = sign(tau) (ts + (c / p) atan(p g)); when p < 2^-20 the last term is c g.  Inverse V(w): for a = |w| <= ts: V = w.  Beyond:
 *     D = a - ts, q = tan(p D / c) / p (D / c when p < 2^-20), V = sign(w) (ts + q p2) / (1 - q ts).  Every value of V is clamped to
 *     [la - tc, lb - tc]; a denominator <= 0 gives the clamp's end on that side.  wa = W(la - tc), wb = W(lb - tc).
 * C4. Samples.  Sample i has w_i = wa + (float(i) + 0.5) s; it exists while w_i < wb and i < max_steps.  A hit ray shorter than half a
 *     step (w_0 >= wb) has the one sample w_0 = (wa + wb) / 2: no hit ray is left without a sample.  tau_i = V(w_i),
 *     t_i = (tc + tau_i) / len, x = o + t_i d, z = contract(x): x when |x| <= 1, else (2 - 1 / |x|) x / |x|.  Its world length is
 *     delta_i = max(e_{i+1} - e_i, 0) with edges e_k = V(min(wa + float(k) s, wb)), except that the upper edge of the last sample by w
 *     (the one with w_{i+1} >= wb) is V(wb) = lb - tc: it takes the remainder of less than half a step.  The deltas partition [la, lb]
 *     exactly (of a ray that max_steps cuts short: [la, e_max_steps]).
 * C5. Evaluation.  A sample with z outside the box on any axis contributes nothing (no clamping to the nearest face).  Otherwise the
 *     cell of z (lattice_sample.hpp), the occupancy bit, the blended row and the shading of rule 4, with
 *     alpha = 1 - exp(-(sigma * delta_i)) and Y from the WORLD direction u; dsum += w t_i.
 *
 * WHAT THE WARP GUARANTEES: for |x| = r > 1 the contracted point moves at |d contract(x) / d tau| <= min(1, c / r^2) (1 inside the unit
 * ball), and W' = min(1, c / (p2 + tau^2)) with r^2 = p2 + tau^2, so two consecutive samples are never more than s apart in the
 * contracted space, and a ray takes about (its contracted length) / s samples however far far_radius lies. */
#ifndef MIPNERF_PREVIEW_360_H
#define MIPNERF_PREVIEW_360_H

#include "mipnerf_preview_sparse.h"

#ifdef __cplusplus
extern "C" {
#endif

int mipnerf_preview_360_abi_version(void);      /* 1 */
const char* mipnerf_preview_360_last_error(void);
/* field: a lattice over a box of the contracted space; far_radius: finite, > 1.  origins / directions fp32 [n_rays, 3], near / far fp32
 * [n_rays]; rgb fp32 [n_rays, 3], acc / distance fp32 [n_rays]; steps int32 [n_rays] or NULL.  n_rays == 0 is ok whatever the ray
 * pointers. */
int mipnerf_preview_360_march(const mipnerf_preview_field_t* field, float far_radius, const mipnerf_preview_params_t* params, int64_t n_rays,
                              const float* origins, const float* directions, const float* near, const float* far, float* rgb, float* acc,
                              float* distance, int32_t* steps, void* stream);
/* the same over compact rows behind a row table (one level of mipnerf_preview_sparse.h): the bytes the dense lattice with the same
 * occupancy gives */
int mipnerf_preview_360_march_sparse(const mipnerf_preview_sparse_field_t* field, float far_radius, const mipnerf_preview_params_t* params,
                                     int64_t n_rays, const float* origins, const float* directions, const float* near, const float* far,
                                     float* rgb, float* acc, float* distance, int32_t* steps, void* stream);

#ifdef __cplusplus
}
#endif
#endif
