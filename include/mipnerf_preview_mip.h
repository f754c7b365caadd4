/* mipnerf_preview_mip.h -- C ABI of libmipnerf_preview_mip.so: the baked preview marched through a PYRAMID of lattices, the level of every
 * sample chosen by the width of the ray's cone there, so the preview is anti-aliased.  A fourth library: libmipnerf_preview.so
 * (include/mipnerf_preview.h) keeps its 4 entry points and the drop-in library (include/mipnerf_hip.h) its 93.
 *
 * Built by `python -m mipnerf_pl_amd.build` from csrc/kernels_preview_mip.hip + csrc/preview_mip_capi.hip; csrc/preview_mip.hpp states
 * the level rule and the mix of two rows once, for the device and for a host compiler, and takes everything else from
 * csrc/preview_march.hpp.  Conventions of mipnerf_preview.h: raw device pointers, the stream as void*, 0 = ok, 1 = invalid argument,
 * 2 = unsupported, 3 = HIP error, the message from the last-error call (thread-local); the library never allocates and never
 * synchronises, so the call can be captured into a hipGraph; every argument is validated before any HIP call.
 *
 * WHY COARSER LATTICES ARE THE RIGHT PRE-FILTER: `bake_field` evaluates the field at the lattice Gaussian of the lattice spacing (variance
 * h^2 / 12 per axis), i.e. with the model's own integrated positional encoding.  A lattice of twice the spacing baked the same way is
 * the field pre-filtered at twice the scale; no other filter is involved.  The rules below only say WHICH lattice a sample reads.
 *
 * RULES (rules 1 - 7 are those of mipnerf_preview.h; fp32 arithmetic, no contraction):
 * P1. Pyramid.  L levels, 1 <= L <= 8, each a mipnerf_preview_field_t.  All levels have the same lo and hi, bit for bit, and the same
 *     degree; each has its own dims (each >= 2), its own rows (the row alignment rule of mipnerf_preview_march) and its own occupancy
 *     words or NULL.  s_l = the smallest axis spacing of level l, with the fp32 h = (hi - lo) / float(n - 1) of rule 1.
 *     s_0 < s_1 < ... < s_{L-1} strictly; anything else is invalid (code 1).
 * P2. Ray and step.  Rules 1 - 3 hold unchanged on level 0: the world step is s = step_scale * s_0, and the interval, the miss rules and
 *     t_i = ta + (float(i) + 0.5) * dt are the same.  In addition a ray whose radius is not finite or is negative is a miss.
 * P3. Footprint.  k = footprint * radius, formed once per ray, and w_i = k * t_i.  t is in units of d and the cone's world radius at t is
 *     radius * t with no |d| factor, as in cast_rays.  footprint is finite and >= 0, otherwise the call is invalid.  With
 *     radii = dx / sqrt(3) (the data sets' convention) footprint = sqrt(3) makes w one pixel's width; that value is a choice.
 * P4. Level.  If L == 1 or w <= s_0 (a w that is not a number counts as such): l = 0, g = 0.  If w >= s_{L-1}: l = L - 1, g = 0.
 *     Otherwise l is the largest level with s_l <= w and g = (w - s_l) / (s_{l+1} - s_l).  lambda_i = float(l) + g.
 * P5. Evaluation.  cell_l and the fractions come from the index rule of lattice_sample.hpp on level l's lattice (and, when g > 0, cell_{l+1}
 *     on level l + 1's).  A sample is OCCUPIED iff bit_l(cell_l) is set, or g > 0 and bit_{l+1}(cell_{l+1}) is set; a NULL occupancy
 *     counts as set.  An unoccupied sample contributes nothing and loads no row.  Otherwise row_l is the trilinear blend of rule 4 and,
 *     when g > 0, row = (1 - g) * row_l + g * row_{l+1} per element (row_{l+1} blended on its own level's cell); then sigma, colour,
 *     alpha (with s) and the sums follow exactly as in rule 4.
 * P6. Early stop, outputs and determinism are rules 5 - 7.  One more optional output: lod = sum_i w_i lambda_i / acc with the
 *     compositing weights w_i = T alpha of rule 4 (not P3's footprint), 0 when acc == 0 and for a miss.
 * P7. With L == 1, or with footprint * radius == 0 for a ray, that ray's rgb, acc, distance and steps are bit for bit
 *     mipnerf_preview_march's on level 0: the shared functions are called in the same order, with the same lane mapping and reductions. */
#ifndef MIPNERF_PREVIEW_MIP_H
#define MIPNERF_PREVIEW_MIP_H

#include "mipnerf_preview.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    int32_t levels;                       /* L, 1 .. 8 */
    mipnerf_preview_field_t level[8];     /* level[0] the finest; entries from L on are ignored */
} mipnerf_preview_pyramid_t;

int mipnerf_preview_mip_abi_version(void);      /* 1 */
const char* mipnerf_preview_mip_last_error(void);
/* origins / directions fp32 [n_rays, 3], radii / near / far fp32 [n_rays]; rgb fp32 [n_rays, 3], acc / distance fp32 [n_rays]; steps int32
 * [n_rays] or NULL; lod fp32 [n_rays] or NULL.  n_rays == 0 is ok whatever the ray pointers. */
int mipnerf_preview_mip_march(const mipnerf_preview_pyramid_t* pyramid, const mipnerf_preview_params_t* params, float footprint,
                              int64_t n_rays, const float* origins, const float* directions, const float* radii, const float* near,
                              const float* far, float* rgb, float* acc, float* distance, int32_t* steps, float* lod, void* stream);

#ifdef __cplusplus
}
#endif
#endif
