/* mipnerf_preview.h -- C ABI of libmipnerf_preview.so: a trained field BAKED into a dense lattice of fp16 rows (density + spherical-
 * harmonic colour) and ray-marched without the MLP.  Not part of the drop-in library (include/mipnerf_hip.h keeps its 93 entry points).
 *
 * Built next to libmipnerf_hip.so by `python -m mipnerf_pl_amd.build` from csrc/kernels_preview.hip + csrc/preview_capi.hip;
 * csrc/preview_march.hpp states the per-sample rules once, for the device and for a host compiler, and takes the cell index and the
 * trilinear fractions from csrc/lattice_sample.hpp.  Same conventions as mipnerf_hip.h: raw device pointers, the stream as void*,
 * 0 = ok, 1 = invalid argument, 2 = unsupported, 3 = HIP error, the message from the last-error call (thread-local).  The library depends on the
 * HIP runtime only; it never allocates and never synchronises, so every call can be captured into a hipGraph.  Arguments are validated
 * before any HIP call.
 *
 * THE BAKED PICTURE IS NOT THE MLP'S PICTURE: colour is a low-order expansion in the view direction, density and colour are blended
 * trilinearly between lattice points, and the march uses point samples (no cone, no anti-aliasing).
 *
 * ROWS.  The lattice has mipnerf_density_grid's geometry: dims = (nx, ny, nz) points, point (i, j, k) at lo + float(i) * h per axis,
 * h = (hi - lo) / float(n - 1), flat index (k * ny + j) * nx + i.  One point is one row of W fp16 values, W = 4, 16, 32 for degree 0, 1, 2
 * (8, 32, 64 bytes: one, two or four 16-byte loads; the 8-byte row is one 8-byte load):
 *     row[0]           = sigma
 *     row[1 + 3 k + c] = coefficient of basis function k, channel c        k < (degree + 1)^2, c < 3
 *     the rest         = 0
 * Values are rounded to nearest even; a sigma above the fp16 maximum 65504 is stored as 65504, not as inf; NaN stays NaN.
 * The basis is the real spherical harmonics in the order and signs of PlenOctrees, on the unit direction (x, y, z) = d / |d|:
 *     Y = [C0, -C1 y, C1 z, -C1 x, C20 x y, C21 y z, C22 (2 z z - x x - y y), C23 x z, C24 (x x - y y)]
 *     C0 = 0.28209479177387814, C1 = 0.4886025119029199,
 *     C2 = (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)
 *
 * MARCHING RULES (directions are NOT normalised, t is in units of d, as everywhere in this project; fp32 arithmetic, no contraction):
 * 1. Step size.  h = (hi - lo) / float(n - 1) per axis, s = step_scale * min(hx, hy, hz) is the world step, dt = s / |d|.
 * 2. Interval.  [ta, tb] = [near, far] intersected with the slab interval of the box: per axis with d != 0 the two values (lo - o) / d and
 *    (hi - o) / d; an axis with d == 0 exactly is a test lo <= o <= hi on the origin alone, not a division.  A ray is a MISS when its
 *    origin or direction is not finite, |d| = 0 (or |d| is not finite in fp32), near or far is not finite, far <= near, or not ta < tb.
 *    A miss gets rgb = background, acc = 0, distance = near (far when near is not finite, 0 when neither is) and steps = 0.
 * 3. Samples.  Sample i sits at t_i = ta + (float(i) + 0.5) * dt; it exists while t_i < tb and i < max_steps; x = o + t_i * d.
 * 4. Evaluation.  The cell comes from the index rule of lattice_sample.hpp (clamped into the box).  If the cell's occupancy bit is
 *    clear the sample contributes nothing and loads no row.  Otherwise row = the trilinear blend of the 8 corner rows, each converted to
 *    fp32 and blended in fp32 (along x, then y, then z, each step (1 - f) * a + f * b), and
 *        sigma = max(row[0], 0)        colour_c = clamp(sum_k row[1 + 3 k + c] * Y_k, 0, 1)        (a NaN stays a NaN in both)
 *        alpha = 1 - exp(-sigma * s)   w = T * alpha
 *        rgb += w * colour, acc += w, dsum += w * t_i, T *= 1 - alpha                    (T starts at 1)
 * 5. Early stop.  The march stops after the first sample at which T < t_min (T after that sample's update).  t_min = 0 never stops early.
 * 6. Outputs.  rgb += (1 - acc) * background; distance = clamp(dsum / acc, near, far), near when acc == 0.  A NaN sigma or colour makes
 *    that ray's rgb, acc and distance NaN and touches no other ray.  steps = the samples actually evaluated (existing, occupied, not
 *    behind the early stop).
 * 7. Determinism.  No atomics; the sums of a ray are taken in a fixed order: two runs give the same bytes. */
#ifndef MIPNERF_PREVIEW_H
#define MIPNERF_PREVIEW_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct {
    int32_t dims[3];              /* (nx, ny, nz) lattice points, each >= 2, 7 nx ny nz < 2^31 */
    float lo[3], hi[3];           /* the box, (x, y, z) order, hi > lo */
    int32_t degree;               /* 0, 1 or 2 */
    const void* rows;             /* fp16 [nz, ny, nx, W], 16-byte aligned (8 for degree 0) */
    const uint32_t* occupancy;    /* [nz - 1, ny - 1, ceil((nx - 1) / 32)] words, cell i of an x row = bit i & 31 of word i >> 5
                                     (the layout of mipnerf_occupancy_build); NULL: every cell is occupied */
} mipnerf_preview_field_t;

typedef struct {
    float step_scale;             /* > 0 */
    float t_min;                  /* in [0, 1) */
    int32_t max_steps;            /* >= 1 */
    float background[3];
} mipnerf_preview_params_t;

int mipnerf_preview_abi_version(void);          /* 1 */
const char* mipnerf_preview_last_error(void);
/* rows [nz, ny, nx, W] from sigma fp32 [nz, ny, nx] and coef fp32 [nz, ny, nx, (degree + 1)^2, 3].  mask: one byte per lattice point or
 * NULL; 0 = the point's colour coefficients are written as zeros (its sigma is kept).  dims = (nx, ny, nz). */
int mipnerf_preview_pack(const int32_t* dims, int32_t degree, const float* sigma, const float* coef, const uint8_t* mask, void* rows,
                         void* stream);
/* origins / directions fp32 [n_rays, 3], near / far fp32 [n_rays]; rgb fp32 [n_rays, 3], acc / distance fp32 [n_rays]; steps int32
 * [n_rays] or NULL.  n_rays == 0 is ok whatever the ray pointers. */
int mipnerf_preview_march(const mipnerf_preview_field_t* field, const mipnerf_preview_params_t* params, int64_t n_rays,
                          const float* origins, const float* directions, const float* near, const float* far, float* rgb, float* acc,
                          float* distance, int32_t* steps, void* stream);

#ifdef __cplusplus
}
#endif
#endif
