/* mipnerf_proposal_360.h -- C ABI of libmipnerf_proposal_360.so: THE PROPOSAL DENSITY OF THE UNBOUNDED-SCENE MODEL, read from a small
 * pyramid of contracted density lattices instead of an MLP pass.  A tenth library: the drop-in library (include/mipnerf_hip.h), the
 * measurement library (include/mipnerf_diag.h) and the seven preview libraries keep their entry points and their ABI versions.
 *
 * Built by `python -m mipnerf_pl_amd.build` from csrc/kernels_proposal_360.hip + csrc/proposal_360_capi.hip; csrc/lattice_sample_360.hpp
 * states rules Q1 - Q4 once, for the device and for a host compiler.  Conventions of mipnerf_hip.h: raw device pointers, the stream as
 * void*, 0 = ok, 1 = invalid argument, 2 = unsupported, 3 = HIP error, the message from the last-error call (thread-local); the library
 * never allocates and never synchronises; every argument is validated before any HIP call.
 *
 * THE PYRAMID.  L levels, 1 <= L <= 4, all over the same box lo .. hi of the CONTRACTED space ((x, y, z) order; the usual box is
 * [-2, 2]^3).  Level l is an fp32 device lattice [nz_l, ny_l, nx_l] in mipnerf_density_grid's layout (point (i, j, k) at lo + float(i) * h
 * per axis, flat index (k * ny + j) * nx + i), at least 2 points per axis and 7 nx ny nz < 2^31.  spacing[l] = max over the axes of
 * (hi - lo) / float(n_l - 1) is formed by the library on the host in fp32 and must increase strictly with l.  A level is meant to be
 * mipnerf_density_grid_360(space = contracted) at its own spacing: a coarser lattice baked at its own lattice Gaussian is the field
 * pre-filtered at that spacing by the model's own encoding.
 *
 * THE RULE, for the sample [t_i, t_{i+1}] of ray b (every operation rounds once, in the order csrc/lattice_sample_360.hpp writes down):
 *   Q1  G = the contracted full-covariance Gaussian of the conical frustum: the mean and covariance mipnerf_cast_ipe_360(contracted = 1)
 *       encodes and returns, bit for bit (csrc/raymath360.hpp, conical_frustum_to_gaussian_full)
 *   Q2  w = footprint * (2.0f * sqrtf((cov_xx + cov_yy) + cov_zz)): the side of the uniform box whose per-axis variance w^2 / 12 equals the
 *       Gaussian's mean per-axis variance (footprint = 1); the yardstick a lattice Gaussian of cov_scale = 1 is baked at.  footprint = 0
 *       always reads level 0.
 *   Q3  (l, g) = mip_level(spacing, L, w) of mipnerf_preview_mip.h (P4): w <= spacing[0] or not a number -> (0, 0); w >= spacing[L - 1] ->
 *       (L - 1, 0); else spacing[l] <= w < spacing[l + 1] and g = (w - spacing[l]) / (spacing[l + 1] - spacing[l])
 *   Q4  v = the trilinear value of level l at G's mean (the rule of mipnerf_lattice_density: i0 = min(int(floorf(u)), n - 2), blended
 *       along x, then y, then z as (1 - f) * a + f * b); only when g > 0: v = (1 - g) * v + g * (the trilinear value of level l + 1).
 *       The upper level is not loaded when g == 0, so with L == 1 the value is the plain trilinear value at the contracted mean.
 * A non-finite mean gives 0 and loads nothing; a NaN covariance reads level 0; a NaN corner propagates; a mean outside the box takes the
 * edge value (|contract(x)| < 2: with the usual box there is none).  The clamp of the trilinear rule keeps every load inside its level,
 * whatever the ray. */
#ifndef MIPNERF_PROPOSAL_360_H
#define MIPNERF_PROPOSAL_360_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MIPNERF_PROPOSAL_MAX_LEVELS 4

typedef struct mipnerf_proposal_pyramid {      /* a host struct with device lattice pointers */
    int32_t levels;                                        /* L: 1 .. MIPNERF_PROPOSAL_MAX_LEVELS */
    int32_t dims[MIPNERF_PROPOSAL_MAX_LEVELS][3];          /* {nx, ny, nz} of level l */
    const float* lattice[MIPNERF_PROPOSAL_MAX_LEVELS];     /* fp32 [nz, ny, nx] of level l */
    float lo[3], hi[3];                                    /* the box every level spans */
} mipnerf_proposal_pyramid;

int mipnerf_proposal_360_abi_version(void);      /* 1 */
const char* mipnerf_proposal_360_last_error(void);
/* The stage on its own: rgb_sigma[b, i] = (0, 0, 0, v of rule Q4) as [num_rays, num_samples, 4] fp32, one 16-byte store per sample --
 * the buffer the compositing kernels read after an MLP pass.  t_samples [num_rays, num_samples + 1], origins / directions [num_rays, 3],
 * radii [num_rays].  Invalid (1) before any device call: a null pointer, levels outside 1 .. 4, an axis < 2, hi <= lo, 7 nx ny nz >= 2^31,
 * spacings not strictly increasing, footprint negative or not finite, num_samples outside 1 .. 1024, num_rays outside [0, 2^31).
 * num_rays = 0 returns without a launch, whatever the ray pointers. */
int mipnerf_lattice_density_360(const mipnerf_proposal_pyramid* pyramid, float footprint, int64_t num_rays, int32_t num_samples,
                                const float* t_samples, const float* origins, const float* directions, const float* radii, float* rgb_sigma,
                                void* stream);
/* t[i] = 1.0f / t_inv[i] for i < n: the step between resampling the inverse-depth fence posts and encoding the fine level, with the bits of
 * the drop-in library's own level loop.  n = 0 returns without a launch. */
int mipnerf_reciprocal_360(int64_t n, const float* t_inv, float* t, void* stream);

#ifdef __cplusplus
}
#endif
#endif
