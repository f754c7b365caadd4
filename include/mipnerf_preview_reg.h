/* mipnerf_preview_reg.h -- C ABI of libmipnerf_preview_reg.so: REGULARISING THE TUNING OF THE BAKED LATTICE.  An eighth library: the
 * drop-in library (include/mipnerf_hip.h), the measurement library (include/mipnerf_diag.h) and the five preview libraries
 * (include/mipnerf_preview.h, _mip.h, _sparse.h, _tune.h, _360.h) keep their entry points and their ABI versions.
 *
 * Built by `python -m mipnerf_pl_amd.build` from csrc/kernels_preview_reg.hip + csrc/preview_reg_capi.hip; csrc/preview_reg.hpp states
 * rules R1 - R4 once, for the device and for a host compiler, with the order of every sum.  Conventions of mipnerf_preview.h: raw device
 * pointers, the stream as void*, 0 = ok, 1 = invalid argument, 2 = unsupported, 3 = HIP error, the message from the last-error call
 * (thread-local); the library never allocates and never synchronises; every argument is validated before any HIP call.
 *
 * THE TERMS, on the fp32 master rows v[p][e] of a lattice (the row layout of mipnerf_preview.h: entry 0 is sigma, entries 1 .. 3 (degree +
 * 1)^2 the colour coefficients, coefficient k of channel c at 1 + 3 k + c, the rest of the W = 4 / 16 / 32 entries padding).  A point is
 * PRESENT when it lies inside the lattice and its mask byte is not 0.
 *   total variation   sum over the present p and the used e of w n(p), w = w_sigma for e == 0, else w_colour, with
 *                     n(p) = sqrtf(((dx dx + dy dy) + dz dz) + eps),  d_a = scale_a (v[p + e_a][e] - v[p][e]) when p + e_a is present, else 0
 *   SH decay          0.5 w_view v[p][e]^2 over the present p and the entries e >= 4 (the coefficients of k >= 1; none at degree 0)
 * The entry point adds the GRADIENT of their sum; the value itself is not formed on the device.  Every operation rounds once and in the
 * order csrc/preview_reg.hpp writes down; the result is a gather from master alone, so two calls on the same inputs give the same bytes.
 * A non-finite master entry v[q][e] spoils only grad entries [p][e] with p = q, q +- e_a or q + e_a - e_b present (exactly which:
 * csrc/preview_reg.hpp), and only through a term whose weight is not 0. */
#ifndef MIPNERF_PREVIEW_REG_H
#define MIPNERF_PREVIEW_REG_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

int mipnerf_preview_reg_abi_version(void);      /* 1 */
const char* mipnerf_preview_reg_last_error(void);
/* grad += the gradient of the two terms above.  dims = {nx, ny, nz}: at least 2 points per axis and 7 nx ny nz < 2^31 (a lattice with a
 * 0 among its sizes has no points: ok whatever the pointers).  scale = {hmin / h_x, hmin / h_y, hmin / h_z}, positive and finite, formed by
 * the caller in fp32 (1 on a cubic lattice).  master fp32 [nz, ny, nx, W] and grad fp32 [nz, ny, nx, W]: 16-byte aligned; mask: one byte
 * per point or NULL (every point).  grad is ADDED INTO at the used entries of the present points and at no other byte: pad entries and the
 * rows of points that are not present are neither read nor written; master rows of such points are not read.  The weights are finite and
 * >= 0, eps is finite and > 0; with all three weights 0 the call checks its arguments and launches nothing. */
int mipnerf_preview_reg_grad(const int32_t* dims, int32_t degree, const float* scale, const float* master, const uint8_t* mask, float* grad,
                             float w_sigma, float w_colour, float w_view, float eps, void* stream);

#ifdef __cplusplus
}
#endif
#endif
