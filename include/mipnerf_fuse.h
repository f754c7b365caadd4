/* mipnerf_fuse.h -- C ABI of libmipnerf_fuse.so: RENDERED DEPTH FUSED INTO A TRUNCATED SIGNED DISTANCE VOLUME, whose zero level set is a
 * mesh that needs no density threshold.  An eleventh library: the drop-in library (include/mipnerf_hip.h), the measurement library
 * (include/mipnerf_diag.h), the seven preview libraries and the proposal library keep their entry points and their ABI versions.
 *
 * Built by `python -m mipnerf_pl_amd.build` from csrc/kernels_fuse.hip + csrc/fuse_capi.hip; csrc/fuse_rules.hpp states rules D, P, T and F
 * once, for the device and for a host compiler.  Conventions of mipnerf_hip.h: raw device pointers, the stream as void*, 0 = ok,
 * 1 = invalid argument, 2 = unsupported, 3 = HIP error, the message from the last-error call (thread-local); the library never allocates
 * and never synchronises; every argument is validated before any HIP call.
 *
 * D  THE DEPTH QUANTILE OF ONE RAY.  Inputs: weights w_i, i < N, and fence posts t_0 .. t_N in world distances, as mipnerf_forward returns
 *    a level's `weights` and `t_samples`; an opacity q, 0 < q < 1.
 *   D1  w'_i = fmaxf(w_i, 0.0f): NaN and negative weights count 0
 *   D2  P_i = sum_{j <= i} w'_j in double, P_{-1} = 0: ONE array of inclusive prefixes, and both ends of every interval's test come from
 *       it, so exactly one interval satisfies P_{i-1} < q <= P_i, or none does
 *   D3  for that i, f = (q - P_{i-1}) / w'_i in double, clamped to [0, 1]; the depth is (float)(t_i + f * (t_{i+1} - t_i)), rounded once
 *   D4  no interval qualifies (P_{N-1} < q: the ray does not reach opacity q): the depth is +inf
 *    q is an opacity, not a share of acc, so a ray that misses the object has no depth.  The device sums a lane's samples, then the lanes
 *    (a double wave scan); the host sums in sample order: the prefixes agree to the rounding of double sums of fp32 values.
 *
 * P  THE PROJECTION ROW OF A CAMERA RECORD (the 32 floats of mipnerf_generate_rays), formed on the host in double and rounded to fp32 once;
 *    camera modes 0 and 1.  pix2cam: mode 1's matrix, whose last row must be (0, 0, -1); mode 0's equivalent
 *    ((1/focal, 0, -W/(2 focal)), (0, -1/focal, H/(2 focal)), (0, 0, -1)).  cam2pix = pix2cam^-1, R | o = c2w, and
 *    P = cam2pix [R^T | -R^T o], 3 x 4.  (a, b, t) = P (p, 1): t is the ray parameter of p (these cameras' directions have z = -1, so t
 *    is the camera's z-depth) and (a / t, b / t) the continuous pixel coordinate, pixel (x, y) covering [x, x+1) x [y, y+1).  The frame
 *    record is 16 floats: P[3][4] | W, H, near, far.  Modes 2 and 3 (distorted cameras) are refused by name: fuse ideal pinhole frames of
 *    the capture's K instead.
 *
 * T  INTEGRATING FRAME f INTO LATTICE POINT (i, j, k); frames are taken in order.  The state is two fp32 planes [nz, ny, nx], `sum` and
 *    `count`, in mipnerf_density_grid's layout (flat index (k * ny + j) * nx + i).
 *   T1  p = lo + float(i) * h per axis, h = (hi - lo) / float(n - 1) formed on the host in fp32
 *   T2  a = (P00 x + P01 y) + (P02 z + P03) in fp32, likewise b and t; u = floorf(a / t), v = floorf(b / t); skipped unless
 *       near_f < t <= far_f, 0 <= u < W_f and 0 <= v < H_f
 *   T3  D = depth[offset_f + v * W_f + u], the nearest pixel; skipped unless D > 0 (NaN, 0, negative values and -inf)
 *   T4  D == +inf: d = 1, the ray is free over [near, far]; with carve = 0 such a pixel is skipped instead
 *   T5  otherwise s = D - t; skipped if s < -trunc; else d = fminf(1.0f, s / trunc)
 *   T6  sum += d; count += 1.0f
 *    No atomics: a point's sums associate in frame order whatever the launch split, so two runs, or one call of F frames against F calls
 *    of one frame, give the same bytes.  A pixel index outside [0, depth_count) is skipped, never read.
 *
 * F  FINALISE.  lattice = count > 0 ? -(sum / count) : fill; fill = +1 calls a point no frame updated inside (space carving: a point
 *    deeper than trunc behind every view's surface is never updated), -1 outside.  The lattice goes to mipnerf_isosurface_count / _emit at
 *    threshold 0, whose inside is lattice > 0. */
#ifndef MIPNERF_FUSE_H
#define MIPNERF_FUSE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MIPNERF_FUSE_MAX_QUANTILES 4
#define MIPNERF_FUSE_FRAME_FLOATS 16
/* frames one launch of the integration kernel takes; mipnerf_fuse_integrate splits any number of frames into such launches.  The frame
 * records are read from memory by the loop counter, so the kernel's registers allow any number; measured, the time per frame falls up to
 * 8 frames per launch and RISES beyond, where the launch's depth maps no longer stay in the L2 caches. */
#define MIPNERF_FUSE_FRAMES_PER_LAUNCH 8

int mipnerf_fuse_abi_version(void);      /* 1 */
const char* mipnerf_fuse_last_error(void);
/* Rule D for num_quantiles opacities q (HOST array) at once: depth [num_rays, num_quantiles] fp32.  weights [num_rays, num_samples],
 * t_samples [num_rays, num_samples + 1].  Invalid (1) before any device call: a null pointer, num_samples outside 1 .. 1024,
 * num_quantiles outside 1 .. 4, a q outside (0, 1), num_rays outside [0, 2^31).  num_rays = 0 returns without a launch. */
int mipnerf_fuse_depth_quantile(int64_t num_rays, int32_t num_samples, const float* weights, const float* t_samples, int32_t num_quantiles,
                                const float* q, float* depth, void* stream);
/* Rule P, host only: camera (32 HOST floats) -> frame (16 HOST floats).  Unsupported (2): camera modes 2 and 3.  Invalid (1): a null
 * pointer, another mode, a pix2cam whose last row is not (0, 0, -1) or that has no inverse, a focal, width or height that is not a
 * positive finite number (width and height whole). */
int mipnerf_fuse_projection(const float* camera, float* frame);
/* Rules T1 - T6 for num_frames frames in order.  frames [num_frames, 16] fp32 and offsets [num_frames] int64 are DEVICE arrays; depth is
 * one flat device buffer of depth_count floats holding every frame's [H_f, W_f] image at offsets[f]; sum and count [nz, ny, nx] fp32 are
 * read and written.  Invalid (1) before any device call: a null pointer, an axis < 2, hi <= lo, 7 nx ny nz >= 2^31, trunc <= 0 or not
 * finite, num_frames or depth_count negative.  num_frames = 0 returns without a launch. */
int mipnerf_fuse_integrate(const int32_t dims[3], const float lo[3], const float hi[3], float trunc, int32_t carve, int64_t num_frames,
                           const float* frames, const int64_t* offsets, const float* depth, int64_t depth_count, float* sum, float* count,
                           void* stream);
/* Rule F: lattice [nz, ny, nx] fp32 from the two planes; fill must be +1 or -1. */
int mipnerf_fuse_finalise(const int32_t dims[3], const float* sum, const float* count, float fill, float* lattice, void* stream);
/* The host build of rules T1 - T6 (the same functions of csrc/fuse_rules.hpp, HOST arrays, no device): what the CPU tests compare a
 * restatement with.  The same checks; the same split into launches, taken one after the other. */
int mipnerf_fuse_integrate_host(const int32_t dims[3], const float lo[3], const float hi[3], float trunc, int32_t carve, int64_t num_frames,
                                const float* frames, const int64_t* offsets, const float* depth, int64_t depth_count, float* sum,
                                float* count);

#ifdef __cplusplus
}
#endif
#endif
