// The rules of fusing rendered depth into a truncated signed distance volume (include/mipnerf_fuse.h states them: D the depth quantile
// of one ray, P the projection row of a camera record, T the integration of a frame into a lattice point, F the finalising pass), each
// written down ONCE.  MIP_HD like lattice_sample_360.hpp: the kernels of kernels_fuse.hip and a host compiler (fuse_capi.hip's
// mipnerf_fuse_integrate_host, tests/hostmath/fuse.cpp) call the same functions.  Plain C++ without HIP headers.  Compile with
// -ffp-contract=off: every operation rounds once, in the order written here.
#pragma once

#include <math.h>
#include <stdint.h>

#include "raymath.hpp"      // MIP_HD

namespace mip {

constexpr int kFuseFrameFloats = 16;      // P[3][4] | W, H, near, far
constexpr int kFuseMaxQuantiles = 4;
// frames per launch of k_fuse_integrate.  The frame records are read from memory by the loop counter, so neither the registers nor the
// kernel arguments grow with the frames of a launch; measured on a 256^3 lattice with 800 x 800 maps, the time per frame falls up to 8
// frames per launch and rises beyond, where the launch's depth maps no longer stay in the L2 caches
constexpr int kFuseFramesPerLaunch = 8;

// the lattice as the kernels take it: h = (hi - lo) / float(n - 1) per axis, formed on the host
struct FuseLattice {
    int nx, ny, nz;
    float lo[3], h[3];
};

// ---- D: the depth quantile of one ray ------------------------------------------------------------------------------------------------
// D1: the weight that counts (NaN and negative weights are 0)
MIP_HD float quantile_weight(float w) { return fmaxf(w, 0.0f); }

// D2's test on the ONE array of inclusive prefixes: does interval i, with P_prev = P_{i-1} and P_here = P_i, hold opacity q?
MIP_HD bool quantile_crosses(double P_prev, double q, double P_here) { return P_prev < q && q <= P_here; }

// D3: the depth inside the interval that holds q, rounded once
MIP_HD float quantile_depth(double P_prev, double q, float w, float t0, float t1) {
    double f = (q - P_prev) / (double)w;
    f = f < 0.0 ? 0.0 : (f > 1.0 ? 1.0 : f);
    return (float)((double)t0 + f * ((double)t1 - (double)t0));
}

// D on the host: the prefixes are summed in sample order; +inf when no interval qualifies (D4)
inline float depth_quantile_ray(int N, const float* w, const float* t, double q) {
    double P_prev = 0.0;
    for (int i = 0; i < N; ++i) {
        const float wi = quantile_weight(w[i]);
        const double P_here = P_prev + (double)wi;
        if (quantile_crosses(P_prev, q, P_here)) return quantile_depth(P_prev, q, wi, t[i], t[i + 1]);
        P_prev = P_here;
    }
    return INFINITY;
}

// ---- P: the projection row of a camera record (host, double, rounded to fp32 once) ----------------------------------------------------
// camera: the 32 floats of mipnerf_generate_rays (c2w[3][4] | pix2cam[3][3] | W, H, near, far, lossmult, mode, focal | distortion[4]);
// frame: P[3][4] | W, H, near, far.  0: done; 1: a mode other than 0 and 1; 2: a pix2cam whose last row is not (0, 0, -1) or that
// has no inverse; 3: a focal, a width or a height that is not positive and finite
inline int fuse_projection_row(const float* cam, float* frame) {
    const double W = cam[21], H = cam[22];
    if (!(W >= 1.0) || !(H >= 1.0) || !isfinite(W) || !isfinite(H) || W != floor(W) || H != floor(H)) return 3;
    double m[3][3];      // pix2cam, acting on (x + .5, y + .5, 1)
    if (cam[26] == 0.0f) {
        const double f = cam[27];
        if (!(f > 0.0) || !isfinite(f)) return 3;
        m[0][0] = 1.0 / f; m[0][1] = 0.0; m[0][2] = -0.5 * W / f;
        m[1][0] = 0.0; m[1][1] = -1.0 / f; m[1][2] = 0.5 * H / f;
        m[2][0] = 0.0; m[2][1] = 0.0; m[2][2] = -1.0;
    } else if (cam[26] == 1.0f) {
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c) m[r][c] = cam[12 + 3 * r + c];
        if (m[2][0] != 0.0 || m[2][1] != 0.0 || m[2][2] != -1.0) return 2;
    } else {
        return 1;
    }
    // cam2pix = pix2cam^-1 with the last row (0, 0, -1): the upper-left 2 x 2 block inverted, the last row kept
    const double det = m[0][0] * m[1][1] - m[0][1] * m[1][0];
    if (!(det != 0.0) || !isfinite(det)) return 2;
    double k[3][3];
    k[0][0] = m[1][1] / det; k[0][1] = -m[0][1] / det;
    k[1][0] = -m[1][0] / det; k[1][1] = m[0][0] / det;
    k[0][2] = k[0][0] * m[0][2] + k[0][1] * m[1][2];      // cam2pix (c0, c1, -t) = t (px, py, 1): the third column carries + A^-1 b
    k[1][2] = k[1][0] * m[0][2] + k[1][1] * m[1][2];
    k[2][0] = 0.0; k[2][1] = 0.0; k[2][2] = -1.0;
    // [R^T | -R^T o]
    double e[3][4];
    for (int r = 0; r < 3; ++r) {
        e[r][3] = 0.0;
        for (int c = 0; c < 3; ++c) {
            e[r][c] = cam[4 * c + r];
            e[r][3] -= (double)cam[4 * c + r] * (double)cam[4 * c + 3];
        }
    }
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 4; ++c) frame[4 * r + c] = (float)(k[r][0] * e[0][c] + k[r][1] * e[1][c] + k[r][2] * e[2][c]);
    frame[12] = cam[21]; frame[13] = cam[22]; frame[14] = cam[23]; frame[15] = cam[24];
    return 0;
}

// ---- T: frame f into the lattice point p ----------------------------------------------------------------------------------------------
// T1: one coordinate of lattice point i
MIP_HD float fuse_point(float lo, int i, float h) { return lo + (float)i * h; }

// T2: one row of P applied to (x, y, z, 1)
MIP_HD float fuse_row(const float* __restrict__ r, float x, float y, float z) { return (r[0] * x + r[1] * y) + (r[2] * z + r[3]); }

// T2 - T5: true and *d set when the frame updates the point.  frame: the 16 floats of rule P; depth: the flat buffer all frames index,
// this frame's image at `offset`; nothing outside [0, depth_count) is read
MIP_HD bool fuse_frame_update(const float* __restrict__ frame, int64_t offset, const float* __restrict__ depth, int64_t depth_count,
                              float trunc, int carve, float x, float y, float z, float* d) {
    const float a = fuse_row(frame, x, y, z), b = fuse_row(frame + 4, x, y, z), t = fuse_row(frame + 8, x, y, z);
    const float W = frame[12], H = frame[13];
    if (!(frame[14] < t && t <= frame[15])) return false;
    const float u = floorf(a / t), v = floorf(b / t);
    if (!(0.0f <= u && u < W && 0.0f <= v && v < H)) return false;
    const int64_t at = offset + (int64_t)v * (int64_t)W + (int64_t)u;
    if (at < 0 || at >= depth_count) return false;
    const float D = depth[at];                                  // T3: the nearest pixel
    if (!(D > 0.0f)) return false;
    if (D == INFINITY) {                                        // T4: the ray is free over [near, far]
        if (!carve) return false;
        *d = 1.0f;
        return true;
    }
    const float s = D - t;                                      // T5
    if (s < -trunc) return false;
    *d = fminf(1.0f, s / trunc);
    return true;
}

// ---- F: the lattice value of a point ---------------------------------------------------------------------------------------------------
MIP_HD float fuse_finalise_value(float sum, float count, float fill) { return count > 0.0f ? -(sum / count) : fill; }

}  // namespace mip
