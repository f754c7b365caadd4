// Per-sample math of the unbounded-scene (mip-NeRF 360) ray path: full-covariance conical-frustum Gaussian,
// scene contraction applied to a Gaussian, off-axis integrated positional encoding.  Host + device (MIP_HD) like
// raymath.hpp, so tests/hostmath can check it against oracle/mipnerf360_oracle.py without a GPU.
//
// The reference's functions for this path are dead and wrong (models/mip.py:38-47 uses t_var for the perpendicular
// term, :445 replaces the covariance by the Jacobian, :316-319 has no frequency scales, and nothing calls them), so this
// follows the paper they aim at -- Barron et al., "Mip-NeRF 360", CVPR 2022 -- equation numbers cited per function.
#pragma once

#include "raymath.hpp"

namespace mip {

struct GaussFull {
    float mean[3];
    float cov[6];     // symmetric 3x3: xx, xy, xz, yy, yz, zz
};

constexpr int kBasis360N = 21;
// the 21 non-antipodal vertices of a twice-tessellated icosahedron (same table as models/mip.py:293-313)
#if defined(__HIPCC__)
__device__ __constant__
#endif
static const float kBasis360[kBasis360N][3] = {
    {0.8506508f, 0.f, 0.5257311f}, {0.809017f, 0.5f, 0.309017f}, {0.5257311f, 0.8506508f, 0.f}, {1.f, 0.f, 0.f},
    {0.809017f, 0.5f, -0.309017f}, {0.8506508f, 0.f, -0.5257311f}, {0.309017f, 0.809017f, -0.5f},
    {0.f, 0.5257311f, -0.8506508f}, {0.5f, 0.309017f, -0.809017f}, {0.f, 1.f, 0.f}, {-0.5257311f, 0.8506508f, 0.f},
    {-0.309017f, 0.809017f, -0.5f}, {0.f, 0.5257311f, 0.8506508f}, {-0.309017f, 0.809017f, 0.5f},
    {0.309017f, 0.809017f, 0.5f}, {0.5f, 0.309017f, 0.809017f}, {0.5f, -0.309017f, 0.809017f}, {0.f, 0.f, 1.f},
    {-0.5f, 0.309017f, 0.809017f}, {-0.809017f, 0.5f, 0.309017f}, {-0.809017f, 0.5f, -0.309017f}};

// Jacobian of contract() at x, |x| > 1 (symmetric): J = a (I - u u^T) + b u u^T, u = x/|x|, a = (2|x| - 1)/|x|^2, b = 1/|x|^2
struct ContractJ {
    float u[3], a, b, mean_scale;
};
MIP_HD ContractJ contract_jacobian(const float m[3], float n2) {
    ContractJ c;
    const float n = sqrtf(n2);
    c.u[0] = m[0] / n; c.u[1] = m[1] / n; c.u[2] = m[2] / n;
    c.a = (2.0f * n - 1.0f) / n2;
    c.b = 1.0f / n2;
    c.mean_scale = (2.0f - 1.0f / n) / n;
    return c;
}

// mip-NeRF eq. (7) (stable form, as raymath.hpp) + eq. (8) with the FULL covariance
//   mean = d t_mean + o,   cov = t_var d d^T + r_var (I - d d^T / |d|^2),
// and, when `contracted`, the paper's eq. (9)/(10): mean' = contract(mean), cov' = J cov J^T.  The structure of cov is
// used instead of a generic 3x3 triple product: with v = J d,
//   cov' = t_var v v^T + r_var (J J^T - v v^T / |d|^2),   J J^T = a^2 (I - u u^T) + b^2 u u^T,
// every term a well-scaled outer product (a generic J C J^T in fp32 loses ~1e-4 of the largest entry at |x| ~ 1e3,
// where J's radial and tangential scales differ by |x| and C's by (t_var / r_var)).
MIP_HD GaussFull conical_frustum_to_gaussian_full(float t0, float t1, const float d[3], const float o[3], float radius,
                                                  bool contracted = false) {
    const float mu = (t0 + t1) / 2.0f;
    const float hw = (t1 - t0) / 2.0f;
    const float mu2 = mu * mu, hw2 = hw * hw, hw4 = hw2 * hw2;
    const float den = 3.0f * mu2 + hw2;
    const float t_mean = mu + (2.0f * mu * hw2) / den;
    const float t_var = hw2 / 3.0f - (float)(4.0 / 15.0) * ((hw4 * (12.0f * mu2 - hw2)) / (den * den));
    const float r_var = (radius * radius) * (mu2 / 4.0f + (float)(5.0 / 12.0) * hw2 - (float)(4.0 / 15.0) * hw4 / den);
    const float dn = (d[0] * d[0] + d[1] * d[1] + d[2] * d[2]) + 1e-10f;
    GaussFull g;
#pragma unroll
    for (int a = 0; a < 3; ++a) g.mean[a] = d[a] * t_mean + o[a];
    const float n2 = (g.mean[0] * g.mean[0] + g.mean[1] * g.mean[1]) + g.mean[2] * g.mean[2];
    if (contracted && n2 > 1.0f) {
        const ContractJ c = contract_jacobian(g.mean, n2);
        const float ud = (c.u[0] * d[0] + c.u[1] * d[1]) + c.u[2] * d[2];
        float v[3];                                   // v = J d = a d + (b - a) (u . d) u
#pragma unroll
        for (int a = 0; a < 3; ++a) v[a] = c.a * d[a] + ((c.b - c.a) * ud) * c.u[a];
        const float a2 = c.a * c.a, b2a2 = c.b * c.b - a2;
        int k = 0;
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = i; j < 3; ++j) {
                const float vv = v[i] * v[j];
                const float jj = (i == j ? a2 : 0.0f) + b2a2 * (c.u[i] * c.u[j]);       // (J J^T)_ij
                g.cov[k++] = t_var * vv + r_var * (jj - vv / dn);
            }
#pragma unroll
        for (int a = 0; a < 3; ++a) g.mean[a] *= c.mean_scale;
        return g;
    }
    int k = 0;
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = a; b < 3; ++b) {
            const float dd = d[a] * d[b];
            const float null_outer = (a == b ? 1.0f : 0.0f) - dd / dn;
            g.cov[k++] = t_var * dd + r_var * null_outer;
        }
    return g;
}

// contract() of an ARBITRARY Gaussian (paper eq. (9)/(10)): mean' = contract(mean), cov' = J cov J^T (generic triple
// product; conditioned like |x| -- prefer the fused form above when the Gaussian comes from a conical frustum).
MIP_HD void contract_gaussian(GaussFull& g) {
    const float n2 = (g.mean[0] * g.mean[0] + g.mean[1] * g.mean[1]) + g.mean[2] * g.mean[2];
    if (!(n2 > 1.0f)) return;
    const ContractJ c = contract_jacobian(g.mean, n2);
    float J[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const float uu = c.u[i] * c.u[j];
            J[i][j] = c.a * ((i == j ? 1.0f : 0.0f) - uu) + c.b * uu;
        }
    const float C[3][3] = {{g.cov[0], g.cov[1], g.cov[2]}, {g.cov[1], g.cov[3], g.cov[4]}, {g.cov[2], g.cov[4], g.cov[5]}};
    float T[3][3];      // J C
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) T[i][j] = (J[i][0] * C[0][j] + J[i][1] * C[1][j]) + J[i][2] * C[2][j];
    int k = 0;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = i; j < 3; ++j) g.cov[k++] = (T[i][0] * J[j][0] + T[i][1] * J[j][1]) + T[i][2] * J[j][2];   // (J C J^T)_ij
#pragma unroll
    for (int a = 0; a < 3; ++a) g.mean[a] *= c.mean_scale;
}

// The way back from the contracted space (include/mipnerf_hip.h, "lattice of the unbounded-scene model"): z -> x with contract(x) = z.
// c = 2 - 1 / far_radius caps |z|.  With n = |z| > 1: r = |x| = min(1 / (2 - min(n, c)), far_radius) -- the difference is exact in fp32 for
// n in [1, 2]; the second minimum holds the promise "nothing beyond far_radius" where c has been rounded up (far_radius no power of two) or
// to 2 (far_radius >= 2^24) -- and x = z * (r / n); n <= 1: x = z.
MIP_HD float uncontract_radius(float n, float far_radius) {
    const float c = 2.0f - 1.0f / far_radius;
    const float r = 1.0f / (2.0f - (n < c ? n : c));
    return r < far_radius ? r : far_radius;
}
MIP_HD void uncontract_point(const float z[3], float far_radius, float x[3]) {
    const float n = sqrtf((z[0] * z[0] + z[1] * z[1]) + z[2] * z[2]);
    const float s = n > 1.0f ? uncontract_radius(n, far_radius) / n : 1.0f;
    x[0] = n > 1.0f ? z[0] * s : z[0]; x[1] = n > 1.0f ? z[1] * s : z[1]; x[2] = n > 1.0f ? z[2] * s : z[2];
}

// A normal g of the contracted space is a density-gradient direction; the world gradient is J^T g with the symmetric J of
// contract_jacobian at x = uncontract_point(z): J = (1 / r^2) ((2 r - 1) (I - u u^T) + u u^T), u = z / |z|.  The common factor drops out of
// the direction: normalize((2 r - 1) (g - (u . g) u) + (u . g) u), every term of the size of g.  |z| <= 1: g as it stands.
// (0, 0, 0), and a result that is not finite, give (0, 0, 0).
MIP_HD void uncontract_normal(const float z[3], float far_radius, const float g[3], float out[3]) {
    const float n = sqrtf((z[0] * z[0] + z[1] * z[1]) + z[2] * z[2]);
    float w[3] = {g[0], g[1], g[2]};
    if (n > 1.0f) {
        const float r = uncontract_radius(n, far_radius);
        const float u[3] = {z[0] / n, z[1] / n, z[2] / n};
        const float ug = (u[0] * g[0] + u[1] * g[1]) + u[2] * g[2];
        const float a = 2.0f * r - 1.0f;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float radial = ug * u[k];
            w[k] = a * (g[k] - radial) + radial;
        }
        const float len = sqrtf((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]);
#pragma unroll
        for (int k = 0; k < 3; ++k) w[k] /= len;
    }
    const float chk = (w[0] + w[1]) + w[2];
    const bool ok = chk - chk == 0.0f;          // false for inf and NaN (0 / 0 when g = 0 outside the unit ball)
    out[0] = ok ? w[0] : 0.0f; out[1] = ok ? w[1] : 0.0f; out[2] = ok ? w[2] : 0.0f;
}

// projection on basis direction j: y = p . mean, var = p^T cov p
MIP_HD void project_360(const GaussFull& g, int j, float& y, float& var) {
    const float px = kBasis360[j][0], py = kBasis360[j][1], pz = kBasis360[j][2];
    y = (g.mean[0] * px + g.mean[1] * py) + g.mean[2] * pz;
    const float cx = (g.cov[0] * px + g.cov[1] * py) + g.cov[2] * pz;
    const float cy = (g.cov[1] * px + g.cov[3] * py) + g.cov[4] * pz;
    const float cz = (g.cov[2] * px + g.cov[4] * py) + g.cov[5] * pz;
    var = (cx * px + cy * py) + cz * pz;
}

// off-axis IPE feature (half, l, basis j): exp(-0.5 * 4^l var) * sin(2^l y [+ pi/2]); index = half*21L + l*21 + j
MIP_HD float ipe360_feature(float y, float var, int half, int l, int min_deg) {
    const float scale = (float)(1u << (l + min_deg));
    const float ys = y * scale;
    const float vs = var * (scale * scale);
    return exp_accurate(-0.5f * vs) * sin_accurate(half ? (ys + kHalfPiF) : ys);
}

// ---- the ray side of empty-space skipping in the contracted space (include/mipnerf_hip.h, mipnerf_ray_occupancy_360) ----
// Inverse-depth fence post k of the coarse level, k in [0, n_samples]: ni = 1 / near, fi = 1 / far.  The ONE statement of the expression:
// k_sample_along_rays_360 and the 360 classifiers call it, so their fence posts are the same bits.
MIP_HD float level0_t_inv_360(float ni, float fi, int n_samples, int k) {
    const float s = torch_linspace_at(0.0f, 1.0f, n_samples + 1, k);
    return fi * s + (1.0f - s) * ni;
}
MIP_HD float level0_t_360(float nearv, float farv, int n_samples, int k) {
    return 1.0f / level0_t_inv_360(1.0f / nearv, 1.0f / farv, n_samples, k);
}

// Per-axis interval [lo_a, hi_a] of the contracted space that holds contract(x) for every x = o + t d + delta with t in [t0, t1], delta
// perpendicular to d and |delta| <= rr t (rr = cone_scale * radius); rho = rr t1 bounds |delta|.  contract keeps directions --
// contract(x) = f(|x|) x / |x| with f(r) = r inside the unit ball and 2 - 1 / r outside -- so radius and direction are bounded apart:
//   tc = clamp(-(o.d) / (d.d), t0, t1), rc = |o + tc d|: the axis point nearest the centre; rmin = rc - rho, rmax = max(|p0|, |p1|) + rho
//   rmin >= 1 (the frustum lies wholly outside the unit ball): with u0 = p0 / |p0|, u1 = p1 / |p1| every axis direction lies within the
//     sagitta sag = 1 - sqrt(max(0, (1 + u0.u1) / 2)) of the chord u0 u1, and |x / |x| - p / |p|| <= |x - p| / sqrt(|x| |p|) <= rho / rmin
//     for the off-axis part: e = sag + rho / rmin, [ulo_a, uhi_a] = [max(min(u0_a, u1_a) - e, -1), min(max(u0_a, u1_a) + e, 1)], and with
//     flo = 2 - 1 / rmin, fhi = 2 - 1 / rmax: lo_a = ulo_a < 0 ? ulo_a fhi : ulo_a flo, hi_a = uhi_a > 0 ? uhi_a fhi : uhi_a flo;
//   otherwise the world interval of the bounded rule, [xlo_a, xhi_a] = [min(p0_a, p1_a) - rho, max(p0_a, p1_a) + rho], shrunk towards 0 by
//     the smallest scale contract applies in it, slo = rmax > 1 ? (2 - 1 / rmax) / rmax : 1: lo_a = xlo_a < 0 ? xlo_a : xlo_a slo,
//     hi_a = xhi_a > 0 ? xhi_a : xhi_a slo, both clamped to [-F, F], F = rmax > 1 ? 2 - 1 / rmax : rmax.
// A value that is not finite anywhere gives NaN bounds on every axis: the caller's cell rule then calls the frustum "outside".
MIP_HD void contracted_frustum_box(float t0, float t1, const float o[3], const float d[3], float rr, float lo[3], float hi[3]) {
    const float rho = rr * t1;
    float p0[3], p1[3], pc[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) { p0[a] = o[a] + t0 * d[a]; p1[a] = o[a] + t1 * d[a]; }
    const float od = (o[0] * d[0] + o[1] * d[1]) + o[2] * d[2];
    const float dd = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2];
    const float tc = fminf(fmaxf(-od / dd, t0), t1);
#pragma unroll
    for (int a = 0; a < 3; ++a) pc[a] = o[a] + tc * d[a];
    const float rc = sqrtf((pc[0] * pc[0] + pc[1] * pc[1]) + pc[2] * pc[2]);
    const float n0 = sqrtf((p0[0] * p0[0] + p0[1] * p0[1]) + p0[2] * p0[2]);
    const float n1 = sqrtf((p1[0] * p1[0] + p1[1] * p1[1]) + p1[2] * p1[2]);
    const float rmin = rc - rho;
    const float rmax = fmaxf(n0, n1) + rho;
    const float chk = (n0 + n1) + (rc + rho);
    if (!(chk - chk == 0.0f)) {                  // inf or NaN (fminf / fmaxf would drop a NaN operand)
#pragma unroll
        for (int a = 0; a < 3; ++a) lo[a] = hi[a] = chk - chk;
        return;
    }
    if (rmin >= 1.0f) {
        float u0[3], u1[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) { u0[a] = p0[a] / n0; u1[a] = p1[a] / n1; }
        const float c = (u0[0] * u1[0] + u0[1] * u1[1]) + u0[2] * u1[2];
        const float sag = 1.0f - sqrtf(fmaxf(0.0f, (1.0f + c) / 2.0f));
        const float e = sag + rho / rmin;
        const float flo = 2.0f - 1.0f / rmin, fhi = 2.0f - 1.0f / rmax;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float ulo = fmaxf(fminf(u0[a], u1[a]) - e, -1.0f), uhi = fminf(fmaxf(u0[a], u1[a]) + e, 1.0f);
            lo[a] = ulo < 0.0f ? ulo * fhi : ulo * flo;
            hi[a] = uhi > 0.0f ? uhi * fhi : uhi * flo;
        }
        return;
    }
    const float slo = rmax > 1.0f ? (2.0f - 1.0f / rmax) / rmax : 1.0f;
    const float F = rmax > 1.0f ? 2.0f - 1.0f / rmax : rmax;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float xlo = fminf(p0[a], p1[a]) - rho, xhi = fmaxf(p0[a], p1[a]) + rho;
        const float l = xlo < 0.0f ? xlo : xlo * slo, h = xhi > 0.0f ? xhi : xhi * slo;
        lo[a] = fminf(fmaxf(l, -F), F);
        hi[a] = fminf(fmaxf(h, -F), F);
    }
}

}  // namespace mip
