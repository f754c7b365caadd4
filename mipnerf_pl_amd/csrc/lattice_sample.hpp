// Trilinear value of an fp32 lattice [nz, ny, nx] at a point: the ONE statement of the arithmetic behind mipnerf_lattice_density /
// mipnerf_forward_proposal (include/mipnerf_hip.h).  MIP_HD like raymath.hpp: the same source is inlined into k_lattice_density and
// compiled with g++ by tests/hostmath/proposal.cpp; both with -ffp-contract=off, so every product and sum below rounds once, as written.
//
// The lattice has mipnerf_density_grid's layout: point (i, j, k) lies at lo + float(i) * h per axis and has the flat index
// (k * ny + j) * nx + i.  Per axis, with n >= 2 points and inv_h = float(n - 1) / (hi - lo) computed ONCE on the host (no division here):
//     u  = (x - lo) * inv_h, clamped to [0, n - 1]          a point outside the box takes the value of the nearest face
//     i0 = min(int(floorf(u)), n - 2),  f = u - float(i0)   a point on the hi face gives i0 = n - 2, f = 1
// and the 8 corners of cell (i0, j0, k0) are blended along x, then y, then z, each step as (1 - f) * a + f * b: non-negative corners
// give a non-negative value.  A non-finite coordinate gives 0 (nothing is loaded); a NaN among the 8 corners propagates.
#pragma once

#include "raymath.hpp"

namespace mip {

struct LatticeBox {          // by-value kernel argument: what the host derives from (dims, lo, hi)
    int nx, ny, nz;
    float lo[3];
    float inv_h[3];          // float(n - 1) / (hi - lo)
};

// The index rule alone (mipnerf_preview_march samples packed rows with it, preview_march.hpp): cell c and fractions f of a FINITE point p.
MIP_HD void lattice_cell(const LatticeBox& g, const float p[3], int c[3], float f[3]) {
    const int n[3] = {g.nx, g.ny, g.nz};
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        float u = (p[a] - g.lo[a]) * g.inv_h[a];
        u = fminf(fmaxf(u, 0.0f), (float)(n[a] - 1));
        const int i = (int)floorf(u);
        c[a] = i < n[a] - 2 ? i : n[a] - 2;
        f[a] = u - (float)c[a];
    }
}

MIP_HD float lattice_trilinear(const float* __restrict__ lattice, const LatticeBox& g, float x, float y, float z) {
    const float big = 3.4028234663852886e38f;
    if (!(fabsf(x) <= big && fabsf(y) <= big && fabsf(z) <= big)) return 0.0f;      // NaN fails the comparison too
    const float p[3] = {x, y, z};
    int c[3];
    float f[3];
    lattice_cell(g, p, c, f);
    const int64_t sy = g.nx, sz = (int64_t)g.nx * g.ny;
    const float* q = lattice + ((int64_t)c[2] * g.ny + c[1]) * g.nx + c[0];
    // the 8 corner loads first, then the blend
    const float v000 = q[0], v100 = q[1], v010 = q[sy], v110 = q[sy + 1];
    const float v001 = q[sz], v101 = q[sz + 1], v011 = q[sz + sy], v111 = q[sz + sy + 1];
    const float gx = 1.0f - f[0], gy = 1.0f - f[1], gz = 1.0f - f[2];
    const float v00 = gx * v000 + f[0] * v100;
    const float v10 = gx * v010 + f[0] * v110;
    const float v01 = gx * v001 + f[0] * v101;
    const float v11 = gx * v011 + f[0] * v111;
    const float v0 = gy * v00 + f[1] * v10;
    const float v1 = gy * v01 + f[1] * v11;
    return gz * v0 + f[2] * v1;
}

}  // namespace mip
