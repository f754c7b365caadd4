// The rules of libmipnerf_preview_reg.so (include/mipnerf_preview_reg.h), stated ONCE: the gradient of a total-variation term and of a
// decay of the view-dependent coefficients on the fp32 master rows of a baked lattice.  MIP_HD like preview_tune.hpp: the same source is
// inlined into k_preview_reg_grad (kernels_preview_reg.hip) and compiled with g++ by tests/hostmath/preview_reg.cpp; both with
// -ffp-contract=off, so every product, sum, quotient and root below rounds once, as written.  Which thread computes which entries is the
// kernel's business, not this file's; the ORDER of every sum is this file's, and tests/preview_reg_fixture.py follows it.
//
// NOTATION.  v[p][e] is entry e of the master row of lattice point p = (x, y, z); e_x, e_y, e_z are the unit steps.  A point is PRESENT
// when it lies inside the lattice and its mask byte is not 0 (no mask: every point inside is present).  r_a = hmin / h_a is the per-axis
// scale (1 on a cubic lattice), w = w_sigma for e == 0 and w_colour for the other used entries.
//   rule R1  at a present anchor p:   d_a(p) = r_a (v[p + e_a][e] - v[p][e]) when p + e_a is present, else 0          (reg_diff)
//   rule R2                           n(p)   = sqrtf(((dx dx + dy dy) + dz dz) + eps)                                  (reg_norm)
//            the value of the term is sum_p w n(p) over the present p and the used e; nothing here forms it (the fixture does)
//   rule R3  for a present p:         t = -(((r_x dx(p) + r_y dy(p)) + r_z dz(p)) / n(p))                              the anchor p itself
//                                     t = t + (r_a d_a(p - e_a)) / n(p - e_a)   for a = x, y, z in this order, each only when p - e_a
//                                                                               is present (an absent anchor adds NO term, not a zero)
//   rule R4                           g = grad[p][e]
//                                     g = g + w t                   only when w != 0
//                                     g = g + w_view v[p][e]        only when e >= 4 and w_view != 0 (the coefficients of k >= 1)
//                                     grad[p][e] = g                only when one of the two lines ran
// Rule R3 reads 13 values of entry e: v[p], v[p + e_a], v[p - e_a] and v[p - e_a + e_b] for b != a; it is a GATHER: every grad[p][e] is
// written by whoever computes p, from master alone, so two runs give the same bytes.  A point that is not present is neither an anchor
// nor a neighbour: its master row is never read and its grad row never touched.  Pad entries (e >= reg_row_used) are never read for
// writing nor written.  A NON-FINITE master entry v[q][e] spoils exactly the grad entries [p][e] whose 13-value stencil holds q as a present
// point: p = q - e_a, q + e_a, q + e_a - e_b, and p = q itself when one of its six axis neighbours is present (else all its differences
// are the constant 0 and do not read v[q]) or the entry decays; a term whose weight is 0 is not formed, so it spoils nothing.
#pragma once

#include <math.h>
#include <stdint.h>

#include "preview_march.hpp"

namespace mip {

struct PreviewReg {          // by-value kernel argument
    int nx, ny, nz;
    float r[3];              // hmin / h_a, formed by the caller in fp32
    float w_sigma, w_colour, w_view, eps;
};

// the used entries of a row: sigma and 3 (degree + 1)^2 coefficients (tune_row_used of preview_tune.hpp, which this library does not include)
MIP_HD constexpr int reg_row_used(int degree) { return 1 + 3 * preview_basis(degree); }

// present: inside the lattice and not masked out
MIP_HD bool reg_present(const PreviewReg& p, const uint8_t* mask, int x, int y, int z) {
    if (x < 0 || y < 0 || z < 0 || x >= p.nx || y >= p.ny || z >= p.nz) return false;
    return mask == nullptr || mask[((int64_t)z * p.ny + y) * p.nx + x] != 0;
}

// which of the 12 neighbours of a present point are present; unit(a) is e_a
struct RegStencil {
    bool fwd[3];             // p + e_a
    bool back[3];            // p - e_a
    bool side[3][3];         // p - e_a + e_b, b != a (side[a][a] is p itself: unused)
};

MIP_HD void reg_stencil(const PreviewReg& p, const uint8_t* mask, int x, int y, int z, RegStencil* s) {
    for (int a = 0; a < 3; ++a) {
        const int ax = a == 0, ay = a == 1, az = a == 2;
        s->fwd[a] = reg_present(p, mask, x + ax, y + ay, z + az);
        s->back[a] = reg_present(p, mask, x - ax, y - ay, z - az);
        for (int b = 0; b < 3; ++b)
            s->side[a][b] = b != a && s->back[a] && reg_present(p, mask, x - ax + (b == 0), y - ay + (b == 1), z - az + (b == 2));
    }
}

// rule R1 for a present neighbour
MIP_HD float reg_diff(float r, float there, float here) { return r * (there - here); }

// rule R2
MIP_HD float reg_norm(float dx, float dy, float dz, float eps) { return sqrtf(((dx * dx + dy * dy) + dz * dz) + eps); }

// rule R3: c = v[p][e], fwd[a] = v[p + e_a][e], back[a] = v[p - e_a][e], side[a][b] = v[p - e_a + e_b][e]; a value whose point is not
// present is never looked at
MIP_HD float reg_tv(const PreviewReg& p, const RegStencil& s, float c, const float fwd[3], const float back[3], const float side[3][3]) {
    float d[3];
    for (int a = 0; a < 3; ++a) d[a] = s.fwd[a] ? reg_diff(p.r[a], fwd[a], c) : 0.0f;
    float t = -(((p.r[0] * d[0] + p.r[1] * d[1]) + p.r[2] * d[2]) / reg_norm(d[0], d[1], d[2], p.eps));
    for (int a = 0; a < 3; ++a) {
        if (!s.back[a]) continue;
        float q[3];
        for (int b = 0; b < 3; ++b) q[b] = b == a ? reg_diff(p.r[a], c, back[a]) : s.side[a][b] ? reg_diff(p.r[b], side[a][b], back[a]) : 0.0f;
        t = t + (p.r[a] * q[a]) / reg_norm(q[0], q[1], q[2], p.eps);
    }
    return t;
}

// does rule R4 touch entry e at all?
MIP_HD bool reg_touches(const PreviewReg& p, int e) { return (e == 0 ? p.w_sigma : p.w_colour) != 0.0f || (e >= 4 && p.w_view != 0.0f); }

// rule R4: the new grad[p][e] of a used entry that reg_touches
MIP_HD float reg_add(const PreviewReg& p, const RegStencil& s, int e, float g, float c, const float fwd[3], const float back[3],
                     const float side[3][3]) {
    const float w = e == 0 ? p.w_sigma : p.w_colour;
    if (w != 0.0f) g = g + w * reg_tv(p, s, c, fwd, back, side);
    if (e >= 4 && p.w_view != 0.0f) g = g + p.w_view * c;
    return g;
}

}  // namespace mip
