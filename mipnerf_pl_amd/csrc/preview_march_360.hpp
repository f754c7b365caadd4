// The rules of mipnerf_preview_360_march (include/mipnerf_preview_360.h), stated ONCE.  MIP_HD like preview_march.hpp: the same source is
// inlined into k_preview_360 (kernels_preview_360.hip) and compiled with g++ by tests/hostmath/preview_360.cpp; both with
// -ffp-contract=off, so every product and sum below rounds once, as written.  Rows, the SH basis, the occupancy words, the cell index and
// the blend are preview_march.hpp's and lattice_sample.hpp's; this file adds what a CONTRACTED lattice needs: the lattice lives in
// z = contract(x), a straight world ray is a curve there, density is per unit of WORLD length, and the step follows the lattice's cells.
//
// C1. Step.  s = step_scale * min(hx, hy, hz) of the lattice: a length in the CONTRACTED space, formed on the host.
// C2. Ray constants (directions are not normalised; t is in units of d).  len = |d|, u = d / len, tc = -(o . u), m = o + tc u (the point
//     nearest the centre), p2 = m . m, p = sqrt(p2), c = sqrt(4 p2 + 1), ts = sqrt(max(c - p2, 0)), half = sqrt(R^2 - p2),
//     la = max(near len, tc - half), lb = min(far len, tc + half), R = far_radius.  A MISS: rule 2's finiteness, |d| and far <= near
//     tests of mipnerf_preview.h, or p2 >= R^2, or not la < lb.  No slab test: the interval is [near, far] cut by the ball of radius R.
// C3. Warp.  tau = the world arclength from m.  W is odd; a = |tau| <= ts: W = tau; beyond: g = (a - ts) / (p2 + a ts),
//     W = sign(tau) (ts + (c / p) atan(p g)), the last term c g when p < 2^-20.  Inverse V(w): a = |w| <= ts: V = w; beyond: D = a - ts,
//     q = tan(p D / c) / p (D / c when p < 2^-20), V = sign(w) (ts + q p2) / (1 - q ts); every value of V is clamped to
//     [la - tc, lb - tc], and a denominator <= 0 gives the clamp's end on that side.  wa = W(la - tc), wb = W(lb - tc).
//     W' = min(1, c / (p2 + tau^2)) bounds the speed of contract(x(tau)) from above, so two consecutive samples are never
//     more than s apart in the contracted space.  atanf / tanf, not the fast intrinsics: tan's argument approaches pi / 2 on long rays.
// C4. Samples.  w_i = wa + (float(i) + 0.5) s, while w_i < wb and i < max_steps; a hit ray shorter than half a step (w_0 >= wb) has the
//     one sample w_0 = (wa + wb) / 2, so no hit ray is left without a sample.  tau_i = V(w_i), t_i = (tc + tau_i) / len, x = o + t_i d,
//     z = contract(x): x when |x| <= 1, else x ((2 - 1 / |x|) / |x|).  World length delta_i = max(e_{i+1} - e_i, 0) with the edges
//     e_k = V(min(wa + float(k) s, wb)), except that the upper edge of the LAST sample by w (w_{i+1} >= wb) is V(wb) = lb - tc: it takes
//     the remainder of less than half a step that no sample of its own would cover, so the deltas partition [la, lb].
// C5. Evaluation.  z outside the box on any axis: nothing (no clamping to the nearest face).  Otherwise lattice_cell on z, the occupancy
//     bit, preview_row, preview_shade with alpha = 1 - exp(-(sigma * delta_i)) and Y from the WORLD direction u; dsum += w t_i.
// Rules 5 - 7 of mipnerf_preview.h hold unchanged.
#pragma once

#include "preview_march.hpp"

namespace mip {

constexpr float kPreview360TinyP = 9.5367431640625e-07f;      // 2^-20

struct PreviewRay360 {       // a ray after C2 - C3; every member is the same in all lanes of the ray's wavefront
    float len, tc, p2, p, c, ts;
    float tau_lo, tau_hi;    // la - tc, lb - tc: the clamp of V
    float wa, wb;
    float u[3];
};

// C3: W on one side, a = |tau| >= 0
MIP_HD float preview360_warp_abs(const PreviewRay360& r, float a) {
    if (a <= r.ts) return a;
    const float g = (a - r.ts) / (r.p2 + a * r.ts);
    return r.ts + (r.p < kPreview360TinyP ? r.c * g : (r.c / r.p) * atanf(r.p * g));
}

MIP_HD float preview360_warp(const PreviewRay360& r, float tau) {
    const float v = preview360_warp_abs(r, fabsf(tau));
    return tau < 0.0f ? -v : v;
}

// C3: V, clamped
MIP_HD float preview360_unwarp(const PreviewRay360& r, float w) {
    const float a = fabsf(w);
    float v = w;
    if (!(a <= r.ts)) {
        const float D = a - r.ts;
        const float q = r.p < kPreview360TinyP ? D / r.c : tanf((r.p * D) / r.c) / r.p;
        const float den = 1.0f - q * r.ts;
        if (!(den > 0.0f)) return w < 0.0f ? r.tau_lo : r.tau_hi;
        const float b = (r.ts + q * r.p2) / den;
        v = w < 0.0f ? -b : b;
    }
    return fminf(fmaxf(v, r.tau_lo), r.tau_hi);
}

// C2 - C3: false = a miss
MIP_HD bool preview360_ray(float R, const float o[3], const float d[3], float near, float far, PreviewRay360* r) {
    if (!(preview_finite(near) && preview_finite(far)) || !(far > near)) return false;
#pragma unroll
    for (int a = 0; a < 3; ++a)
        if (!(preview_finite(o[a]) && preview_finite(d[a]))) return false;
    const float len = sqrtf((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
    if (!(len > 0.0f) || !preview_finite(len)) return false;
#pragma unroll
    for (int a = 0; a < 3; ++a) r->u[a] = d[a] / len;
    const float tc = -((o[0] * r->u[0] + o[1] * r->u[1]) + o[2] * r->u[2]);
    const float m[3] = {o[0] + tc * r->u[0], o[1] + tc * r->u[1], o[2] + tc * r->u[2]};
    const float p2 = (m[0] * m[0] + m[1] * m[1]) + m[2] * m[2];
    const float R2 = R * R;
    if (!(p2 < R2)) return false;                      // p2 >= R^2, and a p2 that is not finite
    const float half = sqrtf(R2 - p2);
    const float la = fmaxf(near * len, tc - half), lb = fminf(far * len, tc + half);
    if (!(la < lb)) return false;
    r->len = len;
    r->tc = tc;
    r->p2 = p2;
    r->p = sqrtf(p2);
    r->c = sqrtf(4.0f * p2 + 1.0f);
    r->ts = sqrtf(fmaxf(r->c - p2, 0.0f));
    r->tau_lo = la - tc;
    r->tau_hi = lb - tc;
    r->wa = preview360_warp(*r, r->tau_lo);
    r->wb = preview360_warp(*r, r->tau_hi);
    return true;
}

// C4: the warped coordinate of sample i, whether it exists (max_steps aside), the ray parameter of an arclength
MIP_HD float preview360_sample_w(const PreviewRay360& r, float s, int i) {
    const float w = r.wa + ((float)i + 0.5f) * s;
    return i == 0 && !(w < r.wb) ? 0.5f * (r.wa + r.wb) : w;
}
MIP_HD bool preview360_exists(const PreviewRay360& r, int i, float w) { return i == 0 || w < r.wb; }
// the upper edge e_{i+1} of sample i, i >= -1 (i = -1: e_0 = V(wa), the lower edge of sample 0)
MIP_HD float preview360_upper_edge(const PreviewRay360& r, float s, int i) {
    const bool last = i >= 0 && !(preview360_sample_w(r, s, i + 1) < r.wb);
    return preview360_unwarp(r, last ? r.wb : fminf(r.wa + (float)(i + 1) * s, r.wb));
}
MIP_HD float preview360_t(const PreviewRay360& r, float tau) { return (r.tc + tau) / r.len; }

// C4: z = contract(x)
MIP_HD void preview360_contract(const float x[3], float z[3]) {
    const float n2 = (x[0] * x[0] + x[1] * x[1]) + x[2] * x[2];
    float k = 1.0f;
    if (n2 > 1.0f) {
        const float n = sqrtf(n2);
        k = (2.0f - 1.0f / n) / n;
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) z[a] = n2 > 1.0f ? x[a] * k : x[a];
}

// C5: whether z lies in the lattice's box (a NaN does not)
MIP_HD bool preview360_inside(const PreviewField& f, const float z[3]) {
    return z[0] >= f.box.lo[0] && z[0] <= f.hi[0] && z[1] >= f.box.lo[1] && z[1] <= f.hi[1] && z[2] >= f.box.lo[2] && z[2] <= f.hi[2];
}

}  // namespace mip
