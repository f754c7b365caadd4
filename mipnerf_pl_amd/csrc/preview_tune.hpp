// The rules of libmipnerf_preview_tune.so (include/mipnerf_preview_tune.h), stated ONCE: rules 8 - 10 (the gradient of mipnerf_preview_march
// with respect to the rows) and the Adam step on the rows.  MIP_HD like preview_march.hpp: the same source is inlined into
// k_preview_tune_grad / k_preview_tune_adam (kernels_preview_tune.hip) and compiled with g++ by tests/hostmath/preview_tune.cpp; both with
// -ffp-contract=off, so every product and sum below rounds once, as written.  The samples, their cells, the blended row, alpha and the
// clamped colour are preview_march.hpp's (rules 1 - 5, by call); nothing here restates them.  How a ray's samples and a cell's corner rows are
// spread over lanes, and in which order the sums over samples are taken, is the kernel's business, not this file's.
//
// NOTATION.  Along one ray the evaluated samples i = 0, 1, ... have alpha_i, the clamped colour colour_i, the transmittance T_i before the
// sample (T_0 = 1, T_{i+1} = T_i (1 - alpha_i)) and the weight w_i = T_i alpha_i.  G is the gradient of the loss with respect to the ray's
// rgb, g_a the one with respect to its acc.
//   rule 8   q_i = sum_c G_c (colour_{i,c} - background_c) + g_a                                   what the loss gains per unit of w_i
//   rule 9   d row[0]          = s (T_{i+1} q_i - S_i)  where row[0] > 0, else 0;   S_i = sum_{j > i} w_j q_j  (no division)
//            d row[1 + 3k + c] = w_i G_c Y_k            where 0 < colour_{i,c} < 1 (the clamp of rule 4 is inactive), else 0
//            d row[pad]        = 0
//   rule 10  corner (a, b, c) of the sample's cell receives (wx_a wy_b) wz_c * d row, the weights (1 - f, f) per axis from lattice_cell
// Samples in clear cells, samples behind the early stop, rays that miss and rays whose rgb, acc, G or g_a is not finite add nothing.
#pragma once

#include "preview_march.hpp"

namespace mip {

// the used entries of a row of degree `degree`: sigma and 3 (degree + 1)^2 coefficients; the rest of its W halves is padding
MIP_HD constexpr int tune_row_used(int degree) { return 1 + 3 * preview_basis(degree); }

// the loss side of a ray: G from grad_rgb, or from the ray's own rgb in target mode
MIP_HD float tune_target_grad(float loss_scale, float rgb, float target) { return loss_scale * (rgb - target); }

// a ray adds something only when all of these are finite
MIP_HD bool tune_ray_ok(const float rgb[3], float acc, const float G[3], float g_a) {
    return preview_finite(rgb[0]) && preview_finite(rgb[1]) && preview_finite(rgb[2]) && preview_finite(acc) && preview_finite(G[0]) &&
           preview_finite(G[1]) && preview_finite(G[2]) && preview_finite(g_a);
}

// rule 8
MIP_HD float tune_q(const float G[3], float g_a, const float colour[3], const float background[3]) {
    return ((G[0] * (colour[0] - background[0]) + G[1] * (colour[1] - background[1])) + G[2] * (colour[2] - background[2])) + g_a;
}

// sum over ALL samples of w_i q_i from the ray's own sums (sc = sum w colour, sa = sum w): S_i = total - sum_{j <= i} w_j q_j
MIP_HD float tune_total(const float G[3], float g_a, const float sc[3], float sa, const float background[3]) {
    return ((G[0] * (sc[0] - sa * background[0]) + G[1] * (sc[1] - sa * background[1])) + G[2] * (sc[2] - sa * background[2])) + g_a * sa;
}

// rule 9, the density entry; t_next = T_{i+1}, rest = S_i, row0 = the blended row's density entry before its clamp
MIP_HD float tune_d_sigma(float s, float t_next, float q, float rest, float row0) { return row0 > 0.0f ? s * (t_next * q - rest) : 0.0f; }

// rule 9, a colour entry before its basis factor: d row[1 + 3k + c] = tune_d_colour(w, G_c, colour_c) * Y_k
MIP_HD float tune_d_colour(float w, float G, float colour) { return colour > 0.0f && colour < 1.0f ? w * G : 0.0f; }

// rule 10: the weight of corner (a, b, c), each 0 (low) or 1 (high), from lattice_cell's fractions
MIP_HD float tune_corner_weight(const float fr[3], int a, int b, int c) {
    return ((a ? fr[0] : 1.0f - fr[0]) * (b ? fr[1] : 1.0f - fr[1])) * (c ? fr[2] : 1.0f - fr[2]);
}

// ---- the optimiser step (mipnerf_preview_tune_adam) --------------------------------------------------------------------------------
struct TuneAdam {            // by-value kernel argument; c1 = 1 / (1 - beta1^t), c2 = 1 / (1 - beta2^t) are formed by the caller
    float lr_sigma, lr_colour, beta1, beta2, eps, c1, c2;
};

// entry e of a used (e < tune_row_used) element of an unmasked point: m, v, the master value p, its fp16 bits, and the gradient cleared
MIP_HD void tune_adam_element(const TuneAdam& a, int e, float* p, float* m, float* v, float* g, uint16_t* half) {
    const float gr = *g;
    const float mn = a.beta1 * *m + (1.0f - a.beta1) * gr;
    const float vn = a.beta2 * *v + (1.0f - a.beta2) * (gr * gr);
    const float lr = e == 0 ? a.lr_sigma : a.lr_colour;
    const float pn = *p - lr * ((mn * a.c1) / (sqrtf(vn * a.c2) + a.eps));
    *m = mn;
    *v = vn;
    *p = pn;
    *half = preview_half_bits(pn, e == 0);
    *g = 0.0f;
}

}  // namespace mip
