// The rules of libmipnerf_preview_tune_360.so (include/mipnerf_preview_tune_360.h), stated ONCE: the gradient of mipnerf_preview_360_march
// with respect to the rows.  MIP_HD like preview_tune.hpp: the same source is inlined into k_preview_360_tune_grad
// (kernels_preview_tune_360.hip) and compiled with g++ by tests/hostmath/preview_tune_360.cpp; both with -ffp-contract=off, so every
// product and sum below rounds once, as written.  The ray, the warp, the samples, their world lengths and the contraction are
// preview_march_360.hpp's (C1 - C5), rules 8 and 10 are preview_tune.hpp's, ALL BY CALL; this file restates only what differs.
//
//   C6  = rule 8:  q_i = sum_c G_c (colour_{i,c} - background_c) + g_a                                              (tune_q)
//   C7  = rule 9 with the sample's own world length:
//            d row[0]          = delta_i (T_{i+1} q_i - S_i)  where row[0] > 0, else 0;  S_i = sum_{j > i} w_j q_j  (no division)
//            d row[1 + 3k + c] = w_i G_c Y_k                  where 0 < colour_{i,c} < 1, else 0;  Y from the WORLD direction u (C5)
//            d row[pad]        = 0
//         delta_i is C4's max(e_{i+1} - e_i, 0): the same number the forward used for alpha_i.
//   C8  = rule 10 on lattice_cell(box, z), z = contract(x) of C4.
// Sample positions, delta_i, the warp and the contraction depend on the ray only: no gradient flows through them.  Samples outside the
// box, samples in clear cells, samples behind the early stop, rays that miss (C2) and rays whose rgb, acc, G or g_a is not finite add
// nothing.  `distance` is not differentiated.
#pragma once

#include "preview_march_360.hpp"
#include "preview_tune.hpp"

namespace mip {

// C4 / C5 / C8: the contracted point of the sample at ray parameter t and, when it lies in the box, its cell and fractions
MIP_HD bool tune360_cell(const PreviewField& f, const float o[3], const float d[3], float t, int c[3], float fr[3]) {
    const float x[3] = {o[0] + t * d[0], o[1] + t * d[1], o[2] + t * d[2]};
    float z[3];
    preview360_contract(x, z);
    if (!preview360_inside(f, z)) return false;
    lattice_cell(f.box, z, c, fr);
    return true;
}

// C4: the world length of sample i from its two edges, as the march forms it
MIP_HD float tune360_delta(float e_lo, float e_hi) { return fmaxf(e_hi - e_lo, 0.0f); }

// C7, the density entry: rule 9's with delta_i in the place of the step; t_next = T_{i+1}, rest = S_i
MIP_HD float tune360_d_sigma(float delta, float t_next, float q, float rest, float row0) { return tune_d_sigma(delta, t_next, q, rest, row0); }

}  // namespace mip
