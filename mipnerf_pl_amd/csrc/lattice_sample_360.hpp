// The density of a pyramid of contracted lattices at one sample of a ray of the unbounded-scene model: the ONE statement of the arithmetic
// behind mipnerf_lattice_density_360 (include/mipnerf_proposal_360.h).  MIP_HD like lattice_sample.hpp: the same source is inlined into
// k_lattice_density_360 and compiled with g++ by tests/hostmath/proposal360.cpp; both with -ffp-contract=off.  The Gaussian is
// raymath360.hpp's, the trilinear value lattice_sample.hpp's and the level rule preview_mip.hpp's, each by call; nothing here restates them.
//
// A pyramid has L levels, 1 <= L <= 4, all over ONE box lo .. hi of the contracted space; level l is an fp32 lattice in
// mipnerf_density_grid's layout with spacing[l] = max over the axes of (hi - lo) / float(n_l - 1), formed on the host, strictly increasing.
// For the sample [t0, t1] of a ray:
//   Q1  G = conical_frustum_to_gaussian_full(t0, t1, d, o, radius, contracted = true): the mean and covariance k_cast_ipe_360 encodes
//   Q2  w = footprint * (2.0f * sqrtf((G.cov[0] + G.cov[3]) + G.cov[5])): the side of the uniform box whose per-axis variance w^2 / 12 is
//       the Gaussian's mean per-axis variance trace / 3 (footprint = 1) -- the yardstick a lattice Gaussian of cov_scale = 1 is baked at
//   Q3  mip_level(spacing, L, w, &l, &g): w <= spacing[0] or not a number -> (0, 0); w >= spacing[L - 1] -> (L - 1, 0)
//   Q4  v = lattice_trilinear(level l, G.mean); only when g > 0: v = (1 - g) * v + g * lattice_trilinear(level l + 1, G.mean)
// A non-finite mean gives 0 and loads nothing; a NaN corner propagates; a mean outside the box takes the edge value (|contract(x)| < 2, so
// with the usual box [-2, 2]^3 there is none).  With L == 1 the value is the plain trilinear value at the contracted mean.
//
// The levels are WALKED by a loop counter and a lane reads the level(s) it selected: the descriptors box[lv] / lattice[lv] of a by-value
// kernel argument are then indexed by a uniform value (scalar loads); indexing them by the lane's own l would move the table to scratch.
#pragma once

#include "lattice_sample.hpp"
#include "preview_mip.hpp"
#include "raymath360.hpp"

namespace mip {

constexpr int kProposalMaxLevels = 4;

struct ProposalPyramid {         // by-value kernel argument: what the host derives from mipnerf_proposal_pyramid
    int levels;                  // L
    float spacing[kProposalMaxLevels];           // strictly increasing over the first L entries
    LatticeBox box[kProposalMaxLevels];
    const float* lattice[kProposalMaxLevels];
};

// Q2
MIP_HD float proposal_footprint(float footprint, const float cov[6]) { return footprint * (2.0f * sqrtf((cov[0] + cov[3]) + cov[5])); }

// Q2 - Q4 on a Gaussian (mean, cov) of the contracted space
MIP_HD float pyramid_density(const ProposalPyramid& p, float footprint, const float mean[3], const float cov[6]) {
    const float big = 3.4028234663852886e38f;
    if (!(fabsf(mean[0]) <= big && fabsf(mean[1]) <= big && fabsf(mean[2]) <= big)) return 0.0f;      // NaN fails the comparison too
    int l;
    float g;
    mip_level(p.spacing, p.levels, proposal_footprint(footprint, cov), &l, &g);
    const bool two = g > 0.0f;
    float v = 0.0f, upper = 0.0f;
    for (int lv = 0; lv < p.levels; ++lv) {
        const bool own = l == lv, next = two && l + 1 == lv;
        if (own || next) {
            const float x = lattice_trilinear(p.lattice[lv], p.box[lv], mean[0], mean[1], mean[2]);
            if (own) v = x; else upper = x;
        }
    }
    return two ? (1.0f - g) * v + g * upper : v;
}

// Q1 - Q4 on a sample of a ray
MIP_HD float pyramid_density_sample(const ProposalPyramid& p, float footprint, float t0, float t1, const float d[3], const float o[3],
                                    float radius) {
    const GaussFull gs = conical_frustum_to_gaussian_full(t0, t1, d, o, radius, true);
    return pyramid_density(p, footprint, gs.mean, gs.cov);
}

}  // namespace mip
