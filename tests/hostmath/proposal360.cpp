// Host build of csrc/lattice_sample_360.hpp for tests/test_proposal360_cpu.py:
//   g++ -O2 -ffp-contract=off -shared -fPIC proposal360.cpp -o _proposal360.so
#include "../../mipnerf_pl_amd/csrc/lattice_sample_360.hpp"

namespace {

// the kernel argument as the library's host code forms it: dims[l] = {nx, ny, nz}, spacing = the largest axis spacing
mip::ProposalPyramid derive(int levels, const int* dims, const float* const* lattices, const float* lo, const float* hi) {
    mip::ProposalPyramid p;
    p.levels = levels;
    for (int l = 0; l < mip::kProposalMaxLevels; ++l) {
        const int s = l < levels ? l : levels - 1;
        p.box[l].nx = dims[3 * s]; p.box[l].ny = dims[3 * s + 1]; p.box[l].nz = dims[3 * s + 2];
        float spacing = 0.0f;
        for (int a = 0; a < 3; ++a) {
            const float span = hi[a] - lo[a];
            p.box[l].lo[a] = lo[a];
            p.box[l].inv_h[a] = (float)(dims[3 * s + a] - 1) / span;
            spacing = fmaxf(spacing, span / (float)(dims[3 * s + a] - 1));
        }
        p.spacing[l] = spacing;
        p.lattice[l] = lattices[s];
    }
    return p;
}

}  // namespace

extern "C" {

void hm_pyramid_spacing(int levels, const int* dims, const float* const* lattices, const float* lo, const float* hi, float* spacing) {
    const mip::ProposalPyramid p = derive(levels, dims, lattices, lo, hi);
    for (int l = 0; l < levels; ++l) spacing[l] = p.spacing[l];
}

// out[s] = rules Q2 - Q4 on the Gaussian (mean[s], cov[s]); level[s], g[s] = what mip_level returned for it (optional)
void hm_pyramid_density(int levels, const int* dims, const float* const* lattices, const float* lo, const float* hi, float footprint,
                        long long n, const float* mean, const float* cov, float* out, int* level, float* g) {
    const mip::ProposalPyramid p = derive(levels, dims, lattices, lo, hi);
    for (long long s = 0; s < n; ++s) {
        out[s] = mip::pyramid_density(p, footprint, mean + 3 * s, cov + 6 * s);
        if (level && g) mip::mip_level(p.spacing, p.levels, mip::proposal_footprint(footprint, cov + 6 * s), level + s, g + s);
    }
}

// out[s] = rules Q1 - Q4 on the sample [t0[s], t1[s]] of the ray (o[s], d[s], radius[s])
void hm_pyramid_density_sample(int levels, const int* dims, const float* const* lattices, const float* lo, const float* hi, float footprint,
                               long long n, const float* t0, const float* t1, const float* o, const float* d, const float* radius,
                               float* out) {
    const mip::ProposalPyramid p = derive(levels, dims, lattices, lo, hi);
    for (long long s = 0; s < n; ++s) out[s] = mip::pyramid_density_sample(p, footprint, t0[s], t1[s], d + 3 * s, o + 3 * s, radius[s]);
}

// Q1 alone: the contracted Gaussian of each sample
void hm_gauss_contracted(long long n, const float* t0, const float* t1, const float* o, const float* d, const float* radius, float* mean,
                         float* cov) {
    for (long long s = 0; s < n; ++s) {
        const mip::GaussFull gs = mip::conical_frustum_to_gaussian_full(t0[s], t1[s], d + 3 * s, o + 3 * s, radius[s], true);
        for (int a = 0; a < 3; ++a) mean[3 * s + a] = gs.mean[a];
        for (int k = 0; k < 6; ++k) cov[6 * s + k] = gs.cov[k];
    }
}

}  // extern "C"
