// Host build of the un-contraction math (mipnerf_pl_amd/csrc/raymath360.hpp -- the source the gfx950 kernel k_uncontract inlines) for
// tests/test_mesh360_cpu.py; g++ -O2 -ffp-contract=off.
#include "../../mipnerf_pl_amd/csrc/raymath.hpp"
#include "../../mipnerf_pl_amd/csrc/raymath360.hpp"

extern "C" {
// z, g, x, normals [n, 3]
void um_uncontract(int n, float far_radius, const float* z, const float* g, float* x, float* normals) {
    for (int i = 0; i < n; ++i) {
        mip::uncontract_point(z + 3 * i, far_radius, x + 3 * i);
        mip::uncontract_normal(z + 3 * i, far_radius, g + 3 * i, normals + 3 * i);
    }
}
// contract() of a point through the Gaussian form the kernels use (zero covariance)
void um_contract(int n, const float* x, float* z) {
    for (int i = 0; i < n; ++i) {
        mip::GaussFull gs;
        for (int a = 0; a < 3; ++a) gs.mean[a] = x[3 * i + a];
        for (int a = 0; a < 6; ++a) gs.cov[a] = 0.0f;
        mip::contract_gaussian(gs);
        for (int a = 0; a < 3; ++a) z[3 * i + a] = gs.mean[a];
    }
}
}
