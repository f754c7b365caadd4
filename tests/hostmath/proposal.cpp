// Host build of csrc/lattice_sample.hpp for tests/test_proposal_cpu.py:
//   g++ -O2 -ffp-contract=off -shared -fPIC proposal.cpp -o _proposal.so
#include "../../mipnerf_pl_amd/csrc/lattice_sample.hpp"

extern "C" {

// out[p] = the trilinear value at xyz[p] of lattice [nz, ny, nx] over lo .. hi; inv_h as the library's host code forms it
void hm_lattice_trilinear(const float* lattice, int nx, int ny, int nz, const float* lo, const float* hi, long long n, const float* xyz,
                          float* out) {
    mip::LatticeBox g;
    g.nx = nx; g.ny = ny; g.nz = nz;
    const int dims[3] = {nx, ny, nz};
    for (int a = 0; a < 3; ++a) {
        g.lo[a] = lo[a];
        g.inv_h[a] = (float)(dims[a] - 1) / (hi[a] - lo[a]);
    }
    for (long long p = 0; p < n; ++p) out[p] = mip::lattice_trilinear(lattice, g, xyz[3 * p], xyz[3 * p + 1], xyz[3 * p + 2]);
}

}  // extern "C"
