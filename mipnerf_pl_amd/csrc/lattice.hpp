// Lattice geometry shared by the kernels that walk a lattice by its flat index (kernels_mesh.hip, kernels_360.hip):
// point (i, j, k) has the flat index (k * ny + j) * nx + i and, per axis, the mean lo + float(i) * h with h = (hi - lo) / float(n - 1)
// (include/mipnerf_hip.h).  Units that include this are compiled with -ffp-contract=off, so the mean rounds as stated there.
#pragma once

#include <hip/hip_runtime.h>

namespace mip {

struct Lattice {
    int nx, ny, nz;
    float lo[3], hi[3];
};

inline Lattice make_lattice(const int dims[3], const float lo[3], const float hi[3]) {
    Lattice g;
    g.nx = dims[0]; g.ny = dims[1]; g.nz = dims[2];
    for (int a = 0; a < 3; ++a) { g.lo[a] = lo[a]; g.hi[a] = hi[a]; }
    return g;
}

__device__ __forceinline__ float lattice_step(const Lattice& g, int a) {
    const int n = a == 0 ? g.nx : (a == 1 ? g.ny : g.nz);
    return (g.hi[a] - g.lo[a]) / (float)(n - 1);
}

__device__ __forceinline__ void lattice_ijk(const Lattice& g, int p, int& i, int& j, int& k) {
    const int row = p / g.nx;
    i = p - row * g.nx;
    k = row / g.ny;
    j = row - k * g.ny;
}

}  // namespace mip
