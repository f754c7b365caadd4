// The density lattice as the proposal level of a chunk forward (include/mipnerf_hip.h, mipnerf_lattice_density /
// mipnerf_forward_proposal): the coarse level's density is read from a lattice of the field's own pre-filtered density
// (mipnerf_density_grid) instead of an MLP pass.  Elementwise: one thread per sample, 8 gathered loads and a 16-byte store, no
// wave-level cooperation -- so it is not one of the samples-per-lane per-ray kernels.  Compiled with -ffp-contract=off: the frustum
// mean rounds as in k_cast_rays / k_cast_ipe (raymath.hpp) and the blend as stated in lattice_sample.hpp.
#include <hip/hip_runtime.h>

#include "kernels.hpp"
#include "lane_buckets.hpp"
#include "lattice_sample.hpp"
#include "raymath.hpp"

namespace mip {

// rgb_sigma[b, i] = (0, 0, 0, lattice at the mean of the conical frustum [t_i, t_{i+1}] of ray b)
__global__ void __launch_bounds__(256)
k_lattice_density(LatticeBox g, const float* __restrict__ lattice, int64_t B, int N, const float* __restrict__ t,
                  const float* __restrict__ origins, const float* __restrict__ dirs, const float* __restrict__ radii,
                  float4* __restrict__ rgb_sigma) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= B * (int64_t)N) return;
    const int64_t b = s / N;
    const int i = (int)(s - b * N);
    const float d[3] = {dirs[b * 3], dirs[b * 3 + 1], dirs[b * 3 + 2]};
    const float o[3] = {origins[b * 3], origins[b * 3 + 1], origins[b * 3 + 2]};
    const float t0 = t[b * (N + 1) + i], t1 = t[b * (N + 1) + i + 1];
    const Gauss3 gs = conical_frustum_to_gaussian(t0, t1, d, o, radii[b]);      // the mean k_cast_ipe encodes; the covariance is unused
    const float sigma = lattice_trilinear(lattice, g, gs.mean[0], gs.mean[1], gs.mean[2]);
    rgb_sigma[s] = make_float4(0.0f, 0.0f, 0.0f, sigma);
}

hipError_t launch_lattice_density(const LatticeBox& g, const float* lattice, int64_t B, int N, const float* t, const float* origins,
                                  const float* dirs, const float* radii, float* rgb_sigma, hipStream_t st) {
    hipLaunchKernelGGL(k_lattice_density, dim3(grid_for(B * (int64_t)N, 256)), dim3(256), 0, st, g, lattice, B, N, t, origins, dirs, radii,
                       (float4*)rgb_sigma);
    return hipGetLastError();
}

}  // namespace mip
