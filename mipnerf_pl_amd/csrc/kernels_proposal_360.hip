// The proposal density of the unbounded-scene model (include/mipnerf_proposal_360.h, mipnerf_lattice_density_360): per sample, the value
// of a small pyramid of contracted density lattices at the sample's own contracted Gaussian, the level chosen from its covariance
// (lattice_sample_360.hpp states the rule once).  Elementwise like k_lattice_density: one thread per sample, 8 gathered loads per level
// read (one level, or two when the footprint falls between two spacings) and one 16-byte store; no LDS, no atomics, no wave-level
// cooperation -- so it is not one of the samples-per-lane per-ray kernels.  The pyramid travels by value in the kernel arguments and its
// levels are walked by a loop counter, so the level descriptors are scalar loads.  Compiled with -ffp-contract=off: the Gaussian rounds
// as in k_cast_ipe_360 (raymath360.hpp) and the blends as stated in lattice_sample.hpp and lattice_sample_360.hpp.
#include <hip/hip_runtime.h>

#include "lattice_sample_360.hpp"

namespace mip {

// rgb_sigma[b, i] = (0, 0, 0, pyramid at the contracted Gaussian of the conical frustum [t_i, t_{i+1}] of ray b)
__global__ void __launch_bounds__(256)
k_lattice_density_360(ProposalPyramid p, float footprint, int64_t B, int N, const float* __restrict__ t, const float* __restrict__ origins,
                      const float* __restrict__ dirs, const float* __restrict__ radii, float4* __restrict__ rgb_sigma) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= B * (int64_t)N) return;
    const int64_t b = s / N;
    const int i = (int)(s - b * N);
    const float d[3] = {dirs[b * 3], dirs[b * 3 + 1], dirs[b * 3 + 2]};
    const float o[3] = {origins[b * 3], origins[b * 3 + 1], origins[b * 3 + 2]};
    const float t0 = t[b * (N + 1) + i], t1 = t[b * (N + 1) + i + 1];
    const float sigma = pyramid_density_sample(p, footprint, t0, t1, d, o, radii[b]);
    rgb_sigma[s] = make_float4(0.0f, 0.0f, 0.0f, sigma);
}

hipError_t launch_lattice_density_360(const ProposalPyramid& p, float footprint, int64_t B, int N, const float* t, const float* origins,
                                      const float* dirs, const float* radii, float* rgb_sigma, hipStream_t st) {
    const int64_t blocks = (B * (int64_t)N + 255) / 256;        // B < 2^31 and N <= 1024: < 2^31 blocks
    hipLaunchKernelGGL(k_lattice_density_360, dim3((unsigned)blocks), dim3(256), 0, st, p, footprint, B, N, t, origins, dirs, radii,
                       (float4*)rgb_sigma);
    return hipGetLastError();
}

// t = 1 / t_inv per fence post: what the level loop of the drop-in library does between the inverse-depth resampling and the encoding
// (k_reciprocal of kernels_360.hip: the same expression under the same flags, so the same bits)
__global__ void __launch_bounds__(256) k_reciprocal_360(int64_t n, const float* __restrict__ x, float* __restrict__ y) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) y[i] = 1.0f / x[i];
}

hipError_t launch_reciprocal_360(int64_t n, const float* x, float* y, hipStream_t st) {
    hipLaunchKernelGGL(k_reciprocal_360, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, n, x, y);
    return hipGetLastError();
}

}  // namespace mip
