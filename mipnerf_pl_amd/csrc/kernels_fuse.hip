// Rendered depth fused into a truncated signed distance volume (include/mipnerf_fuse.h): the depth quantile of a ray's weights, the
// integration of depth frames into a lattice, and the pass that turns the two planes into the lattice the isosurface is cut from.
// csrc/fuse_rules.hpp states the rules once; the kernels call its functions.  Compiled with -ffp-contract=off.
#include <hip/hip_runtime.h>

#include "fuse_rules.hpp"
#include "raywave.hpp"

namespace mip {

struct FuseQuantiles {
    int count;
    float q[kFuseMaxQuantiles];
};

// One wavefront per ray, lane l holding the K consecutive samples l * K .. l * K + K - 1.  A lane sums its samples in double (D1, D2), one
// double wave scan gives the lanes' inclusive prefixes and the wave shift hands each lane its predecessor's: P_i = that + the lane's
// running sum, and the lane's last sample takes the scan's own value, so every interval's lower end IS the previous interval's upper end.
// The one lane that owns the crossing writes; a ballot finds the ray that has none.  No LDS, no atomics, no scratch.
template <int K>
__global__ void __launch_bounds__(64 * kRaysPerBlock)
k_depth_quantile(int64_t B, int N, const float* __restrict__ weights, const float* __restrict__ t, FuseQuantiles qs,
                 float* __restrict__ depth) {
    const int lane = threadIdx.x & 63;
    const int64_t b = (int64_t)blockIdx.x * kRaysPerBlock + (threadIdx.x >> 6);
    if (b >= B) return;                                        // the whole wave: no block barrier follows
    const float* __restrict__ wb = weights + b * N;
    const float* __restrict__ tb = t + b * (int64_t)(N + 1);
    const int i0 = lane * K;
    float w[K], tv[K + 1];
    double loc[K];
    double run = 0.0;
#pragma unroll
    for (int k = 0; k <= K; ++k) tv[k] = (i0 + k <= N) ? tb[i0 + k] : 0.0f;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        w[k] = (i0 + k < N) ? quantile_weight(wb[i0 + k]) : 0.0f;
        run += (double)w[k];
        loc[k] = run;
    }
    const double incl = wave_incl_scan_dpp(run);
    const double before = dpp_f64<kDppWaveShr1, 0xf>(incl);     // lane l <- lane l - 1, lane 0 <- 0
#pragma unroll
    for (int j = 0; j < kFuseMaxQuantiles; ++j) {
        if (j < qs.count) {
            const double q = (double)qs.q[j];
            bool found = false;
            double P_prev = before;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const double P_here = k == K - 1 ? incl : before + loc[k];
                if (i0 + k < N && quantile_crosses(P_prev, q, P_here)) {
                    depth[b * qs.count + j] = quantile_depth(P_prev, q, w[k], tv[k], tv[k + 1]);
                    found = true;
                }
                P_prev = P_here;
            }
            if (__ballot(found) == 0ull && lane == 0) depth[b * qs.count + j] = INFINITY;      // D4
        }
    }
}

hipError_t launch_depth_quantile(int64_t B, int N, const float* weights, const float* t, int nq, const float* q, float* depth,
                                 hipStream_t st) {
    FuseQuantiles qs;
    qs.count = nq;
    for (int j = 0; j < kFuseMaxQuantiles; ++j) qs.q[j] = q[j < nq ? j : nq - 1];
    const dim3 grid(grid_for(B, kRaysPerBlock)), block(64 * kRaysPerBlock);
    const bool ok = for_lane_bucket(N, [&](auto k) {
        hipLaunchKernelGGL((k_depth_quantile<decltype(k)::value>), grid, block, 0, st, B, N, weights, t, qs, depth);
    });
    return ok ? hipGetLastError() : hipErrorInvalidValue;
}

// One thread per lattice point, x fastest across the lanes: the two planes are read and written coalesced.  The frame loop runs inside
// the kernel; a point's sum and count stay in registers over the launch's frames and are stored once, where a frame touched the point.
// The frame records and offsets are indexed by the loop counter alone, so they arrive by wave-uniform (scalar) loads.
__global__ void __launch_bounds__(256)
k_fuse_integrate(FuseLattice g, float trunc, int carve, int num_frames, const float* __restrict__ frames,
                 const int64_t* __restrict__ offsets, const float* __restrict__ depth, int64_t depth_count, float* __restrict__ sum,
                 float* __restrict__ count) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (int64_t)g.nx * g.ny * g.nz) return;
    const int i = (int)(idx % g.nx), jk = (int)(idx / g.nx);
    const int j = jk % g.ny, k = jk / g.ny;
    const float x = fuse_point(g.lo[0], i, g.h[0]), y = fuse_point(g.lo[1], j, g.h[1]), z = fuse_point(g.lo[2], k, g.h[2]);
    float s = sum[idx], c = count[idx];
    bool touched = false;
    for (int f = 0; f < num_frames; ++f) {
        float d;
        if (fuse_frame_update(frames + (size_t)f * kFuseFrameFloats, offsets[f], depth, depth_count, trunc, carve, x, y, z, &d)) {
            s += d;                                             // T6
            c += 1.0f;
            touched = true;
        }
    }
    if (touched) {
        sum[idx] = s;
        count[idx] = c;
    }
}

hipError_t launch_fuse_integrate(const FuseLattice& g, float trunc, int carve, int64_t num_frames, const float* frames,
                                 const int64_t* offsets, const float* depth, int64_t depth_count, float* sum, float* count,
                                 hipStream_t st) {
    const int64_t n = (int64_t)g.nx * g.ny * g.nz;              // 7 n < 2^31
    for (int64_t f0 = 0; f0 < num_frames; f0 += kFuseFramesPerLaunch) {
        const int nf = (int)(num_frames - f0 < kFuseFramesPerLaunch ? num_frames - f0 : kFuseFramesPerLaunch);
        hipLaunchKernelGGL(k_fuse_integrate, dim3(grid_for(n, 256)), dim3(256), 0, st, g, trunc, carve, nf,
                           frames + f0 * kFuseFrameFloats, offsets + f0, depth, depth_count, sum, count);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

__global__ void __launch_bounds__(256)
k_fuse_finalise(int64_t n, const float* __restrict__ sum, const float* __restrict__ count, float fill, float* __restrict__ lattice) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx < n) lattice[idx] = fuse_finalise_value(sum[idx], count[idx], fill);
}

hipError_t launch_fuse_finalise(int64_t n, const float* sum, const float* count, float fill, float* lattice, hipStream_t st) {
    hipLaunchKernelGGL(k_fuse_finalise, dim3(grid_for(n, 256)), dim3(256), 0, st, n, sum, count, fill, lattice);
    return hipGetLastError();
}

}  // namespace mip
