// Frame -> image bytes on the device: the two image writers of utils/vis.py:save_images, so only 3*H*W bytes per image cross to the host.
//
//  visualize_map   visualize_depth (vis.py:83-97) of the distance / acc map: nan_to_num, global min / max, (x - mi) / max(ma - mi, 1e-8)
//                  in fp32 with IEEE division, (uint8)(255 * x) truncating like astype(np.uint8), then the JET row of that value as the
//                  reference writes it (jet_table.hpp: OpenCV's BGR LUT stored by PIL as RGB).  Two launches: per-block min / max partials,
//                  then every block of the colouring kernel folds all partials itself (no atomics, no inter-block signalling).
//  image_to_u8     torchvision save_image of one image after save_image_tensor's clamp: clamp(0, 1), * 255, + 0.5, truncate.
// No allocation, no host synchronisation: both are capturable in a hipGraph.  Built with -ffp-contract=off (255 * x + 0.5 is two
// roundings on the host too).
#include <hip/hip_runtime.h>

#include <cfloat>

#include "jet_table.hpp"
#include "kernels.hpp"

namespace mip {
namespace {
constexpr int kThreads = 256, kMaxPartialBlocks = 256, kItemsPerThread = 8;

__device__ __forceinline__ float nan_to_num(float x) {
    if (x != x) return 0.0f;
    return fminf(fmaxf(x, -FLT_MAX), FLT_MAX);      // +-inf -> +-FLT_MAX
}

// (min, max) over the block; every thread gets the result
__device__ __forceinline__ void block_minmax(float& mi, float& ma, float* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        mi = fminf(mi, __shfl_xor(mi, o, 64));
        ma = fmaxf(ma, __shfl_xor(ma, o, 64));
    }
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { red[2 * w] = mi; red[2 * w + 1] = ma; }
    __syncthreads();
    mi = fminf(fminf(red[0], red[2]), fminf(red[4], red[6]));
    ma = fmaxf(fmaxf(red[1], red[3]), fmaxf(red[5], red[7]));
}

int partial_blocks(int64_t n) {
    const int64_t b = (n + (int64_t)kThreads * kItemsPerThread - 1) / ((int64_t)kThreads * kItemsPerThread);
    return (int)(b < kMaxPartialBlocks ? b : kMaxPartialBlocks);
}
}  // namespace

__global__ void __launch_bounds__(kThreads) k_map_minmax(int64_t n, const float* __restrict__ x, float* __restrict__ partial) {
    __shared__ float red[8];
    float mi = FLT_MAX, ma = -FLT_MAX;
    for (int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x; i < n; i += (int64_t)gridDim.x * kThreads) {
        const float v = nan_to_num(x[i]);
        mi = fminf(mi, v);
        ma = fmaxf(ma, v);
    }
    block_minmax(mi, ma, red);
    if (threadIdx.x == 0) {
        partial[2 * blockIdx.x] = mi;
        partial[2 * blockIdx.x + 1] = ma;
    }
}

__global__ void __launch_bounds__(kThreads) k_map_colorize(int64_t n, int nblk, const float* __restrict__ x, const float* __restrict__ partial,
                                                           unsigned char* __restrict__ out) {
    __shared__ float red[8];
    float mi = FLT_MAX, ma = -FLT_MAX;
    for (int i = threadIdx.x; i < nblk; i += kThreads) {
        mi = fminf(mi, partial[2 * i]);
        ma = fmaxf(ma, partial[2 * i + 1]);
    }
    block_minmax(mi, ma, red);
    const float range = ma - mi;                                  // inf when the map spans -FLT_MAX .. FLT_MAX, as in numpy
    const float den = range > 1e-8f ? range : 1e-8f;              // max(ma - mi, 1e-8)
    const int64_t p = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (p >= n) return;
    const float v = 255.0f * __fdiv_rn(nan_to_num(x[p]) - mi, den);
    // astype(np.uint8): v is in [0, 255] or NaN (inf / inf); NaN converts to 0 as on the host
    const int g = v >= 0.0f ? min((int)v, 255) : 0;
    out[3 * p + 0] = kJetWritten[g][0];
    out[3 * p + 1] = kJetWritten[g][1];
    out[3 * p + 2] = kJetWritten[g][2];
}

__global__ void __launch_bounds__(kThreads) k_image_to_u8(int64_t n, const float* __restrict__ x, unsigned char* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const float c = fminf(fmaxf(x[i], 0.0f), 1.0f);               // NaN -> 0
    const float v = c * 255.0f + 0.5f;                            // two roundings (-ffp-contract=off)
    out[i] = (unsigned char)(int)v;
}

int64_t visualize_partial_floats(int64_t n) { return n > 0 ? 2LL * partial_blocks(n) : 0; }

hipError_t launch_visualize_map(int64_t n, const float* map, float* partial, unsigned char* out_rgb, hipStream_t st) {
    const int nblk = partial_blocks(n);
    hipLaunchKernelGGL(k_map_minmax, dim3(nblk), dim3(kThreads), 0, st, n, map, partial);
    hipLaunchKernelGGL(k_map_colorize, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, n, nblk, map, partial, out_rgb);
    return hipGetLastError();
}

hipError_t launch_image_to_u8(int64_t n, const float* x, unsigned char* out, hipStream_t st) {
    hipLaunchKernelGGL(k_image_to_u8, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, n, x, out);
    return hipGetLastError();
}
}  // namespace mip
