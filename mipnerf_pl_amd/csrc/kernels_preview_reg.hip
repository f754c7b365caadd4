// The kernel of libmipnerf_preview_reg.so (include/mipnerf_preview_reg.h):
//   k_preview_reg_grad   the gradient of the total-variation term and of the SH decay, ADDED INTO grad: a gather, no atomics
// Every rule is preview_reg.hpp's, by call.  The mapping is k_preview_tune_adam's: one thread per point and 4-entry chunk, consecutive
// threads walk the chunks of a point and then the points along x, 16-byte loads, a grid-stride loop.  A thread reads the 13 chunks of
// rule R3 (its own, p + e_a, p - e_a, p - e_a + e_b), each only when its point is present, and the 4 entries of grad it owns; the
// x-neighbours' chunks are the lines its neighbour lanes read anyway; the y / z neighbours' lines are read again by the threads one x-line
// or one xy-plane away, in other blocks and mostly on other XCDs, and measure as L2 misses more often than hits (the kernel
// costs less than the Adam pass, at 1.6 - 3.3 x a copy of its bytes; a tile per block with its halo in LDS is the form not built).  No
// LDS, no atomics, no inline assembly.
#include <hip/hip_runtime.h>

#include "preview_reg.hpp"

namespace mip {

namespace {

__device__ __forceinline__ float4 reg_chunk(const float* __restrict__ master, bool present, int64_t point, int ch_per_row, int chunk) {
    return present ? reinterpret_cast<const float4*>(master)[point * ch_per_row + chunk] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

}  // namespace

template <int DEG>
__global__ void __launch_bounds__(256)
k_preview_reg_grad(const PreviewReg p, const float* __restrict__ master, const uint8_t* __restrict__ mask, float* __restrict__ grad) {
    constexpr int W = preview_row_halves(DEG), CH = W / 4, USED = reg_row_used(DEG), LIVE = (USED + 3) / 4;      // chunks with a used entry
    const int64_t n_points = (int64_t)p.nx * p.ny * p.nz;
    const int64_t n_chunks = n_points * LIVE, stride = (int64_t)gridDim.x * 256;      // n_chunks <= 7 nx ny nz < 2^31
    const int64_t sy = p.nx, sz = (int64_t)p.nx * p.ny;
    for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < n_chunks; k += stride) {
        const uint32_t point = (uint32_t)k / (uint32_t)LIVE;
        const int chunk = (int)((uint32_t)k - point * (uint32_t)LIVE);
        if (mask != nullptr && mask[point] == 0) continue;           // a masked-out point: grad is not touched
        const bool tv = (chunk == 0 && p.w_sigma != 0.0f) || ((chunk > 0 || USED > 1) && p.w_colour != 0.0f);      // a stencil is needed
        bool any = false;
#pragma unroll
        for (int e = 0; e < 4; ++e) any = any || (chunk * 4 + e < USED && reg_touches(p, chunk * 4 + e));
        if (!any) continue;
        const uint32_t line = point / (uint32_t)p.nx;
        const int x = (int)(point - line * (uint32_t)p.nx), z = (int)(line / (uint32_t)p.ny), y = (int)(line - (uint32_t)z * (uint32_t)p.ny);
        RegStencil s = {};
        if (tv) reg_stencil(p, mask, x, y, z, &s);                   // the decay alone reads the thread's own chunk only
        const int64_t step[3] = {1, sy, sz};
        const float4 c4 = reg_chunk(master, true, point, CH, chunk);
        float4 fwd4[3], back4[3], side4[3][3];
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            fwd4[a] = reg_chunk(master, s.fwd[a], (int64_t)point + step[a], CH, chunk);
            back4[a] = reg_chunk(master, s.back[a], (int64_t)point - step[a], CH, chunk);
#pragma unroll
            for (int b = 0; b < 3; ++b)
                side4[a][b] = reg_chunk(master, b != a && s.side[a][b], (int64_t)point - step[a] + step[b], CH, chunk);
        }
        const int64_t at = (int64_t)point * CH + chunk;              // in float4
        const int used = USED - chunk * 4 < 4 ? USED - chunk * 4 : 4;
        float g[4];
        if (used == 4) {
            const float4 g4 = reinterpret_cast<const float4*>(grad)[at];
            g[0] = g4.x; g[1] = g4.y; g[2] = g4.z; g[3] = g4.w;
        } else {                                                     // a chunk that ends in padding: the pad entries are not read
#pragma unroll
            for (int e = 0; e < 4; ++e) g[e] = e < used ? grad[at * 4 + e] : 0.0f;
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int entry = chunk * 4 + e;
            if (e >= used || !reg_touches(p, entry)) continue;
            float fwd[3], back[3], side[3][3];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                fwd[a] = reinterpret_cast<const float*>(&fwd4[a])[e];
                back[a] = reinterpret_cast<const float*>(&back4[a])[e];
#pragma unroll
                for (int b = 0; b < 3; ++b) side[a][b] = reinterpret_cast<const float*>(&side4[a][b])[e];
            }
            g[e] = reg_add(p, s, entry, g[e], reinterpret_cast<const float*>(&c4)[e], fwd, back, side);
        }
        if (used == 4) {
            reinterpret_cast<float4*>(grad)[at] = make_float4(g[0], g[1], g[2], g[3]);
        } else {                                                     // and not written
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (e < used) grad[at * 4 + e] = g[e];
        }
    }
}

hipError_t launch_preview_reg_grad(const PreviewReg& p, int degree, const float* master, const uint8_t* mask, float* grad, hipStream_t stream) {
    const auto kernel = degree == 0 ? k_preview_reg_grad<0> : degree == 1 ? k_preview_reg_grad<1> : k_preview_reg_grad<2>;
    const int64_t chunks = (int64_t)p.nx * p.ny * p.nz * ((reg_row_used(degree) + 3) / 4);
    const int64_t want = (chunks + 255) / 256;
    const unsigned blocks = (unsigned)(want < 1 ? 1 : want > 256 * 64 ? 256 * 64 : want);      // 256 CUs x 64: the loop strides over the rest
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), 0, stream, p, master, mask, grad);
    return hipGetLastError();
}

}  // namespace mip
