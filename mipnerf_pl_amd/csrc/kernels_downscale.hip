// Box shrink of captured images on the device: what a pre-shrunk images_<F>/ folder of an LLFF / mip-NeRF-360 capture holds, made
// from images/ at start-up (datasets.load_realdata360), as the float32 pixel rows of the data set.
//
//  S     the integer sum of the F x F source bytes of one channel of one output pixel (F <= 16: S <= 65280)
//  q     (2 S + F F) / (2 F F) in integer arithmetic: the box mean rounded half up to a byte
//  row   float(q) / 255.f, one correctly rounded division: what datasets._read_image makes of the byte q
//
// The bottom H % F rows and right W % F columns are ignored; a 4th source channel is dropped (no compositing).
//
// k_area_downscale: one workgroup owns `tile` output pixels of `group` consecutive output rows (as many rows as fit in 16 KB of LDS,
// at most 8: at small F one output row is too few bytes in flight to cover the latency of HBM, and above 16 KB fewer than eight
// workgroups stay resident per CU, which is where the overlap of one workgroup's loads with another's sums comes from).  The group * F source rows under them
// are contiguous segments of tile * F * C bytes; C = 3 puts no pixel on a 16-byte boundary, so the segments are streamed as ALIGNED 16-byte loads
// from the boundary at or below each segment's first byte (the 16 bytes that would cross the end of the source are read bytewise)
// into LDS at the same misalignment, and every lane sums the F x F x 3 bytes of one pixel per output row from there with integer adds.  No atomics, nothing shared
// between workgroups, plain vector stores.  Bound by HBM: C bytes read per source pixel, 12 / F^2 written.  Offsets are 64-bit (a data
// set passes 4 GiB).  No allocation, no host synchronisation: capturable.
#include <hip/hip_runtime.h>

#include "kernels.hpp"

namespace mip {
namespace {
constexpr int kThreads = 256;
constexpr int kLdsBudget = 32768;        // bytes of LDS one output row of a workgroup may use (reached at F = 16 only)
constexpr int kGroupBudget = 16384;      // rows are grouped while they fit in this much: eight workgroups stay resident per CU
constexpr int kMaxGroup = 8;             // output rows per workgroup
}  // namespace

// src [n, H, W, C] bytes, 16-byte aligned, `total` bytes in all; out [n * h * w, 3] floats, h = H / F, w = W / F.
// stride = bytes of LDS per source row (a multiple of 16, >= 15 + tile * F * C); tiles = ceil(w / tile); groups = ceil(h / group).
template <int C>
__global__ void __launch_bounds__(kThreads) k_area_downscale(int H, int W, int F, int h, int w, int tile, int tiles, int group, int groups, int stride, int64_t total,
                                                             const unsigned char* __restrict__ src, float* __restrict__ out) {
    extern __shared__ uint4 lds16[];
    unsigned char* lds = reinterpret_cast<unsigned char*>(lds16);
    const int64_t b = blockIdx.x;
    const int tx = (int)(b % tiles), y0 = (int)((b / tiles) % groups) * group;
    const int64_t img = b / ((int64_t)tiles * groups);
    const int x0 = tx * tile;
    const int npix = min(tile, w - x0), nrows = min(group, h - y0);
    // first byte of source row r of the tile: first + r * W * C
    const int64_t first = (((img * H + (int64_t)y0 * F) * W) + (int64_t)x0 * F) * C;
    const int rowbytes = W * C;
    const int chunks = stride >> 4;
    for (int r = 0; r < nrows * F; ++r) {
        const int64_t row0 = (first + (int64_t)r * rowbytes) & ~(int64_t)15;
        for (int k = threadIdx.x; k < chunks; k += kThreads) {
            const int64_t g = row0 + ((int64_t)k << 4);
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (g + 16 <= total) {
                v = *reinterpret_cast<const uint4*>(src + g);
            } else if (g < total) {          // the last, partial 16 bytes of the source
                unsigned int wd[4] = {0u, 0u, 0u, 0u};
                for (int j = 0; j < (int)(total - g); ++j) wd[j >> 2] |= (unsigned int)src[g + j] << (8 * (j & 3));
                v = make_uint4(wd[0], wd[1], wd[2], wd[3]);
            }
            lds16[r * chunks + k] = v;
        }
    }
    __syncthreads();
    const int t = threadIdx.x;
    if (t >= npix) return;
    const unsigned int area = (unsigned int)(F * F);
    for (int g = 0; g < nrows; ++g) {
        unsigned int sum[3] = {0u, 0u, 0u};
        for (int r = g * F; r < (g + 1) * F; ++r) {
            const int head = (int)((first + (int64_t)r * rowbytes) & 15);
            const unsigned char* p = lds + r * stride + head + t * F * C;
            for (int dx = 0; dx < F; ++dx) {
#pragma unroll
                for (int c = 0; c < 3; ++c) sum[c] += p[dx * C + c];
            }
        }
        float* o = out + (((img * h + y0 + g) * (int64_t)w) + x0 + t) * 3;
#pragma unroll
        for (int c = 0; c < 3; ++c) o[c] = __fdiv_rn((float)((2u * sum[c] + area) / (2u * area)), 255.0f);
    }
}

hipError_t launch_area_downscale(int64_t n, int H, int W, int C, int F, const unsigned char* src, float* out_rgb, hipStream_t st) {
    const int h = H / F, w = W / F;
    int tile = (kLdsBudget / F - 32) / (F * C);
    tile = tile < kThreads ? tile : kThreads;
    tile = tile < w ? tile : w;
    const int tiles = (w + tile - 1) / tile;
    tile = (w + tiles - 1) / tiles;          // equal tiles: no workgroup of a row is left with a sliver
    const int stride = (tile * F * C + 15 + 15) / 16 * 16;
    int group = kGroupBudget / (F * stride);
    group = group > 1 ? group : 1;
    group = group < kMaxGroup ? group : kMaxGroup;
    group = group < h ? group : h;
    const int groups = (h + group - 1) / group;
    const int64_t blocks = n * groups * tiles;
    if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
    const int64_t total = n * H * (int64_t)W * C;
    const dim3 grid((unsigned)blocks), block(kThreads);
    const size_t lds = (size_t)group * F * stride;
    if (C == 3)
        hipLaunchKernelGGL(k_area_downscale<3>, grid, block, lds, st, H, W, F, h, w, tile, tiles, group, groups, stride, total, src, out_rgb);
    else
        hipLaunchKernelGGL(k_area_downscale<4>, grid, block, lds, st, H, W, F, h, w, tile, tiles, group, groups, stride, total, src, out_rgb);
    return hipGetLastError();
}
}  // namespace mip
