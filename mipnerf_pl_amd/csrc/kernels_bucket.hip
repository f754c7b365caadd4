// Adaptive sample counts for whole frames (gfx950, wave64): the live rays of a frame partitioned by the sample count their occupied span
// needs, and the way back.
//   the rule (include/mipnerf_hip.h, mipnerf_bucket_rays): need = ((last - first + 1) * N + S - 1) / S, bucket = the smallest b with
//                                c_b >= need; a dead ray has bucket -1.  bucket_of() below is its one statement on the device;
//   k_bucket_count               per block of 1024 rays one count per bucket: a thread packs the counts of its 4 consecutive rays into 16-bit
//                                fields of two 64-bit words (a field holds at most 1024), the block sums the words;
//   k_bucket_scan                ONE workgroup: per bucket, in bucket order, an exclusive scan of its block counts that starts at the
//                                bucket's base, base_0 = 0 and base_{b+1} = round_up(base_b + count_b, 64); the counts go to the header;
//   k_bucket_gather              the same packed words scanned exclusively over the block's threads give every ray its rank inside its
//                                (bucket, block); the ray's seven fields go to slot block base + rank, slot[ray] = that slot or -1;
//   k_gather_frame               one thread per pixel: slot >= 0 copies the compact slot, slot < 0 is the dead-pixel rule of k_scatter_frame.
// Within a bucket the rays keep their order.  No atomics anywhere: two runs give the same bytes.  Every result leaves through ordinary vector
// stores.  Padding slots between the segments are never written.
#include <hip/hip_runtime.h>

#include "kernels.hpp"
#include "lane_buckets.hpp"

namespace mip {

constexpr int kBktBlock = 256;
constexpr int kBktPer = 4;              // consecutive rays per thread
constexpr int kBktTile = kBktBlock * kBktPer;
constexpr int kBktScanBlock = 1024;
constexpr int kBktAlign = 64;           // a segment starts at a multiple of this many rays
static_assert(kBktTile <= 0xffff, "a 16-bit field holds a block's count");
static_assert(kMaxBuckets == 8, "two words of four 16-bit fields");

// the one statement of the rule: 1 <= span <= S for a live ray, so 1 <= need <= N = c_{B-1} and the loop always ends on a bucket
__device__ __forceinline__ int bucket_of(const BucketRule& r, bool live, int first, int last) {
    if (!live) return -1;
    int span = last - first + 1;
    span = span < 1 ? 1 : (span > r.S ? r.S : span);                      // whatever first / last hold, the slot stays inside the buffers
    const int need = (span * r.N + r.S - 1) / r.S;
    int b = 0;
    while (b < r.B - 1 && r.c[b] < need) ++b;
    return b;
}

// the buckets of rays p0 .. p0 + 3 (-1: dead or past the end) and their counts as 16-bit fields: buckets 0 .. 3 in lo, 4 .. 7 in hi
__device__ __forceinline__ void bkt_thread(const BucketRule& r, int64_t n, int64_t p0, const unsigned char* __restrict__ live,
                                           const int* __restrict__ first, const int* __restrict__ last, int bk[kBktPer],
                                           unsigned long long& lo, unsigned long long& hi) {
    lo = 0ull; hi = 0ull;
#pragma unroll
    for (int q = 0; q < kBktPer; ++q) {
        const int64_t p = p0 + q;
        bk[q] = p < n ? bucket_of(r, live[p] != 0, first[p], last[p]) : -1;
        if (bk[q] >= 0) {
            const unsigned long long one = 1ull << (16 * (bk[q] & 3));
            if (bk[q] < 4) lo += one; else hi += one;
        }
    }
}

// workgroup-wide exclusive scan of two packed words (WAVES * 64 threads; s_wave holds 2 * WAVES words), fixed order.  No field overflows:
// a field's block total is at most kBktTile.
template <int WAVES>
__device__ __forceinline__ void bkt_block_scan(unsigned long long& a, unsigned long long& b, unsigned long long* s_wave,
                                               unsigned long long& total_a, unsigned long long& total_b) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned long long ia = a, ib = b;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long oa = __shfl_up(ia, d, 64), ob = __shfl_up(ib, d, 64);
        if (lane >= d) { ia += oa; ib += ob; }
    }
    __syncthreads();                      // s_wave may still be read by an earlier call
    if (lane == 63) { s_wave[2 * wave] = ia; s_wave[2 * wave + 1] = ib; }
    __syncthreads();
    unsigned long long base_a = 0, base_b = 0;
    total_a = 0; total_b = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
        const unsigned long long xa = s_wave[2 * w], xb = s_wave[2 * w + 1];
        if (w < wave) { base_a += xa; base_b += xb; }
        total_a += xa; total_b += xb;
    }
    a = base_a + ia - a;
    b = base_b + ib - b;
}

__device__ __forceinline__ unsigned bkt_field(unsigned long long lo, unsigned long long hi, int b) {
    return (unsigned)(((b < 4 ? lo : hi) >> (16 * (b & 3))) & 0xffffull);
}

// block_sum [B][nblocks]: the count of bucket b in block blk
__global__ void __launch_bounds__(kBktBlock)
k_bucket_count(int64_t n, BucketRule rule, int64_t nblocks, const unsigned char* __restrict__ live, const int* __restrict__ first,
               const int* __restrict__ last, unsigned* __restrict__ block_sum) {
    __shared__ unsigned long long s_wave[2 * kBktBlock / 64];
    const int64_t p0 = ((int64_t)blockIdx.x * kBktBlock + threadIdx.x) * kBktPer;
    int bk[kBktPer];
    unsigned long long lo, hi, tlo, thi;
    bkt_thread(rule, n, p0, live, first, last, bk, lo, hi);
    bkt_block_scan<kBktBlock / 64>(lo, hi, s_wave, tlo, thi);
    if (threadIdx.x < rule.B) block_sum[(int64_t)threadIdx.x * nblocks + blockIdx.x] = bkt_field(tlo, thi, threadIdx.x);
}

// ONE workgroup: the counts of bucket b become exclusive slot bases in place, in block order, starting at the bucket's base;
// header[b] = count_b for b < B
__global__ void __launch_bounds__(kBktScanBlock)
k_bucket_scan(int num_buckets, int64_t nblocks, unsigned* __restrict__ block_sum, unsigned long long* __restrict__ header) {
    __shared__ unsigned s_wave[kBktScanBlock / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned run = 0;                                                     // uniform over the workgroup
    for (int bkt = 0; bkt < num_buckets; ++bkt) {
        const unsigned base = run;
        unsigned* sums = block_sum + (int64_t)bkt * nblocks;
        for (int64_t b0 = 0; b0 < nblocks; b0 += kBktScanBlock * kBktPer) {
            const int64_t b = b0 + (int64_t)threadIdx.x * kBktPer;
            unsigned v[kBktPer], s = 0;
#pragma unroll
            for (int r = 0; r < kBktPer; ++r) {
                v[r] = b + r < nblocks ? sums[b + r] : 0u;
                s += v[r];
            }
            unsigned is = s;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const unsigned o = __shfl_up(is, d, 64);
                if (lane >= d) is += o;
            }
            __syncthreads();                                              // the last round's reads of s_wave are done
            if (lane == 63) s_wave[wave] = is;
            __syncthreads();
            unsigned before = 0, total = 0;
#pragma unroll
            for (int w = 0; w < kBktScanBlock / 64; ++w) {
                const unsigned x = s_wave[w];
                if (w < wave) before += x;
                total += x;
            }
            unsigned ex = run + before + is - s;
#pragma unroll
            for (int r = 0; r < kBktPer; ++r) {
                if (b + r < nblocks) sums[b + r] = ex;
                ex += v[r];
            }
            run += total;
        }
        if (threadIdx.x == 0) header[bkt] = (unsigned long long)(run - base);
        run = (run + (kBktAlign - 1)) / kBktAlign * kBktAlign;
    }
}

struct BucketSoA {
    const float* in[7];
    float* out[7];
};

__global__ void __launch_bounds__(kBktBlock)
k_bucket_gather(int64_t n, BucketRule rule, int64_t nblocks, const unsigned char* __restrict__ live, const int* __restrict__ first,
                const int* __restrict__ last, const unsigned* __restrict__ block_base, BucketSoA rays, int* __restrict__ slot_out) {
    __shared__ unsigned long long s_wave[2 * kBktBlock / 64];
    const int64_t p0 = ((int64_t)blockIdx.x * kBktBlock + threadIdx.x) * kBktPer;
    int bk[kBktPer];
    unsigned long long lo, hi, tlo, thi;
    bkt_thread(rule, n, p0, live, first, last, bk, lo, hi);
    bkt_block_scan<kBktBlock / 64>(lo, hi, s_wave, tlo, thi);             // lo / hi: the ranks of this thread's first ray of each bucket
#pragma unroll
    for (int q = 0; q < kBktPer; ++q) {
        const int64_t p = p0 + q;
        if (p >= n) break;
        const int b = bk[q];
        if (b < 0) { slot_out[p] = -1; continue; }
        const int64_t slot = (int64_t)block_base[(int64_t)b * nblocks + blockIdx.x] + bkt_field(lo, hi, b);
        const unsigned long long one = 1ull << (16 * (b & 3));
        if (b < 4) lo += one; else hi += one;
        slot_out[p] = (int)slot;
#pragma unroll
        for (int f = 0; f < 3; ++f) {                                    // origins, directions, viewdirs [n, 3]
            if (rays.out[f] == nullptr) continue;
#pragma unroll
            for (int a = 0; a < 3; ++a) rays.out[f][slot * 3 + a] = rays.in[f][p * 3 + a];
        }
#pragma unroll
        for (int f = 3; f < 7; ++f)                                      // radii, lossmult, near, far [n, 1]
            if (rays.out[f] != nullptr) rays.out[f][slot] = rays.in[f][p];
    }
}

int64_t bucket_num_blocks(int64_t n) { return (n + kBktTile - 1) / kBktTile; }

hipError_t launch_bucket_rays(int64_t n, const BucketRule& rule, const unsigned char* live, const int* first, const int* last,
                              const float* const in[7], float* const out[7], int* slot, unsigned* block_sum, unsigned long long* header,
                              hipStream_t st) {
    const int64_t nb = bucket_num_blocks(n);
    BucketSoA rays;
    for (int q = 0; q < 7; ++q) { rays.in[q] = in[q]; rays.out[q] = out[q]; }
    hipLaunchKernelGGL(k_bucket_count, dim3((unsigned)nb), dim3(kBktBlock), 0, st, n, rule, nb, live, first, last, block_sum);
    hipLaunchKernelGGL(k_bucket_scan, dim3(1), dim3(kBktScanBlock), 0, st, rule.B, nb, block_sum, header);
    hipLaunchKernelGGL(k_bucket_gather, dim3((unsigned)nb), dim3(kBktBlock), 0, st, n, rule, nb, live, first, last, block_sum, rays, slot);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------
// the way back: every pixel of every level is written once
// ------------------------------------------------------------------------------------------
struct GatherLevels {
    int n;
    const float* c_rgb[kMaxScatterLevels];
    const float* c_dist[kMaxScatterLevels];
    const float* c_acc[kMaxScatterLevels];
    float* f_rgb[kMaxScatterLevels];
    float* f_dist[kMaxScatterLevels];
    float* f_acc[kMaxScatterLevels];
};

// a slot outside [0, rows) is no slot of the compact buffers: the pixel is written as a dead one
__global__ void __launch_bounds__(256)
k_gather_frame(int64_t n, int64_t rows, const int* __restrict__ slot, const float* __restrict__ nearp, float bkgd, GatherLevels lv) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    const int64_t s = slot[p];
    if (s >= 0 && s < rows) {
        for (int l = 0; l < lv.n; ++l) {
#pragma unroll
            for (int a = 0; a < 3; ++a) lv.f_rgb[l][p * 3 + a] = lv.c_rgb[l][s * 3 + a];
            lv.f_dist[l][p] = lv.c_dist[l][s];
            lv.f_acc[l][p] = lv.c_acc[l][s];
        }
    } else {
        const float nv = nearp[p];
        for (int l = 0; l < lv.n; ++l) {
            lv.f_rgb[l][p * 3] = bkgd; lv.f_rgb[l][p * 3 + 1] = bkgd; lv.f_rgb[l][p * 3 + 2] = bkgd;
            lv.f_dist[l][p] = nv;
            lv.f_acc[l][p] = 0.0f;
        }
    }
}

hipError_t launch_gather_frame(int64_t n, int64_t rows, int num_levels, const int* slot, const float* nearp, int white_bkgd,
                               const float* const c_rgb[], const float* const c_dist[], const float* const c_acc[], float* const f_rgb[],
                               float* const f_dist[], float* const f_acc[], hipStream_t st) {
    GatherLevels lv;
    lv.n = num_levels;
    for (int l = 0; l < kMaxScatterLevels; ++l) {
        const bool on = l < num_levels;
        lv.c_rgb[l] = on ? c_rgb[l] : nullptr; lv.c_dist[l] = on ? c_dist[l] : nullptr; lv.c_acc[l] = on ? c_acc[l] : nullptr;
        lv.f_rgb[l] = on ? f_rgb[l] : nullptr; lv.f_dist[l] = on ? f_dist[l] : nullptr; lv.f_acc[l] = on ? f_acc[l] : nullptr;
    }
    hipLaunchKernelGGL(k_gather_frame, dim3(grid_for(n, 256)), dim3(256), 0, st, n, rows, slot, nearp, white_bkgd ? 1.0f : 0.0f, lv);
    return hipGetLastError();
}

}  // namespace mip
