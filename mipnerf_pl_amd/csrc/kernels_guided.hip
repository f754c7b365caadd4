// Error-guided batch sampling (gfx950, wave64): a running squared error per image tile, a mixture "uniform / proportional to error" over
// the tiles as an integer cdf, the draws, and the two per-step kernels of a training step.  The rule is stated in include/mipnerf_hip.h
// (mipnerf_guided_*); every sum that crosses cells is an integer sum, so two runs give the same bytes.
//   the table                    [n_images + 1][4] int64 rows (first cell, first pixel, W, H); the last row holds (n_cells, n_pixels, 0, 0).
//                                guided_cell() below is its one reading: cell -> image, tile origin and tile size;
//   k_guided_apply               one thread per ray: lossmult[i] *= weight[slot];
//   k_guided_accumulate          one thread per ray: fx = round(se * 2^24) added to sum[cell[slot]] (64-bit) and 1 to cnt (32-bit) with
//                                integer vector atomics on global memory: order-free, no float atomic anywhere;
//   k_guided_fold_mass           one thread per cell: the fold into err, sum = cnt = 0, a_c = n_c * round(err * 2^20); per block the integer
//                                totals of a_c and of the cells seen so far;
//   k_guided_totals              ONE workgroup: A and the visited-cell count from the block totals, into the header;
//   k_guided_mass_q              one thread per cell: q_c, and per block the total of q;
//   k_guided_scan_blocks         ONE workgroup: the block totals of q become exclusive bases in place (as many passes as needed), Q into the header;
//   k_guided_scan_apply          one thread per cell: cdf[c] = block base + inclusive scan of q inside the block;
//   k_guided_draw                one thread per draw: binary search of cdf, the image from the table, the pixel pick, the three stores.
// Kernels of one refresh talk through global memory ACROSS launches only: no workgroup reads what another wrote in the same launch.
// Bound: each is one pass over 4 .. 24 bytes per cell (or per draw) with a dependent binary search in the draw: latency- and HBM-bound,
// far off the step's critical path.  Every result leaves through ordinary vector stores or integer vector atomics.
#include <hip/hip_runtime.h>

#include "kernels.hpp"
#include "lane_buckets.hpp"

namespace mip {

constexpr int kGuidedBlock = 256;          // threads = cells (or rays, draws) per workgroup; also the width of one pass of the single-workgroup kernels

struct GuidedCell {
    int img;
    int64_t pix0;                          // first pixel of the image
    int W, x0, y0, w, h;                   // image width, tile origin, tile size (smaller at the right and bottom edges)
};

// cell c (0 <= c < n_cells) -> its image (the last one whose first cell is <= c) and tile
__device__ __forceinline__ GuidedCell guided_cell(const int64_t* __restrict__ table, int n_images, int T, int64_t c) {
    int lo = 0, hi = n_images - 1;         // invariant: table[lo].cell0 <= c < table[hi + 1].cell0
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (table[(int64_t)mid * 4] <= c) lo = mid; else hi = mid - 1;
    }
    const int64_t* row = table + (int64_t)lo * 4;
    GuidedCell g;
    g.img = lo;
    g.pix0 = row[1];
    g.W = (int)row[2];
    const int H = (int)row[3];
    const int tw = (g.W + T - 1) / T;
    const int64_t l = c - row[0];
    const int ty = (int)(l / tw), tx = (int)(l - (int64_t)ty * tw);
    g.x0 = tx * T;
    g.y0 = ty * T;
    g.w = g.W - g.x0 < T ? g.W - g.x0 : T;
    g.h = H - g.y0 < T ? H - g.y0 : T;
    return g;
}

// batch index of this launch: read on the device (b = *step - *epoch_base, as k_gather_train_batch) or given by the host
__device__ __forceinline__ int64_t guided_batch(const int64_t* __restrict__ step, const int64_t* __restrict__ epoch_base, int64_t host_batch) {
    return step ? *step - *epoch_base : host_batch;
}

__global__ void __launch_bounds__(kGuidedBlock)
k_guided_apply(int64_t B, int64_t n_order, int64_t ring, const float* __restrict__ weight, const int64_t* __restrict__ step,
               const int64_t* __restrict__ epoch_base, int64_t host_batch, float* __restrict__ lossmult) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B) return;
    const int64_t b = guided_batch(step, epoch_base, host_batch);
    if (b < 0) return;
    const int64_t j = b * B + i;
    if (j >= n_order) return;
    lossmult[i] = lossmult[i] * weight[j % ring];
}

__global__ void __launch_bounds__(kGuidedBlock)
k_guided_accumulate(int64_t B, int64_t n_order, int64_t ring, const int* __restrict__ cell, int64_t n_cells,
                    const int64_t* __restrict__ step, const int64_t* __restrict__ epoch_base, int64_t host_batch,
                    const float* __restrict__ rgb, const float* __restrict__ gt, unsigned long long* __restrict__ sum,
                    unsigned* __restrict__ cnt) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B) return;
    const int64_t b = guided_batch(step, epoch_base, host_batch);
    if (b < 0) return;
    const int64_t j = b * B + i;
    if (j >= n_order) return;
    const int64_t c = cell[j % ring];
    if (c < 0 || c >= n_cells) return;     // whatever the ring holds, the adds stay inside sum / cnt
    const float d0 = rgb[i * 3] - gt[i * 3], d1 = rgb[i * 3 + 1] - gt[i * 3 + 1], d2 = rgb[i * 3 + 2] - gt[i * 3 + 2];
    const float se = ((d0 * d0) + d1 * d1) + d2 * d2;      // the sef of k_loss_fused
    if (!(se >= 0.0f) || !(se <= 3.4028234663852886e38f)) return;      // not finite, or negative: not counted
    const unsigned long long fx = (unsigned long long)floor((double)se * 16777216.0 + 0.5);
    atomicAdd(sum + c, fx);
    atomicAdd(cnt + c, 1u);
}

// workgroup-wide sum of kGuidedBlock values, fixed order; s_red holds kGuidedBlock / 64 words.  Valid in every thread.
template <typename U>
__device__ __forceinline__ U guided_block_sum(U v, U* s_red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();                       // s_red may still be read by an earlier call
    if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
    __syncthreads();
    U t = 0;
#pragma unroll
    for (int w = 0; w < kGuidedBlock / 64; ++w) t += s_red[w];
    return t;
}

// workgroup-wide inclusive scan of kGuidedBlock 32-bit values, fixed order; `total` = the workgroup's sum
__device__ __forceinline__ unsigned guided_block_scan(unsigned v, unsigned* s_red, unsigned& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned o = __shfl_up(inc, d, 64);
        if (lane >= d) inc += o;
    }
    __syncthreads();
    if (lane == 63) s_red[wave] = inc;
    __syncthreads();
    unsigned before = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < kGuidedBlock / 64; ++w) {
        const unsigned x = s_red[w];
        if (w < wave) before += x;
        total += x;
    }
    return before + inc;
}

__device__ __forceinline__ unsigned long long guided_mass(float err, int n_c) {
    const unsigned long long ef = (unsigned long long)floor((double)err * 1048576.0 + 0.5);
    return (unsigned long long)n_c * ef;
}

__global__ void __launch_bounds__(kGuidedBlock)
k_guided_fold_mass(int64_t n_cells, int n_images, const int64_t* __restrict__ table, int T, float rate, float* __restrict__ err,
                   unsigned long long* __restrict__ sum, unsigned* __restrict__ cnt, unsigned char* __restrict__ seen,
                   unsigned long long* __restrict__ block_a, unsigned* __restrict__ block_seen) {
    __shared__ unsigned long long s_a[kGuidedBlock / 64];
    __shared__ unsigned s_v[kGuidedBlock / 64];
    const int64_t c = (int64_t)blockIdx.x * kGuidedBlock + threadIdx.x;
    unsigned long long a = 0;
    unsigned v = 0;
    if (c < n_cells) {
        float e = err[c];
        const unsigned n = cnt[c];
        v = seen[c] != 0;
        if (n > 0) {
            const float mean = (float)(((double)sum[c] / (double)n) * 5.9604644775390625e-08);      // 2^-24
            e = e + rate * (mean - e);
            err[c] = e;
            if (!v) { v = 1; seen[c] = 1; }
        }
        sum[c] = 0ull;
        cnt[c] = 0u;
        const GuidedCell g = guided_cell(table, n_images, T, c);
        a = guided_mass(e, g.w * g.h);
    }
    a = guided_block_sum(a, s_a);
    v = guided_block_sum(v, s_v);
    if (threadIdx.x == 0) { block_a[blockIdx.x] = a; block_seen[blockIdx.x] = v; }
}

// header: [0] Q, [1] A, [2] cells visited since the start, [3] n_cells
__global__ void __launch_bounds__(kGuidedBlock)
k_guided_totals(int64_t nblocks, int64_t n_cells, const unsigned long long* __restrict__ block_a, const unsigned* __restrict__ block_seen,
                unsigned long long* __restrict__ header) {
    __shared__ unsigned long long s_a[kGuidedBlock / 64];
    __shared__ unsigned long long s_v[kGuidedBlock / 64];
    unsigned long long a = 0, v = 0;
    for (int64_t b = threadIdx.x; b < nblocks; b += kGuidedBlock) { a += block_a[b]; v += block_seen[b]; }
    a = guided_block_sum(a, s_a);
    v = guided_block_sum(v, s_v);
    if (threadIdx.x == 0) { header[1] = a; header[2] = v; header[3] = (unsigned long long)n_cells; }
}

__global__ void __launch_bounds__(kGuidedBlock)
k_guided_mass_q(int64_t n_cells, int n_images, const int64_t* __restrict__ table, int T, double mix, const float* __restrict__ err,
                const unsigned long long* __restrict__ header, unsigned* __restrict__ q, unsigned* __restrict__ block_q) {
    __shared__ unsigned s_q[kGuidedBlock / 64];
    const int64_t c = (int64_t)blockIdx.x * kGuidedBlock + threadIdx.x;
    unsigned qc = 0;
    if (c < n_cells) {
        const unsigned long long A = header[1];
        const GuidedCell g = guided_cell(table, n_images, T, c);
        const int n_c = g.w * g.h;
        const double share = (double)n_c / (double)table[(int64_t)n_images * 4 + 1];
        const double prop = A > 0 ? (double)guided_mass(err[c], n_c) / (double)A : share;
        const double p = (1.0 - mix) * share + mix * prop;
        const unsigned long long f = (unsigned long long)floor(p * 1073741824.0);      // 2^30
        qc = f < 1ull ? 1u : (unsigned)f;
        q[c] = qc;
    }
    qc = guided_block_sum(qc, s_q);
    if (threadIdx.x == 0) block_q[blockIdx.x] = qc;
}

__global__ void __launch_bounds__(kGuidedBlock)
k_guided_scan_blocks(int64_t nblocks, unsigned* __restrict__ block_q, unsigned long long* __restrict__ header) {
    __shared__ unsigned s_red[kGuidedBlock / 64];
    unsigned run = 0;                      // uniform over the workgroup
    for (int64_t b0 = 0; b0 < nblocks; b0 += kGuidedBlock) {
        const int64_t b = b0 + threadIdx.x;
        const unsigned v = b < nblocks ? block_q[b] : 0u;
        unsigned total;
        const unsigned inc = guided_block_scan(v, s_red, total);
        if (b < nblocks) block_q[b] = run + inc - v;
        run += total;
    }
    if (threadIdx.x == 0) header[0] = (unsigned long long)run;
}

__global__ void __launch_bounds__(kGuidedBlock)
k_guided_scan_apply(int64_t n_cells, const unsigned* __restrict__ q, const unsigned* __restrict__ block_base, unsigned* __restrict__ cdf) {
    __shared__ unsigned s_red[kGuidedBlock / 64];
    const int64_t c = (int64_t)blockIdx.x * kGuidedBlock + threadIdx.x;
    const unsigned v = c < n_cells ? q[c] : 0u;
    unsigned total;
    const unsigned inc = guided_block_scan(v, s_red, total);
    if (c < n_cells) cdf[c] = block_base[blockIdx.x] + inc;
}

__global__ void __launch_bounds__(kGuidedBlock)
k_guided_draw(int64_t n, const int64_t* __restrict__ r, int n_images, const int64_t* __restrict__ table, int T, int64_t n_cells,
              const unsigned* __restrict__ cdf, const unsigned long long* __restrict__ header, int64_t* __restrict__ order,
              float* __restrict__ weight, int* __restrict__ cell, int64_t ring, int64_t ring_start) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const unsigned long long Q = header[0];
    const unsigned long long r0 = (unsigned long long)r[j] & 0xffffffffull, r1 = (unsigned long long)r[n + j] & 0xffffffffull;
    const unsigned long long t = (r0 * Q) >> 32;
    int64_t lo = 0, hi = n_cells - 1;      // the first cell with cdf[c] > t; cdf[n_cells - 1] = Q > t, and hi never leaves the table
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if ((unsigned long long)cdf[mid] > t) hi = mid; else lo = mid + 1;
    }
    const int64_t c = lo;
    const unsigned q = cdf[c] - (c > 0 ? cdf[c - 1] : 0u);
    const GuidedCell g = guided_cell(table, n_images, T, c);
    const int n_c = g.w * g.h;
    const int k = (int)((r1 * (unsigned long long)n_c) >> 32);
    const int ky = k / g.w, kx = k - ky * g.w;
    order[j] = g.pix0 + (int64_t)(g.y0 + ky) * g.W + (g.x0 + kx);
    const double share = (double)n_c / (double)table[(int64_t)n_images * 4 + 1];
    const int64_t slot = (ring_start + j) % ring;
    weight[slot] = (float)(share / ((double)q / (double)Q));
    cell[slot] = (int)c;
}

int64_t guided_num_blocks(int64_t n_cells) { return (n_cells + kGuidedBlock - 1) / kGuidedBlock; }

hipError_t launch_guided_apply(int64_t B, int64_t n_order, int64_t ring, const float* weight, const int64_t* step, const int64_t* epoch_base,
                               int64_t host_batch, float* lossmult, hipStream_t st) {
    hipLaunchKernelGGL(k_guided_apply, dim3(grid_for(B, kGuidedBlock)), dim3(kGuidedBlock), 0, st, B, n_order, ring, weight, step, epoch_base,
                       host_batch, lossmult);
    return hipGetLastError();
}

hipError_t launch_guided_accumulate(int64_t B, int64_t n_order, int64_t ring, const int* cell, int64_t n_cells, const int64_t* step,
                                    const int64_t* epoch_base, int64_t host_batch, const float* rgb, const float* gt,
                                    unsigned long long* sum, unsigned* cnt, hipStream_t st) {
    hipLaunchKernelGGL(k_guided_accumulate, dim3(grid_for(B, kGuidedBlock)), dim3(kGuidedBlock), 0, st, B, n_order, ring, cell, n_cells, step,
                       epoch_base, host_batch, rgb, gt, sum, cnt);
    return hipGetLastError();
}

// scratch: guided_num_blocks(n_cells) 64-bit words (the block totals of a), then as many 32-bit words twice (seen, q)
hipError_t launch_guided_refresh(int n_images, const int64_t* table, int T, int64_t n_cells, float rate, double mix, float* err,
                                 unsigned long long* sum, unsigned* cnt, unsigned char* seen, unsigned* q, unsigned* cdf,
                                 unsigned long long* scratch, unsigned long long* header, hipStream_t st) {
    const int64_t nb = guided_num_blocks(n_cells);
    unsigned long long* block_a = scratch;
    unsigned* block_seen = reinterpret_cast<unsigned*>(scratch + nb);
    unsigned* block_q = block_seen + nb;
    const dim3 grid((unsigned)nb), block(kGuidedBlock);
    hipLaunchKernelGGL(k_guided_fold_mass, grid, block, 0, st, n_cells, n_images, table, T, rate, err, sum, cnt, seen, block_a, block_seen);
    hipLaunchKernelGGL(k_guided_totals, dim3(1), block, 0, st, nb, n_cells, block_a, block_seen, header);
    hipLaunchKernelGGL(k_guided_mass_q, grid, block, 0, st, n_cells, n_images, table, T, mix, err, header, q, block_q);
    hipLaunchKernelGGL(k_guided_scan_blocks, dim3(1), block, 0, st, nb, block_q, header);
    hipLaunchKernelGGL(k_guided_scan_apply, grid, block, 0, st, n_cells, q, block_q, cdf);
    return hipGetLastError();
}

hipError_t launch_guided_draw(int64_t n, const int64_t* r, int n_images, const int64_t* table, int T, int64_t n_cells, const unsigned* cdf,
                              const unsigned long long* header, int64_t* order, float* weight, int* cell, int64_t ring, int64_t ring_start,
                              hipStream_t st) {
    hipLaunchKernelGGL(k_guided_draw, dim3(grid_for(n, kGuidedBlock)), dim3(kGuidedBlock), 0, st, n, r, n_images, table, T, n_cells, cdf,
                       header, order, weight, cell, ring, ring_start);
    return hipGetLastError();
}

}  // namespace mip
