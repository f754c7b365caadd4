// libmipnerf_preview_sparse.so: the baked preview over lattices that store only the rows next to an occupied cell
// (include/mipnerf_preview_sparse.h).  The storage rule is preview_sparse.hpp's; the march is the one kernel of preview_wave_march.hpp,
// instantiated here on PreviewSparsePyramid.  This unit adds the kernels that build the row table and fill the compact rows:
//   k_sparse_mask     one thread per table word: the stored bits from the cell words (sparse_point_word), and the block's popcount total
//   k_sparse_scan     ONE workgroup: the block totals become exclusive bases in place, in block order; the grand total is M
//   k_sparse_rank     the popcounts scanned exclusively over the block's threads, plus the block's base, give every word its rank
//   k_sparse_gather   dense rows -> their slots, 16 (degree 0: 8) bytes per thread
//   k_sparse_pack     per-stored-point values -> rows, preview_pack_row of preview_march.hpp
// The scan is the form of kernels_bucket.hip: block totals, one single-workgroup scan, apply.  No atomics: two runs give the same bytes.
// Compile with -ffp-contract=off (preview_march.hpp).
#include <hip/hip_runtime.h>

#include "preview_sparse.hpp"
#include "preview_wave_march.hpp"

namespace mip {

constexpr int kSpBlock = 256;          // table words per block of k_sparse_mask / k_sparse_rank
constexpr int kSpScanBlock = 1024;     // threads of the one workgroup of k_sparse_scan
constexpr int kSpScanPer = 4;          // block totals per thread and round

// workgroup-wide exclusive scan of one count per thread (WAVES * 64 threads), fixed order; `total`: the workgroup's sum
template <int WAVES>
__device__ __forceinline__ unsigned sp_block_scan(unsigned v, unsigned* s_wave, unsigned& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned is = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned o = __shfl_up(is, d, 64);
        if (lane >= d) is += o;
    }
    __syncthreads();                      // s_wave may still be read by an earlier call
    if (lane == 63) s_wave[wave] = is;
    __syncthreads();
    unsigned before = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
        const unsigned x = s_wave[w];
        if (w < wave) before += x;
        total += x;
    }
    return before + is - v;
}

// dims = (nx, ny, nz); table word t = (k * ny + j) * words_p + w
__global__ void __launch_bounds__(kSpBlock)
k_sparse_mask(const int64_t n_words, const int nx, const int ny, const int nz, const uint32_t* __restrict__ occ,
              SparseEntry* __restrict__ table, unsigned* __restrict__ block_sum) {
    __shared__ unsigned s_wave[kSpBlock / 64];
    const int64_t t = (int64_t)blockIdx.x * kSpBlock + threadIdx.x;
    uint32_t mask = 0u;
    if (t < n_words) {
        const int words_p = sparse_words_p(nx);
        const int64_t line = t / words_p;
        mask = sparse_point_word(occ, nx, ny, nz, (int)(line % ny), (int)(line / ny), (int)(t - line * words_p));
        table[t].mask = mask;
    }
    unsigned total;
    sp_block_scan<kSpBlock / 64>((unsigned)__popc(mask), s_wave, total);
    if (threadIdx.x == 0) block_sum[blockIdx.x] = total;
}

__global__ void __launch_bounds__(kSpScanBlock)
k_sparse_scan(const int64_t nblocks, unsigned* __restrict__ block_sum, int32_t* __restrict__ total_out) {
    __shared__ unsigned s_wave[kSpScanBlock / 64];
    unsigned run = 0;                                                     // uniform over the workgroup
    for (int64_t b0 = 0; b0 < nblocks; b0 += kSpScanBlock * kSpScanPer) {
        const int64_t b = b0 + (int64_t)threadIdx.x * kSpScanPer;
        unsigned v[kSpScanPer], s = 0;
#pragma unroll
        for (int r = 0; r < kSpScanPer; ++r) {
            v[r] = b + r < nblocks ? block_sum[b + r] : 0u;
            s += v[r];
        }
        unsigned total;
        unsigned ex = run + sp_block_scan<kSpScanBlock / 64>(s, s_wave, total);
#pragma unroll
        for (int r = 0; r < kSpScanPer; ++r) {
            if (b + r < nblocks) block_sum[b + r] = ex;
            ex += v[r];
        }
        run += total;
    }
    if (threadIdx.x == 0) *total_out = (int32_t)run;                      // M < 2^31: the lattice rule
}

__global__ void __launch_bounds__(kSpBlock)
k_sparse_rank(const int64_t n_words, const unsigned* __restrict__ block_sum, SparseEntry* __restrict__ table) {
    __shared__ unsigned s_wave[kSpBlock / 64];
    const int64_t t = (int64_t)blockIdx.x * kSpBlock + threadIdx.x;
    const uint32_t mask = t < n_words ? table[t].mask : 0u;
    unsigned total;
    const unsigned ex = sp_block_scan<kSpBlock / 64>((unsigned)__popc(mask), s_wave, total);
    if (t < n_words) table[t].rank = block_sum[blockIdx.x] + ex;
}

// one thread per chunk of a dense row: N halves, CH chunks per row (PreviewRowChunks)
template <int DEG>
__global__ void __launch_bounds__(256)
k_sparse_gather(const int64_t n_chunks, const int nx, const SparseEntry* __restrict__ table,
                const typename PreviewRowChunks<DEG>::Chunk* __restrict__ dense, typename PreviewRowChunks<DEG>::Chunk* __restrict__ rows) {
    constexpr int CH = PreviewRowChunks<DEG>::CH;
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= n_chunks) return;
    const int64_t point = q / CH, line = point / nx;
    const int i = (int)(point - line * nx);
    const SparseEntry e = table[line * sparse_words_p(nx) + (i >> 5)];
    if (!((e.mask >> (i & 31)) & 1u)) return;
    rows[sparse_slot(e, i) * CH + (q - point * CH)] = dense[q];
}

__global__ void __launch_bounds__(256)
k_sparse_pack(const int64_t n, const int degree, const float* __restrict__ sigma, const float* __restrict__ coef,
              uint16_t* __restrict__ rows) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    preview_pack_row(degree, sigma[i], coef + i * (3 * preview_basis(degree)), true, rows + i * preview_row_halves(degree));
}

int64_t sparse_index_blocks(const int32_t* dims) {
    const int64_t n_words = (int64_t)dims[2] * dims[1] * sparse_words_p(dims[0]);
    return (n_words + kSpBlock - 1) / kSpBlock;
}

hipError_t launch_sparse_index(const int32_t* dims, const uint32_t* occ, SparseEntry* table, int32_t* total, unsigned* block_sum,
                               hipStream_t stream) {
    const int64_t n_words = (int64_t)dims[2] * dims[1] * sparse_words_p(dims[0]), nb = sparse_index_blocks(dims);
    hipLaunchKernelGGL(k_sparse_mask, dim3((unsigned)nb), dim3(kSpBlock), 0, stream, n_words, dims[0], dims[1], dims[2], occ, table, block_sum);
    hipLaunchKernelGGL(k_sparse_scan, dim3(1), dim3(kSpScanBlock), 0, stream, nb, block_sum, total);
    hipLaunchKernelGGL(k_sparse_rank, dim3((unsigned)nb), dim3(kSpBlock), 0, stream, n_words, block_sum, table);
    return hipGetLastError();
}

template <int DEG>
static void gather(int64_t n_points, int nx, const SparseEntry* table, const void* dense, void* rows, hipStream_t stream) {
    typedef typename PreviewRowChunks<DEG>::Chunk Chunk;
    const int64_t n_chunks = n_points * PreviewRowChunks<DEG>::CH;
    hipLaunchKernelGGL(k_sparse_gather<DEG>, dim3((unsigned)((n_chunks + 255) / 256)), dim3(256), 0, stream, n_chunks, nx, table,
                       static_cast<const Chunk*>(dense), static_cast<Chunk*>(rows));
}

hipError_t launch_sparse_gather(const int32_t* dims, int degree, const SparseEntry* table, const void* dense, void* rows,
                                hipStream_t stream) {
    const int64_t n_points = (int64_t)dims[0] * dims[1] * dims[2];
    if (degree == 0) gather<0>(n_points, dims[0], table, dense, rows, stream);
    else if (degree == 1) gather<1>(n_points, dims[0], table, dense, rows, stream);
    else gather<2>(n_points, dims[0], table, dense, rows, stream);
    return hipGetLastError();
}

hipError_t launch_sparse_pack(int64_t n, int degree, const float* sigma, const float* coef, uint16_t* rows, hipStream_t stream) {
    hipLaunchKernelGGL(k_sparse_pack, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, n, degree, sigma, coef, rows);
    return hipGetLastError();
}

hipError_t launch_preview_sparse_march(const PreviewSparsePyramid& pyr, const PreviewMarch& p, float footprint, int degree, int64_t n_rays,
                                       const float* origins, const float* directions, const float* radii, const float* near,
                                       const float* far, float* rgb, float* acc, float* distance, int32_t* steps, float* lod,
                                       hipStream_t stream) {
    return launch_preview_wave_march(pyr, p, footprint, degree, n_rays, origins, directions, radii, near, far, rgb, acc, distance, steps, lod,
                                     stream);
}

}  // namespace mip
