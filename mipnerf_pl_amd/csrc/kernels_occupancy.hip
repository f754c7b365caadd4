// Empty-space skipping for whole frames (gfx950, wave64), compiled with -ffp-contract=off:
//   k_occ_raw / k_occ_dilate_*   occupancy bits of any fp32 lattice [nz, ny, nx]: one lane per cell, the wave's __ballot is two packed
//                                words; dilation as three separable passes on the packed words (shifts and ORs along x, word ORs along
//                                y and z);
//   k_lattice_decay_max          the lattice a training run keeps: running = max(decay * running, fresh) per point, 16-byte loads and
//                                stores, before the same bit passes;
//   k_ray_occupancy              one wavefront per ray: lanes take the coarse level's frusta lane, lane + 64, ..., test the cell range of
//                                each frustum's bounding box with word masks, the wave reduces with a ballot;
//   k_ray_span                   the same wave and the same per-frustum test: the smallest and the largest hitting frustum of a ray
//                                (lowest / highest set bit of a bucket's ballot) and their outer fence posts near', far';
//   k_ray_occupancy_360 / k_ray_span_360  the same two bodies for the unbounded-scene model and a grid laid out in contracted
//                                coordinates: inverse-depth fence posts, each frustum's image under contract() bounded by the closed
//                                form of raymath360.hpp (contracted_frustum_box);
//   k_compact_* / k_scatter_frame  exclusive scan of the live bytes (sums per 1024 rays + one single-workgroup scan + per-ray bases, the
//                                arrangement of kernels_mesh.hip), the live rays gathered in their order, and the way back: every pixel of
//                                every level written once.
// No atomics anywhere: two runs give the same bytes.  Every result leaves through ordinary vector stores.
#include <hip/hip_runtime.h>

#include "kernels.hpp"
#include "lane_buckets.hpp"
#include "raymath360.hpp"

namespace mip {

// cells (nx - 1, ny - 1, nz - 1), words per x row of cells
struct OccGrid {
    int cx, cy, cz;
    int wx;           // ceil(cx / 32)
};

static OccGrid occ_grid(const int dims[3]) {
    OccGrid g;
    g.cx = dims[0] - 1; g.cy = dims[1] - 1; g.cz = dims[2] - 1;
    g.wx = (g.cx + 31) / 32;
    return g;
}

// ------------------------------------------------------------------------------------------
// raw occupancy: cell (i, j, k) is occupied iff any of its 8 corner values is > thr or NaN
// ------------------------------------------------------------------------------------------
// One wave per 64 consecutive cells of an x row; 4 waves per workgroup.  Lanes past the row vote 0, which are the padding bits.
__global__ void __launch_bounds__(256)
k_occ_raw(OccGrid g, int nx, int ny, const float* __restrict__ f, float thr, unsigned* __restrict__ bits) {
    const int lane = threadIdx.x & 63;
    const int pairs = (g.wx + 1) >> 1;                                   // waves per row
    const int64_t wave = (int64_t)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    const int64_t rows = (int64_t)g.cy * g.cz;
    if (wave >= rows * pairs) return;                                    // wave-uniform
    const int row = (int)(wave / pairs), wp = (int)(wave - (int64_t)row * pairs);
    const int k = row / g.cy, j = row - k * g.cy;
    const int i = wp * 64 + lane;
    bool occ = false;
    if (i < g.cx) {
        const float* p = f + ((int64_t)k * ny + j) * nx + i;
        const int64_t sy = nx, sz = (int64_t)nx * ny;
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const float v = p[(c & 1) + ((c >> 1) & 1) * sy + ((c >> 2) & 1) * sz];
            occ = occ || !(v <= thr);                                    // > thr or NaN
        }
    }
    const unsigned long long m = __ballot(occ);
    unsigned* out = bits + (int64_t)row * g.wx + 2 * wp;
    if (lane == 0) out[0] = (unsigned)m;
    if (lane == 1 && 2 * wp + 1 < g.wx) out[1] = (unsigned)(m >> 32);
}

// bit i of the row shifted towards higher cells by s >= 1: word w of (row << s)
__device__ __forceinline__ unsigned occ_row_shl(const unsigned* __restrict__ row, int wx, int w, int s) {
    const int q = s >> 5, r = s & 31;
    const int a = w - q;
    unsigned v = a >= 0 ? row[a] << r : 0u;
    if (r && a - 1 >= 0) v |= row[a - 1] >> (32 - r);
    return v;
}
__device__ __forceinline__ unsigned occ_row_shr(const unsigned* __restrict__ row, int wx, int w, int s) {
    const int q = s >> 5, r = s & 31;
    const int a = w + q;
    unsigned v = a < wx ? row[a] >> r : 0u;
    if (r && a + 1 < wx) v |= row[a + 1] << (32 - r);
    return v;
}

// x pass: one thread per word; the padding bits of a row's last word stay 0
__global__ void __launch_bounds__(256)
k_occ_dilate_x(OccGrid g, int d, const unsigned* __restrict__ in, unsigned* __restrict__ out) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t total = (int64_t)g.cy * g.cz * g.wx;
    if (idx >= total) return;
    const int64_t rowi = idx / g.wx;
    const int w = (int)(idx - rowi * g.wx);
    const unsigned* row = in + rowi * g.wx;
    unsigned v = row[w];
    const int reach = d < g.cx ? d : g.cx;                               // a shift by the row's length or more brings nothing in
    for (int s = 1; s <= reach; ++s) v |= occ_row_shl(row, g.wx, w, s) | occ_row_shr(row, g.wx, w, s);
    const int last = g.cx - 32 * w;                                      // cells of this word
    if (last < 32) v &= (1u << last) - 1u;
    out[idx] = v;
}

// y (axis 1) and z (axis 2) passes: word ORs over the neighbours within d along the axis
__global__ void __launch_bounds__(256)
k_occ_dilate_axis(OccGrid g, int axis, int d, const unsigned* __restrict__ in, unsigned* __restrict__ out) {
    const int64_t idx = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t total = (int64_t)g.cy * g.cz * g.wx;
    if (idx >= total) return;
    const int64_t rowi = idx / g.wx;
    const int k = (int)(rowi / g.cy), j = (int)(rowi - (int64_t)k * g.cy);
    const int pos = axis == 1 ? j : k, n = axis == 1 ? g.cy : g.cz;
    const int64_t stride = axis == 1 ? (int64_t)g.wx : (int64_t)g.wx * g.cy;
    const int a = pos - d > 0 ? pos - d : 0, b = pos + d < n - 1 ? pos + d : n - 1;
    unsigned v = 0;
    for (int q = a; q <= b; ++q) v |= in[idx + (int64_t)(q - pos) * stride];
    out[idx] = v;
}

hipError_t launch_occupancy_build(const int dims[3], const float* f, float thr, int dilate, unsigned* bits, unsigned* scratch,
                                  hipStream_t st) {
    const OccGrid g = occ_grid(dims);
    const int64_t waves = (int64_t)g.cy * g.cz * ((g.wx + 1) / 2);
    const int64_t words = (int64_t)g.cy * g.cz * g.wx;
    unsigned* raw = dilate > 0 ? scratch : bits;
    hipLaunchKernelGGL(k_occ_raw, dim3(grid_for(waves, 4)), dim3(256), 0, st, g, dims[0], dims[1], f, thr, raw);
    if (dilate > 0) {
        const dim3 grid(grid_for(words, 256)), block(256);
        hipLaunchKernelGGL(k_occ_dilate_x, grid, block, 0, st, g, dilate, scratch, bits);
        hipLaunchKernelGGL(k_occ_dilate_axis, grid, block, 0, st, g, 1, dilate, bits, scratch);
        hipLaunchKernelGGL(k_occ_dilate_axis, grid, block, 0, st, g, 2, dilate, scratch, bits);
    }
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------
// a lattice that follows a field while it trains: running = max(decay * running, fresh), then the bits of it
// ------------------------------------------------------------------------------------------
// d = decay * r (one fp32 multiply); the new value is f where f > d or either is NaN, otherwise d: a NaN in `fresh` is kept, a NaN (or the
// 0 * inf of decay = 0) left in `running` is replaced
__device__ __forceinline__ float occ_decay_max(float f, float r, float decay) {
    const float d = decay * r;
    return (f > d || f != f || d != d) ? f : d;
}

// Elementwise, 12 B per point (two loads, one store).  Thread q takes points 4q .. 4q + 3 as one 16-byte load of each lattice and one
// 16-byte store (the launcher chooses vec4 = n / 4 when both lattices are 16-byte aligned, otherwise vec4 = 0); the n - 4 * vec4
// points of the tail go one per thread to the threads after them.
__global__ void __launch_bounds__(256)
k_lattice_decay_max(int64_t n, int64_t vec4, const float* __restrict__ fresh, float* __restrict__ running, float decay) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (q < vec4) {
        const float4 f = reinterpret_cast<const float4*>(fresh)[q];
        float4 r = reinterpret_cast<const float4*>(running)[q];
        r.x = occ_decay_max(f.x, r.x, decay);
        r.y = occ_decay_max(f.y, r.y, decay);
        r.z = occ_decay_max(f.z, r.z, decay);
        r.w = occ_decay_max(f.w, r.w, decay);
        reinterpret_cast<float4*>(running)[q] = r;
        return;
    }
    const int64_t p = 4 * vec4 + (q - vec4);
    if (p < n) running[p] = occ_decay_max(fresh[p], running[p], decay);
}

hipError_t launch_occupancy_refresh(const int dims[3], const float* fresh, float* running, float decay, float thr, int dilate,
                                    unsigned* bits, unsigned* scratch, hipStream_t st) {
    const int64_t n = (int64_t)dims[0] * dims[1] * dims[2];
    const bool aligned = (((uintptr_t)fresh | (uintptr_t)running) & 15) == 0;
    const int64_t vec4 = aligned ? n / 4 : 0;
    const int64_t threads = vec4 + (n - 4 * vec4);
    hipLaunchKernelGGL(k_lattice_decay_max, dim3(grid_for(threads, 256)), dim3(256), 0, st, n, vec4, fresh, running, decay);
    if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
    return launch_occupancy_build(dims, running, thr, dilate, bits, scratch, st);
}

// ------------------------------------------------------------------------------------------
// ray classification
// ------------------------------------------------------------------------------------------
struct OccBox {
    OccGrid g;
    float lo[3], h[3];
};

// floor((x - lo) / h) as an int in [-1, cells]: everything below the grid is -1, everything past it (and NaN) is `cells`
__device__ __forceinline__ int occ_cell(float x, float lo, float h, int cells) {
    const float c = floorf((x - lo) / h);
    if (c < 0.0f) return -1;
    if (!(c < (float)cells)) return cells;
    return (int)c;
}

// does the inclusive cell box [c0, c1] (inside the grid) hold an occupied bit?
__device__ __forceinline__ bool occ_box_test(const OccGrid& g, const unsigned* __restrict__ bits, const int c0[3], const int c1[3]) {
    const int w0 = c0[0] >> 5, w1 = c1[0] >> 5;
    const unsigned first = ~0u << (c0[0] & 31);
    const unsigned last = ~0u >> (31 - (c1[0] & 31));
    for (int k = c0[2]; k <= c1[2]; ++k) {
        for (int j = c0[1]; j <= c1[1]; ++j) {
            const unsigned* row = bits + ((int64_t)k * g.cy + j) * g.wx;
            for (int w = w0; w <= w1; ++w) {
                unsigned m = ~0u;
                if (w == w0) m &= first;
                if (w == w1) m &= last;
                if (row[w] & m) return true;
            }
        }
    }
    return false;
}

constexpr int kOccRaysPerBlock = 4;

// the ray of one wavefront: what every frustum test of it reads
struct OccRay {
    float o[3], d[3];
    float nv, fv, rr;     // near, far, cone_scale * radius
};

__device__ __forceinline__ OccRay occ_load_ray(int64_t b, const float* __restrict__ origins, const float* __restrict__ dirs,
                                               const float* __restrict__ radii, const float* __restrict__ nearp,
                                               const float* __restrict__ farp, float cone_scale) {
    OccRay r;
#pragma unroll
    for (int a = 0; a < 3; ++a) { r.o[a] = origins[b * 3 + a]; r.d[a] = dirs[b * 3 + a]; }
    r.nv = nearp[b]; r.fv = farp[b];
    r.rr = cone_scale * radii[b];
    return r;
}

// The per-frustum rules: which fence posts a ray's coarse level has and which per-axis interval, in the coordinates the grid is laid out
// in, holds frustum [t0, t1].  The cell test and both kernel bodies below are written once over a rule.
//   OccWorldRule   the bounded model: a grid in world coordinates, the frustum's own bounding box;
//   Occ360Rule     the unbounded-scene model: a grid in contracted coordinates, inverse-depth fence posts (those of k_sample_along_rays_360)
//                  and the box of raymath360.hpp contracted_frustum_box around the frustum's image under contract().
struct OccWorldRule {
    int disparity;
    __device__ __forceinline__ float post(const OccRay& r, int N, int i) const { return level0_t(r.nv, r.fv, N, i, disparity != 0); }
    __device__ __forceinline__ void bounds(const OccRay& r, float t0, float t1, float lo[3], float hi[3]) const {
        const float rho = r.rr * t1;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float p0 = r.o[a] + t0 * r.d[a], p1 = r.o[a] + t1 * r.d[a];
            lo[a] = fminf(p0, p1) - rho;
            hi[a] = fmaxf(p0, p1) + rho;
        }
    }
};
struct Occ360Rule {
    __device__ __forceinline__ float post(const OccRay& r, int N, int i) const { return level0_t_360(r.nv, r.fv, N, i); }
    __device__ __forceinline__ void bounds(const OccRay& r, float t0, float t1, float lo[3], float hi[3]) const {
        contracted_frustum_box(t0, t1, r.o, r.d, r.rr, lo, hi);
    }
};

// does coarse frustum i (i < N) of the ray touch an occupied cell?  The one statement of the predicate: both ray kernels call it.
template <class Rule>
__device__ __forceinline__ bool occ_frustum_hit(const OccBox& box, const unsigned* __restrict__ bits, const OccRay& r, int N, int i,
                                                const Rule& rule, int outside_occupied) {
    const int cells[3] = {box.g.cx, box.g.cy, box.g.cz};
    const float t0 = rule.post(r, N, i), t1 = rule.post(r, N, i + 1);
    float xlo[3], xhi[3];
    rule.bounds(r, t0, t1, xlo, xhi);
    int c0[3], c1[3];
    bool outside = false, empty = false;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        if (!(xlo[a] <= xhi[a])) outside = true;                         // a NaN ray is never culled
        c0[a] = occ_cell(xlo[a], box.lo[a], box.h[a], cells[a]);
        c1[a] = occ_cell(xhi[a], box.lo[a], box.h[a], cells[a]);
        if (c0[a] < 0 || c1[a] >= cells[a]) outside = true;
        if (c0[a] < 0) c0[a] = 0;
        if (c1[a] >= cells[a]) c1[a] = cells[a] - 1;
        if (c0[a] > c1[a]) empty = true;
    }
    if (outside && outside_occupied) return true;
    if (empty) return false;
    return occ_box_test(box.g, bits, c0, c1);
}

// the arguments the ray kernels share
struct OccRayArgs {
    int64_t B;
    int N;
    OccBox box;
    const unsigned* bits;
    const float *origins, *dirs, *radii, *nearp, *farp;
    int outside_occupied;
    float cone_scale;
    unsigned char* live;
    int *first, *last;              // k_ray_span only; each may be null
    float *near_out, *far_out;
};

// K = the sample-count bucket of the per-ray kernels (frusta per lane)
template <int K, class Rule>
__device__ __forceinline__ void ray_occupancy_body(const OccRayArgs& g, const Rule& rule) {
    const int lane = threadIdx.x & 63;
    const int64_t b = (int64_t)blockIdx.x * kOccRaysPerBlock + (threadIdx.x >> 6);
    if (b >= g.B) return;                                                // wave-uniform
    const int N = g.N;
    const OccRay r = occ_load_ray(b, g.origins, g.dirs, g.radii, g.nearp, g.farp, g.cone_scale);
    bool any = false;
    for (int kk = 0; kk < K; ++kk) {
        const int i = lane + 64 * kk;
        const bool hit = i < N && occ_frustum_hit(g.box, g.bits, r, N, i, rule, g.outside_occupied);
        if (__ballot(hit) != 0ull) { any = true; break; }                // wave-uniform
    }
    if (lane == 0) g.live[b] = any ? 1 : 0;
}

// The occupied span of a ray: the smallest and the largest hitting frustum and their outer fence posts.  The buckets are walked forward to
// the first one whose ballot is non-zero (a dead ray costs what it costs k_ray_occupancy), then backward from the last bucket that holds a
// frustum down to that one, whose ballot is kept: no bucket is tested twice.  Every branch on a ballot is wave-uniform.
template <int K, class Rule>
__device__ __forceinline__ void ray_span_body(const OccRayArgs& g, const Rule& rule) {
    const int lane = threadIdx.x & 63;
    const int64_t b = (int64_t)blockIdx.x * kOccRaysPerBlock + (threadIdx.x >> 6);
    if (b >= g.B) return;                                                // wave-uniform
    const int N = g.N;
    const OccRay r = occ_load_ray(b, g.origins, g.dirs, g.radii, g.nearp, g.farp, g.cone_scale);
    int fb = -1;                                                         // the first bucket with a hit and its ballot
    unsigned long long fm = 0ull;
    for (int kk = 0; kk < K; ++kk) {
        const int i = lane + 64 * kk;
        const bool hit = i < N && occ_frustum_hit(g.box, g.bits, r, N, i, rule, g.outside_occupied);
        const unsigned long long m = __ballot(hit);
        if (m != 0ull) { fb = kk; fm = m; break; }                       // wave-uniform
    }
    int fi = N, li = -1;
    if (fb >= 0) {                                                       // wave-uniform
        fi = 64 * fb + __builtin_ctzll(fm);
        int lb = fb;
        unsigned long long lm = fm;
        for (int kk = (N - 1) >> 6; kk > fb; --kk) {                     // (N - 1) >> 6 <= K - 1: the buckets past it hold no frustum
            const int i = lane + 64 * kk;
            const bool hit = i < N && occ_frustum_hit(g.box, g.bits, r, N, i, rule, g.outside_occupied);
            const unsigned long long m = __ballot(hit);
            if (m != 0ull) { lb = kk; lm = m; break; }                   // wave-uniform
        }
        li = 64 * lb + 63 - __builtin_clzll(lm);
    }
    if (lane == 0) {
        g.live[b] = fb >= 0 ? 1 : 0;
        if (g.first != nullptr) g.first[b] = fi;
        if (g.last != nullptr) g.last[b] = li;
        if (g.near_out != nullptr) g.near_out[b] = fb >= 0 ? rule.post(r, N, fi) : r.nv;
        if (g.far_out != nullptr) g.far_out[b] = fb >= 0 ? rule.post(r, N, li + 1) : r.fv;
    }
}

template <int K>
__global__ void __launch_bounds__(64 * kOccRaysPerBlock) k_ray_occupancy(OccRayArgs g, int disparity) {
    ray_occupancy_body<K>(g, OccWorldRule{disparity});
}
template <int K>
__global__ void __launch_bounds__(64 * kOccRaysPerBlock) k_ray_span(OccRayArgs g, int disparity) {
    ray_span_body<K>(g, OccWorldRule{disparity});
}
template <int K>
__global__ void __launch_bounds__(64 * kOccRaysPerBlock) k_ray_occupancy_360(OccRayArgs g) {
    ray_occupancy_body<K>(g, Occ360Rule{});
}
template <int K>
__global__ void __launch_bounds__(64 * kOccRaysPerBlock) k_ray_span_360(OccRayArgs g) {
    ray_span_body<K>(g, Occ360Rule{});
}

static OccBox occ_box(const int dims[3], const float lo[3], const float hi[3]) {
    OccBox box;
    box.g = occ_grid(dims);
    for (int a = 0; a < 3; ++a) {
        box.lo[a] = lo[a];
        box.h[a] = (hi[a] - lo[a]) / (float)(dims[a] - 1);
    }
    return box;
}

// one launcher for the four kernels: a.span chooses the body, a.contracted the rule
hipError_t launch_ray_classify(const RayClassify& a, hipStream_t st) {
    OccRayArgs g;
    g.B = a.B; g.N = a.N;
    g.box = occ_box(a.dims, a.lo, a.hi);
    g.bits = a.bits;
    g.origins = a.origins; g.dirs = a.dirs; g.radii = a.radii; g.nearp = a.nearp; g.farp = a.farp;
    g.outside_occupied = a.outside_occupied; g.cone_scale = a.cone_scale;
    g.live = a.live; g.first = a.first; g.last = a.last; g.near_out = a.near_out; g.far_out = a.far_out;
    const dim3 grid(grid_for(g.B, kOccRaysPerBlock)), block(64 * kOccRaysPerBlock);
    const bool ok = for_lane_bucket(a.N, [&](auto k) {
        if (a.contracted) {
            if (a.span) hipLaunchKernelGGL((k_ray_span_360<decltype(k)::value>), grid, block, 0, st, g);
            else hipLaunchKernelGGL((k_ray_occupancy_360<decltype(k)::value>), grid, block, 0, st, g);
        } else {
            if (a.span) hipLaunchKernelGGL((k_ray_span<decltype(k)::value>), grid, block, 0, st, g, a.disparity);
            else hipLaunchKernelGGL((k_ray_occupancy<decltype(k)::value>), grid, block, 0, st, g, a.disparity);
        }
    });
    return ok ? hipGetLastError() : hipErrorInvalidValue;
}

// ------------------------------------------------------------------------------------------
// compaction: exclusive scan of the live bytes, gather in order
// ------------------------------------------------------------------------------------------
constexpr int kCmpBlock = 256;
constexpr int kCmpPer = 4;              // consecutive rays per thread: one 4-byte load of live bytes
constexpr int kCmpTile = kCmpBlock * kCmpPer;
constexpr int kCmpScanBlock = 1024;

// workgroup-wide exclusive scan (WAVES * 64 threads; s_wave holds WAVES words): a becomes its exclusive prefix, total the sum.
// Fixed order: the same inputs give the same outputs.
template <int WAVES>
__device__ __forceinline__ void cmp_block_scan(unsigned& a, unsigned* s_wave, unsigned& total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned ia = a;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned oa = __shfl_up(ia, d, 64);
        if (lane >= d) ia += oa;
    }
    __syncthreads();                      // s_wave may still be read by an earlier call
    if (lane == 63) s_wave[wave] = ia;
    __syncthreads();
    unsigned base = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
        const unsigned x = s_wave[w];
        if (w < wave) base += x;
        total += x;
    }
    a = base + ia - a;
}

// the live flags of rays p0 .. p0 + 3 as bits 0 .. 3
__device__ __forceinline__ unsigned cmp_flags(const unsigned char* __restrict__ live, int64_t p0, int64_t n) {
    unsigned fl = 0;
    if (p0 + kCmpPer <= n) {
        const unsigned packed = *reinterpret_cast<const unsigned*>(live + p0);     // p0 is a multiple of 4, live 4-byte aligned
#pragma unroll
        for (int r = 0; r < kCmpPer; ++r) fl |= ((packed >> (8 * r)) & 0xffu) ? 1u << r : 0u;
    } else {
        for (int r = 0; p0 + r < n; ++r) fl |= live[p0 + r] ? 1u << r : 0u;
    }
    return fl;
}

__global__ void __launch_bounds__(kCmpBlock)
k_compact_count(int64_t n, const unsigned char* __restrict__ live, unsigned* __restrict__ block_sum) {
    __shared__ unsigned s_wave[kCmpBlock / 64];
    const int64_t p0 = ((int64_t)blockIdx.x * kCmpBlock + threadIdx.x) * kCmpPer;
    unsigned c = p0 < n ? __popc(cmp_flags(live, p0, n)) : 0u, total;
    cmp_block_scan<kCmpBlock / 64>(c, s_wave, total);
    if (threadIdx.x == 0) block_sum[blockIdx.x] = total;
}

// ONE workgroup turns the block sums into exclusive block bases in place, in index order; *total = the live count
__global__ void __launch_bounds__(kCmpScanBlock)
k_compact_scan_blocks(int nblocks, unsigned* __restrict__ block_sum, unsigned long long* __restrict__ total) {
    __shared__ unsigned s_wave[kCmpScanBlock / 64];
    unsigned run = 0;
    for (int b0 = 0; b0 < nblocks; b0 += kCmpScanBlock * kCmpPer) {
        const int b = b0 + threadIdx.x * kCmpPer;
        unsigned v[kCmpPer], s = 0;
#pragma unroll
        for (int r = 0; r < kCmpPer; ++r) {
            v[r] = b + r < nblocks ? block_sum[b + r] : 0u;
            s += v[r];
        }
        unsigned t;
        cmp_block_scan<kCmpScanBlock / 64>(s, s_wave, t);
#pragma unroll
        for (int r = 0; r < kCmpPer; ++r) {
            if (b + r < nblocks) block_sum[b + r] = run + s;
            s += v[r];
        }
        run += t;
    }
    if (threadIdx.x == 0) *total = (unsigned long long)run;
}

struct RaySoA {
    const float* in[7];
    float* out[7];
};

// per-ray bases, then the live rays and their source indices at their compact slots
__global__ void __launch_bounds__(kCmpBlock)
k_compact_gather(int64_t n, const unsigned char* __restrict__ live, const unsigned* __restrict__ block_base, RaySoA rays,
                 int* __restrict__ out_index) {
    __shared__ unsigned s_wave[kCmpBlock / 64];
    const int64_t p0 = ((int64_t)blockIdx.x * kCmpBlock + threadIdx.x) * kCmpPer;
    const unsigned fl = p0 < n ? cmp_flags(live, p0, n) : 0u;
    unsigned c = __popc(fl), total;
    cmp_block_scan<kCmpBlock / 64>(c, s_wave, total);
    if (fl == 0) return;
    int64_t slot = (int64_t)block_base[blockIdx.x] + c;
#pragma unroll
    for (int r = 0; r < kCmpPer; ++r) {
        if (!((fl >> r) & 1u)) continue;
        const int64_t p = p0 + r;
        out_index[slot] = (int)p;
#pragma unroll
        for (int q = 0; q < 3; ++q) {                                    // origins, directions, viewdirs [n, 3]
            if (rays.out[q] == nullptr) continue;
#pragma unroll
            for (int a = 0; a < 3; ++a) rays.out[q][slot * 3 + a] = rays.in[q][p * 3 + a];
        }
#pragma unroll
        for (int q = 3; q < 7; ++q)                                      // radii, lossmult, near, far [n, 1]
            if (rays.out[q] != nullptr) rays.out[q][slot] = rays.in[q][p];
        ++slot;
    }
}

int64_t compact_num_blocks(int64_t n) { return (n + kCmpTile - 1) / kCmpTile; }

hipError_t launch_compact_rays(int64_t n, const unsigned char* live, const float* const in[7], float* const out[7], int* out_index,
                               unsigned* block_sum, unsigned long long* total, hipStream_t st) {
    const int64_t nb = compact_num_blocks(n);
    RaySoA rays;
    for (int q = 0; q < 7; ++q) { rays.in[q] = in[q]; rays.out[q] = out[q]; }
    hipLaunchKernelGGL(k_compact_count, dim3((unsigned)nb), dim3(kCmpBlock), 0, st, n, live, block_sum);
    hipLaunchKernelGGL(k_compact_scan_blocks, dim3(1), dim3(kCmpScanBlock), 0, st, (int)nb, block_sum, total);
    hipLaunchKernelGGL(k_compact_gather, dim3((unsigned)nb), dim3(kCmpBlock), 0, st, n, live, block_sum, rays, out_index);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------
// scatter: every pixel of every level is written once
// ------------------------------------------------------------------------------------------
struct ScatterLevels {
    int n;
    const float* c_rgb[kMaxScatterLevels];
    const float* c_dist[kMaxScatterLevels];
    const float* c_acc[kMaxScatterLevels];
    float* f_rgb[kMaxScatterLevels];
    float* f_dist[kMaxScatterLevels];
    float* f_acc[kMaxScatterLevels];
};

// Thread p does two independent things: a dead pixel p takes the values of a ray with all-zero weights; compact slot p (p < count)
// goes to its source pixel.  The two sets of pixels are disjoint and cover the frame.
__global__ void __launch_bounds__(256)
k_scatter_frame(int64_t n, int64_t count, const int* __restrict__ index, const unsigned char* __restrict__ live,
                const float* __restrict__ nearp, float bkgd, ScatterLevels lv) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= n) return;
    if (!live[p]) {
        const float nv = nearp[p];
        for (int l = 0; l < lv.n; ++l) {
            lv.f_rgb[l][p * 3] = bkgd; lv.f_rgb[l][p * 3 + 1] = bkgd; lv.f_rgb[l][p * 3 + 2] = bkgd;
            lv.f_dist[l][p] = nv;
            lv.f_acc[l][p] = 0.0f;
        }
    }
    if (p < count) {
        const int64_t dst = index[p];
        for (int l = 0; l < lv.n; ++l) {
#pragma unroll
            for (int a = 0; a < 3; ++a) lv.f_rgb[l][dst * 3 + a] = lv.c_rgb[l][p * 3 + a];
            lv.f_dist[l][dst] = lv.c_dist[l][p];
            lv.f_acc[l][dst] = lv.c_acc[l][p];
        }
    }
}

hipError_t launch_scatter_frame(int64_t n, int64_t count, int num_levels, const int* index, const unsigned char* live, const float* nearp,
                                int white_bkgd, const float* const c_rgb[], const float* const c_dist[], const float* const c_acc[],
                                float* const f_rgb[], float* const f_dist[], float* const f_acc[], hipStream_t st) {
    ScatterLevels lv;
    lv.n = num_levels;
    for (int l = 0; l < kMaxScatterLevels; ++l) {
        const bool on = l < num_levels;
        lv.c_rgb[l] = on ? c_rgb[l] : nullptr; lv.c_dist[l] = on ? c_dist[l] : nullptr; lv.c_acc[l] = on ? c_acc[l] : nullptr;
        lv.f_rgb[l] = on ? f_rgb[l] : nullptr; lv.f_dist[l] = on ? f_dist[l] : nullptr; lv.f_acc[l] = on ? f_acc[l] : nullptr;
    }
    hipLaunchKernelGGL(k_scatter_frame, dim3(grid_for(n, 256)), dim3(256), 0, st, n, count, index, live, nearp,
                       white_bkgd ? 1.0f : 0.0f, lv);
    return hipGetLastError();
}

}  // namespace mip
