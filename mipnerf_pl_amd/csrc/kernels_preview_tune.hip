// libmipnerf_preview_tune.so (include/mipnerf_preview_tune.h): fine-tuning the baked lattice through its own renderer.
//   k_preview_tune_grad   the march of one dense lattice AND its gradient with respect to the rows, one launch
//   k_preview_tune_adam   the Adam step on the fp32 master rows and their repack to fp16, one pass
// The per-sample arithmetic is preview_march.hpp's (forward) and preview_tune.hpp's (rules 8 - 10, the Adam rule); this file spreads it
// over lanes.  Compile with -ffp-contract=off (preview_march.hpp).
//
// THE GRADIENT KERNEL.  ONE WAVEFRONT PER RAY, 4 rays per 256-thread block: the mapping of k_preview_wave_march (preview_wave_march.hpp).
//   SWEEP A is that march on one lattice, with the same calls in the same order (tune_block below is one 64-sample block of it), so rgb
//     and acc are mipnerf_preview_march's, bit for bit.  It yields G (from grad_rgb, or from the ray's own rgb in target mode) and
//     total = sum_i w_i q_i.  A ray that misses, a ray with G = 0 and g_a = 0 and a ray with a non-finite output or G ends here.
//   SWEEP B revisits the ray's blocks (their rows are cache-hot).  tune_block recomputes alpha, colour and the scans, so T_{i+1} is the
//     inclusive product scan and S_i = total - (inclusive sum scan of w q); each lane (= sample) forms d row[0] and the three
//     w G_c of rule 9 (d row[1 + 3k + c] is that times Y_k, and Y is the ray's: it needs no broadcast).
//   THE SCATTER IS TRANSPOSED: for the adds, lanes stop being samples and become DESTINATIONS.  The wave walks the block's counted samples
//     in order (a wave-uniform loop over the ballot); the sample's cell, fractions and the four numbers above are broadcast with readlane;
//     every lane owns one element of one corner row on one or more of the cell's four x-lines (y, z), (y + 1, z), (y, z + 1), (y + 1, z + 1).
//     On a line the low-x and the high-x corner rows are consecutive in memory: 2 W floats.
//         degree 1: 128 B per line; a wave instruction covers the two y-lines of one z   -> 2 atomic instructions per flush
//         degree 2: 256 B per line; one instruction each                                  -> 4 atomic instructions per flush
//         degree 0:  32 B per line; lanes 0 .. 31 cover all four lines, 32 .. 63 idle      -> 1 atomic instruction per flush
//     These are the shapes global float atomics run at full rate with (256 contiguous bytes, or two 128-byte segments in two rows); a lane
//     per sample, 64 rows per instruction, is an order of magnitude slower.  Lanes of pad elements stay inactive.
//   RUN COMBINING: consecutive counted samples of a ray in the same cell are summed in the lane's slot registers and flushed as one set of
//     adds when the cell changes and at the ray's end, across block boundaries too.
// The adds are plain atomicAdd(float*), return value unused.  Adds into one destination arrive in no fixed order across rays: two runs
// may differ in the last bits.  No LDS, no inline assembly.
#include <hip/hip_runtime.h>

#include "preview_tune.hpp"
#include "preview_wave_march.hpp"

namespace mip {

// what one 64-sample block of the march leaves in a lane
template <int DEG>
struct TuneBlock {
    int c[3];
    float fr[3];
    float row0;              // the blended row's density entry before its clamp
    float alpha, colour[3];
    float t, incl, excl;     // the sample's distance; the inclusive / exclusive product of (1 - alpha) inside the block
    bool exists, counted;    // counted: evaluated and not behind the early stop
    unsigned long long live; // the ballot of the occupied samples (0: the block loaded nothing and none of the above but `exists` is set)
    bool stop;               // wave-uniform: the early stop lies in this block
};

// one block of k_preview_wave_march on one lattice: the same calls in the same order
template <int DEG>
__device__ __forceinline__ void tune_block(const PreviewField& f, const PreviewMarch& p, const PreviewRay& r, const float o[3], const float d[3],
                                           const float (&Y)[(DEG + 1) * (DEG + 1)], int base, int lane, float carried, TuneBlock<DEG>* b) {
    constexpr int W = preview_row_halves(DEG);
    const int i = base + lane;
    const float t = preview_sample_t(r, i);
    b->t = t;
    b->exists = i < p.max_steps && t < r.tb;
    const float x[3] = {o[0] + t * d[0], o[1] + t * d[1], o[2] + t * d[2]};
    b->c[0] = b->c[1] = b->c[2] = 0;
    b->fr[0] = b->fr[1] = b->fr[2] = 0.0f;
    bool bit = false;
    if (b->exists) {
        lattice_cell(f.box, x, b->c, b->fr);                 // finite: o, d and t are
        bit = preview_occupied(f, b->c);
    }
    const bool occupied = b->exists && bit;
    b->live = __ballot(occupied);
    b->counted = false;
    b->stop = false;
    b->alpha = 0.0f;
    b->colour[0] = b->colour[1] = b->colour[2] = 0.0f;
    b->row0 = 0.0f;
    b->incl = b->excl = 1.0f;
    if (b->live == 0ull) return;
    float row[W];
#pragma unroll
    for (int e = 0; e < W; ++e) row[e] = 0.0f;
    if (occupied) {
        preview_row<DEG>(f, b->c, b->fr, row);
        preview_shade<DEG>(row, Y, p.s, &b->alpha, b->colour);
    }
    b->row0 = row[0];
    b->incl = wave_incl_prod_dpp(1.0f - b->alpha);
    b->excl = dpp_f32<kDppWaveShr1, 0xf>(1.0f, b->incl);
    const unsigned long long stop = __ballot(carried * b->incl < p.t_min);
    b->counted = occupied;
    if (stop != 0ull) {
        const int first = __builtin_ctzll(stop);
        b->counted = occupied && lane <= first;
        b->live &= first == 63 ? ~0ull : (2ull << first) - 1ull;
        b->stop = true;
    }
}

__device__ __forceinline__ float bcast(float v, int src) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src)); }
__device__ __forceinline__ int bcast(int v, int src) { return __builtin_amdgcn_readlane(v, src); }

// how the 8 corner rows of a cell are spread over the lanes of a flush (see the top of this file)
template <int DEG>
struct TuneSlots {
    static constexpr int W = preview_row_halves(DEG);
    static constexpr int N = DEG == 0 ? 1 : DEG == 1 ? 2 : 4;            // atomic instructions per flush = slot registers per lane
    // the lane's element of a row, its x corner, and the (y, z) corner of its slot j
    __device__ static int element(int lane) { return lane & (W - 1); }
    __device__ static int xcorner(int lane) { return (lane / W) & 1; }
    __device__ static int ycorner(int lane, int j) { return DEG == 0 ? (lane >> 3) & 1 : DEG == 1 ? lane >> 5 : j & 1; }
    __device__ static int zcorner(int lane, int j) { return DEG == 0 ? (lane >> 4) & 1 : DEG == 1 ? j : j >> 1; }
    __device__ static bool active(int lane) { return (DEG != 0 || lane < 32) && element(lane) < tune_row_used(DEG); }
};

// `counters` (optional): [0] += the samples that added something, [1] += the flushes (each is TuneSlots::N atomic instructions)
template <int DEG>
__global__ void __launch_bounds__(64 * kPreviewRaysPerBlock)
k_preview_tune_grad(const PreviewField f, const PreviewMarch p, const int64_t n_rays, const float* __restrict__ origins,
                    const float* __restrict__ directions, const float* __restrict__ near, const float* __restrict__ far,
                    const float* __restrict__ grad_rgb, const float* __restrict__ target, const float loss_scale,
                    const float* __restrict__ grad_acc, float* __restrict__ rgb, float* __restrict__ acc, float* __restrict__ grad_rows,
                    unsigned long long* __restrict__ counters) {
    typedef TuneSlots<DEG> Slots;
    constexpr int W = preview_row_halves(DEG), NB = preview_basis(DEG), NS = Slots::N;
    const int lane = threadIdx.x & 63;
    const int64_t ray = (int64_t)blockIdx.x * kPreviewRaysPerBlock + (threadIdx.x >> 6);
    if (ray >= n_rays) return;                                   // wave-uniform
    const float o[3] = {origins[3 * ray], origins[3 * ray + 1], origins[3 * ray + 2]};
    const float d[3] = {directions[3 * ray], directions[3 * ray + 1], directions[3 * ray + 2]};
    const float tn = near[ray], tf = far[ray];                   // wave-uniform
    PreviewRay r;
    if (!preview_ray(f, p.s, o, d, tn, tf, &r)) {                // wave-uniform: a miss adds nothing
        if (lane == 0) {
            rgb[3 * ray] = p.background[0]; rgb[3 * ray + 1] = p.background[1]; rgb[3 * ray + 2] = p.background[2];
            acc[ray] = 0.0f;
        }
        return;
    }
    float Y[NB];
    preview_sh_basis<DEG>(r.u, Y);

    // ---- sweep A: the march ----
    TuneBlock<DEG> b;
    float carried = 1.0f;
    float sr = 0.0f, sg = 0.0f, sb = 0.0f, sa = 0.0f;
    for (int base = 0; base < p.max_steps; base += 64) {
        tune_block<DEG>(f, p, r, o, d, Y, base, lane, carried, &b);
        if (b.live != 0ull) {
            if (b.counted) {
                const float w = (carried * b.excl) * b.alpha;
                sr += w * b.colour[0];
                sg += w * b.colour[1];
                sb += w * b.colour[2];
                sa += w;
            }
            if (b.stop) break;
            carried = carried * readlane63(b.incl);
        }
        if (__ballot(b.exists) != ~0ull) break;                  // the ray's last block
    }
    sr = wave_sum(sr); sg = wave_sum(sg); sb = wave_sum(sb); sa = wave_sum(sa);
    const float rest = 1.0f - sa;
    const float out[3] = {sr + rest * p.background[0], sg + rest * p.background[1], sb + rest * p.background[2]};
    if (lane == 0) {
        rgb[3 * ray] = out[0]; rgb[3 * ray + 1] = out[1]; rgb[3 * ray + 2] = out[2];
        acc[ray] = sa;
    }
    float G[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) G[c] = grad_rgb ? grad_rgb[3 * ray + c] : tune_target_grad(loss_scale, out[c], target[3 * ray + c]);
    const float g_a = grad_acc ? grad_acc[ray] : 0.0f;
    if (!tune_ray_ok(out, sa, G, g_a)) return;                   // wave-uniform
    if (G[0] == 0.0f && G[1] == 0.0f && G[2] == 0.0f && g_a == 0.0f) return;      // every term of rule 9 is a multiple of G or g_a
    const float sc[3] = {sr, sg, sb};
    const float total = tune_total(G, g_a, sc, sa, p.background);

    // ---- sweep B: d row per sample, scattered transposed ----
    // this lane as a destination: its element of the row and what it takes from a broadcast sample
    const int el = Slots::element(lane);
    const bool active = Slots::active(lane);
    float ysel = 0.0f;                                           // Y_k of this lane's element (1 for the density entry)
    int ch = 0;                                                  // and its channel
    if (el == 0) {
        ysel = 1.0f;
    } else {
#pragma unroll
        for (int k = 0; k < NB; ++k)
#pragma unroll
            for (int c = 0; c < 3; ++c)
                if (el == 1 + 3 * k + c) { ysel = Y[k]; ch = c; }
    }
    const int xc = Slots::xcorner(lane);
    const int64_t line_y = (int64_t)f.box.nx * W, line_z = line_y * f.box.ny;      // in floats
    int64_t slot_off[NS];                                        // this lane's float offset from the cell's low corner row, per slot
#pragma unroll
    for (int j = 0; j < NS; ++j) slot_off[j] = Slots::ycorner(lane, j) * line_y + Slots::zcorner(lane, j) * line_z + lane % (2 * W);
    float slot[NS];
#pragma unroll
    for (int j = 0; j < NS; ++j) slot[j] = 0.0f;
    int cur = -1;                                                // the cell whose sums the slots hold (wave-uniform); its low corner's row index
    unsigned long long n_samples = 0ull, n_flushes = 0ull;

    carried = 1.0f;
    float before = 0.0f;                                         // sum of w q over the blocks before this one
    for (int base = 0; base < p.max_steps; base += 64) {
        tune_block<DEG>(f, p, r, o, d, Y, base, lane, carried, &b);
        if (b.live != 0ull) {
            const float w = b.counted ? (carried * b.excl) * b.alpha : 0.0f;
            const float q = tune_q(G, g_a, b.colour, p.background);
            const float wq = b.counted ? w * q : 0.0f;
            const float upto = before + wave_incl_scan_dpp(wq);                    // sum_{j <= i} w_j q_j
            const float ds = tune_d_sigma(p.s, carried * b.incl, q, total - upto, b.row0);
            const float dc[3] = {tune_d_colour(w, G[0], b.colour[0]), tune_d_colour(w, G[1], b.colour[1]), tune_d_colour(w, G[2], b.colour[2])};
            const int cell = (b.c[2] * f.box.ny + b.c[1]) * f.box.nx + b.c[0];     // < nx ny nz < 2^31 / 7
            unsigned long long todo = __ballot(b.counted);
            n_samples += __popcll(todo);
            while (todo != 0ull) {                               // wave-uniform: the counted samples in order
                const int src = __builtin_ctzll(todo);
                todo &= todo - 1ull;
                const int s_cell = bcast(cell, src);
                if (s_cell != cur) {
                    if (cur >= 0) {
                        if (active) {
#pragma unroll
                            for (int j = 0; j < NS; ++j) atomicAdd(grad_rows + ((int64_t)cur * W + slot_off[j]), slot[j]);
                        }
                        ++n_flushes;
                    }
                    cur = s_cell;
#pragma unroll
                    for (int j = 0; j < NS; ++j) slot[j] = 0.0f;
                }
                const float s_fr[3] = {bcast(b.fr[0], src), bcast(b.fr[1], src), bcast(b.fr[2], src)};
                const float s_ds = bcast(ds, src), s_dc0 = bcast(dc[0], src), s_dc1 = bcast(dc[1], src), s_dc2 = bcast(dc[2], src);
                const float value = el == 0 ? s_ds : (ch == 0 ? s_dc0 : ch == 1 ? s_dc1 : s_dc2) * ysel;
#pragma unroll
                for (int j = 0; j < NS; ++j) slot[j] += tune_corner_weight(s_fr, xc, Slots::ycorner(lane, j), Slots::zcorner(lane, j)) * value;
            }
            if (b.stop) break;
            carried = carried * readlane63(b.incl);
            before = readlane63(upto);
        }
        if (__ballot(b.exists) != ~0ull) break;
    }
    if (cur >= 0) {
        if (active) {
#pragma unroll
            for (int j = 0; j < NS; ++j) atomicAdd(grad_rows + ((int64_t)cur * W + slot_off[j]), slot[j]);
        }
        ++n_flushes;
    }
    if (counters != nullptr && lane == 0) {
        atomicAdd(counters, n_samples);
        atomicAdd(counters + 1, n_flushes);
    }
}

hipError_t launch_preview_tune_grad(const PreviewField& f, const PreviewMarch& p, int degree, int64_t n_rays, const float* origins,
                                    const float* directions, const float* near, const float* far, const float* grad_rgb, const float* target,
                                    float loss_scale, const float* grad_acc, float* rgb, float* acc, float* grad_rows,
                                    unsigned long long* counters, hipStream_t stream) {
    const auto kernel = degree == 0 ? k_preview_tune_grad<0> : degree == 1 ? k_preview_tune_grad<1> : k_preview_tune_grad<2>;
    const dim3 grid((unsigned)((n_rays + kPreviewRaysPerBlock - 1) / kPreviewRaysPerBlock)), block(64 * kPreviewRaysPerBlock);
    hipLaunchKernelGGL(kernel, grid, block, 0, stream, f, p, n_rays, origins, directions, near, far, grad_rgb, target, loss_scale, grad_acc, rgb,
                       acc, grad_rows, counters);
    return hipGetLastError();
}

// ---- the optimiser step ------------------------------------------------------------------------------------------------------------
// One thread per 4 consecutive entries of a point: 16-byte loads and stores of master, m, v and grad, 8 bytes of fp16 rows; a grid-stride
// loop.  Chunks that hold padding only are skipped; in a chunk that ends in padding the pad entries are written back as they were read.
template <int DEG>
__global__ void __launch_bounds__(256)
k_preview_tune_adam(const int64_t n_points, const TuneAdam a, float* __restrict__ master, float* __restrict__ m, float* __restrict__ v,
                    float* __restrict__ grad, uint16_t* __restrict__ rows, const uint8_t* __restrict__ mask) {
    constexpr int W = preview_row_halves(DEG), CH = W / 4, USED = tune_row_used(DEG), LIVE = (USED + 3) / 4;      // chunks with a used entry
    const int64_t n_chunks = n_points * LIVE, stride = (int64_t)gridDim.x * 256;
    for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < n_chunks; k += stride) {
        const int64_t point = k / LIVE;
        const int chunk = (int)(k - point * LIVE);
        const int64_t at = point * CH + chunk;                   // in float4 / HalfChunk<4>
        float4 g4 = reinterpret_cast<float4*>(grad)[at];
        float* g = reinterpret_cast<float*>(&g4);
        if (mask != nullptr && mask[point] == 0) {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (chunk * 4 + e < USED) g[e] = 0.0f;
            reinterpret_cast<float4*>(grad)[at] = g4;
            continue;
        }
        float4 p4 = reinterpret_cast<float4*>(master)[at], m4 = reinterpret_cast<float4*>(m)[at], v4 = reinterpret_cast<float4*>(v)[at];
        HalfChunk<4> h4 = reinterpret_cast<HalfChunk<4>*>(rows)[at];
        float *pp = reinterpret_cast<float*>(&p4), *mm = reinterpret_cast<float*>(&m4), *vv = reinterpret_cast<float*>(&v4);
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (chunk * 4 + e < USED) tune_adam_element(a, chunk * 4 + e, pp + e, mm + e, vv + e, g + e, &h4.h[e]);
        reinterpret_cast<float4*>(master)[at] = p4;
        reinterpret_cast<float4*>(m)[at] = m4;
        reinterpret_cast<float4*>(v)[at] = v4;
        reinterpret_cast<float4*>(grad)[at] = g4;
        reinterpret_cast<HalfChunk<4>*>(rows)[at] = h4;
    }
}

hipError_t launch_preview_tune_adam(int64_t n_points, int degree, const TuneAdam& a, float* master, float* m, float* v, float* grad,
                                    uint16_t* rows, const uint8_t* mask, hipStream_t stream) {
    const auto kernel = degree == 0 ? k_preview_tune_adam<0> : degree == 1 ? k_preview_tune_adam<1> : k_preview_tune_adam<2>;
    const int64_t chunks = n_points * ((tune_row_used(degree) + 3) / 4);
    const int64_t want = (chunks + 255) / 256;
    const unsigned blocks = (unsigned)(want < 1 ? 1 : want > 256 * 64 ? 256 * 64 : want);      // 256 CUs x 64: the loop strides over the rest
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(256), 0, stream, n_points, a, master, m, v, grad, rows, mask);
    return hipGetLastError();
}

}  // namespace mip
