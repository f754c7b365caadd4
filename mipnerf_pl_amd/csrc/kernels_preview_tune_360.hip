// libmipnerf_preview_tune_360.so (include/mipnerf_preview_tune_360.h): tuning a lattice over the CONTRACTED space through its own march.
//   k_preview_360_tune_grad   the march of k_preview_360 on one dense lattice AND its gradient with respect to the rows, one launch
// The per-sample arithmetic is preview_march_360.hpp's (C1 - C5), preview_march.hpp's (rows, blend, shading) and preview_tune_360.hpp's
// (C6 - C8); this file spreads it over lanes.  Compile with -ffp-contract=off (preview_march_360.hpp).
//
// ONE WAVEFRONT PER RAY, 4 rays per 256-thread block, and the TWO SWEEPS of k_preview_tune_grad (kernels_preview_tune.hip) on the sample
// placement of k_preview_360 (kernels_preview_360.hip):
//   tune360_block below is one 64-sample block of k_preview_360, the same calls in the same order: the warped coordinate, V, the
//     contraction, the box test, the cell, the occupancy bit and its ballot; the upper edge e_hi, the lower edge by one wave shift with
//     the carried edge_in / edge_at, delta, preview_row, preview_shade(row, Y, delta, ...), the DPP product scan and the stop ballot.
//     BOTH sweeps call it.
//   SWEEP A is therefore that march: rgb and acc are mipnerf_preview_360_march's, bit for bit.  It yields G and total = sum_i w_i q_i.
//     A ray that misses, a ray with G = 0 and g_a = 0 and a ray with a non-finite output or G ends here.
//   SWEEP B revisits the ray's blocks (their rows are cache-hot): T_{i+1} is the inclusive product scan, S_i = total - (before + the
//     inclusive sum scan of w q); each lane (= sample) forms C7 with its OWN delta_i.
//   THE SCATTER IS TRANSPOSED and RUNS ARE COMBINED across block boundaries exactly as in kernels_preview_tune.hip: lanes become
//     destinations, 1 / 2 / 4 atomic wave instructions per flush for degree 0 / 1 / 2, plain atomicAdd(float*) with the result unused.
// THE RAY'S CONSTANTS AND Y are moved to scalar registers as in k_preview_360 (readfirstlane) for degree 0 and stay in vector registers
// for degrees 1 and 2 (kTune360Scalar below): a measured choice per degree.
// TuneSlots and bcast are restated here, not moved into a header shared with kernels_preview_tune.hip: that unit stays untouched, so
// libmipnerf_preview_tune.so is the parent commit's byte for byte.  No LDS, no inline assembly.
#include <hip/hip_runtime.h>

#include "preview_tune_360.hpp"
#include "preview_wave_march.hpp"

namespace mip {

// a value every lane of the wave holds alike, moved to a scalar register
__device__ __forceinline__ float wave_uniform360(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }

// what one 64-sample block of the march leaves in a lane
struct Tune360Block {
    int c[3];
    float fr[3];
    float row0;              // the blended row's density entry before its clamp
    float alpha, colour[3];
    float delta;             // C4's world length of the sample, the number alpha was formed with
    float incl, excl;        // the inclusive / exclusive product of (1 - alpha) inside the block
    bool exists, counted;    // counted: evaluated and not behind the early stop
    unsigned long long live; // the ballot of the occupied samples (0: the block loaded nothing and none of the above but `exists` is set)
    bool stop;               // wave-uniform: the early stop lies in this block
};

// one block of k_preview_360 on a dense lattice: the same calls in the same order.  edge_in / edge_at: the edge carried between blocks.
template <int DEG>
__device__ __forceinline__ void tune360_block(const PreviewField& f, const PreviewMarch& p, const PreviewRay360& r, const float o[3],
                                              const float d[3], const float (&Y)[(DEG + 1) * (DEG + 1)], int base, int lane, float carried,
                                              float* edge_in, int* edge_at, Tune360Block* b) {
    constexpr int W = preview_row_halves(DEG);
    const int i = base + lane;
    const float w = preview360_sample_w(r, p.s, i);
    b->exists = i < p.max_steps && preview360_exists(r, i, w);
    const float t = preview360_t(r, preview360_unwarp(r, w));      // finite also where the sample does not exist: V is clamped
    b->c[0] = b->c[1] = b->c[2] = 0;
    b->fr[0] = b->fr[1] = b->fr[2] = 0.0f;
    int c[3] = {0, 0, 0};
    float fr[3] = {0.0f, 0.0f, 0.0f};
    bool occupied = b->exists && tune360_cell(f, o, d, t, c, fr);      // a z that is not finite is not inside
    if (occupied) occupied = preview_occupied(f, c);
#pragma unroll
    for (int a = 0; a < 3; ++a) { b->c[a] = c[a]; b->fr[a] = fr[a]; }
    b->live = __ballot(occupied);
    b->counted = false;
    b->stop = false;
    b->alpha = 0.0f;
    b->colour[0] = b->colour[1] = b->colour[2] = 0.0f;
    b->row0 = 0.0f;
    b->delta = 0.0f;
    b->incl = b->excl = 1.0f;
    if (b->live == 0ull) return;
    if (*edge_at != base) *edge_in = preview360_upper_edge(r, p.s, base - 1);      // wave-uniform
    const float e_hi = preview360_upper_edge(r, p.s, i);
    const float e_lo = dpp_f32<kDppWaveShr1, 0xf>(*edge_in, e_hi);      // lane i <- lane i - 1, lane 0 <- e_base
    *edge_in = readlane63(e_hi);
    *edge_at = base + 64;
    b->delta = tune360_delta(e_lo, e_hi);
    if (occupied) {
        float row[W];
        preview_row<DEG>(f, c, fr, row);
        preview_shade<DEG>(row, Y, b->delta, &b->alpha, b->colour);
        b->row0 = row[0];
    }
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

__device__ __forceinline__ float bcast360(float v, int src) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src)); }
__device__ __forceinline__ int bcast360(int v, int src) { return __builtin_amdgcn_readlane(v, src); }

// how the 8 corner rows of a cell are spread over the lanes of a flush: TuneSlots of kernels_preview_tune.hip (see the top of that file)
template <int DEG>
struct Tune360Slots {
    static constexpr int W = preview_row_halves(DEG);
    static constexpr int N = DEG == 0 ? 1 : DEG == 1 ? 2 : 4;            // atomic instructions per flush = slot registers per lane
    __device__ static int element(int lane) { return lane & (W - 1); }
    __device__ static int xcorner(int lane) { return (lane / W) & 1; }
    __device__ static int ycorner(int lane, int j) { return DEG == 0 ? (lane >> 3) & 1 : DEG == 1 ? lane >> 5 : j & 1; }
    __device__ static int zcorner(int lane, int j) { return DEG == 0 ? (lane >> 4) & 1 : DEG == 1 ? j : j >> 1; }
    __device__ static bool active(int lane) { return (DEG != 0 || lane < 32) && element(lane) < tune_row_used(DEG); }
};

// whether the ray's constants and Y are moved to scalar registers, per degree: the values are the same either way, the faster form of
// each degree is the one chosen (DESIGN 4.21 has both timings: scalar wins by 4 - 5 % at degree 0, vector by 1 - 2 % at degrees 1 and 2)
constexpr bool kTune360Scalar[3] = {true, false, false};

// `counters` (optional): [0] += the samples that added something, [1] += the flushes (each is Tune360Slots::N atomic instructions)
template <int DEG>
__global__ void __launch_bounds__(64 * kPreviewRaysPerBlock)
k_preview_360_tune_grad(const PreviewField f, const PreviewMarch p, const float far_radius, const int64_t n_rays,
                        const float* __restrict__ origins, const float* __restrict__ directions, const float* __restrict__ near,
                        const float* __restrict__ far, const float* __restrict__ grad_rgb, const float* __restrict__ target,
                        const float loss_scale, const float* __restrict__ grad_acc, float* __restrict__ rgb, float* __restrict__ acc,
                        float* __restrict__ grad_rows, unsigned long long* __restrict__ counters) {
    typedef Tune360Slots<DEG> Slots;
    constexpr int W = preview_row_halves(DEG), NB = preview_basis(DEG), NS = Slots::N;
    const int lane = threadIdx.x & 63;
    const int64_t ray = (int64_t)blockIdx.x * kPreviewRaysPerBlock + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);      // scalar
    if (ray >= n_rays) return;                                   // wave-uniform
    const float o[3] = {origins[3 * ray], origins[3 * ray + 1], origins[3 * ray + 2]};
    const float d[3] = {directions[3 * ray], directions[3 * ray + 1], directions[3 * ray + 2]};
    const float tn = near[ray], tf = far[ray];                   // wave-uniform
    PreviewRay360 r;
    if (!preview360_ray(far_radius, o, d, tn, tf, &r)) {         // wave-uniform: a miss adds nothing
        if (lane == 0) {
            rgb[3 * ray] = p.background[0]; rgb[3 * ray + 1] = p.background[1]; rgb[3 * ray + 2] = p.background[2];
            acc[ray] = 0.0f;
        }
        return;
    }
    float Y[NB];
    preview_sh_basis<DEG>(r.u, Y);
    if (kTune360Scalar[DEG]) {
        r.len = wave_uniform360(r.len); r.tc = wave_uniform360(r.tc); r.p2 = wave_uniform360(r.p2); r.p = wave_uniform360(r.p);
        r.c = wave_uniform360(r.c); r.ts = wave_uniform360(r.ts); r.tau_lo = wave_uniform360(r.tau_lo); r.tau_hi = wave_uniform360(r.tau_hi);
        r.wa = wave_uniform360(r.wa); r.wb = wave_uniform360(r.wb);
#pragma unroll
        for (int k = 0; k < NB; ++k) Y[k] = wave_uniform360(Y[k]);
    }

    // ---- sweep A: the march ----
    Tune360Block b;
    float carried = 1.0f;
    float edge_in = 0.0f;
    int edge_at = -1;
    float sr = 0.0f, sg = 0.0f, sb = 0.0f, sa = 0.0f;
    for (int base = 0; base < p.max_steps; base += 64) {
        tune360_block<DEG>(f, p, r, o, d, Y, base, lane, carried, &edge_in, &edge_at, &b);
        if (b.live != 0ull) {
            if (b.counted) {
                const float wt = (carried * b.excl) * b.alpha;
                sr += wt * b.colour[0];
                sg += wt * b.colour[1];
                sb += wt * b.colour[2];
                sa += wt;
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
    if (G[0] == 0.0f && G[1] == 0.0f && G[2] == 0.0f && g_a == 0.0f) return;      // every term of C7 is a multiple of G or g_a
    const float sc[3] = {sr, sg, sb};
    const float total = tune_total(G, g_a, sc, sa, p.background);

    // ---- sweep B: d row per sample, scattered transposed ----
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
    edge_in = 0.0f;
    edge_at = -1;
    float before = 0.0f;                                         // sum of w q over the blocks before this one
    for (int base = 0; base < p.max_steps; base += 64) {
        tune360_block<DEG>(f, p, r, o, d, Y, base, lane, carried, &edge_in, &edge_at, &b);
        if (b.live != 0ull) {
            const float w = b.counted ? (carried * b.excl) * b.alpha : 0.0f;
            const float q = tune_q(G, g_a, b.colour, p.background);
            const float wq = b.counted ? w * q : 0.0f;
            const float upto = before + wave_incl_scan_dpp(wq);                    // sum_{j <= i} w_j q_j
            const float ds = tune360_d_sigma(b.delta, carried * b.incl, q, total - upto, b.row0);
            const float dc[3] = {tune_d_colour(w, G[0], b.colour[0]), tune_d_colour(w, G[1], b.colour[1]), tune_d_colour(w, G[2], b.colour[2])};
            const int cell = (b.c[2] * f.box.ny + b.c[1]) * f.box.nx + b.c[0];     // < nx ny nz < 2^31 / 7; c <= n - 2 on every axis
            unsigned long long todo = __ballot(b.counted);
            n_samples += __popcll(todo);
            while (todo != 0ull) {                               // wave-uniform: the counted samples in order
                const int src = __builtin_ctzll(todo);
                todo &= todo - 1ull;
                const int s_cell = bcast360(cell, src);
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
                const float s_fr[3] = {bcast360(b.fr[0], src), bcast360(b.fr[1], src), bcast360(b.fr[2], src)};
                const float s_ds = bcast360(ds, src), s_dc0 = bcast360(dc[0], src), s_dc1 = bcast360(dc[1], src), s_dc2 = bcast360(dc[2], src);
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

hipError_t launch_preview_360_tune_grad(const PreviewField& f, const PreviewMarch& p, float far_radius, int degree, int64_t n_rays,
                                        const float* origins, const float* directions, const float* near, const float* far,
                                        const float* grad_rgb, const float* target, float loss_scale, const float* grad_acc, float* rgb,
                                        float* acc, float* grad_rows, unsigned long long* counters, hipStream_t stream) {
    const auto kernel = degree == 0 ? k_preview_360_tune_grad<0> : degree == 1 ? k_preview_360_tune_grad<1> : k_preview_360_tune_grad<2>;
    const dim3 grid((unsigned)((n_rays + kPreviewRaysPerBlock - 1) / kPreviewRaysPerBlock)), block(64 * kPreviewRaysPerBlock);
    hipLaunchKernelGGL(kernel, grid, block, 0, stream, f, p, far_radius, n_rays, origins, directions, near, far, grad_rgb, target, loss_scale,
                       grad_acc, rgb, acc, grad_rows, counters);
    return hipGetLastError();
}

}  // namespace mip
