// libmipnerf_preview_360.so: the baked preview of the unbounded-scene model, a lattice over the CONTRACTED space marched along straight
// world rays (include/mipnerf_preview_360.h).  The rules are preview_march_360.hpp's; the rows, the blend and the shading are
// preview_march.hpp's, the compact storage is preview_sparse.hpp's.  Compile with -ffp-contract=off (preview_march_360.hpp).
//
// THE MAPPING is k_preview_wave_march's (preview_wave_march.hpp): ONE WAVEFRONT PER RAY, 4 rays per 256-thread block; the 64 lanes take
// 64 consecutive samples (a block of the march); per block every lane finds its sample's contracted point, its cell and its occupancy
// bit, a ballot decides wave-uniformly whether the block loads anything, occupied lanes blend their 8 corner rows, the transmittance is
// an exclusive product scan across the lanes (DPP) times what the blocks before carried in, the early stop is a ballot, and one
// fixed-order wave reduction per sum closes the ray.  No atomics, no LDS.
//
// WHAT IS NEW per sample: two evaluations of V (C3: one tanf each) -- the sample's arclength tau_i and its upper edge e_{i+1} -- a
// division by |d|, the contraction (one sqrt, two divisions) and a box test.  THE RAY'S CONSTANTS LIVE IN SCALAR REGISTERS: the wave's
// ray index is formed with readfirstlane, so origin, direction, near and far arrive by scalar loads; gfx950 has no scalar float unit, so
// C2 / C3 and the SH basis are computed once on the vector ALU (every lane the same value) and each result is moved to an SGPR with
// readfirstlane (wave_uniform below): the constants cost no VGPRs in the march loop.  A sample's lower edge e_i is the upper edge of the lane before it (one wave shift):
// the same expression on the same inputs, so the deltas partition [la, lb].  Lane 0 takes the edge carried out of the block before; after
// a block that loaded nothing (its edges were never formed) and at the ray's first block the wave computes e_base itself, uniformly.
#include <hip/hip_runtime.h>

#include "preview_march_360.hpp"
#include "preview_sparse.hpp"
#include "preview_wave_march.hpp"

namespace mip {

// a value every lane of the wave holds alike, moved to a scalar register
__device__ __forceinline__ float wave_uniform(float v) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(v))); }

// `steps` may be null.  FIELD: PreviewField (dense rows) or PreviewSparseField (compact rows behind a row table); the two differ in the
// overloads of preview_occupied and preview_row, nowhere else.
template <typename FIELD, int DEG>
__global__ void __launch_bounds__(64 * kPreviewRaysPerBlock)
k_preview_360(const FIELD f, const PreviewMarch p, const float far_radius, const int64_t n_rays, const float* __restrict__ origins,
                    const float* __restrict__ directions, const float* __restrict__ near, const float* __restrict__ far,
                    float* __restrict__ rgb, float* __restrict__ acc, float* __restrict__ distance, int32_t* __restrict__ steps) {
    constexpr int W = preview_row_halves(DEG);
    const int lane = threadIdx.x & 63;
    const int64_t ray = (int64_t)blockIdx.x * kPreviewRaysPerBlock + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);      // scalar
    if (ray >= n_rays) return;                                   // wave-uniform
    const float o[3] = {origins[3 * ray], origins[3 * ray + 1], origins[3 * ray + 2]};
    const float d[3] = {directions[3 * ray], directions[3 * ray + 1], directions[3 * ray + 2]};
    const float tn = near[ray], tf = far[ray];                   // wave-uniform
    PreviewRay360 r;
    if (!preview360_ray(far_radius, o, d, tn, tf, &r)) {         // wave-uniform: every lane holds the same ray
        if (lane == 0) {
            rgb[3 * ray] = p.background[0]; rgb[3 * ray + 1] = p.background[1]; rgb[3 * ray + 2] = p.background[2];
            acc[ray] = 0.0f;
            distance[ray] = preview_miss_distance(tn, tf);
            if (steps) steps[ray] = 0;
        }
        return;
    }
    float Y[(DEG + 1) * (DEG + 1)];
    preview_sh_basis<DEG>(r.u, Y);
    r.len = wave_uniform(r.len); r.tc = wave_uniform(r.tc); r.p2 = wave_uniform(r.p2); r.p = wave_uniform(r.p); r.c = wave_uniform(r.c);
    r.ts = wave_uniform(r.ts); r.tau_lo = wave_uniform(r.tau_lo); r.tau_hi = wave_uniform(r.tau_hi); r.wa = wave_uniform(r.wa);
    r.wb = wave_uniform(r.wb);
#pragma unroll
    for (int k = 0; k < (DEG + 1) * (DEG + 1); ++k) Y[k] = wave_uniform(Y[k]);

    float carried = 1.0f;                                        // T before the block's first sample
    float edge_in = 0.0f;                                        // e_base, valid when edge_at == base
    int edge_at = -1;
    float sr = 0.0f, sg = 0.0f, sb = 0.0f, sa = 0.0f, sd = 0.0f;      // this lane's partial sums
    int evaluated = 0;
    for (int base = 0; base < p.max_steps; base += 64) {
        const int i = base + lane;
        const float w = preview360_sample_w(r, p.s, i);
        const bool exists = i < p.max_steps && preview360_exists(r, i, w);
        const float t = preview360_t(r, preview360_unwarp(r, w));      // finite also where the sample does not exist: V is clamped
        const float x[3] = {o[0] + t * d[0], o[1] + t * d[1], o[2] + t * d[2]};
        float z[3];
        preview360_contract(x, z);
        int c[3] = {0, 0, 0};
        float fr[3] = {0.0f, 0.0f, 0.0f};
        bool occupied = exists && preview360_inside(f, z);       // a z that is not finite is not inside
        if (occupied) {
            lattice_cell(f.box, z, c, fr);
            occupied = preview_occupied(f, c);
        }
        unsigned long long live = __ballot(occupied);
        if (live != 0ull) {
            if (edge_at != base) edge_in = preview360_upper_edge(r, p.s, base - 1);      // wave-uniform
            const float e_hi = preview360_upper_edge(r, p.s, i);
            const float e_lo = dpp_f32<kDppWaveShr1, 0xf>(edge_in, e_hi);      // lane i <- lane i - 1, lane 0 <- e_base
            edge_in = readlane63(e_hi);
            edge_at = base + 64;
            const float delta = fmaxf(e_hi - e_lo, 0.0f);
            float alpha = 0.0f, colour[3] = {0.0f, 0.0f, 0.0f};
            if (occupied) {
                float row[W];
                preview_row<DEG>(f, c, fr, row);
                preview_shade<DEG>(row, Y, delta, &alpha, colour);
            }
            const float incl = wave_incl_prod_dpp(1.0f - alpha);
            const float excl = dpp_f32<kDppWaveShr1, 0xf>(1.0f, incl);
            const unsigned long long stop = __ballot(carried * incl < p.t_min);
            bool counted = occupied;
            if (stop != 0ull) {
                const int first = __builtin_ctzll(stop);
                counted = occupied && lane <= first;
                live &= first == 63 ? ~0ull : (2ull << first) - 1ull;
            }
            if (counted) {
                const float wt = (carried * excl) * alpha;
                sr += wt * colour[0];
                sg += wt * colour[1];
                sb += wt * colour[2];
                sa += wt;
                sd += wt * t;
            }
            evaluated += __popcll(live);
            if (stop != 0ull) break;
            carried = carried * readlane63(incl);
        }
        if (__ballot(exists) != ~0ull) break;                    // the ray's last block
    }
    sr = wave_sum(sr); sg = wave_sum(sg); sb = wave_sum(sb); sa = wave_sum(sa); sd = wave_sum(sd);
    if (lane == 0) {
        const float rest = 1.0f - sa;
        rgb[3 * ray] = sr + rest * p.background[0];
        rgb[3 * ray + 1] = sg + rest * p.background[1];
        rgb[3 * ray + 2] = sb + rest * p.background[2];
        acc[ray] = sa;
        distance[ray] = preview_distance(sd, sa, tn, tf);
        if (steps) steps[ray] = evaluated;
    }
}

template <typename FIELD>
static hipError_t launch_march_360(const FIELD& f, const PreviewMarch& p, float far_radius, int degree, int64_t n_rays, const float* origins,
                                   const float* directions, const float* near, const float* far, float* rgb, float* acc, float* distance,
                                   int32_t* steps, hipStream_t stream) {
    const auto kernel = degree == 0 ? k_preview_360<FIELD, 0> : degree == 1 ? k_preview_360<FIELD, 1> : k_preview_360<FIELD, 2>;
    const dim3 grid((unsigned)((n_rays + kPreviewRaysPerBlock - 1) / kPreviewRaysPerBlock)), block(64 * kPreviewRaysPerBlock);
    hipLaunchKernelGGL(kernel, grid, block, 0, stream, f, p, far_radius, n_rays, origins, directions, near, far, rgb, acc, distance, steps);
    return hipGetLastError();
}

hipError_t launch_preview_march_360(const PreviewField& f, const PreviewMarch& p, float far_radius, int degree, int64_t n_rays,
                                    const float* origins, const float* directions, const float* near, const float* far, float* rgb,
                                    float* acc, float* distance, int32_t* steps, hipStream_t stream) {
    return launch_march_360(f, p, far_radius, degree, n_rays, origins, directions, near, far, rgb, acc, distance, steps, stream);
}

hipError_t launch_preview_march_360_sparse(const PreviewSparseField& f, const PreviewMarch& p, float far_radius, int degree, int64_t n_rays,
                                           const float* origins, const float* directions, const float* near, const float* far, float* rgb,
                                           float* acc, float* distance, int32_t* steps, hipStream_t stream) {
    return launch_march_360(f, p, far_radius, degree, n_rays, origins, directions, near, far, rgb, acc, distance, steps, stream);
}

}  // namespace mip
