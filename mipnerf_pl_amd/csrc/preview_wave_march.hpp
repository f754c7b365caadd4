// THE march kernel of the baked preview, stated ONCE for libmipnerf_preview.so (kernels_preview.hip: one lattice),
// libmipnerf_preview_mip.so (kernels_preview_mip.hip: a pyramid of lattices) and libmipnerf_preview_sparse.so (kernels_preview_sparse.hip:
// a pyramid whose levels store only the rows next to an occupied cell).  Each unit includes this header and instantiates the kernel
// for itself (the libraries are linked separately, -fno-gpu-rdc).  The per-sample arithmetic is preview_march.hpp's and preview_mip.hpp's;
// this file only spreads a ray's samples, and the levels they read, over a wavefront.  Compile with -ffp-contract=off (preview_march.hpp).
//
// THE MAPPING.  ONE WAVEFRONT PER RAY (the idiom of kernels_ray.hip), 4 rays per 256-thread block.  The 64 lanes take 64 consecutive
// samples of the ray (a "block" of the march); per block
//   - every lane finds its cell and reads its occupancy bit; the ballot decides wave-uniformly whether the block loads anything at all,
//   - occupied lanes blend their 8 corner rows (16-byte loads; neighbouring samples share corners, so most of them hit the vector cache),
//   - the transmittance inside the block is an exclusive product scan of (1 - alpha) across the lanes (DPP, as raywave.hpp's sums),
//     times the transmittance carried in from the blocks before,
//   - the early stop (T < t_min) is found with a ballot and is wave-uniform; lanes behind the first stopping sample contribute nothing.
// Each lane keeps its own partial sums over the blocks; one fixed-order wave reduction per sum closes the ray.  No atomics, no LDS.
// A lane-per-ray loop would diverge in step count between neighbouring rays and issue scattered row loads; this mapping does neither.
//
// THE LEVELS.  The pyramid travels by value in the kernel arguments.  Every lane finds its own (l, g) from the spacings (read at loop
// counters: scalar loads).  lambda = l + g does not decrease along a ray (w = k t, k >= 0), so the 64 samples of a block read a short run
// of consecutive levels.  The block WALKS the levels present from the lowest to the highest, twice: once for the occupancy bits (P5's OR
// needs both levels of a lane before anything is loaded), once for the rows.  A level nobody needs is skipped by a ballot; inside a level
// its descriptor pyr.level[lv] is indexed by the wave-uniform loop counter, so it is read with scalar loads into SGPRs and only the lanes
// that read this level are active.  No lane indexes the argument struct by its own level (that would move the table to scratch).
// A lane with g == 0 issues 8 corner loads per 16-byte chunk of a row; a lane with g > 0 issues 16, 8 in each of two levels.
//
// ONE LATTICE is the pyramid with L == 1 (P7): mip_level returns (l, g) = (0, 0) before it reads anything, the walks visit level 0 alone
// and the calls are lattice_cell, preview_occupied, preview_row, preview_shade, once each per sample: rule 4 of mipnerf_preview.h.
// mipnerf_preview_march launches it so, with footprint 0 and null `radii` (every ray's radius is then 0) and null `lod`.
#pragma once

#include <hip/hip_runtime.h>

#include "preview_mip.hpp"
#include "raywave.hpp"

namespace mip {

constexpr int kPreviewRaysPerBlock = 4;

// inclusive product over the 64 lanes (lane 63 holds the total): wave_incl_scan_dpp with * and the identity 1
__device__ __forceinline__ float wave_incl_prod_dpp(float v) {
    v *= dpp_f32<kDppRowShr1, 0xf>(1.0f, v);
    v *= dpp_f32<kDppRowShr2, 0xf>(1.0f, v);
    v *= dpp_f32<kDppRowShr4, 0xf>(1.0f, v);
    v *= dpp_f32<kDppRowShr8, 0xf>(1.0f, v);
    v *= dpp_f32<kDppRowBcast15, 0xa>(1.0f, v);
    v *= dpp_f32<kDppRowBcast31, 0xc>(1.0f, v);
    return v;
}

// `radii`, `steps` and `lod` may be null.  PYR: PreviewPyramid (dense rows, preview_mip.hpp) or PreviewSparsePyramid (compact rows behind a
// row table, preview_sparse.hpp); the two differ in the overloads of preview_occupied and preview_row their level type selects, nowhere else.
template <typename PYR, int DEG>
__global__ void __launch_bounds__(64 * kPreviewRaysPerBlock)
k_preview_wave_march(const PYR pyr, const PreviewMarch p, const float footprint, const int64_t n_rays,
                     const float* __restrict__ origins, const float* __restrict__ directions, const float* __restrict__ radii,
                     const float* __restrict__ near, const float* __restrict__ far, float* __restrict__ rgb, float* __restrict__ acc,
                     float* __restrict__ distance, int32_t* __restrict__ steps, float* __restrict__ lod) {
    constexpr int W = preview_row_halves(DEG);
    const int lane = threadIdx.x & 63;
    const int64_t ray = (int64_t)blockIdx.x * kPreviewRaysPerBlock + (threadIdx.x >> 6);
    if (ray >= n_rays) return;                                   // wave-uniform
    const float o[3] = {origins[3 * ray], origins[3 * ray + 1], origins[3 * ray + 2]};
    const float d[3] = {directions[3 * ray], directions[3 * ray + 1], directions[3 * ray + 2]};
    const float tn = near[ray], tf = far[ray], radius = radii ? radii[ray] : 0.0f;      // wave-uniform
    PreviewRay r;
    if (!mip_radius_ok(radius) || !preview_ray(pyr.level[0], p.s, o, d, tn, tf, &r)) {      // wave-uniform: every lane holds the same ray
        if (lane == 0) {
            rgb[3 * ray] = p.background[0]; rgb[3 * ray + 1] = p.background[1]; rgb[3 * ray + 2] = p.background[2];
            acc[ray] = 0.0f;
            distance[ray] = preview_miss_distance(tn, tf);
            if (steps) steps[ray] = 0;
            if (lod) lod[ray] = 0.0f;
        }
        return;
    }
    float Y[(DEG + 1) * (DEG + 1)];
    preview_sh_basis<DEG>(r.u, Y);
    const float k = mip_cone_scale(footprint, radius);
    const int L = pyr.levels;

    float carried = 1.0f;                                        // T before the block's first sample
    float sr = 0.0f, sg = 0.0f, sb = 0.0f, sa = 0.0f, sd = 0.0f, sl = 0.0f;      // this lane's partial sums
    int evaluated = 0;
    for (int base = 0; base < p.max_steps; base += 64) {
        const int i = base + lane;
        const float t = preview_sample_t(r, i);
        const bool exists = i < p.max_steps && t < r.tb;
        const float x[3] = {o[0] + t * d[0], o[1] + t * d[1], o[2] + t * d[2]};
        int l;
        float g;
        mip_level(pyr.spacing, L, mip_footprint(k, t), &l, &g);
        const bool two = g > 0.0f;
        // first walk: the cell and the occupancy bit of this lane's level, and of the next one when g > 0
        int ca[3] = {0, 0, 0}, cb[3] = {0, 0, 0};
        float fa[3] = {0.0f, 0.0f, 0.0f}, fb[3] = {0.0f, 0.0f, 0.0f};
        bool bit = false;
        for (int lv = 0; lv < L; ++lv) {
            const bool lower = exists && l == lv, upper = exists && two && l + 1 == lv;
            if (__ballot(lower || upper) == 0ull) continue;      // wave-uniform: nobody reads this level
            const auto& f = pyr.level[lv];                       // lv is wave-uniform: scalar loads
            if (lower || upper) {
                int c[3];
                float fr[3];
                lattice_cell(f.box, x, c, fr);                   // finite: o, d and t are
                bit = preview_occupied(f, c) || bit;
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    if (lower) { ca[a] = c[a]; fa[a] = fr[a]; }
                    else { cb[a] = c[a]; fb[a] = fr[a]; }
                }
            }
        }
        const bool occupied = exists && bit;
        unsigned long long live = __ballot(occupied);
        if (live != 0ull) {
            float alpha = 0.0f, colour[3] = {0.0f, 0.0f, 0.0f};
            float row[W];
#pragma unroll
            for (int e = 0; e < W; ++e) row[e] = 0.0f;
            // second walk: the rows, lowest level first, so that a lane's own level is blended before the next one is mixed in
            for (int lv = 0; lv < L; ++lv) {
                const bool lower = occupied && l == lv, upper = occupied && two && l + 1 == lv;
                if (__ballot(lower || upper) == 0ull) continue;
                const auto& f = pyr.level[lv];
                if (lower || upper) {
                    const int c[3] = {lower ? ca[0] : cb[0], lower ? ca[1] : cb[1], lower ? ca[2] : cb[2]};
                    const float fr[3] = {lower ? fa[0] : fb[0], lower ? fa[1] : fb[1], lower ? fa[2] : fb[2]};
                    float got[W];
                    preview_row<DEG>(f, c, fr, got);
                    if (lower) {
#pragma unroll
                        for (int e = 0; e < W; ++e) row[e] = got[e];
                    } else {
                        mip_mix<W>(row, got, g);
                    }
                }
            }
            if (occupied) preview_shade<DEG>(row, Y, p.s, &alpha, colour);
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
                const float w = (carried * excl) * alpha;
                sr += w * colour[0];
                sg += w * colour[1];
                sb += w * colour[2];
                sa += w;
                sd += w * t;
                sl += w * mip_lambda(l, g);
            }
            evaluated += __popcll(live);
            if (stop != 0ull) break;
            carried = carried * readlane63(incl);
        }
        if (__ballot(exists) != ~0ull) break;                    // the ray's last block
    }
    sr = wave_sum(sr); sg = wave_sum(sg); sb = wave_sum(sb); sa = wave_sum(sa); sd = wave_sum(sd); sl = wave_sum(sl);
    if (lane == 0) {
        const float rest = 1.0f - sa;
        rgb[3 * ray] = sr + rest * p.background[0];
        rgb[3 * ray + 1] = sg + rest * p.background[1];
        rgb[3 * ray + 2] = sb + rest * p.background[2];
        acc[ray] = sa;
        distance[ray] = preview_distance(sd, sa, tn, tf);
        if (steps) steps[ray] = evaluated;
        if (lod) lod[ray] = mip_lod(sl, sa);
    }
}

// the degree switch; static: every unit launches the instantiations of its own library
template <typename PYR>
static hipError_t launch_preview_wave_march(const PYR& pyr, const PreviewMarch& p, float footprint, int degree, int64_t n_rays,
                                            const float* origins, const float* directions, const float* radii, const float* near,
                                            const float* far, float* rgb, float* acc, float* distance, int32_t* steps, float* lod,
                                            hipStream_t stream) {
    const auto kernel = degree == 0 ? k_preview_wave_march<PYR, 0> : degree == 1 ? k_preview_wave_march<PYR, 1> : k_preview_wave_march<PYR, 2>;
    const dim3 grid((unsigned)((n_rays + kPreviewRaysPerBlock - 1) / kPreviewRaysPerBlock)), block(64 * kPreviewRaysPerBlock);
    hipLaunchKernelGGL(kernel, grid, block, 0, stream, pyr, p, footprint, n_rays, origins, directions, radii, near, far, rgb, acc, distance,
                       steps, lod);
    return hipGetLastError();
}

}  // namespace mip
