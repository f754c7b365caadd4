// libmipnerf_preview.so: the baked-lattice renderer (include/mipnerf_preview.h).  k_preview_pack writes the fp16 rows, k_preview_march
// marches rays through them.  The per-sample arithmetic is preview_march.hpp's; this file only spreads a ray's samples over a wavefront.
//
// k_preview_march: ONE WAVEFRONT PER RAY (the idiom of kernels_ray.hip), 4 rays per 256-thread block.  The 64 lanes take 64 consecutive
// samples of the ray (a "block" of the march); per block
//   - every lane finds its cell and reads its occupancy bit; the ballot decides wave-uniformly whether the block loads anything at all,
//   - occupied lanes blend their 8 corner rows (16-byte loads; neighbouring samples share corners, so most of them hit the vector cache),
//   - the transmittance inside the block is an exclusive product scan of (1 - alpha) across the lanes (DPP, as raywave.hpp's sums),
//     times the transmittance carried in from the blocks before,
//   - the early stop (T < t_min) is found with a ballot and is wave-uniform; lanes behind the first stopping sample contribute nothing.
// Each lane keeps its own partial sums over the blocks; one fixed-order wave reduction per sum closes the ray.  No atomics, no LDS.
// A lane-per-ray loop would diverge in step count between neighbouring rays and issue scattered row loads; this mapping does neither.
// Compile with -ffp-contract=off (preview_march.hpp).
#include <hip/hip_runtime.h>

#include "preview_march.hpp"
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

template <int DEG>
__global__ void __launch_bounds__(64 * kPreviewRaysPerBlock)
k_preview_march(const PreviewField f, const PreviewMarch p, const int64_t n_rays, const float* __restrict__ origins,
                const float* __restrict__ directions, const float* __restrict__ near, const float* __restrict__ far, float* __restrict__ rgb,
                float* __restrict__ acc, float* __restrict__ distance, int32_t* __restrict__ steps) {
    const int lane = threadIdx.x & 63;
    const int64_t ray = (int64_t)blockIdx.x * kPreviewRaysPerBlock + (threadIdx.x >> 6);
    if (ray >= n_rays) return;                                   // wave-uniform
    const float o[3] = {origins[3 * ray], origins[3 * ray + 1], origins[3 * ray + 2]};
    const float d[3] = {directions[3 * ray], directions[3 * ray + 1], directions[3 * ray + 2]};
    const float tn = near[ray], tf = far[ray];
    PreviewRay r;
    if (!preview_ray(f, p.s, o, d, tn, tf, &r)) {                // wave-uniform: every lane holds the same ray
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

    float carried = 1.0f;                                        // T before the block's first sample
    float sr = 0.0f, sg = 0.0f, sb = 0.0f, sa = 0.0f, sd = 0.0f; // this lane's partial sums
    int evaluated = 0;
    for (int base = 0; base < p.max_steps; base += 64) {
        const int i = base + lane;
        const float t = preview_sample_t(r, i);
        const bool exists = i < p.max_steps && t < r.tb;
        const float x[3] = {o[0] + t * d[0], o[1] + t * d[1], o[2] + t * d[2]};
        int c[3];
        float fr[3];
        lattice_cell(f.box, x, c, fr);                           // finite: o, d and t are
        const bool occupied = exists && preview_occupied(f, c);
        unsigned long long live = __ballot(occupied);
        if (live != 0ull) {
            float alpha = 0.0f, colour[3] = {0.0f, 0.0f, 0.0f};
            if (occupied) preview_sample<DEG>(f, c, fr, Y, p.s, &alpha, colour);
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

__global__ void __launch_bounds__(256)
k_preview_pack(const int64_t n, const int degree, const float* __restrict__ sigma, const float* __restrict__ coef,
               const uint8_t* __restrict__ mask, uint16_t* __restrict__ rows) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int W = preview_row_halves(degree), used = 3 * preview_basis(degree);
    const bool keep = mask == nullptr || mask[i] != 0;
    uint16_t* row = rows + i * W;
    row[0] = preview_half_bits(sigma[i], true);
    const float* cf = coef + i * used;
    for (int k = 0; k < used; ++k) row[1 + k] = keep ? preview_half_bits(cf[k], false) : (uint16_t)0;
    for (int k = 1 + used; k < W; ++k) row[k] = 0;
}

hipError_t launch_preview_march(const PreviewField& f, const PreviewMarch& p, int degree, int64_t n_rays, const float* origins,
                                const float* directions, const float* near, const float* far, float* rgb, float* acc, float* distance,
                                int32_t* steps, hipStream_t stream) {
    const dim3 grid((unsigned)((n_rays + kPreviewRaysPerBlock - 1) / kPreviewRaysPerBlock)), block(64 * kPreviewRaysPerBlock);
    if (degree == 0)
        hipLaunchKernelGGL(k_preview_march<0>, grid, block, 0, stream, f, p, n_rays, origins, directions, near, far, rgb, acc, distance, steps);
    else if (degree == 1)
        hipLaunchKernelGGL(k_preview_march<1>, grid, block, 0, stream, f, p, n_rays, origins, directions, near, far, rgb, acc, distance, steps);
    else
        hipLaunchKernelGGL(k_preview_march<2>, grid, block, 0, stream, f, p, n_rays, origins, directions, near, far, rgb, acc, distance, steps);
    return hipGetLastError();
}

hipError_t launch_preview_pack(int64_t n, int degree, const float* sigma, const float* coef, const uint8_t* mask, uint16_t* rows,
                               hipStream_t stream) {
    hipLaunchKernelGGL(k_preview_pack, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, n, degree, sigma, coef, mask, rows);
    return hipGetLastError();
}

}  // namespace mip
