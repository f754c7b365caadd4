// Host build of the ray side of empty-space skipping in the contracted space (mipnerf_pl_amd/csrc/raymath360.hpp -- the source the gfx950
// kernels k_ray_occupancy_360 / k_ray_span_360 and the sampler k_sample_along_rays_360 inline) for tests/test_cull360_cpu.py;
// g++ -O2 -ffp-contract=off.
#include "../../mipnerf_pl_amd/csrc/raymath.hpp"
#include "../../mipnerf_pl_amd/csrc/raymath360.hpp"

extern "C" {
// t_inv, t [n, N + 1]: the coarse level's deterministic fence posts
void cb_fence_posts(int n, int N, const float* nearp, const float* farp, float* t_inv, float* t) {
    for (int b = 0; b < n; ++b)
        for (int k = 0; k <= N; ++k) {
            const float ti = mip::level0_t_inv_360(1.0f / nearp[b], 1.0f / farp[b], N, k);
            t_inv[b * (N + 1) + k] = ti;
            t[b * (N + 1) + k] = mip::level0_t_360(nearp[b], farp[b], N, k);
        }
}
// lo, hi [n, N, 3]: the box of every coarse frustum
void cb_boxes(int n, int N, const float* o, const float* d, const float* radii, const float* nearp, const float* farp, float cone_scale,
              float* lo, float* hi) {
    for (int b = 0; b < n; ++b)
        for (int i = 0; i < N; ++i) {
            const float t0 = mip::level0_t_360(nearp[b], farp[b], N, i), t1 = mip::level0_t_360(nearp[b], farp[b], N, i + 1);
            mip::contracted_frustum_box(t0, t1, o + 3 * b, d + 3 * b, cone_scale * radii[b], lo + 3 * (b * N + i), hi + 3 * (b * N + i));
        }
}
}
