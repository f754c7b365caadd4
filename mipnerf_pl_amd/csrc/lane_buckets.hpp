// Host-side launch rules of the per-ray kernels (one wavefront per ray, lane l holds K samples): the samples-per-lane bucket of a sample
// count, the limit it implies, the sampler's draw step and the grid size.  Each is stated here once; every launcher of a kernel templated
// on K goes through for_lane_bucket.  Plain C++17 without HIP headers: tests/test_lane_buckets_cpu.py compiles it with g++.
#pragma once

#include <stdint.h>

#include <type_traits>
#include <utility>

namespace mip {

// K comes from the buckets 1, 2, 4, ..., kMaxSamplesPerLane.  A ray's sums associate by K, so ONE rule lets the fused launches
// (k_composite_resample, k_composite_train) reproduce the per-stage kernels, and k_ray_span's `live` k_ray_occupancy's, bit for bit.
constexpr int kMaxSamplesPerLane = 16;
constexpr int kPdfMaxBins = 64 * kMaxSamplesPerLane;     // N <= 1024 (MIPNERF_MAX_SAMPLES, asserted in capi.hip)
// LDS row length of a kernel instantiated for K samples per lane: the K <= 8 buckets keep their 512-entry rows (24 KiB per block: six blocks per CU);
// only the K = 16 bucket (512 < N <= 1024) pays for 1024-entry rows
template <int K> struct PdfRow { static constexpr int kBins = K <= 8 ? 512 : kPdfMaxBins; };

// the smallest bucket K with 64 * K >= N; 0: N has none (N < 1 or N > kPdfMaxBins)
constexpr int lane_bucket(int N) {
    if (N < 1 || N > kPdfMaxBins) return 0;
    int K = 1;
    while (64 * K < N) K *= 2;
    return K;
}

namespace detail {
template <int K, class F>
inline bool for_lane_bucket_from(int bucket, F&& f) {
    if constexpr (K > kMaxSamplesPerLane) {
        return false;
    } else {
        if (bucket != K) return for_lane_bucket_from<2 * K>(bucket, std::forward<F>(f));
        f(std::integral_constant<int, K>{});
        return true;
    }
}
}  // namespace detail

// f(std::integral_constant<int, lane_bucket(N)>{}) -- the bucket as a compile-time constant; false (f not called): N has no bucket, and
// the launcher returns hipErrorInvalidValue instead of hipGetLastError()
template <class F>
inline bool for_lane_bucket(int N, F&& f) {
    return detail::for_lane_bucket_from<1>(lane_bucket(N), std::forward<F>(f));
}

// The sampler's stratified draws u_j = j * u_step + rand * u_jitter: s = 1 / n_draws and the jitter range s - eps32, evaluated in double
// like the Python reference and rounded once.  The forward and its backward must draw the same u, so both take the pair from here.
struct DrawStep {
    float u_step, u_jitter;
};
inline DrawStep draw_step(int n_draws) {
    const double s = 1.0 / (double)n_draws;
    const float u_step = (float)s;
    const float u_jitter = (float)(s - (double)1.1920928955078125e-07f);
    return {u_step, u_jitter};
}

// workgroups of `block` items that cover n
inline unsigned grid_for(int64_t n, int block) { return (unsigned)((n + block - 1) / block); }

}  // namespace mip
