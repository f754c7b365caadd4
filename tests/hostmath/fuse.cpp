// Host build of csrc/fuse_rules.hpp for tests/test_fuse_cpu.py:
//   g++ -O2 -ffp-contract=off -shared -fPIC fuse.cpp -o _fuse.so
#include "../../mipnerf_pl_amd/csrc/fuse_rules.hpp"

extern "C" {

// rule D: out[b, j] = the depth at which ray b reaches opacity q[j], the prefixes summed in sample order
void hm_depth_quantile(long long B, int N, const float* w, const float* t, int nq, const float* q, float* out) {
    for (long long b = 0; b < B; ++b)
        for (int j = 0; j < nq; ++j) out[b * nq + j] = mip::depth_quantile_ray(N, w + b * N, t + b * (N + 1), (double)q[j]);
}

// rule F, elementwise
void hm_finalise(long long n, const float* sum, const float* count, float fill, float* out) {
    for (long long i = 0; i < n; ++i) out[i] = mip::fuse_finalise_value(sum[i], count[i], fill);
}

int hm_frames_per_launch() { return mip::kFuseFramesPerLaunch; }

}  // extern "C"
