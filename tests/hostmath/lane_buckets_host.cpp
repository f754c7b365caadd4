// Host program around mipnerf_pl_amd/csrc/lane_buckets.hpp (plain C++17, no HIP headers) for tests/test_lane_buckets_cpu.py.
// Prints one line per query: "B <N> <lane_bucket(N)> <constant the dispatcher passed, 0 = not called> <its return value>" for every N in
// [-1, 1030], "D <n_draws> <bits of u_step> <bits of u_jitter>" for each n_draws given on the command line, "G <grid_for results>".
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../mipnerf_pl_amd/csrc/lane_buckets.hpp"

static_assert(mip::lane_bucket(0) == 0 && mip::lane_bucket(1) == 1 && mip::lane_bucket(65) == 2 && mip::lane_bucket(1024) == 16 &&
                  mip::lane_bucket(1025) == 0,
              "lane_bucket is usable in constant expressions");
static_assert(mip::kPdfMaxBins == 1024 && mip::PdfRow<8>::kBins == 512 && mip::PdfRow<16>::kBins == 1024, "LDS rows");

static unsigned bits(float x) {
    unsigned u;
    memcpy(&u, &x, sizeof u);
    return u;
}

int main(int argc, char** argv) {
    for (int N = -1; N <= 1030; ++N) {
        int got = 0, calls = 0;
        const bool ok = mip::for_lane_bucket(N, [&](auto k) {
            static_assert(decltype(k)::value >= 1 && decltype(k)::value <= mip::kMaxSamplesPerLane, "a compile-time constant");
            got = decltype(k)::value;
            ++calls;
        });
        if (calls > 1) return 1;
        printf("B %d %d %d %d\n", N, mip::lane_bucket(N), got, ok ? 1 : 0);
    }
    for (int i = 1; i < argc; ++i) {
        const mip::DrawStep u = mip::draw_step(atoi(argv[i]));
        printf("D %d %u %u\n", atoi(argv[i]), bits(u.u_step), bits(u.u_jitter));
    }
    printf("G %u %u %u %u %u\n", mip::grid_for(0, 256), mip::grid_for(1, 256), mip::grid_for(256, 256), mip::grid_for(257, 256),
           mip::grid_for(((int64_t)1 << 33) + 1, 256));
    return 0;
}
