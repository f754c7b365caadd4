// Test-only: a stand-alone program over the entry points hostmath.cpp has for the unbounded-scene path (hm_sample_360, hm_gauss_360,
// hm_lattice_gauss_360, hm_cast_ipe_360), every buffer a heap block of exactly the documented size, so that a build with
//   g++ -O1 -g -ffp-contract=off -fsanitize=address,undefined ipe360_selftest.cpp -o _ipe360_selftest
// reports any access outside them and any undefined operation.  Prints "ok" and returns 0 when every output is finite.
#include <cmath>
#include <cstdio>
#include <vector>

#include "hostmath.cpp"

static int finite_all(const std::vector<float>& v) {
    for (float x : v)
        if (!std::isfinite(x)) return 0;
    return 1;
}

int main() {
    int ok = 1;
    const int shapes[5][2] = {{1, 1}, {3, 21}, {1, 64}, {5, 13}, {2, 129}};
    const int degs[5][2] = {{0, 16}, {3, 19}, {15, 31}, {0, 8}, {0, 6}};
    for (const auto& sh : shapes) {
        const int B = sh[0], N = sh[1];
        std::vector<float> nearv(B), farv(B), t_rand((size_t)B * (N + 1)), t_inv((size_t)B * (N + 1)), t((size_t)B * (N + 1));
        for (int b = 0; b < B; ++b) { nearv[b] = 0.2f + 0.1f * b; farv[b] = b == B - 1 ? nearv[b] : 40.0f + 100.0f * b; }
        for (size_t i = 0; i < t_rand.size(); ++i) t_rand[i] = (float)((i * 37) % 101) / 101.0f;
        t_rand[0] = 0.0f;
        t_rand.back() = std::nextafterf(1.0f, 0.0f);
        hm_sample_360(B, N, nearv.data(), farv.data(), nullptr, t_inv.data(), t.data());
        ok &= finite_all(t_inv) & finite_all(t);
        hm_sample_360(B, N, nearv.data(), farv.data(), t_rand.data(), t_inv.data(), t.data());
        ok &= finite_all(t_inv) & finite_all(t);
        const int M = B * N;
        std::vector<float> t0(M), t1(M), d(3 * (size_t)M), o(3 * (size_t)M), r(M), means(3 * (size_t)M), covs(9 * (size_t)M);
        for (int b = 0; b < B; ++b)
            for (int i = 0; i < N; ++i) {
                const int s = b * N + i;
                t0[s] = t[(size_t)b * (N + 1) + i]; t1[s] = t[(size_t)b * (N + 1) + i + 1];
                d[3 * s] = 0.6f; d[3 * s + 1] = -0.64f; d[3 * s + 2] = 0.48f;
                o[3 * s] = 0.1f * b; o[3 * s + 1] = -0.2f; o[3 * s + 2] = 0.3f;
                r[s] = 1e-3f;
            }
        for (const auto& dg : degs) {
            const int L = dg[1] - dg[0];
            std::vector<float> enc((size_t)M * 42 * L), means2(3 * (size_t)M), covs2(9 * (size_t)M), enc2((size_t)M * 42 * L);
            for (int contracted = 0; contracted < 3; ++contracted) {
                hm_cast_ipe_360(M, t0.data(), t1.data(), d.data(), o.data(), r.data(), contracted, dg[0], L, means.data(), covs.data(), enc.data());
                ok &= finite_all(means) & finite_all(covs) & finite_all(enc);
            }
            hm_cast_ipe_360(M, t0.data(), t1.data(), d.data(), o.data(), r.data(), 0, dg[0], L, means.data(), covs.data(), enc.data());
            hm_gauss_360(M, means.data(), covs.data(), 1, dg[0], L, means2.data(), covs2.data(), enc2.data());
            ok &= finite_all(means2) & finite_all(covs2) & finite_all(enc2);
            hm_gauss_360(M, means.data(), covs.data(), 0, dg[0], L, means2.data(), covs2.data(), nullptr);
            ok &= finite_all(means2) & finite_all(covs2);
        }
    }
    const int dims[3] = {5, 4, 3};
    const float lo[3] = {-1.7f, -1.1f, -0.6f}, hi[3] = {1.9f, 1.3f, 1.25f};
    const int first = 7, count = 47;
    std::vector<float> lm(3 * (size_t)count), lc(9 * (size_t)count);
    hm_lattice_gauss_360(dims, lo, hi, first, count, 1.5f, lm.data(), lc.data());
    ok &= finite_all(lm) & finite_all(lc);
    hm_lattice_gauss_360(dims, lo, hi, 59, 1, 0.0f, lm.data(), lc.data());      // the last point alone
    ok &= lm[0] == lo[0] + 4.0f * ((hi[0] - lo[0]) / 4.0f) && lc[0] == 0.0f;
    std::printf(ok ? "ipe360 hostmath selftest: ok\n" : "ipe360 hostmath selftest: FAILED\n");
    return ok ? 0 : 1;
}
