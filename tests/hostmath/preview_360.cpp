// Host build of csrc/preview_march_360.hpp for tests/test_preview360_cpu.py:
//   g++ -O2 -ffp-contract=off -shared -fPIC preview_360.cpp -o _preview_360.so
// One ray after the other, one sample after the other, every rule taken from the header (the kernel spreads the same calls over lanes).
#include "../../mipnerf_pl_amd/csrc/preview_march_360.hpp"

namespace {

template <int DEG>
void march_ray(const mip::PreviewField& f, const mip::PreviewMarch& p, float R, const float* o, const float* d, float tn, float tf, float* rgb,
               float* acc, float* distance, int* steps) {
    mip::PreviewRay360 r;
    if (!mip::preview360_ray(R, o, d, tn, tf, &r)) {
        for (int c = 0; c < 3; ++c) rgb[c] = p.background[c];
        *acc = 0.0f;
        *distance = mip::preview_miss_distance(tn, tf);
        *steps = 0;
        return;
    }
    float Y[(DEG + 1) * (DEG + 1)];
    mip::preview_sh_basis<DEG>(r.u, Y);
    float T = 1.0f, s3[3] = {0.0f, 0.0f, 0.0f}, sa = 0.0f, sd = 0.0f;
    int count = 0;
    for (int i = 0; i < p.max_steps; ++i) {
        const float w = mip::preview360_sample_w(r, p.s, i);
        if (!mip::preview360_exists(r, i, w)) break;
        const float t = mip::preview360_t(r, mip::preview360_unwarp(r, w));
        const float x[3] = {o[0] + t * d[0], o[1] + t * d[1], o[2] + t * d[2]};
        float z[3];
        mip::preview360_contract(x, z);
        if (!mip::preview360_inside(f, z)) continue;
        int c[3];
        float fr[3];
        mip::lattice_cell(f.box, z, c, fr);
        if (!mip::preview_occupied(f, c)) continue;
        const float delta = fmaxf(mip::preview360_upper_edge(r, p.s, i) - mip::preview360_upper_edge(r, p.s, i - 1), 0.0f);
        float alpha, colour[3];
        mip::preview_sample<DEG>(f, c, fr, Y, delta, &alpha, colour);
        const float wt = T * alpha;
        for (int ch = 0; ch < 3; ++ch) s3[ch] += wt * colour[ch];
        sa += wt;
        sd += wt * t;
        T *= 1.0f - alpha;
        ++count;
        if (T < p.t_min) break;
    }
    const float rest = 1.0f - sa;
    for (int ch = 0; ch < 3; ++ch) rgb[ch] = s3[ch] + rest * p.background[ch];
    *acc = sa;
    *distance = mip::preview_distance(sd, sa, tn, tf);
    *steps = count;
}

}  // namespace

extern "C" {

void hm_preview360_march(const unsigned short* rows, const unsigned int* occupancy, int nx, int ny, int nz, const float* lo, const float* hi,
                         int degree, float far_radius, float step_scale, float t_min, int max_steps, const float* background, long long n_rays,
                         const float* origins, const float* directions, const float* near, const float* far, float* rgb, float* acc,
                         float* distance, int* steps) {
    mip::PreviewField f;
    f.box.nx = nx; f.box.ny = ny; f.box.nz = nz;
    const int dims[3] = {nx, ny, nz};
    float hmin = INFINITY;
    for (int a = 0; a < 3; ++a) {                                   // as preview_field_host.hpp forms them
        const float span = hi[a] - lo[a];
        f.box.lo[a] = lo[a];
        f.hi[a] = hi[a];
        f.box.inv_h[a] = (float)(dims[a] - 1) / span;
        hmin = fminf(hmin, span / (float)(dims[a] - 1));
    }
    f.rows = rows;
    f.occ = occupancy;
    f.words_x = (nx - 1 + 31) / 32;
    mip::PreviewMarch p;
    p.s = step_scale * hmin;
    p.t_min = t_min;
    p.max_steps = max_steps;
    for (int a = 0; a < 3; ++a) p.background[a] = background[a];
    for (long long b = 0; b < n_rays; ++b) {
        const float *o = origins + 3 * b, *d = directions + 3 * b;
        if (degree == 0) march_ray<0>(f, p, far_radius, o, d, near[b], far[b], rgb + 3 * b, acc + b, distance + b, steps + b);
        else if (degree == 1) march_ray<1>(f, p, far_radius, o, d, near[b], far[b], rgb + 3 * b, acc + b, distance + b, steps + b);
        else march_ray<2>(f, p, far_radius, o, d, near[b], far[b], rgb + 3 * b, acc + b, distance + b, steps + b);
    }
}

// C2 - C3 of one ray: 1 = a hit, with consts = (len, tc, p2, p, c, ts, la - tc, lb - tc, wa, wb)
int hm_preview360_ray(float far_radius, const float* o, const float* d, float near, float far, float* consts) {
    mip::PreviewRay360 r;
    if (!mip::preview360_ray(far_radius, o, d, near, far, &r)) return 0;
    const float v[10] = {r.len, r.tc, r.p2, r.p, r.c, r.ts, r.tau_lo, r.tau_hi, r.wa, r.wb};
    for (int k = 0; k < 10; ++k) consts[k] = v[k];
    return 1;
}

// W(tau) and V(W(tau)) of n arclengths on one ray (a hit)
void hm_preview360_roundtrip(float far_radius, const float* o, const float* d, float near, float far, int n, const float* tau, float* w,
                             float* back) {
    mip::PreviewRay360 r;
    if (!mip::preview360_ray(far_radius, o, d, near, far, &r)) return;
    for (int k = 0; k < n; ++k) {
        w[k] = mip::preview360_warp(r, tau[k]);
        back[k] = mip::preview360_unwarp(r, w[k]);
    }
}

// C4 of one ray: the samples that exist (at most `cap`): z [n, 3], t [n], delta [n]; returns n, -1 for a miss
int hm_preview360_samples(float far_radius, float s, int max_steps, const float* o, const float* d, float near, float far, int cap, float* z,
                          float* t, float* delta) {
    mip::PreviewRay360 r;
    if (!mip::preview360_ray(far_radius, o, d, near, far, &r)) return -1;
    int n = 0;
    for (int i = 0; i < max_steps && n < cap; ++i) {
        const float w = mip::preview360_sample_w(r, s, i);
        if (!mip::preview360_exists(r, i, w)) break;
        t[n] = mip::preview360_t(r, mip::preview360_unwarp(r, w));
        const float x[3] = {o[0] + t[n] * d[0], o[1] + t[n] * d[1], o[2] + t[n] * d[2]};
        mip::preview360_contract(x, z + 3 * n);
        delta[n] = fmaxf(mip::preview360_upper_edge(r, s, i) - mip::preview360_upper_edge(r, s, i - 1), 0.0f);
        ++n;
    }
    return n;
}

}  // extern "C"
