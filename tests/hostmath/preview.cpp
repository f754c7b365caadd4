// Host build of csrc/preview_march.hpp for tests/test_preview_cpu.py:
//   g++ -O2 -ffp-contract=off -shared -fPIC preview.cpp -o _preview.so
// One ray after the other, one sample after the other, every rule taken from the header (the kernel spreads the same calls over lanes).
#include "../../mipnerf_pl_amd/csrc/preview_march.hpp"

namespace {

template <int DEG>
void march_ray(const mip::PreviewField& f, const mip::PreviewMarch& p, const float* o, const float* d, float tn, float tf, float* rgb,
               float* acc, float* distance, int* steps) {
    mip::PreviewRay r;
    if (!mip::preview_ray(f, p.s, o, d, tn, tf, &r)) {
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
        const float t = mip::preview_sample_t(r, i);
        if (!(t < r.tb)) break;
        const float x[3] = {o[0] + t * d[0], o[1] + t * d[1], o[2] + t * d[2]};
        int c[3];
        float fr[3];
        mip::lattice_cell(f.box, x, c, fr);
        if (!mip::preview_occupied(f, c)) continue;
        float alpha, colour[3];
        mip::preview_sample<DEG>(f, c, fr, Y, p.s, &alpha, colour);
        const float w = T * alpha;
        for (int ch = 0; ch < 3; ++ch) s3[ch] += w * colour[ch];
        sa += w;
        sd += w * t;
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

void hm_preview_march(const unsigned short* rows, const unsigned int* occupancy, int nx, int ny, int nz, const float* lo, const float* hi,
                      int degree, float step_scale, float t_min, int max_steps, const float* background, long long n_rays,
                      const float* origins, const float* directions, const float* near, const float* far, float* rgb, float* acc,
                      float* distance, int* steps) {
    mip::PreviewField f;
    f.box.nx = nx; f.box.ny = ny; f.box.nz = nz;
    const int dims[3] = {nx, ny, nz};
    float hmin = INFINITY;
    for (int a = 0; a < 3; ++a) {                                   // as preview_capi.hip forms them
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
        if (degree == 0) march_ray<0>(f, p, o, d, near[b], far[b], rgb + 3 * b, acc + b, distance + b, steps + b);
        else if (degree == 1) march_ray<1>(f, p, o, d, near[b], far[b], rgb + 3 * b, acc + b, distance + b, steps + b);
        else march_ray<2>(f, p, o, d, near[b], far[b], rgb + 3 * b, acc + b, distance + b, steps + b);
    }
}

void hm_preview_half_bits(long long n, const float* v, int saturate, unsigned short* out) {
    for (long long i = 0; i < n; ++i) out[i] = mip::preview_half_bits(v[i], saturate != 0);
}

void hm_preview_half_to_float(long long n, const unsigned short* h, float* out) {
    for (long long i = 0; i < n; ++i) out[i] = mip::half_bits_to_float(h[i]);
}

}  // extern "C"
