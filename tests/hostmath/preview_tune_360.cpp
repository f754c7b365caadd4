// Host build of csrc/preview_tune_360.hpp for tests/test_preview_tune360_cpu.py:
//   g++ -O2 -ffp-contract=off -shared -fPIC preview_tune_360.cpp -o _preview_tune_360.so
// One ray after the other, one sample after the other, one corner after the other, every rule taken from the headers (the kernel spreads
// the same calls over lanes, takes the sums with wave scans and adds with atomics).
#include <vector>

#include "../../mipnerf_pl_amd/csrc/preview_tune_360.hpp"

namespace {

struct Sample {
    int c[3];
    float fr[3];
    float row0, alpha, colour[3], T, delta;
};

template <int DEG>
void grad_ray(const mip::PreviewField& f, const mip::PreviewMarch& p, float R, const float* o, const float* d, float tn, float tf,
              const float* grad_rgb, const float* target, float loss_scale, float g_a, float* rgb, float* acc, float* grad_rows) {
    constexpr int W = mip::preview_row_halves(DEG), NB = mip::preview_basis(DEG);
    mip::PreviewRay360 r;
    if (!mip::preview360_ray(R, o, d, tn, tf, &r)) {
        for (int c = 0; c < 3; ++c) rgb[c] = p.background[c];
        *acc = 0.0f;
        return;
    }
    float Y[NB];
    mip::preview_sh_basis<DEG>(r.u, Y);
    std::vector<Sample> samples;
    float T = 1.0f, sc[3] = {0.0f, 0.0f, 0.0f}, sa = 0.0f;
    for (int i = 0; i < p.max_steps; ++i) {
        const float w = mip::preview360_sample_w(r, p.s, i);
        if (!mip::preview360_exists(r, i, w)) break;
        const float t = mip::preview360_t(r, mip::preview360_unwarp(r, w));
        Sample s;
        if (!mip::tune360_cell(f, o, d, t, s.c, s.fr)) continue;
        if (!mip::preview_occupied(f, s.c)) continue;
        s.delta = mip::tune360_delta(mip::preview360_upper_edge(r, p.s, i - 1), mip::preview360_upper_edge(r, p.s, i));
        float row[W];
        mip::preview_row<DEG>(f, s.c, s.fr, row);
        mip::preview_shade<DEG>(row, Y, s.delta, &s.alpha, s.colour);
        s.row0 = row[0];
        s.T = T;
        const float wt = T * s.alpha;
        for (int ch = 0; ch < 3; ++ch) sc[ch] += wt * s.colour[ch];
        sa += wt;
        T *= 1.0f - s.alpha;
        samples.push_back(s);
        if (T < p.t_min) break;
    }
    const float rest = 1.0f - sa;
    for (int ch = 0; ch < 3; ++ch) rgb[ch] = sc[ch] + rest * p.background[ch];
    *acc = sa;
    float G[3];
    for (int ch = 0; ch < 3; ++ch) G[ch] = grad_rgb ? grad_rgb[ch] : mip::tune_target_grad(loss_scale, rgb[ch], target[ch]);
    if (!mip::tune_ray_ok(rgb, sa, G, g_a)) return;
    const float total = mip::tune_total(G, g_a, sc, sa, p.background);
    const int64_t nx = f.box.nx, ny = f.box.ny;
    float upto = 0.0f;
    for (const Sample& s : samples) {
        const float w = s.T * s.alpha, q = mip::tune_q(G, g_a, s.colour, p.background);
        upto += w * q;
        float drow[W];
        for (int e = 0; e < W; ++e) drow[e] = 0.0f;
        drow[0] = mip::tune360_d_sigma(s.delta, s.T * (1.0f - s.alpha), q, total - upto, s.row0);
        for (int k = 0; k < NB; ++k)
            for (int ch = 0; ch < 3; ++ch) drow[1 + 3 * k + ch] = mip::tune_d_colour(w, G[ch], s.colour[ch]) * Y[k];
        for (int cz = 0; cz < 2; ++cz)
            for (int cy = 0; cy < 2; ++cy)
                for (int cx = 0; cx < 2; ++cx) {
                    float* out = grad_rows + (((s.c[2] + cz) * ny + (s.c[1] + cy)) * nx + (s.c[0] + cx)) * W;
                    const float wt = mip::tune_corner_weight(s.fr, cx, cy, cz);
                    for (int e = 0; e < mip::tune_row_used(DEG); ++e) out[e] += wt * drow[e];
                }
    }
}

}  // namespace

extern "C" {

void hm_preview_tune360_grad(const unsigned short* rows, const unsigned int* occupancy, int nx, int ny, int nz, const float* lo, const float* hi,
                             int degree, float far_radius, float step_scale, float t_min, int max_steps, const float* background,
                             long long n_rays, const float* origins, const float* directions, const float* near, const float* far,
                             const float* grad_rgb, const float* target, float loss_scale, const float* grad_acc, float* rgb, float* acc,
                             float* grad_rows) {
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
        const float* g = grad_rgb ? grad_rgb + 3 * b : nullptr;
        const float* tg = target ? target + 3 * b : nullptr;
        const float ga = grad_acc ? grad_acc[b] : 0.0f;
        if (degree == 0) grad_ray<0>(f, p, far_radius, o, d, near[b], far[b], g, tg, loss_scale, ga, rgb + 3 * b, acc + b, grad_rows);
        else if (degree == 1) grad_ray<1>(f, p, far_radius, o, d, near[b], far[b], g, tg, loss_scale, ga, rgb + 3 * b, acc + b, grad_rows);
        else grad_ray<2>(f, p, far_radius, o, d, near[b], far[b], g, tg, loss_scale, ga, rgb + 3 * b, acc + b, grad_rows);
    }
}

// the header's per-sample functions on n independent samples: delta = tune360_delta(e_lo, e_hi), q (C6), d row[0] (C7), the three colour
// entries before their basis factor (C7) and the 8 corner weights (C8), corner index = 4 cz + 2 cy + cx
void hm_preview_tune360_samples(int n, const float* G, float g_a, const float* background, const float* e_lo, const float* e_hi,
                                const float* colour, const float* w, const float* t_next, const float* rest, const float* row0, const float* fr,
                                float* delta, float* q, float* d_sigma, float* d_colour, float* corner) {
    for (int i = 0; i < n; ++i) {
        delta[i] = mip::tune360_delta(e_lo[i], e_hi[i]);
        q[i] = mip::tune_q(G, g_a, colour + 3 * i, background);
        d_sigma[i] = mip::tune360_d_sigma(delta[i], t_next[i], q[i], rest[i], row0[i]);
        for (int ch = 0; ch < 3; ++ch) d_colour[3 * i + ch] = mip::tune_d_colour(w[i], G[ch], colour[3 * i + ch]);
        for (int k = 0; k < 8; ++k) corner[8 * i + k] = mip::tune_corner_weight(fr + 3 * i, k & 1, (k >> 1) & 1, k >> 2);
    }
}

// C4 / C5 / C8: the cell of z = contract(o + t d) for n ray parameters of one ray: inside [n], c [n, 3], fr [n, 3]
void hm_preview_tune360_cells(int nx, int ny, int nz, const float* lo, const float* hi, const float* o, const float* d, int n, const float* t,
                              int* inside, int* c, float* fr) {
    mip::PreviewField f;
    f.box.nx = nx; f.box.ny = ny; f.box.nz = nz;
    const int dims[3] = {nx, ny, nz};
    for (int a = 0; a < 3; ++a) {
        f.box.lo[a] = lo[a];
        f.hi[a] = hi[a];
        f.box.inv_h[a] = (float)(dims[a] - 1) / (hi[a] - lo[a]);
    }
    for (int i = 0; i < n; ++i) {
        c[3 * i] = c[3 * i + 1] = c[3 * i + 2] = 0;
        fr[3 * i] = fr[3 * i + 1] = fr[3 * i + 2] = 0.0f;
        inside[i] = mip::tune360_cell(f, o, d, t[i], c + 3 * i, fr + 3 * i) ? 1 : 0;
    }
}

}  // extern "C"
