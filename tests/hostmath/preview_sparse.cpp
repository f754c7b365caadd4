// Host build of csrc/preview_sparse.hpp (and, through it, csrc/preview_mip.hpp and csrc/preview_march.hpp) for
// tests/test_preview_sparse_cpu.py:
//   g++ -O2 -ffp-contract=off -shared -fPIC preview_sparse.cpp -o _preview_sparse.so
// The table word by word and in word order (the kernels scan the same popcounts by blocks); the march one ray after the other, one sample
// after the other, in the order of tests/hostmath/preview_mip.cpp, with the level type of the sparse storage.
#include "../../mipnerf_pl_amd/csrc/preview_sparse.hpp"

namespace {

template <int DEG>
void march_ray(const mip::PreviewSparsePyramid& pyr, const mip::PreviewMarch& p, float footprint, const float* o, const float* d, float radius,
               float tn, float tf, float* rgb, float* acc, float* distance, int* steps, float* lod) {
    constexpr int W = mip::preview_row_halves(DEG);
    mip::PreviewRay r;
    if (!mip::mip_radius_ok(radius) || !mip::preview_ray(pyr.level[0], p.s, o, d, tn, tf, &r)) {
        for (int c = 0; c < 3; ++c) rgb[c] = p.background[c];
        *acc = 0.0f;
        *distance = mip::preview_miss_distance(tn, tf);
        *steps = 0;
        *lod = 0.0f;
        return;
    }
    float Y[(DEG + 1) * (DEG + 1)];
    mip::preview_sh_basis<DEG>(r.u, Y);
    const float k = mip::mip_cone_scale(footprint, radius);
    float T = 1.0f, s3[3] = {0.0f, 0.0f, 0.0f}, sa = 0.0f, sd = 0.0f, sl = 0.0f;
    int count = 0;
    for (int i = 0; i < p.max_steps; ++i) {
        const float t = mip::preview_sample_t(r, i);
        if (!(t < r.tb)) break;
        const float x[3] = {o[0] + t * d[0], o[1] + t * d[1], o[2] + t * d[2]};
        int l;
        float g;
        mip::mip_level(pyr.spacing, pyr.levels, mip::mip_footprint(k, t), &l, &g);
        int ca[3], cb[3];
        float fa[3], fb[3];
        mip::lattice_cell(pyr.level[l].box, x, ca, fa);
        bool occupied = mip::preview_occupied(pyr.level[l], ca);
        if (g > 0.0f) {
            mip::lattice_cell(pyr.level[l + 1].box, x, cb, fb);
            occupied = mip::preview_occupied(pyr.level[l + 1], cb) || occupied;
        }
        if (!occupied) continue;
        float row[W];
        mip::preview_row<DEG>(pyr.level[l], ca, fa, row);
        if (g > 0.0f) {
            float upper[W];
            mip::preview_row<DEG>(pyr.level[l + 1], cb, fb, upper);
            mip::mip_mix<W>(row, upper, g);
        }
        float alpha, colour[3];
        mip::preview_shade<DEG>(row, Y, p.s, &alpha, colour);
        const float w = T * alpha;
        for (int ch = 0; ch < 3; ++ch) s3[ch] += w * colour[ch];
        sa += w;
        sd += w * t;
        sl += w * mip::mip_lambda(l, g);
        T *= 1.0f - alpha;
        ++count;
        if (T < p.t_min) break;
    }
    const float rest = 1.0f - sa;
    for (int ch = 0; ch < 3; ++ch) rgb[ch] = s3[ch] + rest * p.background[ch];
    *acc = sa;
    *distance = mip::preview_distance(sd, sa, tn, tf);
    *steps = count;
    *lod = mip::mip_lod(sl, sa);
}

}  // namespace

extern "C" {

int hm_sparse_words_p(int nx) { return mip::sparse_words_p(nx); }

// table [nz, ny, words_p, 2] of occupancy words [nz - 1, ny - 1, words_x]; returns the stored count
long long hm_sparse_table(const unsigned int* occupancy, int nx, int ny, int nz, unsigned int* table) {
    const int words_p = mip::sparse_words_p(nx);
    long long run = 0;
    for (int k = 0; k < nz; ++k)
        for (int j = 0; j < ny; ++j)
            for (int w = 0; w < words_p; ++w) {
                const unsigned int mask = mip::sparse_point_word(occupancy, nx, ny, nz, j, k, w);
                unsigned int* e = table + 2 * (((long long)k * ny + j) * words_p + w);
                e[0] = mask;
                e[1] = (unsigned int)run;
                run += mip::sparse_popc(mask);
            }
    return run;
}

// slot of point (i, j, k) by the lookup rule, -1 when the point is not stored
long long hm_sparse_slot(const unsigned int* table, int nx, int ny, int i, int j, int k) {
    const mip::SparseEntry* e = reinterpret_cast<const mip::SparseEntry*>(table) + ((long long)k * ny + j) * mip::sparse_words_p(nx) + (i >> 5);
    return ((e->mask >> (i & 31)) & 1u) ? (long long)mip::sparse_slot(*e, i) : -1;
}

// rows / occupancy / table / dims: one entry per level (dims as nx, ny, nz triples); rows are compact; radii may be null (every radius 0)
void hm_preview_sparse_march(int levels, const unsigned short* const* rows, const unsigned int* const* occupancy,
                             const unsigned int* const* table, const int* dims, const float* lo, const float* hi, int degree, float footprint,
                             float step_scale, float t_min, int max_steps, const float* background, long long n_rays, const float* origins,
                             const float* directions, const float* radii, const float* near, const float* far, float* rgb, float* acc,
                             float* distance, int* steps, float* lod) {
    mip::PreviewSparsePyramid pyr;
    pyr.levels = levels;
    for (int l = 0; l < levels; ++l) {
        mip::PreviewSparseField& f = pyr.level[l];
        const int* n = dims + 3 * l;
        f.box.nx = n[0]; f.box.ny = n[1]; f.box.nz = n[2];
        float hmin = INFINITY;
        for (int a = 0; a < 3; ++a) {                               // as preview_field_host.hpp forms them
            const float span = hi[a] - lo[a];
            f.box.lo[a] = lo[a];
            f.hi[a] = hi[a];
            f.box.inv_h[a] = (float)(n[a] - 1) / span;
            hmin = fminf(hmin, span / (float)(n[a] - 1));
        }
        f.rows = rows[l];
        f.occ = occupancy[l];
        f.words_x = mip::sparse_words_x(n[0]);
        f.table = reinterpret_cast<const mip::SparseEntry*>(table[l]);
        f.words_p = mip::sparse_words_p(n[0]);
        pyr.spacing[l] = hmin;
    }
    mip::PreviewMarch p;
    p.s = step_scale * pyr.spacing[0];
    p.t_min = t_min;
    p.max_steps = max_steps;
    for (int a = 0; a < 3; ++a) p.background[a] = background[a];
    for (long long b = 0; b < n_rays; ++b) {
        const float *o = origins + 3 * b, *d = directions + 3 * b;
        const float radius = radii ? radii[b] : 0.0f;
        if (degree == 0)
            march_ray<0>(pyr, p, footprint, o, d, radius, near[b], far[b], rgb + 3 * b, acc + b, distance + b, steps + b, lod + b);
        else if (degree == 1)
            march_ray<1>(pyr, p, footprint, o, d, radius, near[b], far[b], rgb + 3 * b, acc + b, distance + b, steps + b, lod + b);
        else
            march_ray<2>(pyr, p, footprint, o, d, radius, near[b], far[b], rgb + 3 * b, acc + b, distance + b, steps + b, lod + b);
    }
}

}  // extern "C"
