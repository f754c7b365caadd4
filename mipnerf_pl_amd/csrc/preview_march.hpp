// The per-sample rules of mipnerf_preview_march (include/mipnerf_preview.h), stated ONCE.  MIP_HD like raymath.hpp: the same source is
// inlined into k_preview_wave_march (preview_wave_march.hpp) and compiled with g++ by tests/hostmath/preview.cpp; both with -ffp-contract=off, so
// every product and sum below rounds once, as written.  The cell index and the trilinear fractions are lattice_sample.hpp's
// (lattice_cell); nothing here restates them.  How the samples of a ray are spread over lanes is the kernel's business, not this file's.
// preview_mip.hpp (mipnerf_preview_mip_march) builds on this file: it calls preview_row and preview_shade, the two halves of
// preview_sample, with its own mix of two rows in between.
#pragma once

#include <string.h>

#include "lattice_sample.hpp"

namespace mip {

constexpr float kShC0 = 0.28209479177387814f;
constexpr float kShC1 = 0.4886025119029199f;
constexpr float kShC2[5] = {1.0925484305920792f, -1.0925484305920792f, 0.31539156525252005f, -1.0925484305920792f, 0.5462742152960396f};
constexpr float kHalfMax = 65504.0f;

MIP_HD constexpr int preview_row_halves(int degree) { return degree == 0 ? 4 : degree == 1 ? 16 : 32; }
MIP_HD constexpr int preview_basis(int degree) { return (degree + 1) * (degree + 1); }

struct PreviewField {        // by-value kernel argument: what the host derives from mipnerf_preview_field_t
    LatticeBox box;
    float hi[3];
    const uint16_t* rows;    // fp16 bits [nz, ny, nx, W]
    const uint32_t* occ;     // [nz - 1, ny - 1, words_x] or nullptr
    int words_x;             // ceil((nx - 1) / 32)
};

struct PreviewMarch {        // by-value kernel argument: mipnerf_preview_params_t plus the world step s of rule 1
    float s;
    float t_min;
    int max_steps;
    float background[3];
};

struct PreviewRay {          // a ray after rules 1 - 2
    float ta, tb, dt;
    float u[3];              // d / |d|
};

// fp16 bits -> fp32, exact
MIP_HD float half_bits_to_float(uint16_t h) {
#if defined(__HIP_DEVICE_COMPILE__)
    _Float16 x;
    __builtin_memcpy(&x, &h, 2);
    return (float)x;
#else
    const uint32_t sign = (uint32_t)(h & 0x8000u) << 16, e = (h >> 10) & 31u, m = h & 1023u;
    uint32_t bits;
    if (e == 31u) {
        bits = sign | 0x7f800000u | (m << 13);
    } else if (e != 0u) {
        bits = sign | ((e + 112u) << 23) | (m << 13);
    } else {
        const float v = ldexpf((float)m, -24);      // zero and the subnormals
        memcpy(&bits, &v, 4);
        bits |= sign;
    }
    float out;
    memcpy(&out, &bits, 4);
    return out;
#endif
}

MIP_HD bool preview_finite(float v) { return fabsf(v) <= 3.4028234663852886e38f; }      // NaN fails the comparison too

// rule 2's distance of a miss
MIP_HD float preview_miss_distance(float near, float far) { return preview_finite(near) ? near : preview_finite(far) ? far : 0.0f; }

// rules 1 - 2: false = a miss
MIP_HD bool preview_ray(const PreviewField& f, float s, const float o[3], const float d[3], float near, float far, PreviewRay* r) {
    if (!(preview_finite(near) && preview_finite(far)) || !(far > near)) return false;
    float ta = near, tb = far;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        if (!(preview_finite(o[a]) && preview_finite(d[a]))) return false;
        if (d[a] == 0.0f) {
            if (!(o[a] >= f.box.lo[a] && o[a] <= f.hi[a])) return false;
        } else {
            const float t0 = (f.box.lo[a] - o[a]) / d[a], t1 = (f.hi[a] - o[a]) / d[a];
            ta = fmaxf(ta, fminf(t0, t1));
            tb = fminf(tb, fmaxf(t0, t1));
        }
    }
    const float len = sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    if (!(len > 0.0f) || !preview_finite(len) || !(ta < tb)) return false;
    r->ta = ta;
    r->tb = tb;
    r->dt = s / len;
#pragma unroll
    for (int a = 0; a < 3; ++a) r->u[a] = d[a] / len;
    return true;
}

template <int DEG>
MIP_HD void preview_sh_basis(const float u[3], float (&Y)[(DEG + 1) * (DEG + 1)]) {
    const float x = u[0], y = u[1], z = u[2];
    Y[0] = kShC0;
    if constexpr (DEG >= 1) {
        Y[1] = -kShC1 * y;
        Y[2] = kShC1 * z;
        Y[3] = -kShC1 * x;
    }
    if constexpr (DEG >= 2) {
        const float xx = x * x, yy = y * y, zz = z * z;
        Y[4] = kShC2[0] * (x * y);
        Y[5] = kShC2[1] * (y * z);
        Y[6] = kShC2[2] * ((2.0f * zz - xx) - yy);
        Y[7] = kShC2[3] * (x * z);
        Y[8] = kShC2[4] * (xx - yy);
    }
}

// rule 3: sample i of a ray
MIP_HD float preview_sample_t(const PreviewRay& r, int i) { return r.ta + ((float)i + 0.5f) * r.dt; }

// rule 4's occupancy bit of cell c (inside the box: lattice_cell clamps)
MIP_HD bool preview_occupied(const PreviewField& f, const int c[3]) {
    if (f.occ == nullptr) return true;
    const uint32_t w = f.occ[((int64_t)c[2] * (f.box.ny - 1) + c[1]) * f.words_x + (c[0] >> 5)];
    return (w >> (c[0] & 31)) & 1u;
}

template <int N>
struct alignas(2 * N) HalfChunk {      // N = 4: one 8-byte load; N = 8: one 16-byte load
    uint16_t h[N];
};

// how a row of degree DEG is loaded: CH chunks of N halves
template <int DEG>
struct PreviewRowChunks {
    static constexpr int W = preview_row_halves(DEG), N = W < 8 ? W : 8, CH = W / N;
    typedef HalfChunk<N> Chunk;
};

// rule 4 on an occupied cell, first half: the trilinear blend of the 8 corner rows, whatever the storage.  q00, q10, q01, q11: the row of
// the cell's low-x corner on its four x-lines (y, z), (y + 1, z), (y, z + 1), (y + 1, z + 1); the high-x corner's row is the NEXT row of
// the same line in both storages (dense: the next lattice point; compact: preview_sparse.hpp's invariant).
template <int DEG>
MIP_HD void preview_blend(const typename PreviewRowChunks<DEG>::Chunk* q00, const typename PreviewRowChunks<DEG>::Chunk* q10,
                          const typename PreviewRowChunks<DEG>::Chunk* q01, const typename PreviewRowChunks<DEG>::Chunk* q11,
                          const float fr[3], float (&row)[preview_row_halves(DEG)]) {
    constexpr int N = PreviewRowChunks<DEG>::N, CH = PreviewRowChunks<DEG>::CH;
    typedef typename PreviewRowChunks<DEG>::Chunk Chunk;
    const float gx = 1.0f - fr[0], gy = 1.0f - fr[1], gz = 1.0f - fr[2];
#pragma unroll
    for (int k = 0; k < CH; ++k) {
        // the 8 corner loads of this chunk first, then the blend
        const Chunk v000 = q00[k], v100 = q00[CH + k], v010 = q10[k], v110 = q10[CH + k];
        const Chunk v001 = q01[k], v101 = q01[CH + k], v011 = q11[k], v111 = q11[CH + k];
#pragma unroll
        for (int e = 0; e < N; ++e) {
            const float v00 = gx * half_bits_to_float(v000.h[e]) + fr[0] * half_bits_to_float(v100.h[e]);
            const float v10 = gx * half_bits_to_float(v010.h[e]) + fr[0] * half_bits_to_float(v110.h[e]);
            const float v01 = gx * half_bits_to_float(v001.h[e]) + fr[0] * half_bits_to_float(v101.h[e]);
            const float v11 = gx * half_bits_to_float(v011.h[e]) + fr[0] * half_bits_to_float(v111.h[e]);
            const float v0 = gy * v00 + fr[1] * v10;
            const float v1 = gy * v01 + fr[1] * v11;
            row[k * N + e] = gz * v0 + fr[2] * v1;
        }
    }
}

// the dense storage's addresses: point (i, j, k) has the row (k * ny + j) * nx + i
template <int DEG>
MIP_HD void preview_row(const PreviewField& f, const int c[3], const float fr[3], float (&row)[preview_row_halves(DEG)]) {
    constexpr int CH = PreviewRowChunks<DEG>::CH;
    typedef typename PreviewRowChunks<DEG>::Chunk Chunk;
    const int64_t sy = (int64_t)f.box.nx * CH, sz = sy * f.box.ny;        // in chunks
    const Chunk* q = reinterpret_cast<const Chunk*>(f.rows) + (((int64_t)c[2] * f.box.ny + c[1]) * f.box.nx + c[0]) * CH;
    preview_blend<DEG>(q, q + sy, q + sz, q + sz + sy, fr, row);
}

// rule 4, second half: a blended row's alpha and clamped colour
template <int DEG>
MIP_HD void preview_shade(const float (&row)[preview_row_halves(DEG)], const float (&Y)[(DEG + 1) * (DEG + 1)], float s, float* alpha,
                          float colour[3]) {
    constexpr int NB = preview_basis(DEG);
    const float sigma = row[0] < 0.0f ? 0.0f : row[0];          // a NaN stays a NaN
    *alpha = 1.0f - expf(-(sigma * s));
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        float v = 0.0f;
#pragma unroll
        for (int k = 0; k < NB; ++k) v += row[1 + 3 * k + ch] * Y[k];
        colour[ch] = v < 0.0f ? 0.0f : v > 1.0f ? 1.0f : v;     // a NaN stays a NaN
    }
}

// rule 4 on an occupied cell: both halves, in this order
template <int DEG>
MIP_HD void preview_sample(const PreviewField& f, const int c[3], const float fr[3], const float (&Y)[(DEG + 1) * (DEG + 1)], float s,
                           float* alpha, float colour[3]) {
    float row[preview_row_halves(DEG)];
    preview_row<DEG>(f, c, fr, row);
    preview_shade<DEG>(row, Y, s, alpha, colour);
}

// rule 6
MIP_HD float preview_distance(float dsum, float acc, float near, float far) {
    if (acc == 0.0f) return near;
    const float q = dsum / acc;
    return q != q ? q : fminf(fmaxf(q, near), far);
}

// fp32 -> fp16 bits of a row entry: round to nearest even, NaN stays NaN; `saturate`: a value above the fp16 maximum is stored as it
MIP_HD uint16_t preview_half_bits(float v, bool saturate) {
    if (saturate && v > kHalfMax) v = kHalfMax;
#if defined(__HIP_DEVICE_COMPILE__)
    const _Float16 x = (_Float16)v;
    uint16_t h;
    __builtin_memcpy(&h, &x, 2);
    return h;
#else
    uint32_t b;
    memcpy(&b, &v, 4);
    const uint32_t sign = (b >> 16) & 0x8000u, a = b & 0x7fffffffu;
    if (a > 0x7f800000u) return (uint16_t)(sign | 0x7e00u);                       // NaN
    if (a >= 0x477ff000u) return (uint16_t)(sign | 0x7c00u);                      // >= 65520 (and inf): inf
    if (a < 0x33000001u) return (uint16_t)sign;                                   // <= 2^-25: zero
    const int e = (int)(a >> 23) - 127;
    uint32_t m = (a & 0x7fffffu) | 0x800000u;
    const int shift = e < -14 ? 13 + (-14 - e) : 13;                              // subnormals lose more bits
    const uint32_t half = 1u << (shift - 1), rest = m & ((1u << shift) - 1u);
    m >>= shift;
    if (rest > half || (rest == half && (m & 1u))) ++m;
    const uint32_t base = e < -14 ? 0u : (uint32_t)(e + 15 - 1) << 10;            // m still carries the hidden bit when normal
    return (uint16_t)(sign | (base + m));
#endif
}

// one packed row (the ROWS paragraph of mipnerf_preview.h) from a point's sigma and its 3 (degree + 1)^2 coefficients; `keep` false: the
// colour coefficients are written as zeros
MIP_HD void preview_pack_row(int degree, float sigma, const float* cf, bool keep, uint16_t* row) {
    const int W = preview_row_halves(degree), used = 3 * preview_basis(degree);
    row[0] = preview_half_bits(sigma, true);
    for (int k = 0; k < used; ++k) row[1 + k] = keep ? preview_half_bits(cf[k], false) : (uint16_t)0;
    for (int k = 1 + used; k < W; ++k) row[k] = 0;
}

}  // namespace mip
