// Multi-scale Blender converter on the device: the box pyramid of datasets/convert_blender_data.py:34-37, 65-81 for a batch of
// RGBA8 frames, as (a) the bytes the converter writes to NNN_dj.png and (b) the float32 pixel rows datasets.load_multicam makes of
// those PNGs when it reads them back.
//
//  level 0       v = float(byte) / 255.f                                     (np.array(Image, float32) / 255.)
//  level j + 1   v' = (((p00 + p01) + p10) + p11) / 4.f of the UNQUANTISED float32 level j, p_rc = row r, column c of the 2 x 2 block,
//                every step rounded to float32: the order in which numpy's mean over axes (1, 3) sums
//  bytes         (uint8)(v * 255.f), truncating                              (np.uint8(img * 255))
//  pixel rows    q = float(byte) / 255.f; white background: q_rgb * q_a + (1.f - q_a), three roundings (datasets._composite)
//
// k_pyramid: one thread owns one T x T source block (T = 2^(levels of the pass - 1) <= 8) and streams it row by row: a row is one
// T*4-byte load (two 16-byte loads for T = 8, lanes side by side in the image row), every odd row folds with the saved even row into
// one row of the next level, which is pushed into the same recursion.  All levels of the block stay in registers; nothing is shared
// between threads, so there is no LDS, no barrier, no atomic and no inter-block signalling.  Pyramids deeper than four levels run
// k_pyramid_step per further level over a float32 scratch that the first pass filled with its unquantised last level.
// The kernel is bound by HBM (4 B read, ~1.33 x 16 B written per source pixel).  No allocation, no host synchronisation: capturable.
// Built with -ffp-contract=off (q_rgb * q_a + (1 - q_a) must not fuse).
#include <hip/hip_runtime.h>

#include "kernels.hpp"

namespace mip {
namespace {
constexpr int kThreads = 256;

// where one level of one pass goes
struct PyramidOut {
    unsigned char* u8[4];    // level l of the pass: [n, h >> l, w >> l, 4]
    float* rgb[4];           // level l, image 0, pixel 0 of the [P, 3] rows (null pointers when no rows are wanted)
};

template <int N>
__device__ __forceinline__ void store_words(unsigned int* p, const unsigned int* v) {
    if constexpr (N % 4 == 0) {
#pragma unroll
        for (int i = 0; i < N; i += 4) *reinterpret_cast<uint4*>(p + i) = make_uint4(v[i], v[i + 1], v[i + 2], v[i + 3]);
    } else if constexpr (N % 2 == 0) {
        *reinterpret_cast<uint2*>(p) = make_uint2(v[0], v[1]);
    } else {
        *p = v[0];
    }
}

// N floats to a 4-byte-aligned address: the widest store the address allows (the caller's row offset decides it)
template <int N>
__device__ __forceinline__ void store_floats(float* p, const float* v) {
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    if (N % 4 == 0 && (a & 15) == 0) {
#pragma unroll
        for (int i = 0; i + 3 < N; i += 4) *reinterpret_cast<float4*>(p + i) = make_float4(v[i], v[i + 1], v[i + 2], v[i + 3]);
    } else if (N % 2 == 0 && (a & 7) == 0) {
#pragma unroll
        for (int i = 0; i + 1 < N; i += 2) *reinterpret_cast<float2*>(p + i) = make_float2(v[i], v[i + 1]);
    } else {
#pragma unroll
        for (int i = 0; i < N; ++i) p[i] = v[i];
    }
}

// S pixels (4 floats each) of one row of one level: their bytes and, when wanted, their pixel rows
template <int S>
__device__ __forceinline__ void emit_row(const float* v, unsigned char* u8, float* rgb, int white) {
    unsigned int words[S];
    float px[S * 3];
#pragma unroll
    for (int x = 0; x < S; ++x) {
        unsigned int b[4];
        float q[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            b[c] = (unsigned int)(int)(v[4 * x + c] * 255.0f) & 255u;          // v in [0, 1]: truncation, as np.uint8
            q[c] = __fdiv_rn((float)b[c], 255.0f);
        }
        words[x] = b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24);
#pragma unroll
        for (int c = 0; c < 3; ++c) px[3 * x + c] = white ? q[c] * q[3] + (1.0f - q[3]) : q[c];
    }
    store_words<S>(reinterpret_cast<unsigned int*>(u8), words);
    if (rgb) store_floats<S * 3>(rgb, px);
}

// One level of the streaming recursion: S = pixels per row of this level inside the thread's block, LV = level index in the pass.
template <int S, int LV>
struct Level {
    float even[S * 4];
    Level<S / 2, LV + 1> next;

    // row r (0 .. S-1, a compile-time constant after unrolling) of this level; (y, x) = block coordinates at level 0 of the pass
    __device__ __forceinline__ void push(int r, const float* row, const PyramidOut& o, int64_t img, int by, int bx, int h, int w, int64_t ppi,
                                         int white, float* carry) {
        const int hl = h >> LV, wl = w >> LV;
        const int64_t pix = (int64_t)(by * S + r) * wl + (int64_t)bx * S;
        if (o.u8[LV])
            emit_row<S>(row, o.u8[LV] + ((img * hl * wl + pix) << 2), o.rgb[LV] ? o.rgb[LV] + (img * ppi + pix) * 3 : nullptr, white);
        if constexpr (S > 1) {
            if ((r & 1) == 0) {
#pragma unroll
                for (int i = 0; i < S * 4; ++i) even[i] = row[i];
            } else {
                float down[S * 2];
#pragma unroll
                for (int x = 0; x < S / 2; ++x)
#pragma unroll
                    for (int c = 0; c < 4; ++c)
                        down[4 * x + c] = (((even[8 * x + c] + even[8 * x + 4 + c]) + row[8 * x + c]) + row[8 * x + 4 + c]) * 0.25f;
                next.push(r >> 1, down, o, img, by, bx, h, w, ppi, white, carry);
            }
        } else if (carry) {
            // the unquantised last level of the pass, for k_pyramid_step: [n, h >> LV, w >> LV, 4]
            *reinterpret_cast<float4*>(carry + ((img * hl * wl + pix) << 2)) = make_float4(row[0], row[1], row[2], row[3]);
        }
    }
};

template <int LV>
struct Level<0, LV> {
    __device__ __forceinline__ void push(int, const float*, const PyramidOut&, int64_t, int, int, int, int, int64_t, int, float*) {}
};

template <int T>
__device__ __forceinline__ void load_row(const unsigned char* p, unsigned int* words) {
    if constexpr (T == 8) {
        const uint4 a = reinterpret_cast<const uint4*>(p)[0], b = reinterpret_cast<const uint4*>(p)[1];
        words[0] = a.x; words[1] = a.y; words[2] = a.z; words[3] = a.w;
        words[4] = b.x; words[5] = b.y; words[6] = b.z; words[7] = b.w;
    } else if constexpr (T == 4) {
        const uint4 a = *reinterpret_cast<const uint4*>(p);
        words[0] = a.x; words[1] = a.y; words[2] = a.z; words[3] = a.w;
    } else if constexpr (T == 2) {
        const uint2 a = *reinterpret_cast<const uint2*>(p);
        words[0] = a.x; words[1] = a.y;
    } else {
        words[0] = *reinterpret_cast<const unsigned int*>(p);
    }
}
}  // namespace

// src [n, h, w, 4] bytes; h, w multiples of T; one thread per T x T block, blocks of one image row side by side in a wave
template <int T>
__global__ void __launch_bounds__(kThreads) k_pyramid(int64_t nblocks, int h, int w, int64_t ppi, const unsigned char* __restrict__ src, PyramidOut o,
                                                      int white, float* __restrict__ carry) {
    const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (t >= nblocks) return;
    const int bw = w / T, bh = h / T;
    const int bx = (int)(t % bw), by = (int)((t / bw) % bh);
    const int64_t img = t / ((int64_t)bw * bh);
    const unsigned char* base = src + (((img * h + (int64_t)by * T) * w + (int64_t)bx * T) << 2);
    Level<T, 0> pyr;
#pragma unroll
    for (int r = 0; r < T; ++r) {
        unsigned int words[T];
        load_row<T>(base + (((int64_t)r * w) << 2), words);
        float row[T * 4];
#pragma unroll
        for (int x = 0; x < T; ++x)
#pragma unroll
            for (int c = 0; c < 4; ++c) row[4 * x + c] = __fdiv_rn((float)((words[x] >> (8 * c)) & 255u), 255.0f);
        pyr.push(r, row, o, img, by, bx, h, w, ppi, white, carry);
    }
}

// One further level: prev [n, 2h, 2w, 4] unquantised float32 -> level (h, w): bytes, pixel rows and (next != null) its unquantised values
__global__ void __launch_bounds__(kThreads) k_pyramid_step(int64_t npix, int h, int w, int64_t ppi, const float* __restrict__ prev, unsigned char* __restrict__ u8,
                                                           float* __restrict__ rgb, int white, float* __restrict__ next) {
    const int64_t t = (int64_t)blockIdx.x * kThreads + threadIdx.x;
    if (t >= npix) return;
    const int x = (int)(t % w), y = (int)((t / w) % h);
    const int64_t img = t / ((int64_t)w * h);
    const float4* p = reinterpret_cast<const float4*>(prev) + (img * 2 * h + 2 * y) * (2 * (int64_t)w) + 2 * x;
    const float4 p00 = p[0], p01 = p[1], p10 = p[2 * w], p11 = p[2 * w + 1];
    float v[4] = {(((p00.x + p01.x) + p10.x) + p11.x) * 0.25f, (((p00.y + p01.y) + p10.y) + p11.y) * 0.25f,
                  (((p00.z + p01.z) + p10.z) + p11.z) * 0.25f, (((p00.w + p01.w) + p10.w) + p11.w) * 0.25f};
    const int64_t pix = (int64_t)y * w + x;
    emit_row<1>(v, u8 + (t << 2), rgb ? rgb + (img * ppi + pix) * 3 : nullptr, white);
    if (next) reinterpret_cast<float4*>(next)[t] = make_float4(v[0], v[1], v[2], v[3]);
}

static int64_t pyramid_pixels_per_image(int h, int w, int n_levels) {
    int64_t p = 0;
    for (int j = 0; j < n_levels; ++j) p += (int64_t)(h >> j) * (w >> j);
    return p;
}

hipError_t launch_box_pyramid(int64_t n, int h, int w, int n_levels, const unsigned char* src, unsigned char* out_u8, float* out_rgb, int white,
                              float* scratch, hipStream_t st) {
    const int64_t ppi = pyramid_pixels_per_image(h, w, n_levels);
    const int first = n_levels < 4 ? n_levels : 4;          // levels of the register pass
    PyramidOut o = {};
    int64_t u8_off = 0, row_off = 0;                        // bytes before level j of out_u8; pixel rows before level j inside one image
    for (int j = 0; j < first; ++j) {
        o.u8[j] = out_u8 + u8_off;
        o.rgb[j] = out_rgb ? out_rgb + row_off * 3 : nullptr;
        u8_off += n * 4 * (int64_t)(h >> j) * (w >> j);
        row_off += (int64_t)(h >> j) * (w >> j);
    }
    float* carry = n_levels > 4 ? scratch : nullptr;
    const int T = 1 << (first - 1);
    const int64_t nblocks = n * (h / T) * (w / T);
    const dim3 grid((unsigned)((nblocks + kThreads - 1) / kThreads)), block(kThreads);
    switch (first) {
        case 1: hipLaunchKernelGGL(k_pyramid<1>, grid, block, 0, st, nblocks, h, w, ppi, src, o, white, carry); break;
        case 2: hipLaunchKernelGGL(k_pyramid<2>, grid, block, 0, st, nblocks, h, w, ppi, src, o, white, carry); break;
        case 3: hipLaunchKernelGGL(k_pyramid<4>, grid, block, 0, st, nblocks, h, w, ppi, src, o, white, carry); break;
        default: hipLaunchKernelGGL(k_pyramid<8>, grid, block, 0, st, nblocks, h, w, ppi, src, o, white, carry); break;
    }
    // level 3 and level 4 of the scratch; the later levels ping-pong between the two
    float* bufs[2] = {scratch, scratch ? scratch + n * 4 * (int64_t)(h >> 3) * (w >> 3) : nullptr};
    for (int j = 4; j < n_levels; ++j) {
        const int hj = h >> j, wj = w >> j;
        const int64_t npix = n * hj * wj;
        hipLaunchKernelGGL(k_pyramid_step, dim3((unsigned)((npix + kThreads - 1) / kThreads)), block, 0, st, npix, hj, wj, ppi, bufs[j & 1],
                           out_u8 + u8_off, out_rgb ? out_rgb + row_off * 3 : nullptr, white, j + 1 < n_levels ? bufs[(j + 1) & 1] : nullptr);
        u8_off += npix * 4;
        row_off += (int64_t)hj * wj;
    }
    return hipGetLastError();
}
}  // namespace mip
