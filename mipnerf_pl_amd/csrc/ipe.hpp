// Device code of the diagonal integrated positional encoding (models/mip.py:322-350), shared by every kernel that writes
// encoding rows for the MLP kernels (kernels_ray.hip: k_cast_ipe, k_integrated_pos_enc; kernels_mesh.hip: k_lattice_ipe) so that
// they all round the same way.  Include from units compiled with -ffp-contract=off (see raymath.hpp).
#pragma once

#include <hip/hip_runtime.h>

#include "raymath.hpp"

namespace mip {

template <typename OutT> struct Pack;
template <> struct Pack<float> {
    static constexpr int kPer16 = 4;
    __device__ static void store(float* dst, const float* v, int n) {  // n multiple of 4
        for (int i = 0; i < n; i += 4)
            *reinterpret_cast<float4*>(dst + i) = make_float4(v[i], v[i + 1], v[i + 2], v[i + 3]);
    }
};
template <> struct Pack<__bf16> {
    static constexpr int kPer16 = 8;
    __device__ static void store(__bf16* dst, const float* v, int n) {  // n multiple of 8
        typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
        for (int i = 0; i < n; i += 8) {
            bf16x8 p;
#pragma unroll
            for (int j = 0; j < 8; ++j) p[j] = (__bf16)v[i + j];   // RNE
            *reinterpret_cast<bf16x8*>(dst + i) = p;
        }
    }
};

// Accuracy policy per output type: float rows feed the exact-fp32 MLP (parity mode) and use the accurate
// libm sin/exp (<= 1-2 ulp, like torch); bf16 rows are rounded to 8 bits anyway and use the fast pair.
template <typename OutT> struct IpeMath;
template <> struct IpeMath<float> {
    __device__ static float sin(float x) { return sin_accurate(x); }
    __device__ static float exp(float x) { return exp_accurate(x); }
};
template <> struct IpeMath<__bf16> {
    __device__ static float sin(float x) { return sin_fast(x); }
    __device__ static float exp(float x) { return exp_fast(x); }
};

// Thread q in {0,1} of a sample writes degrees [q*L/2, (q+1)*L/2) of both halves (sin | "cos").
template <typename OutT, int L>
__device__ __forceinline__ void ipe_write(const Gauss3& g, int q, int min_deg, OutT* row) {
    constexpr int H = 3 * L / 2;   // features per thread per half
    float fs[H], fc[H];
#pragma unroll
    for (int ll = 0; ll < L / 2; ++ll) {
        const int l = q * (L / 2) + ll;
        const float scale = (float)(1u << (l + min_deg));
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float y = g.mean[a] * scale;
            const float yv = g.cov[a] * (scale * scale);
            const float damp = IpeMath<OutT>::exp(-0.5f * yv);
            fs[ll * 3 + a] = damp * IpeMath<OutT>::sin(y);
            fc[ll * 3 + a] = damp * IpeMath<OutT>::sin(y + kHalfPiF);
        }
    }
    Pack<OutT>::store(row + q * H, fs, H);
    Pack<OutT>::store(row + 3 * L + q * H, fc, H);
}

}  // namespace mip
