// What mipnerf_preview_mip_march (include/mipnerf_preview_mip.h) adds to the per-sample rules of preview_march.hpp, stated ONCE: the
// extra miss test of P2, the footprint of P3, the level rule of P4 and the mix of two blended rows of P5.  MIP_HD like preview_march.hpp:
// the same source is inlined into k_preview_wave_march (preview_wave_march.hpp) and compiled with g++ by tests/hostmath/preview_mip.cpp;
// both with -ffp-contract=off.  The ray, the samples, the cell, the occupancy bit, the row blend and the shading are preview_march.hpp's
// and lattice_sample.hpp's; nothing here restates them.  How a ray's samples and levels are spread over lanes is the kernel's business.
#pragma once

#include "preview_march.hpp"

namespace mip {

constexpr int kMipMaxLevels = 8;

struct PreviewPyramid {          // by-value kernel argument: what the host derives from mipnerf_preview_pyramid_t
    int levels;                  // L
    float spacing[kMipMaxLevels];            // s_l, strictly increasing over the first L entries
    PreviewField level[kMipMaxLevels];
};

// P2's extra miss test
MIP_HD bool mip_radius_ok(float radius) { return preview_finite(radius) && !(radius < 0.0f); }

// P3: k of a ray, w of a sample
MIP_HD float mip_cone_scale(float footprint, float radius) { return footprint * radius; }
MIP_HD float mip_footprint(float k, float t) { return k * t; }

// P4.  `spacing` is read at loop counters only (never at the level found), so a kernel reads it from its arguments with scalar loads.
MIP_HD void mip_level(const float* spacing, int L, float w, int* l, float* g) {
    *l = 0;
    *g = 0.0f;
    if (L == 1 || !(w > spacing[0])) return;            // w <= s_0, or not a number
    if (w >= spacing[L - 1]) {
        *l = L - 1;
        return;
    }
    float sl = spacing[0], sn = spacing[1];
    int lv = 0;
    for (int k = 1; k < L - 1; ++k)
        if (spacing[k] <= w) {
            lv = k;
            sl = spacing[k];
            sn = spacing[k + 1];
        }
    *l = lv;
    *g = (w - sl) / (sn - sl);
}

MIP_HD float mip_lambda(int l, float g) { return (float)l + g; }

// P5: row = (1 - g) * row + g * upper per element; called only when g > 0
template <int W>
MIP_HD void mip_mix(float (&row)[W], const float (&upper)[W], float g) {
    const float keep = 1.0f - g;
#pragma unroll
    for (int e = 0; e < W; ++e) row[e] = keep * row[e] + g * upper[e];
}

// P6: the lod of a ray from its sums
MIP_HD float mip_lod(float lsum, float acc) { return acc == 0.0f ? 0.0f : lsum / acc; }

}  // namespace mip
