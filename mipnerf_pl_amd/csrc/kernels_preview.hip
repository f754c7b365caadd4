// libmipnerf_preview.so: the baked-lattice renderer (include/mipnerf_preview.h).  k_preview_pack writes the fp16 rows; the march is the one
// kernel of preview_wave_march.hpp (its mapping is described there), run on a pyramid of one level.
// Compile with -ffp-contract=off (preview_march.hpp).
#include <hip/hip_runtime.h>

#include <string.h>

#include "preview_march.hpp"
#include "preview_wave_march.hpp"

namespace mip {

__global__ void __launch_bounds__(256)
k_preview_pack(const int64_t n, const int degree, const float* __restrict__ sigma, const float* __restrict__ coef,
               const uint8_t* __restrict__ mask, uint16_t* __restrict__ rows) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    preview_pack_row(degree, sigma[i], coef + i * (3 * preview_basis(degree)), mask == nullptr || mask[i] != 0,
                     rows + i * preview_row_halves(degree));
}

// one lattice is a pyramid of one level: footprint 0, no radii, no lod (preview_wave_march.hpp); `hmin` is the field's min(h)
hipError_t launch_preview_march(const PreviewField& f, float hmin, const PreviewMarch& p, int degree, int64_t n_rays, const float* origins,
                                const float* directions, const float* near, const float* far, float* rgb, float* acc, float* distance,
                                int32_t* steps, hipStream_t stream) {
    PreviewPyramid pyr;
    memset(&pyr, 0, sizeof(pyr));
    pyr.levels = 1;
    pyr.level[0] = f;
    for (int l = 0; l < kMipMaxLevels; ++l) pyr.spacing[l] = hmin;      // never read: mip_level returns before it looks when L == 1
    return launch_preview_wave_march(pyr, p, 0.0f, degree, n_rays, origins, directions, nullptr, near, far, rgb, acc, distance, steps, nullptr,
                                     stream);
}

hipError_t launch_preview_pack(int64_t n, int degree, const float* sigma, const float* coef, const uint8_t* mask, uint16_t* rows,
                               hipStream_t stream) {
    hipLaunchKernelGGL(k_preview_pack, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, n, degree, sigma, coef, mask, rows);
    return hipGetLastError();
}

}  // namespace mip
