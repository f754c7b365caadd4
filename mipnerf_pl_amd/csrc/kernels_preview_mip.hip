// libmipnerf_preview_mip.so: the baked-lattice renderer over a pyramid of lattices (include/mipnerf_preview_mip.h).  The march is the one
// kernel of preview_wave_march.hpp (the mapping and the level walk are described there); this unit instantiates it for the library.
// Compile with -ffp-contract=off (preview_march.hpp).
#include <hip/hip_runtime.h>

#include "preview_wave_march.hpp"

namespace mip {

hipError_t launch_preview_mip_march(const PreviewPyramid& pyr, const PreviewMarch& p, float footprint, int degree, int64_t n_rays,
                                    const float* origins, const float* directions, const float* radii, const float* near, const float* far,
                                    float* rgb, float* acc, float* distance, int32_t* steps, float* lod, hipStream_t stream) {
    return launch_preview_wave_march(pyr, p, footprint, degree, n_rays, origins, directions, radii, near, far, rgb, acc, distance, steps, lod,
                                     stream);
}

}  // namespace mip
