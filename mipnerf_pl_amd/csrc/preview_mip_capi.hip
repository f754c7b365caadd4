// C ABI of libmipnerf_preview_mip.so (include/mipnerf_preview_mip.h): argument checks before any HIP call, then the launcher of
// kernels_preview_mip.hip.  Never allocates, never synchronises.  The checks of one level and its kernel argument are
// preview_field_host.hpp's, the ones mipnerf_preview_march makes.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <string>

#include "../../include/mipnerf_preview_mip.h"
#include "preview_field_host.hpp"
#include "preview_mip.hpp"

namespace mip {
hipError_t launch_preview_mip_march(const PreviewPyramid& pyr, const PreviewMarch& p, float footprint, int degree, int64_t n_rays,
                                    const float* origins, const float* directions, const float* radii, const float* near, const float* far,
                                    float* rgb, float* acc, float* distance, int32_t* steps, float* lod, hipStream_t stream);
}  // namespace mip

namespace {

thread_local std::string g_err;
const char* const kWho = "preview_mip_march: ";

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

}  // namespace

extern "C" {

int mipnerf_preview_mip_abi_version(void) { return 1; }

const char* mipnerf_preview_mip_last_error(void) { return g_err.c_str(); }

int mipnerf_preview_mip_march(const mipnerf_preview_pyramid_t* pyramid, const mipnerf_preview_params_t* params, float footprint,
                              int64_t n_rays, const float* origins, const float* directions, const float* radii, const float* near,
                              const float* far, float* rgb, float* acc, float* distance, int32_t* steps, float* lod, void* stream) {
    using namespace mip;
    if (!pyramid || !params) return fail(PV_E_INVALID, std::string(kWho) + "pyramid and params must not be null");
    const int L = pyramid->levels;
    if (L < 1 || L > kMipMaxLevels) return fail(PV_E_INVALID, std::string(kWho) + "pyramid.levels must lie in 1 .. 8");
    PreviewPyramid pyr;
    memset(&pyr, 0, sizeof(pyr));
    pyr.levels = L;
    for (int l = 0; l < L; ++l) {
        const mipnerf_preview_field_t* field = &pyramid->level[l];
        const std::string who = std::string(kWho) + "level " + std::to_string(l) + ": ";
        const char* why = "";
        if (const int code = preview_field_check(field, &why)) return fail(code, who + why);
        if (memcmp(field->lo, pyramid->level[0].lo, sizeof(field->lo)) != 0 || memcmp(field->hi, pyramid->level[0].hi, sizeof(field->hi)) != 0)
            return fail(PV_E_INVALID, who + "every level spans the box of level 0, bit for bit");
        if (field->degree != pyramid->level[0].degree) return fail(PV_E_INVALID, who + "every level has the degree of level 0");
        pyr.spacing[l] = preview_field_derive(field, &pyr.level[l]);
        if (l > 0 && !(pyr.spacing[l] > pyr.spacing[l - 1]))
            return fail(PV_E_INVALID, who + "the smallest spacing must increase strictly from level to level");
    }
    for (int l = L; l < kMipMaxLevels; ++l) pyr.spacing[l] = pyr.spacing[L - 1];      // never read
    if (!(footprint >= 0.0f) || !isfinite(footprint)) return fail(PV_E_INVALID, std::string(kWho) + "footprint must be finite and >= 0");
    const char* why = "";
    if (const int code = preview_call_check(params, n_rays, &why)) return fail(code, std::string(kWho) + why);
    if (n_rays == 0) return PV_OK;
    if (!origins || !directions || !radii || !near || !far || !rgb || !acc || !distance)
        return fail(PV_E_INVALID, std::string(kWho) + "origins, directions, radii, near, far, rgb, acc and distance must not be null");
    for (int l = 0; l < L; ++l)
        if (!preview_rows_aligned(&pyramid->level[l]))
            return fail(PV_E_INVALID, std::string(kWho) + "level " + std::to_string(l) + ": field.rows must be 16-byte aligned (8 for degree 0)");
    PreviewMarch p;
    if (!preview_march_derive(params, pyr.spacing[0], &p))
        return fail(PV_E_INVALID, std::string(kWho) + "the world step step_scale * s_0 must be positive and finite");
    const hipError_t e = launch_preview_mip_march(pyr, p, footprint, pyramid->level[0].degree, n_rays, origins, directions, radii, near, far, rgb,
                                                  acc, distance, steps, lod, reinterpret_cast<hipStream_t>(stream));
    if (e == hipSuccess) return PV_OK;
    return fail(PV_E_HIP, std::string(kWho) + hipGetErrorString(e));
}

}  // extern "C"
