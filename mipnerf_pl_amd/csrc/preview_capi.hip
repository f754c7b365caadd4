// C ABI of libmipnerf_preview.so (include/mipnerf_preview.h): argument checks before any HIP call, then the launchers of
// kernels_preview.hip.  Never allocates, never synchronises.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>

#include <string>

#include "preview_field_host.hpp"

namespace mip {
hipError_t launch_preview_march(const PreviewField& f, float hmin, const PreviewMarch& p, int degree, int64_t n_rays, const float* origins,
                                const float* directions, const float* near, const float* far, float* rgb, float* acc, float* distance,
                                int32_t* steps, hipStream_t stream);
hipError_t launch_preview_pack(int64_t n, int degree, const float* sigma, const float* coef, const uint8_t* mask, uint16_t* rows,
                               hipStream_t stream);
}  // namespace mip

namespace {

thread_local std::string g_err;
using mip::PV_OK;
using mip::PV_E_INVALID;
using mip::PV_E_UNSUPPORTED;
using mip::PV_E_HIP;

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

inline hipStream_t S(void* s) { return reinterpret_cast<hipStream_t>(s); }

bool dims_ok(const int32_t* dims) { return mip::preview_dims_ok(dims); }

int hip_result(hipError_t e, const char* who) {
    if (e == hipSuccess) return PV_OK;
    return fail(PV_E_HIP, std::string(who) + ": " + hipGetErrorString(e));
}

}  // namespace

extern "C" {

int mipnerf_preview_abi_version(void) { return 1; }

const char* mipnerf_preview_last_error(void) { return g_err.c_str(); }

int mipnerf_preview_pack(const int32_t* dims, int32_t degree, const float* sigma, const float* coef, const uint8_t* mask, void* rows,
                         void* stream) {
    if (!dims || !sigma || !coef || !rows) return fail(PV_E_INVALID, "preview_pack: dims, sigma, coef and rows must not be null");
    if (degree < 0 || degree > 2) return fail(PV_E_UNSUPPORTED, "preview_pack: degree must be 0, 1 or 2");
    if (!dims_ok(dims)) return fail(PV_E_INVALID, "preview_pack: a lattice needs at least 2 points per axis and 7 nx ny nz < 2^31");
    const int64_t n = (int64_t)dims[0] * dims[1] * dims[2];
    return hip_result(mip::launch_preview_pack(n, degree, sigma, coef, mask, static_cast<uint16_t*>(rows), S(stream)), "preview_pack");
}

int mipnerf_preview_march(const mipnerf_preview_field_t* field, const mipnerf_preview_params_t* params, int64_t n_rays,
                          const float* origins, const float* directions, const float* near, const float* far, float* rgb, float* acc,
                          float* distance, int32_t* steps, void* stream) {
    if (!field || !params) return fail(PV_E_INVALID, "preview_march: field and params must not be null");
    const char* why = "";
    if (const int code = mip::preview_field_check(field, &why)) return fail(code, std::string("preview_march: ") + why);
    if (const int code = mip::preview_call_check(params, n_rays, &why)) return fail(code, std::string("preview_march: ") + why);
    if (n_rays == 0) return PV_OK;
    if (!origins || !directions || !near || !far || !rgb || !acc || !distance)
        return fail(PV_E_INVALID, "preview_march: origins, directions, near, far, rgb, acc and distance must not be null");
    if (!mip::preview_rows_aligned(field)) return fail(PV_E_INVALID, "preview_march: field.rows must be 16-byte aligned (8 for degree 0)");
    mip::PreviewField f;
    const float hmin = mip::preview_field_derive(field, &f);
    mip::PreviewMarch p;
    if (!mip::preview_march_derive(params, hmin, &p))
        return fail(PV_E_INVALID, "preview_march: the world step step_scale * min(h) must be positive and finite");
    return hip_result(mip::launch_preview_march(f, hmin, p, field->degree, n_rays, origins, directions, near, far, rgb, acc, distance, steps, S(stream)),
                      "preview_march");
}

}  // extern "C"
