// C ABI of libmipnerf_preview_tune_360.so (include/mipnerf_preview_tune_360.h): argument checks before any HIP call, then the launcher of
// kernels_preview_tune_360.hip.  Never allocates, never synchronises.  The checks on the lattice and on the parameters of a march are
// preview_field_host.hpp's, the ones mipnerf_preview_360_march makes; the ones on the loss side are mipnerf_preview_tune_grad's.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>

#include <string>

#include "../../include/mipnerf_preview_tune_360.h"
#include "preview_field_host.hpp"
#include "preview_tune_360.hpp"

namespace mip {
hipError_t launch_preview_360_tune_grad(const PreviewField& f, const PreviewMarch& p, float far_radius, int degree, int64_t n_rays,
                                        const float* origins, const float* directions, const float* near, const float* far,
                                        const float* grad_rgb, const float* target, float loss_scale, const float* grad_acc, float* rgb,
                                        float* acc, float* grad_rows, unsigned long long* counters, hipStream_t stream);
}  // namespace mip

namespace {

thread_local std::string g_err;
using mip::PV_OK;
using mip::PV_E_INVALID;
using mip::PV_E_HIP;

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

inline hipStream_t S(void* s) { return reinterpret_cast<hipStream_t>(s); }

bool aligned(const void* p, uintptr_t to) { return reinterpret_cast<uintptr_t>(p) % to == 0; }

int hip_result(hipError_t e, const char* who) {
    if (e == hipSuccess) return PV_OK;
    return fail(PV_E_HIP, std::string(who) + ": " + hipGetErrorString(e));
}

}  // namespace

extern "C" {

int mipnerf_preview_tune_360_abi_version(void) { return 1; }

const char* mipnerf_preview_tune_360_last_error(void) { return g_err.c_str(); }

int mipnerf_preview_tune_360_grad(const mipnerf_preview_field_t* field, float far_radius, const mipnerf_preview_params_t* params,
                                  int64_t n_rays, const float* origins, const float* directions, const float* near, const float* far,
                                  const float* grad_rgb, const float* target, float loss_scale, const float* grad_acc, float* rgb, float* acc,
                                  float* grad_rows, uint64_t* counters, void* stream) {
    const std::string who = "preview_tune_360_grad: ";
    if (!field || !params) return fail(PV_E_INVALID, who + "field and params must not be null");
    const char* why = "";
    if (const int code = mip::preview_field_check(field, &why)) return fail(code, who + why);
    if (!(far_radius > 1.0f) || !isfinite(far_radius)) return fail(PV_E_INVALID, who + "far_radius must be finite and > 1");
    if (const int code = mip::preview_call_check(params, n_rays, &why)) return fail(code, who + why);
    if ((grad_rgb != nullptr) == (target != nullptr)) return fail(PV_E_INVALID, who + "give exactly one of grad_rgb and target");
    if (target != nullptr && !isfinite(loss_scale)) return fail(PV_E_INVALID, who + "loss_scale must be finite in target mode");
    if (!grad_rows || !aligned(grad_rows, 16)) return fail(PV_E_INVALID, who + "grad_rows must not be null and must be 16-byte aligned");
    if (counters != nullptr && !aligned(counters, 8)) return fail(PV_E_INVALID, who + "counters must be 8-byte aligned");
    if (n_rays == 0) return PV_OK;
    if (!origins || !directions || !near || !far || !rgb || !acc)
        return fail(PV_E_INVALID, who + "origins, directions, near, far, rgb and acc must not be null");
    if (!mip::preview_rows_aligned(field)) return fail(PV_E_INVALID, who + "field.rows must be 16-byte aligned (8 for degree 0)");
    mip::PreviewField f;
    const float hmin = mip::preview_field_derive(field, &f);
    mip::PreviewMarch p;
    if (!mip::preview_march_derive(params, hmin, &p))
        return fail(PV_E_INVALID, who + "the contracted step step_scale * min(h) must be positive and finite");
    return hip_result(mip::launch_preview_360_tune_grad(f, p, far_radius, field->degree, n_rays, origins, directions, near, far, grad_rgb, target,
                                                        loss_scale, grad_acc, rgb, acc, grad_rows,
                                                        reinterpret_cast<unsigned long long*>(counters), S(stream)),
                      "preview_tune_360_grad");
}

}  // extern "C"
