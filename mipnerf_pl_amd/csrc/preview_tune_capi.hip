// C ABI of libmipnerf_preview_tune.so (include/mipnerf_preview_tune.h): argument checks before any HIP call, then the launchers of
// kernels_preview_tune.hip.  Never allocates, never synchronises.  The checks on the lattice and on the parameters of a march are
// preview_field_host.hpp's, the ones mipnerf_preview_march makes.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>

#include <string>

#include "../../include/mipnerf_preview_tune.h"
#include "preview_field_host.hpp"
#include "preview_tune.hpp"

namespace mip {
hipError_t launch_preview_tune_grad(const PreviewField& f, const PreviewMarch& p, int degree, int64_t n_rays, const float* origins,
                                    const float* directions, const float* near, const float* far, const float* grad_rgb, const float* target,
                                    float loss_scale, const float* grad_acc, float* rgb, float* acc, float* grad_rows,
                                    unsigned long long* counters, hipStream_t stream);
hipError_t launch_preview_tune_adam(int64_t n_points, int degree, const TuneAdam& a, float* master, float* m, float* v, float* grad,
                                    uint16_t* rows, const uint8_t* mask, hipStream_t stream);
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

bool aligned(const void* p, uintptr_t to) { return reinterpret_cast<uintptr_t>(p) % to == 0; }

int hip_result(hipError_t e, const char* who) {
    if (e == hipSuccess) return PV_OK;
    return fail(PV_E_HIP, std::string(who) + ": " + hipGetErrorString(e));
}

}  // namespace

extern "C" {

int mipnerf_preview_tune_abi_version(void) { return 1; }

const char* mipnerf_preview_tune_last_error(void) { return g_err.c_str(); }

int mipnerf_preview_tune_grad(const mipnerf_preview_field_t* field, const mipnerf_preview_params_t* params, int64_t n_rays,
                              const float* origins, const float* directions, const float* near, const float* far, const float* grad_rgb,
                              const float* target, float loss_scale, const float* grad_acc, float* rgb, float* acc, float* grad_rows,
                              uint64_t* counters, void* stream) {
    if (!field || !params) return fail(PV_E_INVALID, "preview_tune_grad: field and params must not be null");
    const char* why = "";
    if (const int code = mip::preview_field_check(field, &why)) return fail(code, std::string("preview_tune_grad: ") + why);
    if (const int code = mip::preview_call_check(params, n_rays, &why)) return fail(code, std::string("preview_tune_grad: ") + why);
    if ((grad_rgb != nullptr) == (target != nullptr))
        return fail(PV_E_INVALID, "preview_tune_grad: give exactly one of grad_rgb and target");
    if (target != nullptr && !isfinite(loss_scale)) return fail(PV_E_INVALID, "preview_tune_grad: loss_scale must be finite in target mode");
    if (!grad_rows || !aligned(grad_rows, 16)) return fail(PV_E_INVALID, "preview_tune_grad: grad_rows must not be null and must be 16-byte aligned");
    if (counters != nullptr && !aligned(counters, 8)) return fail(PV_E_INVALID, "preview_tune_grad: counters must be 8-byte aligned");
    if (n_rays == 0) return PV_OK;
    if (!origins || !directions || !near || !far || !rgb || !acc)
        return fail(PV_E_INVALID, "preview_tune_grad: origins, directions, near, far, rgb and acc must not be null");
    if (!mip::preview_rows_aligned(field)) return fail(PV_E_INVALID, "preview_tune_grad: field.rows must be 16-byte aligned (8 for degree 0)");
    mip::PreviewField f;
    const float hmin = mip::preview_field_derive(field, &f);
    mip::PreviewMarch p;
    if (!mip::preview_march_derive(params, hmin, &p))
        return fail(PV_E_INVALID, "preview_tune_grad: the world step step_scale * min(h) must be positive and finite");
    return hip_result(mip::launch_preview_tune_grad(f, p, field->degree, n_rays, origins, directions, near, far, grad_rgb, target, loss_scale,
                                                    grad_acc, rgb, acc, grad_rows, reinterpret_cast<unsigned long long*>(counters), S(stream)),
                      "preview_tune_grad");
}

int mipnerf_preview_tune_adam(int64_t n_points, int32_t degree, float* master, float* m, float* v, float* grad, void* rows,
                              const uint8_t* mask, float lr_sigma, float lr_colour, float beta1, float beta2, float eps, float c1, float c2,
                              void* stream) {
    if (degree < 0 || degree > 2) return fail(PV_E_UNSUPPORTED, "preview_tune_adam: degree must be 0, 1 or 2");
    if (n_points < 0 || n_points > 0x7fffffffll) return fail(PV_E_INVALID, "preview_tune_adam: n_points must lie in [0, 2^31)");
    const float scalars[7] = {lr_sigma, lr_colour, beta1, beta2, eps, c1, c2};
    for (float x : scalars)
        if (!isfinite(x)) return fail(PV_E_INVALID, "preview_tune_adam: the learning rates, betas, eps and bias corrections must be finite");
    if (!(beta1 >= 0.0f && beta1 < 1.0f && beta2 >= 0.0f && beta2 < 1.0f)) return fail(PV_E_INVALID, "preview_tune_adam: the betas must lie in [0, 1)");
    if (!(eps >= 0.0f)) return fail(PV_E_INVALID, "preview_tune_adam: eps must not be negative");
    if (n_points == 0) return PV_OK;
    if (!master || !m || !v || !grad || !rows) return fail(PV_E_INVALID, "preview_tune_adam: master, m, v, grad and rows must not be null");
    if (!aligned(master, 16) || !aligned(m, 16) || !aligned(v, 16) || !aligned(grad, 16) || !aligned(rows, 8))
        return fail(PV_E_INVALID, "preview_tune_adam: master, m, v and grad must be 16-byte aligned, rows 8-byte aligned");
    const mip::TuneAdam a = {lr_sigma, lr_colour, beta1, beta2, eps, c1, c2};
    return hip_result(mip::launch_preview_tune_adam(n_points, degree, a, master, m, v, grad, static_cast<uint16_t*>(rows), mask, S(stream)),
                      "preview_tune_adam");
}

}  // extern "C"
