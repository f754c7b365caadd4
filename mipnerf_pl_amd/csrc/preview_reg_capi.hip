// C ABI of libmipnerf_preview_reg.so (include/mipnerf_preview_reg.h): argument checks before any HIP call, then the launcher of
// kernels_preview_reg.hip.  Never allocates, never synchronises.  The rule for the lattice sizes is preview_field_host.hpp's, the one
// every preview entry point applies.
#include <hip/hip_runtime.h>
#include <math.h>

#include <string>

#include "../../include/mipnerf_preview_reg.h"
#include "preview_field_host.hpp"
#include "preview_reg.hpp"

namespace mip {
hipError_t launch_preview_reg_grad(const PreviewReg& p, int degree, const float* master, const uint8_t* mask, float* grad, hipStream_t stream);
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

bool aligned(const void* p, uintptr_t to) { return reinterpret_cast<uintptr_t>(p) % to == 0; }

}  // namespace

extern "C" {

int mipnerf_preview_reg_abi_version(void) { return 1; }

const char* mipnerf_preview_reg_last_error(void) { return g_err.c_str(); }

int mipnerf_preview_reg_grad(const int32_t* dims, int32_t degree, const float* scale, const float* master, const uint8_t* mask, float* grad,
                             float w_sigma, float w_colour, float w_view, float eps, void* stream) {
    if (!dims || !scale) return fail(PV_E_INVALID, "preview_reg_grad: dims and scale must not be null");
    if (degree < 0 || degree > 2) return fail(PV_E_UNSUPPORTED, "preview_reg_grad: degree must be 0, 1 or 2");
    const bool empty = dims[0] >= 0 && dims[1] >= 0 && dims[2] >= 0 && (dims[0] == 0 || dims[1] == 0 || dims[2] == 0);
    if (!empty && !mip::preview_dims_ok(dims))
        return fail(PV_E_INVALID, "preview_reg_grad: a lattice needs at least 2 points per axis and 7 nx ny nz < 2^31");
    for (int a = 0; a < 3; ++a)
        if (!(scale[a] > 0.0f) || !isfinite(scale[a])) return fail(PV_E_INVALID, "preview_reg_grad: the axis scales must be positive and finite");
    const float weights[3] = {w_sigma, w_colour, w_view};
    for (float w : weights)
        if (!(w >= 0.0f) || !isfinite(w)) return fail(PV_E_INVALID, "preview_reg_grad: the weights must be finite and >= 0");
    if (!(eps > 0.0f) || !isfinite(eps)) return fail(PV_E_INVALID, "preview_reg_grad: eps must be finite and > 0");
    if (empty) return PV_OK;
    if (!master || !grad) return fail(PV_E_INVALID, "preview_reg_grad: master and grad must not be null");
    if (!aligned(master, 16) || !aligned(grad, 16)) return fail(PV_E_INVALID, "preview_reg_grad: master and grad must be 16-byte aligned");
    if (w_sigma == 0.0f && w_colour == 0.0f && w_view == 0.0f) return PV_OK;      // nothing to add: no launch
    const mip::PreviewReg p = {dims[0], dims[1], dims[2], {scale[0], scale[1], scale[2]}, w_sigma, w_colour, w_view, eps};
    const hipError_t e = mip::launch_preview_reg_grad(p, degree, master, mask, grad, reinterpret_cast<hipStream_t>(stream));
    if (e == hipSuccess) return PV_OK;
    return fail(PV_E_HIP, std::string("preview_reg_grad: ") + hipGetErrorString(e));
}

}  // extern "C"
