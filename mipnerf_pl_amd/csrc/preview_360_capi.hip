// C ABI of libmipnerf_preview_360.so (include/mipnerf_preview_360.h): argument checks before any HIP call, then the launchers of
// kernels_preview_360.hip.  Never allocates, never synchronises.  The checks of a lattice and of a call, and the kernel arguments derived
// from them, are preview_field_host.hpp's, the ones mipnerf_preview_march and mipnerf_preview_sparse_march make.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <string>

#include "../../include/mipnerf_preview_360.h"
#include "preview_field_host.hpp"
#include "preview_sparse.hpp"

namespace mip {
hipError_t launch_preview_march_360(const PreviewField& f, const PreviewMarch& p, float far_radius, int degree, int64_t n_rays,
                                    const float* origins, const float* directions, const float* near, const float* far, float* rgb,
                                    float* acc, float* distance, int32_t* steps, hipStream_t stream);
hipError_t launch_preview_march_360_sparse(const PreviewSparseField& f, const PreviewMarch& p, float far_radius, int degree, int64_t n_rays,
                                           const float* origins, const float* directions, const float* near, const float* far, float* rgb,
                                           float* acc, float* distance, int32_t* steps, hipStream_t stream);
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

int hip_result(hipError_t e, const char* who) {
    if (e == hipSuccess) return PV_OK;
    return fail(PV_E_HIP, std::string(who) + ": " + hipGetErrorString(e));
}

// everything both entry points check after the field itself; PV_OK with *go = false: n_rays == 0, nothing to launch
int call_check(const std::string& who, const mipnerf_preview_field_t* field, float far_radius, const mipnerf_preview_params_t* params,
               int64_t n_rays, const float* origins, const float* directions, const float* near, const float* far, const float* rgb,
               const float* acc, const float* distance, mip::PreviewField* f, mip::PreviewMarch* p, bool* go) {
    *go = false;
    if (!(far_radius > 1.0f) || !isfinite(far_radius)) return fail(PV_E_INVALID, who + "far_radius must be finite and > 1");
    const char* why = "";
    if (const int code = mip::preview_call_check(params, n_rays, &why)) return fail(code, who + why);
    if (n_rays == 0) return PV_OK;
    if (!origins || !directions || !near || !far || !rgb || !acc || !distance)
        return fail(PV_E_INVALID, who + "origins, directions, near, far, rgb, acc and distance must not be null");
    if (!mip::preview_rows_aligned(field)) return fail(PV_E_INVALID, who + "field.rows must be 16-byte aligned (8 for degree 0)");
    const float hmin = mip::preview_field_derive(field, f);
    if (!mip::preview_march_derive(params, hmin, p))
        return fail(PV_E_INVALID, who + "the contracted step step_scale * min(h) must be positive and finite");
    *go = true;
    return PV_OK;
}

}  // namespace

extern "C" {

int mipnerf_preview_360_abi_version(void) { return 1; }

const char* mipnerf_preview_360_last_error(void) { return g_err.c_str(); }

int mipnerf_preview_360_march(const mipnerf_preview_field_t* field, float far_radius, const mipnerf_preview_params_t* params, int64_t n_rays,
                              const float* origins, const float* directions, const float* near, const float* far, float* rgb, float* acc,
                              float* distance, int32_t* steps, void* stream) {
    const std::string who = "preview_360_march: ";
    if (!field || !params) return fail(PV_E_INVALID, who + "field and params must not be null");
    const char* why = "";
    if (const int code = mip::preview_field_check(field, &why)) return fail(code, who + why);
    mip::PreviewField f;
    mip::PreviewMarch p;
    bool go;
    if (const int code = call_check(who, field, far_radius, params, n_rays, origins, directions, near, far, rgb, acc, distance, &f, &p, &go))
        return code;
    if (!go) return PV_OK;
    return hip_result(mip::launch_preview_march_360(f, p, far_radius, field->degree, n_rays, origins, directions, near, far, rgb, acc, distance,
                                                    steps, S(stream)), "preview_360_march");
}

int mipnerf_preview_360_march_sparse(const mipnerf_preview_sparse_field_t* sparse, float far_radius, const mipnerf_preview_params_t* params,
                                     int64_t n_rays, const float* origins, const float* directions, const float* near, const float* far,
                                     float* rgb, float* acc, float* distance, int32_t* steps, void* stream) {
    const std::string who = "preview_360_march_sparse: ";
    if (!sparse || !params) return fail(PV_E_INVALID, who + "field and params must not be null");
    if (sparse->n_rows < 0) return fail(PV_E_INVALID, who + "n_rows must not be negative");
    mipnerf_preview_field_t field = sparse->field;
    if (!field.rows && sparse->n_rows == 0) field.rows = &field;      // no stored point, no rows: the shared check sees a non-null pointer
    const char* why = "";
    if (const int code = mip::preview_field_check(&field, &why)) return fail(code, who + why);
    if (sparse->n_rows > (int64_t)field.dims[0] * field.dims[1] * field.dims[2]) return fail(PV_E_INVALID, who + "n_rows exceeds the lattice's points");
    if (!field.occupancy || !sparse->table)
        return fail(PV_E_INVALID, who + "a sparse lattice needs its occupancy words and its table (neither may be null)");
    if (reinterpret_cast<uintptr_t>(sparse->table) % 8 != 0) return fail(PV_E_INVALID, who + "table must be 8-byte aligned");
    mip::PreviewSparseField f;
    mip::PreviewMarch p;
    bool go;
    if (const int code = call_check(who, &sparse->field, far_radius, params, n_rays, origins, directions, near, far, rgb, acc, distance, &f, &p, &go))
        return code;
    if (!go) return PV_OK;
    f.table = reinterpret_cast<const mip::SparseEntry*>(sparse->table);
    f.words_p = mip::sparse_words_p(field.dims[0]);
    return hip_result(mip::launch_preview_march_360_sparse(f, p, far_radius, field.degree, n_rays, origins, directions, near, far, rgb, acc,
                                                           distance, steps, S(stream)), "preview_360_march_sparse");
}

}  // extern "C"
