// C ABI of libmipnerf_preview_sparse.so (include/mipnerf_preview_sparse.h): argument checks before any HIP call, then the launchers of
// kernels_preview_sparse.hip.  Never allocates, never synchronises.  The checks of one level and of a call, and the kernel arguments
// derived from them, are preview_field_host.hpp's, the ones mipnerf_preview_march and mipnerf_preview_mip_march make.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <string.h>

#include <string>

#include "../../include/mipnerf_preview_sparse.h"
#include "preview_field_host.hpp"
#include "preview_sparse.hpp"

namespace mip {
int64_t sparse_index_blocks(const int32_t* dims);
hipError_t launch_sparse_index(const int32_t* dims, const uint32_t* occ, SparseEntry* table, int32_t* total, unsigned* block_sum,
                               hipStream_t stream);
hipError_t launch_sparse_gather(const int32_t* dims, int degree, const SparseEntry* table, const void* dense, void* rows,
                                hipStream_t stream);
hipError_t launch_sparse_pack(int64_t n, int degree, const float* sigma, const float* coef, uint16_t* rows, hipStream_t stream);
hipError_t launch_preview_sparse_march(const PreviewSparsePyramid& pyr, const PreviewMarch& p, float footprint, int degree, int64_t n_rays,
                                       const float* origins, const float* directions, const float* radii, const float* near,
                                       const float* far, float* rgb, float* acc, float* distance, int32_t* steps, float* lod,
                                       hipStream_t stream);
}  // namespace mip

namespace {

thread_local std::string g_err;
using mip::PV_OK;
using mip::PV_E_INVALID;
using mip::PV_E_UNSUPPORTED;
using mip::PV_E_HIP;
const char* const kLattice = "a lattice needs at least 2 points per axis and 7 nx ny nz < 2^31";

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

inline hipStream_t S(void* s) { return reinterpret_cast<hipStream_t>(s); }

int hip_result(hipError_t e, const char* who) {
    if (e == hipSuccess) return PV_OK;
    return fail(PV_E_HIP, std::string(who) + ": " + hipGetErrorString(e));
}

bool aligned(const void* p, int bytes) { return reinterpret_cast<uintptr_t>(p) % bytes == 0; }

int row_alignment(int degree) { return mip::preview_row_halves(degree) < 8 ? 8 : 16; }

}  // namespace

extern "C" {

int mipnerf_preview_sparse_abi_version(void) { return 1; }

const char* mipnerf_preview_sparse_last_error(void) { return g_err.c_str(); }

size_t mipnerf_preview_sparse_scratch_bytes(const int32_t* dims) {
    if (!dims || !mip::preview_dims_ok(dims)) {
        fail(PV_E_INVALID, std::string("preview_sparse_scratch_bytes: ") + (dims ? kLattice : "dims must not be null"));
        return 0;
    }
    return (size_t)mip::sparse_index_blocks(dims) * sizeof(unsigned);
}

int mipnerf_preview_sparse_index(const int32_t* dims, const uint32_t* occupancy, uint32_t* table, int32_t* total, void* scratch,
                                 void* stream) {
    const std::string who = "preview_sparse_index: ";
    if (!dims || !table || !total || !scratch) return fail(PV_E_INVALID, who + "dims, table, total and scratch must not be null");
    if (!occupancy) return fail(PV_E_INVALID, who + "occupancy must not be null (a lattice with every cell occupied stays dense)");
    if (!mip::preview_dims_ok(dims)) return fail(PV_E_INVALID, who + kLattice);
    if (!aligned(table, 8) || !aligned(total, 4) || !aligned(scratch, 4) || !aligned(occupancy, 4))
        return fail(PV_E_INVALID, who + "table must be 8-byte aligned, occupancy, total and scratch 4-byte aligned");
    return hip_result(mip::launch_sparse_index(dims, occupancy, reinterpret_cast<mip::SparseEntry*>(table), total,
                                               static_cast<unsigned*>(scratch), S(stream)), "preview_sparse_index");
}

int mipnerf_preview_sparse_gather(const int32_t* dims, int32_t degree, const uint32_t* table, const void* dense_rows, void* rows,
                                  void* stream) {
    const std::string who = "preview_sparse_gather: ";
    if (!dims || !table || !dense_rows || !rows) return fail(PV_E_INVALID, who + "dims, table, dense_rows and rows must not be null");
    if (degree < 0 || degree > 2) return fail(PV_E_UNSUPPORTED, who + "degree must be 0, 1 or 2");
    if (!mip::preview_dims_ok(dims)) return fail(PV_E_INVALID, who + kLattice);
    if (!aligned(table, 8)) return fail(PV_E_INVALID, who + "table must be 8-byte aligned");
    if (!aligned(dense_rows, row_alignment(degree)) || !aligned(rows, row_alignment(degree)))
        return fail(PV_E_INVALID, who + "dense_rows and rows must be 16-byte aligned (8 for degree 0)");
    return hip_result(mip::launch_sparse_gather(dims, degree, reinterpret_cast<const mip::SparseEntry*>(table), dense_rows, rows, S(stream)),
                      "preview_sparse_gather");
}

int mipnerf_preview_sparse_pack(int64_t n_rows, int32_t degree, const float* sigma, const float* coef, void* rows, void* stream) {
    const std::string who = "preview_sparse_pack: ";
    if (n_rows < 0 || n_rows > 0x7fffffffll) return fail(PV_E_INVALID, who + "n_rows must lie in [0, 2^31)");
    if (degree < 0 || degree > 2) return fail(PV_E_UNSUPPORTED, who + "degree must be 0, 1 or 2");
    if (n_rows == 0) return PV_OK;
    if (!sigma || !coef || !rows) return fail(PV_E_INVALID, who + "sigma, coef and rows must not be null");
    return hip_result(mip::launch_sparse_pack(n_rows, degree, sigma, coef, static_cast<uint16_t*>(rows), S(stream)), "preview_sparse_pack");
}

int mipnerf_preview_sparse_march(const mipnerf_preview_sparse_pyramid_t* pyramid, const mipnerf_preview_params_t* params, float footprint,
                                 int64_t n_rays, const float* origins, const float* directions, const float* radii, const float* near,
                                 const float* far, float* rgb, float* acc, float* distance, int32_t* steps, float* lod, void* stream) {
    using namespace mip;
    const std::string kWho = "preview_sparse_march: ";
    if (!pyramid || !params) return fail(PV_E_INVALID, kWho + "pyramid and params must not be null");
    const int L = pyramid->levels;
    if (L < 1 || L > kMipMaxLevels) return fail(PV_E_INVALID, kWho + "pyramid.levels must lie in 1 .. 8");
    PreviewSparsePyramid pyr;
    memset(&pyr, 0, sizeof(pyr));
    pyr.levels = L;
    const mipnerf_preview_field_t* first = &pyramid->level[0].field;
    for (int l = 0; l < L; ++l) {
        const mipnerf_preview_sparse_field_t* level = &pyramid->level[l];
        const std::string who = kWho + "level " + std::to_string(l) + ": ";
        if (level->n_rows < 0) return fail(PV_E_INVALID, who + "n_rows must not be negative");
        mipnerf_preview_field_t field = level->field;
        if (!field.rows && level->n_rows == 0) field.rows = &field;      // no stored point, no rows: the shared check sees a non-null pointer
        const char* why = "";
        if (const int code = preview_field_check(&field, &why)) return fail(code, who + why);
        if (level->n_rows > (int64_t)field.dims[0] * field.dims[1] * field.dims[2])
            return fail(PV_E_INVALID, who + "n_rows exceeds the lattice's points");
        if (!field.occupancy || !level->table)
            return fail(PV_E_INVALID, who + "a sparse level needs its occupancy words and its table (neither may be null)");
        if (memcmp(field.lo, first->lo, sizeof(field.lo)) != 0 || memcmp(field.hi, first->hi, sizeof(field.hi)) != 0)
            return fail(PV_E_INVALID, who + "every level spans the box of level 0, bit for bit");
        if (field.degree != first->degree) return fail(PV_E_INVALID, who + "every level has the degree of level 0");
        pyr.spacing[l] = preview_field_derive(&level->field, &pyr.level[l]);
        pyr.level[l].table = reinterpret_cast<const SparseEntry*>(level->table);
        pyr.level[l].words_p = sparse_words_p(field.dims[0]);
        if (l > 0 && !(pyr.spacing[l] > pyr.spacing[l - 1]))
            return fail(PV_E_INVALID, who + "the smallest spacing must increase strictly from level to level");
    }
    for (int l = L; l < kMipMaxLevels; ++l) pyr.spacing[l] = pyr.spacing[L - 1];      // never read
    if (!(footprint >= 0.0f) || !isfinite(footprint)) return fail(PV_E_INVALID, kWho + "footprint must be finite and >= 0");
    const char* why = "";
    if (const int code = preview_call_check(params, n_rays, &why)) return fail(code, kWho + why);
    if (n_rays == 0) return PV_OK;
    if (!origins || !directions || !near || !far || !rgb || !acc || !distance)
        return fail(PV_E_INVALID, kWho + "origins, directions, near, far, rgb, acc and distance must not be null");
    for (int l = 0; l < L; ++l) {
        if (!preview_rows_aligned(&pyramid->level[l].field))
            return fail(PV_E_INVALID, kWho + "level " + std::to_string(l) + ": field.rows must be 16-byte aligned (8 for degree 0)");
        if (!aligned(pyramid->level[l].table, 8)) return fail(PV_E_INVALID, kWho + "level " + std::to_string(l) + ": table must be 8-byte aligned");
    }
    PreviewMarch p;
    if (!preview_march_derive(params, pyr.spacing[0], &p)) return fail(PV_E_INVALID, kWho + "the world step step_scale * s_0 must be positive and finite");
    return hip_result(launch_preview_sparse_march(pyr, p, footprint, first->degree, n_rays, origins, directions, radii, near, far, rgb, acc,
                                                  distance, steps, lod, S(stream)), "preview_sparse_march");
}

}  // extern "C"
