// Host side of a march, stated ONCE for preview_capi.hip and preview_mip_capi.hip: the checks both entry points make on a lattice
// (mipnerf_preview_field_t) and on the parameters of a call before any HIP call, and the by-value kernel arguments (PreviewField and
// PreviewMarch, preview_march.hpp) derived from them.  Each entry point prepends its own name to a message.  Compile with
// -ffp-contract=off: the spacing (hi - lo) / float(n - 1) and inv_h = float(n - 1) / (hi - lo) round once, as the header states them.
#pragma once

#include <math.h>
#include <stdint.h>

#include "../../include/mipnerf_preview.h"
#include "preview_march.hpp"

namespace mip {

enum { PV_OK = 0, PV_E_INVALID = 1, PV_E_UNSUPPORTED = 2, PV_E_HIP = 3 };      // the codes of mipnerf_hip.h

// dims of a lattice every entry point accepts: >= 2 points per axis and 7 nx ny nz < 2^31 (the rule of mipnerf_occupancy_words)
inline bool preview_dims_ok(const int32_t* dims) {
    if (dims[0] < 2 || dims[1] < 2 || dims[2] < 2) return false;
    return 7ll * dims[0] * (long long)dims[1] < (1ll << 31) && 7ll * dims[0] * (long long)dims[1] * dims[2] < (1ll << 31);
}

// everything about a field that does not depend on the rays: PV_OK, or the code with *why set (no entry-point prefix)
inline int preview_field_check(const mipnerf_preview_field_t* field, const char** why) {
    if (!field->rows) { *why = "field.rows must not be null"; return PV_E_INVALID; }
    if (field->degree < 0 || field->degree > 2) { *why = "field.degree must be 0, 1 or 2"; return PV_E_UNSUPPORTED; }
    if (!preview_dims_ok(field->dims)) { *why = "a lattice needs at least 2 points per axis and 7 nx ny nz < 2^31"; return PV_E_INVALID; }
    for (int a = 0; a < 3; ++a)
        if (!(field->hi[a] > field->lo[a]) || !isfinite(field->lo[a]) || !isfinite(field->hi[a])) {
            *why = "the box needs finite lo < hi on every axis";
            return PV_E_INVALID;
        }
    return PV_OK;
}

// the row alignment rule of mipnerf_preview_march
inline bool preview_rows_aligned(const mipnerf_preview_field_t* field) {
    const int W = preview_row_halves(field->degree);
    return reinterpret_cast<uintptr_t>(field->rows) % (W < 8 ? 8 : 16) == 0;
}

// the kernel argument of a checked field; returns min(h), the smallest axis spacing of rule 1
inline float preview_field_derive(const mipnerf_preview_field_t* field, PreviewField* f) {
    f->box.nx = field->dims[0]; f->box.ny = field->dims[1]; f->box.nz = field->dims[2];
    float hmin = INFINITY;
    for (int a = 0; a < 3; ++a) {
        const float span = field->hi[a] - field->lo[a];
        f->box.lo[a] = field->lo[a];
        f->hi[a] = field->hi[a];
        f->box.inv_h[a] = (float)(field->dims[a] - 1) / span;        // as mipnerf_lattice_density forms it
        hmin = fminf(hmin, span / (float)(field->dims[a] - 1));
    }
    f->rows = static_cast<const uint16_t*>(field->rows);
    f->occ = field->occupancy;
    f->words_x = (field->dims[0] - 1 + 31) / 32;
    return hmin;
}

// everything about a call that does not depend on the field: PV_OK, or the code with *why set (no entry-point prefix)
inline int preview_call_check(const mipnerf_preview_params_t* params, int64_t n_rays, const char** why) {
    *why = nullptr;
    if (!(params->step_scale > 0.0f) || !isfinite(params->step_scale)) *why = "step_scale must be positive and finite";
    else if (params->max_steps < 1) *why = "max_steps must be at least 1";
    else if (!(params->t_min >= 0.0f && params->t_min < 1.0f)) *why = "t_min must lie in [0, 1)";
    else if (n_rays < 0 || n_rays > 0x7fffffffll) *why = "n_rays must lie in [0, 2^31)";
    return *why ? PV_E_INVALID : PV_OK;
}

// the kernel argument of checked parameters, with the world step step_scale * s0; false: that step is not positive and finite
inline bool preview_march_derive(const mipnerf_preview_params_t* params, float s0, PreviewMarch* p) {
    p->s = params->step_scale * s0;
    p->t_min = params->t_min;
    p->max_steps = params->max_steps;
    for (int a = 0; a < 3; ++a) p->background[a] = params->background[a];
    return p->s > 0.0f && isfinite(p->s);
}

}  // namespace mip
