// C ABI of libmipnerf_proposal_360.so (include/mipnerf_proposal_360.h): argument checks before any HIP call, then the launcher of
// kernels_proposal_360.hip.  Never allocates, never synchronises.  Compiled with -ffp-contract=off: the spacings (hi - lo) / float(n - 1)
// and inv_h = float(n - 1) / (hi - lo) round once, as the header states them.
#include <hip/hip_runtime.h>
#include <math.h>

#include <string>

#include "../../include/mipnerf_hip.h"
#include "../../include/mipnerf_proposal_360.h"
#include "lattice_sample_360.hpp"

namespace mip {
hipError_t launch_lattice_density_360(const ProposalPyramid& p, float footprint, int64_t B, int N, const float* t, const float* origins,
                                      const float* dirs, const float* radii, float* rgb_sigma, hipStream_t st);
hipError_t launch_reciprocal_360(int64_t n, const float* x, float* y, hipStream_t st);
}  // namespace mip

namespace {

enum { PQ_OK = 0, PQ_E_INVALID = 1, PQ_E_UNSUPPORTED = 2, PQ_E_HIP = 3 };      // the codes of mipnerf_hip.h
constexpr int kMaxSamples = MIPNERF_MAX_SAMPLES;
static_assert(MIPNERF_PROPOSAL_MAX_LEVELS == mip::kProposalMaxLevels, "the header and lattice_sample_360.hpp disagree on the level count");

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

// the kernel argument of a checked pyramid; PQ_OK, or the code with the message set
int pyramid_derive(const std::string& who, const mipnerf_proposal_pyramid* pyramid, mip::ProposalPyramid* p) {
    if (!pyramid) return fail(PQ_E_INVALID, who + "null argument (pyramid)");
    const int L = pyramid->levels;
    if (L < 1 || L > MIPNERF_PROPOSAL_MAX_LEVELS) return fail(PQ_E_INVALID, who + "levels must be in [1, 4] (got " + std::to_string(L) + ")");
    for (int a = 0; a < 3; ++a)
        if (!(pyramid->hi[a] > pyramid->lo[a]) || !isfinite(pyramid->lo[a]) || !isfinite(pyramid->hi[a]))
            return fail(PQ_E_INVALID, who + "the box needs finite hi > lo on every axis");
    p->levels = L;
    for (int l = 0; l < L; ++l) {
        const std::string lv = who + "level " + std::to_string(l) + ": ";
        const int32_t* n = pyramid->dims[l];
        if (!pyramid->lattice[l]) return fail(PQ_E_INVALID, lv + "null argument (lattice)");
        if (n[0] < 2 || n[1] < 2 || n[2] < 2) return fail(PQ_E_INVALID, lv + "a lattice needs at least 2 points per axis");
        if (7ll * n[0] * (long long)n[1] >= (1ll << 31) || 7ll * n[0] * (long long)n[1] * n[2] >= (1ll << 31))
            return fail(PQ_E_INVALID, lv + "the lattice index limit is 7 nx ny nz < 2^31");
        mip::LatticeBox& box = p->box[l];
        box.nx = n[0]; box.ny = n[1]; box.nz = n[2];
        float spacing = 0.0f;
        for (int a = 0; a < 3; ++a) {
            const float span = pyramid->hi[a] - pyramid->lo[a];
            box.lo[a] = pyramid->lo[a];
            box.inv_h[a] = (float)(n[a] - 1) / span;                 // as mipnerf_lattice_density forms it
            if (!isfinite(box.inv_h[a])) return fail(PQ_E_INVALID, lv + "the box is too thin: (n - 1) / (hi - lo) is not finite");
            spacing = fmaxf(spacing, span / (float)(n[a] - 1));
        }
        if (!isfinite(spacing)) return fail(PQ_E_INVALID, lv + "the box is too wide: (hi - lo) / (n - 1) is not finite");
        p->spacing[l] = spacing;
        p->lattice[l] = pyramid->lattice[l];
        if (l > 0 && !(p->spacing[l] > p->spacing[l - 1]))
            return fail(PQ_E_INVALID, lv + "the spacing must increase strictly from level to level");
    }
    for (int l = L; l < MIPNERF_PROPOSAL_MAX_LEVELS; ++l) {             // never read
        p->spacing[l] = p->spacing[L - 1];
        p->box[l] = p->box[L - 1];
        p->lattice[l] = p->lattice[L - 1];
    }
    return PQ_OK;
}

}  // namespace

extern "C" {

int mipnerf_proposal_360_abi_version(void) { return 1; }

const char* mipnerf_proposal_360_last_error(void) { return g_err.c_str(); }

int mipnerf_lattice_density_360(const mipnerf_proposal_pyramid* pyramid, float footprint, int64_t B, int32_t N, const float* t,
                                const float* origins, const float* dirs, const float* radii, float* rgb_sigma, void* stream) {
    const std::string who = "lattice_density_360: ";
    mip::ProposalPyramid p;
    if (const int rc = pyramid_derive(who, pyramid, &p)) return rc;
    if (!(footprint >= 0.0f) || !isfinite(footprint)) return fail(PQ_E_INVALID, who + "footprint must be finite and >= 0");
    if (N < 1 || N > kMaxSamples)
        return fail(PQ_E_INVALID, who + "num_samples must be in [1, " + std::to_string(kMaxSamples) + "] (got " + std::to_string(N) + ")");
    if (B < 0 || B >= (1ll << 31)) return fail(PQ_E_INVALID, who + "bad ray count " + std::to_string((long long)B));
    if (B == 0) return PQ_OK;
    if (!t || !origins || !dirs || !radii || !rgb_sigma) return fail(PQ_E_INVALID, who + "null argument");
    if (reinterpret_cast<uintptr_t>(rgb_sigma) % 16 != 0) return fail(PQ_E_INVALID, who + "rgb_sigma must be 16-byte aligned");
    if ((B * (int64_t)N + 255) / 256 > 0x7fffffffll) return fail(PQ_E_INVALID, who + "num_rays * num_samples must stay below 2^39");
    const hipError_t e = mip::launch_lattice_density_360(p, footprint, B, N, t, origins, dirs, radii, rgb_sigma, reinterpret_cast<hipStream_t>(stream));
    if (e == hipSuccess) return PQ_OK;
    return fail(PQ_E_HIP, who + hipGetErrorString(e));
}

int mipnerf_reciprocal_360(int64_t n, const float* t_inv, float* t, void* stream) {
    const std::string who = "reciprocal_360: ";
    if (n < 0 || (n + 255) / 256 > 0x7fffffffll) return fail(PQ_E_INVALID, who + "bad count " + std::to_string((long long)n));
    if (n == 0) return PQ_OK;
    if (!t_inv || !t) return fail(PQ_E_INVALID, who + "null argument");
    const hipError_t e = mip::launch_reciprocal_360(n, t_inv, t, reinterpret_cast<hipStream_t>(stream));
    if (e == hipSuccess) return PQ_OK;
    return fail(PQ_E_HIP, who + hipGetErrorString(e));
}

}  // extern "C"
