// C ABI of libmipnerf_fuse.so (include/mipnerf_fuse.h): argument checks before any HIP call, then the launchers of kernels_fuse.hip; the
// host-only projection row (rule P) and the host build of the integration (rules T).  Never allocates, never synchronises.  Compiled with
// -ffp-contract=off: the spacing (hi - lo) / float(n - 1) rounds once, and the host build rounds like the kernel.
#include <hip/hip_runtime.h>
#include <math.h>

#include <string>

#include "../../include/mipnerf_hip.h"
#include "../../include/mipnerf_fuse.h"
#include "fuse_rules.hpp"

namespace mip {
hipError_t launch_depth_quantile(int64_t B, int N, const float* weights, const float* t, int nq, const float* q, float* depth,
                                 hipStream_t st);
hipError_t launch_fuse_integrate(const FuseLattice& g, float trunc, int carve, int64_t num_frames, const float* frames,
                                 const int64_t* offsets, const float* depth, int64_t depth_count, float* sum, float* count, hipStream_t st);
hipError_t launch_fuse_finalise(int64_t n, const float* sum, const float* count, float fill, float* lattice, hipStream_t st);
}  // namespace mip

namespace {

enum { FZ_OK = 0, FZ_E_INVALID = 1, FZ_E_UNSUPPORTED = 2, FZ_E_HIP = 3 };      // the codes of mipnerf_hip.h
static_assert(MIPNERF_FUSE_MAX_QUANTILES == mip::kFuseMaxQuantiles, "the header and fuse_rules.hpp disagree on the quantile count");
static_assert(MIPNERF_FUSE_FRAME_FLOATS == mip::kFuseFrameFloats, "the header and fuse_rules.hpp disagree on the frame record");
static_assert(MIPNERF_FUSE_FRAMES_PER_LAUNCH == mip::kFuseFramesPerLaunch, "the header and fuse_rules.hpp disagree on the frames per launch");

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

// the kernel argument of a checked lattice; FZ_OK, or the code with the message set
int lattice_derive(const std::string& who, const int32_t* dims, const float* lo, const float* hi, mip::FuseLattice* g) {
    if (!dims || !lo || !hi) return fail(FZ_E_INVALID, who + "null argument (dims, lo or hi)");
    if (dims[0] < 2 || dims[1] < 2 || dims[2] < 2) return fail(FZ_E_INVALID, who + "a lattice needs at least 2 points per axis");
    if (7ll * dims[0] * (long long)dims[1] >= (1ll << 31) || 7ll * dims[0] * (long long)dims[1] * dims[2] >= (1ll << 31))
        return fail(FZ_E_INVALID, who + "the lattice index limit is 7 nx ny nz < 2^31");
    g->nx = dims[0]; g->ny = dims[1]; g->nz = dims[2];
    for (int a = 0; a < 3; ++a) {
        if (!(hi[a] > lo[a]) || !isfinite(lo[a]) || !isfinite(hi[a])) return fail(FZ_E_INVALID, who + "the box needs finite hi > lo on every axis");
        g->lo[a] = lo[a];
        g->h[a] = (hi[a] - lo[a]) / (float)(dims[a] - 1);
        if (!isfinite(g->h[a])) return fail(FZ_E_INVALID, who + "the box is too wide: (hi - lo) / (n - 1) is not finite");
    }
    return FZ_OK;
}

int integrate_check(const std::string& who, const int32_t* dims, const float* lo, const float* hi, float trunc, int64_t num_frames,
                    const float* frames, const int64_t* offsets, const float* depth, int64_t depth_count, float* sum, float* count,
                    mip::FuseLattice* g) {
    if (const int rc = lattice_derive(who, dims, lo, hi, g)) return rc;
    if (!(trunc > 0.0f) || !isfinite(trunc)) return fail(FZ_E_INVALID, who + "trunc must be finite and > 0");
    if (num_frames < 0) return fail(FZ_E_INVALID, who + "bad frame count " + std::to_string((long long)num_frames));
    if (depth_count < 0) return fail(FZ_E_INVALID, who + "bad depth count " + std::to_string((long long)depth_count));
    if (!sum || !count) return fail(FZ_E_INVALID, who + "null argument (sum or count)");
    if (num_frames > 0 && (!frames || !offsets || !depth)) return fail(FZ_E_INVALID, who + "null argument (frames, offsets or depth)");
    return FZ_OK;
}

}  // namespace

extern "C" {

int mipnerf_fuse_abi_version(void) { return 1; }

const char* mipnerf_fuse_last_error(void) { return g_err.c_str(); }

int mipnerf_fuse_depth_quantile(int64_t B, int32_t N, const float* weights, const float* t_samples, int32_t num_quantiles, const float* q,
                                float* depth, void* stream) {
    const std::string who = "fuse_depth_quantile: ";
    if (N < 1 || N > MIPNERF_MAX_SAMPLES)
        return fail(FZ_E_INVALID, who + "num_samples must be in [1, " + std::to_string(MIPNERF_MAX_SAMPLES) + "] (got " + std::to_string(N) + ")");
    if (num_quantiles < 1 || num_quantiles > MIPNERF_FUSE_MAX_QUANTILES)
        return fail(FZ_E_INVALID, who + "num_quantiles must be in [1, 4] (got " + std::to_string(num_quantiles) + ")");
    if (!q) return fail(FZ_E_INVALID, who + "null argument (q)");
    for (int j = 0; j < num_quantiles; ++j)
        if (!(q[j] > 0.0f && q[j] < 1.0f)) return fail(FZ_E_INVALID, who + "a quantile must lie in (0, 1) (got " + std::to_string(q[j]) + ")");
    if (B < 0 || B >= (1ll << 31)) return fail(FZ_E_INVALID, who + "bad ray count " + std::to_string((long long)B));
    if (B == 0) return FZ_OK;
    if (!weights || !t_samples || !depth) return fail(FZ_E_INVALID, who + "null argument");
    const hipError_t e = mip::launch_depth_quantile(B, N, weights, t_samples, num_quantiles, q, depth, reinterpret_cast<hipStream_t>(stream));
    if (e == hipSuccess) return FZ_OK;
    return fail(FZ_E_HIP, who + hipGetErrorString(e));
}

int mipnerf_fuse_projection(const float* camera, float* frame) {
    const std::string who = "fuse_projection: ";
    if (!camera || !frame) return fail(FZ_E_INVALID, who + "null argument");
    if (camera[26] == 2.0f || camera[26] == 3.0f)
        return fail(FZ_E_UNSUPPORTED, who + "camera mode " + std::to_string((int)camera[26]) + " (a distorted camera: " +
                    (camera[26] == 2.0f ? "radial-tangential" : "fisheye") + ") has no projection row; fuse ideal pinhole frames of the "
                    "capture's K instead, as PathGen builds them");
    switch (mip::fuse_projection_row(camera, frame)) {
        case 0: return FZ_OK;
        case 1: return fail(FZ_E_INVALID, who + "unknown camera mode " + std::to_string(camera[26]));
        case 2: return fail(FZ_E_INVALID, who + "pix2cam needs the last row (0, 0, -1) and an inverse");
        default: return fail(FZ_E_INVALID, who + "focal, width and height must be positive finite numbers (width and height whole)");
    }
}

int mipnerf_fuse_integrate(const int32_t dims[3], const float lo[3], const float hi[3], float trunc, int32_t carve, int64_t num_frames,
                           const float* frames, const int64_t* offsets, const float* depth, int64_t depth_count, float* sum, float* count,
                           void* stream) {
    const std::string who = "fuse_integrate: ";
    mip::FuseLattice g;
    if (const int rc = integrate_check(who, dims, lo, hi, trunc, num_frames, frames, offsets, depth, depth_count, sum, count, &g)) return rc;
    if (num_frames == 0) return FZ_OK;
    const hipError_t e = mip::launch_fuse_integrate(g, trunc, carve != 0, num_frames, frames, offsets, depth, depth_count, sum, count,
                                                    reinterpret_cast<hipStream_t>(stream));
    if (e == hipSuccess) return FZ_OK;
    return fail(FZ_E_HIP, who + hipGetErrorString(e));
}

int mipnerf_fuse_finalise(const int32_t dims[3], const float* sum, const float* count, float fill, float* lattice, void* stream) {
    const std::string who = "fuse_finalise: ";
    const float unit_lo[3] = {0.0f, 0.0f, 0.0f}, unit_hi[3] = {1.0f, 1.0f, 1.0f};
    mip::FuseLattice g;
    if (const int rc = lattice_derive(who, dims, unit_lo, unit_hi, &g)) return rc;
    if (!(fill == 1.0f || fill == -1.0f)) return fail(FZ_E_INVALID, who + "fill must be +1 (unseen points inside) or -1 (outside)");
    if (!sum || !count || !lattice) return fail(FZ_E_INVALID, who + "null argument");
    const hipError_t e = mip::launch_fuse_finalise((int64_t)g.nx * g.ny * g.nz, sum, count, fill, lattice, reinterpret_cast<hipStream_t>(stream));
    if (e == hipSuccess) return FZ_OK;
    return fail(FZ_E_HIP, who + hipGetErrorString(e));
}

int mipnerf_fuse_integrate_host(const int32_t dims[3], const float lo[3], const float hi[3], float trunc, int32_t carve, int64_t num_frames,
                                const float* frames, const int64_t* offsets, const float* depth, int64_t depth_count, float* sum,
                                float* count) {
    const std::string who = "fuse_integrate_host: ";
    mip::FuseLattice g;
    if (const int rc = integrate_check(who, dims, lo, hi, trunc, num_frames, frames, offsets, depth, depth_count, sum, count, &g)) return rc;
    // launch by launch and point by point, as k_fuse_integrate takes them
    for (int64_t f0 = 0; f0 < num_frames; f0 += mip::kFuseFramesPerLaunch) {
        const int64_t f1 = f0 + mip::kFuseFramesPerLaunch < num_frames ? f0 + mip::kFuseFramesPerLaunch : num_frames;
        for (int k = 0; k < g.nz; ++k)
            for (int j = 0; j < g.ny; ++j)
                for (int i = 0; i < g.nx; ++i) {
                    const int64_t idx = ((int64_t)k * g.ny + j) * g.nx + i;
                    const float x = mip::fuse_point(g.lo[0], i, g.h[0]), y = mip::fuse_point(g.lo[1], j, g.h[1]),
                                z = mip::fuse_point(g.lo[2], k, g.h[2]);
                    float s = sum[idx], c = count[idx];
                    bool touched = false;
                    for (int64_t f = f0; f < f1; ++f) {
                        float d;
                        if (mip::fuse_frame_update(frames + f * mip::kFuseFrameFloats, offsets[f], depth, depth_count, trunc, carve != 0, x, y, z,
                                                   &d)) {
                            s += d;
                            c += 1.0f;
                            touched = true;
                        }
                    }
                    if (touched) {
                        sum[idx] = s;
                        count[idx] = c;
                    }
                }
    }
    return FZ_OK;
}

}  // extern "C"
