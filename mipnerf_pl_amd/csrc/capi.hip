// C ABI of libmipnerf_hip.so (see include/mipnerf_hip.h): context, weight packing, per-stage
// entry points and the level loop of MipNerf.forward (models/mip_nerf.py:172-248).
#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <cmath>
#include <string>
#include <algorithm>
#include <vector>

#include "../../include/mipnerf_hip.h"
#include "camera_models.hpp"
#include "kernels.hpp"
#include "lane_buckets.hpp"
#include "lattice_sample.hpp"
#include "mlp_variants_gen.hpp"
#include "mlp_train_variants_gen.hpp"
#include "mlp_f32r_variants_gen.hpp"
#include "mlp_pre_variants_gen.hpp"
#include "mlp_plan_gen.hpp"

// binary tables of the training kernels (mlp_train_plan.TrainPlan.blob()), linked in through train_tables.c (.incbin)

static_assert(MIPNERF_MAX_SAMPLES == mip::kPdfMaxBins, "the public sample-count limit is 64 lanes x kMaxSamplesPerLane (lane_buckets.hpp)");

namespace {

thread_local std::string g_err;

int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

#define HIP_TRY(expr)                                                                                  \
    do {                                                                                               \
        hipError_t e_ = (expr);                                                                        \
        if (e_ != hipSuccess) return fail(MIPNERF_E_HIP, "%s: %s", #expr, hipGetErrorString(e_));      \
    } while (0)

inline hipStream_t S(void* s) { return reinterpret_cast<hipStream_t>(s); }
inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

using mip::plan::PlanDesc;

// ---- plan tables: binary blob produced by mlp_plan.blob() (the only definition of the weight-stream layout), linked in by
// train_tables.c.  Every 512-entry chunk of a pack table travels as one record (tensor, row0, ld, nrows, col[16]) ----------
constexpr int kDescInts = 20, kLayerInts = 12;
struct PlanTables {
    const int32_t* pack = nullptr;       // [num_chunks] records of the plain plan's bf16 stream (debug table 0)
    const int32_t* bias = nullptr;       // [num_tiles * 32] flat parameter index or -1 (the fp32 kernel's bias table)
    const int32_t* fwd_pack = nullptr;   // [fwd_num_chunks] records of the bf16 forward kernels' stream
    const int32_t* fwd_bias = nullptr;   // [fwd_num_tiles * 32]
    const int32_t* pack_f32 = nullptr;   // [n_f32_chunks] records of the fp32 stream
    const int32_t* layers = nullptr;     // [num_ops] rows x_in0, kb0, x_in1, kb1, x_out, ntiles, first_tile, relu, kind, chunk0, stage_view, enc_mask
    int n_f32_chunks = 0;
};

int total_params(const PlanDesc& P) {
    int n = 0;
    for (int i = 0; i < P.num_param_tensors; ++i) n += P.param_numel[i];
    return n;
}

bool plan_tables(PlanTables& T, const PlanDesc& P) {
    const int32_t* h = reinterpret_cast<const int32_t*>(mip::kPlanTableBlobs[P.variant]);
    if (h[0] != 0x504C4E31 || h[1] != P.num_chunks || h[2] != P.num_tiles || h[3] != P.fwd_num_chunks || h[4] != P.fwd_num_tiles ||
        h[5] < 0 || h[5] > P.num_chunks || h[6] != P.num_ops || h[6] > mip::kF32MaxLayers || h[7] != total_params(P) || h[8] != P.fold)
        return false;
    if (!P.fold && (h[3] != h[1] || h[4] != h[2])) return false;
    T.pack = h + 16;
    T.bias = T.pack + (size_t)h[1] * kDescInts;
    const int32_t* p = T.bias + (size_t)h[2] * 32;
    T.fwd_pack = P.fold ? p : T.pack;
    T.fwd_bias = P.fold ? p + (size_t)h[3] * kDescInts : T.bias;
    if (P.fold) p = T.fwd_bias + (size_t)h[4] * 32;
    T.pack_f32 = p;
    T.n_f32_chunks = h[5];
    T.layers = T.pack_f32 + (size_t)h[5] * kDescInts;
    return T.layers + (size_t)h[6] * kLayerInts == h + h[9];
}

// flat offset of each parameter tensor, then of the derived tensors of the folded plan (mlp_plan.Plan.derived_shapes: tensors
// num_param_tensors and num_param_tensors + 1, computed by the pack kernel: FoldDesc)
std::vector<int> tensor_offsets(const PlanDesc& P) {
    std::vector<int> off(P.num_param_tensors);
    int o = 0;
    for (int i = 0; i < P.num_param_tensors; ++i) { off[i] = o; o += P.param_numel[i]; }
    if (P.fold) {
        off.push_back(o);
        off.push_back(o + P.net_width_cond * (P.net_width + P.view_dim));
    }
    return off;
}

// chunk records -> index table of `table_chunks` chunks (the rest stays -1): entry (hi * 32 + m, j) of a chunk is element
// (row0 + m) * ld + col[hi * 8 + j] of `tensor`, written as a flat parameter index (toff) or as (tensor << 20) | element for k_pack
std::vector<int32_t> expand(const int32_t* desc, int n, int table_chunks, const std::vector<int>* toff) {
    std::vector<int32_t> out((size_t)table_chunks * 512, -1);
    for (int ci = 0; ci < n; ++ci) {
        const int32_t* d = desc + (size_t)ci * kDescInts;
        const int32_t base = toff ? (*toff)[d[0]] : d[0] << 20;
        for (int hi = 0; hi < 2; ++hi)
            for (int m = 0; m < d[3]; ++m)
                for (int j = 0; j < 8; ++j)
                    if (d[4 + hi * 8 + j] >= 0) out[(size_t)ci * 512 + (hi * 32 + m) * 8 + j] = base + (d[1] + m) * d[2] + d[4 + hi * 8 + j];
    }
    return out;
}

// LDS layout of kernels_mlp_f32.hip: [buffer B | buffer A | encoding]; the layer rows come from mlp_plan.Plan.f32_layers.
// Wide encodings (the 672 off-axis features of the unbounded-scene model): a 64-sample tile with the encoding resident does not
// fit the CU's LDS.  Instead of halving the tile (half the reuse of every weight chunk), the two layers that read the encoding
// stream that B operand from global memory (it stays in L1 / L2: 64 rows x 64 B per k block), and the encoding columns shrink to
// the view features + the VALU heads' partials.
mip::F32Net f32net(const PlanDesc& P, const int32_t* layers) {
    mip::F32Net net;
    memset(&net, 0, sizeof net);
    const int W = P.net_width, ecols_full = P.xyz_dim > 32 ? P.xyz_dim : 32;
    const bool stream_enc = mip::mlp_f32_tile_samples(2 * W + ecols_full + 4) < 64 && mip::mlp_f32_tile_samples(2 * W + 64 + 4) == 64;
    const int ecols = stream_enc ? 64 : ecols_full;
    net.nlayers = P.num_ops;
    net.width = W;
    net.xyz_dim = P.xyz_dim;
    net.pad = stream_enc ? 1 : 0;
    net.enc_col = 2 * W;
    net.dens_col = 2 * W + ecols;
    net.num_rgb = P.num_rgb;
    net.ldx = 2 * W + ecols + 4;
    for (int i = 0; i < P.num_ops; ++i) {
        const int32_t* r = layers + i * kLayerInts;
        // pad: bit 0 / 1 = K segment 0 / 1 is the sample encoding and is streamed from global memory
        net.layers[i] = mip::F32Layer{r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7], r[8], r[9], r[10], stream_enc ? r[11] : 0};
    }
    return net;
}

bool max_deg_span_is_16(const mipnerf_config& cfg) { return cfg.max_deg_point - cfg.min_deg_point == 16 && cfg.min_deg_point >= 0 && cfg.max_deg_point <= 31; }

// flat index -> (tensor << 20 | offset) as consumed by k_pack
std::vector<int32_t> encode(const int32_t* flat, size_t n, const std::vector<int>& toff) {
    std::vector<int32_t> out(n);
    for (size_t i = 0; i < n; ++i) {
        const int32_t f = flat[i];
        if (f < 0) { out[i] = -1; continue; }
        int t = (int)toff.size() - 1;
        while (toff[t] > f) --t;
        out[i] = (t << 20) | (f - toff[t]);
    }
    return out;
}

// ---- training tables: binary blob produced by mlp_train_plan.TrainPlan.blob(), linked in by train_tables.c ------
struct TrainTables {
    int n_bchunks, njobs, NH, NG, NMASK, NE, job_floats, nparams, n_scratch;     // NE: encoding blocks per wave tile (pre-GEMM plans), else 0
    int off_extra_w, off_extra_b, off_view_w, off_view_b;
    const int32_t* bpack;    // [n_bchunks * 512] flat parameter index or -1
    const int32_t* jobs;     // [njobs * 20]
    const int32_t* otab;     // [njobs * job_floats] flat parameter index or -1
};

bool train_tables(TrainTables& T, int variant = 0) {
    if (variant < 0 || variant >= mip::plan::kNumVariants || !mip::kTrainTableBlobs[variant]) return false;
    const int32_t* h = reinterpret_cast<const int32_t*>(mip::kTrainTableBlobs[variant]);
    if (h[0] != 0x54524E31) return false;
    T.n_bchunks = h[1]; T.njobs = h[2]; T.NH = h[3]; T.NG = h[4]; T.NMASK = h[5] & 0xffff; T.NE = h[5] >> 16; T.job_floats = h[6]; T.nparams = h[7];
    T.n_scratch = h[11]; T.off_extra_w = h[12]; T.off_extra_b = h[13]; T.off_view_w = h[14]; T.off_view_b = h[15];
    T.bpack = h + 16;
    T.jobs = T.bpack + h[8];
    T.otab = T.jobs + h[9];
    return h[9] == T.njobs * 20 && h[10] == T.njobs * T.job_floats && T.job_floats == mip::kWgradJobFloats;
}

// ---- register-resident fp32 kernel: blob produced by mlp_f32r_plan.F32RPlan.blob(), linked in by train_tables.c ------
struct F32RTables {
    int n_chunks = 0, n_aux = 0, n_groups = 0;
    const int32_t* pack = nullptr;   // [n_chunks * 256] flat parameter index or -1
    const int32_t* aux = nullptr;    // [n_aux]
};
bool f32r_tables(F32RTables& T, int variant, int nparams) {
    if (variant < 0 || variant >= mip::plan::kNumVariants || !mip::kF32RTableBlobs[variant]) return false;
    const int32_t* h = reinterpret_cast<const int32_t*>(mip::kF32RTableBlobs[variant]);
    if (h[0] != 0x46335231 || h[4] != h[1] * 256 || h[5] != nparams) return false;
    T.n_chunks = h[1]; T.n_aux = h[3]; T.n_groups = h[6];
    T.pack = h + 16;
    T.aux = T.pack + h[4];
    return true;
}

// ---- two-kernel bf16 form of wide encodings: blob produced by mlp_pre_plan.PrePlan.blob(), linked in by train_tables.c ------
struct PreTables {
    int n_gemm_chunks = 0, n_gemm_bias = 0, n_trunk_chunks = 0, n_trunk_tiles = 0, nk = 0;
    const int32_t* gemm_pack = nullptr;    // [n_gemm_chunks * 512] flat parameter index or -1
    const int32_t* gemm_bias = nullptr;    // [n_gemm_bias]
    const int32_t* trunk_pack = nullptr;   // [n_trunk_chunks * 512]
    const int32_t* trunk_bias = nullptr;   // [n_trunk_tiles * 32]
    // round 6: the one-kernel form of the same model (mlp_plan.Plan.build(arch, fused=True)), tables behind the two-kernel form's
    int n_fused_chunks = 0, n_fused_tiles = 0;
    const int32_t* fused_pack = nullptr;   // [n_fused_chunks * 512]
    const int32_t* fused_bias = nullptr;   // [n_fused_tiles * 32]
};
bool pre_tables(PreTables& T, int variant, int nparams) {
    if (variant < 0 || variant >= mip::plan::kNumVariants || !mip::kPreTableBlobs[variant]) return false;
    const int32_t* h = reinterpret_cast<const int32_t*>(mip::kPreTableBlobs[variant]);
    if (h[0] != 0x50524731 || h[7] != nparams || h[1] != h[2]) return false;
    T.n_gemm_chunks = h[1]; T.n_gemm_bias = h[3]; T.n_trunk_chunks = h[4]; T.n_trunk_tiles = h[6]; T.nk = h[8];
    T.gemm_pack = h + 16;
    T.gemm_bias = T.gemm_pack + (size_t)h[1] * 512;
    T.trunk_pack = T.gemm_bias + h[3];
    T.trunk_bias = T.trunk_pack + (size_t)h[4] * 512;
    T.n_fused_chunks = h[10]; T.n_fused_tiles = h[11];
    T.fused_pack = T.trunk_bias + (size_t)h[6] * 32;
    T.fused_bias = T.fused_pack + (size_t)h[10] * 512;
    return true;
}

}  // namespace

struct mipnerf_ctx {
    mipnerf_config cfg;
    const PlanDesc* P = nullptr;     // the generated architecture variant this context runs (mlp_plan_gen.hpp kPlans)
    std::vector<int> tensor_off;     // flat offset of each parameter tensor (tensor_offsets)
    mip::F32Net net;                 // the LDS-resident fp32 kernel's layers (f32net)
    // every packed stream of the context: mipnerf_set_params gathers `n` parameters through the device index table `idx` into `out`
    // (add_stream fills the list, mipnerf_destroy frees both buffers; the launchers read `out` through the typed pointers below)
    struct PackedStream { int32_t* idx; void* out; int64_t n; bool bf16; };
    std::vector<PackedStream> streams;
    void* d_stream_bf16 = nullptr;   // fwd_num_chunks * 1 KiB (inference + training forward)
    float* d_stream_f32 = nullptr;   // num_chunks * 2 KiB
    float* d_bias = nullptr;         // num_tiles * 32 floats (fp32 kernel)
    float* d_fwd_bias = nullptr;     // fwd_num_tiles * 32 floats (bf16 forward kernels)
    // register-resident fp32 kernel (variants up to 256 wide): its own weight stream (1-KiB chunks) and aux table
    F32RTables f32r;
    float* d_stream_f32r = nullptr;
    float* d_aux_f32r = nullptr;
    int f32_resident = 1;            // option 5: 1 = k_mlp_f32r where generated (inference), 0 = the LDS-resident k_mlp_f32
    // two-kernel bf16 inference of the variants whose encoding does not fit k_mlp_bf16's wave-private LDS area (gen_pre_gemm.py):
    // k_pre_gemm's weight stream + accumulator images, the trunk kernel's stream + bias table, and scratch for the per-stage entry point
    PreTables pre;
    void* d_fused_stream = nullptr;  // one-kernel form (round 6): its weight stream and bias table
    float* d_fused_bias = nullptr;
    int fused_pre = 1;               // option 6: 1 = mipnerf_forward runs the one-kernel form where generated, 0 = k_pre_gemm + trunk (same bits)
    void* d_pre_gemm_stream = nullptr;
    float* d_pre_gemm_bias = nullptr;
    void* d_pre_trunk_stream = nullptr;
    float* d_pre_trunk_bias = nullptr;
    void* d_pre_scratch = nullptr;   // pre_x | pre_acc of mipnerf_mlp_forward (mipnerf_forward carves them out of the caller's workspace)
    size_t pre_scratch_bytes = 0;
    hipEvent_t pre_scratch_event = nullptr;     // recorded behind the last user's kernels: another stream waits for it before it overwrites the buffer
    void* pre_scratch_stream = nullptr;
    bool pre_scratch_used = false;
    // training (bf16): W^T stream of the dgrad kernel, wgrad job tables
    TrainTables tt;
    void* d_stream_dgrad = nullptr;
    mip::WgradJob* d_jobs = nullptr;
    int32_t* d_otab = nullptr;
    int4* d_wgtab = nullptr;
    int2* d_jobslots = nullptr;
    float* d_scratch = nullptr;      // fp32 scratch behind the parameters (M, db_view of one backward call)
    float* d_extra_wT = nullptr;     // W_extra^T (fp32), refreshed by mipnerf_set_params
    int num_wgrad_wgs = 0;
    mip::ParamPtrs pp;               // device pointers of the fp32 master parameters (last mipnerf_set_params)
    bool params_set = false;
    int mlp_dma = 1;                 // 1: global_load_lds ring, 0: register-staged ring (debug)
    int fused_ipe = 1;               // bf16 mipnerf_forward: IPE computed inside the MLP kernel (0: k_cast_ipe + enc buffer)
    int fuse_small = 1;              // mipnerf_forward: k_ray_prologue / k_composite_resample instead of one launch per stage (option 4)
    int grid_limit = 256;            // persistent workgroups of the bf16 MLP kernel (= CUs)
    // optional instrumentation: HIP events around every MLP launch made by mipnerf_forward
    int time_mlp = 0;
    std::vector<hipEvent_t> ev;      // pairs (start, stop)
    size_t ev_used = 0;
};

namespace {
// the bf16 inference kernel generated for this context's architecture variant
hipError_t launch_bf16_variant(mipnerf_ctx* c, const void* enc, const void* viewenc, float* rgb_sigma, float* raw, int64_t M, int N,
                               bool dma, const mip::RayInputs* rays, const float* dnoise, hipStream_t st) {
    // dnoise: density-noise draws of the level being evaluated, an ARGUMENT (not context state): two host threads / streams
    // driving the same context cannot see each other's pointer
    const mip::LaunchBf16Fn fn = mip::kLaunchBf16[c->P->variant];
    if (!fn) return hipErrorInvalidValue;          // fp32-only architecture variant (callers check has_bf16 first)
    return fn(c->d_stream_bf16, c->d_fwd_bias, enc, viewenc, rgb_sigma, raw, M, N, c->cfg.density_bias, c->cfg.rgb_padding,
              c->grid_limit, dma, rays, dnoise, c->cfg.density_noise, st);
}

// ... and its training kernels (variants whose row of the generated kLaunchTrainFwd table is not null)
static inline bool has_bf16_train(const PlanDesc* P) { return mip::kLaunchTrainFwd[P->variant] != nullptr; }
// round 5: the training form of the two-kernel bf16 MLP (wide encodings: the unbounded-scene model) -- k_pre_gemm + a trunk forward-with-save,
// the standard dgrad, weight-gradient jobs that read the row-major encoding (mlp_train_plan.TrainPlan.build(arch, pre_gemm=True))
static inline bool has_bf16_train_pre(const PlanDesc* P) { return mip::kLaunchTrainFwdPre[P->variant] != nullptr; }
static inline bool has_bf16_train_any(const PlanDesc* P) { return has_bf16_train(P) || has_bf16_train_pre(P); }
static inline bool has_bf16_pre(const PlanDesc* P) { return mip::kLaunchPreGemm[P->variant] != nullptr; }      // the two-kernel form
static inline bool has_bf16(const PlanDesc* P) { return mip::kLaunchBf16[P->variant] != nullptr || has_bf16_pre(P); }
// bytes of k_pre_gemm's two outputs for M samples: 16 KiB (X fragments) + 32 KiB (accumulator images) per wave tile, whole 256-sample tiles
static inline size_t pre_x_bytes(int64_t M) { return (size_t)((M + 255) / 256) * 8 * 16384; }
static inline size_t pre_acc_bytes(int64_t M) { return (size_t)((M + 255) / 256) * 8 * 32768; }
// bf16 B-operand fragments of the encoding: whole 256-sample tiles
static size_t pre_frag_bytes(const mipnerf_ctx* c, size_t M) { return ((M + 255) / 256) * 256 * (size_t)c->P->xyz_dim * 2; }
// k_pre_gemm + the trunk kernel.  enc: bf16, row-major [M, xyz_dim] (frag = 0) or the fragment layout launch_cast_ipe_360 writes
hipError_t launch_bf16_pre(mipnerf_ctx* c, const void* enc, int frag, const void* viewenc, float* rgb_sigma, float* raw, int64_t M, int N,
                           void* pre_x, void* pre_acc, const float* dnoise, hipStream_t st) {
    // round 6: fragment encodings go through ONE kernel where it was generated (layer 0 and the skip layer as k-step-major ops of the trunk
    // kernel, the encoding streamed through a wave-private LDS ring): no pre_x / pre_acc hand-off through HBM, same bits (option 6 = 0: two kernels)
    if (frag && c->fused_pre && c->d_fused_stream && mip::kLaunchBf16Fused[c->P->variant])
        return mip::kLaunchBf16Fused[c->P->variant](c->d_fused_stream, c->d_fused_bias, enc, nullptr, viewenc, rgb_sigma, raw, M, N,
                                                    c->cfg.density_bias, c->cfg.rgb_padding, c->grid_limit, dnoise, c->cfg.density_noise, st);
    hipError_t er = mip::kLaunchPreGemm[c->P->variant](c->d_pre_gemm_stream, c->d_pre_gemm_bias, enc, frag, pre_x, pre_acc, M, c->grid_limit, st);
    if (er != hipSuccess) return er;
    return mip::kLaunchBf16Pre[c->P->variant](c->d_pre_trunk_stream, c->d_pre_trunk_bias, pre_x, pre_acc, viewenc, rgb_sigma, raw, M, N,
                                              c->cfg.density_bias, c->cfg.rgb_padding, c->grid_limit, dnoise, c->cfg.density_noise, st);
}
hipError_t launch_trainfwd_variant(mipnerf_ctx* c, const void* enc, const void* viewenc, float* rgb_sigma, float* raw, void* act,
                                   void* masks, int64_t M, int N, const mip::RayInputs* rays, const float* dnoise, hipStream_t st) {
    const mip::LaunchTrainFwdFn fn = mip::kLaunchTrainFwd[c->P->variant];
    if (!fn) return hipErrorInvalidValue;
    return fn(c->d_stream_bf16, c->d_fwd_bias, enc, viewenc, rgb_sigma, raw, act, masks, M, N, c->cfg.density_bias, c->cfg.rgb_padding,
              c->grid_limit, rays, dnoise, c->cfg.density_noise, st);
}
hipError_t launch_dgrad_variant(mipnerf_ctx* c, const float* d_raw, const void* masks, void* delta, int64_t M, hipStream_t st) {
    const mip::LaunchDgradFn fn = mip::kLaunchDgrad[c->P->variant];
    if (!fn) return hipErrorInvalidValue;
    return fn(c->d_stream_dgrad, d_raw, masks, delta, M, c->grid_limit, st);
}

// split-K factor of the sample-contracted fp32 GEMMs: 1 x 2(3) output tiles (256 x 128) x 256 splits = 512+ eight-wave workgroups (with
// 64 splits every CU ran ONE 4-wave workgroup and nothing covered its barriers: 1.24 ms per 256 x 256 x 524288 wgrad)
constexpr int kF32WgradSplits = 256;

// the fp32 kernel evaluates the two thin heads (density, colour) on the VALU straight from the fp32 master parameters
mip::F32Net f32net_with_heads(const mipnerf_ctx* c) {
    mip::F32Net net = c->net;
    const int D = c->P->net_depth, Dc = c->P->net_depth_cond;
    net.dens_w = c->pp.p[2 * D];
    net.dens_b = c->pp.p[2 * D + 1];
    net.col_w = c->pp.p[2 * D + 4 + 2 * Dc];
    net.col_b = c->pp.p[2 * D + 5 + 2 * Dc];
    return net;
}

// one packed stream of the context: upload its index table, allocate its output (2 bytes per entry in bf16, else 4) and list it
template <typename T>
hipError_t add_stream(mipnerf_ctx* c, const std::vector<int32_t>& idx, bool bf16, T** out) {
    mipnerf_ctx::PackedStream s{nullptr, nullptr, (int64_t)idx.size(), bf16};
    hipError_t er = hipMalloc(&s.idx, idx.size() * 4);
    if (er == hipSuccess) er = hipMalloc(&s.out, idx.size() * (bf16 ? 2 : 4));
    if (er == hipSuccess) er = hipMemcpy(s.idx, idx.data(), idx.size() * 4, hipMemcpyHostToDevice);
    c->streams.push_back(s);          // also after a failure: mipnerf_destroy frees what was allocated
    *out = static_cast<T*>(s.out);
    return er;
}

#define NEED_BF16_TRAIN(what)                                                                                               \
    if (!has_bf16_train_any(c->P))                                                                                           \
        return fail(MIPNERF_E_UNSUPPORTED, what ": no bf16 training kernels were generated for this architecture variant " \
                                                "(gen_mlp_train.train_variants); train this shape in fp32 precision")

struct TrainWs {                   // carve-up of the caller's workspace (all 256-byte aligned)
    char* base;
    size_t off = 0;
    template <typename T> T* take(size_t bytes) {
        T* p = reinterpret_cast<T*>(base + off);
        off += align256(bytes);
        return p;
    }
};
}  // namespace

extern "C" {

int mipnerf_set_wgrad_splits(mipnerf_ctx* c, const int32_t* splits_host);

const char* mipnerf_last_error(void) { return g_err.c_str(); }
int mipnerf_abi_version(void) { return MIPNERF_ABI_VERSION; }

static void variant_to_cfg(const PlanDesc& P, mipnerf_config* cfg) {
    memset(cfg, 0, sizeof *cfg);
    cfg->num_samples = 128; cfg->num_levels = 2; cfg->min_deg_point = 0; cfg->max_deg_point = P.xyz_dim / P.feat_per_deg;
    cfg->unbounded = P.feat_per_deg == 42;
    cfg->deg_view = (P.view_dim - 3) / 6; cfg->use_viewdirs = P.use_viewdirs; cfg->net_depth = P.net_depth; cfg->net_width = P.net_width;
    cfg->net_depth_condition = P.net_depth_cond; cfg->net_width_condition = P.net_width_cond; cfg->skip_index = P.skip_index;
    cfg->num_rgb_channels = P.num_rgb; cfg->num_density_channels = P.num_density;
    cfg->resample_padding = 0.01f; cfg->density_bias = -1.0f; cfg->rgb_padding = 0.001f; cfg->density_noise = 0.0f;
}

int mipnerf_compiled_arch(mipnerf_config* cfg) {
    if (!cfg) return fail(MIPNERF_E_INVALID, "cfg is null");
    variant_to_cfg(mip::plan::kPlans[0], cfg);
    return MIPNERF_OK;
}

int mipnerf_num_variants(void) { return mip::plan::kNumVariants; }

int mipnerf_variant_arch(int variant, mipnerf_config* cfg, int* has_bf16_training) {
    if (!cfg || variant < 0 || variant >= mip::plan::kNumVariants) return fail(MIPNERF_E_INVALID, "variant_arch: bad argument");
    variant_to_cfg(mip::plan::kPlans[variant], cfg);
    if (has_bf16_training) *has_bf16_training = has_bf16_train_any(&mip::plan::kPlans[variant]);
    return MIPNERF_OK;
}

int mipnerf_create(const mipnerf_config* cfg, mipnerf_ctx** out) {
    using namespace mip::plan;
    if (!cfg || !out) return fail(MIPNERF_E_INVALID, "null argument");
    if (cfg->num_samples < 1 || cfg->num_samples > MIPNERF_MAX_SAMPLES)
        return fail(MIPNERF_E_INVALID, "num_samples must be in [1, %d]", MIPNERF_MAX_SAMPLES);
    if (cfg->num_levels < 1 || cfg->num_levels > 2) return fail(MIPNERF_E_UNSUPPORTED, "num_levels must be 1 or 2");
    if (!cfg->use_viewdirs && cfg->net_width_condition != cfg->net_width)
        return fail(MIPNERF_E_UNSUPPORTED, "use_viewdirs=False feeds the trunk output (net_width=%d) to color_layer, which has "
                                           "net_width_condition=%d inputs: the reference MLP fails on this shape too "
                                           "(models/mip_nerf.py:99-110)", cfg->net_width, cfg->net_width_condition);
    const PlanDesc* P = nullptr;
    for (int v = 0; v < kNumVariants && !P; ++v) {
        const PlanDesc& q = kPlans[v];
        if (cfg->net_depth == q.net_depth && cfg->net_width == q.net_width && cfg->net_depth_condition == q.net_depth_cond &&
            cfg->net_width_condition == q.net_width_cond && cfg->skip_index == q.skip_index && cfg->num_rgb_channels == q.num_rgb &&
            cfg->num_density_channels == q.num_density && (cfg->unbounded ? 42 : 6) == q.feat_per_deg &&
            q.feat_per_deg * (cfg->max_deg_point - cfg->min_deg_point) == q.xyz_dim &&
            3 + 6 * cfg->deg_view == q.view_dim && (cfg->use_viewdirs != 0) == (q.use_viewdirs != 0))
            P = &q;
    }
    if (!P) {
        std::string have;
        for (int v = 0; v < kNumVariants; ++v) {
            char b[160];
            snprintf(b, sizeof b, "%s[depth %d width %d cond %dx%d skip %d xyz %d (%d per degree) view %d viewdirs %d%s]", v ? ", " : "", kPlans[v].net_depth,
                     kPlans[v].net_width, kPlans[v].net_depth_cond, kPlans[v].net_width_cond, kPlans[v].skip_index, kPlans[v].xyz_dim,
                     kPlans[v].feat_per_deg, kPlans[v].view_dim, kPlans[v].use_viewdirs, has_bf16(&kPlans[v]) ? "" : ", fp32 only");
            have += b;
        }
        return fail(MIPNERF_E_UNSUPPORTED, "no kernels / tables were generated for this MLP shape; generated: %s.  Add the shape to "
                                           "VARIANTS in csrc/gen_mlp_bf16.py and rebuild", have.c_str());
    }
    if (P->num_param_tensors + (P->fold ? 2 : 0) > mip::kMaxParamTensors)
        return fail(MIPNERF_E_UNSUPPORTED, "variant has %d parameter tensors, the library handles up to %d", P->num_param_tensors, mip::kMaxParamTensors);
    mipnerf_ctx* c = new mipnerf_ctx();
    c->cfg = *cfg;
    c->P = P;
    c->tensor_off = tensor_offsets(*P);
    PlanTables pl;
    if (!plan_tables(pl, *P)) {
        mipnerf_destroy(c);
        return fail(MIPNERF_E_INVALID, "mipnerf_create: embedded plan tables are inconsistent with the compiled plan");
    }
    c->net = f32net(*P, pl.layers);
    hipError_t er = hipSuccess;
    auto chk = [&](hipError_t e) { if (er == hipSuccess) er = e; };
    auto add = [&](const std::vector<int32_t>& idx, bool bf16, auto** out) { if (er == hipSuccess) er = add_stream(c, idx, bf16, out); };
    auto flat = [&](const int32_t* idx, size_t n) { return encode(idx, n, c->tensor_off); };
    add(expand(pl.fwd_pack, P->fwd_num_chunks, P->fwd_num_chunks, nullptr), true, &c->d_stream_bf16);
    add(expand(pl.pack_f32, pl.n_f32_chunks, P->num_chunks, nullptr), false, &c->d_stream_f32);      // sized like the plain bf16 stream
    add(flat(pl.bias, (size_t)P->num_tiles * 32), false, &c->d_bias);
    add(flat(pl.fwd_bias, (size_t)P->fwd_num_tiles * 32), false, &c->d_fwd_bias);
    if (er != hipSuccess) {
        mipnerf_destroy(c);
        return fail(MIPNERF_E_HIP, "mipnerf_create: %s", hipGetErrorString(er));
    }
    if (mip::kLaunchF32R[P->variant]) {
        if (!f32r_tables(c->f32r, P->variant, total_params(*P))) {
            mipnerf_destroy(c);
            return fail(MIPNERF_E_INVALID, "mipnerf_create: embedded tables of the register-resident fp32 kernel are inconsistent with the compiled plan");
        }
        add(flat(c->f32r.pack, (size_t)c->f32r.n_chunks * 256), false, &c->d_stream_f32r);
        add(flat(c->f32r.aux, (size_t)c->f32r.n_aux), false, &c->d_aux_f32r);
        if (er != hipSuccess) {
            mipnerf_destroy(c);
            return fail(MIPNERF_E_HIP, "mipnerf_create (fp32 register-resident tables): %s", hipGetErrorString(er));
        }
    }
    if (has_bf16_pre(P)) {
        if (!pre_tables(c->pre, P->variant, total_params(*P))) {
            mipnerf_destroy(c);
            return fail(MIPNERF_E_INVALID, "mipnerf_create: embedded tables of the two-kernel bf16 form are inconsistent with the compiled plan");
        }
        const PreTables& pt = c->pre;
        add(flat(pt.gemm_pack, (size_t)pt.n_gemm_chunks * 512), true, &c->d_pre_gemm_stream);
        add(flat(pt.gemm_bias, (size_t)pt.n_gemm_bias), false, &c->d_pre_gemm_bias);
        add(flat(pt.trunk_pack, (size_t)pt.n_trunk_chunks * 512), true, &c->d_pre_trunk_stream);
        add(flat(pt.trunk_bias, (size_t)pt.n_trunk_tiles * 32), false, &c->d_pre_trunk_bias);
        if (pt.n_fused_chunks) {
            add(flat(pt.fused_pack, (size_t)pt.n_fused_chunks * 512), true, &c->d_fused_stream);
            add(flat(pt.fused_bias, (size_t)pt.n_fused_tiles * 32), false, &c->d_fused_bias);
        }
        if (er != hipSuccess) {
            mipnerf_destroy(c);
            return fail(MIPNERF_E_HIP, "mipnerf_create (tables of the two-kernel bf16 form): %s", hipGetErrorString(er));
        }
    }
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) == hipSuccess &&
        hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && cus > 0)
        c->grid_limit = cus;
    // ---- training tables (one blob per variant with generated bf16 training kernels) ----
    if (has_bf16_train_any(P) && (!train_tables(c->tt, P->variant) || c->tt.nparams != total_params(*P))) {
        mipnerf_destroy(c);
        return fail(MIPNERF_E_INVALID, "mipnerf_create: embedded training tables are inconsistent with the compiled plan");
    }
    if (has_bf16_train_any(P)) {
        const TrainTables& tt = c->tt;
        add(flat(tt.bpack, (size_t)tt.n_bchunks * 512), true, &c->d_stream_dgrad);
        chk(hipMalloc(&c->d_jobs, (size_t)tt.njobs * sizeof(mip::WgradJob)));
        chk(hipMalloc(&c->d_otab, (size_t)tt.njobs * tt.job_floats * 4));
        chk(hipMalloc(&c->d_jobslots, (size_t)tt.njobs * sizeof(int2)));
        chk(hipMalloc(&c->d_scratch, (size_t)(tt.n_scratch > 0 ? tt.n_scratch : 1) * 4));
        const int Wn = P->net_width, t_extra = 2 * P->net_depth + 2;
        std::vector<int32_t> e_xt((size_t)Wn * Wn);
        for (int i = 0; i < Wn; ++i)
            for (int j = 0; j < Wn; ++j) e_xt[(size_t)i * Wn + j] = (int32_t)((t_extra << 20) | (j * Wn + i));     // out[i][j] = W[j][i]
        add(e_xt, false, &c->d_extra_wT);      // W_extra^T: the transpose as a gather, so it joins the one pack launch
        if (er == hipSuccess) {
            chk(hipMemcpy(c->d_jobs, tt.jobs, (size_t)tt.njobs * sizeof(mip::WgradJob), hipMemcpyHostToDevice));
            chk(hipMemcpy(c->d_otab, tt.otab, (size_t)tt.njobs * tt.job_floats * 4, hipMemcpyHostToDevice));
        }
        if (er != hipSuccess) {
            mipnerf_destroy(c);
            return fail(MIPNERF_E_HIP, "mipnerf_create (training tables): %s", hipGetErrorString(er));
        }
    }
    if (has_bf16_train_any(P)) {
        const int rc = mipnerf_set_wgrad_splits(c, nullptr);
        if (rc) { mipnerf_destroy(c); return rc; }
    }
    if ((int)c->streams.size() > mip::kMaxPackSegments) {
        mipnerf_destroy(c);
        return fail(MIPNERF_E_INVALID, "mipnerf_create: more than %d packed streams", mip::kMaxPackSegments);
    }
    *out = c;
    return MIPNERF_OK;
}

int mipnerf_destroy(mipnerf_ctx* c) {
    if (!c) return MIPNERF_OK;
    for (const mipnerf_ctx::PackedStream& s : c->streams) { (void)hipFree(s.idx); (void)hipFree(s.out); }
    (void)hipFree(c->d_jobs); (void)hipFree(c->d_otab); (void)hipFree(c->d_wgtab); (void)hipFree(c->d_jobslots); (void)hipFree(c->d_scratch);
    (void)hipFree(c->d_pre_scratch);
    if (c->pre_scratch_event) (void)hipEventDestroy(c->pre_scratch_event);
    for (hipEvent_t e : c->ev) (void)hipEventDestroy(e);
    delete c;
    return MIPNERF_OK;
}

int mipnerf_set_option(mipnerf_ctx* c, int option, int value) {
    if (!c) return fail(MIPNERF_E_INVALID, "ctx is null");
    switch (option) {
        case 0: c->mlp_dma = value ? 1 : 0; return MIPNERF_OK;
        case 1: if (value < 1) return fail(MIPNERF_E_INVALID, "grid_limit < 1"); c->grid_limit = value; return MIPNERF_OK;
        case 2: c->time_mlp = value < 0 ? 0 : (value > 2 ? 2 : value); c->ev_used = 0; return MIPNERF_OK;
        case 3: c->fused_ipe = value ? 1 : 0; return MIPNERF_OK;
        case 4: c->fuse_small = value ? 1 : 0; return MIPNERF_OK;
        case 5: c->f32_resident = value ? 1 : 0; return MIPNERF_OK;
        case 6: c->fused_pre = value ? 1 : 0; return MIPNERF_OK;
        default: return fail(MIPNERF_E_INVALID, "unknown option %d", option);
    }
}

int mipnerf_num_param_tensors(const mipnerf_ctx* c) { return c ? c->P->num_param_tensors : -1; }

int mipnerf_set_params(mipnerf_ctx* c, const float* const* params_host, void* stream) {
    if (!c || !params_host) return fail(MIPNERF_E_INVALID, "null argument");
    const PlanDesc& P = *c->P;
    mip::ParamPtrs pp;
    memset(&pp, 0, sizeof pp);
    for (int i = 0; i < P.num_param_tensors; ++i) {
        if (!params_host[i]) return fail(MIPNERF_E_INVALID, "parameter tensor %d is null", i);
        pp.p[i] = params_host[i];
    }
    // every stream of the context in ONE launch: bf16 stream, fp32 stream, bias tables, and for the trainable variants the
    // transposed (dgrad) stream and W_extra^T (a gather through an index table like the others).  The bf16 forward stream and its
    // bias table read the folded view layer, which the pack kernel computes from the parameters where it meets it (FoldDesc)
    mip::PackSegments sg;
    memset(&sg, 0, sizeof sg);
    sg.fold.slot = -1;
    if (P.fold) {
        const int D = P.net_depth;
        sg.fold = mip::FoldDesc{P.num_param_tensors, P.net_width, P.net_width + P.view_dim, 2 * D + 4, 2 * D + 5, 2 * D + 2, 2 * D + 3};
    }
    for (const mipnerf_ctx::PackedStream& s : c->streams) {      // (mipnerf_create keeps the list within kMaxPackSegments)
        sg.table[sg.n] = s.idx; sg.out[sg.n] = s.out; sg.bf16[sg.n] = s.bf16 ? 1 : 0;
        sg.start[sg.n + 1] = sg.start[sg.n] + s.n;
        ++sg.n;
    }
    HIP_TRY(mip::launch_pack_multi(sg, pp, S(stream)));
    c->pp = pp;
    c->params_set = true;
    return MIPNERF_OK;
}

// ---- per-stage entry points -----------------------------------------------------------------------
int mipnerf_sample_along_rays(int64_t B, int32_t N, const float* nearp, const float* farp, const float* t_rand,
                              int32_t disparity, float* t_samples, void* stream) {
    if (B < 1 || N < 1 || !nearp || !farp || !t_samples) return fail(MIPNERF_E_INVALID, "sample_along_rays: bad argument");
    HIP_TRY(mip::launch_sample_along_rays(B, N, nearp, farp, t_rand, disparity, t_samples, S(stream)));
    return MIPNERF_OK;
}

int mipnerf_cast_rays(int64_t B, int32_t N, const float* t, const float* origins, const float* dirs, const float* radii,
                      float* means, float* covs, void* stream) {
    if (B < 1 || N < 1 || !t || !origins || !dirs || !radii) return fail(MIPNERF_E_INVALID, "cast_rays: bad argument");
    HIP_TRY(mip::launch_cast_rays(B, N, t, origins, dirs, radii, means, covs, S(stream)));
    return MIPNERF_OK;
}

int mipnerf_cast_ipe(int64_t B, int32_t N, int32_t min_deg, int32_t max_deg, int32_t disable_integration, const float* t,
                     const float* origins, const float* dirs, const float* radii, void* enc, int out_dtype, void* stream) {
    if (B < 1 || N < 1 || !t || !origins || !dirs || !radii || !enc) return fail(MIPNERF_E_INVALID, "cast_ipe: bad argument");
    if (max_deg - min_deg != 16 || min_deg < 0 || max_deg > 31)
        return fail(MIPNERF_E_UNSUPPORTED, "cast_ipe is generated for max_deg-min_deg == 16");
    HIP_TRY(mip::launch_cast_ipe(B, N, min_deg, max_deg, disable_integration, t, origins, dirs, radii, enc,
                                 out_dtype == MIPNERF_PREC_BF16, S(stream)));
    return MIPNERF_OK;
}

int mipnerf_integrated_pos_enc(int64_t M, int32_t min_deg, int32_t max_deg, const float* means, const float* covs,
                               void* enc, int out_dtype, void* stream) {
    if (M < 1 || !means || !covs || !enc) return fail(MIPNERF_E_INVALID, "integrated_pos_enc: bad argument");
    if (max_deg - min_deg != 16 || min_deg < 0 || max_deg > 31)
        return fail(MIPNERF_E_UNSUPPORTED, "integrated_pos_enc is generated for max_deg-min_deg == 16");
    HIP_TRY(mip::launch_integrated_pos_enc(M, min_deg, max_deg, means, covs, enc, out_dtype == MIPNERF_PREC_BF16, S(stream)));
    return MIPNERF_OK;
}

int mipnerf_pos_enc(int64_t B, int32_t deg, const float* viewdirs, void* out, int32_t ld, int out_dtype, void* stream) {
    if (B < 1 || deg < 0 || !viewdirs || !out || ld < 3 + 6 * deg) return fail(MIPNERF_E_INVALID, "pos_enc: bad argument");
    HIP_TRY(mip::launch_pos_enc(B, deg, viewdirs, out, ld, out_dtype == MIPNERF_PREC_BF16, S(stream)));
    return MIPNERF_OK;
}

static int mlp_forward_noise(mipnerf_ctx* c, int64_t M, int32_t N, const void* enc, const void* viewenc, int precision,
                             float* rgb_sigma, float* raw, const float* dnoise, void* stream);

int mipnerf_mlp_forward(mipnerf_ctx* c, int64_t M, int32_t N, const void* enc, const void* viewenc, int precision,
                        float* rgb_sigma, float* raw, void* stream) {
    return mlp_forward_noise(c, M, N, enc, viewenc, precision, rgb_sigma, raw, nullptr, stream);
}

static int mlp_forward_noise(mipnerf_ctx* c, int64_t M, int32_t N, const void* enc, const void* viewenc, int precision,
                             float* rgb_sigma, float* raw, const float* dnoise, void* stream) {
    if (!c || M < 1 || N < 1 || !enc || !viewenc || !rgb_sigma) return fail(MIPNERF_E_INVALID, "mlp_forward: bad argument");
    if (!c->params_set) return fail(MIPNERF_E_INVALID, "mlp_forward: mipnerf_set_params has not been called");
    if (precision == MIPNERF_PREC_BF16) {
        if (!has_bf16(c->P)) return fail(MIPNERF_E_UNSUPPORTED, "this architecture variant (xyz_dim %d) has fp32 kernels only", c->P->xyz_dim);
        if (has_bf16_pre(c->P)) {
            // the two-kernel form needs 1.5 KiB of scratch per sample between its kernels; this per-stage entry point has no workspace
            // argument, so the context keeps a buffer that grows on demand (hipMalloc: not capturable -- mipnerf_forward uses the caller's)
            const size_t need = pre_x_bytes(M) + pre_acc_bytes(M);
            // ONE buffer per context: a call on another stream than the previous one waits for that call's kernels (event recorded behind
            // them below) before it overwrites the buffer; a regrow waits for every user
            if (!c->pre_scratch_event) { HIP_TRY(hipEventCreateWithFlags(&c->pre_scratch_event, hipEventDisableTiming)); }
            if (need > c->pre_scratch_bytes) {
                HIP_TRY(hipStreamSynchronize(S(stream)));
                if (c->pre_scratch_used) { HIP_TRY(hipEventSynchronize(c->pre_scratch_event)); }
                (void)hipFree(c->d_pre_scratch);
                c->d_pre_scratch = nullptr; c->pre_scratch_bytes = 0;
                HIP_TRY(hipMalloc(&c->d_pre_scratch, need));
                c->pre_scratch_bytes = need;
            } else if (c->pre_scratch_used && c->pre_scratch_stream != stream) {
                HIP_TRY(hipStreamWaitEvent(S(stream), c->pre_scratch_event, 0));
            }
            HIP_TRY(launch_bf16_pre(c, enc, 0, viewenc, rgb_sigma, raw, M, N, c->d_pre_scratch, (char*)c->d_pre_scratch + pre_x_bytes(M), dnoise, S(stream)));
            HIP_TRY(hipEventRecord(c->pre_scratch_event, S(stream)));
            c->pre_scratch_stream = stream; c->pre_scratch_used = true;
            return MIPNERF_OK;
        }
        HIP_TRY(launch_bf16_variant(c, enc, viewenc, rgb_sigma, raw, M, N, c->mlp_dma != 0, nullptr, dnoise, S(stream)));
    } else if (precision == MIPNERF_PREC_FP32 && c->f32_resident && c->d_stream_f32r) {
        // register-resident kernel (generated per variant, gen_mlp_f32r.py): activations in registers, weights through an LDS ring
        HIP_TRY(mip::kLaunchF32R[c->P->variant](c->d_stream_f32r, c->d_aux_f32r, (const float*)enc, (const float*)viewenc, rgb_sigma, raw, M, N,
                                                c->cfg.density_bias, c->cfg.rgb_padding, c->grid_limit, dnoise, c->cfg.density_noise, S(stream)));
    } else if (precision == MIPNERF_PREC_FP32) {
        HIP_TRY(mip::launch_mlp_f32(f32net_with_heads(c), c->d_stream_f32, c->d_bias, (const float*)enc, (const float*)viewenc,
                                    rgb_sigma, raw, M, N, c->cfg.density_bias, c->cfg.rgb_padding, nullptr, nullptr, dnoise,
                                    c->cfg.density_noise, S(stream)));
    } else {
        return fail(MIPNERF_E_INVALID, "unknown precision %d", precision);
    }
    return MIPNERF_OK;
}

int mipnerf_volumetric_rendering(int64_t B, int32_t N, const float* rgb_sigma, const float* t, const float* dirs,
                                 int32_t white_bkgd, float* comp_rgb, float* distance, float* acc, float* weights,
                                 void* stream) {
    if (B < 1 || N < 1 || N > MIPNERF_MAX_SAMPLES || !rgb_sigma || !t || !dirs || !comp_rgb || !distance || !acc || !weights)
        return fail(MIPNERF_E_INVALID, "volumetric_rendering: bad argument");
    HIP_TRY(mip::launch_volumetric_rendering(B, N, rgb_sigma, t, dirs, white_bkgd, comp_rgb, distance, acc, weights,
                                             S(stream)));
    return MIPNERF_OK;
}

int mipnerf_resample_along_rays(int64_t B, int32_t N, const float* t, const float* weights, const float* u_rand,
                                float resample_padding, float* t_new, void* stream) {
    if (B < 1 || N < 1 || N > MIPNERF_MAX_SAMPLES || !t || !weights || !t_new)
        return fail(MIPNERF_E_INVALID, "resample_along_rays: bad argument");
    HIP_TRY(mip::launch_piecewise_constant_pdf(B, N, t, weights, N + 1, u_rand, true, resample_padding, t_new, S(stream)));
    return MIPNERF_OK;
}

int mipnerf_sorted_piecewise_constant_pdf(int64_t B, int32_t nbins, const float* bins, const float* weights,
                                          int32_t ndraws, const float* u_rand, float* samples, void* stream) {
    if (B < 1 || nbins < 1 || nbins > MIPNERF_MAX_SAMPLES || ndraws < 1 || !bins || !weights || !samples)
        return fail(MIPNERF_E_INVALID, "sorted_piecewise_constant_pdf: bad argument");
    HIP_TRY(mip::launch_piecewise_constant_pdf(B, nbins, bins, weights, ndraws, u_rand, false, 0.0f, samples, S(stream)));
    return MIPNERF_OK;
}

// ---- unbounded scenes (mip-NeRF 360): what the reference's dead code at mip.py:106-124, 292-319, 424-447 aims at ----
int mipnerf_sample_along_rays_360(int64_t B, int32_t N, const float* nearp, const float* farp, const float* t_rand,
                                  float* t_inv, float* t_samples, void* stream) {
    if (B < 1 || N < 1 || !nearp || !farp || !t_inv || !t_samples) return fail(MIPNERF_E_INVALID, "sample_along_rays_360: bad argument");
    HIP_TRY(mip::launch_sample_along_rays_360(B, N, nearp, farp, t_rand, t_inv, t_samples, S(stream)));
    return MIPNERF_OK;
}

int mipnerf_cast_ipe_360(int64_t B, int32_t N, int32_t min_deg, int32_t max_deg, int32_t contracted, const float* t,
                         const float* origins, const float* dirs, const float* radii, void* enc, int out_dtype, float* means,
                         float* covs, void* stream) {
    if (B < 1 || N < 1 || !t || !origins || !dirs || !radii || (!enc && !means) || ((means == nullptr) != (covs == nullptr)))
        return fail(MIPNERF_E_INVALID, "cast_ipe_360: bad argument");
    if (min_deg < 0 || max_deg <= min_deg || max_deg > 31) return fail(MIPNERF_E_INVALID, "cast_ipe_360: need 0 <= min_deg < max_deg <= 31");
    const bool frag = out_dtype == MIPNERF_OUT_BF16_FRAGMENTS;
    if (frag && (!enc || means)) return fail(MIPNERF_E_INVALID, "cast_ipe_360: the fragment layout is an encoding-only output");
    HIP_TRY(mip::launch_cast_ipe_360(B, N, min_deg, max_deg, contracted, t, origins, dirs, radii, enc,
                                     out_dtype == MIPNERF_PREC_BF16 || frag, means, covs, S(stream), frag));
    return MIPNERF_OK;
}

int mipnerf_gauss_360(int64_t M, int32_t min_deg, int32_t max_deg, int32_t contracted, const float* means, const float* covs,
                      void* enc, int out_dtype, float* means_out, float* covs_out, void* stream) {
    if (M < 1 || !means || !covs || (!enc && !means_out)) return fail(MIPNERF_E_INVALID, "gauss_360: bad argument");
    if (enc && (min_deg < 0 || max_deg <= min_deg || max_deg > 31)) return fail(MIPNERF_E_INVALID, "gauss_360: need 0 <= min_deg < max_deg <= 31");
    HIP_TRY(mip::launch_gauss_360(M, min_deg, enc ? max_deg : min_deg + 1, contracted, means, covs, enc, out_dtype == MIPNERF_PREC_BF16,
                                  means_out, covs_out, S(stream)));
    return MIPNERF_OK;
}

// ---- device-side ray generation (datasets/datasets.py:116-168, 214-263) ---------------------------------------
int mipnerf_num_camera_modes(void) { return camera_models::NUM_CAMERA_MODES; }

int mipnerf_generate_rays(int64_t n, const float* cameras, const int32_t* cam_idx, const int32_t* pix_idx,
                          const mipnerf_rays_out* out, void* stream) {
    if (n < 1 || !cameras || !out || !out->origins || !out->directions || !out->viewdirs || !out->radii ||
        !out->lossmult || !out->near || !out->far)
        return fail(MIPNERF_E_INVALID, "generate_rays: bad argument");
    HIP_TRY(mip::launch_generate_rays(n, cameras, cam_idx, pix_idx, out->origins, out->directions, out->viewdirs,
                                      out->radii, out->lossmult, out->near, out->far, S(stream)));
    return MIPNERF_OK;
}

int mipnerf_generate_rays_f64(int64_t n, const double* cameras, const int32_t* cam_idx, const int32_t* pix_idx,
                              const mipnerf_rays_out* out, void* stream) {
    if (n < 1 || !cameras || !out || !out->origins || !out->directions || !out->viewdirs || !out->radii ||
        !out->lossmult || !out->near || !out->far)
        return fail(MIPNERF_E_INVALID, "generate_rays_f64: bad argument");
    HIP_TRY(mip::launch_generate_rays_f64(n, cameras, cam_idx, pix_idx, out->origins, out->directions, out->viewdirs,
                                          out->radii, out->lossmult, out->near, out->far, S(stream)));
    return MIPNERF_OK;
}

int mipnerf_gather_train_batch(int64_t batch_size, int64_t n_order, const int64_t* order, int32_t n_images, const int64_t* offsets,
                               const float* cameras, const float* pixels, const int64_t* step, const int64_t* epoch_base,
                               const mipnerf_rays_out* out, float* gt, void* stream) {
    if (batch_size < 1 || n_order < 0 || n_images < 1 || !order || !offsets || !cameras || !pixels || !step || !epoch_base || !out ||
        !out->origins || !out->directions || !out->viewdirs || !out->radii || !out->lossmult || !out->near || !out->far || !gt)
        return fail(MIPNERF_E_INVALID, "gather_train_batch: bad argument");
    HIP_TRY(mip::launch_gather_train_batch(batch_size, n_order, order, n_images, offsets, cameras, pixels, step, epoch_base, out->origins,
                                           out->directions, out->viewdirs, out->radii, out->lossmult, out->near, out->far, gt, S(stream)));
    return MIPNERF_OK;
}

// ---- error-guided batch sampling (kernels_guided.hip) --------------------------------------------------------------------------
int mipnerf_guided_apply(int64_t batch_size, int64_t n_order, int64_t ring_len, const float* weight, const int64_t* step,
                         const int64_t* epoch_base, int64_t host_batch, float* lossmult, void* stream) {
    if (batch_size < 1 || n_order < 0 || ring_len < 1 || !weight || !lossmult)
        return fail(MIPNERF_E_INVALID, "guided_apply: bad argument");
    if ((step == nullptr) != (epoch_base == nullptr))
        return fail(MIPNERF_E_INVALID, "guided_apply: step and epoch_base must both be given (device batch index) or both null (host_batch)");
    HIP_TRY(mip::launch_guided_apply(batch_size, n_order, ring_len, weight, step, epoch_base, host_batch, lossmult, S(stream)));
    return MIPNERF_OK;
}

int mipnerf_guided_accumulate(int64_t batch_size, int64_t n_order, int64_t ring_len, const int32_t* cell, int64_t n_cells,
                              const int64_t* step, const int64_t* epoch_base, int64_t host_batch, const float* rgb, const float* gt,
                              uint64_t* sum, uint32_t* cnt, void* stream) {
    if (batch_size < 1 || n_order < 0 || ring_len < 1 || n_cells < 1 || !cell || !rgb || !gt || !sum || !cnt)
        return fail(MIPNERF_E_INVALID, "guided_accumulate: bad argument");
    if ((step == nullptr) != (epoch_base == nullptr))
        return fail(MIPNERF_E_INVALID, "guided_accumulate: step and epoch_base must both be given (device batch index) or both null (host_batch)");
    HIP_TRY(mip::launch_guided_accumulate(batch_size, n_order, ring_len, cell, n_cells, step, epoch_base, host_batch, rgb, gt,
                                          reinterpret_cast<unsigned long long*>(sum), cnt, S(stream)));
    return MIPNERF_OK;
}

int mipnerf_guided_refresh(int32_t n_images, const int64_t* table, int32_t tile, int64_t n_cells, float rate, double mix, float* err,
                           uint64_t* sum, uint32_t* cnt, uint8_t* seen, uint32_t* q, uint32_t* cdf, uint64_t* scratch,
                           size_t scratch_words, uint64_t* header, void* stream) {
    if (n_images < 1 || !table || tile < 1 || !err || !sum || !cnt || !seen || !q || !cdf || !scratch || !header)
        return fail(MIPNERF_E_INVALID, "guided_refresh: bad argument");
    if (n_cells < 1 || n_cells >= ((int64_t)1 << 30))
        return fail(MIPNERF_E_INVALID, "guided_refresh: n_cells must be in [1, 2^30) (got %lld)", (long long)n_cells);
    if (!(rate > 0.0f && rate <= 1.0f)) return fail(MIPNERF_E_INVALID, "guided_refresh: rate must be in (0, 1] (got %g)", (double)rate);
    if (!(mix >= 0.0 && mix < 1.0)) return fail(MIPNERF_E_INVALID, "guided_refresh: mix must be in [0, 1) (got %g)", mix);
    if (scratch_words < (size_t)(2 * mip::guided_num_blocks(n_cells) + 2))
        return fail(MIPNERF_E_WORKSPACE, "guided_refresh: scratch holds %zu words, %lld are needed", scratch_words,
                    (long long)(2 * mip::guided_num_blocks(n_cells) + 2));
    HIP_TRY(mip::launch_guided_refresh(n_images, table, tile, n_cells, rate, mix, err, reinterpret_cast<unsigned long long*>(sum), cnt, seen, q,
                                       cdf, reinterpret_cast<unsigned long long*>(scratch), reinterpret_cast<unsigned long long*>(header),
                                       S(stream)));
    return MIPNERF_OK;
}

int mipnerf_guided_draw(int64_t n_draws, const int64_t* r, int32_t n_images, const int64_t* table, int32_t tile, int64_t n_cells,
                        const uint32_t* cdf, const uint64_t* header, int64_t* order, float* weight, int32_t* cell, int64_t ring_len,
                        int64_t ring_start, void* stream) {
    if (n_draws < 0 || n_images < 1 || !table || tile < 1 || n_cells < 1 || n_cells >= ((int64_t)1 << 30) || !cdf || !header || !weight ||
        !cell || ring_len < 1 || ring_start < 0)
        return fail(MIPNERF_E_INVALID, "guided_draw: bad argument");
    if (n_draws > ring_len) return fail(MIPNERF_E_INVALID, "guided_draw: %lld draws do not fit a ring of %lld", (long long)n_draws, (long long)ring_len);
    if (n_draws == 0) return MIPNERF_OK;
    if (!r || !order) return fail(MIPNERF_E_INVALID, "guided_draw: null argument");
    HIP_TRY(mip::launch_guided_draw(n_draws, r, n_images, table, tile, n_cells, cdf, reinterpret_cast<const unsigned long long*>(header), order,
                                    weight, cell, ring_len, ring_start, S(stream)));
    return MIPNERF_OK;
}

// ---- evaluation metrics (utils/metrics.py:191-197) ---------------------------------------------------------------
int64_t mipnerf_eval_workspace_floats(int32_t height, int32_t width) {
    return height > 0 && width > 0 ? mip::eval_errors_partial_floats(height, width) : 0;
}

int mipnerf_eval_errors(int32_t H, int32_t W, const float* pred, const float* gt, float* workspace, float* out_psnr_ssim,
                        void* stream) {
    if (H < 1 || W < 1 || !pred || !gt || !workspace || !out_psnr_ssim) return fail(MIPNERF_E_INVALID, "eval_errors: bad argument");
    HIP_TRY(mip::launch_eval_errors(H, W, pred, gt, workspace, out_psnr_ssim, S(stream)));
    return MIPNERF_OK;
}

// ---- image bytes (utils/vis.py:save_images) -----------------------------------------------------------------------
static constexpr int64_t kMaxImageValues = 1LL << 36;     // keeps every grid dimension of kernels_vis.hip below 2^31

int64_t mipnerf_visualize_workspace_floats(int64_t n) { return n > 0 && n <= kMaxImageValues ? mip::visualize_partial_floats(n) : 0; }

int mipnerf_visualize_map(int64_t n, const float* map, float* workspace, uint8_t* out_rgb, void* stream) {
    if (n < 1 || n > kMaxImageValues || !map || !workspace || !out_rgb) return fail(MIPNERF_E_INVALID, "visualize_map: bad argument");
    HIP_TRY(mip::launch_visualize_map(n, map, workspace, out_rgb, S(stream)));
    return MIPNERF_OK;
}

int mipnerf_image_to_u8(int64_t n, const float* x, uint8_t* out, void* stream) {
    if (n < 1 || n > kMaxImageValues || !x || !out) return fail(MIPNERF_E_INVALID, "image_to_u8: bad argument");
    HIP_TRY(mip::launch_image_to_u8(n, x, out, S(stream)));
    return MIPNERF_OK;
}

// ---- multi-scale converter (datasets/convert_blender_data.py:34-37, 65-81) ----------------------------------------
int mipnerf_box_pyramid(int32_t n, int32_t H, int32_t W, int32_t n_levels, const uint8_t* src_rgba, uint8_t* out_u8, float* out_rgb,
                        int64_t rgb_row_offset, int32_t white_bkgd, float* scratch, void* stream) {
    if (n_levels < 1 || n_levels > MIPNERF_MAX_PYRAMID_LEVELS) return fail(MIPNERF_E_INVALID, "box_pyramid: n_levels must be in [1, %d]", MIPNERF_MAX_PYRAMID_LEVELS);
    if (n < 1 || H < 1 || W < 1 || (int64_t)n * H * W > kMaxImageValues / 4) return fail(MIPNERF_E_INVALID, "box_pyramid: bad image count or size");
    const int T = 1 << (n_levels - 1);
    if (H % T || W % T) return fail(MIPNERF_E_INVALID, "box_pyramid: %d x %d (H x W) is not divisible by 2^(n_levels-1) = %d", H, W, T);
    if (!src_rgba || !out_u8 || (n_levels > 4 && !scratch)) return fail(MIPNERF_E_INVALID, "box_pyramid: null argument");
    if (rgb_row_offset < 0) return fail(MIPNERF_E_INVALID, "box_pyramid: negative row offset");
    if (((uintptr_t)src_rgba | (uintptr_t)out_u8 | (uintptr_t)scratch) & 15 || ((uintptr_t)out_rgb & 3))
        return fail(MIPNERF_E_INVALID, "box_pyramid: src, out_u8 and scratch must be 16-byte aligned, out_rgb 4-byte aligned");
    HIP_TRY(mip::launch_box_pyramid(n, H, W, n_levels, src_rgba, out_u8, out_rgb ? out_rgb + 3 * rgb_row_offset : nullptr, white_bkgd != 0,
                                    scratch, S(stream)));
    return MIPNERF_OK;
}

// ---- box shrink of captured images (datasets.load_realdata360 off images/) -------------------------------------------
int mipnerf_area_downscale(int32_t n, int32_t H, int32_t W, int32_t C, int32_t F, const uint8_t* src, float* out_rgb, int64_t rgb_row_offset,
                           void* stream) {
    if (F < 1 || F > MIPNERF_MAX_DOWNSCALE_FACTOR) return fail(MIPNERF_E_INVALID, "area_downscale: factor must be in [1, %d]", MIPNERF_MAX_DOWNSCALE_FACTOR);
    if (C != 3 && C != 4) return fail(MIPNERF_E_INVALID, "area_downscale: channels must be 3 or 4");
    if (n < 1 || H < F || W < F || (int64_t)n * H * W > kMaxImageValues / 4) return fail(MIPNERF_E_INVALID, "area_downscale: bad image count or size");
    if (!src || !out_rgb) return fail(MIPNERF_E_INVALID, "area_downscale: null argument");
    if (rgb_row_offset < 0) return fail(MIPNERF_E_INVALID, "area_downscale: negative row offset");
    if (((uintptr_t)src & 15) || ((uintptr_t)out_rgb & 3)) return fail(MIPNERF_E_INVALID, "area_downscale: src must be 16-byte aligned, out_rgb 4-byte aligned");
    HIP_TRY(mip::launch_area_downscale(n, H, W, C, F, src, out_rgb + 3 * rgb_row_offset, S(stream)));
    return MIPNERF_OK;
}

// ---- geometry out of a trained field (kernels_mesh.hip) -----------------------------------------------------------------
static constexpr size_t kGridViewBytes = 256;                       // one zero view-encoding row [32] of either dtype, 256-aligned
static inline size_t grid_row_bytes(int precision) { return (size_t)96 * (precision == MIPNERF_PREC_BF16 ? 2 : 4) + 16; }

static int lattice_check(const char* who, const int32_t* dims, const float* lo, const float* hi) {
    if (!dims || !lo || !hi) return fail(MIPNERF_E_INVALID, "%s: null argument", who);
    for (int a = 0; a < 3; ++a) {
        if (dims[a] < 2) return fail(MIPNERF_E_INVALID, "%s: a lattice needs at least 2 points per axis (got %d x %d x %d)", who, dims[0], dims[1], dims[2]);
        if (!(std::isfinite(lo[a]) && std::isfinite(hi[a]))) return fail(MIPNERF_E_INVALID, "%s: the box is not finite", who);
    }
    if (7 * (int64_t)dims[0] * dims[1] * dims[2] >= (1LL << 31))
        return fail(MIPNERF_E_INVALID, "%s: %d x %d x %d lattice points: indices are 32-bit, 7 nx ny nz must stay below 2^31", who, dims[0], dims[1], dims[2]);
    return MIPNERF_OK;
}

size_t mipnerf_density_grid_workspace_bytes(const mipnerf_ctx* c, int64_t chunk_points, int precision) {
    if (!c || chunk_points < 1 || (precision != MIPNERF_PREC_FP32 && precision != MIPNERF_PREC_BF16)) return 0;
    return kGridViewBytes + (size_t)chunk_points * grid_row_bytes(precision);
}

int mipnerf_density_grid(mipnerf_ctx* c, const int32_t* dims, const float* lo, const float* hi, float cov_scale, int precision,
                         float* sigma, void* workspace, size_t workspace_bytes, void* stream) {
    if (!c || !sigma || !workspace) return fail(MIPNERF_E_INVALID, "density_grid: null argument");
    if (int rc = lattice_check("density_grid", dims, lo, hi)) return rc;
    if (precision != MIPNERF_PREC_FP32 && precision != MIPNERF_PREC_BF16) return fail(MIPNERF_E_INVALID, "density_grid: unknown precision %d", precision);
    if (!(cov_scale >= 0.0f) || !std::isfinite(cov_scale)) return fail(MIPNERF_E_INVALID, "density_grid: cov_scale must be finite and >= 0");
    if (c->cfg.unbounded) return fail(MIPNERF_E_UNSUPPORTED, "density_grid: the unbounded-scene model lives in a contracted space; its lattice is not implemented");
    if (c->cfg.max_deg_point - c->cfg.min_deg_point != 16 || c->cfg.min_deg_point < 0 || c->cfg.max_deg_point > 31)
        return fail(MIPNERF_E_UNSUPPORTED, "density_grid: the lattice encoder is generated for max_deg_point - min_deg_point == 16");
    if ((uintptr_t)workspace & 15) return fail(MIPNERF_E_INVALID, "density_grid: the workspace must be 16-byte aligned");
    const size_t row = grid_row_bytes(precision);
    if (workspace_bytes < kGridViewBytes + row) return fail(MIPNERF_E_WORKSPACE, "density_grid: the workspace holds no lattice point (see mipnerf_density_grid_workspace_bytes)");
    const int64_t n = (int64_t)dims[0] * dims[1] * dims[2];
    int64_t chunk = (int64_t)((workspace_bytes - kGridViewBytes) / row);
    if (chunk > n) chunk = n;
    if (chunk > 256) chunk -= chunk % 256;                             // whole MLP tiles except in the last chunk
    // workspace: zero view row | activated outputs [chunk, 4] | encoding rows [chunk, 96]
    char* ws = (char*)workspace;
    float* rgb_sigma = (float*)(ws + kGridViewBytes);
    void* enc = ws + kGridViewBytes + (size_t)chunk * 16;
    HIP_TRY(hipMemsetAsync(ws, 0, kGridViewBytes, S(stream)));
    for (int64_t first = 0; first < n; first += chunk) {
        const int64_t m = n - first < chunk ? n - first : chunk;
        HIP_TRY(mip::launch_lattice_ipe(dims, lo, hi, first, m, cov_scale, c->cfg.min_deg_point, c->cfg.max_deg_point, enc,
                                        precision == MIPNERF_PREC_BF16, S(stream)));
        // num_samples = m: every point of the chunk reads view row 0
        if (int rc = mipnerf_mlp_forward(c, m, (int32_t)m, enc, ws, precision, rgb_sigma, nullptr, stream)) return rc;
        HIP_TRY(mip::launch_store_sigma(m, rgb_sigma, sigma + first, S(stream)));
    }
    return MIPNERF_OK;
}

// ---- the same for the unbounded-scene model (kernels_360.hip) ---------------------------------------------------------------
// bf16 runs the one-kernel form on fragments where the variant has one (and option 6 has not switched it off); the two-kernel form
// needs its 1.5 KiB per point of scratch between the kernels
static inline bool grid360_one_kernel(const mipnerf_ctx* c) {
    return c->fused_pre && c->d_fused_stream && mip::kLaunchBf16Fused[c->P->variant] != nullptr;
}
// workspace: zero view row | encoding (fp32 rows, or bf16 fragments of whole 256-point tiles) | pre_x | pre_acc | activated outputs [chunk, 4];
// strictly increasing in the chunk, so the chunk a workspace holds is well defined
static size_t grid360_bytes(const mipnerf_ctx* c, int64_t chunk, int precision) {
    size_t b = kGridViewBytes + (size_t)chunk * 16;
    if (precision == MIPNERF_PREC_BF16) {
        b += pre_frag_bytes(c, (size_t)chunk);
        if (!grid360_one_kernel(c)) b += pre_x_bytes(chunk) + pre_acc_bytes(chunk);
    } else {
        b += (size_t)chunk * c->P->xyz_dim * 4;
    }
    return b;
}
static int grid360_check(const char* who, const mipnerf_ctx* c, int precision) {
    if (!c->cfg.unbounded) return fail(MIPNERF_E_UNSUPPORTED, "%s: a bounded model; its lattice is mipnerf_density_grid", who);
    if (!max_deg_span_is_16(c->cfg) || c->P->xyz_dim != 42 * 16)
        return fail(MIPNERF_E_UNSUPPORTED, "%s: the lattice encoder is generated for max_deg_point - min_deg_point == 16", who);
    if (precision == MIPNERF_PREC_BF16 && !has_bf16_pre(c->P))
        return fail(MIPNERF_E_UNSUPPORTED, "%s: this architecture variant has no bf16 kernel for the 672-wide encoding", who);
    return MIPNERF_OK;
}
static int lattice360_args(const char* who, const int32_t* dims, const float* lo, const float* hi, float cov_scale, int space, float far_radius,
                           int precision) {
    if (int rc = lattice_check(who, dims, lo, hi)) return rc;
    if (space != MIPNERF_SPACE_WORLD && space != MIPNERF_SPACE_CONTRACTED) return fail(MIPNERF_E_INVALID, "%s: unknown space %d", who, space);
    if (!(std::isfinite(far_radius) && far_radius > 1.0f)) return fail(MIPNERF_E_INVALID, "%s: far_radius must be finite and > 1", who);
    if (!(cov_scale >= 0.0f) || !std::isfinite(cov_scale)) return fail(MIPNERF_E_INVALID, "%s: cov_scale must be finite and >= 0", who);
    if (precision != MIPNERF_PREC_FP32 && precision != MIPNERF_PREC_BF16) return fail(MIPNERF_E_INVALID, "%s: unknown precision %d", who, precision);
    return MIPNERF_OK;
}

size_t mipnerf_density_grid_360_workspace_bytes(const mipnerf_ctx* c, int64_t chunk_points, int precision) {
    if (!c || chunk_points < 1 || (precision != MIPNERF_PREC_FP32 && precision != MIPNERF_PREC_BF16)) return 0;
    if (!c->cfg.unbounded || c->P->xyz_dim != 42 * 16 || (precision == MIPNERF_PREC_BF16 && !has_bf16_pre(c->P))) return 0;
    return grid360_bytes(c, chunk_points, precision);
}

int mipnerf_density_grid_360(mipnerf_ctx* c, const int32_t* dims, const float* lo, const float* hi, float cov_scale, int space,
                             float far_radius, int precision, float* sigma, void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = lattice360_args("density_grid_360", dims, lo, hi, cov_scale, space, far_radius, precision)) return rc;
    if (!c || !sigma || !workspace) return fail(MIPNERF_E_INVALID, "density_grid_360: null argument");
    if (int rc = grid360_check("density_grid_360", c, precision)) return rc;
    if (!c->params_set) return fail(MIPNERF_E_INVALID, "density_grid_360: mipnerf_set_params has not been called");
    if ((uintptr_t)workspace & 255) return fail(MIPNERF_E_INVALID, "density_grid_360: the workspace must be 256-byte aligned");
    const int64_t n = (int64_t)dims[0] * dims[1] * dims[2];
    if (workspace_bytes < grid360_bytes(c, 1, precision))
        return fail(MIPNERF_E_WORKSPACE, "density_grid_360: the workspace holds no lattice point (see mipnerf_density_grid_360_workspace_bytes)");
    int64_t chunk = 1, up = n;                                         // the largest chunk the workspace holds
    while (chunk < up) {
        const int64_t mid = chunk + (up - chunk + 1) / 2;
        if (grid360_bytes(c, mid, precision) <= workspace_bytes) chunk = mid; else up = mid - 1;
    }
    if (chunk > 256 && chunk < n) chunk -= chunk % 256;                // whole MLP tiles except in the last chunk
    const bool bf16 = precision == MIPNERF_PREC_BF16;
    char* ws = (char*)workspace;
    char* enc = ws + kGridViewBytes;
    char* pre_x = enc + (bf16 ? pre_frag_bytes(c, (size_t)chunk) : (size_t)chunk * c->P->xyz_dim * 4);
    char* pre_acc = pre_x + (bf16 && !grid360_one_kernel(c) ? pre_x_bytes(chunk) : 0);
    float* rgb_sigma = (float*)(pre_acc + (bf16 && !grid360_one_kernel(c) ? pre_acc_bytes(chunk) : 0));
    const float cap = 2.0f - 1.0f / far_radius;
    HIP_TRY(hipMemsetAsync(ws, 0, kGridViewBytes, S(stream)));
    for (int64_t first = 0; first < n; first += chunk) {
        const int64_t m = n - first < chunk ? n - first : chunk;
        HIP_TRY(mip::launch_lattice_ipe_360(dims, lo, hi, first, m, cov_scale, space == MIPNERF_SPACE_WORLD, c->cfg.min_deg_point,
                                            c->cfg.max_deg_point, enc, bf16, bf16, S(stream)));
        // num_samples = m: every point of the chunk reads view row 0
        if (bf16) {
            HIP_TRY(launch_bf16_pre(c, enc, 1, ws, rgb_sigma, nullptr, m, (int)m, pre_x, pre_acc, nullptr, S(stream)));
        } else if (int rc = mipnerf_mlp_forward(c, m, (int32_t)m, enc, ws, precision, rgb_sigma, nullptr, stream)) {
            return rc;
        }
        if (space == MIPNERF_SPACE_CONTRACTED) {
            HIP_TRY(mip::launch_store_sigma_360(dims, lo, hi, first, m, cap * cap, rgb_sigma, sigma, S(stream)));
        } else {
            HIP_TRY(mip::launch_store_sigma(m, rgb_sigma, sigma + first, S(stream)));
        }
    }
    return MIPNERF_OK;
}

int mipnerf_lattice_ipe_360(const int32_t* dims, const float* lo, const float* hi, int64_t first, int64_t count, float cov_scale, int space,
                            int32_t min_deg, int32_t max_deg, void* enc, int out_dtype, void* stream) {
    if (int rc = lattice360_args("lattice_ipe_360", dims, lo, hi, cov_scale, space, 2.0f, MIPNERF_PREC_FP32)) return rc;
    const bool frag = out_dtype == MIPNERF_OUT_BF16_FRAGMENTS;
    if (out_dtype != MIPNERF_PREC_FP32 && out_dtype != MIPNERF_PREC_BF16 && !frag) return fail(MIPNERF_E_INVALID, "lattice_ipe_360: unknown out_dtype %d", out_dtype);
    if (min_deg < 0 || max_deg <= min_deg || max_deg > 31 || (21 * (max_deg - min_deg)) % 8)
        return fail(MIPNERF_E_INVALID, "lattice_ipe_360: need 0 <= min_deg < max_deg <= 31 and max_deg - min_deg a multiple of 8");
    if (first < 0 || count < 1 || first + count > (int64_t)dims[0] * dims[1] * dims[2]) return fail(MIPNERF_E_INVALID, "lattice_ipe_360: points outside the lattice");
    if (!enc || ((uintptr_t)enc & 31)) return fail(MIPNERF_E_INVALID, "lattice_ipe_360: enc must be a 32-byte aligned device pointer");
    HIP_TRY(mip::launch_lattice_ipe_360(dims, lo, hi, first, count, cov_scale, space == MIPNERF_SPACE_WORLD, min_deg, max_deg, enc,
                                        out_dtype != MIPNERF_PREC_FP32, frag, S(stream)));
    return MIPNERF_OK;
}

int mipnerf_uncontract_vertices(int64_t V, float far_radius, const float* z, const float* normals_z, float* x_out, float* normals_out,
                                void* stream) {
    if (V < 0 || !(std::isfinite(far_radius) && far_radius > 1.0f)) return fail(MIPNERF_E_INVALID, "uncontract_vertices: far_radius must be finite and > 1, num_vertices >= 0");
    if ((normals_z == nullptr) != (normals_out == nullptr)) return fail(MIPNERF_E_INVALID, "uncontract_vertices: normals in and out go together");
    if (V == 0) return MIPNERF_OK;
    if (!z || (!x_out && !normals_out)) return fail(MIPNERF_E_INVALID, "uncontract_vertices: null argument");
    HIP_TRY(mip::launch_uncontract(V, far_radius, z, normals_z, x_out, normals_out, S(stream)));
    return MIPNERF_OK;
}

// workspace of the extraction: totals [2] (padded to 256 bytes) | vbase [n] | block_v [nb] | block_f [nb] | mask [n]
struct IsoWorkspace {
    unsigned* totals; unsigned* vbase; unsigned* block_v; unsigned* block_f; unsigned char* mask;
    size_t bytes;
};
static IsoWorkspace iso_workspace(void* base, int64_t n) {
    const size_t nb = ((size_t)mip::iso_num_blocks(n) + 63) / 64 * 64;
    const size_t np = ((size_t)n + 63) / 64 * 64;
    char* p = (char*)base;
    IsoWorkspace w;
    w.totals = (unsigned*)p;
    w.vbase = (unsigned*)(p + 256);
    w.block_v = w.vbase + np;
    w.block_f = w.block_v + nb;
    w.mask = (unsigned char*)(w.block_f + nb);
    w.bytes = 256 + 4 * (np + 2 * nb) + np;
    return w;
}

size_t mipnerf_isosurface_workspace_bytes(int32_t nx, int32_t ny, int32_t nz) {
    if (nx < 2 || ny < 2 || nz < 2 || 7 * (int64_t)nx * ny * nz >= (1LL << 31)) return 0;
    return iso_workspace(nullptr, (int64_t)nx * ny * nz).bytes;
}

int mipnerf_isosurface_count(const int32_t* dims, const float* grid, float threshold, void* workspace, size_t workspace_bytes,
                             int64_t* num_vertices_host, int64_t* num_faces_host, void* stream) {
    const float unit_lo[3] = {0.f, 0.f, 0.f}, unit_hi[3] = {1.f, 1.f, 1.f};
    if (int rc = lattice_check("isosurface_count", dims, unit_lo, unit_hi)) return rc;
    if (!grid || !workspace || !num_vertices_host || !num_faces_host) return fail(MIPNERF_E_INVALID, "isosurface_count: null argument");
    if (std::isnan(threshold)) return fail(MIPNERF_E_INVALID, "isosurface_count: the threshold is NaN");
    if ((uintptr_t)workspace & 15) return fail(MIPNERF_E_INVALID, "isosurface_count: the workspace must be 16-byte aligned");
    const IsoWorkspace w = iso_workspace(workspace, (int64_t)dims[0] * dims[1] * dims[2]);
    if (workspace_bytes < w.bytes) return fail(MIPNERF_E_WORKSPACE, "isosurface_count: workspace too small (%zu < %zu bytes)", workspace_bytes, w.bytes);
    HIP_TRY(mip::launch_iso_count(dims, grid, threshold, w.mask, w.vbase, w.block_v, w.block_f, w.totals, S(stream)));
    unsigned totals[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(totals, w.totals, sizeof(totals), hipMemcpyDeviceToHost, S(stream)));
    HIP_TRY(hipStreamSynchronize(S(stream)));
    *num_vertices_host = (int64_t)totals[0];
    *num_faces_host = (int64_t)totals[1];
    return MIPNERF_OK;
}

int mipnerf_isosurface_emit(const int32_t* dims, const float* lo, const float* hi, const float* grid, float threshold,
                            const void* workspace, size_t workspace_bytes, float* vertices, float* normals, int32_t* faces,
                            int64_t* vertex_edges, void* stream) {
    if (int rc = lattice_check("isosurface_emit", dims, lo, hi)) return rc;
    if (!grid || !workspace) return fail(MIPNERF_E_INVALID, "isosurface_emit: null argument");
    if ((uintptr_t)workspace & 15) return fail(MIPNERF_E_INVALID, "isosurface_emit: the workspace must be 16-byte aligned");
    const IsoWorkspace w = iso_workspace(const_cast<void*>(workspace), (int64_t)dims[0] * dims[1] * dims[2]);
    if (workspace_bytes < w.bytes) return fail(MIPNERF_E_WORKSPACE, "isosurface_emit: workspace too small (%zu < %zu bytes)", workspace_bytes, w.bytes);
    if (!vertices && !normals && !faces && !vertex_edges) return MIPNERF_OK;
    static_assert(sizeof(long long) == sizeof(int64_t), "vertex_edges is int64");
    HIP_TRY(mip::launch_iso_emit(dims, lo, hi, grid, threshold, w.mask, w.vbase, w.block_f, vertices, normals, faces,
                                 (long long*)vertex_edges, S(stream)));
    return MIPNERF_OK;
}

// ---- empty-space skipping for whole frames (kernels_occupancy.hip) -------------------------------------------------------
int64_t mipnerf_occupancy_words(int32_t nx, int32_t ny, int32_t nz) {
    if (nx < 2 || ny < 2 || nz < 2 || 7 * (int64_t)nx * ny * nz >= (1LL << 31)) return 0;
    return (int64_t)(ny - 1) * (nz - 1) * ((nx - 1 + 31) / 32);
}

int mipnerf_occupancy_build(const int32_t* dims, const float* grid, float threshold, int32_t dilate, uint32_t* bits, uint32_t* scratch,
                            void* stream) {
    const float unit_lo[3] = {0.f, 0.f, 0.f}, unit_hi[3] = {1.f, 1.f, 1.f};
    if (int rc = lattice_check("occupancy_build", dims, unit_lo, unit_hi)) return rc;
    if (!grid || !bits) return fail(MIPNERF_E_INVALID, "occupancy_build: null argument");
    if (std::isnan(threshold)) return fail(MIPNERF_E_INVALID, "occupancy_build: the threshold is NaN");
    if (dilate < 0) return fail(MIPNERF_E_INVALID, "occupancy_build: dilate must be >= 0 (got %d)", dilate);
    if (dilate > 0 && !scratch) return fail(MIPNERF_E_INVALID, "occupancy_build: dilate > 0 needs the scratch words");
    if (dilate > 0 && scratch == bits) return fail(MIPNERF_E_INVALID, "occupancy_build: bits and scratch must not be the same buffer");
    HIP_TRY(mip::launch_occupancy_build(dims, grid, threshold, dilate, bits, scratch, S(stream)));
    return MIPNERF_OK;
}

int mipnerf_occupancy_refresh(const int32_t* dims, const float* fresh, float* running, float decay, float threshold, int32_t dilate,
                              uint32_t* bits, uint32_t* scratch, void* stream) {
    const float unit_lo[3] = {0.f, 0.f, 0.f}, unit_hi[3] = {1.f, 1.f, 1.f};
    if (int rc = lattice_check("occupancy_refresh", dims, unit_lo, unit_hi)) return rc;
    if (!fresh || !running || !bits) return fail(MIPNERF_E_INVALID, "occupancy_refresh: null argument");
    if (!(decay >= 0.0f && decay <= 1.0f)) return fail(MIPNERF_E_INVALID, "occupancy_refresh: decay must be in [0, 1] (got %g)", (double)decay);
    if (std::isnan(threshold)) return fail(MIPNERF_E_INVALID, "occupancy_refresh: the threshold is NaN");
    if (dilate < 0) return fail(MIPNERF_E_INVALID, "occupancy_refresh: dilate must be >= 0 (got %d)", dilate);
    if (dilate > 0 && !scratch) return fail(MIPNERF_E_INVALID, "occupancy_refresh: dilate > 0 needs the scratch words");
    if (dilate > 0 && scratch == bits) return fail(MIPNERF_E_INVALID, "occupancy_refresh: bits and scratch must not be the same buffer");
    const size_t bytes = sizeof(float) * (size_t)dims[0] * dims[1] * dims[2];
    const uintptr_t f0 = (uintptr_t)fresh, r0 = (uintptr_t)running;
    if (f0 < r0 + bytes && r0 < f0 + bytes) return fail(MIPNERF_E_INVALID, "occupancy_refresh: fresh and running must not overlap");
    HIP_TRY(mip::launch_occupancy_refresh(dims, fresh, running, decay, threshold, dilate, bits, scratch, S(stream)));
    return MIPNERF_OK;
}

// what the four ray calls check before anything is launched, and the launch arguments they share; > 0: a return code, 0: launch,
// -1: zero rays, nothing to do
static int ray_occupancy_check(const char* name, const int32_t* dims, const float* lo, const float* hi, const uint32_t* bits, int64_t B,
                               int32_t N, const mipnerf_rays* rays, int32_t outside_occupied, float cone_scale, uint8_t* live,
                               mip::RayClassify* out) {
    if (int rc = lattice_check(name, dims, lo, hi)) return rc;
    for (int a = 0; a < 3; ++a)
        if (!(hi[a] > lo[a])) return fail(MIPNERF_E_INVALID, "%s: the box needs hi > lo on every axis", name);
    if (B < 0 || B >= (1LL << 31)) return fail(MIPNERF_E_INVALID, "%s: bad ray count", name);
    if (N < 1 || N > MIPNERF_MAX_SAMPLES) return fail(MIPNERF_E_INVALID, "%s: num_samples must be in [1, %d]", name, MIPNERF_MAX_SAMPLES);
    if (!(cone_scale >= 0.0f) || !std::isfinite(cone_scale)) return fail(MIPNERF_E_INVALID, "%s: cone_scale must be finite and >= 0", name);
    if (B == 0) return -1;
    if (!bits || !rays || !rays->origins || !rays->directions || !rays->radii || !rays->near || !rays->far || !live)
        return fail(MIPNERF_E_INVALID, "%s: null argument", name);
    static_assert(sizeof(int) == sizeof(int32_t), "dims / first / last are int32");
    mip::RayClassify a{};             // occupancy of a world grid, no disparity, no span outputs: the callers set what differs
    a.dims = dims; a.lo = lo; a.hi = hi; a.bits = bits;
    a.B = B; a.N = N;
    a.origins = rays->origins; a.dirs = rays->directions; a.radii = rays->radii; a.nearp = rays->near; a.farp = rays->far;
    a.outside_occupied = outside_occupied != 0; a.cone_scale = cone_scale;
    a.live = live;
    *out = a;
    return 0;
}

int mipnerf_ray_occupancy(const int32_t* dims, const float* lo, const float* hi, const uint32_t* bits, int64_t B, int32_t N,
                          const mipnerf_rays* rays, int32_t disparity, int32_t outside_occupied, float cone_scale, uint8_t* live,
                          void* stream) {
    mip::RayClassify a;
    if (int rc = ray_occupancy_check("ray_occupancy", dims, lo, hi, bits, B, N, rays, outside_occupied, cone_scale, live, &a))
        return rc < 0 ? MIPNERF_OK : rc;
    a.disparity = disparity != 0;
    HIP_TRY(mip::launch_ray_classify(a, S(stream)));
    return MIPNERF_OK;
}

int mipnerf_ray_span(const int32_t* dims, const float* lo, const float* hi, const uint32_t* bits, int64_t B, int32_t N,
                     const mipnerf_rays* rays, int32_t disparity, int32_t outside_occupied, float cone_scale, uint8_t* live,
                     int32_t* first, int32_t* last, float* near_out, float* far_out, void* stream) {
    mip::RayClassify a;
    if (int rc = ray_occupancy_check("ray_span", dims, lo, hi, bits, B, N, rays, outside_occupied, cone_scale, live, &a))
        return rc < 0 ? MIPNERF_OK : rc;
    a.disparity = disparity != 0;
    a.span = true; a.first = first; a.last = last; a.near_out = near_out; a.far_out = far_out;
    HIP_TRY(mip::launch_ray_classify(a, S(stream)));
    return MIPNERF_OK;
}

int mipnerf_ray_occupancy_360(const int32_t* dims, const float* lo, const float* hi, const uint32_t* bits, int64_t B, int32_t N,
                              const mipnerf_rays* rays, int32_t outside_occupied, float cone_scale, uint8_t* live, void* stream) {
    mip::RayClassify a;
    if (int rc = ray_occupancy_check("ray_occupancy_360", dims, lo, hi, bits, B, N, rays, outside_occupied, cone_scale, live, &a))
        return rc < 0 ? MIPNERF_OK : rc;
    a.contracted = true;
    HIP_TRY(mip::launch_ray_classify(a, S(stream)));
    return MIPNERF_OK;
}

int mipnerf_ray_span_360(const int32_t* dims, const float* lo, const float* hi, const uint32_t* bits, int64_t B, int32_t N,
                         const mipnerf_rays* rays, int32_t outside_occupied, float cone_scale, uint8_t* live, int32_t* first,
                         int32_t* last, float* near_out, float* far_out, void* stream) {
    mip::RayClassify a;
    if (int rc = ray_occupancy_check("ray_span_360", dims, lo, hi, bits, B, N, rays, outside_occupied, cone_scale, live, &a))
        return rc < 0 ? MIPNERF_OK : rc;
    a.contracted = true;
    a.span = true; a.first = first; a.last = last; a.near_out = near_out; a.far_out = far_out;
    HIP_TRY(mip::launch_ray_classify(a, S(stream)));
    return MIPNERF_OK;
}

// workspace of the compaction: the live count (8 bytes, padded to 256) | block_sum [compact_num_blocks(n)]
size_t mipnerf_compact_rays_workspace_bytes(int64_t n) {
    if (n < 0 || n >= (1LL << 31)) return 0;
    return 256 + 4 * (((size_t)mip::compact_num_blocks(n) + 63) / 64 * 64);
}

int mipnerf_compact_rays(int64_t n, const uint8_t* live, const mipnerf_rays* rays, const mipnerf_rays_out* out_rays, int32_t* out_index,
                         void* workspace, size_t workspace_bytes, int64_t* count_host, void* stream) {
    if (n < 0 || n >= (1LL << 31)) return fail(MIPNERF_E_INVALID, "compact_rays: bad ray count");
    if (!count_host) return fail(MIPNERF_E_INVALID, "compact_rays: null argument");
    *count_host = 0;
    if (n == 0) return MIPNERF_OK;
    if (!live || !rays || !out_rays || !out_index || !workspace) return fail(MIPNERF_E_INVALID, "compact_rays: null argument");
    if (((uintptr_t)workspace & 15) || ((uintptr_t)live & 3)) return fail(MIPNERF_E_INVALID, "compact_rays: the workspace must be 16-byte aligned, live 4-byte aligned");
    const size_t need = mipnerf_compact_rays_workspace_bytes(n);
    if (workspace_bytes < need) return fail(MIPNERF_E_WORKSPACE, "compact_rays: workspace too small (%zu < %zu bytes)", workspace_bytes, need);
    const float* in[7] = {rays->origins, rays->directions, rays->viewdirs, rays->radii, rays->lossmult, rays->near, rays->far};
    float* out[7] = {out_rays->origins, out_rays->directions, out_rays->viewdirs, out_rays->radii, out_rays->lossmult, out_rays->near, out_rays->far};
    for (int q = 0; q < 7; ++q)
        if (out[q] && !in[q]) return fail(MIPNERF_E_INVALID, "compact_rays: an output field has no input");
    unsigned long long* total = (unsigned long long*)workspace;
    HIP_TRY(mip::launch_compact_rays(n, live, in, out, out_index, (unsigned*)((char*)workspace + 256), total, S(stream)));
    unsigned long long host_total = 0;
    HIP_TRY(hipMemcpyAsync(&host_total, total, sizeof(host_total), hipMemcpyDeviceToHost, S(stream)));
    HIP_TRY(hipStreamSynchronize(S(stream)));
    *count_host = (int64_t)host_total;
    return MIPNERF_OK;
}

int mipnerf_scatter_frame(int64_t n, int64_t count, int32_t num_levels, const int32_t* index, const uint8_t* live, const float* nearp,
                          int32_t white_bkgd, const mipnerf_level_out* compact, const mipnerf_level_out* full, void* stream) {
    if (n < 0 || n >= (1LL << 31) || count < 0 || count > n) return fail(MIPNERF_E_INVALID, "scatter_frame: bad ray count");
    if (num_levels < 1 || num_levels > mip::kMaxScatterLevels) return fail(MIPNERF_E_INVALID, "scatter_frame: num_levels must be in [1, %d]", mip::kMaxScatterLevels);
    if (n == 0) return MIPNERF_OK;
    if (!live || !nearp || !full || (count > 0 && (!index || !compact))) return fail(MIPNERF_E_INVALID, "scatter_frame: null argument");
    const float* c_rgb[mip::kMaxScatterLevels]; const float* c_dist[mip::kMaxScatterLevels]; const float* c_acc[mip::kMaxScatterLevels];
    float* f_rgb[mip::kMaxScatterLevels]; float* f_dist[mip::kMaxScatterLevels]; float* f_acc[mip::kMaxScatterLevels];
    for (int l = 0; l < num_levels; ++l) {
        f_rgb[l] = full[l].comp_rgb; f_dist[l] = full[l].distance; f_acc[l] = full[l].acc;
        c_rgb[l] = count ? compact[l].comp_rgb : nullptr; c_dist[l] = count ? compact[l].distance : nullptr; c_acc[l] = count ? compact[l].acc : nullptr;
        if (!f_rgb[l] || !f_dist[l] || !f_acc[l] || (count > 0 && (!c_rgb[l] || !c_dist[l] || !c_acc[l])))
            return fail(MIPNERF_E_INVALID, "scatter_frame: level %d has a null comp_rgb, distance or acc", l);
    }
    HIP_TRY(mip::launch_scatter_frame(n, count, num_levels, index, live, nearp, white_bkgd, c_rgb, c_dist, c_acc, f_rgb, f_dist, f_acc,
                                      S(stream)));
    return MIPNERF_OK;
}

// ---- adaptive sample counts for whole frames (kernels_bucket.hip) ----------------------------------------------------------
// workspace of the partition: the B counts (8 bytes each, padded to 256) | block_sum [B][bucket_num_blocks(n)]
size_t mipnerf_bucket_rays_workspace_bytes(int64_t n, int32_t num_buckets) {
    if (n < 0 || n >= (1LL << 31) || num_buckets < 1 || num_buckets > mip::kMaxBuckets) return 0;
    return 256 + 4 * (((size_t)num_buckets * (size_t)mip::bucket_num_blocks(n) + 63) / 64 * 64);
}

int mipnerf_bucket_rays(int64_t n, const uint8_t* live, const int32_t* first, const int32_t* last, int32_t span_samples,
                        int32_t num_samples, int32_t num_buckets, const int32_t* ladder, const mipnerf_rays* rays,
                        const mipnerf_rays_out* out_rays, int32_t* slot, void* workspace, size_t workspace_bytes, int64_t* counts_host,
                        void* stream) {
    if (n < 0 || n >= (1LL << 31)) return fail(MIPNERF_E_INVALID, "bucket_rays: bad ray count");
    if (span_samples < 1 || span_samples > MIPNERF_MAX_SAMPLES || num_samples < 1 || num_samples > MIPNERF_MAX_SAMPLES)
        return fail(MIPNERF_E_INVALID, "bucket_rays: span_samples and num_samples must be in [1, %d]", MIPNERF_MAX_SAMPLES);
    if (num_buckets < 1 || num_buckets > mip::kMaxBuckets)
        return fail(MIPNERF_E_INVALID, "bucket_rays: the ladder has 1 to %d entries (got %d)", mip::kMaxBuckets, num_buckets);
    if (!ladder || !counts_host) return fail(MIPNERF_E_INVALID, "bucket_rays: null argument");
    mip::BucketRule rule{};
    rule.S = span_samples; rule.N = num_samples; rule.B = num_buckets;
    for (int b = 0; b < num_buckets; ++b) {
        if (ladder[b] < 1 || (b > 0 && ladder[b] <= ladder[b - 1]))
            return fail(MIPNERF_E_INVALID, "bucket_rays: the ladder must be strictly increasing from at least 1");
        rule.c[b] = ladder[b];
    }
    if (ladder[num_buckets - 1] != num_samples)
        return fail(MIPNERF_E_INVALID, "bucket_rays: the ladder must end at num_samples (%d != %d)", ladder[num_buckets - 1], num_samples);
    for (int b = 0; b < num_buckets; ++b) counts_host[b] = 0;
    if (n == 0) return MIPNERF_OK;
    if (!live || !first || !last || !rays || !out_rays || !slot || !workspace) return fail(MIPNERF_E_INVALID, "bucket_rays: null argument");
    if ((uintptr_t)workspace & 15) return fail(MIPNERF_E_INVALID, "bucket_rays: the workspace must be 16-byte aligned");
    const size_t need = mipnerf_bucket_rays_workspace_bytes(n, num_buckets);
    if (workspace_bytes < need) return fail(MIPNERF_E_WORKSPACE, "bucket_rays: workspace too small (%zu < %zu bytes)", workspace_bytes, need);
    const float* in[7] = {rays->origins, rays->directions, rays->viewdirs, rays->radii, rays->lossmult, rays->near, rays->far};
    float* out[7] = {out_rays->origins, out_rays->directions, out_rays->viewdirs, out_rays->radii, out_rays->lossmult, out_rays->near, out_rays->far};
    for (int q = 0; q < 7; ++q)
        if (out[q] && !in[q]) return fail(MIPNERF_E_INVALID, "bucket_rays: an output field has no input");
    unsigned long long* header = (unsigned long long*)workspace;
    HIP_TRY(mip::launch_bucket_rays(n, rule, live, first, last, in, out, slot, (unsigned*)((char*)workspace + 256), header, S(stream)));
    unsigned long long host_counts[mip::kMaxBuckets] = {};
    HIP_TRY(hipMemcpyAsync(host_counts, header, sizeof(unsigned long long) * num_buckets, hipMemcpyDeviceToHost, S(stream)));
    HIP_TRY(hipStreamSynchronize(S(stream)));
    for (int b = 0; b < num_buckets; ++b) counts_host[b] = (int64_t)host_counts[b];
    return MIPNERF_OK;
}

int mipnerf_gather_frame(int64_t n, int64_t compact_rows, int32_t num_levels, const int32_t* slot, const float* nearp, int32_t white_bkgd,
                         const mipnerf_level_out* compact, const mipnerf_level_out* full, void* stream) {
    if (n < 0 || n >= (1LL << 31) || compact_rows < 0 || compact_rows >= (1LL << 31)) return fail(MIPNERF_E_INVALID, "gather_frame: bad ray count");
    if (num_levels < 1 || num_levels > mip::kMaxScatterLevels) return fail(MIPNERF_E_INVALID, "gather_frame: num_levels must be in [1, %d]", mip::kMaxScatterLevels);
    if (n == 0) return MIPNERF_OK;
    if (!slot || !nearp || !full || (compact_rows > 0 && !compact)) return fail(MIPNERF_E_INVALID, "gather_frame: null argument");
    const float* c_rgb[mip::kMaxScatterLevels]; const float* c_dist[mip::kMaxScatterLevels]; const float* c_acc[mip::kMaxScatterLevels];
    float* f_rgb[mip::kMaxScatterLevels]; float* f_dist[mip::kMaxScatterLevels]; float* f_acc[mip::kMaxScatterLevels];
    for (int l = 0; l < num_levels; ++l) {
        f_rgb[l] = full[l].comp_rgb; f_dist[l] = full[l].distance; f_acc[l] = full[l].acc;
        c_rgb[l] = compact_rows ? compact[l].comp_rgb : nullptr; c_dist[l] = compact_rows ? compact[l].distance : nullptr;
        c_acc[l] = compact_rows ? compact[l].acc : nullptr;
        if (!f_rgb[l] || !f_dist[l] || !f_acc[l] || (compact_rows > 0 && (!c_rgb[l] || !c_dist[l] || !c_acc[l])))
            return fail(MIPNERF_E_INVALID, "gather_frame: level %d has a null comp_rgb, distance or acc", l);
    }
    HIP_TRY(mip::launch_gather_frame(n, compact_rows, num_levels, slot, nearp, white_bkgd, c_rgb, c_dist, c_acc, f_rgb, f_dist, f_acc,
                                     S(stream)));
    return MIPNERF_OK;
}

// ---- training-side entry points ------------------------------------------------------------------
int mipnerf_activate(int64_t M, const float* raw, float rgb_padding, float density_bias, const float* density_randn,
                     float density_noise, float* rgb_sigma, void* stream) {
    if (M < 1 || !raw || !rgb_sigma) return fail(MIPNERF_E_INVALID, "activate: bad argument");
    HIP_TRY(mip::launch_activate(M, raw, rgb_padding, density_bias, density_randn, density_noise, rgb_sigma, S(stream)));
    return MIPNERF_OK;
}

int mipnerf_volumetric_rendering_bwd(int64_t B, int32_t N, const float* rgb_sigma, const float* t, const float* dirs,
                                     int32_t white_bkgd, const float* g_rgb, const float* g_dist, const float* g_acc,
                                     const float* g_w, float rgb_padding, float* d_raw, void* stream) {
    if (B < 1 || N < 1 || N > MIPNERF_MAX_SAMPLES || !rgb_sigma || !t || !dirs || !d_raw)
        return fail(MIPNERF_E_INVALID, "volumetric_rendering_bwd: bad argument");
    HIP_TRY(mip::launch_volumetric_rendering_bwd(B, N, rgb_sigma, t, dirs, white_bkgd, g_rgb, g_dist, g_acc, g_w,
                                                 rgb_padding, d_raw, S(stream)));
    return MIPNERF_OK;
}

int mipnerf_distloss(int64_t B, int32_t N, const float* weights, const float* t, float* ray_loss, const float* g_ray,
                     float* d_w, void* stream) {
    if (B < 1 || N < 1 || N > MIPNERF_MAX_SAMPLES || !weights || !t || (!ray_loss && !d_w) || ((g_ray == nullptr) != (d_w == nullptr)))
        return fail(MIPNERF_E_INVALID, "distloss: bad argument");
    HIP_TRY(mip::launch_distloss(B, N, weights, t, ray_loss, g_ray, 0.0f, d_w, S(stream)));
    return MIPNERF_OK;
}

// ---- the fused per-ray launches of mipnerf_forward / mipnerf_train_step as stage entry points: the same launchers, fed by the caller ----
int mipnerf_composite_resample(int64_t B, int32_t N, const float* rgb_sigma, const float* t, const float* dirs, int32_t white_bkgd,
                               float* comp_rgb, float* distance, float* acc, float* weights, const float* bins, const float* u_rand,
                               float resample_padding, float* t_new, void* stream) {
    if (B < 1 || N < 1 || N > MIPNERF_MAX_SAMPLES || !rgb_sigma || !t || !dirs || !comp_rgb || !distance || !acc || !weights || !bins ||
        !t_new)
        return fail(MIPNERF_E_INVALID, "composite_resample: bad argument");
    HIP_TRY(mip::launch_composite_resample(B, N, rgb_sigma, t, dirs, white_bkgd, comp_rgb, distance, acc, weights, bins, u_rand,
                                           resample_padding, t_new, S(stream)));
    return MIPNERF_OK;
}

int mipnerf_composite_train(int64_t B, int32_t N, const float* rgb_sigma, const float* t, const float* dirs, int32_t white_bkgd,
                            float* comp_rgb, float* distance, float* acc, float* weights, float* ray_loss, float g_const, float* d_w,
                            const float* u_rand, float resample_padding, float* t_new, const float* bins, void* stream) {
    if (B < 1 || N < 1 || N > MIPNERF_MAX_SAMPLES || !rgb_sigma || !t || !dirs || !comp_rgb || !distance || !acc || !weights || !ray_loss ||
        !d_w)
        return fail(MIPNERF_E_INVALID, "composite_train: bad argument");
    HIP_TRY(mip::launch_composite_train(B, N, rgb_sigma, t, dirs, white_bkgd, comp_rgb, distance, acc, weights, ray_loss, g_const, d_w,
                                        u_rand, resample_padding, t_new, S(stream), bins));
    return MIPNERF_OK;
}

// ---- gradient through the resampler (stop_resample_grad=False, mip.py:265-279): the pieces autograd chains ------------------
int mipnerf_volumetric_rendering_bwd_t(int64_t B, int32_t N, const float* rgb_sigma, const float* t, const float* dirs,
                                       int32_t white_bkgd, const float* g_rgb, const float* g_dist, const float* g_acc,
                                       const float* g_w, float rgb_padding, float* d_raw, float* d_t, void* stream) {
    if (B < 1 || N < 1 || N > MIPNERF_MAX_SAMPLES || !rgb_sigma || !t || !dirs || !d_raw || !d_t)
        return fail(MIPNERF_E_INVALID, "volumetric_rendering_bwd_t: bad argument");
    HIP_TRY(mip::launch_volumetric_rendering_bwd(B, N, rgb_sigma, t, dirs, white_bkgd, g_rgb, g_dist, g_acc, g_w,
                                                 rgb_padding, d_raw, S(stream), d_t));
    return MIPNERF_OK;
}

int mipnerf_distloss_bwd(int64_t B, int32_t N, const float* weights, const float* t, const float* g_ray, float* d_w, float* d_t,
                         void* stream) {
    if (B < 1 || N < 1 || N > MIPNERF_MAX_SAMPLES || !weights || !t || !g_ray || !d_w || !d_t)
        return fail(MIPNERF_E_INVALID, "distloss_bwd: bad argument");
    HIP_TRY(mip::launch_distloss(B, N, weights, t, nullptr, g_ray, 0.0f, d_w, S(stream), d_t));
    return MIPNERF_OK;
}

int mipnerf_cast_ipe_bwd(int64_t B, int32_t N, int32_t min_deg, int32_t max_deg, int32_t disable_integration, const float* t,
                         const float* origins, const float* dirs, const float* radii, const float* d_enc, float* d_t, void* stream) {
    if (B < 1 || N < 1 || !t || !origins || !dirs || !radii || !d_enc || !d_t || min_deg < 0 || max_deg > 31 || max_deg <= min_deg)
        return fail(MIPNERF_E_INVALID, "cast_ipe_bwd: bad argument");
    HIP_TRY(mip::launch_cast_ipe_bwd(B, N, min_deg, max_deg, disable_integration, t, origins, dirs, radii, d_enc, d_t, S(stream)));
    return MIPNERF_OK;
}

int mipnerf_resample_along_rays_bwd(int64_t B, int32_t N, const float* t, const float* weights, const float* u_rand,
                                    float resample_padding, const float* d_t_new, float* d_weights, void* stream) {
    if (B < 1 || N < 1 || N > MIPNERF_MAX_SAMPLES || !t || !weights || !d_t_new || !d_weights)
        return fail(MIPNERF_E_INVALID, "resample_along_rays_bwd: bad argument");
    HIP_TRY(mip::launch_resample_bwd(B, N, t, weights, u_rand, resample_padding, d_t_new, d_weights, S(stream)));
    return MIPNERF_OK;
}

// ---- native MLP training step (bf16) ------------------------------------------------------------------
int mipnerf_mlp_train_sizes(const mipnerf_ctx* c, int64_t M, size_t* act_bytes, size_t* mask_bytes, size_t* delta_bytes,
                            size_t* partial_bytes) {
    if (!c || M < 1) return fail(MIPNERF_E_INVALID, "mlp_train_sizes: bad argument");
    NEED_BF16_TRAIN("mlp_train_sizes");
    const size_t n_wt = (size_t)((M + 255) / 256) * 8;          // wave tiles (32 samples) of whole workgroup tiles
    // pre-GEMM form: behind the T-blocks a 256-byte record of the encoding the forward ran on (the weight-gradient kernel reads it: the act
    // buffer describes itself, mipnerf_mlp_wgrad needs no extra argument) and the two buffers between k_pre_gemm and the trunk kernel
    if (act_bytes) *act_bytes = n_wt * c->tt.NH * 2048 + (has_bf16_train_pre(c->P) ? 256 + pre_x_bytes(M) + pre_acc_bytes(M) : 0);
    if (mask_bytes) *mask_bytes = n_wt * c->tt.NMASK * 1024;
    if (delta_bytes) *delta_bytes = n_wt * c->tt.NG * 2048;
    if (partial_bytes) *partial_bytes = (size_t)c->num_wgrad_wgs * c->tt.job_floats * 4;
    return MIPNERF_OK;
}

// enc_frag (two-kernel form only): enc is the B-operand fragment buffer of whole 256-sample tiles (launch_cast_ipe_360(..., frag = true)) instead of
// row-major rows -- what the one-call training step writes (k_pre_gemm reads fragments 40 % faster than rows)
static int mlp_forward_train_noise(mipnerf_ctx* c, int64_t M, int32_t N, const void* enc, const void* viewenc, float* rgb_sigma,
                                   float* raw, void* act, void* masks, const float* dnoise, void* stream, bool enc_frag = false) {
    if (!c || M < 1 || N < 1 || !enc || !viewenc || !rgb_sigma || !raw || !act || !masks)
        return fail(MIPNERF_E_INVALID, "mlp_forward_train: bad argument");
    NEED_BF16_TRAIN("mlp_forward_train");
    if (!c->params_set) return fail(MIPNERF_E_INVALID, "mlp_forward_train: mipnerf_set_params has not been called");
    if (has_bf16_train_pre(c->P)) {
        // enc: bf16 row-major [M, xyz_dim] (what mipnerf_cast_ipe_360 writes); it must stay valid until the backward of this act buffer
        const size_t n_wt = (size_t)((M + 255) / 256) * 8;
        char* rec = (char*)act + n_wt * c->tt.NH * 2048;
        char* pre_x = rec + 256;
        char* pre_acc = pre_x + pre_x_bytes(M);
        HIP_TRY(mip::kLaunchPreGemm[c->P->variant](c->d_pre_gemm_stream, c->d_pre_gemm_bias, enc, enc_frag ? 1 : 0, pre_x, pre_acc, M, c->grid_limit, S(stream)));
        HIP_TRY(mip::kLaunchTrainFwdPre[c->P->variant](c->d_pre_trunk_stream, c->d_pre_trunk_bias, pre_x, pre_acc, viewenc, rgb_sigma, raw, act, masks,
                                                        M, N, c->cfg.density_bias, c->cfg.rgb_padding, c->grid_limit, dnoise,
                                                        c->cfg.density_noise, S(stream)));
        HIP_TRY(mip::launch_wgrad_record_enc(rec, enc, M, enc_frag ? 0 : c->P->xyz_dim * 2, S(stream), c->P->xyz_dim / 16));
        return MIPNERF_OK;
    }
    HIP_TRY(launch_trainfwd_variant(c, enc, viewenc, rgb_sigma, raw, act, masks, M, N, nullptr, dnoise, S(stream)));
    return MIPNERF_OK;
}

int mipnerf_mlp_forward_train(mipnerf_ctx* c, int64_t M, int32_t N, const void* enc, const void* viewenc, float* rgb_sigma,
                              float* raw, void* act, void* masks, void* stream) {
    return mlp_forward_train_noise(c, M, N, enc, viewenc, rgb_sigma, raw, act, masks, nullptr, stream, false);
}

int mipnerf_mlp_forward_train_fragments(mipnerf_ctx* c, int64_t M, int32_t N, const void* enc, const void* viewenc, float* rgb_sigma,
                                        float* raw, void* act, void* masks, void* stream) {
    if (c && !has_bf16_train_pre(c->P))
        return fail(MIPNERF_E_UNSUPPORTED, "mlp_forward_train_fragments: this context has no two-kernel (pre-GEMM) training form; its kernels read row-major encodings");
    return mlp_forward_train_noise(c, M, N, enc, viewenc, rgb_sigma, raw, act, masks, nullptr, stream, true);
}

int mipnerf_mlp_dgrad(mipnerf_ctx* c, int64_t M, const float* d_raw, const void* masks, void* delta, void* stream) {
    if (!c || M < 1 || !d_raw || !masks || !delta) return fail(MIPNERF_E_INVALID, "mlp_dgrad: bad argument");
    NEED_BF16_TRAIN("mlp_dgrad");
    if (!c->params_set) return fail(MIPNERF_E_INVALID, "mlp_dgrad: mipnerf_set_params has not been called");
    HIP_TRY(launch_dgrad_variant(c, d_raw, masks, delta, M, S(stream)));
    return MIPNERF_OK;
}

// weight gradients of `n_wt` consecutive wave tiles (32 samples each; the tiles of several levels may be concatenated)
static int wgrad_tiles(mipnerf_ctx* c, int64_t n_wt, const void* act, const void* delta, float* partials, float* grad_flat,
                       int32_t accumulate, void* stream);

int mipnerf_mlp_wgrad(mipnerf_ctx* c, int64_t M, const void* act, const void* delta, float* partials, float* grad_flat,
                      int32_t accumulate, void* stream) {
    if (!c || M < 1 || !act || !delta || !partials) return fail(MIPNERF_E_INVALID, "mlp_wgrad: bad argument");
    NEED_BF16_TRAIN("mlp_wgrad");
    return wgrad_tiles(c, ((M + 255) / 256) * 8, act, delta, partials, grad_flat, accumulate, stream);
}

static int wgrad_tiles(mipnerf_ctx* c, int64_t n_wt, const void* act, const void* delta, float* partials, float* grad_flat,
                       int32_t accumulate, void* stream) {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (c->time_mlp == 2) {          // option 2 = 2: time the weight-gradient launches (bench.py --mode train roofline)
        if (c->ev_used + 2 > c->ev.size())
            for (int i = 0; i < 64; ++i) { hipEvent_t e; HIP_TRY(hipEventCreate(&e)); c->ev.push_back(e); }
        e0 = c->ev[c->ev_used]; e1 = c->ev[c->ev_used + 1]; c->ev_used += 2;
        HIP_TRY(hipEventRecord(e0, S(stream)));
    }
    const mip::WgradEnc* rec = has_bf16_train_pre(c->P) ? (const mip::WgradEnc*)((const char*)act + (size_t)n_wt * c->tt.NH * 2048) : nullptr;
    HIP_TRY(mip::launch_mlp_wgrad(act, delta, c->d_jobs, c->d_wgtab, c->num_wgrad_wgs, n_wt, c->tt.NH, c->tt.NG, partials,
                                  S(stream), rec));
    if (e1) HIP_TRY(hipEventRecord(e1, S(stream)));
    if (grad_flat) {
        if (!c->params_set) return fail(MIPNERF_E_INVALID, "mlp_wgrad: mipnerf_set_params has not been called");
        const PlanDesc& P = *c->P;
        mip::WgradPost post = {};
        if (P.use_viewdirs) {
            post.W = P.net_width; post.Wc = P.net_width_cond; post.ldv = P.net_width + P.view_dim;
            post.off_extra_w = c->tt.off_extra_w; post.off_extra_b = c->tt.off_extra_b;
            post.off_view_w = c->tt.off_view_w; post.off_view_b = c->tt.off_view_b;
            // state_dict order: ... density (2*D, 2*D+1), extra (2*D+2, +3), view (2*D+4, +5), colour
            post.extra_wT = c->d_extra_wT;
            post.extra_w = c->pp.p[2 * P.net_depth + 2]; post.extra_b = c->pp.p[2 * P.net_depth + 3];
            post.view_w = c->pp.p[2 * P.net_depth + 4];
        } else if (!accumulate) {
            // MLP.forward(x, None): extra_layer / view_layers are unused parameters (autograd leaves their .grad None) and no
            // partial feeds them: zero unless accumulating
            const int D = P.net_depth;
            for (int t = 2 * D + 2; t < 2 * D + 6; ++t)
                HIP_TRY(hipMemsetAsync(grad_flat + c->tensor_off[t], 0, (size_t)P.param_numel[t] * 4, S(stream)));
        }
        HIP_TRY(mip::launch_wgrad_reduce(partials, c->d_otab, c->d_jobslots, c->tt.njobs, grad_flat, c->d_scratch,
                                         c->tt.nparams, post, accumulate != 0, S(stream)));
    }
    return MIPNERF_OK;
}

int mipnerf_mlp_backward(mipnerf_ctx* c, int64_t M, const float* d_raw, const void* act, const void* masks, void* delta,
                         float* partials, float* grad_flat, int32_t accumulate, void* stream) {
    if (!grad_flat) return fail(MIPNERF_E_INVALID, "mlp_backward: grad_flat is null");
    int rc = mipnerf_mlp_dgrad(c, M, d_raw, masks, delta, stream);
    if (rc) return rc;
    return mipnerf_mlp_wgrad(c, M, act, delta, partials, grad_flat, accumulate, stream);
}

int mipnerf_adam_step(int64_t n, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, double lr, double beta1,
                      double beta2, double eps, int32_t step, void* stream) {
    if (n < 1 || !param || !grad || !exp_avg || !exp_avg_sq || step < 1) return fail(MIPNERF_E_INVALID, "adam_step: bad argument");
    HIP_TRY(mip::launch_adam_flat(n, param, grad, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, step, S(stream)));
    return MIPNERF_OK;
}

int mipnerf_adam_step_scheduled(int64_t n, float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                                const mipnerf_lr_schedule* sc, int64_t* step_count, float* hyper_out, void* stream) {
    if (n < 1 || !param || !grad || !exp_avg || !exp_avg_sq || !sc || !step_count || !hyper_out)
        return fail(MIPNERF_E_INVALID, "adam_step_scheduled: bad argument");
    if (sc->constant_lr <= 0.0 && (sc->lr_init <= 0.0 || sc->lr_final <= 0.0 || sc->max_steps < 1))
        return fail(MIPNERF_E_INVALID, "adam_step_scheduled: lr_init, lr_final and max_steps must be positive");
    static_assert(sizeof(mipnerf_lr_schedule) == sizeof(mip::LrSchedule), "schedule structs must match");
    mip::LrSchedule k;
    memcpy(&k, sc, sizeof k);
    HIP_TRY(mip::launch_adam_scheduled(n, param, grad, exp_avg, exp_avg_sq, k, step_count, hyper_out, S(stream)));
    return MIPNERF_OK;
}

// Replace the wgrad work split: splits_host[njobs] workgroups per job (0 = skip the job: its gradients are then
// NOT produced -- timing experiments only).  NULL restores the default (workgroups per job ~ blocks per stage + 4, all CUs handed out).
int mipnerf_set_wgrad_splits(mipnerf_ctx* c, const int32_t* splits_host) {
    if (!c) return fail(MIPNERF_E_INVALID, "ctx is null");
    NEED_BF16_TRAIN("set_wgrad_splits");
    const TrainTables& tt = c->tt;
    std::vector<int> sp(tt.njobs);
    if (splits_host) {
        for (int j = 0; j < tt.njobs; ++j) sp[j] = splits_host[j] < 0 ? 0 : splits_host[j];
    } else {
        // Workgroups per job ~ (blocks the job moves per stage) + kStageFixedBlocks: a stage costs its bytes plus a fixed part (barrier +
        // DMA latency; a job alone on 16 workgroups takes 0.09 us + 0.046 us per 2-KiB block per stage, scripts/prof_train.py
        // --experiments).  Measured on MI355X at 4096 x 128 samples per level (profiles/r03aa_wgrad_splits.txt): bytes-proportional
        // (fixed part 0) 0.954 ms, equal workgroups per job (the rounds 1-2 default; fixed part -> infinity) 0.851-0.853 ms, fixed part
        // of 4 blocks 0.817 ms -- the small jobs no longer hold 21 CUs each long after they could have finished on 11.  All of the
        // grid is handed out (largest remainders first).
        constexpr double kStageFixedBlocks = 4.0;
        std::vector<double> w(tt.njobs);
        double wsum = 0.0;
        for (int j = 0; j < tt.njobs; ++j) wsum += (w[j] = tt.jobs[j * 20 + 0] + tt.jobs[j * 20 + 1] + kStageFixedBlocks);
        int total = 0;
        std::vector<std::pair<double, int>> frac(tt.njobs);
        for (int j = 0; j < tt.njobs; ++j) {
            const double x = w[j] / wsum * c->grid_limit;
            sp[j] = (int)x < 1 ? 1 : (int)x;
            frac[j] = {x - sp[j], j};
            total += sp[j];
        }
        std::sort(frac.begin(), frac.end(), [](const std::pair<double, int>& a, const std::pair<double, int>& b) {
            return a.first > b.first || (a.first == b.first && a.second < b.second); });
        for (int k = 0; total < c->grid_limit && k < tt.njobs; ++k, ++total) ++sp[frac[k].second];
    }
    std::vector<int4> wgtab;
    std::vector<int2> slots(tt.njobs);
    for (int j = 0; j < tt.njobs; ++j) {
        slots[j] = make_int2((int)wgtab.size(), sp[j]);
        for (int k = 0; k < sp[j]; ++k) wgtab.push_back(make_int4(j, k, sp[j], (int)wgtab.size()));
    }
    if (wgtab.empty()) return fail(MIPNERF_E_INVALID, "set_wgrad_splits: no workgroups");
    HIP_TRY(hipDeviceSynchronize());
    (void)hipFree(c->d_wgtab);
    c->d_wgtab = nullptr;
    HIP_TRY(hipMalloc(&c->d_wgtab, wgtab.size() * sizeof(int4)));
    HIP_TRY(hipMemcpy(c->d_wgtab, wgtab.data(), wgtab.size() * sizeof(int4), hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(c->d_jobslots, slots.data(), slots.size() * sizeof(int2), hipMemcpyHostToDevice));
    c->num_wgrad_wgs = (int)wgtab.size();
    return MIPNERF_OK;
}



// ---- parity-mode (fp32) MLP training: fused forward that saves every layer output + GEMM-based backward ------------
// `save` = one [M, width] fp32 slot per op of the plan (shipped: layers 0..7 outputs, bottleneck, view-layer output
// [M,128] in slot 9), followed by the ReLU sign bits of the same slots (1 bit per element, f32_bits_slot_words) that the
// dgrad epilogue reads instead of the fp32 values.
size_t mipnerf_mlp_train_f32_bytes(const mipnerf_ctx* c, int64_t M, size_t* save_bytes, size_t* workspace_bytes) {
    if (!c || M < 1) return 0;
    const PlanDesc& P = *c->P;
    const size_t save = (size_t)P.num_ops * M * P.net_width * 4           // one [M, width] slot per layer (op) of the plan
                        + (size_t)P.num_ops * mip::f32_bits_slot_words(M, P.net_width) * 8;   // + their sign bits
    const int splits = kF32WgradSplits;
    const size_t wmax = P.net_width > P.net_width_cond ? P.net_width : P.net_width_cond;
    size_t part = (size_t)splits * wmax * (wmax + P.xyz_dim + 32);                 // split-K partials of the big wgrad GEMMs
    const size_t thin = (size_t)((M + 2047) / 2048) * 32 * (wmax + 1);              // per-slice partials of the thin ones
    if (thin > part) part = thin;
    const size_t ws = 2 * (size_t)M * wmax * 4 + part * 4 + 1024;
    if (save_bytes) *save_bytes = save;
    if (workspace_bytes) *workspace_bytes = ws;
    return save + ws;
}

int mipnerf_mlp_forward_train_f32(mipnerf_ctx* c, int64_t M, int32_t N, const float* enc, const float* viewenc, float* rgb_sigma,
                                  float* raw, float* save, void* stream) {
    if (!c || M < 1 || N < 1 || !enc || !viewenc || !rgb_sigma || !raw || !save)
        return fail(MIPNERF_E_INVALID, "mlp_forward_train_f32: bad argument");
    if (!c->params_set) return fail(MIPNERF_E_INVALID, "mlp_forward_train_f32: mipnerf_set_params has not been called");
    HIP_TRY(mip::launch_mlp_f32(f32net_with_heads(c), c->d_stream_f32, c->d_bias, enc, viewenc, rgb_sigma, raw, M, N, c->cfg.density_bias,
                                c->cfg.rgb_padding, save,
                                reinterpret_cast<unsigned long long*>(save + (size_t)c->P->num_ops * M * c->P->net_width), nullptr, 0.0f,
                                S(stream)));
    return MIPNERF_OK;
}

static int mlp_backward_f32_impl(mipnerf_ctx* c, int64_t M, int32_t N, const float* d_raw, const float* enc, const float* viewenc,
                                 const float* save, void* workspace, float* grad_flat, int32_t accumulate, float* d_enc, void* stream);

int mipnerf_mlp_backward_f32(mipnerf_ctx* c, int64_t M, int32_t N, const float* d_raw, const float* enc, const float* viewenc,
                             const float* save, void* workspace, float* grad_flat, int32_t accumulate, void* stream) {
    return mlp_backward_f32_impl(c, M, N, d_raw, enc, viewenc, save, workspace, grad_flat, accumulate, nullptr, stream);
}

// ... plus d_enc [M, xyz_dim] = dL/d(encoding) = delta_0 W_0 + delta_skip W_skip[:, W:] (the input gradient the reference's
// autograd produces when the encoding requires grad, i.e. with stop_resample_grad=False)
int mipnerf_mlp_backward_f32_enc(mipnerf_ctx* c, int64_t M, int32_t N, const float* d_raw, const float* enc, const float* viewenc,
                                 const float* save, void* workspace, float* grad_flat, int32_t accumulate, float* d_enc,
                                 void* stream) {
    if (!d_enc) return fail(MIPNERF_E_INVALID, "mlp_backward_f32_enc: d_enc is null");
    return mlp_backward_f32_impl(c, M, N, d_raw, enc, viewenc, save, workspace, grad_flat, accumulate, d_enc, stream);
}

static int mlp_backward_f32_impl(mipnerf_ctx* c, int64_t M, int32_t N, const float* d_raw, const float* enc, const float* viewenc,
                                 const float* save, void* workspace, float* grad_flat, int32_t accumulate, float* d_enc, void* stream) {
    if (!c || M < 1 || N < 1 || !d_raw || !enc || !viewenc || !save || !workspace || !grad_flat)
        return fail(MIPNERF_E_INVALID, "mlp_backward_f32: bad argument");
    if (!c->params_set) return fail(MIPNERF_E_INVALID, "mlp_backward_f32: mipnerf_set_params has not been called");
    if (M > 0x7fffffff) return fail(MIPNERF_E_INVALID, "mlp_backward_f32: too many samples");
    const PlanDesc& PL = *c->P;
    const int W = PL.net_width, Wc = PL.net_width_cond, E = PL.xyz_dim, D = PL.net_depth, V = PL.view_dim, RGB = PL.num_rgb;
    const bool views = PL.use_viewdirs != 0;
    const int splits = kF32WgradSplits, Mi = (int)M;
    hipStream_t st = S(stream);
    const size_t wmax = W > Wc ? W : Wc;
    float* g0 = reinterpret_cast<float*>(workspace);
    float* g1 = g0 + (size_t)M * wmax;
    float* part = g1 + (size_t)M * wmax;
    const bool acc = accumulate != 0;
    // `save` slot of op L (k_mlp_f32): [M, 32 * hidden tiles] fp32 at offset L * M * W
    auto slot = [&](int L) { return save + (size_t)L * M * W; };
    const unsigned long long* bits0 = reinterpret_cast<const unsigned long long*>(save + (size_t)PL.num_ops * M * W);
    auto slot_bits = [&](int L) { return bits0 + (size_t)L * mip::f32_bits_slot_words(M, W); };
    auto P = [&](int t) { return c->pp.p[t]; };                       // fp32 master parameter t (state_dict order)
    auto G = [&](int t) { return grad_flat + c->tensor_off[t]; }; // its gradient
    const int Dc = PL.net_depth_cond;        // view layers (mip_nerf.py:62-69): the first reads [bottleneck | view encoding], the others Wc -> Wc
    const int tDensW = 2 * D, tDensB = 2 * D + 1, tExW = 2 * D + 2, tExB = 2 * D + 3, tVW = 2 * D + 4, tVB = 2 * D + 5,
              tCW = 2 * D + 4 + 2 * Dc, tCB = 2 * D + 5 + 2 * Dc;
    const float* x8 = slot(D - 1);     // trunk output [M, W]
    // wgrad / bias helpers: dW[out, ldw] (cols [col0, col0+n)) (+)= dY[M, out]^T X[M, n];  db[out] (+)= dY^T 1.
    // Shapes with >= 64 rows / columns go to the 128 x 128-tile kernel (bias gradient fused into its A-tile staging, ReLU mask
    // fused into the dgrad epilogue); thin ones (colour / density heads, the 27 view features) to the 64 x 64 kernel.
    auto wgrad = [&](const float* dY, int64_t ldy, int nout, const float* X, int64_t ldx, int rowdiv, int ncols, float* dW, int64_t ldw,
                     float* db) -> hipError_t {
        if (rowdiv == 1 && mip::gemm_f32_big_ok(nout, ncols, M, dY, ldy))
            return mip::launch_gemm_f32_big(true, nout, ncols, M, dY, ldy, X, ldx, dW, ldw, acc, splits, part, nullptr, nullptr, 0, nullptr, db, st);
        if (nout <= 4)            // colour / density heads: few output ROWS, wide in the input features
            return mip::launch_thin_wgrad(M, ncols, nout, X, ldx, dY, ldy, 1, dW, 1, ldw, db, acc, part, st);
        if (ncols <= 32 && !db)   // the view features: few input COLUMNS (one row of X per ray), wide in the output features
            return mip::launch_thin_wgrad(M, nout, ncols, dY, ldy, X, ldx, rowdiv, dW, ldw, 1, nullptr, acc, part, st);
        hipError_t e = mip::launch_gemm_f32(true, nout, ncols, M, dY, ldy, X, ldx, rowdiv, false, dW, ldw, acc, splits, part, st);
        if (e == hipSuccess && db) e = mip::launch_gemm_f32(true, nout, 1, M, dY, ldy, nullptr, 0, 1, true, db, 1, acc, splits, part, st);
        return e;
    };
    // dX[M, nin] = dY[M, nout] Wt[nout, ldw] (first nin columns) [+ r1_col[m * r1_ld] * r1_row[n]], then (optionally) the ReLU
    // mask of the layer input x
    auto dgrad = [&](const float* dY, int64_t ldy, int nout, const float* Wt, int64_t ldw, int nin, float* dX, int64_t ldxo,
                     int relu_slot, const float* r1_col = nullptr, int64_t r1_ld = 0, const float* r1_row = nullptr) -> hipError_t {
        const float* relu_x = relu_slot >= 0 ? slot(relu_slot) : nullptr;
        if (mip::gemm_f32_big_ok(Mi, nin, nout, dY, ldy))
            return mip::launch_gemm_f32_big(false, Mi, nin, nout, dY, ldy, Wt, ldw, dX, ldxo, false, 1, nullptr, relu_x, r1_col, r1_ld,
                                            r1_row, nullptr, st, relu_slot >= 0 ? slot_bits(relu_slot) : nullptr);
        hipError_t e = mip::launch_gemm_f32(false, Mi, nin, nout, dY, ldy, Wt, ldw, 1, false, dX, ldxo, false, 1, nullptr, st);
        if (e == hipSuccess && r1_col)
            e = mip::launch_gemm_f32(false, Mi, nin, 1, r1_col, r1_ld, r1_row, nin, 1, false, dX, ldxo, true, 1, nullptr, st);
        if (e == hipSuccess && relu_x) e = mip::launch_relu_mask((int64_t)M * nin, relu_x, dX, st);
        return e;
    };
    if (views) {
        const float* hv = slot(D + Dc);    // output of the LAST view layer [M, Wc] (slot D + 1 + i = output of view layer i)
        const float* bott = slot(D);       // bottleneck [M, W]
        // colour layer (mip_nerf.py:110): d_rgb = d_raw[:, 0:3]
        HIP_TRY(wgrad(d_raw, 4, RGB, hv, Wc, 1, Wc, G(tCW), Wc, G(tCB)));
        // g_hv = (d_rgb Wc) * relu'   [M, Wc] in g0
        HIP_TRY(dgrad(d_raw, 4, RGB, P(tCW), Wc, Wc, g0, Wc, D + Dc));
        // view layers Dc-1 .. 1 (Wc -> Wc, mip_nerf.py:62-69 with net_depth_condition > 1): delta ping-pongs g0 -> g1 -> g0;
        // an odd number of them leaves it in g1: copy back so the first view layer below reads g0 as it always did
        {
            float *ga = g0, *gb = g1;
            for (int i = Dc - 1; i >= 1; --i) {
                HIP_TRY(wgrad(ga, Wc, Wc, slot(D + i), Wc, 1, Wc, G(tVW + 2 * i), Wc, G(tVB + 2 * i)));
                HIP_TRY(dgrad(ga, Wc, Wc, P(tVW + 2 * i), Wc, Wc, gb, Wc, D + i));
                float* t = ga; ga = gb; gb = t;
            }
            if (ga != g0) HIP_TRY(hipMemcpyAsync(g0, ga, (size_t)M * Wc * 4, hipMemcpyDeviceToDevice, st));
        }
        // view layer (mip_nerf.py:106-109): input [bottleneck | view encoding of the sample's ray]
        HIP_TRY(wgrad(g0, Wc, Wc, bott, W, 1, W, G(tVW), W + V, G(tVB)));
        HIP_TRY(wgrad(g0, Wc, Wc, viewenc, 32, N, V, G(tVW) + W, W + V, nullptr));
        // g_bott = g_hv Wv[:, :W]   [M, W] in g1
        HIP_TRY(dgrad(g0, Wc, Wc, P(tVW), W + V, W, g1, W, -1));
        // bottleneck (extra_layer, :102) and density head (:100)
        HIP_TRY(wgrad(g1, W, W, x8, W, 1, W, G(tExW), W, G(tExB)));
        HIP_TRY(wgrad(d_raw + 3, 4, 1, x8, W, 1, W, G(tDensW), W, G(tDensB)));
        // g8 = (g_bott We + d_den Wd) * relu'(x8)   in g0: the density head's dgrad is the rank-1 term of the epilogue
        HIP_TRY(dgrad(g1, W, W, P(tExW), W, W, g0, W, D - 1, d_raw + 3, 4, P(tDensW)));
    } else {
        // MLP.forward(x, None) (mip_nerf.py:99-110): colour and density heads both read the trunk output; extra_layer and
        // view_layers are unused parameters (autograd leaves their .grad None; here: zero unless accumulating)
        HIP_TRY(wgrad(d_raw, 4, RGB, x8, W, 1, W, G(tCW), Wc, G(tCB)));
        HIP_TRY(wgrad(d_raw + 3, 4, 1, x8, W, 1, W, G(tDensW), W, G(tDensB)));
        if (!acc) {
            const int unused[4] = {tExW, tExB, tVW, tVB};
            for (int u = 0; u < 4; ++u)
                HIP_TRY(hipMemsetAsync(G(unused[u]), 0, (size_t)PL.param_numel[unused[u]] * 4, st));
        }
        HIP_TRY(dgrad(d_raw, 4, RGB, P(tCW), Wc, W, g0, W, D - 1, d_raw + 3, 4, P(tDensW)));
    }
    bool d_enc_written = false;
    float* g = g0;          // delta of layer i (gradient w.r.t. its pre-activation)
    float* gn = g1;
    for (int i = D - 1; i >= 0; --i) {
        const int ld = PL.param_numel[2 * i] / W;                    // in_features of layer i
        const float* xin = i == 0 ? enc : slot(i - 1);
        const int nin = i == 0 ? E : W;
        HIP_TRY(wgrad(g, W, W, xin, nin, 1, nin, G(2 * i), ld, G(2 * i + 1)));
        if (ld > nin) HIP_TRY(wgrad(g, W, W, enc, E, 1, E, G(2 * i) + W, ld, nullptr));      // skip concat (:96-97)
        if (d_enc && (ld > nin || i == 0)) {
            // the encoding columns of this layer's weight: [W, W + E) of the skip layer, [0, E) of layer 0
            if (!mip::gemm_f32_big_ok(Mi, E, W, g, W)) return fail(MIPNERF_E_UNSUPPORTED, "mlp_backward_f32_enc: encoding narrower than 64");
            HIP_TRY(mip::launch_gemm_f32_big(false, Mi, E, W, g, W, P(2 * i) + (i == 0 ? 0 : W), ld, d_enc, E, d_enc_written, 1, nullptr,
                                             nullptr, nullptr, 0, nullptr, nullptr, st));
            d_enc_written = true;
        }
        if (i > 0) {
            HIP_TRY(dgrad(g, W, W, P(2 * i), ld, W, gn, W, i - 1));
            float* t = g; g = gn; gn = t;
        }
    }
    return MIPNERF_OK;
}

// ---- the whole training step of the hot path in one call ---------------------------------------------------------
// MipNeRFSystem.training_step (nerf_system.py:95-111) = MipNerf.forward(randomized) + loss, followed by what
// loss.backward() does to the 24 MLP parameters -- native kernels only, no autograd graph, graph-capturable.
// the one-call step covers the bounded model's generated shapes and (round 5) the unbounded-scene model's two-kernel bf16 form
static inline bool has_train_step(const mipnerf_ctx* c) {
    return has_bf16_train(c->P) || (c->cfg.unbounded && has_bf16_train_pre(c->P));
}
size_t mipnerf_train_workspace_bytes(const mipnerf_ctx* c, int64_t B) {
    if (!c || B < 1 || !has_train_step(c)) return 0;
    const size_t N = c->cfg.num_samples, M = (size_t)B * N, L = c->cfg.num_levels;
    size_t act, masks, delta, partials;
    if (mipnerf_mlp_train_sizes(c, (int64_t)M, &act, &masks, &delta, &partials)) return 0;
    size_t per_level = align256(B * (N + 1) * 4) + align256(B * N * 4) + align256(B * 3 * 4) + 2 * align256(B * 4) +   // t, w, rgb, dist, acc
                       align256(((M + 255) / 256) * 256 * c->P->xyz_dim * 2) + 2 * align256(M * 16) +              // enc (whole tiles), rgb_sigma, raw
                       align256(masks) + align256(B * 4) + align256(B * N * 4) + align256(B * 3 * 4);   // masks, ray_loss, d_w, g_rgb
    // act and delta: one contiguous run of wave tiles over ALL levels (one weight-gradient launch over both levels)
    if (c->cfg.unbounded) per_level += align256(B * (N + 1) * 4) + 256;      // inverse-depth fence posts; every level's act region starts aligned
    return 256 + L * per_level + align256(B * 32 * 2) + align256(L * align256(act)) + align256(L * delta) + align256(partials) + align256(M * 16) + 256;
}

int mipnerf_train_step(mipnerf_ctx* c, int64_t B, const mipnerf_rays* rays, const float* gt_rgb, const float* t_rand,
                       const float* u_rand, const float* density_randn, uint32_t flags, float coarse_loss_mult, float distloss_mult,
                       int32_t disable_multiscale_loss, void* workspace, size_t workspace_bytes, float* grad_flat,
                       int32_t accumulate, float* out_scalars, const mipnerf_level_out* out, void* stream) {
    if (!c || !rays || !gt_rgb || !workspace || !grad_flat || !out_scalars || B < 1)
        return fail(MIPNERF_E_INVALID, "train_step: bad argument");
    if (!has_train_step(c))
        return fail(MIPNERF_E_UNSUPPORTED, "train_step: no bf16 training kernels for this variant; it trains in fp32 precision");
    if (c->cfg.unbounded && !has_bf16_train_pre(c->P))      // the unbounded branch hands FRAGMENT encodings to the two-kernel form only
        return fail(MIPNERF_E_UNSUPPORTED, "train_step: the unbounded-scene model trains through the two-kernel (pre-GEMM) form");
    if (!rays->origins || !rays->directions || !rays->viewdirs || !rays->radii || !rays->near || !rays->far || !rays->lossmult)
        return fail(MIPNERF_E_INVALID, "train_step: a Rays field is null");
    if (!c->params_set) return fail(MIPNERF_E_INVALID, "train_step: mipnerf_set_params has not been called");
    if ((t_rand == nullptr) != (u_rand == nullptr) && c->cfg.num_levels > 1)
        return fail(MIPNERF_E_INVALID, "train_step: t_rand and u_rand must both be given (randomized) or both null");
    if (workspace_bytes < mipnerf_train_workspace_bytes(c, B)) return fail(MIPNERF_E_WORKSPACE, "train_step: workspace too small");
    const mipnerf_config& cfg = c->cfg;
    const int N = cfg.num_samples, L = cfg.num_levels;
    const size_t M = (size_t)B * N;
    size_t act_b, mask_b, delta_b, part_b;
    int rc = mipnerf_mlp_train_sizes(c, (int64_t)M, &act_b, &mask_b, &delta_b, &part_b);
    if (rc) return rc;
    TrainWs ws;
    ws.base = reinterpret_cast<char*>(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
    const bool unb = cfg.unbounded != 0;       // inverse-depth fence posts, contracted off-axis IPE, the two-kernel MLP form (mipnerf_forward's unbounded branch)
    struct Lvl { float *t, *t_inv, *w, *rgb, *dist, *acc, *rgb_sigma, *raw, *ray_loss, *d_w, *g_rgb; void *enc, *act, *masks; } lv[2];
    for (int l = 0; l < L; ++l) {
        lv[l].t = ws.take<float>(B * (N + 1) * 4); lv[l].w = ws.take<float>(B * N * 4); lv[l].rgb = ws.take<float>(B * 3 * 4);
        lv[l].t_inv = unb ? ws.take<float>(B * (N + 1) * 4) : nullptr;
        lv[l].dist = ws.take<float>(B * 4); lv[l].acc = ws.take<float>(B * 4);
        lv[l].enc = ws.take<char>(unb ? pre_frag_bytes(c, M) : M * c->P->xyz_dim * 2);      // (fragments cover whole 256-sample tiles)
        lv[l].rgb_sigma = ws.take<float>(M * 16); lv[l].raw = ws.take<float>(M * 16);
        lv[l].masks = ws.take<char>(mask_b);
        lv[l].ray_loss = ws.take<float>(B * 4); lv[l].d_w = ws.take<float>(B * N * 4); lv[l].g_rgb = ws.take<float>(B * 3 * 4);
    }
    void* viewenc = ws.take<char>(B * 32 * 2);
    // T-blocks of the activations and of the deltas: level l owns wave tiles [l * n_wt, (l + 1) * n_wt) of one contiguous run,
    // so that ONE weight-gradient launch (+ one reduction) covers every level (padding tiles carry delta = 0)
    // (two-kernel form: a level's region also holds the encoding record and k_pre_gemm's two outputs behind its T-blocks, and every level
    // gets its own weight-gradient launch -- the kernel reads ONE encoding per launch)
    const size_t act_stride = unb ? align256(act_b) : act_b;
    char* act_all = ws.take<char>((size_t)L * act_stride);
    char* delta_all = ws.take<char>((size_t)L * delta_b);
    for (int l = 0; l < L; ++l) lv[l].act = act_all + (size_t)l * act_stride;
    float* partials = ws.take<float>(part_b);
    float* d_raw = ws.take<float>(M * 16);
    const int disparity = (cfg.disparity || (flags & MIPNERF_FLAG_DISPARITY)) ? 1 : 0;
    const int white = (flags & MIPNERF_FLAG_WHITE_BKGD) ? 1 : 0;
    // ---- forward (mip_nerf.py:182-246), activations saved for the backward -------------------------------------------
    // option 4 (fuse_small): pos_enc + coarse fence posts in one launch; per level compositing + distloss (+ the next level's
    // fence posts) in one launch instead of three -- same per-ray device functions, same bits
    const bool fuse_tail = c->fuse_small != 0;        // every N <= MIPNERF_MAX_SAMPLES (round 5: one set of K buckets in all per-ray kernels)
    if (c->fuse_small && !unb) {
        HIP_TRY(mip::launch_ray_prologue(B, cfg.deg_view, rays->viewdirs, viewenc, 32, true, N, rays->near, rays->far, t_rand, disparity,
                                         lv[0].t, S(stream)));
    } else if ((rc = mipnerf_pos_enc(B, cfg.deg_view, rays->viewdirs, viewenc, 32, MIPNERF_PREC_BF16, stream))) {
        return rc;
    }
    for (int l = 0; l < L; ++l) {
        const float* dnoise = density_randn ? density_randn + (size_t)l * M : nullptr;      // this level's draws (mip_nerf.py:232-233)
        if (unb) {
            // the fine level inverts the coarse weights' PDF over the INVERSE-DEPTH fence posts, then t = 1 / t_inv (as mipnerf_forward)
            if (l == 0) {
                HIP_TRY(mip::launch_sample_along_rays_360(B, N, rays->near, rays->far, t_rand, lv[0].t_inv, lv[0].t, S(stream)));
            } else {
                if (!fuse_tail && (rc = mipnerf_resample_along_rays(B, N, lv[l - 1].t_inv, lv[l - 1].w, u_rand, cfg.resample_padding,
                                                                    lv[l].t_inv, stream))) return rc;
                HIP_TRY(mip::launch_reciprocal((int64_t)B * (N + 1), lv[l].t_inv, lv[l].t, S(stream)));
            }
        } else if (l == 0) {
            if (!c->fuse_small && (rc = mipnerf_sample_along_rays(B, N, rays->near, rays->far, t_rand, disparity, lv[0].t, stream))) return rc;
        } else if (!fuse_tail) {
            if ((rc = mipnerf_resample_along_rays(B, N, lv[l - 1].t, lv[l - 1].w, u_rand, cfg.resample_padding, lv[l].t, stream))) return rc;
        }
        if (unb) {      // the 672-wide encoding as bf16 B-operand fragments: k_pre_gemm reads them, and so does this level's weight-gradient launch
            HIP_TRY(mip::launch_cast_ipe_360(B, N, cfg.min_deg_point, cfg.max_deg_point, 1, lv[l].t, rays->origins, rays->directions, rays->radii,
                                             lv[l].enc, true, nullptr, nullptr, S(stream), true));
            if ((rc = mlp_forward_train_noise(c, (int64_t)M, N, lv[l].enc, viewenc, lv[l].rgb_sigma, lv[l].raw, lv[l].act, lv[l].masks, dnoise,
                                              stream, true))) return rc;
        } else if (c->fused_ipe && max_deg_span_is_16(cfg)) {      // encoding computed inside the forward-with-save kernel
            const mip::RayInputs ri = {lv[l].t, rays->origins, rays->directions, rays->radii, cfg.min_deg_point,
                                       cfg.disable_integration};
            HIP_TRY(launch_trainfwd_variant(c, nullptr, viewenc, lv[l].rgb_sigma, lv[l].raw, lv[l].act, lv[l].masks, (int64_t)M, N, &ri,
                                            dnoise, S(stream)));
        } else {
            if ((rc = mipnerf_cast_ipe(B, N, cfg.min_deg_point, cfg.max_deg_point, cfg.disable_integration, lv[l].t, rays->origins,
                                       rays->directions, rays->radii, lv[l].enc, MIPNERF_PREC_BF16, stream))) return rc;
            if ((rc = mlp_forward_train_noise(c, (int64_t)M, N, lv[l].enc, viewenc, lv[l].rgb_sigma, lv[l].raw, lv[l].act,
                                              lv[l].masks, dnoise, stream))) return rc;
        }
        // distloss (mip.py:8-20) forward AND backward in one pass: d loss / d ray_loss is the constant k_l * dm / B
        const float k = (L > 1 && l == 0) ? coarse_loss_mult : 1.0f;
        if (fuse_tail) {
            HIP_TRY(mip::launch_composite_train(B, N, lv[l].rgb_sigma, lv[l].t, rays->directions, white, lv[l].rgb, lv[l].dist, lv[l].acc,
                                                lv[l].w, lv[l].ray_loss, k * distloss_mult / (float)B, lv[l].d_w, u_rand,
                                                cfg.resample_padding, l + 1 < L ? (unb ? lv[l + 1].t_inv : lv[l + 1].t) : nullptr, S(stream),
                                                unb ? lv[l].t_inv : nullptr));
            continue;
        }
        if ((rc = mipnerf_volumetric_rendering(B, N, lv[l].rgb_sigma, lv[l].t, rays->directions, white, lv[l].rgb, lv[l].dist,
                                               lv[l].acc, lv[l].w, stream))) return rc;
        HIP_TRY(mip::launch_distloss(B, N, lv[l].w, lv[l].t, lv[l].ray_loss, nullptr, k * distloss_mult / (float)B, lv[l].d_w,
                                     S(stream)));
    }
    // ---- loss (nerf_system.py:99-111) and d loss / d comp_rgb ------------------------------------------------------------
    HIP_TRY(mip::launch_loss_fused(B, L, lv[0].rgb, L > 1 ? lv[1].rgb : nullptr, gt_rgb, disable_multiscale_loss ? nullptr : rays->lossmult,
                                   lv[0].ray_loss, L > 1 ? lv[1].ray_loss : nullptr, coarse_loss_mult, distloss_mult, lv[0].g_rgb,
                                   L > 1 ? lv[1].g_rgb : lv[0].g_rgb, out_scalars, S(stream)));
    // ---- backward: compositing + activations, then the MLP, level by level (resampling carries no gradient,
    //      mip_nerf.py:187-196 stop_resample_grad) ----------------------------------------------------------------------------
    for (int l = L - 1; l >= 0; --l) {
        if ((rc = mipnerf_volumetric_rendering_bwd(B, N, lv[l].rgb_sigma, lv[l].t, rays->directions, white, lv[l].g_rgb, nullptr,
                                                   nullptr, lv[l].d_w, cfg.rgb_padding, d_raw, stream))) return rc;
        if ((rc = mipnerf_mlp_dgrad(c, (int64_t)M, d_raw, lv[l].masks, delta_all + (size_t)l * delta_b, stream))) return rc;
        if (unb && (rc = wgrad_tiles(c, (int64_t)(((M + 255) / 256) * 8), lv[l].act, delta_all + (size_t)l * delta_b, partials, grad_flat,
                                     (accumulate || l < L - 1) ? 1 : 0, stream))) return rc;
    }
    // one weight-gradient pass over the wave tiles of all levels (the sum over levels is part of the sample contraction)
    if (!unb && (rc = wgrad_tiles(c, (int64_t)L * (int64_t)(((M + 255) / 256) * 8), act_all, delta_all, partials, grad_flat, accumulate ? 1 : 0,
                                  stream))) return rc;
    if (out)      // optional copies of what MipNerf.forward returns (async device-to-device)
        for (int l = 0; l < L; ++l) {
            const mipnerf_level_out& o = out[l];
            if (o.comp_rgb) HIP_TRY(hipMemcpyAsync(o.comp_rgb, lv[l].rgb, B * 3 * 4, hipMemcpyDeviceToDevice, S(stream)));
            if (o.distance) HIP_TRY(hipMemcpyAsync(o.distance, lv[l].dist, B * 4, hipMemcpyDeviceToDevice, S(stream)));
            if (o.acc) HIP_TRY(hipMemcpyAsync(o.acc, lv[l].acc, B * 4, hipMemcpyDeviceToDevice, S(stream)));
            if (o.weights) HIP_TRY(hipMemcpyAsync(o.weights, lv[l].w, B * N * 4, hipMemcpyDeviceToDevice, S(stream)));
            if (o.t_samples) HIP_TRY(hipMemcpyAsync(o.t_samples, lv[l].t, B * (N + 1) * 4, hipMemcpyDeviceToDevice, S(stream)));
        }
    return MIPNERF_OK;
}

// ---- the level loop ---------------------------------------------------------------------------------
// encoding region of one level: [M, xyz_dim] fp32 (or bf16) -- or, two-kernel bf16 form, the bf16 fragments of whole 256-sample tiles followed by
// k_pre_gemm's two outputs (1,344 + 1,536 B per sample: 7 % more than the fp32 encodings they replace, so one region serves either precision)
static size_t enc_region_bytes(const mipnerf_ctx* c, size_t M) {
    const size_t rowmajor = M * c->P->xyz_dim * 4;
    const size_t pre = has_bf16_pre(c->P) ? align256(pre_frag_bytes(c, M)) + align256(pre_x_bytes((int64_t)M)) + align256(pre_acc_bytes((int64_t)M)) : 0;
    return rowmajor > pre ? rowmajor : pre;
}
size_t mipnerf_workspace_bytes(const mipnerf_ctx* c, int64_t B) {
    if (!c || B < 1) return 0;
    const size_t M = (size_t)B * (size_t)c->cfg.num_samples;
    return align256(enc_region_bytes(c, M)) + align256((size_t)B * 32 * 4) + align256(M * 16) + 256 +
           (c->cfg.unbounded ? 2 * align256((size_t)B * (c->cfg.num_samples + 1) * 4) : 0);       // inverse-depth fence posts of two levels
}

// the proposal level of mipnerf_forward_proposal: level 0 takes its density from this lattice instead of the encoding + MLP launch
struct ProposalLevel {
    mip::LatticeBox box;
    const float* lattice;
};

// the level loop of mipnerf_forward (prop == nullptr: its launches exactly) and of mipnerf_forward_proposal
static int forward_levels(mipnerf_ctx* c, int64_t B, const mipnerf_rays* rays, const float* t_rand, const float* u_rand,
                          const float* density_randn, uint32_t flags, int precision, void* workspace, size_t workspace_bytes,
                          const mipnerf_level_out* out, void* stream, const ProposalLevel* prop) {
    if (!c || !rays || !out || !workspace || B < 1) return fail(MIPNERF_E_INVALID, "forward: bad argument");
    if (!rays->origins || !rays->directions || !rays->viewdirs || !rays->radii || !rays->near || !rays->far)
        return fail(MIPNERF_E_INVALID, "forward: a Rays field is null");
    if (!c->params_set) return fail(MIPNERF_E_INVALID, "forward: mipnerf_set_params has not been called");
    if ((t_rand == nullptr) != (u_rand == nullptr) && c->cfg.num_levels > 1)
        return fail(MIPNERF_E_INVALID, "forward: t_rand and u_rand must both be given (randomized) or both null");
    if (workspace_bytes < mipnerf_workspace_bytes(c, B)) return fail(MIPNERF_E_WORKSPACE, "forward: workspace too small");
    if (precision != MIPNERF_PREC_BF16 && precision != MIPNERF_PREC_FP32)
        return fail(MIPNERF_E_INVALID, "unknown precision %d", precision);
    if (precision == MIPNERF_PREC_BF16 && !has_bf16(c->P))
        return fail(MIPNERF_E_UNSUPPORTED, "forward: this architecture variant has fp32 kernels only (csrc/gen_mlp_bf16.py VARIANTS)");
    const mipnerf_config& cfg = c->cfg;
    const int N = cfg.num_samples;
    const size_t M = (size_t)B * N;
    char* ws = reinterpret_cast<char*>(((uintptr_t)workspace + 255) & ~(uintptr_t)255);
    void* enc = ws;
    const size_t enc_b = align256(enc_region_bytes(c, M));
    void* viewenc = ws + enc_b;
    float* rgb_sigma = reinterpret_cast<float*>(ws + enc_b + align256((size_t)B * 32 * 4));
    float* t_inv[2] = {nullptr, nullptr};
    if (cfg.unbounded) {
        char* q = reinterpret_cast<char*>(rgb_sigma) + align256(M * 16);
        t_inv[0] = reinterpret_cast<float*>(q);
        t_inv[1] = reinterpret_cast<float*>(q + align256((size_t)B * (N + 1) * 4));
    }
    // bf16 on a variant whose encoding is too wide for k_mlp_bf16 (the unbounded-scene model): k_pre_gemm + trunk kernel (gen_pre_gemm.py);
    // its fragments and the two buffers between the kernels share the encoding region
    const bool pre_form = precision == MIPNERF_PREC_BF16 && has_bf16_pre(c->P);
    char* pre_x = pre_form ? ws + align256(pre_frag_bytes(c, M)) : nullptr;
    char* pre_acc = pre_form ? pre_x + align256(pre_x_bytes((int64_t)M)) : nullptr;
    const int disparity = (cfg.disparity || (flags & MIPNERF_FLAG_DISPARITY)) ? 1 : 0;
    const int white = (flags & MIPNERF_FLAG_WHITE_BKGD) ? 1 : 0;
    int rc;
    // pos_enc(viewdirs) is level-independent: computed once (the reference recomputes it, mip_nerf.py:220-226) -- in the same launch
    // as the coarse level's fence posts (option 4 = 0: one launch per stage, the per-stage kernels; both routes give the same bits)
    bool have_t0 = false;
    if (c->fuse_small && !cfg.unbounded) {
        if (!out[0].t_samples) return fail(MIPNERF_E_INVALID, "forward: output pointer of level 0 is null");
        HIP_TRY(mip::launch_ray_prologue(B, cfg.deg_view, rays->viewdirs, viewenc, 32, precision == MIPNERF_PREC_BF16, N, rays->near, rays->far,
                                         t_rand, disparity, out[0].t_samples, S(stream)));
        have_t0 = true;
    } else if ((rc = mipnerf_pos_enc(B, cfg.deg_view, rays->viewdirs, viewenc, 32, precision, stream))) {
        return rc;
    }
    bool have_resampled = false;      // the previous level's launch already drew this level's fence posts (k_composite_resample)
    for (int lvl = 0; lvl < cfg.num_levels; ++lvl) {
        const float* dnoise = density_randn ? density_randn + (size_t)lvl * M : nullptr;    // this level's draws (mip_nerf.py:232-233)
        const mipnerf_level_out& o = out[lvl];
        if (!o.comp_rgb || !o.distance || !o.acc || !o.weights || !o.t_samples)
            return fail(MIPNERF_E_INVALID, "forward: output pointer of level %d is null", lvl);
        const bool fused = !cfg.unbounded && precision == MIPNERF_PREC_BF16 && c->fused_ipe && c->mlp_dma;
        if (cfg.unbounded) {
            // SURVEY 8(f)-4 (what mip.py:106-124, 292-319, 424-447 aim at): fence posts uniform in inverse depth; the fine level
            // inverts the coarse weights' piecewise-constant PDF over the INVERSE-DEPTH fence posts (the same blur pool + padding
            // as mip.py:252-257; the inversion only interpolates between bins, so it is the s-space resampling of the paper up
            // to the affine map s <-> 1/t), then t = 1 / t_inv; contracted full-covariance Gaussians -> off-axis IPE
            if (lvl == 0) {
                HIP_TRY(mip::launch_sample_along_rays_360(B, N, rays->near, rays->far, t_rand, t_inv[0], o.t_samples, S(stream)));
            } else {
                if (!have_resampled &&
                    (rc = mipnerf_resample_along_rays(B, N, t_inv[lvl - 1], out[lvl - 1].weights, u_rand, cfg.resample_padding,
                                                      t_inv[lvl], stream))) return rc;
                HIP_TRY(mip::launch_reciprocal((int64_t)B * (N + 1), t_inv[lvl], o.t_samples, S(stream)));
            }
            // dtype of the encoding = the precision (fragments when the two-kernel form will read them); an unbounded variant with bf16
            // kernels of some OTHER form must not be handed fp32 rows here
            if (precision == MIPNERF_PREC_BF16 && !pre_form)
                return fail(MIPNERF_E_UNSUPPORTED, "forward: bf16 inference of an unbounded variant needs the two-kernel (pre-GEMM) form");
            HIP_TRY(mip::launch_cast_ipe_360(B, N, cfg.min_deg_point, cfg.max_deg_point, 1, o.t_samples, rays->origins, rays->directions,
                                             rays->radii, enc, precision == MIPNERF_PREC_BF16, nullptr, nullptr, S(stream), pre_form));
        } else if (lvl == 0) {
            if (!have_t0 && (rc = mipnerf_sample_along_rays(B, N, rays->near, rays->far, t_rand, disparity, o.t_samples, stream))) return rc;
        } else if (!have_resampled) {
            if ((rc = mipnerf_resample_along_rays(B, N, out[lvl - 1].t_samples, out[lvl - 1].weights, u_rand,
                                                  cfg.resample_padding, o.t_samples, stream))) return rc;
        }
        have_resampled = false;
        if (prop && lvl == 0) {
            // proposal level: no encoding and no MLP launch; k_lattice_density writes (0, 0, 0, sigma) where the MLP kernel would have
            HIP_TRY(mip::launch_lattice_density(prop->box, prop->lattice, B, N, o.t_samples, rays->origins, rays->directions, rays->radii,
                                                rgb_sigma, S(stream)));
        } else {
            if (!fused && !cfg.unbounded &&
                (rc = mipnerf_cast_ipe(B, N, cfg.min_deg_point, cfg.max_deg_point, cfg.disable_integration, o.t_samples,
                                       rays->origins, rays->directions, rays->radii, enc, precision, stream))) return rc;
            hipEvent_t e0 = nullptr, e1 = nullptr;
            if (c->time_mlp == 1) {
                if (c->ev_used + 2 > c->ev.size()) {
                    for (int i = 0; i < 64; ++i) { hipEvent_t e; HIP_TRY(hipEventCreate(&e)); c->ev.push_back(e); }
                }
                e0 = c->ev[c->ev_used]; e1 = c->ev[c->ev_used + 1]; c->ev_used += 2;
                HIP_TRY(hipEventRecord(e0, S(stream)));
            }
            if (fused) {
                if (max_deg_span_is_16(cfg) == false)
                    return fail(MIPNERF_E_UNSUPPORTED, "fused IPE is generated for max_deg-min_deg == 16");
                const mip::RayInputs ri = {o.t_samples, rays->origins, rays->directions, rays->radii, cfg.min_deg_point,
                                           cfg.disable_integration};
                HIP_TRY(launch_bf16_variant(c, nullptr, viewenc, rgb_sigma, nullptr, (int64_t)M, N, true, &ri, dnoise, S(stream)));
            } else if (pre_form) {
                HIP_TRY(launch_bf16_pre(c, enc, 1, viewenc, rgb_sigma, nullptr, (int64_t)M, N, pre_x, pre_acc, dnoise, S(stream)));
            } else if ((rc = mlp_forward_noise(c, (int64_t)M, N, enc, viewenc, precision, rgb_sigma, nullptr, dnoise, stream))) {
                return rc;
            }
            if (c->time_mlp == 1) HIP_TRY(hipEventRecord(e1, S(stream)));
        }
        if (c->fuse_small && lvl + 1 < cfg.num_levels) {
            // compositing of this level + the next level's fence posts in one launch (weights go registers -> LDS, not through HBM)
            const mipnerf_level_out& nx = out[lvl + 1];
            if (!nx.t_samples) return fail(MIPNERF_E_INVALID, "forward: output pointer of level %d is null", lvl + 1);
            HIP_TRY(mip::launch_composite_resample(B, N, rgb_sigma, o.t_samples, rays->directions, white, o.comp_rgb, o.distance, o.acc,
                                                   o.weights, cfg.unbounded ? t_inv[lvl] : o.t_samples, u_rand, cfg.resample_padding,
                                                   cfg.unbounded ? t_inv[lvl + 1] : nx.t_samples, S(stream)));
            have_resampled = true;
            continue;
        }
        if ((rc = mipnerf_volumetric_rendering(B, N, rgb_sigma, o.t_samples, rays->directions, white, o.comp_rgb,
                                               o.distance, o.acc, o.weights, stream))) return rc;
    }
    return MIPNERF_OK;
}

int mipnerf_forward(mipnerf_ctx* c, int64_t B, const mipnerf_rays* rays, const float* t_rand, const float* u_rand,
                    const float* density_randn, uint32_t flags, int precision, void* workspace, size_t workspace_bytes,
                    const mipnerf_level_out* out, void* stream) {
    return forward_levels(c, B, rays, t_rand, u_rand, density_randn, flags, precision, workspace, workspace_bytes, out, stream, nullptr);
}

// ---- the density lattice as the proposal level (kernels_proposal.hip, lattice_sample.hpp) ------------------------------------------
static int proposal_box(const char* who, const int32_t* dims, const float* lo, const float* hi, const float* lattice, mip::LatticeBox* box) {
    if (!lattice) return fail(MIPNERF_E_INVALID, "%s: null argument (lattice)", who);
    if (int rc = lattice_check(who, dims, lo, hi)) return rc;
    box->nx = dims[0]; box->ny = dims[1]; box->nz = dims[2];
    for (int a = 0; a < 3; ++a) {
        if (!(hi[a] > lo[a])) return fail(MIPNERF_E_INVALID, "%s: the box needs hi > lo on every axis", who);
        box->lo[a] = lo[a];
        box->inv_h[a] = (float)(dims[a] - 1) / (hi[a] - lo[a]);
        if (!std::isfinite(box->inv_h[a])) return fail(MIPNERF_E_INVALID, "%s: the box is too thin: (n - 1) / (hi - lo) is not finite", who);
    }
    return MIPNERF_OK;
}

int mipnerf_lattice_density(const int32_t* dims, const float* lo, const float* hi, const float* lattice, int64_t B, int32_t N,
                            const float* t, const float* origins, const float* dirs, const float* radii, float* rgb_sigma, void* stream) {
    mip::LatticeBox box;
    if (int rc = proposal_box("lattice_density", dims, lo, hi, lattice, &box)) return rc;
    if (N < 1 || N > MIPNERF_MAX_SAMPLES) return fail(MIPNERF_E_INVALID, "lattice_density: num_samples must be in [1, %d] (got %d)", MIPNERF_MAX_SAMPLES, N);
    if (B < 0 || B >= (1LL << 31)) return fail(MIPNERF_E_INVALID, "lattice_density: bad ray count %lld", (long long)B);
    if (B == 0) return MIPNERF_OK;
    if (!t || !origins || !dirs || !radii || !rgb_sigma) return fail(MIPNERF_E_INVALID, "lattice_density: null argument");
    HIP_TRY(mip::launch_lattice_density(box, lattice, B, N, t, origins, dirs, radii, rgb_sigma, S(stream)));
    return MIPNERF_OK;
}

int mipnerf_forward_proposal(mipnerf_ctx* c, int64_t B, const mipnerf_rays* rays, const int32_t* dims, const float* lo, const float* hi,
                             const float* lattice, const float* t_rand, const float* u_rand, uint32_t flags, int precision,
                             void* workspace, size_t workspace_bytes, const mipnerf_level_out* out, void* stream) {
    ProposalLevel prop;
    if (int rc = proposal_box("forward_proposal", dims, lo, hi, lattice, &prop.box)) return rc;
    prop.lattice = lattice;
    if (!c) return fail(MIPNERF_E_INVALID, "forward_proposal: null argument (ctx)");
    if (c->cfg.unbounded)
        return fail(MIPNERF_E_UNSUPPORTED, "forward_proposal: the unbounded-scene model lives in a contracted space; its proposal pyramid is read by mipnerf_lattice_density_360 (mipnerf_proposal_360.h) and the level loop around it is composed of the stage entry points, not by this call");
    if (c->cfg.num_levels != 2)
        return fail(MIPNERF_E_UNSUPPORTED, "forward_proposal: the lattice replaces the coarse level of a two-level model (num_levels = %d)", c->cfg.num_levels);
    if (B >= (1LL << 31)) return fail(MIPNERF_E_INVALID, "forward_proposal: bad ray count %lld", (long long)B);
    return forward_levels(c, B, rays, t_rand, u_rand, nullptr, flags, precision, workspace, workspace_bytes, out, stream, &prop);
}

// ---- instrumentation -----------------------------------------------------------------------------------
int mipnerf_time_mlp(mipnerf_ctx* c, int64_t M, int32_t N, const void* enc, const void* viewenc, int precision,
                     float* rgb_sigma, int iters, float* ms, void* stream) {
    if (!ms || iters < 1) return fail(MIPNERF_E_INVALID, "time_mlp: bad argument");
    hipEvent_t e0, e1;
    HIP_TRY(hipEventCreate(&e0));
    HIP_TRY(hipEventCreate(&e1));
    int rc = mipnerf_mlp_forward(c, M, N, enc, viewenc, precision, rgb_sigma, nullptr, stream);   // warm
    if (rc) return rc;
    HIP_TRY(hipEventRecord(e0, S(stream)));
    for (int i = 0; i < iters; ++i)
        if ((rc = mipnerf_mlp_forward(c, M, N, enc, viewenc, precision, rgb_sigma, nullptr, stream))) return rc;
    HIP_TRY(hipEventRecord(e1, S(stream)));
    HIP_TRY(hipEventSynchronize(e1));
    float t = 0;
    HIP_TRY(hipEventElapsedTime(&t, e0, e1));
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    *ms = t / iters;
    return MIPNERF_OK;
}

int mipnerf_mlp_launch_stats(mipnerf_ctx* c, double* total_ms, int64_t* launches) {
    if (!c || !total_ms || !launches) return fail(MIPNERF_E_INVALID, "mlp_launch_stats: null argument");
    double tot = 0;
    for (size_t i = 0; i + 1 < c->ev_used; i += 2) {
        HIP_TRY(hipEventSynchronize(c->ev[i + 1]));
        float t = 0;
        HIP_TRY(hipEventElapsedTime(&t, c->ev[i], c->ev[i + 1]));
        tot += t;
    }
    *total_ms = tot;
    *launches = (int64_t)(c->ev_used / 2);
    c->ev_used = 0;
    return MIPNERF_OK;
}

int mipnerf_selftest(void* stream) {
    char msg[256];
    const int bad = mip::run_selftest(S(stream), msg, sizeof msg);
    g_err = msg;
    if (bad < 0) return MIPNERF_E_HIP;
    return bad == 0 ? MIPNERF_OK : (0x100 | bad);
}

// Host-only debug export of the plan tables (flat parameter indices), used by the CPU tests to prove that what the library expands
// from its embedded tables equals mlp_plan.py.  which: 0 bf16 pack, 1 bias, 2 fp32 pack (Plan.build), 6 / 7 the bf16 pack / bias table of
// the forward kernels (Plan.build(fold_view=True)).  Returns element count.
int64_t mipnerf_debug_table_variant(int variant, int which, int32_t* out_host, int64_t cap) {
    if (variant < 0 || variant >= mip::plan::kNumVariants || which < 0 || which > 7) return -1;
    const PlanDesc& P = mip::plan::kPlans[variant];
    std::vector<int32_t> v;
    if (which >= 3 && which <= 5) {     // training tables of the variant (3 dgrad pack, 4 wgrad partial -> parameter, 5 jobs)
        TrainTables tt;
        if (!train_tables(tt, variant)) return -1;
        const int32_t* src = which == 3 ? tt.bpack : (which == 4 ? tt.otab : tt.jobs);
        v.assign(src, src + (which == 3 ? (size_t)tt.n_bchunks * 512 : (which == 4 ? (size_t)tt.njobs * tt.job_floats : (size_t)tt.njobs * 20)));
    } else {
        PlanTables T;
        if (!plan_tables(T, P)) return -1;
        const std::vector<int> toff = tensor_offsets(P);
        if (which == 0) v = expand(T.pack, P.num_chunks, P.num_chunks, &toff);      // includes the zero padding chunks at the end of the stream
        else if (which == 6) v = expand(T.fwd_pack, P.fwd_num_chunks, P.fwd_num_chunks, &toff);
        else if (which == 2) v = expand(T.pack_f32, T.n_f32_chunks, P.num_chunks, &toff);
        else if (which == 1) v.assign(T.bias, T.bias + (size_t)P.num_tiles * 32);
        else v.assign(T.fwd_bias, T.fwd_bias + (size_t)P.fwd_num_tiles * 32);
    }
    if (out_host && cap >= (int64_t)v.size()) memcpy(out_host, v.data(), v.size() * 4);
    return (int64_t)v.size();
}

int64_t mipnerf_debug_table(int which, int32_t* out_host, int64_t cap) { return mipnerf_debug_table_variant(0, which, out_host, cap); }

// Host-only: fp32 layer descriptors (x_in0, kb0, x_in1, kb1, x_out, ntiles, first_tile, relu, kind, chunk0, stage_view, ldx) x nlayers
int64_t mipnerf_debug_f32net(int32_t* out_host, int64_t cap) {
    PlanTables T;
    if (!plan_tables(T, mip::plan::kPlans[0])) return -1;
    const mip::F32Net net = f32net(mip::plan::kPlans[0], T.layers);
    const int n = net.nlayers;
    if (out_host && cap >= (int64_t)n * 12)
        for (int i = 0; i < n; ++i) {
            const mip::F32Layer& L = net.layers[i];
            const int32_t row[12] = {L.x_in0, L.kb0, L.x_in1, L.kb1, L.x_out, L.ntiles, L.first_tile, L.relu, L.kind, L.chunk0,
                                     L.stage_view, net.ldx};
            memcpy(out_host + i * 12, row, sizeof row);
        }
    return n;
}

}  // extern "C"
