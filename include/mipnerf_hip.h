/* mipnerf_hip.h -- C ABI of the MI355X-native Mip-NeRF volume-rendering hot path.
 *
 * Shared library: mipnerf_pl_amd/csrc/libmipnerf_hip.so (hipcc --offload-arch=gfx950).
 * The reference (hjxwhy/mipnerf_pl) has no FFI of its own -- its boundary is the Python
 * class contract `MipNerf.forward(rays, randomized, white_bkgd)` (models/mip_nerf.py:172-248)
 * built from the free functions of models/mip.py.  Each entry point below replaces one of
 * those functions (cited per prototype); `mipnerf_forward` replaces the whole level loop.
 * INTEGRATION.md shows the ctypes binding a reference maintainer would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (hipMalloc / torch.cuda tensor .data_ptr()) unless
 *     the parameter name ends in `_host`; float32, row-major, contiguous;
 *   - `stream` is a hipStream_t passed as void* (0 = default stream); all work is
 *     enqueued asynchronously on it, no entry point synchronises or allocates, except
 *     mipnerf_create / mipnerf_destroy (hipMalloc / hipFree of the packed-weight buffers);
 *   - return value: 0 = MIPNERF_OK, otherwise an error code; mipnerf_last_error() returns
 *     a thread-local message.  The Python host turns codes into RuntimeError /
 *     NotImplementedError (the reference raises NotImplementedError for unsupported
 *     enum values: mip_nerf.py:50,70,165,170, mip.py:98);
 *   - inputs are never written; outputs never alias inputs (mip.py:184 mutates its
 *     argument in place -- this library does not).
 */
#ifndef MIPNERF_HIP_H
#define MIPNERF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MIPNERF_ABI_VERSION 6

enum {
    MIPNERF_OK = 0,
    MIPNERF_E_INVALID = 1,      /* bad argument (null pointer, size <= 0, N too large ...) */
    MIPNERF_E_UNSUPPORTED = 2,  /* NotImplementedError in the reference, or an MLP shape the
                                   compiled kernels do not cover */
    MIPNERF_E_HIP = 3,          /* a HIP runtime call failed (message has hipGetErrorString) */
    MIPNERF_E_WORKSPACE = 4     /* workspace too small */
};

/* compute precision of the MLP (the rest of the path is always fp32) */
enum {
    MIPNERF_PREC_FP32 = 0, /* v_mfma_f32_32x32x2_f32, exact fp32 products (parity mode)   */
    MIPNERF_PREC_BF16 = 1, /* v_mfma_f32_32x32x16_bf16, bf16 operands / fp32 accumulate    */
    MIPNERF_OUT_BF16_FRAGMENTS = 2 /* out_dtype of mipnerf_cast_ipe_360 only: bf16 in the MFMA B-operand fragment layout  */
                                   /* [wave tile of 32 samples][k-step][64 lanes][8], whole 256-sample tiles (the buffer    */
                                   /* holds ceil(M / 256) * 256 rows) -- what the two-kernel MLP form reads fastest         */
};

/* flags */
enum {
    MIPNERF_FLAG_WHITE_BKGD = 1, /* volumetric_rendering(white_bkgd=True), mip.py:399-400  */
    MIPNERF_FLAG_DISPARITY = 2   /* sample linearly in disparity, mip.py:149-150           */
};

/* Mirrors the keyword arguments of MipNerf.__init__ (models/mip_nerf.py:117-141) that
 * change the arithmetic.  ray_shape is always 'cone' ('cylinder' raises in the reference). */
typedef struct mipnerf_config {
    int32_t num_samples;         /* nerf.num_samples, N (<= MIPNERF_MAX_SAMPLES)           */
    int32_t num_levels;          /* nerf.num_levels (1 or 2)                                */
    int32_t min_deg_point;       /* 0                                                       */
    int32_t max_deg_point;       /* 16                                                      */
    int32_t deg_view;            /* 4                                                       */
    int32_t use_viewdirs;        /* 1                                                       */
    int32_t disparity;           /* 0                                                       */
    int32_t disable_integration; /* 0 ; 1 => covariances zeroed before the IPE (PE)         */
    int32_t net_depth;           /* 8                                                       */
    int32_t net_width;           /* 256                                                     */
    int32_t net_depth_condition; /* 1                                                       */
    int32_t net_width_condition; /* 128                                                     */
    int32_t skip_index;          /* 4                                                       */
    int32_t num_rgb_channels;    /* 3                                                       */
    int32_t num_density_channels;/* 1                                                       */
    float resample_padding;      /* 0.01                                                    */
    float density_bias;          /* -1                                                      */
    float rgb_padding;           /* 0.001                                                   */
    float density_noise;         /* 0 ; std-dev of the noise added to raw density when a    */
                                 /* density_randn tensor is given (mip_nerf.py:232-233)     */
    int32_t unbounded;           /* 0 ; 1 => the unbounded-scene (mip-NeRF 360) path: fence posts uniform in inverse depth,  */
                                 /* contracted full-covariance Gaussians, off-axis IPE with 42 features per degree (what     */
                                 /* models/mip.py:106-124, 292-319, 424-447 aim at).  fp32 or bf16 (the 672-wide encoding    */
                                 /* runs as k_pre_gemm + a trunk kernel, csrc/gen_pre_gemm.py): mipnerf_forward,             */
                                 /* mipnerf_mlp_forward and the per-stage training entry points (mipnerf_mlp_forward_train / */
                                 /* _dgrad / _backward) and, in bf16, mipnerf_train_step                                     */
} mipnerf_config;

#define MIPNERF_MAX_SAMPLES 1024
#define MIPNERF_NUM_PARAM_TENSORS 24 /* 2 x (8 trunk + density + extra + 1 view + color)   */

/* The 7 fields of the reference `Rays` namedtuple (datasets/datasets.py:13-16), SoA. */
typedef struct mipnerf_rays {
    const float* origins;    /* [B,3] */
    const float* directions; /* [B,3] un-normalised */
    const float* viewdirs;   /* [B,3] unit          */
    const float* radii;      /* [B,1] */
    const float* lossmult;   /* [B,1] (unused by forward) */
    const float* near;       /* [B,1] */
    const float* far;        /* [B,1] */
} mipnerf_rays;

/* One level of the list returned by MipNerf.forward (mip_nerf.py:246). */
typedef struct mipnerf_level_out {
    float* comp_rgb;  /* [B,3]   */
    float* distance;  /* [B]     */
    float* acc;       /* [B]     */
    float* weights;   /* [B,N]   */
    float* t_samples; /* [B,N+1] */
} mipnerf_level_out;

/* Output of mipnerf_generate_rays: the same 7 fields, writable. */
typedef struct mipnerf_rays_out {
    float* origins; float* directions; float* viewdirs; float* radii; float* lossmult; float* near; float* far;
} mipnerf_rays_out;

/* One camera for mipnerf_generate_rays: 32 floats =
 * c2w[3][4] | pix2cam[3][3] | width, height, near, far, lossmult, mode, focal | distortion[4]   (floats 28..31; 0 for modes 0 and 1).
 * mode 0: Blender pinhole formula with `focal` (datasets.py:226-228); mode 1: pix2cam matrix (datasets.py:125-131).
 * Modes 2 and 3 are distorted COLMAP cameras (csrc/camera_models.hpp).  c = pix2cam @ (x + .5, y + .5, 1) as in mode 1, and pix2cam
 * must be K^-1 with rows 1 and 2 negated (last row (0, 0, -1)), so that (xd, yd) = (c0, -c1) is the normalised DISTORTED image point;
 * it is undistorted by 8 Newton steps started there (a fixed count, no data-dependent exit; a step with |determinant| < 1e-9 is a zero
 * step; a non-finite result falls back to (xd, yd)).
 * mode 2: radial-tangential, distortion = k1, k2, p1, p2 (COLMAP SIMPLE_RADIAL, RADIAL, OPENCV):
 *     r2 = x^2 + y^2;  xd = x (1 + k1 r2 + k2 r2^2) + 2 p1 x y + p2 (r2 + 2 x^2);  yd likewise with p1 and p2 swapped.
 *     camera direction (xu, -yu, -1).  All-zero coefficients give the bits of mode 1.
 * mode 3: equidistant fisheye, distortion = k1, k2, k3, k4 (COLMAP OPENCV_FISHEYE): theta_d = |(xd, yd)| =
 *     theta (1 + k1 theta^2 + k2 theta^4 + k3 theta^6 + k4 theta^8); camera direction (sin theta xd / theta_d, -sin theta yd / theta_d,
 *     -cos theta).  This direction is of UNIT length (modes 0-2: third component -1), so t, near and far of a mode-3 camera are distances
 *     along the ray; it is the only form that survives a 90 degree half-angle.
 * Radii of every mode: |d(y, x) - d(y + 1, x)| * 2/sqrt(12), the neighbour undistorted by its own solve. */
#define MIPNERF_CAMERA_FLOATS 32

typedef struct mipnerf_ctx mipnerf_ctx;

const char* mipnerf_last_error(void);
int mipnerf_abi_version(void);
/* Number of camera modes mipnerf_generate_rays knows (4: modes 0..3 above).  A library without this symbol knows modes 0 and 1 only
 * and would render a distorted record as a pinhole: check before building a mode-2 or mode-3 record. */
int mipnerf_num_camera_modes(void);

/* ---- context: configuration + packed weights ------------------------------------------ */
/* MipNerf.__init__ (mip_nerf.py:117-170).  Fails with MIPNERF_E_UNSUPPORTED when the MLP
 * shape is not the one the MFMA kernels were generated for (see mipnerf_compiled_arch). */
int mipnerf_create(const mipnerf_config* cfg, mipnerf_ctx** out);
int mipnerf_destroy(mipnerf_ctx* ctx);
/* Writes the MLP shape the library was compiled for into *cfg (other fields defaulted). */
int mipnerf_compiled_arch(mipnerf_config* cfg);
/* The library carries tables (+ a bf16 inference kernel) for a fixed list of MLP shapes ("variants", csrc/gen_mlp_bf16.py
 * VARIANTS); variant 0 is the shipped shape; bf16 TRAINING kernels + tables are generated per variant as well
 * (*has_bf16_training; a variant without them would train in fp32).
 * mipnerf_create picks the variant that matches cfg or fails with MIPNERF_E_UNSUPPORTED listing them. */
int mipnerf_num_variants(void);
int mipnerf_variant_arch(int variant, mipnerf_config* cfg, int* has_bf16_training);

/* Number of parameter tensors of the context's architecture = 2 x (net_depth + 3 + net_depth_condition) in the reference
 * MLP's state_dict order (MIPNERF_NUM_PARAM_TENSORS = 24 for the shipped 8-layer shape). */
int mipnerf_num_param_tensors(const mipnerf_ctx* ctx);
/* (Re)pack the fp32 master parameters into the MFMA operand streams (bf16 fragment stream,
 * fp32 fragment stream, bias tables).  `params` is a HOST array of
 * mipnerf_num_param_tensors(ctx) device pointers (24 for the shipped shape) in state_dict order of the reference MLP
 * (mip_nerf.py:19-73): layers.{0..7}.0.{weight,bias}, density_layer.{weight,bias},
 * extra_layer.{weight,bias}, view_layers.0.0.{weight,bias}, color_layer.{weight,bias}.
 * The bf16 forward stream multiplies the bottleneck into view layer 0 (W_view[:, :W] W_extra, b_view + W_view[:, :W] b_extra), computed
 * in the same launch with a float64 accumulator in a fixed order: the same parameters always give the same bits.
 * Call after every optimizer step / load_state_dict. */
int mipnerf_set_params(mipnerf_ctx* ctx, const float* const* params_host, void* stream);

/* ---- the whole hot path: MipNerf.forward (mip_nerf.py:172-248) ------------------------ */
size_t mipnerf_workspace_bytes(const mipnerf_ctx* ctx, int64_t num_rays);
/* t_rand [B,N+1] / u_rand [B,N+1]: uniform [0,1) noise replacing torch.rand (mip.py:159)
 * and uniform_ (mip.py:201); both NULL <=> randomized=False.  density_randn (NULL = none):
 * standard-normal draws [num_levels, B, N] replacing torch.randn of mip_nerf.py:232-233; the raw
 * density of level l becomes raw + cfg.density_noise * density_randn[l] before the softplus.
 * out[level], level < num_levels. */
int mipnerf_forward(mipnerf_ctx* ctx, int64_t num_rays, const mipnerf_rays* rays,
                    const float* t_rand, const float* u_rand, const float* density_randn,
                    uint32_t flags, int precision,
                    void* workspace, size_t workspace_bytes, const mipnerf_level_out* out,
                    void* stream);

/* ---- per-stage entry points (each parity-tested alone) --------------------------------- */
/* sample_along_rays (mip.py:127-165), t part: t_samples [B,N+1]. */
int mipnerf_sample_along_rays(int64_t num_rays, int32_t num_samples, const float* near,
                              const float* far, const float* t_rand, int32_t disparity,
                              float* t_samples, void* stream);
/* cast_rays (mip.py:81-103) + conical_frustum_to_gaussian (50-78) + lift_gaussian (22-36):
 * means, covs [B,N,3] (either may be NULL). */
int mipnerf_cast_rays(int64_t num_rays, int32_t num_samples, const float* t_samples,
                      const float* origins, const float* directions, const float* radii,
                      float* means, float* covs, void* stream);
/* cast_rays + integrated_pos_enc (mip.py:322-350) fused: enc [B*N, 6*(max_deg-min_deg)];
 * out_dtype MIPNERF_PREC_FP32 (float) or MIPNERF_PREC_BF16 (bfloat16 RNE). */
int mipnerf_cast_ipe(int64_t num_rays, int32_t num_samples, int32_t min_deg, int32_t max_deg,
                     int32_t disable_integration, const float* t_samples, const float* origins,
                     const float* directions, const float* radii, void* enc, int out_dtype,
                     void* stream);
/* integrated_pos_enc (mip.py:322-350, diagonal) on given means / covs [M,3]. */
int mipnerf_integrated_pos_enc(int64_t num_points, int32_t min_deg, int32_t max_deg,
                               const float* means, const float* covs, void* enc, int out_dtype,
                               void* stream);
/* pos_enc(viewdirs, 0, deg_view, append_identity=True) (mip.py:353-363): [B, 3+6*deg_view]
 * written with row stride `ld` elements (ld >= 3+6*deg; pad columns zeroed). */
int mipnerf_pos_enc(int64_t num_rays, int32_t deg_view, const float* viewdirs, void* out,
                    int32_t ld, int out_dtype, void* stream);
/* MLP.forward (mip_nerf.py:75-111) + activations (mip_nerf.py:236-238):
 * enc [M,xyz_dim] row-major (dtype = precision; xyz_dim = 96, or 672 for the unbounded-scene variant), viewenc [B,32]
 * (dtype = precision, ld 32), sample m belongs to ray m / num_samples.  rgb_sigma [M,4] = (r,g,b,sigma) after
 * sigmoid/padding and softplus(raw+bias); raw [M,4] = (raw_rgb, raw_density) or NULL.
 * bf16 on the unbounded-scene variant runs two kernels with 1.5 KiB of scratch per sample between them; this entry point has no
 * workspace argument, so the context keeps that buffer and GROWS it with hipMalloc when num_points exceeds every earlier call
 * (synchronises the stream, not capturable into a hipGraph at that moment; one stream at a time per context for this entry point on
 * that variant) -- mipnerf_forward uses the caller's workspace and has neither restriction. */
int mipnerf_mlp_forward(mipnerf_ctx* ctx, int64_t num_points, int32_t num_samples,
                        const void* enc, const void* viewenc, int precision, float* rgb_sigma,
                        float* raw, void* stream);
/* volumetric_rendering (mip.py:366-401). */
int mipnerf_volumetric_rendering(int64_t num_rays, int32_t num_samples, const float* rgb_sigma,
                                 const float* t_samples, const float* directions,
                                 int32_t white_bkgd, float* comp_rgb, float* distance, float* acc,
                                 float* weights, void* stream);
/* resample_along_rays (mip.py:232-280) t part: blur-pool + padding +
 * sorted_piecewise_constant_pdf (mip.py:168-229) with num_samples+1 draws. */
int mipnerf_resample_along_rays(int64_t num_rays, int32_t num_samples, const float* t_samples,
                                const float* weights, const float* u_rand, float resample_padding,
                                float* t_new, void* stream);
/* sorted_piecewise_constant_pdf alone (mip.py:168-229): bins [B,N+1], weights [B,N]
 * (not mutated), num_draws samples out [B,num_draws]. */
int mipnerf_sorted_piecewise_constant_pdf(int64_t num_rays, int32_t num_bins, const float* bins,
                                          const float* weights, int32_t num_draws,
                                          const float* u_rand, float* samples, void* stream);

/* ---- device-side ray generation (Blender._generate_rays datasets.py:214-263, Multicam._generate_rays :116-168):
 * ray i = pixel pix_idx[i] (row-major y*W + x; NULL = pixel i) of camera cam_idx[i] (NULL = camera 0) of the
 * `cameras` table [ncam][MIPNERF_CAMERA_FLOATS] (device memory).  Radii follow the reference: distance to the
 * neighbouring pixel along image rows, last row repeated, times 2/sqrt(12).  Camera modes 0..3: see MIPNERF_CAMERA_FLOATS; modes 2 and 3
 * (distorted COLMAP cameras) cost two 8-step Newton solves per ray, the pixel's and its neighbour's. */
int mipnerf_generate_rays(int64_t num_rays, const float* cameras, const int32_t* cam_idx,
                          const int32_t* pix_idx, const mipnerf_rays_out* out, void* stream);
/* The same with a camera table of DOUBLES and float64 arithmetic, results rounded to float32 once at the end: `RenderGen`
 * (render_video.py:29-112) forms its rays in float64 numpy from the float64 poses of create_spheric_poses and casts with .float()
 * (render_video.py:131); the radii are the norm of a DIFFERENCE of neighbouring directions (1e-3 of their size), which float32
 * arithmetic gets to 1e-4 relative only.  Same camera modes, same bits per (camera, pixel) as the float32 entry point has among its
 * own callers; the Newton solves of modes 2 and 3 run in float64 too. */
int mipnerf_generate_rays_f64(int64_t num_rays, const double* cameras, const int32_t* cam_idx,
                              const int32_t* pix_idx, const mipnerf_rays_out* out, void* stream);
/* One training batch of an epoch straight into caller-owned buffers (the static inputs of a captured training step):
 * b = *step - *epoch_base (device int64s, read when the kernel runs, so a replayed graph advances through the epoch);
 * ray i = global pixel id order[b * batch_size + i] over the concatenation of the `n_images` images of the `cameras` table,
 * image c found in the int64 table offsets[0..n_images] (pixel counts, cumulative; offsets[0] = 0), pixel id - offsets[c],
 * the arithmetic of mipnerf_generate_rays; gt[i][0..2] = pixels[id][0..2] (pixels [offsets[n_images]][3] fp32).  Bit-identical
 * to mipnerf_generate_rays of the same (camera, pixel) pairs, whatever their camera modes (a table may mix modes 0..3).  Rays whose
 * index is past n_order are left unwritten.
 * No host synchronisation, no allocation: capturable. */
int mipnerf_gather_train_batch(int64_t batch_size, int64_t n_order, const int64_t* order, int32_t n_images,
                               const int64_t* offsets, const float* cameras, const float* pixels, const int64_t* step,
                               const int64_t* epoch_base, const mipnerf_rays_out* out, float* gt, void* stream);

/* ---- error-guided batch sampling (train_guided.TrainGuided): which pixels a training batch holds --------------------------------
 * Every training image is cut into tiles of T x T pixels (smaller at the right and bottom edges); the tiles are the CELLS, numbered
 * image by image, row-major inside an image.  `table` (device, int64 [n_images + 1][4]): row i = (first cell of image i, first pixel of
 * image i, W_i, H_i), the last row = (n_cells, N = pixel count, 0, 0).  Cell c has n_c pixels.  State per cell: err (float, starts at 1),
 * sum (uint64), cnt (uint32), seen (uint8), q and cdf (uint32).  header (device, 4 x uint64): Q, A, cells visited since the start, n_cells.
 * The rule, integers wherever a sum crosses cells, so two runs give the same bytes:
 *   per draw    se = ((d0 d0) + d1 d1) + d2 d2 in float32 without contraction, d = rgb - gt; fx = (uint64) floor((double) se 2^24 + 0.5);
 *               a draw whose se is not finite or negative is not counted; sum_c += fx, cnt_c += 1 (integer vector atomics)
 *   fold        per cell with cnt_c > 0: mean = (float)(((double) sum_c / (double) cnt_c) 2^-24), err_c += rate (mean - err_c) in float32
 *               without contraction, seen_c = 1; then sum_c = cnt_c = 0
 *   mass        ef_c = (uint64) floor((double) err_c 2^20 + 0.5), a_c = n_c ef_c, A = sum a_c; share_c = (double) n_c / (double) N;
 *               p_c = (1 - mix) share_c + mix (A > 0 ? (double) a_c / (double) A : share_c) in float64, in this order;
 *               q_c = max(1, (uint64) floor(p_c 2^30)); cdf = inclusive integer scan of q, Q = cdf[n_cells - 1] (< 2^31: n_cells < 2^30)
 *   draw j      from two integers r0 = r[j], r1 = r[n_draws + j] in [0, 2^32) (int64): t = (r0 Q) >> 32, c = the first cell with cdf[c] > t,
 *               k = (r1 n_c) >> 32, the pixel is column x0 + k % w_c, row y0 + k / w_c of the cell; order[j] = first pixel of the image +
 *               y W + x; slot = (ring_start + j) % ring_len; weight[slot] = (float)(share_c / ((double) q_c / (double) Q)), cell[slot] = c
 * so a pixel is drawn with probability q_c / (Q n_c) to within 2^-32 / n_c, sum_c P_c w_c = 1 to float32 rounding and
 * w <= (1 + 1e-5) / (1 - mix).
 * mipnerf_guided_apply: lossmult[i] *= weight[(b batch_size + i) % ring_len] for the rays i of batch b; mipnerf_guided_accumulate: the
 * per-draw line above for ray i into cell[(b batch_size + i) % ring_len] (a ring entry outside [0, n_cells) is skipped).  Both take
 * b = *step - *epoch_base from the device, as mipnerf_gather_train_batch does, or, with step == NULL, b = host_batch; a ray with b < 0 or
 * b batch_size + i >= n_order is left alone.  Neither allocates or synchronises: capturable.
 * mipnerf_guided_refresh: fold + mass + scan in place (block totals, one single-workgroup pass over them, apply: no workgroup reads what
 * another wrote in the same launch), then the header.  scratch: at least 2 ceil(n_cells / 256) + 2 uint64 words.  0 <= mix < 1,
 * 0 < rate <= 1, 1 <= n_cells < 2^30.  mipnerf_guided_draw reads Q from the header on the device; n_draws = 0 returns without a launch.
 * Neither allocates or synchronises. */
int mipnerf_guided_apply(int64_t batch_size, int64_t n_order, int64_t ring_len, const float* weight, const int64_t* step,
                         const int64_t* epoch_base, int64_t host_batch, float* lossmult, void* stream);
int mipnerf_guided_accumulate(int64_t batch_size, int64_t n_order, int64_t ring_len, const int32_t* cell, int64_t n_cells,
                              const int64_t* step, const int64_t* epoch_base, int64_t host_batch, const float* rgb, const float* gt,
                              uint64_t* sum, uint32_t* cnt, void* stream);
int mipnerf_guided_refresh(int32_t n_images, const int64_t* table, int32_t tile, int64_t n_cells, float rate, double mix, float* err,
                           uint64_t* sum, uint32_t* cnt, uint8_t* seen, uint32_t* q, uint32_t* cdf, uint64_t* scratch,
                           size_t scratch_words, uint64_t* header, void* stream);
int mipnerf_guided_draw(int64_t n_draws, const int64_t* r, int32_t n_images, const int64_t* table, int32_t tile, int64_t n_cells,
                        const uint32_t* cdf, const uint64_t* header, int64_t* order, float* weight, int32_t* cell, int64_t ring_len,
                        int64_t ring_start, void* stream);

/* ---- unbounded scenes (mip-NeRF 360) --------------------------------------------------------------------------------
 * Correct versions of what the reference's dead code aims at (models/mip.py:106-124 sample_along_rays_360, :38-47 full
 * lift_gaussian, :424-447 contract / parameterization, :292-319 integrated_pos_enc_360); they follow Barron et al.,
 * "Mip-NeRF 360" (CVPR 2022), see csrc/raymath360.hpp.  Parity: against oracle/mipnerf360_oracle.py ("parity unpinned":
 * the reference code is broken and has no outputs to pin against).
 * sample_along_rays_360: fence posts uniform in normalised inverse depth, t = 1 / (s / far + (1 - s) / near); t_rand [B,N+1]
 *   (NULL = deterministic) jitters between midpoints in inverse-depth space.  Outputs t_inv, t_samples [B,N+1].
 * cast_ipe_360: t [B,N+1] -> conical-frustum Gaussians with FULL covariance -> scene contraction of mean and covariance
 *   (contracted != 0) -> off-axis IPE on 21 basis directions and frequencies 2^l, l in [min_deg, max_deg):
 *   enc [B*N, 2*21*(max_deg-min_deg)] (fp32 or bf16; feature = half*21L + l*21 + basis; or MIPNERF_OUT_BF16_FRAGMENTS).  means [B*N,3] / covs [B*N,3,3]
 *   (both or neither; may be the only outputs, enc = NULL) receive the (contracted) Gaussians. */
int mipnerf_sample_along_rays_360(int64_t num_rays, int32_t num_samples, const float* near, const float* far,
                                  const float* t_rand, float* t_inv, float* t_samples, void* stream);
int mipnerf_cast_ipe_360(int64_t num_rays, int32_t num_samples, int32_t min_deg, int32_t max_deg, int32_t contracted,
                         const float* t_samples, const float* origins, const float* directions, const float* radii,
                         void* enc, int out_dtype, float* means, float* covs, void* stream);
/* The same on GIVEN Gaussians, means [M,3] / covs [M,3,3]: contraction of mean and covariance (contracted != 0; `contract`,
 * `parameterization`, mip.py:424-447) into means_out / covs_out (covs_out may be NULL) and / or the off-axis encoding
 * enc [M, 2*21*(max_deg-min_deg)] (`integrated_pos_enc_360`, mip.py:292-319) of the (contracted) Gaussians. */
int mipnerf_gauss_360(int64_t num_points, int32_t min_deg, int32_t max_deg, int32_t contracted, const float* means,
                      const float* covs, void* enc, int out_dtype, float* means_out, float* covs_out, void* stream);

/* ---- evaluation metrics: eval_errors (utils/metrics.py:191-197) on one frame: pred, gt [H,W,3] fp32 in [0,1];
 * out[0] = PSNR (metrics.py:182-188), out[1] = mean SSIM, 11x11 Gaussian window sigma 1.5, zero padding
 * (metrics.py:44-126).  workspace: mipnerf_eval_workspace_floats(H, W) floats. */
int64_t mipnerf_eval_workspace_floats(int32_t height, int32_t width);
int mipnerf_eval_errors(int32_t height, int32_t width, const float* pred, const float* gt,
                        float* workspace, float* out_psnr_ssim, void* stream);

/* ---- image bytes (utils/vis.py:save_images): what the reference writes to PNG, as packed uint8 RGB on the device.
 * mipnerf_visualize_map: visualize_depth (vis.py:83-97) of one map [num_pixels] fp32 (distance or acc) -> out_rgb
 * [num_pixels, 3]: nan_to_num, min / max over the whole map, (x - min) / max(max - min, 1e-8) in fp32, (uint8)(255 x)
 * truncated, then the JET row of that value as the reference writes it (OpenCV's BGR LUT stored as RGB).
 * workspace: mipnerf_visualize_workspace_floats(num_pixels) floats.
 * mipnerf_image_to_u8: torchvision save_image of an image already clamped by save_image_tensor: x [num_values] fp32 ->
 * out [num_values] = (uint8)(clamp(x, 0, 1) * 255 + 0.5).  Neither allocates or synchronises (graph-capturable). */
int64_t mipnerf_visualize_workspace_floats(int64_t num_pixels);
int mipnerf_visualize_map(int64_t num_pixels, const float* map, float* workspace, uint8_t* out_rgb, void* stream);
int mipnerf_image_to_u8(int64_t num_values, const float* x, uint8_t* out, void* stream);

/* ---- multi-scale Blender converter (datasets/convert_blender_data.py:34-37 `down2`, 65-81 the level loop): the box pyramid
 * of num_images RGBA8 frames src_rgba [num_images, H, W, 4]; H and W divisible by 2^(num_levels-1), 1 <= num_levels <=
 * MIPNERF_MAX_PYRAMID_LEVELS (else MIPNERF_E_INVALID before any launch).  Level 0 is v = float(byte) / 255.f, level j+1 the
 * float32 mean of each 2x2 block of the UNQUANTISED level j, summed ((p00 + p01) + p10) + p11 (row-major in the block) and
 * divided by 4, as numpy's mean over axes (1, 3) does.  With H_j = H >> j, W_j = W >> j, PPI = sum_j H_j W_j:
 *   out_u8   level-major: level j is [num_images, H_j, W_j, 4] at byte offset 4 * num_images * sum_{k<j} H_k W_k; the bytes
 *            (uint8)(v * 255.f), truncating, that the converter writes to NNN_dj.png.  4 * num_images * PPI bytes.
 *   out_rgb  (may be NULL) float32 rows [*, 3] in the data set's order: pixel (y, x) of level j of image i is row
 *            rgb_row_offset + i * PPI + sum_{k<j} H_k W_k + y * W_j + x; the value datasets.py:108-111 makes of the PNG:
 *            q = float(byte) / 255.f, white_bkgd != 0: q_rgb * q_a + (1.f - q_a) (three roundings), else q_rgb.
 *   scratch  num_levels > 4 only (else may be NULL): 4 * num_images * (H_3 W_3 + H_4 W_4) floats.
 * src_rgba, out_u8 and scratch 16-byte aligned.  Does not allocate or synchronise (graph-capturable). */
#define MIPNERF_MAX_PYRAMID_LEVELS 8
int mipnerf_box_pyramid(int32_t num_images, int32_t height, int32_t width, int32_t num_levels, const uint8_t* src_rgba,
                        uint8_t* out_u8, float* out_rgb, int64_t rgb_row_offset, int32_t white_bkgd, float* scratch,
                        void* stream);

/* ---- box shrink of captured images (LLFF / mip-NeRF-360 `images/` -> what `images_<factor>/` would hold): src
 * [num_images, height, width, channels] bytes, channels 3 or 4 (a 4th channel is dropped, no compositing), 1 <= factor <=
 * MIPNERF_MAX_DOWNSCALE_FACTOR, height and width >= factor (else MIPNERF_E_INVALID before any launch).  h = height / factor,
 * w = width / factor; the height % factor bottom rows and width % factor right columns are ignored.  Per output channel value:
 * S = the integer sum of the factor x factor source bytes, q = (2 S + factor^2) / (2 factor^2) in integer arithmetic (the box
 * mean rounded half up to a byte), and out_rgb row rgb_row_offset + (i * h + y) * w + x, float32 [*, 3], gets float(q) / 255.f
 * (one correctly rounded division).  src 16-byte aligned.  Does not allocate or synchronise (graph-capturable). */
#define MIPNERF_MAX_DOWNSCALE_FACTOR 16
int mipnerf_area_downscale(int32_t num_images, int32_t height, int32_t width, int32_t channels, int32_t factor, const uint8_t* src,
                           float* out_rgb, int64_t rgb_row_offset, void* stream);

/* ---- geometry out of a trained field: density on a lattice, isosurface of any lattice (ABI 6 grows; nothing above changes) ----
 * A lattice has dims = (nx, ny, nz) points, each >= 2, over the box lo[3] .. hi[3] (HOST arrays, (x, y, z) order); 7 nx ny nz < 2^31
 * (indices are 32-bit; 512 x 512 x 512 fits), else MIPNERF_E_INVALID before any launch.  Point (i, j, k) has the flat index
 * (k * ny + j) * nx + i and, per axis, the mean lo + float(i) * h with h = (hi - lo) / float(n - 1), in fp32 without contraction.
 * mipnerf_density_grid: the field's activated density softplus(raw + density_bias) at an isotropic-per-axis Gaussian on every point:
 * diagonal covariance cov_scale * h * h / 12 (the variance of a uniform box of side h; cov_scale = 0 is a point query), sigma
 * [nz, ny, nx] fp32.  The lattice is walked in chunks: encoding rows written from the lattice index (the device code of
 * mipnerf_integrated_pos_enc, no means or covariances in memory), the MLP path of mipnerf_mlp_forward on a ZERO view encoding (its
 * colour is dropped), a strided store of the density.  The chunk is what the workspace holds: any size from
 * mipnerf_density_grid_workspace_bytes(ctx, chunk_points >= 1, precision) on is accepted (16-byte aligned), results do not depend on
 * it; a chunk past 256 points is cut to whole 256-point tiles.  Both precisions and every MLP shape of the bounded model;
 * cfg.unbounded = 1: MIPNERF_E_UNSUPPORTED (that model's lattice has to name its space: mipnerf_density_grid_360 below).  Does not allocate or
 * synchronise (graph-capturable). */
size_t mipnerf_density_grid_workspace_bytes(const mipnerf_ctx* ctx, int64_t chunk_points, int precision);
int mipnerf_density_grid(mipnerf_ctx* ctx, const int32_t* dims_host, const float* lo_host, const float* hi_host, float cov_scale,
                         int precision, float* sigma, void* workspace, size_t workspace_bytes, void* stream);
/* ---- the density lattice as the proposal level of a forward (ABI 6 grows; bounded model, inference) ----
 * Trilinear value of an fp32 device lattice [nz, ny, nx] (the layout above; mipnerf_density_grid's output is one) at a point,
 * stated once in csrc/lattice_sample.hpp: per axis u = (x - lo) * inv_h with inv_h = float(n - 1) / (hi - lo) computed once on the host
 * (no division on the device), u clamped to [0, n - 1] (a point outside the box takes the edge value), i0 = min(int(floorf(u)), n - 2),
 * f = u - float(i0) (a point on the hi face gives f = 1); the 8 corners are blended along x, then y, then z, each step as
 * (1 - f) * a + f * b in fp32 without contraction, so non-negative corners give a non-negative value.  A non-finite coordinate gives 0;
 * a NaN among the 8 corners propagates.
 * mipnerf_lattice_density: the stage on its own.  One thread per sample: rgb_sigma[b, i] = (0, 0, 0, value at the mean of
 * conical_frustum_to_gaussian(t[b, i], t[b, i + 1]) of ray b) -- the mean mipnerf_cast_rays returns, bit for bit --, [B, N, 4] as
 * mipnerf_mlp_forward writes it.  MIPNERF_E_INVALID before any device call for a null pointer, an axis below 2 points, hi <= lo or
 * num_samples outside 1 .. MIPNERF_MAX_SAMPLES; num_rays = 0 returns without a launch.  Does not allocate or synchronise.
 * mipnerf_forward_proposal: mipnerf_forward with level 0's encoding and MLP launch replaced by that kernel, writing into the same
 * rgb_sigma buffer; the ray prologue, level 0's compositing + resampling and all of level 1 are mipnerf_forward's launches (options 3
 * and 4 apply as there: same bits either way).  Level 0's outputs are what compositing yields for colour 0 and the lattice's density:
 * comp_rgb = the background times (1 - acc) -- the lattice's silhouette, not a coarse render --, acc, distance, weights and t_samples as
 * usual; level 1 draws its samples from those weights.  The picture is NOT mipnerf_forward's: the fine samples sit elsewhere.  Needs
 * mipnerf_workspace_bytes and no more.  MIPNERF_E_UNSUPPORTED for cfg.unbounded = 1 (that model's proposal pyramid is read by
 * mipnerf_lattice_density_360 of include/mipnerf_proposal_360.h, a library of its own, and its level loop is composed of the stage entry
 * points around that call; there is no single entry point for it) and for
 * num_levels != 2; MIPNERF_E_INVALID for the lattice argument errors above.  No density noise.  Graph-capturable like mipnerf_forward. */
int mipnerf_lattice_density(const int32_t* dims_host, const float* lo_host, const float* hi_host, const float* lattice, int64_t num_rays,
                            int32_t num_samples, const float* t_samples, const float* origins, const float* directions, const float* radii,
                            float* rgb_sigma, void* stream);
int mipnerf_forward_proposal(mipnerf_ctx* ctx, int64_t num_rays, const mipnerf_rays* rays, const int32_t* dims_host, const float* lo_host,
                             const float* hi_host, const float* lattice, const float* t_rand, const float* u_rand, uint32_t flags,
                             int precision, void* workspace, size_t workspace_bytes, const mipnerf_level_out* out, void* stream);
/* Marching tetrahedra on the Kuhn split of ANY fp32 device lattice grid [nz, ny, nx] (it need not be a density): every cell is cut
 * into the six tetrahedra (c, c + e_p0, c + e_p0 + e_p1, c + (1,1,1)), p the permutations of the axes in lexicographic order; 16
 * sign cases, none ambiguous, face diagonals of neighbouring cells coincide, so a surface that stays off the box is a closed,
 * consistently oriented 2-manifold.  Where it reaches the box it is cut open, not capped.
 *   - a point is inside when grid > threshold (NaN and a value equal to the threshold are outside);
 *   - one vertex per lattice edge whose ends differ; a point owns the 7 edges to its larger neighbours, slots x, y, xy, z, xz, yz,
 *     xyz (the order of the far end's flat index); position p_in + t (p_out - p_in), t = (threshold - f_in) / (f_out - f_in) in fp32,
 *     t = 0.5 when that is not finite; vertices ordered by (owning point, slot) = sorted by (smaller end, larger end);
 *   - faces int32 [F, 3] ordered by (cell, tetrahedron, triangle), wound so that the normal points from inside to outside; the winding
 *     comes from the sign case and the tetrahedron (that of the triangle through the edge midpoints), never from positions, so a
 *     triangle that collapses because a lattice value equals the threshold keeps a defined winding and is kept;
 *   - normals [V, 3]: -grad f normalised; the gradient by central differences at the two ends of the edge (one-sided on the faces of
 *     the box), interpolated with the same t; (0, 0, 0) where it is zero or not finite;
 *   - vertex_edges int64 [V, 2]: flat indices of the (inside, outside) ends of each vertex's edge.
 * Both orders come from exclusive scans, not atomics: two runs give identical bytes.
 * mipnerf_isosurface_count classifies and scans into `workspace` (mipnerf_isosurface_workspace_bytes, 16-byte aligned), SYNCHRONISES
 * the stream and returns V and F through host pointers -- it cannot be captured into a hipGraph.  mipnerf_isosurface_emit fills the
 * caller's buffers (any may be NULL) from the same workspace, grid, dims and threshold; it does not synchronise. */
size_t mipnerf_isosurface_workspace_bytes(int32_t nx, int32_t ny, int32_t nz);
int mipnerf_isosurface_count(const int32_t* dims_host, const float* grid, float threshold, void* workspace, size_t workspace_bytes,
                             int64_t* num_vertices_host, int64_t* num_faces_host, void* stream);
int mipnerf_isosurface_emit(const int32_t* dims_host, const float* lo_host, const float* hi_host, const float* grid, float threshold,
                            const void* workspace, size_t workspace_bytes, float* vertices, float* normals, int32_t* faces,
                            int64_t* vertex_edges, void* stream);

/* ---- lattice of the unbounded-scene model (cfg.unbounded = 1; ABI 6 grows; nothing above changes) ----
 * The MLP of that model reads the off-axis encoding of CONTRACTED Gaussians, so a lattice has to say in which space it lies.  dims, lo,
 * hi, the flat index, h and cov_scale are those of the lattice above.
 *   MIPNERF_SPACE_WORLD       the lattice lies in world coordinates: the Gaussian (lo + float(i) * h, diag(cov_scale * h * h / 12)) per
 *                             axis in fp32 is contracted -- mean' = contract(mean), cov' = J cov J^T, the generic triple product of
 *                             csrc/raymath360.hpp contract_gaussian, the sequence mipnerf_gauss_360 runs with contracted = 1 -- and then
 *                             encoded.  For the central object of a capture.
 *   MIPNERF_SPACE_CONTRACTED  the lattice is uniform in the contracted coordinates z (the whole scene lies in |z| < 2; the usual box is
 *                             [-2, 2]^3): the Gaussian (z, diag(cov_scale * h * h / 12)) is encoded as it stands (contracted = 0).  With
 *                             c = 2.f - 1.f / far_radius in fp32 (far_radius finite and > 1, world units) a point is OUTSIDE when its
 *                             fp32 (zx * zx + zy * zy) + zz * zz exceeds c * c, and its density is then exactly 0.f.  far_radius is not
 *                             read in world space.
 * Un-contraction z -> x with contract(x) = z, in fp32: n = sqrt((zx * zx + zy * zy) + zz * zz); n <= 1: x = z; otherwise
 * r = min(1.f / (2.f - min(n, c)), far_radius) and x = z * (r / n).  |z| is capped at c and the difference is exact for n in [1, 2]; the
 * outer minimum keeps the promise that no result lies beyond far_radius where c is rounded up (far_radius no power of two) or to 2
 * (far_radius >= 2^24).  A normal g of the contracted lattice is a density-gradient direction; its world direction is J^T g with the
 * symmetric Jacobian J of the contraction at x, evaluated as normalize((2 r - 1) (g - (u . g) u) + (u . g) u), u = z / n; n <= 1: g
 * unchanged; (0, 0, 0), or a result that is not finite, gives (0, 0, 0).
 * mipnerf_density_grid_360: sigma [nz, ny, nx] fp32 of the lattice, walked in chunks as mipnerf_density_grid does: encoding rows from the
 * lattice index (fp32 rows, or bf16 fragments of whole 256-point tiles), the MLP path of mipnerf_mlp_forward on a zero view encoding (bf16:
 * the one-kernel form where the variant has one and option 6 is on, else the two-kernel form with its scratch inside the workspace), the
 * density store (with the outside rule in the contracted space).  The chunk is the largest the workspace holds by
 * mipnerf_density_grid_360_workspace_bytes(ctx, chunk_points >= 1, precision) (256-byte aligned); a chunk past 256 points is cut to whole
 * 256-point tiles; results do not depend on it.  MIPNERF_E_UNSUPPORTED: a bounded context, or a variant without a kernel at `precision`
 * (the workspace size is then 0).  MIPNERF_E_INVALID before any launch: bad dims, an unknown space, far_radius not finite or <= 1,
 * cov_scale negative or not finite.  Does not allocate or synchronise (graph-capturable).
 * mipnerf_lattice_ipe_360: the encoder alone (no context): rows [count, 42 * (max_deg - min_deg)] of the lattice points first ..
 * first + count - 1 in fp32, bf16 or MIPNERF_OUT_BF16_FRAGMENTS (the buffer then holds ceil(count / 256) * 256 rows; points past the end
 * repeat the last one); max_deg - min_deg a multiple of 8; enc 32-byte aligned.  Bit-identical to mipnerf_gauss_360 on the same Gaussians.
 * mipnerf_uncontract_vertices: z [V, 3] -> x_out [V, 3] (may be NULL) and, when normals_z [V, 3] is given, normals_out [V, 3] by the rules
 * above.  V = 0 returns without a launch.  Does not allocate or synchronise. */
enum { MIPNERF_SPACE_WORLD = 0, MIPNERF_SPACE_CONTRACTED = 1 };
size_t mipnerf_density_grid_360_workspace_bytes(const mipnerf_ctx* ctx, int64_t chunk_points, int precision);
int mipnerf_density_grid_360(mipnerf_ctx* ctx, const int32_t* dims_host, const float* lo_host, const float* hi_host, float cov_scale,
                             int space, float far_radius, int precision, float* sigma, void* workspace, size_t workspace_bytes,
                             void* stream);
int mipnerf_lattice_ipe_360(const int32_t* dims_host, const float* lo_host, const float* hi_host, int64_t first, int64_t count,
                            float cov_scale, int space, int32_t min_deg, int32_t max_deg, void* enc, int out_dtype, void* stream);
int mipnerf_uncontract_vertices(int64_t num_vertices, float far_radius, const float* z, const float* normals_z, float* x_out,
                                float* normals_out, void* stream);

/* ---- empty-space skipping for whole frames: occupancy bits of any lattice, ray culling, compaction (ABI 6 grows; nothing above changes) ----
 * The conventions are those of the lattice above: dims = (nx, ny, nz) points over lo .. hi in (x, y, z) order, h = (hi - lo) /
 * float(n - 1) per axis in fp32.  There are (nx - 1) (ny - 1) (nz - 1) CELLS; cell (i, j, k) spans lo + i h .. lo + (i + 1) h.
 *   - cell (i, j, k) is raw-occupied iff any of its 8 corner values grid[k + dz][j + dy][i + dx] is > threshold or is NaN;
 *   - a cell is occupied iff any raw-occupied cell lies within Chebyshev distance `dilate` (>= 0) of it;
 *   - storage is bit-packed along x: uint32 bits [nz - 1, ny - 1, ceil((nx - 1) / 32)]; cell i is bit i & 31 of word i >> 5; padding bits
 *     are 0.  mipnerf_occupancy_words is that word count (0 for dims no lattice may have).
 * mipnerf_occupancy_build: one lane per cell, a wave's ballot is two words; dilation is three separable passes on the packed words
 * (`scratch`: as many words again, needed only when dilate > 0).  No atomics: two runs give the same bytes.  Does not allocate or
 * synchronise (graph-capturable).
 * mipnerf_occupancy_refresh: the lattice a training run keeps while its field changes.  For every lattice point p: d = decay *
 * running[p] (one fp32 multiply) and running[p] = (fresh[p] > d || isnan(fresh[p]) || isnan(d)) ? fresh[p] : d -- the larger of the
 * decayed old value and the fresh one, where a NaN of `fresh` is kept and a NaN (or the 0 * inf of decay = 0) left in `running` is
 * replaced by `fresh`.  Then `bits` becomes exactly what mipnerf_occupancy_build(dims, running, threshold, dilate, bits, scratch) writes
 * (the call launches those kernels after k_lattice_decay_max: 12 bytes per point, 16-byte loads and stores where both lattices are
 * 16-byte aligned, a scalar tail).  `fresh` and `running` [nz, ny, nx] must not overlap; decay in [0, 1] (NaN refused); the other
 * arguments as mipnerf_occupancy_build (`scratch` only when dilate > 0).  No atomics: two runs give the same bytes.  Does not allocate or
 * synchronise (graph-capturable).
 * mipnerf_ray_occupancy: live [num_rays] bytes (1 / 0).  Per ray the coarse level's deterministic fence posts t_0 .. t_N (those of
 * mipnerf_sample_along_rays with t_rand = NULL: near + (far - near) * linspace(0, 1, N + 1)[i], or linear in disparity); frustum i has
 * the end points p0 = o + t_i d and p1 = o + t_{i+1} d, the half-width rho = cone_scale * radii * t_{i+1}, per axis the bounding
 * interval [min(p0, p1) - rho, max(p0, p1) + rho] and the cell range floor((x - lo) / h) of its two ends, inclusive at both ends.  The
 * part of a range that falls outside the grid counts as occupied when outside_occupied != 0, otherwise it is clipped away.  A ray is
 * live iff some frustum's cell range contains an occupied bit (a ray with a NaN coordinate is live).  Fine samples lie inside
 * [t_0, t_N], so the coarse frusta cover them.  hi > lo on every axis, 1 <= num_samples <= MIPNERF_MAX_SAMPLES.  viewdirs and lossmult
 * of `rays` are not read.  Does not allocate or synchronise.
 * mipnerf_ray_span: the occupied span of every ray.  "Frustum i hits" is exactly the per-frustum test of mipnerf_ray_occupancy above (the
 * same fence posts, p0, p1, rho, cell ranges, clipping and outside_occupied), and live [num_rays] is byte for byte what
 * mipnerf_ray_occupancy writes for the same arguments.  first = the smallest hitting frustum index, last = the largest; near' = t_first
 * and far' = t_{last + 1}: near_out and far_out are the fence posts themselves, the same fp32 function of (near, far, N, i) that
 * mipnerf_sample_along_rays evaluates with t_rand = NULL, bit for bit.  A dead ray gets first = N, last = -1, near' = near and
 * far' = far.  first, last (int32 [num_rays]) and near_out, far_out (fp32 [num_rays]) may each be NULL and are then skipped.  One
 * wavefront per ray: the 64-frustum buckets are tested forward up to the first one with a hit and then backward from the last one down
 * to it; no bucket is tested twice and a dead ray costs what it costs mipnerf_ray_occupancy.  What a renderer drops when it samples
 * [near', far'] instead of [near, far] lies in frusta that hit nothing: only in cells whose 8 lattice corners are at or below the
 * threshold, after dilation -- the statement culling makes about dead rays -- but the samples of a tightened ray sit elsewhere, so its
 * results are NOT those of the untightened ray.  The frusta cover [near, far] for any N, so the span found with one num_samples is valid
 * for a renderer that uses another.  Arguments, validation and the zero-ray return as mipnerf_ray_occupancy.  Does not allocate or
 * synchronise.
 * mipnerf_ray_occupancy_360 / mipnerf_ray_span_360: the same two calls for the unbounded-scene model and a bit grid laid out in CONTRACTED
 * coordinates (the bits of a lattice of mipnerf_density_grid_360 with MIPNERF_SPACE_CONTRACTED; the whole scene lies in |z| < 2, so the box
 * is usually [-2, 2]^3).  There is no disparity argument: the fence posts are those of mipnerf_sample_along_rays_360 with t_rand = NULL,
 * t_i = 1 / (fi s_i + (1 - s_i) ni) with ni = 1 / near, fi = 1 / far, s_i = linspace(0, 1, N + 1)[i], bit for bit (one device function
 * serves the sampler and these kernels), and near_out / far_out are those values.  Frustum i (t0 = t_i, t1 = t_{i+1}, rho = cone_scale *
 * radii * t1, p0 = o + t0 d, p1 = o + t1 d) is bounded per axis by an interval [lo_a, hi_a] of contracted coordinates that contains
 * contract(x) for every x = o + t d + delta with t in [t0, t1], delta perpendicular to d and |delta| <= cone_scale * radii * t.  The rule
 * uses that contract keeps directions -- contract(x) = f(|x|) x / |x| with f(r) = r for r <= 1 and 2 - 1 / r otherwise -- and that
 * |x / |x| - p / |p|| <= |x - p| / sqrt(|x| |p|).  With tc = clamp(-(o.d) / (d.d), t0, t1), rc = |o + tc d|, rmin = rc - rho and
 * rmax = max(|p0|, |p1|) + rho:
 *   - rmin >= 1 (the frustum lies wholly outside the unit ball): u0 = p0 / |p0|, u1 = p1 / |p1|, sag = 1 - sqrt(max(0, (1 + u0.u1) / 2))
 *     (the sagitta of the great-circle arc between them), e = sag + rho / rmin, ulo_a = max(min(u0_a, u1_a) - e, -1), uhi_a =
 *     min(max(u0_a, u1_a) + e, 1), flo = 2 - 1 / rmin, fhi = 2 - 1 / rmax, lo_a = ulo_a < 0 ? ulo_a fhi : ulo_a flo, hi_a = uhi_a > 0 ?
 *     uhi_a fhi : uhi_a flo;
 *   - otherwise: the world interval of the bounded rule, xlo_a = min(p0_a, p1_a) - rho, xhi_a = max(p0_a, p1_a) + rho, slo = rmax > 1 ?
 *     (2 - 1 / rmax) / rmax : 1, lo_a = xlo_a < 0 ? xlo_a : xlo_a slo, hi_a = xhi_a > 0 ? xhi_a : xhi_a slo, both clamped to [-F, F] with
 *     F = rmax > 1 ? 2 - 1 / rmax : rmax.
 * The cell range of [lo_a, hi_a], the clipping, outside_occupied (which keeps its meaning for a box smaller than [-2, 2]^3), the ballot
 * walk and the results of a dead ray are those of the bounded calls; a value that is not finite anywhere makes the frustum "outside", so
 * such a ray is never culled when outside_occupied != 0.  Density is 0 beyond |z| = 2 - 1 / far_radius on the lattice, so far_radius must
 * be no smaller than the largest |o + far d| of the rays to be classified.  Arguments (without `disparity`), validation and the zero-ray
 * return as the bounded calls.  Neither call allocates or synchronises.
 * mipnerf_compact_rays: an exclusive scan of `live` (sums per 1024 rays, one single-workgroup scan, per-ray bases; no atomics), then
 * the live rays gathered IN THEIR ORIGINAL ORDER into out_rays (a NULL field is skipped) and out_index[j] = the source ray of compact
 * slot j.  The live count has to reach the host: the call makes one 8-byte read-back and SYNCHRONISES the stream -- it cannot be
 * captured into a hipGraph.  workspace: mipnerf_compact_rays_workspace_bytes(num_rays), 16-byte aligned; live 4-byte aligned;
 * num_rays < 2^31; num_rays = 0 returns count 0 without a launch.
 * mipnerf_scatter_frame: writes every pixel of every level once (comp_rgb, distance, acc of `full`; weights / t_samples are not
 * touched): pixel index[j], j < count, takes slot j of `compact`; a pixel with live = 0 takes what volumetric_rendering (mip.py:395-400)
 * yields for all-zero weights: rgb = 1 with white_bkgd != 0 else 0, acc = 0, distance = near[pixel].  1 <= num_levels <= 4.  Does not
 * allocate or synchronise.
 * mipnerf_bucket_rays: a sample count per ray that follows its occupied span.  S = span_samples (the frusta count first / last were found
 * with), N = num_samples (the count the renderer uses), ladder c_0 < c_1 < ... < c_{B-1} with 1 <= c_0, c_{B-1} == N and 1 <= B <= 8.  For a
 * live ray with span [first, last]: need = ((last - first + 1) * N + S - 1) / S in integer division (1 <= need <= N) and bucket = the
 * smallest b with c_b >= need; a dead ray has bucket -1.  A ray of bucket b is meant to be rendered with c_b samples per level on
 * [near', far'], so its coarse spacing is at most the untightened ray's: (far' - near') / c_b <= (far - near) / N.  The call is a stable
 * B-way partition of the rays by bucket (counts per 1024 rays and bucket, one single-workgroup scan, per-ray ranks; no atomics): segment b
 * begins at base_0 = 0, base_{b+1} = round_up(base_b + count_b, 64), and within a bucket the rays keep their original order.  out_rays
 * (a NULL field is skipped) holds num_rays + 64 * B rays; the padding slots between the segments are never written.  slot[ray] (int32)
 * is the compact slot of the ray, or -1 for a dead ray; counts_host [B] receives the counts: one read-back and one stream
 * SYNCHRONISATION per call -- it cannot be captured into a hipGraph.  `rays` are read as given: pass the span arrays near' / far' as its
 * near / far to gather tightened rays.  workspace: mipnerf_bucket_rays_workspace_bytes(num_rays, num_buckets), 16-byte aligned;
 * num_rays < 2^31; num_rays = 0 returns zero counts without a launch.  S and N in [1, MIPNERF_MAX_SAMPLES].
 * mipnerf_gather_frame: writes every pixel of every level once (comp_rgb, distance, acc of `full`): a pixel with slot >= 0 copies compact
 * slot `slot` (slot < compact_rows, the rows the compact outputs hold; a slot outside them is treated as dead); a pixel with slot < 0 gets
 * the dead-pixel rule of mipnerf_scatter_frame: rgb = 1 with white_bkgd != 0 else 0, acc = 0, distance = near[pixel], the ORIGINAL near.
 * 1 <= num_levels <= 4.  Does not allocate or synchronise. */
int64_t mipnerf_occupancy_words(int32_t nx, int32_t ny, int32_t nz);
int mipnerf_occupancy_build(const int32_t* dims_host, const float* grid, float threshold, int32_t dilate, uint32_t* bits,
                            uint32_t* scratch, void* stream);
int mipnerf_occupancy_refresh(const int32_t* dims_host, const float* fresh, float* running, float decay, float threshold, int32_t dilate,
                              uint32_t* bits, uint32_t* scratch, void* stream);
int mipnerf_ray_occupancy(const int32_t* dims_host, const float* lo_host, const float* hi_host, const uint32_t* bits, int64_t num_rays,
                          int32_t num_samples, const mipnerf_rays* rays, int32_t disparity, int32_t outside_occupied, float cone_scale,
                          uint8_t* live, void* stream);
int mipnerf_ray_span(const int32_t* dims_host, const float* lo_host, const float* hi_host, const uint32_t* bits, int64_t num_rays,
                     int32_t num_samples, const mipnerf_rays* rays, int32_t disparity, int32_t outside_occupied, float cone_scale,
                     uint8_t* live, int32_t* first, int32_t* last, float* near_out, float* far_out, void* stream);
int mipnerf_ray_occupancy_360(const int32_t* dims_host, const float* lo_host, const float* hi_host, const uint32_t* bits, int64_t num_rays,
                              int32_t num_samples, const mipnerf_rays* rays, int32_t outside_occupied, float cone_scale, uint8_t* live,
                              void* stream);
int mipnerf_ray_span_360(const int32_t* dims_host, const float* lo_host, const float* hi_host, const uint32_t* bits, int64_t num_rays,
                         int32_t num_samples, const mipnerf_rays* rays, int32_t outside_occupied, float cone_scale, uint8_t* live,
                         int32_t* first, int32_t* last, float* near_out, float* far_out, void* stream);
size_t mipnerf_compact_rays_workspace_bytes(int64_t num_rays);
int mipnerf_compact_rays(int64_t num_rays, const uint8_t* live, const mipnerf_rays* rays, const mipnerf_rays_out* out_rays,
                         int32_t* out_index, void* workspace, size_t workspace_bytes, int64_t* count_host, void* stream);
int mipnerf_scatter_frame(int64_t num_rays, int64_t count, int32_t num_levels, const int32_t* index, const uint8_t* live,
                          const float* near, int32_t white_bkgd, const mipnerf_level_out* compact, const mipnerf_level_out* full,
                          void* stream);
size_t mipnerf_bucket_rays_workspace_bytes(int64_t num_rays, int32_t num_buckets);
int mipnerf_bucket_rays(int64_t num_rays, const uint8_t* live, const int32_t* first, const int32_t* last, int32_t span_samples,
                        int32_t num_samples, int32_t num_buckets, const int32_t* ladder_host, const mipnerf_rays* rays,
                        const mipnerf_rays_out* out_rays, int32_t* slot, void* workspace, size_t workspace_bytes, int64_t* counts_host,
                        void* stream);
int mipnerf_gather_frame(int64_t num_rays, int64_t compact_rows, int32_t num_levels, const int32_t* slot, const float* near,
                         int32_t white_bkgd, const mipnerf_level_out* compact, const mipnerf_level_out* full, void* stream);

/* ---- training side ---------------------------------------------------------------------- */
/* activations (mip_nerf.py:236-238): raw [M,4] = (raw_rgb, raw_density) -> rgb_sigma [M,4];
 * density_randn [M] (NULL = none): raw_density + density_noise * density_randn first (mip_nerf.py:232-233). */
int mipnerf_activate(int64_t num_points, const float* raw, float rgb_padding, float density_bias,
                     const float* density_randn, float density_noise, float* rgb_sigma, void* stream);
/* backward of volumetric_rendering (mip.py:366-401) fused with the activation derivatives:
 * upstream g_rgb [B,3], g_dist [B], g_acc [B], g_w [B,N] (any may be NULL = zero) ->
 * d_raw [B*N,4] = dL/d(raw_rgb, raw_density).  rgb_sigma is the ACTIVATED forward tensor. */
int mipnerf_volumetric_rendering_bwd(int64_t num_rays, int32_t num_samples, const float* rgb_sigma,
                                     const float* t_samples, const float* directions,
                                     int32_t white_bkgd, const float* g_rgb, const float* g_dist,
                                     const float* g_acc, const float* g_w, float rgb_padding,
                                     float* d_raw, void* stream);
/* distloss (mip.py:8-20) without the [B,N,N] temporaries: ray_loss [B] (the reference value is
 * its mean over rays); if g_ray [B] is given also d_w [B,N] = g_ray[b] * d ray_loss[b] / d w. */
int mipnerf_distloss(int64_t num_rays, int32_t num_samples, const float* weights,
                     const float* t_samples, float* ray_loss, const float* g_ray, float* d_w,
                     void* stream);

/* ---- gradient through the resampler: MipNerf(stop_resample_grad=False) (mip.py:265-279, mip_nerf.py:204-214) ----
 * With the flag off the fine level's fence posts stay in the autograd graph; these are the extra backward pieces
 * (fp32 parity mode): compositing and distloss also return dL/dt_samples [B, N+1]; the MLP backward returns the gradient
 * w.r.t. its input encoding; cast_rays + integrated_pos_enc and the PDF resampler get their backward. */
int mipnerf_volumetric_rendering_bwd_t(int64_t num_rays, int32_t num_samples, const float* rgb_sigma,
                                       const float* t_samples, const float* directions, int32_t white_bkgd,
                                       const float* g_rgb, const float* g_dist, const float* g_acc, const float* g_w,
                                       float rgb_padding, float* d_raw, float* d_t, void* stream);
int mipnerf_distloss_bwd(int64_t num_rays, int32_t num_samples, const float* weights, const float* t_samples,
                         const float* g_ray, float* d_w, float* d_t, void* stream);
/* d_t [B, N+1] += dL/dt from d_enc [B*N, 6*(max_deg-min_deg)] fp32 (d_t zeroed or holding earlier contributions). */
int mipnerf_cast_ipe_bwd(int64_t num_rays, int32_t num_samples, int32_t min_deg, int32_t max_deg,
                         int32_t disable_integration, const float* t_samples, const float* origins,
                         const float* directions, const float* radii, const float* d_enc, float* d_t, void* stream);
/* d_weights [B, N] of mipnerf_resample_along_rays for d_t_new [B, N+1]; same u_rand (or NULL) as the forward. */
int mipnerf_resample_along_rays_bwd(int64_t num_rays, int32_t num_samples, const float* t_samples, const float* weights,
                                    const float* u_rand, float resample_padding, const float* d_t_new,
                                    float* d_weights, void* stream);

/* ---- native MLP training step (bf16 MFMA kernels; what torch autograd does to mip_nerf.py:75-111) ----
 * mipnerf_mlp_forward_train = mipnerf_mlp_forward (bf16) that also saves, per 32-sample wave tile, the
 * transposed activations of every layer input (`act`) and the ReLU bit masks (`masks`).
 * mipnerf_mlp_backward: d_raw [M,4] = dL/d(raw_rgb, raw_density) -> grad_flat [612,740] fp32, the gradients
 * of the 24 parameter tensors concatenated in state_dict order (accumulate = 0: overwritten; 1: added to).  `delta` and
 * `partials` are scratch.  Buffer sizes for M samples come from mipnerf_mlp_train_sizes. */
int mipnerf_mlp_train_sizes(const mipnerf_ctx* ctx, int64_t num_points, size_t* act_bytes,
                            size_t* mask_bytes, size_t* delta_bytes, size_t* partial_bytes);
/* `enc`: bf16, row-major [num_points, xyz_dim].  LIFETIME (two-kernel variants, i.e. contexts with unbounded = 1): their weight-gradient
 * jobs read the ENCODING ITSELF -- `act` ends in a record of the `enc` pointer -- so `enc` must stay allocated and unmodified until the
 * mipnerf_mlp_backward / mipnerf_mlp_wgrad call that consumes this `act` has been issued on the same stream; the standard shapes transpose
 * their 96 features into `act` and do not look at `enc` again. */
int mipnerf_mlp_forward_train(mipnerf_ctx* ctx, int64_t num_points, int32_t num_samples,
                              const void* enc, const void* viewenc, float* rgb_sigma, float* raw,
                              void* act, void* masks, void* stream);
/* The same with `enc` in the MFMA-fragment layout mipnerf_cast_ipe_360 writes for MIPNERF_OUT_BF16_FRAGMENTS (whole 256-sample tiles;
 * k_pre_gemm and the weight-gradient jobs read it lane-linearly).  Two-kernel variants only: MIPNERF_E_UNSUPPORTED for every other
 * context (a fragment buffer must never be read as rows).  Same lifetime rule for `enc`.  (ABI 6: replaces the per-context option 6.) */
int mipnerf_mlp_forward_train_fragments(mipnerf_ctx* ctx, int64_t num_points, int32_t num_samples,
                                        const void* enc, const void* viewenc, float* rgb_sigma, float* raw,
                                        void* act, void* masks, void* stream);
int mipnerf_mlp_backward(mipnerf_ctx* ctx, int64_t num_points, const float* d_raw, const void* act,
                         const void* masks, void* delta, float* partials, float* grad_flat,
                         int32_t accumulate, void* stream);
/* The two halves of mipnerf_mlp_backward, separately testable / timeable: delta chain (writes `delta`), and
 * weight gradients (reads act + delta; grad_flat may be NULL = leave the fp32 partials unreduced). */
int mipnerf_mlp_dgrad(mipnerf_ctx* ctx, int64_t num_points, const float* d_raw, const void* masks,
                      void* delta, void* stream);
int mipnerf_mlp_wgrad(mipnerf_ctx* ctx, int64_t num_points, const void* act, const void* delta,
                      float* partials, float* grad_flat, int32_t accumulate, void* stream);
/* torch.optim.Adam.step() of nerf_system.py:71-72 (betas, eps as given; no weight decay / amsgrad) over ONE flat
 * buffer of n parameters: param, grad, exp_avg, exp_avg_sq [n] fp32; `step` = 1-based step count.  The hyper-parameters are the
 * doubles torch holds (ABI 4; floats before): bias corrections, lr / (1 - beta1^t) and 1 - beta are formed in double. */
int mipnerf_adam_step(int64_t n, float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                      double lr, double beta1, double beta2, double eps, int32_t step, void* stream);
/* Tuning: workgroups per weight-gradient job (HOST array, one entry per job of the context's architecture: 12 for the shipped MLP;
 * 0 skips a job, for timing only).  NULL restores the default (workgroups ~ the 2-KiB blocks a job moves per stage + 4, all CUs
 * handed out).  Changes partial_bytes of mipnerf_mlp_train_sizes; synchronises. */
int mipnerf_set_wgrad_splits(mipnerf_ctx* ctx, const int32_t* splits_host);

/* ---- parity-mode (fp32) MLP training: the fused fp32 forward also writes every layer output into `save`
 * (mipnerf_mlp_train_f32_bytes), the backward is dgrad / wgrad GEMMs on v_mfma_f32_32x32x2_f32 (exact fp32
 * products, fp32 accumulation).  enc [M,96] and viewenc [B,32] are fp32.  Correctness-first. */
size_t mipnerf_mlp_train_f32_bytes(const mipnerf_ctx* ctx, int64_t num_points, size_t* save_bytes,
                                   size_t* workspace_bytes);
int mipnerf_mlp_forward_train_f32(mipnerf_ctx* ctx, int64_t num_points, int32_t num_samples, const float* enc,
                                  const float* viewenc, float* rgb_sigma, float* raw, float* save,
                                  void* stream);
int mipnerf_mlp_backward_f32(mipnerf_ctx* ctx, int64_t num_points, int32_t num_samples, const float* d_raw,
                             const float* enc, const float* viewenc, const float* save, void* workspace,
                             float* grad_flat, int32_t accumulate, void* stream);
/* The same plus d_enc [num_points, xyz_dim] = dL/d(encoding) (needed only with stop_resample_grad=False). */
int mipnerf_mlp_backward_f32_enc(mipnerf_ctx* ctx, int64_t num_points, int32_t num_samples, const float* d_raw,
                                 const float* enc, const float* viewenc, const float* save, void* workspace,
                                 float* grad_flat, int32_t accumulate, float* d_enc, void* stream);

/* ---- optimiser step with the LR schedule on the device (graph-capturable: no per-step host scalars) ------------------
 * torch.optim.Adam(lr) + MipLRDecay of the reference (nerf_system.py:70-76, utils/lr_schedule.py:51-59).
 * *step_count (device int64, starts at 0) is incremented to t; the step runs with lr = MipLRDecay(last_epoch = t - 1)
 * (constant_lr > 0 overrides the schedule), bias corrections of step t, and grad * grad_scale (1 / world_size after a SUM
 * all-reduce).  hyper_out (device float[4]) receives lr, lr/(1-beta1^t), sqrt(1-beta2^t), grad_scale (the `lr` that
 * nerf_system.py:117 logs). */
typedef struct mipnerf_lr_schedule {
    double lr_init, lr_final, lr_delay_mult, constant_lr;
    int64_t max_steps, lr_delay_steps;
    double beta1, beta2, eps;
    float grad_scale;
    int32_t reserved;
} mipnerf_lr_schedule;
int mipnerf_adam_step_scheduled(int64_t n, float* param, const float* grad, float* exp_avg, float* exp_avg_sq,
                                const mipnerf_lr_schedule* schedule, int64_t* step_count, float* hyper_out,
                                void* stream);

/* ---- the whole training step (bf16): MipNeRFSystem.training_step (nerf_system.py:95-111) + loss.backward() --------
 * forward of all levels with saved activations, loss = cm (mse_c + dm dl_c) + mse_f + dm dl_f (cm = loss.coarse_loss_mult,
 * dm = 0.01, mse masked by rays.lossmult unless disable_multiscale_loss), backward of compositing / activations / MLP.
 * grad_flat [612,740] = d loss / d parameters in state_dict order (accumulate = 0 overwrites).  out_scalars [6] =
 * loss, mse_coarse, mse_fine, distloss_coarse, distloss_fine, psnr_fine.  `out` (may be NULL, or hold NULL fields)
 * receives copies of what MipNerf.forward returns.  No autograd graph, no allocation, one stream: graph-capturable.
 * Every variant with bf16 training kernels, including (round 5) the unbounded-scene model's two-kernel form: inverse-depth
 * fence posts, encodings as fragments, one weight-gradient launch per level; grad_flat then has that variant's numel. */
size_t mipnerf_train_workspace_bytes(const mipnerf_ctx* ctx, int64_t num_rays);
int mipnerf_train_step(mipnerf_ctx* ctx, int64_t num_rays, const mipnerf_rays* rays, const float* gt_rgb,
                       const float* t_rand, const float* u_rand, const float* density_randn, uint32_t flags,
                       float coarse_loss_mult,
                       float distloss_mult, int32_t disable_multiscale_loss, void* workspace,
                       size_t workspace_bytes, float* grad_flat, int32_t accumulate, float* out_scalars,
                       const mipnerf_level_out* out, void* stream);

/* ---- the fused per-ray launches as stage entry points (ABI 6 grows; nothing above changes) ----
 * What mipnerf_forward (option 4) and mipnerf_train_step run behind the MLP of a level, on the caller's rays: one launch each, the same
 * per-ray device functions as the stand-alone entry points, so the same bits.  Inputs and the four compositing outputs as
 * mipnerf_volumetric_rendering (all four required).  mipnerf_composite_resample then draws t_new [B, N+1] as
 * mipnerf_resample_along_rays does from those weights, inverting over `bins` [B, N+1] (t_samples itself for a bounded scene) with
 * u_rand [B, N+1] or NULL.  mipnerf_composite_train also writes ray_loss [B] and d_w [B, N] = g_const * d ray_loss / d w as
 * mipnerf_distloss does with g_ray[b] = g_const; t_new = NULL is a last level (no resampling: u_rand, resample_padding and bins are not
 * read), bins = NULL inverts over t_samples.  num_samples > MIPNERF_MAX_SAMPLES is MIPNERF_E_INVALID before anything is launched. */
int mipnerf_composite_resample(int64_t num_rays, int32_t num_samples, const float* rgb_sigma, const float* t_samples,
                               const float* directions, int32_t white_bkgd, float* comp_rgb, float* distance, float* acc,
                               float* weights, const float* bins, const float* u_rand, float resample_padding, float* t_new,
                               void* stream);
int mipnerf_composite_train(int64_t num_rays, int32_t num_samples, const float* rgb_sigma, const float* t_samples,
                            const float* directions, int32_t white_bkgd, float* comp_rgb, float* distance, float* acc,
                            float* weights, float* ray_loss, float g_const, float* d_w, const float* u_rand, float resample_padding,
                            float* t_new /* NULL: last level */, const float* bins /* NULL: t_samples */, void* stream);

/* ---- instrumentation ------------------------------------------------------------------ */
/* Times `iters` launches of the bf16 MLP kernel with hipEvents on `stream`; returns the
 * average milliseconds per launch in *ms (used by bench.py for roofline.achieved). */
int mipnerf_time_mlp(mipnerf_ctx* ctx, int64_t num_points, int32_t num_samples, const void* enc,
                     const void* viewenc, int precision, float* rgb_sigma, int iters, float* ms,
                     void* stream);
/* Hardware self-test of the MFMA fragment layouts and the LDS-DMA path the kernels rely
 * on; returns 0 when the device behaves as the kernels assume (message in
 * mipnerf_last_error() either way). */
int mipnerf_selftest(void* stream);
/* Tuning / debug knobs.  option 0: bf16 MLP weight staging (1 = global_load_lds ring
 * [default], 0 = register-staged ring, same schedule); option 1: persistent grid size of the
 * bf16 MLP kernel (default = number of CUs); option 2: 1 = record a HIP event pair around
 * every MLP launch issued by mipnerf_forward, 2 = around every weight-gradient launch (read with
 * mipnerf_mlp_launch_stats); option 3: 1 [default] = the bf16
 * MLP kernel of mipnerf_forward computes the integrated positional encoding itself (no [M,96] buffer, no k_cast_ipe
 * launch), 0 = separate mipnerf_cast_ipe + encoding buffer (same bits); option 4: 1 [default] = mipnerf_forward runs pos_enc + the
 * coarse fence posts as ONE launch and the coarse level's compositing + the fine level's resampling as ONE launch (N <= 128 or 192 < N <= 256; the
 * weights go from registers to the sampler's LDS row), 0 = one launch per stage (same bits); option 5: 1 [default] = fp32 inference (mipnerf_mlp_forward,
 * mipnerf_forward) runs the register-resident kernel k_mlp_f32r where one was generated for the architecture (widths <= 256), 0 = the LDS-resident
 * k_mlp_f32 (same function, another summation order: results agree to fp32 rounding); option 6 (ABI 6, round 6): 1 [default] = the bf16 forward of an
 * unbounded = 1 context (mipnerf_forward) runs as ONE MLP kernel per level -- layer 0 and the skip layer as k-step-major ops of the trunk kernel, the 672-wide encoding
 * streamed through a wave-private LDS ring --, 0 = k_pre_gemm + trunk kernel with their 1.5-KiB-per-sample hand-off through HBM (same bits). */
int mipnerf_set_option(mipnerf_ctx* ctx, int option, int value);
/* Sum of the elapsed times (ms) and the number of MLP launches recorded since the last call
 * (option 2); synchronises on the recorded events. */
int mipnerf_mlp_launch_stats(mipnerf_ctx* ctx, double* total_ms, int64_t* launches);
/* Host-only exports of the static plan tables (no GPU needed), used by the CPU tests to
 * prove that the tables the library expands from its embedded chunk records (mlp_plan.blob) equal mipnerf_pl_amd/mlp_plan.py.  which: 0 = bf16 stream
 * pack table, 1 = bias table, 2 = fp32 stream pack table (flat parameter indices, -1 = 0) of Plan.build(),
 * 3 = dgrad (W^T) stream pack table, 4 = wgrad partial -> parameter index table, 5 = wgrad job table,
 * 6 = pack table and 7 = bias table of the stream the bf16 forward kernels read (Plan.build(fold_view=True): the bottleneck
 * folded into view layer 0; indices at or past the parameter count address the derived tensors that follow the parameters).
 * Return the element count; copy only when cap is large enough. */
int64_t mipnerf_debug_table_variant(int variant, int which, int32_t* out_host, int64_t cap);   /* which: 0 bf16 pack, 1 bias, 2 fp32 pack, 6 / 7 forward pack / bias */
int64_t mipnerf_debug_table(int which, int32_t* out_host, int64_t cap);
int64_t mipnerf_debug_f32net(int32_t* out_host, int64_t cap);

#ifdef __cplusplus
}
#endif
#endif /* MIPNERF_HIP_H */
