"""ctypes binding of libmipnerf_hip.so (the C ABI declared in include/mipnerf_hip.h).

The library is built in-tree by `python -m mipnerf_pl_amd.build` (hipcc --offload-arch=gfx950).
There is no CPU fallback: if the shared object is missing, loading fails loudly."""
from __future__ import annotations

import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MIPNERF_LIB", os.path.join(HERE, "csrc", "libmipnerf_hip.so"))   # override: A/B builds

OK, E_INVALID, E_UNSUPPORTED, E_HIP, E_WORKSPACE = 0, 1, 2, 3, 4
PREC_FP32, PREC_BF16 = 0, 1
OUT_BF16_FRAGMENTS = 2      # out_dtype of mipnerf_cast_ipe_360 only (include/mipnerf_hip.h)
SPACE_WORLD, SPACE_CONTRACTED = 0, 1   # lattice spaces of the unbounded-scene model (include/mipnerf_hip.h)
SPACES = {"world": SPACE_WORLD, "contracted": SPACE_CONTRACTED}
FLAG_WHITE_BKGD, FLAG_DISPARITY = 1, 2
NUM_PARAM_TENSORS = 24
MAX_SAMPLES = 1024
MAX_PYRAMID_LEVELS = 8
MAX_DOWNSCALE_FACTOR = 16


class Config(C.Structure):
    _fields_ = [(n, C.c_int32) for n in (
        "num_samples", "num_levels", "min_deg_point", "max_deg_point", "deg_view", "use_viewdirs",
        "disparity", "disable_integration", "net_depth", "net_width", "net_depth_condition",
        "net_width_condition", "skip_index", "num_rgb_channels", "num_density_channels")] + [
        ("resample_padding", C.c_float), ("density_bias", C.c_float), ("rgb_padding", C.c_float),
        ("density_noise", C.c_float), ("unbounded", C.c_int32)]


class RaysPtrs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in
                ("origins", "directions", "viewdirs", "radii", "lossmult", "near", "far")]


class LrSchedule(C.Structure):
    _fields_ = [("lr_init", C.c_double), ("lr_final", C.c_double), ("lr_delay_mult", C.c_double), ("constant_lr", C.c_double),
                ("max_steps", C.c_int64), ("lr_delay_steps", C.c_int64), ("beta1", C.c_double), ("beta2", C.c_double),
                ("eps", C.c_double), ("grad_scale", C.c_float), ("reserved", C.c_int32)]


class LevelOut(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("comp_rgb", "distance", "acc", "weights", "t_samples")]


_P, _I32, _I64, _F, _SZ = C.c_void_p, C.c_int32, C.c_int64, C.c_float, C.c_size_t

# name -> (restype, argtypes); every symbol include/mipnerf_hip.h declares
SIGNATURES = {
    "mipnerf_last_error": (C.c_char_p, []),
    "mipnerf_abi_version": (C.c_int, []),
    "mipnerf_num_param_tensors": (C.c_int, [_P]),
    "mipnerf_create": (C.c_int, [C.POINTER(Config), C.POINTER(_P)]),
    "mipnerf_destroy": (C.c_int, [_P]),
    "mipnerf_compiled_arch": (C.c_int, [C.POINTER(Config)]),
    "mipnerf_num_variants": (C.c_int, []),
    "mipnerf_variant_arch": (C.c_int, [C.c_int, C.POINTER(Config), C.POINTER(C.c_int)]),
    "mipnerf_set_params": (C.c_int, [_P, C.POINTER(_P), _P]),
    "mipnerf_workspace_bytes": (_SZ, [_P, _I64]),
    "mipnerf_forward": (C.c_int, [_P, _I64, C.POINTER(RaysPtrs), _P, _P, _P, C.c_uint32, C.c_int, _P, _SZ,
                                  C.POINTER(LevelOut), _P]),
    "mipnerf_sample_along_rays": (C.c_int, [_I64, _I32, _P, _P, _P, _I32, _P, _P]),
    "mipnerf_cast_rays": (C.c_int, [_I64, _I32, _P, _P, _P, _P, _P, _P, _P]),
    "mipnerf_cast_ipe": (C.c_int, [_I64, _I32, _I32, _I32, _I32, _P, _P, _P, _P, _P, C.c_int, _P]),
    "mipnerf_integrated_pos_enc": (C.c_int, [_I64, _I32, _I32, _P, _P, _P, C.c_int, _P]),
    "mipnerf_pos_enc": (C.c_int, [_I64, _I32, _P, _P, _I32, C.c_int, _P]),
    "mipnerf_mlp_forward": (C.c_int, [_P, _I64, _I32, _P, _P, C.c_int, _P, _P, _P]),
    "mipnerf_volumetric_rendering": (C.c_int, [_I64, _I32, _P, _P, _P, _I32, _P, _P, _P, _P, _P]),
    "mipnerf_resample_along_rays": (C.c_int, [_I64, _I32, _P, _P, _P, _F, _P, _P]),
    "mipnerf_sorted_piecewise_constant_pdf": (C.c_int, [_I64, _I32, _P, _P, _I32, _P, _P, _P]),
    "mipnerf_sample_along_rays_360": (C.c_int, [_I64, _I32, _P, _P, _P, _P, _P, _P]),
    "mipnerf_cast_ipe_360": (C.c_int, [_I64, _I32, _I32, _I32, _I32, _P, _P, _P, _P, _P, C.c_int, _P, _P, _P]),
    "mipnerf_gauss_360": (C.c_int, [_I64, _I32, _I32, _I32, _P, _P, _P, C.c_int, _P, _P, _P]),
    "mipnerf_num_camera_modes": (C.c_int, []),
    "mipnerf_generate_rays": (C.c_int, [_I64, _P, _P, _P, C.POINTER(RaysPtrs), _P]),
    "mipnerf_generate_rays_f64": (C.c_int, [_I64, _P, _P, _P, C.POINTER(RaysPtrs), _P]),
    "mipnerf_gather_train_batch": (C.c_int, [_I64, _I64, _P, _I32, _P, _P, _P, _P, _P, C.POINTER(RaysPtrs), _P, _P]),
    "mipnerf_eval_workspace_floats": (_I64, [_I32, _I32]),
    "mipnerf_eval_errors": (C.c_int, [_I32, _I32, _P, _P, _P, _P, _P]),
    "mipnerf_visualize_workspace_floats": (_I64, [_I64]),
    "mipnerf_visualize_map": (C.c_int, [_I64, _P, _P, _P, _P]),
    "mipnerf_image_to_u8": (C.c_int, [_I64, _P, _P, _P]),
    "mipnerf_box_pyramid": (C.c_int, [_I32, _I32, _I32, _I32, _P, _P, _P, _I64, _I32, _P, _P]),
    "mipnerf_area_downscale": (C.c_int, [_I32, _I32, _I32, _I32, _I32, _P, _P, _I64, _P]),
    "mipnerf_density_grid_workspace_bytes": (_SZ, [_P, _I64, C.c_int]),
    "mipnerf_density_grid": (C.c_int, [_P, C.POINTER(_I32), C.POINTER(_F), C.POINTER(_F), _F, C.c_int, _P, _P, _SZ, _P]),
    "mipnerf_lattice_density": (C.c_int, [C.POINTER(_I32), C.POINTER(_F), C.POINTER(_F), _P, _I64, _I32, _P, _P, _P, _P, _P, _P]),
    "mipnerf_forward_proposal": (C.c_int, [_P, _I64, C.POINTER(RaysPtrs), C.POINTER(_I32), C.POINTER(_F), C.POINTER(_F), _P, _P, _P,
                                           C.c_uint32, C.c_int, _P, _SZ, C.POINTER(LevelOut), _P]),
    "mipnerf_density_grid_360_workspace_bytes":(_SZ, [_P, _I64, C.c_int]),
    "mipnerf_density_grid_360": (C.c_int, [_P, C.POINTER(_I32), C.POINTER(_F), C.POINTER(_F), _F, C.c_int, _F, C.c_int, _P, _P, _SZ, _P]),
    "mipnerf_lattice_ipe_360": (C.c_int, [C.POINTER(_I32), C.POINTER(_F), C.POINTER(_F), _I64, _I64, _F, C.c_int, _I32, _I32, _P, C.c_int, _P]),
    "mipnerf_uncontract_vertices": (C.c_int, [_I64, _F, _P, _P, _P, _P, _P]),
    "mipnerf_isosurface_workspace_bytes": (_SZ, [_I32, _I32, _I32]),
    "mipnerf_isosurface_count": (C.c_int, [C.POINTER(_I32), _P, _F, _P, _SZ, C.POINTER(_I64), C.POINTER(_I64), _P]),
    "mipnerf_isosurface_emit": (C.c_int, [C.POINTER(_I32), C.POINTER(_F), C.POINTER(_F), _P, _F, _P, _SZ, _P, _P, _P, _P, _P]),
    "mipnerf_occupancy_words": (_I64, [_I32, _I32, _I32]),
    "mipnerf_occupancy_build": (C.c_int, [C.POINTER(_I32), _P, _F, _I32, _P, _P, _P]),
    "mipnerf_occupancy_refresh": (C.c_int, [C.POINTER(_I32), _P, _P, _F, _F, _I32, _P, _P, _P]),
    "mipnerf_ray_occupancy": (C.c_int, [C.POINTER(_I32), C.POINTER(_F), C.POINTER(_F), _P, _I64, _I32, C.POINTER(RaysPtrs), _I32, _I32, _F,
                                        _P, _P]),
    "mipnerf_ray_span": (C.c_int, [C.POINTER(_I32), C.POINTER(_F), C.POINTER(_F), _P, _I64, _I32, C.POINTER(RaysPtrs), _I32, _I32, _F,
                                   _P, _P, _P, _P, _P, _P]),
    "mipnerf_ray_occupancy_360": (C.c_int, [C.POINTER(_I32), C.POINTER(_F), C.POINTER(_F), _P, _I64, _I32, C.POINTER(RaysPtrs), _I32, _F, _P, _P]),
    "mipnerf_ray_span_360": (C.c_int, [C.POINTER(_I32), C.POINTER(_F), C.POINTER(_F), _P, _I64, _I32, C.POINTER(RaysPtrs), _I32, _F,
                                       _P, _P, _P, _P, _P, _P]),
    "mipnerf_compact_rays_workspace_bytes": (_SZ, [_I64]),
    "mipnerf_compact_rays": (C.c_int, [_I64, _P, C.POINTER(RaysPtrs), C.POINTER(RaysPtrs), _P, _P, _SZ, C.POINTER(_I64), _P]),
    "mipnerf_scatter_frame": (C.c_int, [_I64, _I64, _I32, _P, _P, _P, _I32, C.POINTER(LevelOut), C.POINTER(LevelOut), _P]),
    "mipnerf_bucket_rays_workspace_bytes": (_SZ, [_I64, _I32]),
    "mipnerf_bucket_rays": (C.c_int, [_I64, _P, _P, _P, _I32, _I32, _I32, C.POINTER(_I32), C.POINTER(RaysPtrs), C.POINTER(RaysPtrs), _P, _P, _SZ,
                                      C.POINTER(_I64), _P]),
    "mipnerf_gather_frame": (C.c_int, [_I64, _I64, _I32, _P, _P, _I32, C.POINTER(LevelOut), C.POINTER(LevelOut), _P]),
    "mipnerf_guided_apply": (C.c_int, [_I64, _I64, _I64, _P, _P, _P, _I64, _P, _P]),
    "mipnerf_guided_accumulate": (C.c_int, [_I64, _I64, _I64, _P, _I64, _P, _P, _I64, _P, _P, _P, _P, _P]),
    "mipnerf_guided_refresh": (C.c_int, [_I32, _P, _I32, _I64, _F, C.c_double, _P, _P, _P, _P, _P, _P, _P, _SZ, _P, _P]),
    "mipnerf_guided_draw": (C.c_int, [_I64, _P, _I32, _P, _I32, _I64, _P, _P, _P, _P, _P, _I64, _I64, _P]),
    "mipnerf_activate": (C.c_int, [_I64, _P, _F, _F, _P, _F, _P, _P]),
    "mipnerf_volumetric_rendering_bwd": (C.c_int, [_I64, _I32, _P, _P, _P, _I32, _P, _P, _P, _P, _F, _P, _P]),
    "mipnerf_distloss": (C.c_int, [_I64, _I32, _P, _P, _P, _P, _P, _P]),
    "mipnerf_volumetric_rendering_bwd_t": (C.c_int, [_I64, _I32, _P, _P, _P, _I32, _P, _P, _P, _P, _F, _P, _P, _P]),
    "mipnerf_distloss_bwd": (C.c_int, [_I64, _I32, _P, _P, _P, _P, _P, _P]),
    "mipnerf_cast_ipe_bwd": (C.c_int, [_I64, _I32, _I32, _I32, _I32, _P, _P, _P, _P, _P, _P, _P]),
    "mipnerf_resample_along_rays_bwd": (C.c_int, [_I64, _I32, _P, _P, _P, _F, _P, _P, _P]),
    "mipnerf_mlp_train_sizes": (C.c_int, [_P, _I64, C.POINTER(_SZ), C.POINTER(_SZ), C.POINTER(_SZ), C.POINTER(_SZ)]),
    "mipnerf_mlp_forward_train": (C.c_int, [_P, _I64, _I32, _P, _P, _P, _P, _P, _P, _P]),
    "mipnerf_mlp_forward_train_fragments": (C.c_int, [_P, _I64, _I32, _P, _P, _P, _P, _P, _P, _P]),
    "mipnerf_mlp_backward": (C.c_int, [_P, _I64, _P, _P, _P, _P, _P, _P, _I32, _P]),
    "mipnerf_adam_step": (C.c_int, [_I64, _P, _P, _P, _P, C.c_double, C.c_double, C.c_double, C.c_double, _I32, _P]),
    "mipnerf_adam_step_scheduled": (C.c_int, [_I64, _P, _P, _P, _P, C.POINTER(LrSchedule), _P, _P, _P]),
    "mipnerf_mlp_dgrad": (C.c_int, [_P, _I64, _P, _P, _P, _P]),
    "mipnerf_mlp_wgrad": (C.c_int, [_P, _I64, _P, _P, _P, _P, _I32, _P]),
    "mipnerf_set_wgrad_splits": (C.c_int, [_P, _P]),
    "mipnerf_mlp_train_f32_bytes": (_SZ, [_P, _I64, C.POINTER(_SZ), C.POINTER(_SZ)]),
    "mipnerf_mlp_forward_train_f32": (C.c_int, [_P, _I64, _I32, _P, _P, _P, _P, _P, _P]),
    "mipnerf_mlp_backward_f32": (C.c_int, [_P, _I64, _I32, _P, _P, _P, _P, _P, _P, _I32, _P]),
    "mipnerf_mlp_backward_f32_enc": (C.c_int, [_P, _I64, _I32, _P, _P, _P, _P, _P, _P, _I32, _P, _P]),
    "mipnerf_train_workspace_bytes": (_SZ, [_P, _I64]),
    "mipnerf_train_step": (C.c_int, [_P, _I64, C.POINTER(RaysPtrs), _P, _P, _P, _P, C.c_uint32, _F, _F, _I32, _P, _SZ, _P, _I32, _P,
                                     C.POINTER(LevelOut), _P]),
    "mipnerf_composite_resample": (C.c_int, [_I64, _I32, _P, _P, _P, _I32, _P, _P, _P, _P, _P, _P, _F, _P, _P]),
    "mipnerf_composite_train": (C.c_int, [_I64, _I32, _P, _P, _P, _I32, _P, _P, _P, _P, _P, _F, _P, _P, _F, _P, _P, _P]),
    "mipnerf_time_mlp": (C.c_int, [_P, _I64, _I32, _P, _P, C.c_int, _P, C.c_int, C.POINTER(_F), _P]),
    "mipnerf_selftest": (C.c_int, [_P]),
    "mipnerf_set_option": (C.c_int, [_P, C.c_int, C.c_int]),
    "mipnerf_mlp_launch_stats": (C.c_int, [_P, C.POINTER(C.c_double), C.POINTER(_I64)]),
    "mipnerf_debug_table": (_I64, [C.c_int, _P, _I64]),
    "mipnerf_debug_table_variant": (_I64, [C.c_int, C.c_int, _P, _I64]),
    "mipnerf_debug_f32net": (_I64, [_P, _I64]),
}

# include/mipnerf_diag.h: measurement tooling in its own library (bench.py, scripts/handoff_probe.py); never needed by the product path
DIAG_LIB_PATH = os.environ.get("MIPNERF_DIAG_LIB", os.path.join(HERE, "csrc", "libmipnerf_diag.so"))
DIAG_SIGNATURES = {
    "mipnerf_diag_last_error": (C.c_char_p, []),
    "mipnerf_mfma_ceiling": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_double, C.POINTER(C.c_double), _P]),
    "mipnerf_handoff_probe": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), _P]),
}


# include/mipnerf_preview.h: the baked-lattice preview renderer in its own library (mipnerf_pl_amd.preview); the drop-in library keeps
# its ABI version and its entry points
PREVIEW_LIB_PATH = os.environ.get("MIPNERF_PREVIEW_LIB", os.path.join(HERE, "csrc", "libmipnerf_preview.so"))
PREVIEW_ABI = 1


class PreviewField(C.Structure):
    _fields_ = [("dims", _I32 * 3), ("lo", _F * 3), ("hi", _F * 3), ("degree", _I32), ("rows", _P), ("occupancy", _P)]


class PreviewParams(C.Structure):
    _fields_ = [("step_scale", _F), ("t_min", _F), ("max_steps", _I32), ("background", _F * 3)]


PREVIEW_SIGNATURES = {
    "mipnerf_preview_abi_version": (C.c_int, []),
    "mipnerf_preview_last_error": (C.c_char_p, []),
    "mipnerf_preview_pack": (C.c_int, [C.POINTER(_I32), _I32, _P, _P, _P, _P, _P]),
    "mipnerf_preview_march": (C.c_int, [C.POINTER(PreviewField), C.POINTER(PreviewParams), _I64, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
}

# include/mipnerf_preview_mip.h: the preview over a cone-radius pyramid of lattices, in a fourth library; the preview library keeps its
# ABI version and its entry points
PREVIEW_MIP_LIB_PATH = os.environ.get("MIPNERF_PREVIEW_MIP_LIB", os.path.join(HERE, "csrc", "libmipnerf_preview_mip.so"))
PREVIEW_MIP_ABI = 1
PREVIEW_MIP_MAX_LEVELS = 8


class PreviewPyramid(C.Structure):
    _fields_ = [("levels", _I32), ("level", PreviewField * PREVIEW_MIP_MAX_LEVELS)]


PREVIEW_MIP_SIGNATURES = {
    "mipnerf_preview_mip_abi_version": (C.c_int, []),
    "mipnerf_preview_mip_last_error": (C.c_char_p, []),
    "mipnerf_preview_mip_march": (C.c_int, [C.POINTER(PreviewPyramid), C.POINTER(PreviewParams), _F, _I64, _P, _P, _P, _P, _P, _P, _P, _P, _P,
                                            _P, _P]),
}

# include/mipnerf_preview_sparse.h: the preview over lattices that store only the rows next to an occupied cell, in a fifth library; the
# other two preview libraries keep their ABI versions and their entry points
PREVIEW_SPARSE_LIB_PATH = os.environ.get("MIPNERF_PREVIEW_SPARSE_LIB", os.path.join(HERE, "csrc", "libmipnerf_preview_sparse.so"))
PREVIEW_SPARSE_ABI = 1


class PreviewSparseField(C.Structure):
    _fields_ = [("field", PreviewField), ("table", _P), ("n_rows", _I64)]


class PreviewSparsePyramid(C.Structure):
    _fields_ = [("levels", _I32), ("level", PreviewSparseField * PREVIEW_MIP_MAX_LEVELS)]


PREVIEW_SPARSE_SIGNATURES = {
    "mipnerf_preview_sparse_abi_version": (C.c_int, []),
    "mipnerf_preview_sparse_last_error": (C.c_char_p, []),
    "mipnerf_preview_sparse_scratch_bytes": (_SZ, [C.POINTER(_I32)]),
    "mipnerf_preview_sparse_index": (C.c_int, [C.POINTER(_I32), _P, _P, _P, _P, _P]),
    "mipnerf_preview_sparse_gather": (C.c_int, [C.POINTER(_I32), _I32, _P, _P, _P, _P]),
    "mipnerf_preview_sparse_pack": (C.c_int, [_I64, _I32, _P, _P, _P, _P]),
    "mipnerf_preview_sparse_march": (C.c_int, [C.POINTER(PreviewSparsePyramid), C.POINTER(PreviewParams), _F, _I64, _P, _P, _P, _P, _P, _P, _P,
                                               _P, _P, _P, _P]),
}

# include/mipnerf_preview_tune.h: the gradient of the single-lattice march with respect to the rows and an Adam step on them, in a sixth
# library; the three preview libraries keep their ABI versions and their entry points
PREVIEW_TUNE_LIB_PATH = os.environ.get("MIPNERF_PREVIEW_TUNE_LIB", os.path.join(HERE, "csrc", "libmipnerf_preview_tune.so"))
PREVIEW_TUNE_ABI = 1
PREVIEW_TUNE_SIGNATURES = {
    "mipnerf_preview_tune_abi_version": (C.c_int, []),
    "mipnerf_preview_tune_last_error": (C.c_char_p, []),
    "mipnerf_preview_tune_grad": (C.c_int, [C.POINTER(PreviewField), C.POINTER(PreviewParams), _I64, _P, _P, _P, _P, _P, _P, _F, _P, _P, _P, _P,
                                            _P, _P]),
    "mipnerf_preview_tune_adam": (C.c_int, [_I64, _I32, _P, _P, _P, _P, _P, _P, _F, _F, _F, _F, _F, _F, _F, _P]),
}

# include/mipnerf_preview_360.h: the preview of the unbounded-scene model, a lattice over the contracted space marched along world rays, in
# a seventh library; the four preview libraries keep their ABI versions and their entry points
PREVIEW_360_LIB_PATH = os.environ.get("MIPNERF_PREVIEW_360_LIB", os.path.join(HERE, "csrc", "libmipnerf_preview_360.so"))
PREVIEW_360_ABI = 1
PREVIEW_360_SIGNATURES = {
    "mipnerf_preview_360_abi_version": (C.c_int, []),
    "mipnerf_preview_360_last_error": (C.c_char_p, []),
    "mipnerf_preview_360_march": (C.c_int, [C.POINTER(PreviewField), _F, C.POINTER(PreviewParams), _I64, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "mipnerf_preview_360_march_sparse": (C.c_int, [C.POINTER(PreviewSparseField), _F, C.POINTER(PreviewParams), _I64, _P, _P, _P, _P, _P, _P,
                                                   _P, _P, _P]),
}

# include/mipnerf_preview_reg.h: the gradient of a total-variation term and of an SH decay on the tuned lattice's fp32 master rows, in an
# eighth library; the five preview libraries keep their ABI versions and their entry points
PREVIEW_REG_LIB_PATH = os.environ.get("MIPNERF_PREVIEW_REG_LIB", os.path.join(HERE, "csrc", "libmipnerf_preview_reg.so"))
PREVIEW_REG_ABI = 1
PREVIEW_REG_SIGNATURES = {
    "mipnerf_preview_reg_abi_version": (C.c_int, []),
    "mipnerf_preview_reg_last_error": (C.c_char_p, []),
    "mipnerf_preview_reg_grad": (C.c_int, [C.POINTER(_I32), _I32, C.POINTER(_F), _P, _P, _P, _F, _F, _F, _F, _P]),
}

# include/mipnerf_preview_tune_360.h: the gradient of the contracted lattice's march with respect to the rows, in a ninth library; the
# other eight keep their ABI versions and their entry points
PREVIEW_TUNE_360_LIB_PATH = os.environ.get("MIPNERF_PREVIEW_TUNE_360_LIB", os.path.join(HERE, "csrc", "libmipnerf_preview_tune_360.so"))
PREVIEW_TUNE_360_ABI = 1
PREVIEW_TUNE_360_SIGNATURES = {
    "mipnerf_preview_tune_360_abi_version": (C.c_int, []),
    "mipnerf_preview_tune_360_last_error": (C.c_char_p, []),
    "mipnerf_preview_tune_360_grad": (C.c_int, [C.POINTER(PreviewField), _F, C.POINTER(PreviewParams), _I64, _P, _P, _P, _P, _P, _P, _F, _P,
                                                _P, _P, _P, _P, _P]),
}

# include/mipnerf_proposal_360.h: the proposal density of the unbounded-scene model from a pyramid of contracted density lattices, in a
# tenth library; the other nine keep their ABI versions and their entry points
PROPOSAL_360_LIB_PATH = os.environ.get("MIPNERF_PROPOSAL_360_LIB", os.path.join(HERE, "csrc", "libmipnerf_proposal_360.so"))
PROPOSAL_360_ABI = 1
PROPOSAL_MAX_LEVELS = 4


class ProposalPyramid(C.Structure):
    _fields_ = [("levels", _I32), ("dims", (_I32 * 3) * PROPOSAL_MAX_LEVELS), ("lattice", _P * PROPOSAL_MAX_LEVELS), ("lo", _F * 3),
                ("hi", _F * 3)]


PROPOSAL_360_SIGNATURES = {
    "mipnerf_proposal_360_abi_version": (C.c_int, []),
    "mipnerf_proposal_360_last_error": (C.c_char_p, []),
    "mipnerf_lattice_density_360": (C.c_int, [C.POINTER(ProposalPyramid), _F, _I64, _I32, _P, _P, _P, _P, _P, _P]),
    "mipnerf_reciprocal_360": (C.c_int, [_I64, _P, _P, _P]),
}

# include/mipnerf_fuse.h: rendered depth fused into a truncated signed distance volume, in an eleventh library; the other ten keep their
# ABI versions and their entry points
FUSE_LIB_PATH = os.environ.get("MIPNERF_FUSE_LIB", os.path.join(HERE, "csrc", "libmipnerf_fuse.so"))
FUSE_ABI = 1
FUSE_MAX_QUANTILES = 4
FUSE_FRAME_FLOATS = 16
FUSE_FRAMES_PER_LAUNCH = 8
_FUSE_VOLUME = [C.POINTER(_I32), C.POINTER(_F), C.POINTER(_F), _F, _I32, _I64, _P, _P, _P, _I64, _P, _P]
FUSE_SIGNATURES = {
    "mipnerf_fuse_abi_version": (C.c_int, []),
    "mipnerf_fuse_last_error": (C.c_char_p, []),
    "mipnerf_fuse_depth_quantile": (C.c_int, [_I64, _I32, _P, _P, _I32, C.POINTER(_F), _P, _P]),
    "mipnerf_fuse_projection": (C.c_int, [_P, _P]),
    "mipnerf_fuse_integrate": (C.c_int, _FUSE_VOLUME + [_P]),
    "mipnerf_fuse_finalise": (C.c_int, [C.POINTER(_I32), _P, _P, _F, _P, _P]),
    "mipnerf_fuse_integrate_host": (C.c_int, list(_FUSE_VOLUME)),
}

_handles = {}


def _load(path, signatures, missing=None, abi=None):
    """Load (once) the library at `path` and set the argtypes of `signatures`.  `missing`: what the RuntimeError says after the path when
    the file is absent (None: return None instead).  `abi`: (name of the version getter, the version this binding speaks)."""
    if path not in _handles:
        if not os.path.exists(path):
            if missing is None:
                return None
            raise RuntimeError(f"{path} is missing: {missing} Build it with `python -m mipnerf_pl_amd.build` (needs hipcc / ROCm).")
        try:
            # PyTorch-ROCm bundles its own HIP runtime (soname-less libamdhip64.so): map it FIRST so the
            # library's DT_NEEDED "libamdhip64.so" binds to the same runtime instance torch uses
            # (one runtime per process => torch streams / synchronize() cover our kernels).
            import torch  # noqa: F401
        except ImportError:
            pass
        h = C.CDLL(path)
        for name, (res, args) in signatures.items():
            fn = getattr(h, name)       # AttributeError if the .so lacks a declared symbol
            fn.restype = res
            fn.argtypes = args
        if abi is not None and getattr(h, abi[0])() != abi[1]:
            raise RuntimeError(f"{path}: ABI {getattr(h, abi[0])()}, this binding speaks {abi[1]}: rebuild")
        _handles[path] = h
    return _handles[path]


def _check(rc, last_error_fn, what):
    """Turn a C error code into the exception the reference would raise."""
    if rc == OK:
        return
    msg = (last_error_fn() or b"").decode(errors="replace")
    msg = f"{what}: {msg}" if what else msg
    if rc == E_UNSUPPORTED:
        raise NotImplementedError(msg)
    if rc == E_INVALID:
        raise ValueError(msg)
    raise RuntimeError(f"{msg} (code {rc})")


def lib():
    """Load (once) and return the ctypes handle with argtypes set."""
    return _load(LIB_PATH, SIGNATURES, "the MI355X-native Mip-NeRF path has no CPU fallback.")


def diag_lib():
    """libmipnerf_diag.so or None when it was not built (callers report the diagnostics as absent)."""
    return _load(DIAG_LIB_PATH, DIAG_SIGNATURES)


def preview_360_lib():
    """Load (once) libmipnerf_preview_360.so.  No fallback: a missing library is an error."""
    return _load(PREVIEW_360_LIB_PATH, PREVIEW_360_SIGNATURES, "the contracted-lattice renderer has no fallback.",
                 ("mipnerf_preview_360_abi_version", PREVIEW_360_ABI))


def preview_360_check(rc: int, what: str = "") -> None:
    _check(rc, lambda: preview_360_lib().mipnerf_preview_360_last_error(), what)


def preview_lib():
    """Load (once) libmipnerf_preview.so.  No fallback: a missing library is an error."""
    return _load(PREVIEW_LIB_PATH, PREVIEW_SIGNATURES, "the baked-lattice renderer has no fallback.", ("mipnerf_preview_abi_version", PREVIEW_ABI))


def preview_mip_lib():
    """Load (once) libmipnerf_preview_mip.so.  No fallback: a missing library is an error."""
    return _load(PREVIEW_MIP_LIB_PATH, PREVIEW_MIP_SIGNATURES, "the pyramid renderer has no fallback.",
                 ("mipnerf_preview_mip_abi_version", PREVIEW_MIP_ABI))


def preview_sparse_lib():
    """Load (once) libmipnerf_preview_sparse.so.  No fallback: a missing library is an error."""
    return _load(PREVIEW_SPARSE_LIB_PATH, PREVIEW_SPARSE_SIGNATURES, "the sparse-lattice renderer has no fallback.",
                 ("mipnerf_preview_sparse_abi_version", PREVIEW_SPARSE_ABI))


def preview_tune_lib():
    """Load (once) libmipnerf_preview_tune.so.  No fallback: a missing library is an error."""
    return _load(PREVIEW_TUNE_LIB_PATH, PREVIEW_TUNE_SIGNATURES, "tuning the baked lattice has no fallback.",
                 ("mipnerf_preview_tune_abi_version", PREVIEW_TUNE_ABI))


def preview_tune_check(rc: int, what: str = "") -> None:
    _check(rc, lambda: preview_tune_lib().mipnerf_preview_tune_last_error(), what)


def preview_tune_360_lib():
    """Load (once) libmipnerf_preview_tune_360.so.  No fallback: a missing library is an error."""
    return _load(PREVIEW_TUNE_360_LIB_PATH, PREVIEW_TUNE_360_SIGNATURES, "tuning a contracted lattice has no fallback.",
                 ("mipnerf_preview_tune_360_abi_version", PREVIEW_TUNE_360_ABI))


def preview_tune_360_check(rc: int, what: str = "") -> None:
    _check(rc, lambda: preview_tune_360_lib().mipnerf_preview_tune_360_last_error(), what)


def proposal_360_lib():
    """Load (once) libmipnerf_proposal_360.so.  No fallback: a missing library is an error."""
    return _load(PROPOSAL_360_LIB_PATH, PROPOSAL_360_SIGNATURES, "the contracted proposal lattice has no fallback.",
                 ("mipnerf_proposal_360_abi_version", PROPOSAL_360_ABI))


def proposal_360_check(rc: int, what: str = "") -> None:
    _check(rc, lambda: proposal_360_lib().mipnerf_proposal_360_last_error(), what)


def fuse_lib():
    """Load (once) libmipnerf_fuse.so.  No fallback: a missing library is an error."""
    return _load(FUSE_LIB_PATH, FUSE_SIGNATURES, "fusing depth into a signed distance volume has no fallback.",
                 ("mipnerf_fuse_abi_version", FUSE_ABI))


def fuse_check(rc: int, what: str = "") -> None:
    _check(rc, lambda: fuse_lib().mipnerf_fuse_last_error(), what)


def preview_reg_lib():
    """Load (once) libmipnerf_preview_reg.so.  No fallback: a missing library is an error."""
    return _load(PREVIEW_REG_LIB_PATH, PREVIEW_REG_SIGNATURES, "regularising the tuning of the baked lattice has no fallback.",
                 ("mipnerf_preview_reg_abi_version", PREVIEW_REG_ABI))


def preview_reg_check(rc: int, what: str = "") -> None:
    _check(rc, lambda: preview_reg_lib().mipnerf_preview_reg_last_error(), what)


def preview_sparse_check(rc: int, what: str = "") -> None:
    _check(rc, lambda: preview_sparse_lib().mipnerf_preview_sparse_last_error(), what)


def preview_check(rc: int, what: str = "") -> None:
    _check(rc, lambda: preview_lib().mipnerf_preview_last_error(), what)


def preview_mip_check(rc: int, what: str = "") -> None:
    _check(rc, lambda: preview_mip_lib().mipnerf_preview_mip_last_error(), what)


def diag_check(rc: int, what: str = "") -> None:
    if rc != OK:
        msg = (diag_lib().mipnerf_diag_last_error() or b"").decode(errors="replace")
        raise (ValueError if rc == E_INVALID else RuntimeError)(f"{what}: {msg} (code {rc})")


def num_camera_modes() -> int:
    """Camera modes `mipnerf_generate_rays` of the loaded library knows (4: Blender focal, pix2cam, radial-tangential, fisheye)."""
    return int(lib().mipnerf_num_camera_modes())


def last_error() -> str:
    return (lib().mipnerf_last_error() or b"").decode(errors="replace")


def check(rc: int, what: str = "") -> None:
    """Turn a C error code into the exception the reference would raise."""
    _check(rc, lambda: lib().mipnerf_last_error(), what)
