"""Host-side mirror of the free functions of the reference's models/mip.py, same names and
argument meaning, executing on MI355X through the C ABI of libmipnerf_hip.so.

Every function takes / returns torch tensors that live on a HIP device (`tensor.is_cuda`);
torch is only the owner of device memory and of the current stream.  There is no CPU path:
CPU tensors raise.  Randomised variants draw their uniform noise with torch's device RNG
(`torch.rand`) and hand it to the kernels, which apply it exactly like mip.py:155-160 / 198-204.
"""
from __future__ import annotations

import torch

from . import _lib as L


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _f32c(t: torch.Tensor, name: str) -> torch.Tensor:
    if not t.is_cuda:
        raise RuntimeError(f"{name}: the MI355X-native path needs HIP device tensors (got {t.device}); "
                           "there is no CPU fallback")
    if t.dtype != torch.float32:
        raise TypeError(f"{name}: expected float32, got {t.dtype}")
    return t.contiguous()


def _ptr(t):
    return None if t is None else t.data_ptr()


def _torch_dtype(precision: int):
    return torch.bfloat16 if precision == L.PREC_BF16 else torch.float32


# ---------------------------------------------------------------------------------------------
def cast_rays(t_samples, origins, directions, radii, ray_shape="cone", diagonal=True):
    """models/mip.py:81-103 -> (means [B,N,3], covs [B,N,3])."""
    if ray_shape != "cone" or not diagonal:
        raise NotImplementedError  # mip.py:97-98 ('cylinder'); full covariances are dead code upstream
    t_samples = _f32c(t_samples, "t_samples")
    B, N1 = t_samples.shape
    N = N1 - 1
    means = torch.empty(B, N, 3, device=t_samples.device, dtype=torch.float32)
    covs = torch.empty_like(means)
    # contiguous copies (if any) are bound to locals: a temporary would be freed, and its block re-used by the next
    # temporary, before the launch
    o, d, r = _f32c(origins, "origins"), _f32c(directions, "directions"), _f32c(radii, "radii")
    L.check(L.lib().mipnerf_cast_rays(B, N, _ptr(t_samples), _ptr(o), _ptr(d), _ptr(r), _ptr(means), _ptr(covs), _stream()),
            "cast_rays")
    return means, covs


def sample_t(num_samples, near, far, randomized, disparity, t_rand=None):
    """t part of sample_along_rays (mip.py:143-163): [B, N+1]."""
    near = _f32c(near, "near")
    far = _f32c(far, "far")
    B = near.shape[0]
    if randomized and t_rand is None:
        t_rand = torch.rand(B, num_samples + 1, device=near.device)   # mip.py:159
    t = torch.empty(B, num_samples + 1, device=near.device, dtype=torch.float32)
    tr = _f32c(t_rand, "t_rand") if randomized else None
    L.check(L.lib().mipnerf_sample_along_rays(B, num_samples, _ptr(near), _ptr(far), _ptr(tr),
                                              int(bool(disparity)), _ptr(t), _stream()), "sample_along_rays")
    return t


def sample_along_rays(origins, directions, radii, num_samples, near, far, randomized, disparity, ray_shape,
                      t_rand=None):
    """models/mip.py:127-165 -> (t_samples [B,N+1], (means, covs))."""
    t = sample_t(num_samples, near, far, randomized, disparity, t_rand)
    return t, cast_rays(t, origins, directions, radii, ray_shape)


def sorted_piecewise_constant_pdf(bins, weights, num_samples, randomized, u_rand=None):
    """models/mip.py:168-229.  `weights` is NOT mutated (the reference pads it in place)."""
    bins = _f32c(bins, "bins")
    weights = _f32c(weights, "weights")
    B, nb = weights.shape
    if randomized and u_rand is None:
        u_rand = torch.rand(B, num_samples, device=bins.device)       # stands in for uniform_(mip.py:201)
    out = torch.empty(B, num_samples, device=bins.device, dtype=torch.float32)
    ur = _f32c(u_rand, "u_rand") if randomized else None
    L.check(L.lib().mipnerf_sorted_piecewise_constant_pdf(
        B, nb, _ptr(bins), _ptr(weights), num_samples, _ptr(ur), _ptr(out), _stream()),
        "sorted_piecewise_constant_pdf")
    return out


def resample_t(t_samples, weights, randomized, resample_padding, u_rand=None):
    """t part of resample_along_rays (mip.py:250-271): blur-pool + padding + PDF inversion."""
    t_samples = _f32c(t_samples, "t_samples")
    weights = _f32c(weights.detach(), "weights")     # no graph here; the differentiable form is autograd._ResampleT
    B, N = weights.shape
    if randomized and u_rand is None:
        u_rand = torch.rand(B, N + 1, device=weights.device)
    out = torch.empty(B, N + 1, device=weights.device, dtype=torch.float32)
    ur = _f32c(u_rand, "u_rand") if randomized else None
    L.check(L.lib().mipnerf_resample_along_rays(
        B, N, _ptr(t_samples), _ptr(weights), _ptr(ur), float(resample_padding), _ptr(out), _stream()), "resample_along_rays")
    return out


def resample_along_rays(origins, directions, radii, t_samples, weights, randomized, ray_shape, stop_grad,
                        resample_padding, u_rand=None):
    """models/mip.py:232-280 -> (new_t_vals [B,N+1], (means, covs))."""
    if not stop_grad and torch.is_grad_enabled() and weights.requires_grad:
        # mip.py:265-279: new_t_vals stays differentiable w.r.t. the weights (native backward, autograd._ResampleT); the Gaussians
        # below are computed without a graph -- inside MipNerf the fused encoding (autograd._CastIPE) carries that gradient
        from .autograd import _ResampleT
        if randomized and u_rand is None:
            u_rand = torch.rand(weights.shape[0], weights.shape[1] + 1, device=weights.device)
        t = _ResampleT.apply(t_samples, weights, resample_padding, u_rand if randomized else None)
        # the reference keeps means / covs differentiable w.r.t. t here (mip.py:265-280).  The native backward of that link is
        # fused with the encoding (autograd._CastIPE, what MipNerf uses); the stand-alone Gaussians stay attached to the graph
        # through a node whose backward RAISES, so composing this op with integrated_pos_enc can never silently drop the gradient
        from .autograd import _CastRaysNoBackward
        means, covs = _CastRaysNoBackward.apply(t, origins, directions, radii, ray_shape)
        return t, (means, covs)
    t = resample_t(t_samples, weights, randomized, resample_padding, u_rand)
    return t, cast_rays(t, origins, directions, radii, ray_shape)


def integrated_pos_enc(means_covs, min_deg, max_deg, diagonal=True, precision=L.PREC_FP32):
    """models/mip.py:322-350 -> [B, N, 6*(max_deg-min_deg)] (float32, or bfloat16 for the bf16 MLP)."""
    if not diagonal:
        raise NotImplementedError
    means, covs = means_covs
    means = _f32c(means, "means")
    covs = _f32c(covs, "covs")
    M = means.numel() // 3
    enc = torch.empty(*means.shape[:-1], 6 * (max_deg - min_deg), device=means.device, dtype=_torch_dtype(precision))
    L.check(L.lib().mipnerf_integrated_pos_enc(M, min_deg, max_deg, _ptr(means), _ptr(covs), _ptr(enc),
                                               precision, _stream()), "integrated_pos_enc")
    return enc


def cast_ipe(t_samples, origins, directions, radii, min_deg, max_deg, disable_integration=False,
             precision=L.PREC_FP32):
    """cast_rays + integrated_pos_enc fused (what MipNerf.forward uses): [B, N, 6L]."""
    t_samples = _f32c(t_samples, "t_samples")
    B, N1 = t_samples.shape
    enc = torch.empty(B, N1 - 1, 6 * (max_deg - min_deg), device=t_samples.device, dtype=_torch_dtype(precision))
    o, d, r = _f32c(origins, "origins"), _f32c(directions, "directions"), _f32c(radii, "radii")   # kept alive until after the launch
    L.check(L.lib().mipnerf_cast_ipe(B, N1 - 1, min_deg, max_deg, int(bool(disable_integration)), _ptr(t_samples),
                                     _ptr(o), _ptr(d), _ptr(r), _ptr(enc), precision, _stream()), "cast_ipe")
    return enc


def pos_enc(x, min_deg, max_deg, append_identity=True, precision=L.PREC_FP32, ld=None):
    """models/mip.py:353-363 for min_deg == 0, append_identity=True -> [B, 3 + 6*max_deg] (row stride ld)."""
    if min_deg != 0 or not append_identity:
        raise NotImplementedError("pos_enc is implemented for min_deg=0, append_identity=True (the only call "
                                  "on the hot path, mip_nerf.py:220-225)")
    x = _f32c(x, "x")
    B = x.shape[0]
    width = 3 + 6 * max_deg
    ld = width if ld is None else ld
    out = torch.empty(B, ld, device=x.device, dtype=_torch_dtype(precision))
    L.check(L.lib().mipnerf_pos_enc(B, max_deg, _ptr(x), _ptr(out), ld, precision, _stream()), "pos_enc")
    return out


def volumetric_rendering(rgb, density, t_samples, dirs, white_bkgd):
    """models/mip.py:366-401 -> (comp_rgb [B,3], distance [B], acc [B], weights [B,N])."""
    rgb_sigma = torch.cat([_f32c(rgb, "rgb"), _f32c(density, "density")], dim=-1).contiguous()
    return volumetric_rendering_packed(rgb_sigma, t_samples, dirs, white_bkgd)


def volumetric_rendering_packed(rgb_sigma, t_samples, dirs, white_bkgd):
    """Same, on the MLP kernel's packed output [B, N, 4] = (r, g, b, sigma)."""
    rgb_sigma = _f32c(rgb_sigma, "rgb_sigma")
    t_samples = _f32c(t_samples, "t_samples")
    B, N1 = t_samples.shape
    N = N1 - 1
    dev = t_samples.device
    comp_rgb = torch.empty(B, 3, device=dev)
    distance = torch.empty(B, device=dev)
    acc = torch.empty(B, device=dev)
    weights = torch.empty(B, N, device=dev)
    dirs = _f32c(dirs, "dirs")
    L.check(L.lib().mipnerf_volumetric_rendering(B, N, _ptr(rgb_sigma), _ptr(t_samples), _ptr(dirs),
                                                 int(bool(white_bkgd)), _ptr(comp_rgb), _ptr(distance), _ptr(acc),
                                                 _ptr(weights), _stream()), "volumetric_rendering")
    return comp_rgb, distance, acc, weights


CAMERA_MODES = {"pinhole": 1, "radial": 2, "fisheye": 3}      # rec[26] of a pix2cam record (0: the Blender focal formula)


def camera_record(c2w, width, height, near, far, focal=None, pix2cam=None, lossmult=1.0, dtype=torch.float32, model="pinhole",
                  distortion=None):
    """One row of the camera table of `generate_rays` (32 numbers, include/mipnerf_hip.h): Blender pinhole camera
    when `focal` is given (datasets.py:226-228), Multicam when `pix2cam` is given (datasets.py:125-131).
    dtype=torch.float64: a table for float64 ray arithmetic (RenderGen, render_video.py:29-112).
    `model='radial'` with `distortion=(k1, k2, p1, p2)` (COLMAP SIMPLE_RADIAL / RADIAL / OPENCV) or `model='fisheye'` with
    `distortion=(k1, k2, k3, k4)` (OPENCV_FISHEYE): a distorted camera, whose rays the kernel undistorts per pixel (csrc/camera_models.hpp).
    `pix2cam` must then be K^-1 with rows 1 and 2 negated (last row (0, 0, -1)), as `datasets.load_realdata360` builds it.  A fisheye
    camera's directions are of unit length, so its near / far are distances along the ray."""
    if model not in CAMERA_MODES:
        raise ValueError(f"camera_record: model must be one of {sorted(CAMERA_MODES)}, got {model!r}")
    if (model != "pinhole" or distortion is not None) and pix2cam is None:
        raise ValueError("camera_record: a distorted camera (model / distortion) needs pix2cam, not focal")
    rec = torch.zeros(32, dtype=dtype)
    rec[0:12] = torch.as_tensor(c2w, dtype=dtype)[:3, :4].reshape(-1)
    if (focal is None) == (pix2cam is None):
        raise ValueError("give exactly one of focal (Blender) / pix2cam (Multicam)")
    if pix2cam is not None:
        rec[12:21] = torch.as_tensor(pix2cam, dtype=dtype)[:3, :3].reshape(-1)
        rec[26] = 1.0
    else:
        rec[27] = float(focal)
    rec[21], rec[22], rec[23], rec[24], rec[25] = float(width), float(height), float(near), float(far), float(lossmult)
    if model != "pinhole":
        coeffs = [0.0] * 4 if distortion is None else [float(v) for v in distortion]
        if len(coeffs) != 4:
            raise ValueError(f"camera_record: distortion holds 4 coefficients ({'k1, k2, p1, p2' if model == 'radial' else 'k1, k2, k3, k4'}), "
                             f"got {len(coeffs)}")
        if rec[18:21].tolist() != [0.0, 0.0, -1.0]:
            raise ValueError("camera_record: a distorted camera needs a pix2cam whose last row is (0, 0, -1) (K^-1 with rows 1 and 2 negated), "
                             f"got {rec[18:21].tolist()}")
        if L.num_camera_modes() <= CAMERA_MODES[model]:
            raise RuntimeError(f"camera_record: the loaded library knows camera modes 0..{L.num_camera_modes() - 1} only; it would render a "
                               f"{model!r} camera as a pinhole")
        rec[26] = float(CAMERA_MODES[model])
        rec[28:32] = torch.tensor(coeffs, dtype=dtype)
    elif distortion is not None:
        if len(tuple(distortion)) != 4:
            raise ValueError(f"camera_record: distortion holds 4 coefficients, got {len(tuple(distortion))}")
        if any(float(v) != 0.0 for v in distortion):
            raise ValueError("camera_record: model='pinhole' has no distortion; give model='radial' or 'fisheye'")
    return rec


def generate_rays(cameras, num_rays=None, cam_idx=None, pix_idx=None):
    """Rays of datasets.py:214-263 / 116-168 computed on the device: `cameras` [ncam, 32] float32 HIP tensor of
    `camera_record` rows, ray i = pixel pix_idx[i] (y*W + x; None = i) of camera cam_idx[i] (None = 0).
    A float64 table selects float64 arithmetic (mipnerf_generate_rays_f64); the rays are float32 either way."""
    from .rays import Rays
    f64 = cameras.dtype == torch.float64
    if f64:
        if not cameras.is_cuda:
            raise RuntimeError("cameras: needs a HIP device tensor")
        cameras = cameras.contiguous().reshape(-1, 32)
    else:
        cameras = _f32c(cameras, "cameras").reshape(-1, 32)
    dev = cameras.device
    if num_rays is None:
        num_rays = int(pix_idx.numel()) if pix_idx is not None else int(cameras[0, 21].item() * cameras[0, 22].item())

    def i32(t, name):
        if t is None:
            return None
        if not t.is_cuda:
            raise RuntimeError(f"{name}: needs a HIP device tensor")
        return t.to(torch.int32).contiguous()
    ci, pi = i32(cam_idx, "cam_idx"), i32(pix_idx, "pix_idx")
    out = [torch.empty(num_rays, k, device=dev, dtype=torch.float32) for k in (3, 3, 3, 1, 1, 1, 1)]
    rp = L.RaysPtrs(*[t.data_ptr() for t in out])
    import ctypes as C
    fn = L.lib().mipnerf_generate_rays_f64 if f64 else L.lib().mipnerf_generate_rays
    L.check(fn(num_rays, _ptr(cameras), _ptr(ci), _ptr(pi), C.byref(rp), _stream()), "generate_rays")
    return Rays(*out)


def gather_train_batch(order, offsets, cameras, pixels, step, epoch_base, rays_out, gt_out):
    """Batch b = step[0] - epoch_base[0] (both read on the device) of an epoch order, written into `rays_out` (Rays of [B, k] fp32
    buffers) and `gt_out` [B, 3]: the same bits as `dataset.rays_at(order[b*B:(b+1)*B])` (BaseDataset: `offsets` int64 [n_images + 1],
    `cameras` [n_images, 32] fp32, `pixels` [P, 3] fp32), with no host synchronisation -- the batch source of a captured training
    step (train_graph.GraphedTrainStep).  Rays past the end of `order` are left unwritten."""
    import ctypes as C
    B = int(gt_out.shape[0])
    dev = gt_out.device

    def chk(t, name, dtype, shape=None):
        if not (t.is_cuda and t.device == dev and t.dtype == dtype and t.is_contiguous()):
            raise ValueError(f"gather_train_batch: {name} must be a contiguous {dtype} tensor on {dev}")
        if shape is not None and tuple(t.shape) != tuple(shape):
            raise ValueError(f"gather_train_batch: {name} has shape {tuple(t.shape)}, expected {tuple(shape)}")
        return t
    chk(gt_out, "gt_out", torch.float32, (B, 3))
    for k, w in zip(rays_out._fields, (3, 3, 3, 1, 1, 1, 1)):
        chk(getattr(rays_out, k), k, torch.float32, (B, w))
    chk(order, "order", torch.int64)
    chk(offsets, "offsets", torch.int64)
    chk(cameras, "cameras", torch.float32, (offsets.numel() - 1, 32))
    chk(pixels, "pixels", torch.float32)
    chk(step, "step", torch.int64)
    chk(epoch_base, "epoch_base", torch.int64)
    rp = L.RaysPtrs(*[t.data_ptr() for t in rays_out])
    L.check(L.lib().mipnerf_gather_train_batch(B, order.numel(), _ptr(order), offsets.numel() - 1, _ptr(offsets), _ptr(cameras),
                                               _ptr(pixels), _ptr(step), _ptr(epoch_base), C.byref(rp), _ptr(gt_out), _stream()),
            "gather_train_batch")


def eval_errors(pred_color, batch_pixels):
    """utils/metrics.py:191-197: (psnr, ssim) of one rendered frame, pred/gt [1,H,W,3] (or [H,W,3]) fp32 HIP tensors;
    one fused kernel instead of six conv2d passes.  Returns two 0-d tensors."""
    a = _f32c(pred_color, "pred_color")
    b = _f32c(batch_pixels, "batch_pixels")
    if a.dim() == 4:
        if a.shape[0] != 1:
            raise NotImplementedError("eval_errors: one frame at a time (eval.py evaluates image by image)")
        a, b = a[0], b[0]
    if a.shape != b.shape or a.dim() != 3 or a.shape[-1] != 3:
        raise ValueError("eval_errors: expected matching [H,W,3] images")
    H, W = int(a.shape[0]), int(a.shape[1])
    ws = torch.empty(int(L.lib().mipnerf_eval_workspace_floats(H, W)), device=a.device, dtype=torch.float32)
    out = torch.empty(2, device=a.device, dtype=torch.float32)
    a, b = a.contiguous(), b.contiguous()
    L.check(L.lib().mipnerf_eval_errors(H, W, _ptr(a), _ptr(b), _ptr(ws), _ptr(out), _stream()),
            "eval_errors")
    return out[0], out[1]


def _u8_out(out, shape, device, name):
    if out is None:
        return torch.empty(shape, dtype=torch.uint8, device=device)
    if out.dtype != torch.uint8 or tuple(out.shape) != tuple(shape) or not out.is_contiguous() or out.device != device:
        raise ValueError(f"{name}: `out` must be a contiguous uint8 tensor of shape {tuple(shape)} on {device}")
    return out


def visualize_workspace_floats(num_pixels: int) -> int:
    return int(L.lib().mipnerf_visualize_workspace_floats(int(num_pixels)))


def visualize_map(x, out=None, workspace=None):
    """utils/vis.py:visualize_depth of a distance / acc map [..., H, W] (any shape; the min / max run over all of it): the uint8 RGB
    bytes [*x.shape, 3] that the reference writes to its _dist.png / _acc.png.  `out` / `workspace` (visualize_workspace_floats(numel)
    floats) may be given, e.g. inside a captured graph."""
    a = _f32c(x, "visualize_map")
    n = a.numel()
    out = _u8_out(out, (*a.shape, 3), a.device, "visualize_map")
    if workspace is None:
        workspace = torch.empty(visualize_workspace_floats(n), device=a.device, dtype=torch.float32)
    elif workspace.dtype != torch.float32 or workspace.numel() < visualize_workspace_floats(n):
        raise ValueError("visualize_map: workspace too small")
    L.check(L.lib().mipnerf_visualize_map(n, _ptr(a), _ptr(workspace), _ptr(out), _stream()), "visualize_map")
    return out


def image_to_u8(x, out=None):
    """torchvision save_image after save_image_tensor's clamp (vis.py:46-63) on one image: (uint8)(clamp(x, 0, 1) * 255 + 0.5),
    elementwise, same shape as x."""
    a = _f32c(x, "image_to_u8")
    out = _u8_out(out, a.shape, a.device, "image_to_u8")
    L.check(L.lib().mipnerf_image_to_u8(a.numel(), _ptr(a), _ptr(out), _stream()), "image_to_u8")
    return out


def pyramid_sizes(height: int, width: int, n_levels: int):
    """[(H >> j, W >> j)] of the converter's levels; ValueError when a level would not halve exactly (the reference crashes in reshape)."""
    n_levels = int(n_levels)
    if not 1 <= n_levels <= L.MAX_PYRAMID_LEVELS:
        raise ValueError(f"box_pyramid: n_levels must be in [1, {L.MAX_PYRAMID_LEVELS}], got {n_levels}")
    t = 1 << (n_levels - 1)
    if height < 1 or width < 1 or height % t or width % t:
        raise ValueError(f"box_pyramid: {height} x {width} (H x W) is not divisible by 2^(n_levels-1) = {t}")
    return [(height >> j, width >> j) for j in range(n_levels)]


def box_pyramid(src_u8, n_levels, white_bkgd=None, out_u8=None, out_rgb=None, rgb_row_offset=0, scratch=None):
    """convert_blender_data.py:65-81 on a batch of frames.  src_u8 [n, H, W, 4] uint8 RGBA on the device -> (u8_levels, rgb_levels):
    u8_levels[j] [n, H >> j, W >> j, 4] = the bytes of NNN_dj.png (views of one level-major buffer `out_u8`, 4 * n * PPI bytes, PPI =
    sum_j (H >> j)(W >> j)); rgb_levels[j] [n, H >> j, W >> j, 3] float32 = what datasets.load_multicam makes of those PNGs, composited
    over white or not per `white_bkgd`, as strided views of the data set's row order (image-major, level inside the image): rows
    rgb_row_offset ... rgb_row_offset + n * PPI of `out_rgb` [P, 3].  white_bkgd=None and no `out_rgb`: no rows, rgb_levels is None.
    `scratch` (n_levels > 4): float32, at least 5 * n * (H >> 3) * (W >> 3) floats.  Given buffers make the call allocation-free (capturable)."""
    if not src_u8.is_cuda:
        raise RuntimeError(f"box_pyramid: the MI355X-native path needs HIP device tensors (got {src_u8.device}); there is no CPU fallback")
    if src_u8.dtype != torch.uint8 or src_u8.dim() != 4 or src_u8.shape[-1] != 4:
        raise TypeError(f"box_pyramid: expected uint8 [n, H, W, 4], got {src_u8.dtype} {tuple(src_u8.shape)}")
    src = src_u8.contiguous()
    n, h, w, _ = src.shape
    sizes = pyramid_sizes(h, w, n_levels)
    if n < 1:
        raise ValueError("box_pyramid: no images")
    ppi = sum(a * b for a, b in sizes)
    out_u8 = _u8_out(out_u8, (4 * n * ppi,), src.device, "box_pyramid")
    want_rgb = out_rgb is not None or white_bkgd is not None
    if want_rgb:
        if out_rgb is None:
            out_rgb = torch.empty(rgb_row_offset + n * ppi, 3, dtype=torch.float32, device=src.device)
        elif (out_rgb.dtype != torch.float32 or out_rgb.dim() != 2 or out_rgb.shape[1] != 3 or not out_rgb.is_contiguous()
              or out_rgb.device != src.device or rgb_row_offset < 0 or out_rgb.shape[0] < rgb_row_offset + n * ppi):
            raise ValueError(f"box_pyramid: `out_rgb` must be a contiguous float32 [P, 3] tensor on {src.device} with P >= row offset + {n * ppi}")
    need = 5 * n * (h >> 3) * (w >> 3) if len(sizes) > 4 else 0
    if need:
        if scratch is None:
            scratch = torch.empty(need, dtype=torch.float32, device=src.device)
        elif scratch.dtype != torch.float32 or scratch.numel() < need or not scratch.is_contiguous() or scratch.device != src.device:
            raise ValueError(f"box_pyramid: scratch must hold {need} float32 values on {src.device}")
    L.check(L.lib().mipnerf_box_pyramid(n, h, w, len(sizes), _ptr(src), _ptr(out_u8), _ptr(out_rgb) if want_rgb else None, int(rgb_row_offset),
                                        int(bool(white_bkgd)), _ptr(scratch) if need else None, _stream()), "box_pyramid")
    u8_levels, rgb_levels, off, row = [], [] if want_rgb else None, 0, int(rgb_row_offset)
    for hj, wj in sizes:
        u8_levels.append(out_u8[off:off + 4 * n * hj * wj].view(n, hj, wj, 4))
        if want_rgb:
            rgb_levels.append(out_rgb.as_strided((n, hj, wj, 3), (3 * ppi, 3 * wj, 3, 1), 3 * row))
        off += 4 * n * hj * wj
        row += hj * wj
    return u8_levels, rgb_levels


def area_downscale(src_u8, factor, out_rgb=None, row_offset=0):
    """Box shrink of captured images by an integer `factor` F in [1, 16]: src_u8 [n, H, W, C] uint8 on the device, C in {3, 4} (a 4th
    channel is dropped, no compositing) -> rows row_offset ... row_offset + n * h * w of `out_rgb` [P, 3] float32 (image-major,
    row-major: the data set's pixel table), h = H // F, w = W // F, the H % F bottom rows and W % F right columns ignored.  Per value:
    q = (2 S + F F) // (2 F F) of the integer sum S of the F x F source bytes (the box mean rounded half up to a byte), stored as
    float32(q) / 255: what `datasets._read_image` makes of an images_<F>/ file holding the bytes q.  Returns the written rows as
    [n, h, w, 3] (a view of `out_rgb`)."""
    if not src_u8.is_cuda:
        raise RuntimeError(f"area_downscale: the MI355X-native path needs HIP device tensors (got {src_u8.device}); there is no CPU fallback")
    if src_u8.dtype != torch.uint8 or src_u8.dim() != 4 or src_u8.shape[-1] not in (3, 4):
        raise TypeError(f"area_downscale: expected uint8 [n, H, W, 3 or 4], got {src_u8.dtype} {tuple(src_u8.shape)}")
    if isinstance(factor, bool) or int(factor) != factor or not 1 <= int(factor) <= L.MAX_DOWNSCALE_FACTOR:
        raise ValueError(f"area_downscale: factor must be an integer in [1, {L.MAX_DOWNSCALE_FACTOR}], got {factor!r}")
    factor = int(factor)
    src = src_u8.contiguous()
    if src.data_ptr() % 16:
        src = src.clone()
    n, H, W, C = src.shape
    h, w = H // factor, W // factor
    if n < 1 or h < 1 or w < 1:
        raise ValueError(f"area_downscale: no output pixels ({n} images of {H} x {W} at factor {factor})")
    row_offset = int(row_offset)
    if out_rgb is None:
        out_rgb = torch.empty(row_offset + n * h * w, 3, dtype=torch.float32, device=src.device)
    elif (out_rgb.dtype != torch.float32 or out_rgb.dim() != 2 or out_rgb.shape[1] != 3 or not out_rgb.is_contiguous()
          or out_rgb.device != src.device or row_offset < 0 or out_rgb.shape[0] < row_offset + n * h * w):
        raise ValueError(f"area_downscale: `out_rgb` must be a contiguous float32 [P, 3] tensor on {src.device} with P >= row offset + {n * h * w}")
    L.check(L.lib().mipnerf_area_downscale(n, H, W, C, factor, _ptr(src), _ptr(out_rgb), row_offset, _stream()), "area_downscale")
    return out_rgb[row_offset:row_offset + n * h * w].view(n, h, w, 3)


def selftest() -> str:
    """Run the hardware self-test (MFMA lane layouts, LDS DMA); returns the report, raises on failure."""
    rc = L.lib().mipnerf_selftest(_stream())
    msg = L.last_error()
    if rc != 0:
        raise RuntimeError(f"gfx950 self-test failed (code {rc:#x}): {msg}")
    return msg


# ---- unbounded scenes (mip-NeRF 360) -------------------------------------------------------------------------------------
# Working versions of the reference's dead functions (models/mip.py:106-124, 292-319, 424-447); they follow the paper the
# dead code aims at (Barron et al., "Mip-NeRF 360", CVPR 2022) -- csrc/raymath360.hpp explains what is wrong upstream.
def sample_t_360(num_samples, near, far, randomized, t_rand=None):
    """Fence posts uniform in normalised inverse depth: (t_inv [B,N+1], t [B,N+1]) (mip.py:106-121)."""
    near, far = _f32c(near, "near"), _f32c(far, "far")
    B = near.shape[0]
    if randomized and t_rand is None:
        t_rand = torch.rand(B, num_samples + 1, device=near.device)
    tr = _f32c(t_rand, "t_rand") if randomized else None
    t_inv = torch.empty(B, num_samples + 1, device=near.device, dtype=torch.float32)
    t = torch.empty_like(t_inv)
    L.check(L.lib().mipnerf_sample_along_rays_360(B, num_samples, _ptr(near), _ptr(far), _ptr(tr), _ptr(t_inv), _ptr(t),
                                                  _stream()), "sample_along_rays_360")
    return t_inv, t


def cast_rays_360(t_samples, origins, directions, radii, contracted=False):
    """Conical frustums -> Gaussians with FULL covariance, optionally contracted: (means [B,N,3], covs [B,N,3,3])."""
    t_samples = _f32c(t_samples, "t_samples")
    B, N1 = t_samples.shape
    means = torch.empty(B, N1 - 1, 3, device=t_samples.device, dtype=torch.float32)
    covs = torch.empty(B, N1 - 1, 3, 3, device=t_samples.device, dtype=torch.float32)
    o, d, r = _f32c(origins, "origins"), _f32c(directions, "directions"), _f32c(radii, "radii")
    L.check(L.lib().mipnerf_cast_ipe_360(B, N1 - 1, 0, 1, int(bool(contracted)), _ptr(t_samples), _ptr(o), _ptr(d), _ptr(r), None,
                                         L.PREC_FP32, _ptr(means), _ptr(covs), _stream()), "cast_rays_360")
    return means, covs


def sample_along_rays_360(origins, directions, radii, num_samples, near, far, randomized, disparity=False, ray_shape="cone",
                          t_rand=None):
    """models/mip.py:106-124 (same signature and return): (t_inv [B,N+1], (means [B,N,3], covs [B,N,3,3]))."""
    if ray_shape != "cone":
        raise NotImplementedError
    t_inv, t = sample_t_360(num_samples, near, far, randomized, t_rand)
    return t_inv, cast_rays_360(t, origins, directions, radii, contracted=False)


def cast_ipe_360(t_samples, origins, directions, radii, min_deg, max_deg, contracted=True, precision=L.PREC_FP32, fragments=False):
    """Fused frustum -> full-covariance Gaussian -> contraction -> off-axis IPE: [B, N, 2*21*(max_deg-min_deg)]; what
    `integrated_pos_enc_360(parameterization(cast_rays(...)))` of the reference is meant to compute (mip.py:292-319, 431-447).
    fragments=True (bf16 only): the MFMA B-operand fragment layout the two-kernel MLP form reads fastest -- an opaque
    [ceil(B N / 256) * 256, features] bf16 buffer for `autograd.mlp_native(..., frag_shape=(B, N))`, not a row-major tensor."""
    t_samples = _f32c(t_samples, "t_samples")
    B, N1 = t_samples.shape
    F = 42 * (max_deg - min_deg)
    o, d, r = _f32c(origins, "origins"), _f32c(directions, "directions"), _f32c(radii, "radii")
    if fragments:
        if precision != L.PREC_BF16:
            raise ValueError("cast_ipe_360(fragments=True) is a bf16 layout")
        M = B * (N1 - 1)
        enc = torch.empty((M + 255) // 256 * 256, F, device=t_samples.device, dtype=torch.bfloat16)
        L.check(L.lib().mipnerf_cast_ipe_360(B, N1 - 1, min_deg, max_deg, int(bool(contracted)), _ptr(t_samples), _ptr(o), _ptr(d),
                                             _ptr(r), _ptr(enc), L.OUT_BF16_FRAGMENTS, None, None, _stream()), "cast_ipe_360")
        return enc
    enc = torch.empty(B, N1 - 1, F, device=t_samples.device, dtype=_torch_dtype(precision))
    L.check(L.lib().mipnerf_cast_ipe_360(B, N1 - 1, min_deg, max_deg, int(bool(contracted)), _ptr(t_samples), _ptr(o), _ptr(d),
                                         _ptr(r), _ptr(enc), precision, None, None, _stream()), "cast_ipe_360")
    return enc


def parameterization(means, covs):
    """models/mip.py:431-447 done right: the scene contraction pushed through Gaussians, (contract(mean), J cov J^T)."""
    means, covs = _f32c(means, "means"), _f32c(covs, "covs")
    M = means.numel() // 3
    if covs.numel() != 9 * M:
        raise ValueError("parameterization: covs must be [..., 3, 3] full covariances")
    mo, co = torch.empty_like(means), torch.empty_like(covs)
    L.check(L.lib().mipnerf_gauss_360(M, 0, 1, 1, _ptr(means), _ptr(covs), None, L.PREC_FP32, _ptr(mo), _ptr(co), _stream()),
            "parameterization")
    return mo, co


def contract(x):
    """models/mip.py:424-426: x inside the unit ball, (2 - 1/|x|) x/|x| outside (mip-NeRF 360 eq. 10); x [..., 3]."""
    x = _f32c(x, "x")
    M = x.numel() // 3
    out = torch.empty_like(x)
    zero = torch.zeros(M, 9, device=x.device, dtype=torch.float32)
    L.check(L.lib().mipnerf_gauss_360(M, 0, 1, 1, _ptr(x), _ptr(zero), None, L.PREC_FP32, _ptr(out), None, _stream()), "contract")
    return out


def integrated_pos_enc_360(means_covs, min_deg=0, max_deg=1, contracted=True, precision=L.PREC_FP32):
    """models/mip.py:292-319 done right: off-axis integrated positional encoding of (means [...,3], covs [...,3,3]) on the 21
    icosahedron directions at the frequencies 2^min_deg .. 2^(max_deg-1) (the dead upstream code has a single frequency =
    the defaults here), contracting the Gaussians first like its `parameterization` call: [..., 2*21*(max_deg-min_deg)]."""
    means, covs = means_covs
    means, covs = _f32c(means, "means"), _f32c(covs, "covs")
    M = means.numel() // 3
    enc = torch.empty(*means.shape[:-1], 42 * (max_deg - min_deg), device=means.device, dtype=_torch_dtype(precision))
    L.check(L.lib().mipnerf_gauss_360(M, min_deg, max_deg, int(bool(contracted)), _ptr(means), _ptr(covs), _ptr(enc), precision,
                                      None, None, _stream()), "integrated_pos_enc_360")
    return enc


# ---- geometry out of a trained field (csrc/kernels_mesh.hip) -------------------------------------------------------------
def _lattice_args(name, dims, lo, hi):
    import ctypes as C
    dims = [int(d) for d in (dims if hasattr(dims, "__len__") else (dims,) * 3)]
    lo = [float(v) for v in (lo if hasattr(lo, "__len__") else (lo,) * 3)]
    hi = [float(v) for v in (hi if hasattr(hi, "__len__") else (hi,) * 3)]
    if len(dims) != 3 or len(lo) != 3 or len(hi) != 3:
        raise ValueError(f"{name}: dims, lo and hi have three entries, in (x, y, z) order")
    return dims, (C.c_int32 * 3)(*dims), (C.c_float * 3)(*lo), (C.c_float * 3)(*hi)


def _field_mlp(mlp_or_model, name, space=None):
    """The MLP of a system / MipNerf / MLP.  `space` None: the bounded model; the unbounded-scene model is refused (its field lives in a
    contracted space, so its lattice has to name one).  `space` 'world' / 'contracted': the unbounded-scene model, and nothing else."""
    m = getattr(mlp_or_model, "mip_nerf", mlp_or_model)
    mlp = getattr(m, "mlp", m)
    unbounded = bool(getattr(m, "unbounded", False) or getattr(mlp, "_cfg_extra", {}).get("unbounded", 0))
    if space is not None and space not in L.SPACES:
        raise ValueError(f"{name}: space must be None, 'world' or 'contracted', got {space!r}")
    if unbounded and space is None:
        raise NotImplementedError(f"{name}: unbounded=True models are not supported (meshing a contracted space is a different question) "
                                  "unless the lattice names its space: space='world' or space='contracted'")
    if space is not None and not unbounded:
        raise ValueError(f"{name}: space={space!r} belongs to unbounded=True models; a bounded model's lattice lies in world space as it is")
    if not hasattr(mlp, "native"):
        raise TypeError(f"{name}: expected a MipNeRFSystem, MipNerf or MLP, got {type(mlp_or_model).__name__}")
    return mlp


def density_grid(mlp_or_model, dims, lo, hi, cov_scale=1.0, precision=None, chunk=None, space=None, far_radius=64.0):
    """Activated density of the field on a lattice of dims = (nx, ny, nz) Gaussians over the box lo .. hi: `sigma` [nz, ny, nx] fp32.
    Point (i, j, k) has the mean lo + float32(i) * h, h = (hi - lo) / float32(n - 1), and the diagonal covariance cov_scale * h * h / 12
    (cov_scale = 0: a point query); the view branch runs on a zero view encoding.  `precision`: L.PREC_FP32 / L.PREC_BF16 or 'fp32' /
    'bf16' (default: the model's).  `chunk`: lattice points per MLP launch (default 2^18); the result does not depend on it.
    `space` (unbounded=True models only, which need it): 'world' -- the lattice lies in world coordinates and each Gaussian is contracted
    before it is encoded -- or 'contracted' -- the lattice is uniform in the contracted coordinates (the whole scene lies in |z| < 2) and
    points beyond |z| = 2 - 1 / far_radius get the density 0; the rules are those of include/mipnerf_hip.h (mipnerf_density_grid_360)."""
    mlp = _field_mlp(mlp_or_model, "density_grid", space)
    dev = next(mlp.parameters()).device
    if dev.type != "cuda":
        raise RuntimeError(f"density_grid: the MI355X-native path needs the model on a HIP device (it is on {dev}); there is no CPU fallback")
    prec = mlp.precision if precision is None else {"fp32": L.PREC_FP32, "bf16": L.PREC_BF16}.get(precision, precision)
    dims, cdims, clo, chi = _lattice_args("density_grid", dims, lo, hi)
    n = dims[0] * dims[1] * dims[2]
    chunk = min(max(n, 1), 1 << 18) if chunk is None else int(chunk)
    if chunk < 1:
        raise ValueError("density_grid: chunk must be positive")
    with torch.cuda.device(dev):
        ctx = mlp.native(dev)
        sizer = L.lib().mipnerf_density_grid_workspace_bytes if space is None else L.lib().mipnerf_density_grid_360_workspace_bytes
        need = int(sizer(ctx.handle, chunk, prec))
        if need == 0:
            if space is not None and prec in (L.PREC_FP32, L.PREC_BF16):
                raise NotImplementedError("density_grid: this unbounded model's architecture has no lattice kernel at the requested precision")
            raise ValueError(f"density_grid: unknown precision {precision!r}")
        ws = ctx.scratch("density_grid", need)
        sigma = torch.empty(max(dims[2], 0), max(dims[1], 0), max(dims[0], 0), device=dev, dtype=torch.float32)
        if space is None:
            L.check(L.lib().mipnerf_density_grid(ctx.handle, cdims, clo, chi, float(cov_scale), prec, _ptr(sigma), _ptr(ws), need, _stream()),
                    "density_grid")
        else:
            L.check(L.lib().mipnerf_density_grid_360(ctx.handle, cdims, clo, chi, float(cov_scale), L.SPACES[space], float(far_radius), prec,
                                                     _ptr(sigma), _ptr(ws), need, _stream()), "density_grid")
    return sigma


# ---- the density lattice as the proposal level of a forward (csrc/kernels_proposal.hip) ------------------------------------------
class ProposalGrid:
    """An fp32 device lattice [nz, ny, nx] over the box lo .. hi ((x, y, z) order; the layout of `density_grid`) that stands in for the
    coarse level's density: `lattice_density`, `MipNerf._forward_native(proposal=)`, `model.GraphedFrame` / `CulledFrame(proposal=)`.
    Keeps the host arrays `dims`, `lo`, `hi` the C ABI reads (`cdims`, `clo`, `chi`) next to the tensor.  The lattice must stay alive and in
    place while a captured frame uses it; a frame handed ANOTHER ProposalGrid object re-captures."""

    def __init__(self, lattice, lo, hi):
        g = _f32c(lattice, "lattice")
        if g.dim() != 3:
            raise ValueError(f"ProposalGrid: expected a [nz, ny, nx] lattice, got {tuple(g.shape)}")
        dims, self.cdims, self.clo, self.chi = _lattice_args("ProposalGrid", (g.shape[2], g.shape[1], g.shape[0]), lo, hi)
        if min(dims) < 2:
            raise ValueError(f"ProposalGrid: a lattice needs at least 2 points per axis (got {dims})")
        self.lattice, self.dims = g, tuple(dims)
        self.lo, self.hi = tuple(float(v) for v in self.clo), tuple(float(v) for v in self.chi)
        if not all(h > l for l, h in zip(self.lo, self.hi)):
            raise ValueError(f"ProposalGrid: the box needs hi > lo on every axis (got {self.lo} .. {self.hi})")


def _refuse_proposal_model(model, name, grid=None):
    """A lattice proposal replaces the coarse level of a two-level model, and the grid's type says which: a `ProposalGrid` (or no grid: the
    two-argument call of before) goes with a bounded model, a `ProposalGrid360` with an unbounded=True one.  Every mismatch is refused."""
    unbounded = bool(getattr(model, "unbounded", False))
    if isinstance(grid, ProposalGrid360):
        if not unbounded:
            raise NotImplementedError(f"{name}: a ProposalGrid360 lies in the contracted space of unbounded=True models; this model is "
                                      "bounded (its lattice is ops.field_proposal's ProposalGrid)")
    elif unbounded:
        raise NotImplementedError(f"{name}: unbounded=True models are not supported by a ProposalGrid (their field lives in a contracted "
                                  "space): they take the ProposalGrid360 of ops.field_proposal_360")
    if int(getattr(model, "num_levels", 2)) != 2:
        raise NotImplementedError(f"{name}: the lattice replaces the coarse level of a two-level model (num_levels = {model.num_levels})")


def field_proposal(model_or_system, grid=256, lo=None, hi=None, cov_scale=1.0, precision=None):
    """`density_grid` of the field on grid^3 (or (nx, ny, nz)) points over lo .. hi, wrapped into a `ProposalGrid`.  unbounded=True
    models are refused (their field lives in a contracted space: `field_proposal_360`)."""
    try:
        _field_mlp(model_or_system, "field_proposal")
    except NotImplementedError as e:
        raise NotImplementedError(f"{e}; for a proposal lattice of such a model: field_proposal_360") from None
    if lo is None or hi is None:
        raise ValueError("field_proposal: give the box lo .. hi the lattice spans (the rays to be rendered should stay inside it: outside, a "
                         "sample takes the value of the nearest face)")
    return ProposalGrid(density_grid(model_or_system, grid, lo, hi, cov_scale=cov_scale, precision=precision), lo, hi)


def lattice_density(grid, t_samples, origins, directions, radii):
    """The proposal level on its own (mipnerf_lattice_density): the trilinear value of `grid` (a `ProposalGrid`) at the mean of every
    conical frustum [t_i, t_{i+1}] -- the means `cast_rays` returns, bit for bit -- as [B, N].  A point outside the box takes the edge
    value, a non-finite one 0 (the rules of include/mipnerf_hip.h)."""
    t_samples = _f32c(t_samples, "t_samples")
    B, N1 = t_samples.shape
    out = torch.empty(B, N1 - 1, 4, device=t_samples.device, dtype=torch.float32)
    o, d, r = _f32c(origins, "origins"), _f32c(directions, "directions"), _f32c(radii, "radii")
    with torch.cuda.device(t_samples.device):
        L.check(L.lib().mipnerf_lattice_density(grid.cdims, grid.clo, grid.chi, _ptr(grid.lattice), B, N1 - 1, _ptr(t_samples), _ptr(o), _ptr(d),
                                                _ptr(r), _ptr(out), _stream()), "lattice_density")
    return out[..., 3]


# ---- the proposal density of the unbounded-scene model: a pyramid of contracted lattices (csrc/kernels_proposal_360.hip) -----------
class ProposalGrid360:
    """A pyramid of 1 .. 4 fp32 device lattices [nz_l, ny_l, nx_l] (finest first; the layout of `density_grid`), all over the box lo .. hi
    of the CONTRACTED space, that stands in for the coarse level's density of an unbounded=True model: `lattice_density_360` reads, per
    sample, the level(s) whose spacing matches the sample's own contracted covariance (include/mipnerf_proposal_360.h, rules Q1 - Q4).
    Not a `ProposalGrid`: `space` is 'contracted', `far_radius` is the radius the levels were baked with (beyond |z| = 2 - 1 / far_radius
    their density is 0) and `footprint` scales the yardstick that picks the level (0: always level 0).  Keeps the host struct the C ABI
    reads (`cpyramid`) next to the tensors, which must stay alive and in place while it is in use."""

    space = "contracted"

    def __init__(self, lattices, lo, hi, far_radius, footprint=1.0):
        lattices = [lattices] if torch.is_tensor(lattices) else list(lattices)
        if not 1 <= len(lattices) <= L.PROPOSAL_MAX_LEVELS:
            raise ValueError(f"ProposalGrid360: a pyramid has 1 .. {L.PROPOSAL_MAX_LEVELS} levels (got {len(lattices)})")
        self.lattices = [_f32c(g, "lattice") for g in lattices]
        _, _, clo, chi = _lattice_args("ProposalGrid360", (2, 2, 2), lo, hi)
        self.lo, self.hi = tuple(float(v) for v in clo), tuple(float(v) for v in chi)
        if not all(h > l for l, h in zip(self.lo, self.hi)):
            raise ValueError(f"ProposalGrid360: the box needs hi > lo on every axis (got {self.lo} .. {self.hi})")
        self.far_radius, self.footprint = float(far_radius), float(footprint)
        if not self.far_radius > 1.0:
            raise ValueError(f"ProposalGrid360: far_radius must exceed 1, the radius of the uncontracted ball (got {far_radius})")
        if not (self.footprint >= 0.0 and self.footprint < float("inf")):
            raise ValueError(f"ProposalGrid360: footprint must be finite and >= 0 (got {footprint})")
        self.dims, self.spacing = [], []
        self.cpyramid = L.ProposalPyramid()
        self.cpyramid.levels = len(self.lattices)
        span = torch.tensor(self.hi, dtype=torch.float32) - torch.tensor(self.lo, dtype=torch.float32)
        for l, g in enumerate(self.lattices):
            if g.dim() != 3 or min(g.shape) < 2:
                raise ValueError(f"ProposalGrid360: level {l}: expected a [nz, ny, nx] lattice with at least 2 points per axis, got {tuple(g.shape)}")
            dims = (g.shape[2], g.shape[1], g.shape[0])
            self.dims.append(dims)
            self.spacing.append(float((span / (torch.tensor(dims, dtype=torch.float32) - 1.0)).max()))       # fp32, as the library forms it
            if l > 0 and not self.spacing[l] > self.spacing[l - 1]:
                raise ValueError(f"ProposalGrid360: the spacing must increase strictly from level to level (level {l}: {self.spacing[l]} "
                                 f"after {self.spacing[l - 1]})")
            for a in range(3):
                self.cpyramid.dims[l][a] = dims[a]
            self.cpyramid.lattice[l] = g.data_ptr()
        for a in range(3):
            self.cpyramid.lo[a], self.cpyramid.hi[a] = self.lo[a], self.hi[a]

    def __len__(self):
        return len(self.lattices)


def proposal_ladder_360(grid, levels):
    """Points per axis of the levels of `field_proposal_360`: n_0 = grid, n_l = max(2, ((n_{l-1} - 1) >> 1) + 1) -- every other point of the
    level below when n - 1 is even.  A level that would repeat the one below (the ladder has reached 2 points) is an error."""
    grid, levels = int(grid), int(levels)
    if not 1 <= levels <= L.PROPOSAL_MAX_LEVELS:
        raise ValueError(f"field_proposal_360: levels must be in 1 .. {L.PROPOSAL_MAX_LEVELS} (got {levels})")
    if grid < 2:
        raise ValueError(f"field_proposal_360: a lattice needs at least 2 points per axis (got {grid})")
    n = [grid]
    for l in range(1, levels):
        n.append(max(2, ((n[-1] - 1) >> 1) + 1))
        if n[-1] >= n[-2]:
            raise ValueError(f"field_proposal_360: grid = {grid} has no level {l}: the ladder {n[:-1]} ends at {n[-2]} points per axis")
    return n


def field_proposal_360(model_or_system, grid=256, levels=1, far_radius=64.0, bound=2.0, cov_scale=1.0, footprint=1.0, precision=None):
    """A `ProposalGrid360` of an unbounded=True model's own density: level l is ONE `density_grid(..., space='contracted', far_radius=,
    cov_scale=)` call on n_l^3 points (`proposal_ladder_360`) over [-bound, bound]^3 at its own spacing -- a coarser lattice baked at its own
    lattice Gaussian is the field pre-filtered at that spacing by the model's own encoding, so there is no bake code of its own.
    `levels` = 1 and `footprint` = 1 are choices, not measurements."""
    _field_mlp(model_or_system, "field_proposal_360", "contracted")
    ladder = proposal_ladder_360(grid, levels)
    bound = float(bound)
    if not bound > 0.0:
        raise ValueError(f"field_proposal_360: the half-width of the box must be positive (got {bound})")
    lattices = [density_grid(model_or_system, n, -bound, bound, cov_scale=cov_scale, precision=precision, space="contracted",
                             far_radius=far_radius) for n in ladder]
    return ProposalGrid360(lattices, -bound, bound, far_radius, footprint)


def lattice_density_360(grid, t_samples, origins, directions, radii):
    """The proposal density of the unbounded-scene model on its own (mipnerf_lattice_density_360): per conical frustum [t_i, t_{i+1}] the
    value of `grid` (a `ProposalGrid360`) at the contracted Gaussian `cast_rays_360(contracted=True)` returns -- the trilinear value of the
    level its covariance selects at its mean, mixed with the next level's in between two spacings -- as [B, N].  A non-finite mean gives 0
    (the rules of include/mipnerf_proposal_360.h)."""
    if not isinstance(grid, ProposalGrid360):
        raise TypeError(f"lattice_density_360: expected a ProposalGrid360, got {type(grid).__name__}")
    t_samples = _f32c(t_samples, "t_samples")
    B, N1 = t_samples.shape
    out = torch.empty(B, N1 - 1, 4, device=t_samples.device, dtype=torch.float32)
    o, d, r = _f32c(origins, "origins"), _f32c(directions, "directions"), _f32c(radii, "radii")
    import ctypes as C
    with torch.cuda.device(t_samples.device):
        L.proposal_360_check(L.proposal_360_lib().mipnerf_lattice_density_360(C.byref(grid.cpyramid), grid.footprint, B, N1 - 1, _ptr(t_samples),
                                                                              _ptr(o), _ptr(d), _ptr(r), _ptr(out), _stream()),
                             "lattice_density_360")
    return out[..., 3]


def reciprocal_360(t_inv, out=None):
    """t = 1 / t_inv per fence post (mipnerf_reciprocal_360): the bits of the native forward's own step between the inverse-depth
    resampling and the fine level's encoding."""
    t_inv = _f32c(t_inv, "t_inv")
    out = torch.empty_like(t_inv) if out is None else out
    with torch.cuda.device(t_inv.device):
        L.proposal_360_check(L.proposal_360_lib().mipnerf_reciprocal_360(t_inv.numel(), _ptr(t_inv), _ptr(out), _stream()), "reciprocal_360")
    return out


def lattice_ipe_360(dims, lo, hi, cov_scale=1.0, space="contracted", min_deg=0, max_deg=16, precision=L.PREC_FP32, fragments=False,
                    first=0, count=None, device="cuda"):
    """The lattice encoder of the unbounded-scene model alone (mipnerf_lattice_ipe_360): rows [count, 42 * (max_deg - min_deg)] of the
    lattice points first .. first + count - 1, fp32 or bf16; fragments=True (bf16): the MFMA B-operand fragment layout, an opaque
    [ceil(count / 256) * 256, features] buffer.  The bits of `integrated_pos_enc_360` on the Gaussians the header states."""
    if space not in L.SPACES:
        raise ValueError(f"lattice_ipe_360: space must be 'world' or 'contracted', got {space!r}")
    dims, cdims, clo, chi = _lattice_args("lattice_ipe_360", dims, lo, hi)
    count = dims[0] * dims[1] * dims[2] - first if count is None else int(count)
    if fragments and precision != L.PREC_BF16:
        raise ValueError("lattice_ipe_360(fragments=True) is a bf16 layout")
    rows = (count + 255) // 256 * 256 if fragments else count
    enc = torch.empty(max(rows, 0), 42 * (max_deg - min_deg), device=device, dtype=_torch_dtype(precision))
    with torch.cuda.device(enc.device):
        L.check(L.lib().mipnerf_lattice_ipe_360(cdims, clo, chi, int(first), count, float(cov_scale), L.SPACES[space], min_deg, max_deg,
                                                _ptr(enc), L.OUT_BF16_FRAGMENTS if fragments else precision, _stream()), "lattice_ipe_360")
    return enc


def uncontract(points, normals=None, far_radius=64.0):
    """The way back from the contracted space: points z [..., 3] -> x with contract(x) = z, |z| capped at 2 - 1 / far_radius so that no
    result lies beyond far_radius.  With `normals` (density-gradient directions of the contracted space at those points) returns
    (x, world normals): J^T g normalised, (0, 0, 0) staying (0, 0, 0).  The rules are those of include/mipnerf_hip.h."""
    z = _f32c(points, "points")
    g = None if normals is None else _f32c(normals, "normals")
    if g is not None and g.shape != z.shape:
        raise ValueError("uncontract: one normal per point")
    V = z.numel() // 3
    x = torch.empty_like(z)
    nw = None if g is None else torch.empty_like(g)
    with torch.cuda.device(z.device):
        L.check(L.lib().mipnerf_uncontract_vertices(V, float(far_radius), _ptr(z), _ptr(g), _ptr(x), _ptr(nw), _stream()), "uncontract")
    return x if g is None else (x, nw)


def field_at(mlp_or_model, points, variances, viewdirs, precision=None, space=None):
    """The field at given Gaussians: points [M, 3], variances [M] (one isotropic variance per point) or [M, 3], unit view directions
    [M, 3] -> rgb_sigma [M, 4] = (r, g, b, sigma) activated.  mipnerf_integrated_pos_enc + mipnerf_pos_enc + mipnerf_mlp_forward with one
    sample per ray: the calls the renderer's per-stage path makes, no second path.
    `space` (unbounded=True models only, which need it): the points and variances are given in that lattice space -- 'world': each
    Gaussian is contracted, then encoded; 'contracted': encoded as given (mipnerf_gauss_360 either way).  The view directions are always
    world directions."""
    mlp = _field_mlp(mlp_or_model, "field_at", space)
    prec = mlp.precision if precision is None else {"fp32": L.PREC_FP32, "bf16": L.PREC_BF16}.get(precision, precision)
    points = _f32c(points, "points").reshape(-1, 3)
    M = points.shape[0]
    if M == 0:
        return torch.empty(0, 4, device=points.device, dtype=torch.float32)
    var = _f32c(variances, "variances")
    var = (var.reshape(M, 1).expand(M, 3) if var.numel() == M else var.reshape(M, 3)).contiguous()
    e = mlp._cfg_extra
    min_deg = e.get("min_deg_point", 0)
    max_deg = e.get("max_deg_point", min_deg + mlp.arch["xyz_dim"] // (6 if space is None else 42))
    with torch.no_grad():
        if space is None:
            enc = integrated_pos_enc((points, var), min_deg, max_deg, precision=prec).reshape(M, 1, -1)
        else:
            enc = integrated_pos_enc_360((points, torch.diag_embed(var)), min_deg, max_deg, contracted=space == "world",
                                         precision=prec).reshape(M, 1, -1)
        venc = None
        if e.get("use_viewdirs", 1):
            venc = pos_enc(_f32c(viewdirs, "viewdirs").reshape(M, 3), 0, (mlp.arch["view_dim"] - 3) // 6, precision=prec)
        return mlp(enc, venc, precision=prec, return_activated=True)[2].reshape(M, 4)


def isosurface(grid, threshold, lo, hi, return_edges=False):
    """Marching tetrahedra (Kuhn split) of any fp32 device lattice `grid` [nz, ny, nx] over the box lo .. hi ((x, y, z) order): inside is
    grid > threshold.  Returns (vertices [V, 3] fp32, normals [V, 3] fp32, faces [F, 3] int32[, vertex_edges [V, 2] int64]) on the device;
    the rules and the orders are those of include/mipnerf_hip.h (mipnerf_isosurface_count / _emit).  The vertex count has to reach the
    host, so the call synchronises the stream and cannot be captured into a graph."""
    import ctypes as C
    g = _f32c(grid, "grid")
    if g.dim() != 3:
        raise ValueError(f"isosurface: expected a [nz, ny, nx] lattice, got {tuple(g.shape)}")
    dims, cdims, clo, chi = _lattice_args("isosurface", (g.shape[2], g.shape[1], g.shape[0]), lo, hi)
    dev = g.device
    with torch.cuda.device(dev):
        need = int(L.lib().mipnerf_isosurface_workspace_bytes(*dims))
        ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
        nv, nf = C.c_int64(0), C.c_int64(0)
        L.check(L.lib().mipnerf_isosurface_count(cdims, _ptr(g), float(threshold), _ptr(ws), need, C.byref(nv), C.byref(nf), _stream()),
                "isosurface_count")
        V, F = int(nv.value), int(nf.value)
        vertices = torch.empty(V, 3, device=dev, dtype=torch.float32)
        normals = torch.empty(V, 3, device=dev, dtype=torch.float32)
        faces = torch.empty(F, 3, device=dev, dtype=torch.int32)
        edges = torch.empty(V, 2, device=dev, dtype=torch.int64) if return_edges else None
        if V:
            L.check(L.lib().mipnerf_isosurface_emit(cdims, clo, chi, _ptr(g), float(threshold), _ptr(ws), need, _ptr(vertices), _ptr(normals),
                                                    _ptr(faces) if F else None, _ptr(edges), _stream()), "isosurface_emit")
    return (vertices, normals, faces, edges) if return_edges else (vertices, normals, faces)


# ---- empty-space skipping for whole frames (csrc/kernels_occupancy.hip) ----------------------------------------------------
class Occupancy:
    """Occupancy bits of a lattice (include/mipnerf_hip.h, mipnerf_occupancy_build): `bits` uint32 on the device
    [nz - 1, ny - 1, ceil((nx - 1) / 32)], cell i of an x row is bit i & 31 of word i >> 5, padding bits are 0; `dims` =
    (nx, ny, nz) lattice POINTS, `lo` / `hi` the box in (x, y, z) order, h = (hi - lo) / float(n - 1).  `space`: None -- the box lies in
    world coordinates (the bounded model) -- or 'contracted' -- in the contracted coordinates of the unbounded-scene model;
    `ray_occupancy` / `ray_span` / `model.CulledFrame` dispatch on it.  Attributes `threshold` / `dilate`: what the bits were built with
    (None when unknown; `occupancy_grid` sets them); `occupancy_refresh` rebuilds the bits with these."""
    threshold = None
    dilate = None

    def __init__(self, bits, dims, lo, hi, space=None):
        if space not in (None, "contracted"):
            raise ValueError(f"Occupancy: space must be None or 'contracted', got {space!r}")
        self.bits, self.dims, self.lo, self.hi = bits, tuple(int(d) for d in dims), tuple(float(v) for v in lo), tuple(float(v) for v in hi)
        self.space = space

    @property
    def cells(self):
        return tuple(d - 1 for d in self.dims)

    def occupied_fraction(self) -> float:
        """Share of the cells that are occupied (a host read-back of the words)."""
        import numpy as np
        words = self.bits.cpu().numpy()
        count = int(np.unpackbits(words.view(np.uint8)).sum())
        cx, cy, cz = self.cells
        return count / float(cx * cy * cz)


def occupancy_grid(lattice, threshold, lo, hi, dilate=1):
    """Occupancy bits of any fp32 device lattice [nz, ny, nx] over the box lo .. hi ((x, y, z) order, the conventions of `isosurface`):
    cell (i, j, k) is raw-occupied iff any of its 8 corner values is > threshold or is NaN; a cell is occupied iff a raw-occupied cell lies
    within Chebyshev distance `dilate` (>= 0) of it.  Returns an `Occupancy`.  No atomics: two runs give the same bytes."""
    g = _f32c(lattice, "lattice")
    if g.dim() != 3:
        raise ValueError(f"occupancy_grid: expected a [nz, ny, nx] lattice, got {tuple(g.shape)}")
    dims, cdims, clo, chi = _lattice_args("occupancy_grid", (g.shape[2], g.shape[1], g.shape[0]), lo, hi)
    dilate = int(dilate)
    with torch.cuda.device(g.device):
        words = int(L.lib().mipnerf_occupancy_words(*dims))
        if words == 0:
            raise ValueError(f"occupancy_grid: a lattice needs at least 2 points per axis and 7 nx ny nz < 2^31 (got {dims})")
        shape = (dims[2] - 1, dims[1] - 1, (dims[0] - 1 + 31) // 32)
        bits = torch.empty(shape, dtype=torch.uint32, device=g.device)
        scratch = torch.empty(shape, dtype=torch.uint32, device=g.device) if dilate > 0 else None
        L.check(L.lib().mipnerf_occupancy_build(cdims, _ptr(g), float(threshold), dilate, _ptr(bits), _ptr(scratch), _stream()),
                "occupancy_build")
    occ = Occupancy(bits, dims, [float(v) for v in clo], [float(v) for v in chi])
    occ.threshold, occ.dilate = float(threshold), dilate
    return occ


def occupancy_refresh(occ, fresh, running, decay, scratch=None):
    """The grid of a field that is still training (include/mipnerf_hip.h, mipnerf_occupancy_refresh), IN PLACE: `running` (fp32 device
    lattice [nz, ny, nx] of `occ.dims`) becomes max(decay * running, fresh) per point -- a NaN of `fresh` is kept, a NaN of decay * running
    replaced by `fresh` --, then `occ.bits` becomes what `occupancy_grid(running, occ.threshold, ..., dilate=occ.dilate)` holds.  The bits
    tensor keeps its storage (a captured graph that reads it sees the new grid at its next replay).  `scratch`: uint32 words of the shape of
    `occ.bits`, needed when occ.dilate > 0 (allocated when None, which a graph capture must avoid).  Returns `occ`."""
    if occ.threshold is None or occ.dilate is None:
        raise ValueError("occupancy_refresh: the Occupancy does not say which threshold and dilate its bits were built with "
                         "(set occ.threshold and occ.dilate)")
    nx, ny, nz = occ.dims
    for name, t in (("fresh", fresh), ("running", running)):
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() and tuple(t.shape) == (nz, ny, nx)):
            raise ValueError(f"occupancy_refresh: {name} must be a contiguous fp32 device lattice [nz, ny, nx] = {(nz, ny, nx)}")
    bits = occ.bits
    if not (bits.dtype == torch.uint32 and bits.is_contiguous() and tuple(bits.shape) == (nz - 1, ny - 1, (nx - 1 + 31) // 32)):
        raise ValueError("occupancy_refresh: occ.bits does not have the words of occ.dims")
    _, cdims, _, _ = _lattice_args("occupancy_refresh", occ.dims, occ.lo, occ.hi)
    with torch.cuda.device(bits.device):
        if occ.dilate > 0 and scratch is None:
            scratch = torch.empty_like(bits)
        if scratch is not None and (scratch.dtype != torch.uint32 or scratch.numel() < bits.numel() or not scratch.is_contiguous()):
            raise ValueError("occupancy_refresh: scratch holds as many uint32 words as occ.bits")
        L.check(L.lib().mipnerf_occupancy_refresh(cdims, _ptr(fresh), _ptr(running), float(decay), float(occ.threshold), int(occ.dilate), _ptr(bits),
                                                  _ptr(scratch), _stream()), "occupancy_refresh")
    return occ


def field_occupancy(model_or_system, grid=128, lo=None, hi=None, threshold=0.01, dilate=1, cov_scale=1.0, precision=None, space=None,
                    far_radius=64.0):
    """`density_grid` of the field on grid^3 (or (nx, ny, nz)) points over lo .. hi, then `occupancy_grid` of it.  The threshold is a
    density and scene dependent, like the mesh threshold.  unbounded=True models are refused (their field lives in a contracted space)
    unless `space='contracted'` names it: the lattice is then `density_grid(space='contracted', far_radius=far_radius)` over lo .. hi
    (default [-2, 2]^3, the whole contracted space) and the result is tagged `space='contracted'`.  The density is 0 beyond
    |z| = 2 - 1 / far_radius, so `far_radius` must be no smaller than the largest |o + far d| of the rays to be classified.
    `space='world'` is refused: a world box cannot hold an unbounded ray."""
    if space == "world":
        raise ValueError("field_occupancy: space='world' is not supported: a world box cannot hold an unbounded ray (its far end lies anywhere); "
                         "use space='contracted'")
    _field_mlp(model_or_system, "field_occupancy", space)
    if space is None:
        if lo is None or hi is None:
            raise ValueError("field_occupancy: give the box lo .. hi the grid spans (the rays of the cameras to be rendered should stay inside it)")
        sigma = density_grid(model_or_system, grid, lo, hi, cov_scale=cov_scale, precision=precision)
        return occupancy_grid(sigma, threshold, lo, hi, dilate=dilate)
    if not (far_radius > 1.0 and far_radius < float("inf")):
        raise ValueError(f"field_occupancy: far_radius must be finite and > 1 (got {far_radius})")
    lo, hi = -2.0 if lo is None else lo, 2.0 if hi is None else hi
    sigma = density_grid(model_or_system, grid, lo, hi, cov_scale=cov_scale, precision=precision, space=space, far_radius=far_radius)
    occ = occupancy_grid(sigma, threshold, lo, hi, dilate=dilate)
    occ.space = space
    return occ


def _rays_ptrs(rays, n, name):
    """RaysPtrs of 7 flat fp32 device fields [n, k] plus the tensors that keep them alive"""
    keep = []
    for k, t in zip(type(rays)._fields, rays):
        t = _f32c(t, k)
        if t.shape[0] != n:
            raise ValueError(f"{name}: {k} has {t.shape[0]} rays, expected {n}")
        keep.append(t)
    return L.RaysPtrs(*[t.data_ptr() for t in keep]), keep


def _contracted_grid(occ, disparity, name):
    """whether `occ` lies in the contracted space of the unbounded-scene model (whose rays are sampled in inverse depth: no disparity flag)"""
    contracted = getattr(occ, "space", None) == "contracted"
    if contracted and disparity:
        raise ValueError(f"{name}: disparity=True does not apply to a grid in the contracted space (the unbounded-scene model samples in "
                         "inverse depth)")
    return contracted


def _classify_rays(name, occ, rays, n, num_samples, disparity, outside_occupied, cone_scale, contracted, outs):
    """the call `ray_occupancy` and `ray_span` share: mipnerf_<name> (or, for a contracted grid, mipnerf_<name>_360, which takes no disparity
    flag) on n > 0 rays with the output tensors `outs`"""
    import ctypes as C
    _, cdims, clo, chi = _lattice_args(name, occ.dims, occ.lo, occ.hi)
    fn = name + "_360" if contracted else name
    flags = () if contracted else (int(bool(disparity)),)
    with torch.cuda.device(occ.bits.device):
        rp, keep = _rays_ptrs(rays, n, name)
        L.check(getattr(L.lib(), "mipnerf_" + fn)(cdims, clo, chi, _ptr(occ.bits), n, int(num_samples), C.byref(rp), *flags,
                                                  int(bool(outside_occupied)), float(cone_scale), *[_ptr(t) for t in outs], _stream()), fn)


def ray_occupancy(occ, rays, num_samples, disparity=False, outside_occupied=True, cone_scale=1.0, out=None):
    """live uint8 [n]: 1 where some coarse frustum of the ray touches an occupied cell of `occ`.  Frustum i of the coarse level's
    deterministic fence posts t_0 .. t_N has the end points p0 = o + t_i d, p1 = o + t_{i+1} d, the half-width rho = cone_scale * radii *
    t_{i+1}, per axis the bounding interval [min(p0, p1) - rho, max(p0, p1) + rho] and the cell range floor((x - lo) / h), inclusive at both
    ends; the part of a range outside the grid counts as occupied when `outside_occupied`, otherwise it is clipped away.  `rays`: flat
    [n, k] device rays.
    A grid with `occ.space == 'contracted'` (the unbounded-scene model): the fence posts are the inverse-depth ones of `sample_t_360` and
    each frustum's image under `contract` is bounded by the closed form of include/mipnerf_hip.h (mipnerf_ray_occupancy_360);
    `disparity=True` is refused."""
    contracted = _contracted_grid(occ, disparity, "ray_occupancy")
    n = int(rays.origins.shape[0])
    dev = occ.bits.device
    live = torch.empty(n, dtype=torch.uint8, device=dev) if out is None else out
    if live.dtype != torch.uint8 or live.numel() != n or not live.is_contiguous():
        raise ValueError("ray_occupancy: out must be a contiguous uint8 tensor with one byte per ray")
    if n == 0:
        return live
    _classify_rays("ray_occupancy", occ, rays, n, num_samples, disparity, outside_occupied, cone_scale, contracted, (live,))
    return live


def ray_span(occ, rays, num_samples, disparity=False, outside_occupied=True, cone_scale=1.0, out=None):
    """(live uint8 [n], first int32 [n], last int32 [n], near' fp32 [n, 1], far' fp32 [n, 1]): the occupied span of every ray.  "Frustum i
    hits" is exactly the per-frustum test of `ray_occupancy`, and `live` is byte for byte what `ray_occupancy` returns for the same
    arguments.  first = the smallest hitting frustum index, last = the largest; near' = t_first and far' = t_{last + 1} are the coarse
    level's deterministic fence posts themselves, bit for bit those of the sampler.  A dead ray gets first = N, last = -1, near' = near and
    far' = far.  `out`: a tuple of five preallocated tensors of those types (an entry of first / last / near' / far' may be None: it is
    skipped and returned as None).  The frusta cover [near, far] for any N, so the span found with one `num_samples` is valid for a renderer
    that uses another.  A ray rendered on [near', far'] is NOT the ray rendered on [near, far]: its samples sit elsewhere; what it leaves
    out lies only in cells whose 8 lattice corners are at or below the threshold, after dilation.
    A grid with `occ.space == 'contracted'`: the rules of `ray_occupancy` for such a grid (mipnerf_ray_span_360); near' / far' are the fence
    posts of `sample_t_360`, bit for bit, and `disparity=True` is refused."""
    contracted = _contracted_grid(occ, disparity, "ray_span")
    n = int(rays.origins.shape[0])
    dev = occ.bits.device
    if out is None:
        out = (torch.empty(n, dtype=torch.uint8, device=dev), torch.empty(n, dtype=torch.int32, device=dev),
               torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, 1, device=dev), torch.empty(n, 1, device=dev))
    if len(out) != 5 or out[0] is None:
        raise ValueError("ray_span: out is (live, first, last, near, far); only the last four may be None")
    for t, dt in zip(out, (torch.uint8, torch.int32, torch.int32, torch.float32, torch.float32)):
        if t is not None and (t.dtype != dt or t.numel() != n or not t.is_contiguous() or t.device != dev):
            raise ValueError("ray_span: out holds contiguous device tensors with one element per ray: uint8, int32, int32, fp32, fp32")
    if n == 0:
        return tuple(out)
    _classify_rays("ray_span", occ, rays, n, num_samples, disparity, outside_occupied, cone_scale, contracted, out)
    return tuple(out)


def compact_rays(live, rays, out_rays, out_index, workspace=None):
    """Gathers the rays with live != 0, in their original order, into the first `count` rows of `out_rays` (7 preallocated [n, k] fp32
    fields) and writes the source ray of compact slot j to out_index[j] (int32 [n]).  Returns `count`.  The count has to reach the host:
    one 8-byte read-back and one stream synchronisation per call, which is why the call cannot be captured into a graph."""
    import ctypes as C
    n = int(live.numel())
    if live.dtype != torch.uint8 or not live.is_contiguous() or out_index.dtype != torch.int32 or out_index.numel() < n:
        raise ValueError("compact_rays: live is uint8 [n], out_index int32 [n]")
    if n == 0:
        return 0
    with torch.cuda.device(live.device):
        need = int(L.lib().mipnerf_compact_rays_workspace_bytes(n))
        ws = torch.empty(need, dtype=torch.uint8, device=live.device) if workspace is None else workspace
        rp, keep = _rays_ptrs(rays, n, "compact_rays")
        op, keep_out = _rays_ptrs(out_rays, n, "compact_rays")
        for a, b in zip(out_rays, keep_out):
            if a.data_ptr() != b.data_ptr():
                raise ValueError("compact_rays: out_rays must be contiguous fp32 tensors")
        count = C.c_int64(0)
        L.check(L.lib().mipnerf_compact_rays(n, _ptr(live), C.byref(rp), C.byref(op), _ptr(out_index), _ptr(ws), ws.numel(),
                                             C.byref(count), _stream()), "compact_rays")
    return int(count.value)


def scatter_frame(index, count, compact_outputs, full_outputs, live, near, white_bkgd):
    """Writes every pixel of every level once.  `compact_outputs` / `full_outputs`: per level (rgb [m, 3], distance [m], acc [m]) with
    m >= count and m = n.  Pixel index[j], j < count, takes compact slot j; a pixel with live = 0 takes what volumetric_rendering yields
    for all-zero weights: rgb = 1 with `white_bkgd` else 0, acc = 0, distance = near."""
    n = int(live.numel())
    if n == 0:
        return
    nl = len(full_outputs)
    if len(compact_outputs) != nl:
        raise ValueError("scatter_frame: compact and full outputs have different level counts")
    comp, full = (L.LevelOut * nl)(), (L.LevelOut * nl)()
    keep = []
    for l in range(nl):
        for arr, outs, rows in ((comp, compact_outputs[l], int(count)), (full, full_outputs[l], n)):
            rgb, dist, acc = outs
            for t, width in ((rgb, 3), (dist, 1), (acc, 1)):
                if t.dtype != torch.float32 or not t.is_contiguous() or not t.is_cuda or t.numel() < rows * width:
                    raise ValueError("scatter_frame: outputs are contiguous fp32 device tensors with at least `count` / n rows")
            arr[l] = L.LevelOut(rgb.data_ptr(), dist.data_ptr(), acc.data_ptr(), None, None)
            keep += [rgb, dist, acc]
    near = _f32c(near, "near")
    with torch.cuda.device(live.device):
        L.check(L.lib().mipnerf_scatter_frame(n, int(count), nl, _ptr(index), _ptr(live), _ptr(near), int(bool(white_bkgd)), comp, full,
                                              _stream()), "scatter_frame")


# ---- adaptive sample counts for whole frames (csrc/kernels_bucket.hip) ------------------------------------------------------
MAX_BUCKETS = 8
BUCKET_ALIGN = 64
LADDER_RULE = ("a ladder is 1 to 8 strictly increasing sample counts c_0 < c_1 < ... < c_{B-1} with 1 <= c_0 and c_{B-1} == num_samples")


def sample_ladder(num_samples, ladder=None):
    """The sample counts adaptive rendering chooses from, as a tuple c_0 < c_1 < ... < c_{B-1} with 1 <= c_0, c_{B-1} == num_samples and
    1 <= B <= 8.  `ladder=None`: the default ladder, the distinct values of ceil(num_samples * k / 4), k = 1..4 (32, 64, 96, 128 for 128
    samples).  A given ladder is validated against that rule and returned as a tuple of ints."""
    N = int(num_samples)
    if not 1 <= N <= L.MAX_SAMPLES:
        raise ValueError(f"sample_ladder: num_samples must be in [1, {L.MAX_SAMPLES}] (got {N})")
    if ladder is None:
        return tuple(sorted({(N * k + 3) // 4 for k in range(1, 5)}))
    try:
        lad = tuple(int(c) for c in ladder)
        exact = all(float(c) == float(i) for c, i in zip(ladder, lad))
    except (TypeError, ValueError):
        lad, exact = (), False
    if not (exact and 1 <= len(lad) <= MAX_BUCKETS and lad[0] >= 1 and all(a < b for a, b in zip(lad, lad[1:])) and lad[-1] == N):
        raise ValueError(f"sample_ladder: {LADDER_RULE} (num_samples {N}, got {ladder!r})")
    return lad


def bucket_bases(counts):
    """Where the segments of `bucket_rays` begin: base_0 = 0, base_{b+1} = round_up(base_b + count_b, 64).  Returns B + 1 values; the last
    is the number of rows the partition spans."""
    bases = [0]
    for c in counts:
        bases.append((bases[-1] + int(c) + BUCKET_ALIGN - 1) // BUCKET_ALIGN * BUCKET_ALIGN)
    return bases


def bucket_rays(live, first, last, rays, span_samples, ladder, out_rays, slot, workspace=None):
    """A stable B-way partition of the rays by the sample count their occupied span needs (include/mipnerf_hip.h, mipnerf_bucket_rays).
    S = `span_samples` (the frusta count `ray_span` found first / last with), N = ladder[-1] (the count the model renders with), `ladder`
    c_0 < c_1 < ... < c_{B-1} with 1 <= c_0, c_{B-1} == N and 1 <= B <= 8 (`sample_ladder`).  For a live ray with span [first, last]:
    need = ((last - first + 1) * N + S - 1) / S in integer division (1 <= need <= N) and bucket = the smallest b with c_b >= need; a dead
    ray has bucket -1.  A ray of bucket b is meant to be rendered with c_b samples per level on [near', far'], so its coarse spacing is at
    most the untightened ray's.  Segment b begins at base_0 = 0, base_{b+1} = round_up(base_b + count_b, 64) (`bucket_bases`); within a
    bucket the rays keep their original order.  `rays`: 7 flat [n, k] fields, read as given (pass near' / far' as near / far); `out_rays`:
    7 preallocated [n + 64 * B, k] fp32 fields, whose padding rows are never written; `slot` int32 [n]: the compact slot of every ray, -1
    for a dead one.  Returns the list of the B counts: one read-back and one stream synchronisation per call, which is why the call cannot
    be captured into a graph."""
    import ctypes as C
    n = int(live.numel())
    lad = tuple(int(c) for c in ladder)
    B = len(lad)
    if not 1 <= B <= MAX_BUCKETS:
        raise ValueError(f"bucket_rays: {LADDER_RULE}")
    if live.dtype != torch.uint8 or not live.is_contiguous():
        raise ValueError("bucket_rays: live is a contiguous uint8 tensor [n]")
    for t, name in ((first, "first"), (last, "last"), (slot, "slot")):
        if t.dtype != torch.int32 or t.numel() != n or not t.is_contiguous() or t.device != live.device:
            raise ValueError(f"bucket_rays: {name} is a contiguous int32 tensor [n] on the device of live")
    rows = n + BUCKET_ALIGN * B
    counts = (C.c_int64 * B)()
    clad = (C.c_int32 * B)(*lad)
    if n == 0:
        L.check(L.lib().mipnerf_bucket_rays(0, None, None, None, int(span_samples), lad[-1], B, clad, None, None, None, None, 0, counts, None),
                "bucket_rays")
        return [0] * B
    with torch.cuda.device(live.device):
        need = int(L.lib().mipnerf_bucket_rays_workspace_bytes(n, B))
        ws = torch.empty(max(need, 16), dtype=torch.uint8, device=live.device) if workspace is None else workspace
        rp, keep = _rays_ptrs(rays, n, "bucket_rays")
        for k, t in zip(type(out_rays)._fields, out_rays):
            if t.dtype != torch.float32 or not t.is_contiguous() or t.device != live.device or t.dim() != 2 or t.shape[0] < rows \
                    or t.shape[1] != getattr(rays, k).shape[-1]:
                raise ValueError(f"bucket_rays: out_rays.{k} must be a contiguous fp32 device tensor with at least n + 64 * B = {rows} rows")
        op = L.RaysPtrs(*[t.data_ptr() for t in out_rays])
        L.check(L.lib().mipnerf_bucket_rays(n, _ptr(live), _ptr(first), _ptr(last), int(span_samples), lad[-1], B, clad, C.byref(rp), C.byref(op),
                                            _ptr(slot), _ptr(ws), ws.numel(), counts, _stream()), "bucket_rays")
    return [int(c) for c in counts]


def gather_frame(slot, compact_outputs, full_outputs, near, white_bkgd):
    """Writes every pixel of every level once (include/mipnerf_hip.h, mipnerf_gather_frame).  `compact_outputs` / `full_outputs`: per level
    (rgb [m, 3], distance [m], acc [m]) with m = the rows of the compact buffers and m = n.  A pixel with slot >= 0 copies compact slot
    `slot` (which must lie below the rows of the compact outputs); a pixel with slot < 0 gets the dead-pixel rule of `scatter_frame`:
    rgb = 1 with `white_bkgd` else 0, acc = 0, distance = near, the ORIGINAL near."""
    n = int(slot.numel())
    if n == 0:
        return
    if slot.dtype != torch.int32 or not slot.is_contiguous() or not slot.is_cuda:
        raise ValueError("gather_frame: slot is a contiguous int32 device tensor [n]")
    nl = len(full_outputs)
    if len(compact_outputs) != nl:
        raise ValueError("gather_frame: compact and full outputs have different level counts")
    comp, full = (L.LevelOut * nl)(), (L.LevelOut * nl)()
    keep, rows = [], None
    for l in range(nl):
        for arr, outs, is_full in ((comp, compact_outputs[l], False), (full, full_outputs[l], True)):
            rgb, dist, acc = outs
            for t, width in ((rgb, 3), (dist, 1), (acc, 1)):
                if t.dtype != torch.float32 or not t.is_contiguous() or not t.is_cuda or (is_full and t.numel() < n * width):
                    raise ValueError("gather_frame: outputs are contiguous fp32 device tensors; the full ones hold n rows")
                if not is_full:
                    rows = t.numel() // width if rows is None else min(rows, t.numel() // width)
            arr[l] = L.LevelOut(rgb.data_ptr(), dist.data_ptr(), acc.data_ptr(), None, None)
            keep += [rgb, dist, acc]
    near = _f32c(near, "near")
    if near.numel() < n:
        raise ValueError("gather_frame: near holds one value per pixel")
    with torch.cuda.device(slot.device):
        L.check(L.lib().mipnerf_gather_frame(n, int(rows or 0), nl, _ptr(slot), _ptr(near), int(bool(white_bkgd)), comp if rows else None, full,
                                             _stream()), "gather_frame")


# ---------------------------------------------------------------------------------------------
# error-guided batch sampling (include/mipnerf_hip.h, mipnerf_guided_*; train_guided.TrainGuided)
# ---------------------------------------------------------------------------------------------
GUIDED_BLOCK = 256      # cells per workgroup of the refresh kernels (csrc/kernels_guided.hip): sizes the scratch words


class GuidedState:
    """The device state of one error map: `table` int64 [n_images + 1, 4] (first cell, first pixel, W, H; last row n_cells, N, 0, 0), per
    cell `err` fp32 (ones), `sum` int64 and `cnt` int32 (the bits of the uint64 / uint32 counters), `seen` uint8, `q` / `cdf` int32, the
    `scratch` words and the `header` int64 [4] = Q, A, cells visited, n_cells of the last refresh; the rings `weight` fp32 / `cell` int32
    of length `ring_len`.  `table`: a [n_images + 1, 4] integer array (`train_guided.cell_table`)."""

    def __init__(self, table, tile, ring_len, device):
        t = torch.as_tensor(table, dtype=torch.int64).reshape(-1, 4)
        if t.shape[0] < 2 or int(tile) < 1 or int(ring_len) < 1:
            raise ValueError("GuidedState: needs at least one image, tile >= 1 and ring_len >= 1")
        self.dev = torch.device(device)
        self.tile, self.ring_len = int(tile), int(ring_len)
        self.n_images, self.n_cells, self.n_pixels = t.shape[0] - 1, int(t[-1, 0]), int(t[-1, 1])
        if not 1 <= self.n_cells < (1 << 30):
            raise ValueError(f"GuidedState: the table has {self.n_cells} cells; 1 .. 2^30 - 1 are supported")
        self.table = t.to(self.dev).contiguous()
        n, z = self.n_cells, dict(device=self.dev)
        self.err = torch.ones(n, dtype=torch.float32, **z)
        self.sum = torch.zeros(n, dtype=torch.int64, **z)
        self.cnt = torch.zeros(n, dtype=torch.int32, **z)
        self.seen = torch.zeros(n, dtype=torch.uint8, **z)
        self.q = torch.zeros(n, dtype=torch.int32, **z)
        self.cdf = torch.zeros(n, dtype=torch.int32, **z)
        self.scratch = torch.zeros(2 * ((n + GUIDED_BLOCK - 1) // GUIDED_BLOCK) + 2, dtype=torch.int64, **z)
        self.header = torch.zeros(4, dtype=torch.int64, **z)
        self.weight = torch.ones(self.ring_len, dtype=torch.float32, **z)
        self.cell = torch.zeros(self.ring_len, dtype=torch.int32, **z)


def _guided_batch(who, state, rows, tensors, n_order, step, epoch_base, batch, batch_size):
    """(B, step pointer, epoch_base pointer, host batch index) of a guided_apply / guided_accumulate call, checked."""
    for name, t, dtype, width in tensors:
        if not (t.is_cuda and t.device == state.dev and t.dtype == dtype and t.is_contiguous()) or t.numel() != rows * width:
            raise ValueError(f"{who}: {name} must be a contiguous {dtype} tensor of {rows} x {width} values on {state.dev}")
    if (step is None) != (epoch_base is None):
        raise ValueError(f"{who}: step and epoch_base go together")
    for name, t in (("step", step), ("epoch_base", epoch_base)):
        if t is not None and not (t.is_cuda and t.device == state.dev and t.dtype == torch.int64 and t.numel() >= 1):
            raise ValueError(f"{who}: {name} must be an int64 tensor on {state.dev}")
    B = rows if batch_size is None else int(batch_size)
    if B != rows and (step is not None or B < rows or int(n_order) - int(batch) * B > rows):
        raise ValueError(f"{who}: a batch of {B} rays in buffers of {rows} needs a host batch index whose rays end with the order")
    return B, _ptr(step), _ptr(epoch_base), int(batch)


def guided_apply(state, lossmult, n_order, step=None, epoch_base=None, batch=0, batch_size=None):
    """lossmult[i] *= state.weight[(b * B + i) % ring_len] IN PLACE for the rays of batch b: b = step[0] - epoch_base[0] read on the device
    (capturable), or, without them, the host's `batch`.  A ray with b < 0 or b * B + i >= n_order is left alone.  `batch_size`: B when
    `lossmult` holds fewer rows (the epoch's short last batch)."""
    B, sp, ep, b = _guided_batch("guided_apply", state, lossmult.shape[0], [("lossmult", lossmult, torch.float32, 1)], n_order, step,
                                 epoch_base, batch, batch_size)
    with torch.cuda.device(state.dev):
        L.check(L.lib().mipnerf_guided_apply(B, int(n_order), state.ring_len, _ptr(state.weight), sp, ep, b, _ptr(lossmult), _stream()),
                "guided_apply")
    return lossmult


def guided_accumulate(state, rgb, gt, n_order, step=None, epoch_base=None, batch=0, batch_size=None):
    """The squared error of every ray of batch b (rgb, gt [rows, 3] fp32) into state.sum / state.cnt of the cell its ring slot names:
    integer adds, so two runs give the same bytes.  Batch index as in `guided_apply`."""
    B, sp, ep, b = _guided_batch("guided_accumulate", state, rgb.shape[0], [("rgb", rgb, torch.float32, 3), ("gt", gt, torch.float32, 3)],
                                 n_order, step, epoch_base, batch, batch_size)
    with torch.cuda.device(state.dev):
        L.check(L.lib().mipnerf_guided_accumulate(B, int(n_order), state.ring_len, _ptr(state.cell), state.n_cells, sp, ep, b, _ptr(rgb),
                                                  _ptr(gt), _ptr(state.sum), _ptr(state.cnt), _stream()), "guided_accumulate")


def guided_refresh(state, rate, mix):
    """Fold state.sum / state.cnt into state.err (rate = alpha), zero them, and rebuild state.q / state.cdf for the mixture `mix` (lambda),
    all IN PLACE; state.header receives Q, A, the cells visited since the start and n_cells.  No synchronisation."""
    with torch.cuda.device(state.dev):
        L.check(L.lib().mipnerf_guided_refresh(state.n_images, _ptr(state.table), state.tile, state.n_cells, float(rate), float(mix),
                                               _ptr(state.err), _ptr(state.sum), _ptr(state.cnt), _ptr(state.seen), _ptr(state.q),
                                               _ptr(state.cdf), _ptr(state.scratch), state.scratch.numel(), _ptr(state.header), _stream()),
                "guided_refresh")
    return state


def guided_draw(state, r, order, ring_start=0):
    """`order[j]` = the pixel id of draw j from the integers r[0, j], r[1, j] in [0, 2^32) (int64 [2, n]) and the cdf of the last refresh;
    the rings take the draw's importance weight and cell at slot (ring_start + j) % ring_len.  `order`: a contiguous int64 tensor (or
    slice) of n entries, written IN PLACE."""
    n = int(order.numel())
    for name, t, numel in (("r", r, 2 * n), ("order", order, n)):
        if not (t.is_cuda and t.device == state.dev and t.dtype == torch.int64 and t.is_contiguous() and t.numel() == numel):
            raise ValueError(f"guided_draw: {name} must be a contiguous int64 tensor of {numel} entries on {state.dev}")
    if n > state.ring_len or int(ring_start) < 0:
        raise ValueError(f"guided_draw: {n} draws do not fit a ring of {state.ring_len}")
    with torch.cuda.device(state.dev):
        L.check(L.lib().mipnerf_guided_draw(n, _ptr(r), state.n_images, _ptr(state.table), state.tile, state.n_cells, _ptr(state.cdf),
                                            _ptr(state.header), _ptr(order), _ptr(state.weight), _ptr(state.cell), state.ring_len,
                                            int(ring_start), _stream()), "guided_draw")
    return order


# ---- rendered depth fused into a truncated signed distance volume (csrc/kernels_fuse.hip, include/mipnerf_fuse.h) ---------------------
def depth_quantile(weights, t_samples, q=0.5, out=None):
    """The depth at which a ray's opacity reaches `q` (mipnerf_fuse_depth_quantile, rule D of include/mipnerf_fuse.h): `weights` [B, N] and
    `t_samples` [B, N + 1] as `MipNerf.forward` returns a level's (world distances, for the unbounded-scene model too) -> [B], or [B, Q]
    for a sequence of up to 4 quantiles.  q = 0.5 is the median depth; a ray whose weights sum to less than q has the depth +inf: `q` is an
    opacity, not a share of acc, so a ray that misses the object has no depth."""
    import ctypes as C
    single = not hasattr(q, "__len__")
    qs = [float(q)] if single else [float(v) for v in q]
    if not 1 <= len(qs) <= L.FUSE_MAX_QUANTILES:
        raise ValueError(f"depth_quantile: 1 to {L.FUSE_MAX_QUANTILES} quantiles per call, got {len(qs)}")
    w, t = _f32c(weights, "weights"), _f32c(t_samples, "t_samples")
    if w.dim() != 2 or t.dim() != 2 or t.shape[0] != w.shape[0] or t.shape[1] != w.shape[1] + 1:
        raise ValueError(f"depth_quantile: expected weights [B, N] and t_samples [B, N + 1], got {tuple(w.shape)} and {tuple(t.shape)}")
    B, N = w.shape
    shape = (B,) if single else (B, len(qs))
    if out is None:
        out = torch.empty(shape, device=w.device, dtype=torch.float32)
    elif tuple(out.shape) != shape or out.dtype != torch.float32 or not out.is_contiguous() or out.device != w.device:
        raise ValueError(f"depth_quantile: bad preallocated output {tuple(out.shape)} (want {shape}, contiguous fp32 on {w.device})")
    with torch.cuda.device(w.device):
        L.fuse_check(L.fuse_lib().mipnerf_fuse_depth_quantile(B, N, _ptr(w), _ptr(t), len(qs), (C.c_float * len(qs))(*qs), _ptr(out), _stream()),
                     "depth_quantile")
    return out


def fuse_projection(cameras):
    """The frame records of `camera_record` rows (mipnerf_fuse_projection, rule P of include/mipnerf_fuse.h; host only): [F, 32] ->
    [F, 16] float32 on the CPU, each P[3][4] | W, H, near, far with (a, b, t) = P (p, 1), t the ray parameter of the world point p and
    (a / t, b / t) its continuous pixel coordinate.  Camera modes 0 and 1; a distorted camera (modes 2 and 3) is refused
    (NotImplementedError): fuse ideal pinhole frames of the capture's K instead, as `render_video.PathGen` builds them."""
    import numpy as np
    cams = np.ascontiguousarray(torch.as_tensor(cameras).detach().cpu().reshape(-1, 32).to(torch.float32).numpy())
    frames = np.zeros((cams.shape[0], L.FUSE_FRAME_FLOATS), np.float32)
    for f in range(cams.shape[0]):
        L.fuse_check(L.fuse_lib().mipnerf_fuse_projection(cams[f].ctypes.data, frames[f].ctypes.data), f"fuse_projection (camera {f})")
    return torch.from_numpy(frames)


class TSDF:
    """A truncated signed distance volume over the lattice dims = (nx, ny, nz) of the box lo .. hi (include/mipnerf_fuse.h, rules T and F):
    two fp32 planes `sum` and `count` [nz, ny, nx] on the device.  `integrate` adds depth frames, in order and without atomics, so the
    bytes do not depend on how the frames are split over calls; `lattice` is the volume whose zero level set `isosurface(v, 0.0, lo, hi)`
    cuts -- no density threshold.  `trunc`: the truncation distance in world units."""

    def __init__(self, dims, lo, hi, trunc, device="cuda"):
        self.dims, self.cdims, self.clo, self.chi = _lattice_args("TSDF", dims, lo, hi)
        self.lo, self.hi, self.trunc = tuple(self.clo), tuple(self.chi), float(trunc)
        if min(self.dims) < 2 or 7 * self.dims[0] * self.dims[1] * self.dims[2] >= 2 ** 31:
            raise ValueError(f"TSDF: a lattice needs 2 points per axis and 7 nx ny nz < 2^31, got {self.dims}")
        if not (self.trunc > 0.0 and self.trunc < float("inf")):
            raise ValueError(f"TSDF: trunc must be finite and > 0, got {trunc!r}")
        shape = (self.dims[2], self.dims[1], self.dims[0])
        self.sum = torch.zeros(shape, device=device, dtype=torch.float32)
        self.count = torch.zeros(shape, device=device, dtype=torch.float32)

    def integrate(self, frames, depth, offsets=None, carve=True):
        """frames [F, 16] (`fuse_projection`; CPU or device), depth: one fp32 device buffer that holds frame f's [H_f, W_f] image at
        offsets[f] (int64 [F]; None: the images lie one behind the other).  A pixel's depth is the ray parameter of its surface (what
        `depth_quantile` returns): +inf carves the ray free over [near, far] (carve=False: skipped), NaN / 0 / negative are skipped."""
        fr = torch.as_tensor(frames).detach().to(torch.float32).reshape(-1, L.FUSE_FRAME_FLOATS)
        host = fr.cpu()
        F = host.shape[0]
        depth = _f32c(depth, "depth").reshape(-1)
        pixels = (host[:, 12].double() * host[:, 13].double()).to(torch.int64)
        if offsets is None:
            off = torch.cumsum(pixels, 0) - pixels
        else:
            off = torch.as_tensor(offsets).detach().cpu().to(torch.int64).reshape(-1)
        if off.shape[0] != F:
            raise ValueError(f"TSDF.integrate: one offset per frame ({F}), got {off.shape[0]}")
        if F and (bool((off < 0).any()) or bool((off + pixels > depth.numel()).any()) or bool((pixels < 1).any())):
            raise ValueError(f"TSDF.integrate: a frame's image does not lie inside the depth buffer ({depth.numel()} floats)")
        dev = self.sum.device
        fr, off = fr.to(dev).contiguous(), off.to(dev).contiguous()
        with torch.cuda.device(dev):
            L.fuse_check(L.fuse_lib().mipnerf_fuse_integrate(self.cdims, self.clo, self.chi, self.trunc, int(bool(carve)), F, _ptr(fr), _ptr(off),
                                                             _ptr(depth), depth.numel(), _ptr(self.sum), _ptr(self.count), _stream()),
                         "TSDF.integrate")
        return self

    def lattice(self, unseen="inside"):
        """[nz, ny, nx] fp32: -(sum / count) where a frame updated the point, else +1 (unseen='inside', the default: space carving -- a
        point deeper than trunc behind every view's surface is never updated, and calling it outside wraps the object in a second, inner
        shell) or -1 ('outside').  Inside is > 0, the convention of `isosurface`."""
        if unseen not in ("inside", "outside"):
            raise ValueError(f"TSDF.lattice: unseen must be 'inside' or 'outside', got {unseen!r}")
        out = torch.empty_like(self.sum)
        with torch.cuda.device(out.device):
            L.fuse_check(L.fuse_lib().mipnerf_fuse_finalise(self.cdims, _ptr(self.sum), _ptr(self.count), 1.0 if unseen == "inside" else -1.0,
                                                            _ptr(out), _stream()), "TSDF.lattice")
        return out
