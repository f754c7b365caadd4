"""The reference's eval.py loop on the device: test-set PSNR / SSIM and the rgb / distance / acc images of every test view.

Per test image (eval.py:49-79): the fine level of the whole frame from one captured hipGraph (`model.GraphedFrame`, one per image size,
so a multi-scale test set captures four), PSNR and SSIM in one kernel (`ops.eval_errors`), and -- with `save_image` -- the three PNGs
of utils/vis.py:save_images made on the device (`ops.image_to_u8`, `ops.visualize_map`): only their bytes cross to the host.
Same directory layout, file names and metric files as the reference:

    <out_dir>/test/<exp_name>/<base_w / W>/{n:05d}_rgb.png, _dist.png, _acc.png     n advances every `scale` images
    <out_dir>/test/<exp_name>/psnrs.txt, ssims.txt                                   one space-separated line each

`summarize_results` is utils/metrics.py:128-152 and `generate_video` render_video.py:156-180 (imageio when importable, otherwise an
animated PNG written by PIL).  The command line is `python -m mipnerf_pl_amd.eval`.
"""
from __future__ import annotations

import glob
import os

import numpy as np
import torch

from . import ops
from .rays import Rays

DEFAULT_CHUNK = 12288        # eval.py / render_video.py --chunk_size


class FrameEvaluator:
    """Everything one image size needs: the frame's `GraphedFrame` (or its eager form) and the device buffers of the image bytes."""

    def __init__(self, model, height, width, chunk_size, white_bkgd, device, use_graph=True, occupancy=None, tighten=False, span_samples=None,
                 adaptive=False, ladder=None, proposal=None):
        from .model import CulledFrame, GraphedFrame
        self.h, self.w = int(height), int(width)
        n = self.h * self.w
        if occupancy is None:
            if tighten or adaptive:
                raise ValueError("FrameEvaluator: tighten=True / adaptive=True need an occupancy grid")
            self.frame = GraphedFrame(model, n, chunk_size, white_bkgd, device, capture=use_graph, proposal=proposal)
        else:       # rays that touch no occupied cell are skipped; the live count varies per frame, so the chunks run eagerly
            self.frame = CulledFrame(model, n, chunk_size, white_bkgd, device, occupancy, tighten=tighten, span_samples=span_samples,
                                     proposal=proposal, adaptive=adaptive, ladder=ladder)
        self.vis_ws = torch.empty(ops.visualize_workspace_floats(n), dtype=torch.float32, device=device)
        self.rgb_u8 = torch.empty(self.h, self.w, 3, dtype=torch.uint8, device=device)
        self.dist_u8 = torch.empty(self.h, self.w, 3, dtype=torch.uint8, device=device)
        self.acc_u8 = torch.empty(self.h, self.w, 3, dtype=torch.uint8, device=device)

    def render(self, rays):
        """Rays [H, W, k] -> fine (rgb [H, W, 3], distance [H, W], acc [H, W]): views of the frame's static outputs."""
        flat = Rays(*[t.reshape(self.h * self.w, -1) for t in rays])
        _, rgb, dist = self.frame(flat)
        return rgb.view(self.h, self.w, 3), dist.view(self.h, self.w), self.frame.acc[-1].view(self.h, self.w)

    def images(self, rgb, dist, acc):
        """The bytes of the three PNGs of vis.py:save_images, on the device: (rgb, dist, acc) uint8 [H, W, 3]."""
        ops.image_to_u8(rgb, out=self.rgb_u8)
        ops.visualize_map(dist, out=self.dist_u8, workspace=self.vis_ws)
        ops.visualize_map(acc, out=self.acc_u8, workspace=self.vis_ws)
        return self.rgb_u8, self.dist_u8, self.acc_u8


def _frame_flags(distorted):
    """`distorted` of the cull defaults as one flag per frame: None / a bool for all frames, or a sequence with one entry per frame."""
    if distorted is None or isinstance(distorted, (bool, np.bool_)):
        return None if not distorted else True
    flags = [bool(v) for v in distorted]
    return flags if any(flags) else None


def _end_points(rays):
    """o + near d and o + far d of every pixel of a frame, on the frame's device: two [H, W, 3] tensors."""
    return rays.origins + rays.near * rays.directions, rays.origins + rays.far * rays.directions


def corner_ray_bound(frames, distorted=None):
    """The largest absolute coordinate of the segment end points o + near d and o + far d over the four corner rays of every frame of
    `frames` (Rays of [H, W, k] tensors).  The end points are affine in the pixel position, so the corners bound every pixel's.
    That argument fails for a frame of a distorted camera (camera record mode 2 or 3): for the frames `distorted` flags (True: all; a
    sequence: one flag per frame) the maximum is taken over EVERY pixel, a reduction on the device where the rays already are."""
    flags = _frame_flags(distorted)
    bound = 0.0
    for i, rays in enumerate(frames):
        if flags is True or (flags is not None and flags[i]):
            bound = max([bound] + [float(p.abs().max()) for p in _end_points(rays)])
            continue
        for y in (0, -1):
            for x in (0, -1):
                o, d = rays.origins[y, x], rays.directions[y, x]
                for t in (rays.near[y, x], rays.far[y, x]):
                    bound = max(bound, float((o + t * d).abs().max()))
    return bound


def cull_box(frames, grid, distorted=None):
    """The half-width B of the occupancy box [-B, B]^3 of `grid` points per axis that holds every ray segment of `frames` plus one cell:
    B = B0 + h with h = 2 B / (grid - 1) the box's own cell, i.e. B = B0 (grid - 1) / (grid - 3).  `distorted`: see `corner_ray_bound`."""
    if grid < 4:
        raise ValueError("the occupancy grid needs at least 4 points per axis")
    return corner_ray_bound(frames, distorted) * (grid - 1) / (grid - 3)


def corner_ray_radius(frames, distorted=None):
    """The largest distance from the centre of the segment end points o + near d and o + far d over the four corner rays of every frame of
    `frames` (Rays of [H, W, k] tensors).  The norm of an end point is convex in the pixel position, so the corners bound every pixel's, and
    convex in t, so the two ends bound the whole segment.  Convexity in the pixel position fails under lens distortion: for the frames
    `distorted` flags (as in `corner_ray_bound`) the maximum is taken over every pixel, on the device."""
    flags = _frame_flags(distorted)
    radius = 0.0
    for i, rays in enumerate(frames):
        if flags is True or (flags is not None and flags[i]):
            radius = max([radius] + [float(p.double().norm(dim=-1).max()) for p in _end_points(rays)])
            continue
        for y in (0, -1):
            for x in (0, -1):
                o, d = rays.origins[y, x], rays.directions[y, x]
                for t in (rays.near[y, x], rays.far[y, x]):
                    radius = max(radius, float((o + t * d).double().norm()))
    return radius


def cull_far_radius(frames, grid, distorted=None):
    """The far radius R of a contracted-space occupancy grid of `grid` points per axis for `frames`: `corner_ray_radius` times
    (grid - 1) / (grid - 3), the allowance `cull_box` makes.  The lattice's density is 0 beyond |z| = 2 - 1 / R, so nothing a ray reaches
    may lie beyond it.  `distorted`: see `corner_ray_radius`."""
    if grid < 4:
        raise ValueError("the occupancy grid needs at least 4 points per axis")
    return max(corner_ray_radius(frames, distorted) * (grid - 1) / (grid - 3), 1.0 + 1e-3)


def distorted_frames(dataset):
    """One flag per image of `dataset`: whether its camera record is a distorted one (mode 2 or 3), for the `distorted` argument of the
    cull defaults.  None for a data set without a camera table."""
    cams = getattr(dataset, "cameras", None)
    return None if cams is None else [bool(v) for v in (cams[:, 26] >= 2).tolist()]


def scene_occupancy(system, frames=None, grid=128, threshold=0.01, dilate=1, bound=None, verbose=True, space=None, far_radius=None,
                    distorted=None):
    """`ops.field_occupancy` of the system's field on grid^3 points over [-bound, bound]^3 (default: `cull_box` of `frames`), printing the
    occupied share of the grid once.  The unbounded-scene model is refused unless `space='contracted'`: the grid then spans
    [-bound, bound]^3 of the contracted space (default 2, all of it) with the density 0 beyond |z| = 2 - 1 / far_radius (default:
    `cull_far_radius` of `frames`), and a bounded model is refused.  `distorted` flags the frames of distorted cameras, whose default
    bound / far radius is taken over every pixel (`corner_ray_bound`)."""
    unbounded = bool(getattr(system.mip_nerf, "unbounded", False))
    if space is None:
        if unbounded:
            raise NotImplementedError("empty-space culling: unbounded=True models are not supported (their field lives in a contracted space) "
                                      "unless the grid lies there too: space='contracted'")
        if bound is None:
            if frames is None:
                raise ValueError("scene_occupancy: give the frames to be rendered or a bound")
            bound = cull_box(frames, grid, distorted)
        occ = ops.field_occupancy(system, grid=grid, lo=-float(bound), hi=float(bound), threshold=threshold, dilate=dilate)
        if verbose:
            print("cull: occupied share of the {0}^3 grid over +-{1:.4f} (threshold {2:g}, dilate {3}): {4:.4f}".format(
                grid, float(bound), threshold, dilate, occ.occupied_fraction()))
        return occ
    if space != "contracted":
        raise ValueError(f"scene_occupancy: space must be None or 'contracted' (a world box cannot hold an unbounded ray), got {space!r}")
    if not unbounded:
        raise ValueError("scene_occupancy: space='contracted' belongs to unbounded=True models; a bounded model's grid lies in world space")
    if far_radius is None:
        if frames is None:
            raise ValueError("scene_occupancy: give the frames to be rendered or a far_radius")
        far_radius = cull_far_radius(frames, grid, distorted)
    bound = 2.0 if bound is None else float(bound)
    occ = ops.field_occupancy(system, grid=grid, lo=-bound, hi=bound, threshold=threshold, dilate=dilate, space=space, far_radius=float(far_radius))
    if verbose:
        print("cull: occupied share of the {0}^3 grid over +-{1:.4f} of the contracted space, far radius {2:.4f} (threshold {3:g}, dilate {4}): "
              "{5:.4f}".format(grid, bound, float(far_radius), threshold, dilate, occ.occupied_fraction()))
    return occ


def scene_proposal(system, frames=None, grid=256, bound=None, verbose=True, distorted=None, space=None, far_radius=None, levels=1,
                   footprint=1.0):
    """`ops.field_proposal` of the system's field on grid^3 points over [-bound, bound]^3 (default: `cull_box` of `frames`, the box that
    holds every ray segment plus one cell), printing the lattice size and its build time once.  The unbounded-scene model is refused
    unless `space='contracted'`: the result is then `ops.field_proposal_360` -- a pyramid of `levels` contracted lattices, the finest with
    grid^3 points, over [-bound, bound]^3 of the contracted space (default 2, all of it), with the density 0 beyond |z| = 2 - 1 / far_radius
    (default: `cull_far_radius` of `frames`) and the level picked with `footprint` -- and a bounded model is refused.  `levels` = 1 and
    `footprint` = 1 are choices, not measurements."""
    import time
    unbounded = bool(getattr(system.mip_nerf, "unbounded", False))
    if space is None:
        if unbounded:
            raise NotImplementedError("lattice proposals: unbounded=True models are not supported (their field lives in a contracted space) "
                                      "unless the lattice lies there too: space='contracted'")
        if bound is None:
            if frames is None:
                raise ValueError("scene_proposal: give the frames to be rendered or a bound")
            bound = cull_box(frames, grid, distorted)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        prop = ops.field_proposal(system, grid=grid, lo=-float(bound), hi=float(bound))
        torch.cuda.synchronize()
        if verbose:
            print("proposal: {0}^3 density lattice over +-{1:.4f} built in {2:.1f} ms".format(grid, float(bound), 1e3 * (time.perf_counter() - t0)))
        return prop
    if space != "contracted":
        raise ValueError(f"scene_proposal: space must be None or 'contracted' (a world box cannot hold an unbounded ray), got {space!r}")
    if not unbounded:
        raise ValueError("scene_proposal: space='contracted' belongs to unbounded=True models; a bounded model's lattice lies in world space")
    ops.proposal_ladder_360(grid, levels)            # a bad ladder is refused before the frames are walked
    if far_radius is None:
        if frames is None:
            raise ValueError("scene_proposal: give the frames to be rendered or a far_radius")
        far_radius = cull_far_radius(frames, grid, distorted)
    bound = 2.0 if bound is None else float(bound)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    prop = ops.field_proposal_360(system, grid=grid, levels=levels, far_radius=float(far_radius), bound=bound, footprint=footprint)
    torch.cuda.synchronize()
    if verbose:
        print("proposal: {0}^3 x {1} levels contracted density lattice over +-{2:.4f}, far radius {3:.4f}, built in {4:.1f} ms".format(
            grid, int(levels), bound, float(far_radius), 1e3 * (time.perf_counter() - t0)))
    return prop


def report_live_share(shares, spans=None, samples=None):
    """The closing line of a culled run: the mean share of rays rendered per frame and, for a tightened run (`spans`), the mean share
    of [near, far] between the live rays' first and last occupied coarse frustum (`CulledFrame.span_share`; frames without a live ray do
    not count); for an adaptive run (`samples`) also the mean share of the model's sample count the live rays were rendered with
    (`CulledFrame.sample_share`)."""
    if shares:
        line = "cull: mean live share per frame: {:.4f} ({} frames)".format(float(np.mean(shares)), len(shares))
        spans = [v for v in (spans or []) if v == v]
        if spans:
            line += "; mean span share of the live rays: {:.4f}".format(float(np.mean(spans)))
        samples = [v for v in (samples or []) if v == v]
        if samples:
            line += "; mean sample share of the live rays: {:.4f}".format(float(np.mean(samples)))
        print(line)


def save_images(rgb_u8, dist_u8, acc_u8, path, idx):
    """vis.py:save_images with the bytes already made: {idx:05d}_rgb.png, _dist.png, _acc.png under `path`."""
    from PIL import Image
    names = []
    for tag, img in (("rgb", rgb_u8), ("dist", dist_u8), ("acc", acc_u8)):
        arr = img.cpu().numpy() if torch.is_tensor(img) else np.asarray(img)
        name = os.path.join(path, "{:05d}_{}.png".format(idx, tag))
        Image.fromarray(arr).save(name)
        names.append(name)
    return names


def image_slots(sizes, scale, base_width):
    """(n, sub-directory) of each image of a test set with image sizes `sizes` [(H, W)]: n advances every `scale` images
    (eval.py:54-56), the sub-directory is str(int(base_width / W)) (eval.py:76)."""
    n, out = -1, []
    for idx, (_, w) in enumerate(sizes):
        if idx % scale == 0:
            n += 1
        out.append((n, str(int(base_width / w))))
    return out


def write_metrics(folder, psnrs, ssims):
    """psnrs.txt / ssims.txt of eval.py:80-83: the values of one scene as one space-separated line."""
    os.makedirs(folder, exist_ok=True)
    for name, values in (("psnrs.txt", psnrs), ("ssims.txt", ssims)):
        with open(os.path.join(folder, name), "w") as f:
            f.write(" ".join(str(float(v)) for v in values))


def evaluate(system, dataset, out_dir, exp_name, scale=1, save_image=False, chunk_size=DEFAULT_CHUNK, white_bkgd=True, use_graph=True,
             base_size=(800, 800), occupancy=None, tighten=False, span_samples=None, adaptive=False, ladder=None, proposal=None):
    """eval.py:main after the checkpoint is loaded: every image of `dataset` (a test split of `datasets.dataset_dict`) rendered by
    `system.mip_nerf`, PSNR / SSIM recorded, the images written when `save_image`.  Returns (psnrs, ssims) as lists of floats.
    `occupancy` (an `ops.Occupancy`, e.g. `scene_occupancy`; for the unbounded-scene model one with `space='contracted'`): rays that touch
    no occupied cell are not rendered (`model.CulledFrame`); None is the full path.  `tighten` / `span_samples` are `CulledFrame`'s (live rays rendered on their occupied span -- not the untightened
    frame --; the frusta count of the classification), and so are `adaptive` / `ladder` (every live ray rendered with a sample count that
    follows its occupied span; implies `tighten`).  `proposal` (an `ops.ProposalGrid`, e.g. `scene_proposal`; bounded models): the coarse
    level's density comes from that lattice instead of an MLP pass -- not the two-level frame; works with and without `occupancy`."""
    if scale not in (1, 4):
        raise ValueError("scale must be 1 or 4 (eval.py --scale)")
    model = system.mip_nerf
    device = next(model.parameters()).device
    folder = os.path.join(out_dir, "test", exp_name)
    for i in range(scale):
        os.makedirs(os.path.join(folder, str(2 ** i)), exist_ok=True)
    slots = image_slots(dataset.sizes, scale, base_size[0])
    evaluators, psnrs, ssims, shares, spans, samples = {}, [], [], [], [], []
    with torch.no_grad():
        for idx in range(len(dataset)):
            rays, gt = dataset[idx]
            h, w = int(gt.shape[0]), int(gt.shape[1])
            ev = evaluators.get((h, w))
            if ev is None:
                ev = evaluators[(h, w)] = FrameEvaluator(model, h, w, chunk_size, white_bkgd, device, use_graph, occupancy, tighten=tighten,
                                                         span_samples=span_samples, adaptive=adaptive, ladder=ladder, proposal=proposal)
            rgb, dist, acc = ev.render(rays)
            if occupancy is not None:
                shares.append(ev.frame.live_count / float(h * w))
                if tighten or adaptive:         # the spans are there already; an untightened run launches and reads back nothing more
                    spans.append(ev.frame.span_share)
                if adaptive:
                    samples.append(ev.frame.sample_share)
            psnr, ssim = ops.eval_errors(rgb, gt[..., :3])
            psnrs.append(psnr.item())
            ssims.append(ssim.item())
            if save_image:
                n, sub = slots[idx]
                save_images(*ev.images(rgb, dist, acc), os.path.join(folder, sub), n)
    write_metrics(folder, psnrs, ssims)
    generate_video(folder)
    report_live_share(shares, spans, samples)
    return psnrs, ssims


def summarize_results(folder, scene_names, num_buckets):
    """utils/metrics.py:128-152: 'psnr per bucket | ssim per bucket | average' over the scenes' psnrs.txt / ssims.txt."""
    results = []
    for scene in scene_names:
        values = []
        for metric in ("psnrs", "ssims"):
            with open(os.path.join(folder, "test", scene, f"{metric}.txt")) as f:
                v = np.array([float(s) for s in f.readline().split(" ")])
            values.append(np.mean(np.reshape(v, [-1, num_buckets]), 0))
        results.append(np.concatenate(values))
    avg = np.mean(np.array(results), 0)
    psnr, ssim = np.mean(np.reshape(avg, [-1, num_buckets]), 1)
    mse = np.exp(-0.1 * np.log(10.) * psnr)
    dssim = np.sqrt(1 - ssim)
    avg_avg = np.exp(np.mean(np.log(np.array([mse, dssim]))))
    s = [" ".join(f"{x:0.4f}" for x in row) for row in np.reshape(avg, [-1, num_buckets])]
    s.append(f"{avg_avg:0.4f}")
    return " | ".join(s)


def generate_video(image_path):
    """render_video.py:156-180: per scale directory 1, 2, 4, ... the *_rgb.png frames in name order, then the same frames reversed,
    at 40 fps.  With imageio: video_<s>.mov (as the reference); without it: an animated PNG video_<s>.png written by PIL.
    Returns the written paths."""
    try:
        import imageio
    except ImportError:
        imageio = None
    from PIL import Image
    n_dirs = sum(os.path.isdir(os.path.join(image_path, d)) for d in os.listdir(image_path))
    written = []
    for i in range(n_dirs):
        d = os.path.join(image_path, str(2 ** i))
        files = sorted(glob.glob(os.path.join(d, "*_rgb.png")))
        if not files:
            continue
        frames = [np.array(Image.open(f)).astype(np.uint8) for f in files]
        frames += frames[::-1]
        if imageio is not None:
            name = os.path.join(d, "video_{}.mov".format(2 ** i))
            imageio.mimwrite(name, frames, fps=40, quality=10)
            print("generate video in {}".format(name))
        else:
            name = os.path.join(d, "video_{}.png".format(2 ** i))
            ims = [Image.fromarray(f) for f in frames]
            ims[0].save(name, save_all=True, append_images=ims[1:], duration=25, loop=0)
            print("imageio is not installed: generate animated PNG in {}".format(name))
        written.append(name)
    return written
