"""Tuning the CONTRACTED preview lattice (the unbounded-scene model's, `preview.bake_field(space='contracted')`) through its own march:
`python -m mipnerf_pl_amd.preview_tune360`.  The gradient of mipnerf_preview_360_march with respect to the rows is
libmipnerf_preview_tune_360.so's (include/mipnerf_preview_tune_360.h, rules C6 - C8); the Adam pass and the regulariser are the bounded
lattice's, `preview.tune_adam` and `preview.tune_regularise`, called unchanged: neither knows which space a lattice lives in.

`preview.march_grad`, `preview.TuneState`, `preview.tune_field` and `preview --tune` keep refusing a contracted lattice; this module
refuses a lattice in world coordinates.  The file the command writes is rendered by the unchanged `preview --space contracted --baked`."""
import argparse
import ctypes as C
import os
import time

import numpy as np
import torch

from . import _lib as L
from . import preview as pv
from .preview import (DEFAULT_MAX_STEPS, DEFAULT_STEP_SCALE, DEFAULT_T_MIN, DEFAULT_TUNE_BATCH, DEFAULT_TUNE_LR_COLOUR, DEFAULT_TUNE_LR_SIGMA,
                      DEFAULT_TUNE_TV_EPS, BakedField, BakedPyramid, SparseField)


def _require_contracted(baked, who):
    """A dense single lattice of the contracted space, or the exception that says where the other kinds go."""
    if isinstance(baked, SparseField):
        raise NotImplementedError(f"{who}: a SparseField is not a tuning target (the gradient is scattered into dense rows): tune the dense "
                                  "BakedField, then .to_sparse()")
    if isinstance(baked, BakedPyramid):
        raise NotImplementedError(f"{who}: a BakedPyramid is not a tuning target (a contracted pyramid is not implemented): tune a single "
                                  "BakedField")
    if not isinstance(baked, BakedField):
        raise TypeError(f"{who}: expected a BakedField, got {type(baked).__name__}")
    if baked.space != "contracted":
        raise ValueError(f"{who}: this lattice lies in world coordinates (a bounded scene); its gradient is preview.march_grad's and its "
                         "tuning preview.TuneState's / preview.tune_field's")


def march_grad(baked, origins, directions, near, far, background, grad_rgb=None, grad_acc=None, target=None, loss_scale=None, grad_rows=None,
               step_scale=DEFAULT_STEP_SCALE, t_min=DEFAULT_T_MIN, max_steps=DEFAULT_MAX_STEPS, use_occupancy=True, out=None, counters=None):
    """mipnerf_preview_tune_360_grad: the march `preview.march` gives a contracted lattice and its gradient with respect to the rows in one
    launch -> (grad_rows, rgb, acc).  Arguments as `preview.march_grad`: the loss side is `grad_rgb` [B, 3], or `target` [B, 3] with
    `loss_scale` (G = loss_scale * (rgb - target), rgb this launch's own); `grad_acc` [B] is optional.  `grad_rows` fp32 [nz, ny, nx, W] is
    ADDED INTO (None: a fresh zero tensor); rgb and acc are the bytes `preview.march` gives (`out`: the two, preallocated).  `counters`:
    an int64 [2] tensor that is added to (samples, flushes).  The sums over rays use float atomics: two runs may differ in the last bits
    of grad_rows."""
    _require_contracted(baked, "preview_tune360.march_grad")
    B, dev, _, (field,), params = pv._march_args("march_grad", [baked], dict(origins=origins, directions=directions, near=near, far=far),
                                                 background, step_scale, t_min, max_steps, (None, None, None), None, use_occupancy)
    if (grad_rgb is None) == (target is None):
        raise ValueError("march_grad: give exactly one of grad_rgb and target")
    if target is not None and loss_scale is None:
        raise ValueError("march_grad: target needs loss_scale")
    for name, t, shape in (("grad_rgb", grad_rgb, (B, 3)), ("target", target, (B, 3)), ("grad_acc", grad_acc, (B,))):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or t.device != dev or tuple(t.shape) != shape):
            raise ValueError(f"march_grad: {name} must be a contiguous fp32 tensor of {shape} on {dev}")
    if grad_rows is None:
        grad_rows = torch.zeros(baked.rows.shape, dtype=torch.float32, device=dev)
    elif grad_rows.dtype != torch.float32 or grad_rows.shape != baked.rows.shape or not grad_rows.is_contiguous() or grad_rows.device != dev:
        raise ValueError(f"march_grad: grad_rows must be a contiguous fp32 tensor of {tuple(baked.rows.shape)} on {dev}")
    if counters is not None and (counters.dtype != torch.int64 or counters.numel() != 2 or counters.device != dev):
        raise ValueError("march_grad: counters must be an int64 tensor of 2 entries")
    rgb, acc = (torch.empty(B, 3, device=dev), torch.empty(B, device=dev)) if out is None else out
    for name, t, shape in (("out[0] (rgb)", rgb, (B, 3)), ("out[1] (acc)", acc, (B,))):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.device != dev or tuple(t.shape) != shape:
            raise ValueError(f"march_grad: {name} must be a contiguous fp32 tensor of {shape} on {dev}")
    ptr = lambda t: None if t is None else t.data_ptr()
    with torch.cuda.device(dev):
        L.preview_tune_360_check(L.preview_tune_360_lib().mipnerf_preview_tune_360_grad(
            C.byref(field), baked.far_radius, C.byref(params), B, origins.data_ptr(), directions.data_ptr(), near.data_ptr(), far.data_ptr(),
            ptr(grad_rgb), ptr(target), 0.0 if loss_scale is None else float(loss_scale), ptr(grad_acc), rgb.data_ptr(), acc.data_ptr(),
            grad_rows.data_ptr(), ptr(counters), torch.cuda.current_stream().cuda_stream), "preview_tune_360_grad")
    return grad_rows, rgb, acc


class TuneState360(pv.TuneState):
    """`preview.TuneState` for a lattice of the contracted space: the same fields, `state_dict` / `load_state_dict`, mask (`baked_points` of
    the occupancy) and regulariser weights; `step` marches with `march_grad` of this module, then calls `preview.tune_regularise` and
    `preview.tune_adam` unchanged.  The mask of the points that can ever receive a gradient is fixed by the bake's occupancy: `reoccupy`
    runs after tuning, not during it."""

    def _refuse(self, baked):
        _require_contracted(baked, "TuneState360")

    def _march_grad(self, *args, **kwargs):
        return march_grad(*args, **kwargs)


def tune_field(baked, rays_and_targets, steps, white_bkgd=True, state=None, **kwargs):
    """`steps` steps of `TuneState360.step` on `baked`: `rays_and_targets(step)` -> (Rays, target [B, 3]).  Returns (state, losses), the
    losses a [steps] device tensor of each batch's mean squared error before its step.  `kwargs` go to `TuneState360`."""
    if steps < 1:
        raise ValueError("tune_field: at least one step")
    state = TuneState360(baked, **kwargs) if state is None else state
    losses = []
    for k in range(int(steps)):
        rays, target = rays_and_targets(k)
        losses.append(state.step(rays, target, white_bkgd))
    return state, torch.stack(losses)


def reoccupy(baked, threshold, dilate=1):
    """Rebuild `baked.occupancy` from the rows' own density: `ops.occupancy_grid` of the sigma entries as an fp32 lattice.  A lattice baked
    with a low threshold can be tuned where the bake's point density was too low and pruned afterwards with this.  Returns the new
    occupied share of the cells (a read-back)."""
    from . import ops
    _require_contracted(baked, "reoccupy")
    if not (threshold >= 0 and np.isfinite(threshold)) or int(dilate) < 0:
        raise ValueError("reoccupy: the threshold must be finite and >= 0, dilate >= 0")
    sigma = baked.rows[..., 0].float().contiguous()
    occ = ops.occupancy_grid(sigma, float(threshold), baked.lo, baked.hi, dilate=int(dilate))
    occ.space = baked.space
    baked.occupancy, baked.threshold = occ, float(threshold)
    return occ.occupied_fraction()


# ---- the command -----------------------------------------------------------------------------------------------------------------
BAKE_FLAGS = ("grid", "sh_degree", "bound", "threshold", "dilate", "far_radius", "precision")
BAKE_DEFAULTS = dict(grid=128, sh_degree=1, bound=2.0, threshold=0.01, dilate=1, far_radius=None, precision=None)


def build_parser():
    from .evaluate import DEFAULT_CHUNK
    p = argparse.ArgumentParser(prog="python -m mipnerf_pl_amd.preview_tune360",
                                description="Bake (or load) the contracted preview lattice of a llff / realdata360 checkpoint, tune its rows "
                                            "through its own march against the train split, and save it for `preview --space contracted "
                                            "--baked`.  The float-atomic gradient sums make two runs differ in the last bits.")
    p.add_argument("--ckpt", help="Path to ckpt.")
    p.add_argument("--data", help="path to the captured scene: its train split is tuned against, its test split compared on", default=None)
    p.add_argument("--out_dir", help="Output directory: the lattice goes to <out_dir>/preview_tune360/<exp_name>/baked.npz", type=str, required=True)
    p.add_argument("--steps", help="Adam steps", type=int, required=True, metavar="N")
    p.add_argument("--baked", help="tune a contracted dense lattice saved earlier instead of baking one", type=str, default=None, metavar="FILE")
    p.add_argument("--grid", help="bake: lattice points per axis (default 128)", type=int, default=None)
    p.add_argument("--sh_degree", help="bake: degree of the view-dependent colour (default 1)", type=int, default=None)
    p.add_argument("--bound", help="bake: half-width of the lattice in the contracted space (default 2, all of it)", type=float, default=None)
    p.add_argument("--threshold", help="bake: a cell is marched, and its corners tuned, when the density at one of them exceeds this (default "
                   "0.01); a low value leaves more points to the tuning, --reoccupy prunes afterwards", type=float, default=None, metavar="T")
    p.add_argument("--dilate", help="bake and --reoccupy: occupied cells grow by this many cells (default 1)", type=int, default=None)
    p.add_argument("--far_radius", help="bake: rays are cut beyond this distance from the centre (default: the largest distance any ray of "
                   "the test split reaches, plus one cell's allowance)", type=float, default=None, metavar="R")
    p.add_argument("--precision", help="bake: MLP precision (default: the checkpoint's)", choices=["fp32", "bf16"], default=None)
    p.add_argument("--batch", help=f"rays per step (default {DEFAULT_TUNE_BATCH})", type=int, default=DEFAULT_TUNE_BATCH)
    p.add_argument("--lr_sigma", help=f"Adam step of the density entries (a choice, not a measurement: default {DEFAULT_TUNE_LR_SIGMA})",
                   type=float, default=DEFAULT_TUNE_LR_SIGMA)
    p.add_argument("--lr_colour", help=f"Adam step of the colour coefficients (a choice, not a measurement: default {DEFAULT_TUNE_LR_COLOUR})",
                   type=float, default=DEFAULT_TUNE_LR_COLOUR)
    p.add_argument("--target", help="what the lattice is tuned against: the train split's photos, or the MLP's render of the same rays",
                   choices=["photos", "mlp"], default="photos")
    p.add_argument("--seed", help="seed of the batch draws", type=int, default=0)
    p.add_argument("--tv_sigma", help="weight of the total variation of the density, per tuned point (default 0: off)", type=float, default=0.0,
                   metavar="X")
    p.add_argument("--tv_colour", help="weight of the total variation of the colour coefficients, per tuned point (default 0: off)", type=float,
                   default=0.0, metavar="X")
    p.add_argument("--sh_decay", help="weight of 0.5 x the squared view-dependent coefficients, per tuned point (default 0: off)", type=float,
                   default=0.0, metavar="X")
    p.add_argument("--tv_eps", help=f"the eps under the total variation's root (default {DEFAULT_TUNE_TV_EPS})", type=float,
                   default=DEFAULT_TUNE_TV_EPS, metavar="X")
    p.add_argument("--reoccupy", help="after tuning, rebuild the occupancy from the tuned density with this threshold", type=float, default=None,
                   metavar="T")
    p.add_argument("--sparse", help="save the tuned lattice as sparse rows (render it with `preview --space contracted --sparse --baked`)",
                   action="store_true")
    p.add_argument("--factor", help="the data set's shrink factor (default: the checkpoint's)", type=int, default=None)
    p.add_argument("--compare", help="render the test split from the untuned and the tuned lattice and with the MLP: mean PSNR of each lattice "
                   "against the photos and against the MLP", action="store_true")
    p.add_argument("--step", help="march step in units of the smallest cell edge of the contracted lattice", type=float, default=DEFAULT_STEP_SCALE)
    p.add_argument("--t_min", help="stop a ray when its transmittance falls below this", type=float, default=DEFAULT_T_MIN)
    p.add_argument("--chunk_size", help="chunk size of the MLP renders (--target mlp, --compare)", type=int, default=DEFAULT_CHUNK)
    return p


def refuse_arguments(args):
    """Everything that can be refused from the command line alone, before any file is opened."""
    if args.steps < 1:
        raise SystemExit(f"--steps {args.steps}: at least one step")
    for f in ("lr_sigma", "lr_colour", "tv_sigma", "tv_colour", "sh_decay"):
        v = getattr(args, f)
        if not (v >= 0 and np.isfinite(v)):
            raise SystemExit(f"--{f} {v}: must be finite and >= 0")
    if not (args.tv_eps > 0 and np.isfinite(args.tv_eps)):
        raise SystemExit(f"--tv_eps {args.tv_eps}: must be finite and > 0")
    if args.batch < 1:
        raise SystemExit(f"--batch {args.batch}: at least one ray")
    if args.reoccupy is not None and not (args.reoccupy >= 0 and np.isfinite(args.reoccupy)):
        raise SystemExit(f"--reoccupy {args.reoccupy}: the threshold must be finite and >= 0")
    if args.baked is not None:
        given = [f for f in BAKE_FLAGS if getattr(args, f) is not None]
        if given:
            raise SystemExit(f"--baked tunes a lattice that exists already; --{given[0]} belongs to baking one: give one of them")
    else:
        if args.grid is not None and (args.grid < 2 or 7 * args.grid ** 3 >= 2 ** 31):
            raise SystemExit(f"--grid {args.grid}: the lattice needs at least 2 points per axis and 7 n^3 < 2^31")
        if args.sh_degree is not None and args.sh_degree not in (0, 1, 2):
            raise SystemExit(f"--sh_degree {args.sh_degree}: the degree must be 0, 1 or 2")
        if args.bound is not None and not 0 < args.bound <= 2:
            raise SystemExit(f"--bound {args.bound}: must be positive, and the contracted space ends at 2")
        if args.far_radius is not None and not (args.far_radius > 1 and np.isfinite(args.far_radius)):
            raise SystemExit(f"--far_radius {args.far_radius}: must be finite and > 1")
        if args.dilate is not None and args.dilate < 0:
            raise SystemExit(f"--dilate {args.dilate}: must not be negative")
    if not args.step > 0:
        raise SystemExit(f"--step {args.step}: the step must be positive")
    if not 0 <= args.t_min < 1:
        raise SystemExit(f"--t_min {args.t_min}: must lie in [0, 1)")
    if args.data is None:
        raise SystemExit("give --data: the lattice is tuned on pixels of its train split")
    if args.ckpt is None:
        raise SystemExit("give --ckpt: the checkpoint names the experiment, is what is baked, and is what --target mlp and --compare render")


def refuse_baked_file(args):
    """A --baked file that is not a contracted dense single lattice: refused after reading the file's keys alone."""
    if args.baked is None:
        return
    if BakedPyramid.stored_sparse(args.baked):
        raise SystemExit(f"--baked {args.baked} holds sparse rows: sparse rows are not a tuning target; tune the dense lattice and give --sparse")
    if BakedPyramid.stored_levels(args.baked) is not None:
        raise SystemExit(f"--baked {args.baked} holds a pyramid of lattices: a pyramid is not a tuning target")
    if BakedField.stored_space(args.baked) != "contracted":
        raise SystemExit(f"--baked {args.baked} holds a lattice of world coordinates (a bounded scene): tune it with `preview --tune`")


def refuse_checkpoint(system):
    """A bounded checkpoint: refused before anything is moved to the device."""
    from .render_video import is_scene360
    if not (is_scene360(system.hparams) and bool(getattr(system.mip_nerf, "unbounded", False))):
        raise SystemExit("preview_tune360: this command tunes the contracted lattice of a llff / realdata360 checkpoint of the unbounded-scene "
                         "model; this checkpoint ({}) holds a bounded model: tune its lattice with `preview --tune`".format(
                             system.hparams.get("dataset_name")))
    try:
        pv.refuse_model(system, "preview_tune360", "contracted")
    except NotImplementedError as e:
        raise SystemExit(str(e))


def _test_psnr(system, lattices, dataset, args, white, dev):
    """mean PSNR over the test split of every lattice of `lattices` against the photos and against the MLP's frame -> [(photos, mlp)]"""
    from .evaluate import FrameEvaluator
    frames, sums = {}, [[[], []] for _ in lattices]
    for idx in range(len(dataset)):
        rays, gt = dataset[idx]
        h, w = int(gt.shape[0]), int(gt.shape[1])
        if (h, w) not in frames:
            frames[(h, w)] = (FrameEvaluator(system.mip_nerf, h, w, args.chunk_size, white, dev),
                              [pv.PreviewFrame(b, h, w, white, args.step, args.t_min) for b in lattices])
        ev, previews = frames[(h, w)]
        want = ev.render(rays)[0]
        for k, fr in enumerate(previews):
            got = fr.render(rays)[0]
            sums[k][0].append(pv._psnr(got, gt[..., :3]))
            sums[k][1].append(pv._psnr(got, want))
    return [(float(np.mean(a)), float(np.mean(b))) for a, b in sums]


def main(argv=None):
    from .datasets import RealData360
    from .evaluate import cull_far_radius
    from .render_video import load_system
    args = build_parser().parse_args(argv)
    refuse_arguments(args)
    refuse_baked_file(args)
    system = load_system(args)
    refuse_checkpoint(system)
    dev = torch.device("cuda", torch.cuda.current_device())
    system = system.to(dev).eval()
    hp = system.hparams
    factor = args.factor if args.factor is not None else int(hp.get("factor", 4))
    white = bool(hp["val.white_bkgd"])

    def split(name):
        return RealData360(args.data, split=name, white_bkgd=white, batch_type="all_images" if name == "train" else "single_image", factor=factor,
                           device=dev)
    train = split("train")
    test = split("test") if (args.compare or (args.baked is None and args.far_radius is None)) else None
    folder = os.path.join(args.out_dir, "preview_tune360", hp["exp_name"])
    os.makedirs(folder, exist_ok=True)
    with torch.no_grad():
        if args.baked is not None:
            baked = BakedField.load(args.baked, dev)
        else:
            how = {k: (BAKE_DEFAULTS[k] if getattr(args, k) is None else getattr(args, k)) for k in BAKE_FLAGS}
            radius = how["far_radius"]
            if radius is None:
                if how["grid"] < 4:
                    raise SystemExit("--grid: the default far radius needs at least 4 points per axis; give --far_radius")
                radius = cull_far_radius([test[i][0] for i in range(len(test))], how["grid"])
            baked = pv.bake_field(system, grid=how["grid"], degree=how["sh_degree"], lo=-float(how["bound"]), hi=float(how["bound"]),
                                  threshold=how["threshold"], dilate=how["dilate"], precision=how["precision"], space="contracted",
                                  far_radius=radius)
        untuned = BakedField(baked.rows.clone(), baked.dims, baked.lo, baked.hi, baked.degree, baked.occupancy, baked.threshold, baked.space,
                             baked.far_radius) if args.compare else None
        batches = pv.photo_batches(train, args.batch, args.seed) if args.target == "photos" else \
            pv.mlp_batches(system.mip_nerf, train, args.batch, args.seed, white, args.chunk_size)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        state, losses = tune_field(baked, batches, args.steps, white, lr_sigma=args.lr_sigma, lr_colour=args.lr_colour, step_scale=args.step,
                                   t_min=args.t_min, tv_sigma=args.tv_sigma, tv_colour=args.tv_colour, sh_decay=args.sh_decay, tv_eps=args.tv_eps)
        torch.cuda.synchronize()
        secs = time.perf_counter() - t0
        print("preview_tune360: tuned {0} steps of {1} rays against the {2} in {3:.2f} s ({4:.2f} ms per step), batch loss {5:.3e} -> {6:.3e}".format(
            args.steps, args.batch, "photos" if args.target == "photos" else "MLP", secs, 1e3 * secs / args.steps, float(losses[0]),
            float(losses[-1])))
        if state.regularised:
            print("preview_tune360: regularised with tv_sigma {0:g}, tv_colour {1:g}, sh_decay {2:g} (tv_eps {3:g}), each divided by the {4} "
                  "tuned points".format(state.tv_sigma, state.tv_colour, state.sh_decay, state.tv_eps, state.n_points))
        if args.reoccupy is not None:
            before = baked.occupancy.occupied_fraction() if baked.occupancy is not None else 1.0
            after = reoccupy(baked, args.reoccupy, BAKE_DEFAULTS["dilate"] if args.dilate is None else args.dilate)
            print("preview_tune360: occupancy rebuilt from the tuned density at threshold {0:g}: occupied share {1:.4f} -> {2:.4f}".format(
                args.reoccupy, before, after))
        if args.compare:
            (p0, m0), (p1, m1) = _test_psnr(system, [untuned, baked], test, args, white, dev)
            print("preview_tune360: tuning moved the mean PSNR over {0} test images: vs photos {1:.3f} -> {2:.3f}, vs MLP {3:.3f} -> {4:.3f}".format(
                len(test), p0, p1, m0, m1))
        out = baked.to_sparse() if args.sparse else baked
        print("preview_tune360: lattice saved to {}".format(out.save(os.path.join(folder, "baked.npz"))))
    return folder


if __name__ == "__main__":
    main()
