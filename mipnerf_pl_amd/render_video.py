"""The reference's render_video.py on the device: the spherical camera path rendered at `scale` pyramid levels.

`render_video(system, out_dir, exp_name, scale, ...)` restates render_video.py:run_render: rays of `datasets.RenderGen` (generated on the
device), each frame from one captured hipGraph per image size (`evaluate.FrameEvaluator`), its rgb / distance / acc PNGs made on the
device and written to <out_dir>/render_spheric/<exp_name>/<base_w / W>/{i % n_poses:05d}_{rgb,dist,acc}.png, then `generate_video`.
`n_poses` (not in the reference) shortens the path; the default 120 is the reference's.

    python -m mipnerf_pl_amd.render_video --ckpt CKPT --out_dir OUT --scale 4 [--gen_video_only --render_images_dir DIR]

A checkpoint of a captured scene (`dataset_name` llff / realdata360) has no spherical path to fly: `--path interp` (its default) renders
`datasets.gen_render_path` -- the reference's utils/vis.py path, `--n_views // 3` poses between consecutive poses of the `--split` of
`--data` and back to the first -- at the data set's own size to <out_dir>/render_path/<exp_name>/1/{i:05d}_{rgb,dist,acc}.png:

    python -m mipnerf_pl_amd.render_video --ckpt CKPT --data DATA_DIR --out_dir OUT --scale 1 [--split test] [--n_views 30]
"""
from __future__ import annotations

import argparse
import os

import numpy as np
import torch

from .evaluate import DEFAULT_CHUNK, FrameEvaluator, generate_video, report_live_share, save_images, scene_occupancy, scene_proposal

CAMERA_ANGLE_X = 0.6911112070083618       # render_video.py --camera_angle_x default (Blender's lego)


def render_video(system, out_dir, exp_name, scale, base_size=(800, 800), camera_angle_x=CAMERA_ANGLE_X, chunk_size=DEFAULT_CHUNK,
                 white_bkgd=True, n_poses=120, use_graph=True, occupancy=None, tighten=False, span_samples=None, adaptive=False,
                 ladder=None, proposal=None):
    """render_video.py:run_render after the checkpoint is loaded.  Returns the output folder.  `occupancy` (an `ops.Occupancy`): rays
    that touch no occupied cell are not rendered (`model.CulledFrame`); None is the full path.  `tighten` / `span_samples` are
    `CulledFrame`'s (live rays rendered on their occupied span; the frusta count of the classification) and need an `occupancy`; so do
    `adaptive` / `ladder` (every live ray rendered with a sample count that follows its occupied span; implies `tighten`).  `proposal`
    (an `ops.ProposalGrid`): the coarse level's density comes from that lattice instead of an MLP pass (not the two-level frame)."""
    from .datasets import RenderGen
    model = system.mip_nerf
    device = next(model.parameters()).device
    folder = os.path.join(out_dir, "render_spheric", exp_name)
    for i in range(scale):
        os.makedirs(os.path.join(folder, str(2 ** i)), exist_ok=True)
    focal = .5 * base_size[0] / np.tan(.5 * camera_angle_x)
    dataset = RenderGen(focal, base_size, scale, device=device, n_poses=n_poses)
    nums = len(dataset) // scale
    evaluators, shares, spans, samples = {}, [], [], []
    with torch.no_grad():
        for idx in range(len(dataset)):
            rays = dataset[idx]
            h, w = dataset.sizes[idx]
            ev = evaluators.get((h, w))
            if ev is None:
                ev = evaluators[(h, w)] = FrameEvaluator(model, h, w, chunk_size, white_bkgd, device, use_graph, occupancy, tighten=tighten,
                                                         span_samples=span_samples, adaptive=adaptive, ladder=ladder, proposal=proposal)
            images = ev.images(*ev.render(rays))
            if occupancy is not None:
                shares.append(ev.frame.live_count / float(h * w))
                if tighten or adaptive:
                    spans.append(ev.frame.span_share)
                if adaptive:
                    samples.append(ev.frame.sample_share)
            save_images(*images, os.path.join(folder, str(int(base_size[0] / w))), idx % nums)
    generate_video(folder)
    report_live_share(shares, spans, samples)
    return folder


def render_path(system, dataset, out_dir, exp_name, n_views=30, chunk_size=DEFAULT_CHUNK, white_bkgd=False, use_graph=True, occupancy=None,
                tighten=False, span_samples=None, adaptive=False, ladder=None, proposal=None):
    """The interpolated path through the poses of `dataset` (a `datasets.RealData360` split), every frame as in `render_video`.
    Returns the output folder."""
    from .datasets import PathGen
    model = system.mip_nerf
    device = next(model.parameters()).device
    folder = os.path.join(out_dir, "render_path", exp_name)
    os.makedirs(os.path.join(folder, "1"), exist_ok=True)
    path = PathGen(dataset, n_views, device=device)
    h, w = path.sizes[0]
    ev = FrameEvaluator(model, h, w, chunk_size, white_bkgd, device, use_graph, occupancy, tighten=tighten, span_samples=span_samples,
                        adaptive=adaptive, ladder=ladder, proposal=proposal)
    shares, spans, samples = [], [], []
    with torch.no_grad():
        for idx in range(len(path)):
            images = ev.images(*ev.render(path[idx]))
            if occupancy is not None:
                shares.append(ev.frame.live_count / float(h * w))
                if tighten or adaptive:
                    spans.append(ev.frame.span_share)
                if adaptive:
                    samples.append(ev.frame.sample_share)
            save_images(*images, os.path.join(folder, "1"), idx)
    generate_video(folder)
    report_live_share(shares, spans, samples)
    return folder


def is_scene360(hparams):
    from .config import SCENE360_DATASETS
    return hparams.get("dataset_name") in SCENE360_DATASETS


def flag_given(argv, flag):
    """Whether `flag` is on the command line `argv` (None: this process's): tells a default from a choice."""
    import sys
    return any(a == flag or a.startswith(flag + "=") for a in (sys.argv[1:] if argv is None else argv))


def _bool(s):
    if str(s).lower() in ("1", "true", "yes", "y"):
        return True
    if str(s).lower() in ("0", "false", "no", "n"):
        return False
    raise argparse.ArgumentTypeError(f"expected a boolean, got {s!r}")


def add_common_args(p):
    """Flags both command lines share with the reference, and the two of their own (--precision, --no-graph)."""
    p.add_argument("--ckpt", help="Path to ckpt.")
    p.add_argument("--out_dir", help="Output directory.", type=str, required=True)
    p.add_argument("--chunk_size", help="Chunk size for render.", type=int, default=DEFAULT_CHUNK)
    p.add_argument("--white_bkgd", help="Train set image background color.", type=_bool, default=True)
    p.add_argument("--base_size", help="source image size: W H", type=int, nargs=2, default=[800, 800])
    p.add_argument("--factor", help="llff / realdata360 checkpoints: the data set's shrink factor (default: the checkpoint's)", type=int, default=None)
    p.add_argument("--precision", help="MLP precision (default: the checkpoint's)", choices=["fp32", "bf16"], default=None)
    p.add_argument("--no-graph", dest="use_graph", help="render each frame eagerly instead of replaying a captured hipGraph",
                   action="store_false")
    p.add_argument("--cull", help="skip the rays that touch no occupied cell of the field's occupancy grid (a checkpoint of the unbounded-scene "
                   "model needs --cull_space contracted as well)", action="store_true")
    p.add_argument("--cull_space", help="--cull with a checkpoint of the unbounded-scene model: the space the occupancy grid is laid out in; "
                   "its box is then [-B, B]^3 of the contracted space with --cull_bound B (default 2: all of it)", choices=["contracted"], default=None)
    p.add_argument("--cull_far_radius", help="--cull_space contracted: the grid's density is 0 beyond this distance from the centre (default: the "
                   "largest distance any corner ray of the cameras to be rendered reaches between near and far, times (grid - 1) / (grid - 3))",
                   type=float, default=None)
    p.add_argument("--cull_grid", help="--cull: lattice points per axis of the occupancy grid", type=int, default=128)
    p.add_argument("--cull_threshold", help="--cull: a cell is occupied when the density at one of its corners exceeds this; scene dependent, like "
                   "the mesh threshold: a foggy field needs a higher one", type=float, default=0.01)
    p.add_argument("--cull_dilate", help="--cull: occupied cells grow by this many cells in every direction", type=int, default=1)
    p.add_argument("--cull_bound", help="--cull: the grid spans [-B, B]^3 (default: the largest coordinate any ray of the cameras to be rendered "
                   "reaches between near and far, plus one cell)", type=float, default=None)
    p.add_argument("--cull_tighten", help="--cull: render every live ray on [near', far'], the fence posts around the coarse frusta of it that "
                   "touch an occupied cell, instead of [near, far]: the same samples in a shorter interval.  Not the untightened frame: the "
                   "samples sit elsewhere; the dropped parts of a ray lie only in cells the grid proves empty", action="store_true")
    p.add_argument("--cull_span_samples", help="--cull: coarse frusta per ray the classification uses (default: the checkpoint's num_samples)",
                   type=int, default=None)
    p.add_argument("--cull_adaptive", help="--cull: render every live ray with a sample count that follows its occupied span (implies "
                   "--cull_tighten): a ray whose span covers a quarter of its coarse frusta gets a quarter of the samples, on [near', far'], "
                   "from the ladder of --cull_ladder.  Not the untightened frame.  Guaranteed: a ray's coarse sample spacing is never wider "
                   "than the untightened frame's, and the parts of a ray it no longer samples lie only in cells the grid proves empty",
                   action="store_true")
    p.add_argument("--cull_ladder", help="--cull_adaptive: the sample counts to choose from, 1 to 8 strictly increasing values that end at the "
                   "rendered count (default: the distinct values of ceil(N k / 4), k = 1..4: 32 64 96 128 for 128 samples)", type=int,
                   nargs="+", default=None, metavar="C")
    p.add_argument("--proposal_grid", help="take the coarse level's density from a lattice of the field's own density with this many points per "
                   "axis (bare: 256) instead of an MLP pass: one MLP launch per chunk instead of two.  Not the two-level frame: the fine "
                   "samples sit elsewhere.  Bounded checkpoints only; works with and without --cull", type=int, nargs="?", const=256, default=None,
                   metavar="N")
    p.add_argument("--proposal_bound", help="--proposal_grid: the lattice spans [-B, B]^3 (default: the largest coordinate any ray of the "
                   "cameras to be rendered reaches between near and far, plus one cell)", type=float, default=None)
    p.add_argument("--proposal_space", help="--proposal_grid on a checkpoint of the unbounded-scene model: 'contracted' lays the lattice out in "
                   "the contracted space (a pyramid of --proposal_levels lattices over [-2, 2]^3, or [-B, B]^3 with --proposal_bound), read at "
                   "every sample's own contracted Gaussian", choices=["contracted"], default=None)
    p.add_argument("--proposal_far_radius", help="--proposal_space contracted: the lattice's density is 0 beyond this world radius (default: "
                   "the farthest point any ray of the cameras to be rendered reaches, plus one cell)", type=float, default=None, metavar="R")
    p.add_argument("--proposal_levels", help="--proposal_space contracted: levels of the pyramid, 1 to 4, each with every other point of the one "
                   "below and baked at its own spacing; a sample reads the level(s) as wide as its own Gaussian (default 1: a choice, not a "
                   "measurement)", type=int, default=None, metavar="L")
    p.add_argument("--proposal_footprint", help="--proposal_space contracted: scales the width that picks the level; 0 always reads the finest "
                   "(default 1: a choice, not a measurement)", type=float, default=None, metavar="F")
    p.add_argument("--render_samples", help="samples per ray and level to render with (default: the checkpoint's num_samples; the parameters do "
                   "not depend on it); independent of --cull", type=int, default=None)
    return p


def refuse_tighten_without_cull(args):
    """--cull_tighten is a way of culling: without --cull it exits with a message before anything is loaded."""
    if getattr(args, "cull_tighten", False) and not args.cull:
        raise SystemExit("--cull_tighten tightens the rays that --cull keeps: give --cull as well")
    if (getattr(args, "cull_space", None) is not None or getattr(args, "cull_far_radius", None) is not None) and not args.cull:
        raise SystemExit("--cull_space / --cull_far_radius describe the grid of --cull: give --cull as well")
    if getattr(args, "cull_far_radius", None) is not None and getattr(args, "cull_space", None) is None:
        raise SystemExit("--cull_far_radius belongs to --cull_space contracted")


def refuse_adaptive_without_cull(args):
    """--cull_adaptive is a way of culling and --cull_ladder belongs to it: anything else exits with a message before anything is loaded,
    and so does a ladder that is not 1 to 8 strictly increasing counts from at least 1 (that it ends at the rendered count is checked by
    `cli_ladder`, which knows the count)."""
    from .ops import LADDER_RULE, MAX_BUCKETS
    if getattr(args, "cull_adaptive", False) and not args.cull:
        raise SystemExit("--cull_adaptive chooses the sample counts of the rays that --cull keeps: give --cull as well")
    ladder = getattr(args, "cull_ladder", None)
    if ladder is not None and not getattr(args, "cull_adaptive", False):
        raise SystemExit("--cull_ladder lists the sample counts of --cull_adaptive: give --cull_adaptive as well")
    if ladder is not None and not (1 <= len(ladder) <= MAX_BUCKETS and ladder[0] >= 1 and all(a < b for a, b in zip(ladder, ladder[1:]))):
        raise SystemExit(f"--cull_ladder {' '.join(str(c) for c in ladder)}: {LADDER_RULE}")


def cli_ladder(args, system):
    """The validated ladder of --cull_adaptive against the count the system renders with (None without the flag); a bad one exits with
    the rule in the message."""
    if not getattr(args, "cull_adaptive", False):
        return None
    from .ops import sample_ladder
    try:
        return sample_ladder(int(system.mip_nerf.num_samples), args.cull_ladder)
    except ValueError as e:
        raise SystemExit(f"--cull_ladder: {e}")


def cli_span_samples(args, system):
    """The frusta count of the classification: --cull_span_samples, else the CHECKPOINT's num_samples -- with --render_samples the
    renderer's count changes and the classification does not coarsen."""
    if args.cull_span_samples is not None:
        return int(args.cull_span_samples)
    return int(getattr(system, "checkpoint_num_samples", system.hparams["nerf.num_samples"]))


def refuse_unbounded_cull(args, system):
    """--cull and the checkpoint's model must agree on the space: the unbounded-scene model needs --cull_space contracted, a bounded one
    must not have it.  Exits before anything is rendered."""
    unbounded, space = bool(getattr(system.mip_nerf, "unbounded", False)), getattr(args, "cull_space", None)
    if args.cull and unbounded and space is None:
        raise SystemExit("--cull: this checkpoint holds the unbounded-scene model (unbounded=True); its field lives in a contracted space -- "
                         "give --cull_space contracted (and optionally --cull_far_radius R) for an occupancy grid laid out there, or render it "
                         "without --cull")
    if args.cull and space is not None and not unbounded:
        raise SystemExit(f"--cull_space {space}: this checkpoint holds a bounded model; its occupancy grid lies in world space -- drop --cull_space")


def refuse_proposal_without_grid(args):
    """--proposal_bound describes the lattice of --proposal_grid: without it the command exits before anything is loaded; so does a
    lattice too small to hold a box."""
    grid = getattr(args, "proposal_grid", None)
    if getattr(args, "proposal_bound", None) is not None and grid is None:
        raise SystemExit("--proposal_bound describes the lattice of --proposal_grid: give --proposal_grid as well")
    if grid is not None and grid < 4:
        raise SystemExit(f"--proposal_grid {grid}: the lattice needs at least 4 points per axis")
    if getattr(args, "proposal_bound", None) is not None and not args.proposal_bound > 0:
        raise SystemExit(f"--proposal_bound {args.proposal_bound}: the half-width of the box must be positive")
    space = getattr(args, "proposal_space", None)
    if space is not None and grid is None:
        raise SystemExit("--proposal_space describes the lattice of --proposal_grid: give --proposal_grid as well")
    for flag in ("proposal_far_radius", "proposal_levels", "proposal_footprint"):
        if getattr(args, flag, None) is not None and space != "contracted":
            raise SystemExit(f"--{flag} belongs to --proposal_space contracted")
    levels, footprint, far = (getattr(args, k, None) for k in ("proposal_levels", "proposal_footprint", "proposal_far_radius"))
    if levels is not None and not 1 <= levels <= 4:
        raise SystemExit(f"--proposal_levels {levels}: a pyramid has 1 to 4 levels")
    if footprint is not None and not (footprint >= 0 and footprint < float("inf")):
        raise SystemExit(f"--proposal_footprint {footprint}: must be finite and >= 0")
    if far is not None and not far > 1:
        raise SystemExit(f"--proposal_far_radius {far}: must exceed 1, the radius of the uncontracted ball")
    if space is not None:
        from .ops import proposal_ladder_360
        try:
            proposal_ladder_360(grid, 1 if levels is None else levels)
        except ValueError as e:
            raise SystemExit(f"--proposal_grid {grid} --proposal_levels {levels}: {e}")


def refuse_scene360_proposal(args, system):
    """--proposal_grid and the checkpoint's model must agree on the space: a llff / realdata360 checkpoint (and any unbounded-scene model)
    needs --proposal_space contracted, a bounded one must not have it.  Exits with a message before anything is rendered."""
    if getattr(args, "proposal_grid", None) is None:
        return
    unbounded, space = bool(getattr(system.mip_nerf, "unbounded", False)), getattr(args, "proposal_space", None)
    if space is None and (is_scene360(system.hparams) or unbounded):
        raise SystemExit("--proposal_grid: this checkpoint holds a captured scene ({}); its rays leave any box and the unbounded-scene model "
                         "lives in a contracted space -- give --proposal_space contracted (and optionally --proposal_levels L, "
                         "--proposal_far_radius R, --proposal_footprint F) for a lattice laid out there, or render it without "
                         "--proposal_grid".format(system.hparams.get("dataset_name")))
    if space is not None and not unbounded:
        raise SystemExit(f"--proposal_space {space}: this checkpoint holds a bounded model; its proposal lattice lies in world space -- drop "
                         "--proposal_space")


def cli_proposal(args, system, frames, distorted=None):
    """The proposal lattice the --proposal flags ask for (None without --proposal_grid); `frames` / `distorted` as in `cli_occupancy`."""
    if getattr(args, "proposal_grid", None) is None:
        return None
    if getattr(args, "proposal_space", None) is not None:
        levels, footprint = getattr(args, "proposal_levels", None), getattr(args, "proposal_footprint", None)
        return scene_proposal(system, frames if args.proposal_far_radius is None else None, grid=args.proposal_grid, bound=args.proposal_bound,
                              distorted=distorted, space=args.proposal_space, far_radius=args.proposal_far_radius,
                              levels=1 if levels is None else levels, footprint=1.0 if footprint is None else footprint)
    return scene_proposal(system, frames if args.proposal_bound is None else None, grid=args.proposal_grid, bound=args.proposal_bound,
                          distorted=distorted)


def cli_occupancy(args, system, frames, distorted=None):
    """The occupancy grid the --cull flags ask for (None without --cull); `frames`: an iterable of the Rays [H, W, k] to be rendered,
    `distorted`: which of them come from a distorted camera (`evaluate.distorted_frames`; a path of pinhole records has none)."""
    if not args.cull:
        return None
    space = getattr(args, "cull_space", None)
    if space is None:
        return scene_occupancy(system, frames if args.cull_bound is None else None, grid=args.cull_grid, threshold=args.cull_threshold,
                               dilate=args.cull_dilate, bound=args.cull_bound, distorted=distorted)
    return scene_occupancy(system, frames if args.cull_far_radius is None else None, grid=args.cull_grid, threshold=args.cull_threshold,
                           dilate=args.cull_dilate, bound=args.cull_bound, space=space, far_radius=args.cull_far_radius, distorted=distorted)


def build_parser():
    p = add_common_args(argparse.ArgumentParser(prog="python -m mipnerf_pl_amd.render_video"))
    p.add_argument("--render_images_dir", help="already render image directory.", type=str, default=None)
    p.add_argument("--scale", help="must specify nums of scale", type=int, required=True)
    p.add_argument("--camera_angle_x", help="camera_angle_x in source dataset", type=float, default=CAMERA_ANGLE_X)
    p.add_argument("--gen_video_only", help="only generate the video of images rendered before", action="store_true")
    p.add_argument("--n_poses", help="poses on the spherical path", type=int, default=120)
    p.add_argument("--path", help="camera path (default: spheric, or interp for a llff / realdata360 checkpoint)", choices=["spheric", "interp"],
                   default=None)
    p.add_argument("--data", help="interp: path to the data whose poses the path runs through.", default=None)
    p.add_argument("--split", help="interp: the split whose poses the path runs through", choices=["train", "test"], default="test")
    p.add_argument("--n_views", help="interp: three times the poses per pair of consecutive poses", type=int, default=30)
    return p


def load_system(args):
    """MipNeRFSystem.load_from_checkpoint(--ckpt), with --precision when given (on the host; the caller moves it)."""
    from .system import MipNeRFSystem
    kw = {"precision": args.precision} if args.precision else {}
    n = getattr(args, "render_samples", None)
    if n is None:
        system = MipNeRFSystem.load_from_checkpoint(args.ckpt, **kw)
        system.checkpoint_num_samples = int(system.hparams["nerf.num_samples"])
        return system
    # the parameters do not depend on num_samples: the checkpoint's own count is read from its hyper-parameters, then the system is built
    # with the other one (Lightning merges extra keywords into the stored hyper-parameters; the stand-in takes them as `hparams`)
    from . import system as system_module
    stored = torch.load(args.ckpt, map_location="cpu", weights_only=False).get("hyper_parameters", {})
    override = {"nerf.num_samples": int(n)}
    kw.update(override if system_module._HAVE_PL else {"hparams": override})
    system = MipNeRFSystem.load_from_checkpoint(args.ckpt, **kw)
    system.checkpoint_num_samples = int(stored.get("nerf.num_samples", n))
    return system


def main(argv=None):
    args = build_parser().parse_args(argv)
    refuse_tighten_without_cull(args)
    refuse_adaptive_without_cull(args)
    refuse_proposal_without_grid(args)
    if args.gen_video_only:
        if args.render_images_dir is None:
            raise SystemExit("only generate video, you must give the different scale image base dir (--render_images_dir)")
        return generate_video(args.render_images_dir)
    system = load_system(args)
    refuse_unbounded_cull(args, system)
    refuse_scene360_proposal(args, system)
    ladder = cli_ladder(args, system)
    system = system.to(torch.device("cuda")).eval()
    hp = system.hparams
    if (args.path or ("interp" if is_scene360(hp) else "spheric")) == "interp":
        from .datasets import RealData360
        if args.data is None:
            raise SystemExit("the interp path runs through the poses of a data set: give --data")
        dev = torch.device("cuda", torch.cuda.current_device())
        dataset = RealData360(args.data, split=args.split, white_bkgd=hp["val.white_bkgd"],
                              batch_type="all_images" if args.split == "train" else "single_image",
                              factor=args.factor if args.factor is not None else int(hp.get("factor", 4)), device=dev)
        occupancy = proposal = None
        if args.cull or args.proposal_grid is not None:
            from .datasets import PathGen
            path = PathGen(dataset, args.n_views, device=dev)
            occupancy = cli_occupancy(args, system, (path[i] for i in range(len(path))))
            proposal = cli_proposal(args, system, (path[i] for i in range(len(path))))
        return render_path(system, dataset, args.out_dir, hp["exp_name"], n_views=args.n_views, chunk_size=args.chunk_size,
                           white_bkgd=args.white_bkgd if flag_given(argv, "--white_bkgd") else bool(hp["val.white_bkgd"]),
                           use_graph=args.use_graph, occupancy=occupancy, tighten=args.cull_tighten,
                           span_samples=cli_span_samples(args, system) if args.cull else None, adaptive=args.cull_adaptive, ladder=ladder,
                           proposal=proposal)
    occupancy = proposal = None
    if args.cull or args.proposal_grid is not None:
        from .datasets import RenderGen
        focal = .5 * args.base_size[0] / np.tan(.5 * args.camera_angle_x)
        gen = RenderGen(focal, args.base_size, args.scale, device=next(system.parameters()).device, n_poses=args.n_poses)
        occupancy = cli_occupancy(args, system, (gen[i] for i in range(len(gen))))
        proposal = cli_proposal(args, system, (gen[i] for i in range(len(gen))))
    return render_video(system, args.out_dir, system.hparams["exp_name"], args.scale, base_size=args.base_size,
                        camera_angle_x=args.camera_angle_x, chunk_size=args.chunk_size, white_bkgd=args.white_bkgd,
                        n_poses=args.n_poses, use_graph=args.use_graph, occupancy=occupancy, tighten=args.cull_tighten,
                        span_samples=cli_span_samples(args, system) if args.cull else None, adaptive=args.cull_adaptive, ladder=ladder,
                        proposal=proposal)


if __name__ == "__main__":
    main()
