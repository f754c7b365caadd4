"""Command line of the depth-fusion mesh (no counterpart in the reference; flags shared with extract_mesh / eval where they apply):

    python -m mipnerf_pl_amd.fuse_mesh --ckpt CKPT --data DIR --out_dir OUT [--split train] [--every 1] [--scale 1]
                                       [--grid 256 | --grid NX NY NZ] [--bound 1.5 | --aabb x0 y0 z0 x1 y1 z1] [--trunc_cells 3]
                                       [--quantile 0.5] [--unseen inside|outside] [--no_carve] [--precision fp32|bf16] [--no_color]
                                       [--save_depth] [--save_tsdf]

Renders the median depth of every `--every`-th camera of the split, fuses the maps into a truncated signed distance volume and writes its
zero level set as OUT/mesh/<exp_name>/fused_<nx>x<ny>x<nz>.ply: a mesh that needs no density threshold (`fuse.fuse_mesh`).  For a llff /
realdata360 checkpoint the cameras are ideal pinholes of the capture's K at the split's poses (`datasets.PathGen(dataset, poses=...)`), so
distorted captures work.  --save_tsdf writes the lattice as tsdf_<nx>x<ny>x<nz>.npy, --save_depth the depth maps as
depth/<index>_depth.png (`ops.visualize_map`).  Prints views, vertices, faces, the unseen share of the lattice and the share of pixels
without a depth."""
from __future__ import annotations

import argparse
import os

import numpy as np
import torch

from .extract_mesh import lattice_of
from .fuse import DEFAULT_TRUNC_CELLS, check_fuse_arguments, fuse_volume, mesh_of_volume
from .mesh import write_ply
from .render_video import add_common_args, is_scene360, load_system


def build_parser():
    p = add_common_args(argparse.ArgumentParser(prog="python -m mipnerf_pl_amd.fuse_mesh"))
    p.add_argument("--data", help="Path to the data whose cameras are fused.")
    p.add_argument("--split", help="the split whose cameras are fused", choices=["train", "val", "test"], default="train")
    p.add_argument("--every", help="fuse every n-th camera of the split", type=int, default=1)
    p.add_argument("--scale", help="multicam data: fuse the cameras of the first SCALE pyramid levels only (1: the full-size images)", type=int,
                   default=1)
    p.add_argument("--grid", help="lattice points per axis: N, or NX NY NZ", type=int, nargs="+", default=[256])
    p.add_argument("--bound", help="the box is [-bound, bound]^3 in world coordinates", type=float, default=1.5)
    p.add_argument("--aabb", help="the box x0 y0 z0 x1 y1 z1 (overrides --bound)", type=float, nargs=6, default=None)
    p.add_argument("--trunc_cells", help="truncation distance in units of the largest lattice spacing (default 3: a choice, not a measurement)",
                   type=float, default=DEFAULT_TRUNC_CELLS)
    p.add_argument("--quantile", help="the opacity whose depth is the surface (0.5: the median depth)", type=float, default=0.5)
    p.add_argument("--unseen", help="a lattice point no camera updated: inside (space carving) or outside (an inner shell wherever the object "
                   "is thicker than the truncation)", choices=["inside", "outside"], default="inside")
    p.add_argument("--no_carve", dest="carve", help="rays without a depth do not free the space they cross", action="store_false")
    p.add_argument("--no_color", dest="color", help="no vertex colours", action="store_false")
    p.add_argument("--save_depth", help="also write every depth map as a PNG", action="store_true")
    p.add_argument("--save_tsdf", help="also write the finalised lattice [nz, ny, nx] as .npy", action="store_true")
    return p


def refuse_before_rendering(args):
    """what the flags alone decide: before a checkpoint is read or a file is written"""
    try:
        check_fuse_arguments(args.trunc_cells, args.quantile, args.unseen)
    except ValueError as e:
        raise SystemExit(str(e).replace("fuse_mesh: quantile", "--quantile").replace("fuse_mesh: trunc_cells", "--trunc_cells"))
    if args.every < 1:
        raise SystemExit(f"--every must be at least 1, got {args.every}")
    if args.scale < 1:
        raise SystemExit(f"--scale must be at least 1, got {args.scale}")
    if args.data is None:
        raise SystemExit("the cameras to fuse come from a data set: give --data")
    args.space = None                      # the box of lattice_of: a world box for every model
    return lattice_of(args)


def split_cameras(system, args, device):
    """[F, 32] float32 camera records of the split: the data set's own table, or ideal pinholes of the capture's K at its poses"""
    from .datasets import PathGen, dataset_dict
    hp = system.hparams
    scene360 = is_scene360(hp)
    kw = {"factor": args.factor if args.factor is not None else int(hp.get("factor", 4))} if scene360 else {}
    listed = None                          # the frames the split's own index lists, where there is one to read before any image is
    for name, count in (("transforms_%s.json" % args.split, lambda m: len(m["frames"])),
                        ("metadata.json", lambda m: len(m.get(args.split, {}).get("file_path", [])))):
        if not scene360 and listed is None and os.path.exists(os.path.join(args.data, name)):
            import json
            with open(os.path.join(args.data, name)) as f:
                listed = count(json.load(f))
    if listed == 0:
        raise SystemExit(f"the {args.split} split of {args.data} has no frames to fuse")
    dataset = dataset_dict[hp["dataset_name"]](data_dir=args.data, split=args.split, white_bkgd=hp["val.white_bkgd"],
                                              batch_type="all_images" if args.split == "train" else "single_image", device=device, **kw)
    if scene360:
        cams = PathGen(dataset, poses=dataset.camtoworlds, device=device).cameras
    else:
        cams = dataset.cameras
        if hp["dataset_name"] == "multicam":          # levels are interleaved per frame or listed level by level: keep the largest images
            widths = sorted({float(w) for w in cams[:, 21].tolist()}, reverse=True)[:args.scale]
            cams = cams[torch.isin(cams[:, 21], torch.tensor(widths, dtype=cams.dtype))]
    return cams.to(torch.float32)[::args.every]


def main(argv=None):
    args = build_parser().parse_args(argv)
    dims, lo, hi = refuse_before_rendering(args)
    system = load_system(args)
    dev = torch.device("cuda", torch.cuda.current_device())
    system = system.to(dev).eval()
    cams = split_cameras(system, args, dev)
    if cams.shape[0] == 0:
        raise SystemExit(f"the {args.split} split of {args.data} has no frames to fuse (--every {args.every})")
    folder = os.path.join(args.out_dir, "mesh", system.hparams["exp_name"])
    os.makedirs(folder, exist_ok=True)
    on_frame = None
    if args.save_depth:
        from PIL import Image
        from . import ops
        os.makedirs(os.path.join(folder, "depth"), exist_ok=True)

        def on_frame(f, depth, frame):
            finite = torch.where(torch.isinf(depth), torch.zeros_like(depth), depth)
            Image.fromarray(ops.visualize_map(finite).cpu().numpy()).save(os.path.join(folder, "depth", f"{f:05d}_depth.png"))
    tsdf, stats = fuse_volume(system, cams, grid=dims, lo=lo, hi=hi, trunc_cells=args.trunc_cells, quantile=args.quantile, carve=args.carve,
                              precision=args.precision, chunk=args.chunk_size, on_frame=on_frame)
    mesh = mesh_of_volume(system, tsdf, unseen=args.unseen, color=args.color, precision=args.precision)
    tag = "x".join(str(d) for d in dims)
    path = write_ply(os.path.join(folder, f"fused_{tag}.ply"), mesh.vertices, mesh.normals, mesh.faces, mesh.colors)
    if args.save_tsdf:
        np.save(os.path.join(folder, f"tsdf_{tag}.npy"), mesh.sigma.cpu().numpy())
    unseen = float((tsdf.count == 0).float().mean())
    print(f"{path}: {stats['views']} views, {mesh.vertices.shape[0]} vertices, {mesh.faces.shape[0]} faces, {100.0 * unseen:.2f} % of the "
          f"lattice points unseen (called {args.unseen}), {100.0 * stats['pixels_without_depth'] / max(stats['pixels'], 1):.2f} % of the pixels "
          f"without a depth (opacity below {args.quantile:g})")
    return path


if __name__ == "__main__":
    main()
