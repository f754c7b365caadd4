"""Command line of the mesh extraction (no counterpart in the reference; flags shared with render_video / eval where they apply):

    python -m mipnerf_pl_amd.extract_mesh --ckpt CKPT --out_dir OUT [--grid 256 | --grid NX NY NZ] [--bound 1.5 | --aabb x0 y0 z0 x1 y1 z1]
                                          [--threshold 10] [--cov_scale 1] [--precision fp32|bf16] [--no_color] [--save_density]
                                          [--space world|contracted [--far_radius 64]]

Writes OUT/mesh/<exp_name>/mesh_<nx>x<ny>x<nz>.ply (and density_<nx>x<ny>x<nz>.npy with --save_density) and prints the number of
vertices and faces and the share of lattice points inside the surface.  A checkpoint of the unbounded-scene model (llff / realdata360)
needs --space: `world` meshes a box in world coordinates (the central object), `contracted` the whole scene -- the lattice is uniform in
the contracted coordinates, the box defaults to [-2, 2]^3, and no vertex lies beyond --far_radius; the files are then named
mesh_<space>_<nx>x<ny>x<nz>.ply and density_<space>_<nx>x<ny>x<nz>.npy."""
from __future__ import annotations

import argparse
import os

import numpy as np
import torch

from .mesh import DEFAULT_THRESHOLD, default_box, extract_mesh, write_ply
from .render_video import add_common_args, load_system


class _NotGiven(float):
    """The default of --bound.  It has to read as 1.5 (the parsed default is part of this command line's tested surface) and still be told from
    a typed `--bound 1.5`, because with --space contracted an untyped bound means the whole contracted space, [-2, 2]^3."""


def build_parser():
    p = add_common_args(argparse.ArgumentParser(prog="python -m mipnerf_pl_amd.extract_mesh"))
    p.add_argument("--grid", help="lattice points per axis: N, or NX NY NZ", type=int, nargs="+", default=[256])
    p.add_argument("--bound", help="the box is [-bound, bound]^3 (default 1.5; 2 with --space contracted)", type=float, default=_NotGiven(1.5))
    p.add_argument("--aabb", help="the box x0 y0 z0 x1 y1 z1 (overrides --bound)", type=float, nargs=6, default=None)
    p.add_argument("--threshold", help="density of the surface; scene dependent -- the default is a choice, not a measurement: look at the "
                   "share of points inside that is printed, or at --save_density", type=float, default=DEFAULT_THRESHOLD)
    p.add_argument("--cov_scale", help="lattice Gaussians' variance in units of a uniform cell's (0: point queries)", type=float, default=1.0)
    p.add_argument("--no_color", dest="color", help="no vertex colours", action="store_false")
    p.add_argument("--save_density", help="also write the density volume [nz, ny, nx] as .npy", action="store_true")
    p.add_argument("--space", help="checkpoints of the unbounded-scene model (llff / realdata360) only, which need it: the space the lattice "
                   "lies in -- world coordinates, or the contracted coordinates that hold the whole scene", choices=["world", "contracted"],
                   default=None)
    p.add_argument("--far_radius", help="--space contracted: no vertex lies beyond this distance from the origin (world units)", type=float,
                   default=64.0)
    return p


def lattice_of(args):
    """(dims, lo, hi) of the parsed flags."""
    if len(args.grid) not in (1, 3):
        raise SystemExit("--grid takes one number or three")
    dims = tuple(args.grid) if len(args.grid) == 3 else tuple(args.grid) * 3
    if args.aabb is not None:
        return dims, tuple(args.aabb[:3]), tuple(args.aabb[3:])
    if isinstance(args.bound, _NotGiven):
        return (dims,) + default_box(args.space)
    return dims, (-args.bound,) * 3, (args.bound,) * 3


def main(argv=None):
    args = build_parser().parse_args(argv)
    dims, lo, hi = lattice_of(args)
    system = load_system(args).to(torch.device("cuda")).eval()
    mesh = extract_mesh(system, grid=dims, lo=lo, hi=hi, threshold=args.threshold, cov_scale=args.cov_scale, color=args.color,
                        precision=args.precision, space=args.space, far_radius=args.far_radius)
    folder = os.path.join(args.out_dir, "mesh", system.hparams["exp_name"])
    os.makedirs(folder, exist_ok=True)
    tag = ("" if args.space is None else args.space + "_") + "x".join(str(d) for d in dims)
    path = write_ply(os.path.join(folder, f"mesh_{tag}.ply"), mesh.vertices, mesh.normals, mesh.faces, mesh.colors)
    if args.save_density:
        np.save(os.path.join(folder, f"density_{tag}.npy"), mesh.sigma.cpu().numpy())
    inside = float((mesh.sigma > args.threshold).float().mean())
    print(f"{path}: {mesh.vertices.shape[0]} vertices, {mesh.faces.shape[0]} faces, {100.0 * inside:.2f} % of the lattice points inside "
          f"(density > {args.threshold:g})")
    return path


if __name__ == "__main__":
    main()
