"""A coloured triangle mesh out of a trained field, on the device.

`extract_mesh(system_or_model, grid=256, ...)`: the field's density on a lattice of Gaussians of the lattice spacing
(`ops.density_grid`: an anti-aliased volume at any resolution), its isosurface by marching tetrahedra (`ops.isosurface`), and the MLP's
colour at every vertex seen against the surface normal (`ops.field_at`, bytes by `ops.image_to_u8`).  `write_ply` / `read_ply`: binary
little-endian PLY with float positions and normals, uchar colours and int faces -- what viewers, slicers and physics tools load.
The unbounded-scene model's field lives in a contracted space, so its mesh has to name the lattice's space: `space="world"` (a box in
world coordinates, for the central object of a capture) or `space="contracted"` (the whole scene: the surface is cut in contracted
coordinates and un-contracted, `ops.uncontract`); without a `space` that model is refused."""
from __future__ import annotations

from typing import NamedTuple, Optional

import numpy as np
import torch

from . import ops

DEFAULT_THRESHOLD = 10.0      # a choice, not a measurement: the density where a surface is drawn depends on the scene's scale


class Mesh(NamedTuple):
    vertices: torch.Tensor                 # [V, 3] float32
    normals: torch.Tensor                  # [V, 3] float32, unit (or 0 where the gradient vanishes), pointing to lower density
    faces: torch.Tensor                    # [F, 3] int32, normal from inside to outside
    colors: Optional[torch.Tensor]         # [V, 3] uint8, or None
    sigma: torch.Tensor                    # [nz, ny, nx] float32, the density volume the surface was cut from
    rgb: Optional[torch.Tensor] = None     # [V, 3] float32, the colours before quantisation
    vertices_contracted: Optional[torch.Tensor] = None     # [V, 3] float32, space="contracted" only: the vertices where the surface was cut


def _triple(v, cast):
    return tuple(cast(x) for x in (v if hasattr(v, "__len__") else (v,) * 3))


def lattice_variance(dims, lo, hi, cov_scale):
    """cov_scale * h * h / 12 per axis in float32, h = (hi - lo) / float32(n - 1): the lattice Gaussians' variance as the kernel forms it."""
    lo, hi = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
    h = (hi - lo) / (np.asarray(dims) - 1).astype(np.float32)
    return np.float32(cov_scale) * h * h / np.float32(12)


CONTRACTED_BOUND = 2.0        # the contracted space is the ball |z| < 2


def default_box(space):
    """(lo, hi) of a mesh whose box is not given: [-1.5, 1.5]^3, or all of the contracted space [-2, 2]^3"""
    b = CONTRACTED_BOUND if space == "contracted" else 1.5
    return (-b,) * 3, (b,) * 3


def extract_mesh(system_or_model, grid=256, lo=None, hi=None, threshold=DEFAULT_THRESHOLD, cov_scale=1.0, color=True,
                 precision=None, space=None, far_radius=64.0):
    """Density volume -> isosurface at `threshold` -> vertex colours.  `grid`: points per axis, or (nx, ny, nz); lo / hi: the box,
    (x, y, z) (default: `default_box(space)`).  Colours are the MLP's activated rgb at each vertex as a Gaussian of the lattice's variance,
    seen along -normal.  `space` (unbounded=True models, which need it): 'world' -- the lattice lies in world coordinates --, or
    'contracted': the surface is cut in the contracted coordinates, coloured at the contracted vertices seen along minus the WORLD normal,
    and then positions and normals are un-contracted (`ops.uncontract`; no vertex beyond `far_radius`); `vertices_contracted` keeps the
    cut.  Where the surface reaches the box or the far sphere it is cut open, not capped."""
    box = default_box(space)
    dims, lo, hi = _triple(grid, int), _triple(box[0] if lo is None else lo, float), _triple(box[1] if hi is None else hi, float)
    with torch.no_grad():
        sigma = ops.density_grid(system_or_model, dims, lo, hi, cov_scale=cov_scale, precision=precision, space=space, far_radius=far_radius)
        vertices, normals, faces = ops.isosurface(sigma, threshold, lo, hi)
        cut = None
        if space == "contracted":
            cut = vertices
            vertices, normals = ops.uncontract(cut, normals, far_radius=far_radius)
        rgb = colors = None
        if color:
            var = torch.from_numpy(lattice_variance(dims, lo, hi, cov_scale)).to(vertices.device)
            at = vertices if cut is None else cut
            rgb = ops.field_at(system_or_model, at, var.expand(at.shape[0], 3), -normals, precision=precision, space=space)[:, :3].contiguous()
            colors = ops.image_to_u8(rgb) if rgb.numel() else torch.empty(0, 3, dtype=torch.uint8, device=rgb.device)
    return Mesh(vertices, normals, faces, colors, sigma, rgb, cut)


def _ply_header(num_vertices, num_faces, with_color):
    lines = ["ply", "format binary_little_endian 1.0", "comment mipnerf_pl_amd.mesh", f"element vertex {num_vertices}",
             "property float x", "property float y", "property float z", "property float nx", "property float ny", "property float nz"]
    if with_color:
        lines += ["property uchar red", "property uchar green", "property uchar blue"]
    lines += [f"element face {num_faces}", "property list uchar int vertex_indices", "end_header"]
    return ("\n".join(lines) + "\n").encode("ascii")


def _vertex_dtype(with_color):
    fields = [(n, "<f4") for n in ("x", "y", "z", "nx", "ny", "nz")]
    if with_color:
        fields += [(n, "u1") for n in ("red", "green", "blue")]
    return np.dtype(fields)


_FACE_DTYPE = np.dtype([("n", "u1"), ("v", "<i4", (3,))])


def _host(a, dtype):
    if torch.is_tensor(a):
        a = a.detach().cpu().numpy()
    return np.ascontiguousarray(a, dtype=dtype)


def write_ply(path, vertices, normals, faces, colors=None):
    """Binary little-endian PLY: vertex = float x y z, float nx ny nz[, uchar red green blue]; face = uchar count (3) + int indices."""
    v, n, f = _host(vertices, np.float32).reshape(-1, 3), _host(normals, np.float32).reshape(-1, 3), _host(faces, np.int32).reshape(-1, 3)
    if n.shape != v.shape:
        raise ValueError("write_ply: one normal per vertex")
    rec = np.empty(v.shape[0], _vertex_dtype(colors is not None))
    for k, name in enumerate(("x", "y", "z")):
        rec[name] = v[:, k]
        rec["n" + name] = n[:, k]
    if colors is not None:
        c = _host(colors, np.uint8).reshape(-1, 3)
        if c.shape != v.shape:
            raise ValueError("write_ply: one colour per vertex")
        for k, name in enumerate(("red", "green", "blue")):
            rec[name] = c[:, k]
    fr = np.empty(f.shape[0], _FACE_DTYPE)
    fr["n"] = 3
    fr["v"] = f
    with open(path, "wb") as out:
        out.write(_ply_header(v.shape[0], f.shape[0], colors is not None))
        out.write(rec.tobytes())
        out.write(fr.tobytes())
    return path


def read_ply(path):
    """Inverse of `write_ply`: (vertices [V, 3] float32, normals [V, 3] float32, faces [F, 3] int32, colors [V, 3] uint8 or None)."""
    with open(path, "rb") as f:
        data = f.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    head = data[:end].decode("ascii").split("\n")
    if head[:2] != ["ply", "format binary_little_endian 1.0"]:
        raise ValueError(f"{path}: not a binary little-endian PLY")
    nv = int(next(ln for ln in head if ln.startswith("element vertex ")).split()[2])
    nf = int(next(ln for ln in head if ln.startswith("element face ")).split()[2])
    with_color = "property uchar red" in head
    if data[:end] != _ply_header(nv, nf, with_color):
        raise ValueError(f"{path}: not a header write_ply writes")
    vd = _vertex_dtype(with_color)
    rec = np.frombuffer(data, vd, nv, end)
    fr = np.frombuffer(data, _FACE_DTYPE, nf, end + nv * vd.itemsize)
    if len(data) != end + nv * vd.itemsize + nf * _FACE_DTYPE.itemsize or (nf and not (fr["n"] == 3).all()):
        raise ValueError(f"{path}: truncated, or faces that are not triangles")
    v = np.stack([rec["x"], rec["y"], rec["z"]], -1)
    n = np.stack([rec["nx"], rec["ny"], rec["nz"]], -1)
    c = np.stack([rec["red"], rec["green"], rec["blue"]], -1) if with_color else None
    return v, n, fr["v"].copy(), c
