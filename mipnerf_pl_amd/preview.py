"""Bake a trained field into a dense lattice of density + spherical-harmonic colour and render frames from the lattice alone.

The PlenOctrees / Plenoxels idea in its simplest dense form (include/mipnerf_preview.h states the row layout and the marching rules):

    bake_field(system)          `ops.density_grid` -> sigma, `ops.occupancy_grid` -> bits, `ops.field_at` once per direction of a Fibonacci
                                sphere at the lattice Gaussians of the points next to an occupied cell, `fit_sh`, mipnerf_preview_pack
    render_rays(baked, rays)    mipnerf_preview_march: no MLP, one wavefront per ray
    PreviewFrame                the frame-shaped wrapper (`render` / `images` like `evaluate.FrameEvaluator`)

    bake_field(system, sparse=True) / BakedField.to_sparse()    a `SparseField`: only the rows next to an occupied cell, behind a row table
                                (include/mipnerf_preview_sparse.h); marched by mipnerf_preview_sparse_march to the same bytes

    march_grad / TuneState / tune_field    mipnerf_preview_tune_grad + mipnerf_preview_tune_adam (include/mipnerf_preview_tune.h): the
                                gradient of `march` with respect to the rows and Adam steps on them against photos or the MLP's renders;
                                a single dense `BakedField` only, and the float-atomic sums are not bitwise reproducible
    tune_regularise             mipnerf_preview_reg_grad (include/mipnerf_preview_reg.h): the gradient of a total-variation term and of
                                an SH decay on the master rows, added between the two by `TuneState(tv_sigma=, tv_colour=, sh_decay=)`

    bake_pyramid(system)        `bake_field` at grid, then at about half the points per axis, ...: a `BakedPyramid`
    march_pyramid / render_rays of a pyramid    mipnerf_preview_mip_march (include/mipnerf_preview_mip.h): every sample reads the level (or
                                the two levels) whose spacing brackets footprint * radius * t, the width of the ray's cone there

    python -m mipnerf_pl_amd.preview --ckpt CKPT --out_dir OUT [--grid 256 | --grid NX NY NZ] [--sh_degree 0|1|2] [--bound B]
        [--threshold 0.01] [--dilate 1] [--step 0.5] [--t_min 1e-3] [--precision fp32|bf16] [--n_poses 120] [--scale 1]
        [--save_baked] [--baked FILE] [--data DIR --compare] [--mip [L]] [--footprint F] [--sparse]
        [--tune STEPS [--tune_batch 65536] [--tune_lr_sigma 0.2] [--tune_lr_colour 0.01] [--tune_target photos|mlp] [--tune_seed 0]
                      [--tune_tv_sigma 0] [--tune_tv_colour 0] [--tune_sh_decay 0] [--tune_tv_eps 1e-4]]
    python -m mipnerf_pl_amd.preview --ckpt CKPT --data DIR --out_dir OUT --space contracted [--far_radius R] [--bound B] [--split test]
        [--n_views 30] [--factor F] [--sparse] [--compare] [--save_baked] [--baked FILE]      (a llff / realdata360 checkpoint: the unbounded-scene model)

renders the spherical path of `render_video` to OUT/preview_spheric/<exp_name>/ and prints one `preview:` line.

THE BAKED PICTURE IS NOT THE MLP'S PICTURE: colour is a low-order expansion in the view direction fitted to `n_dirs` directions, density
and colour are blended trilinearly between lattice points, and without `--mip` the march takes point samples of one lattice (no cones:
that preview is not anti-aliased).  With `--mip` the coarser lattices, baked at their own lattice Gaussians, are the field pre-filtered
at their spacing, and the cone radius chooses between them.  `--data DIR --compare` measures how far below the MLP either scores.
Two-level models only.  Without `--space` the model must be bounded; `--space contracted` bakes the unbounded-scene model into a lattice
over its contracted space and marches it along straight world rays (include/mipnerf_preview_360.h): `bake_field(..., space='contracted',
far_radius=R)`, the interpolated path of `render_video`, frames in OUT/preview_path/<exp_name>/1/.
"""
from __future__ import annotations

import argparse
import ctypes as C
import os
import time

import numpy as np
import torch

from . import _lib as L

SH_C0 = 0.28209479177387814
SH_C1 = 0.4886025119029199
SH_C2 = (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)
ROW_HALVES = {0: 4, 1: 16, 2: 32}
# Choices, not measurements: half a cell per step keeps two samples in every cell a ray crosses; a march that stops at T < 1e-3 leaves out
# at most 1e-3 of any output; 32 directions over-determine the 9 coefficients of degree 2 about 3.5 times.
DEFAULT_STEP_SCALE = 0.5
DEFAULT_T_MIN = 1e-3
DEFAULT_MAX_STEPS = 4096
DEFAULT_N_DIRS = 32
# Choices as well: with radii = dx / sqrt(3) (the data sets' convention) a footprint of sqrt(3) makes w = footprint * radius * t one pixel's
# width; 4 levels reach 8 times the finest spacing, the 1 / 8 scale of the multi-scale Blender set.
DEFAULT_FOOTPRINT = float(np.sqrt(3.0))
DEFAULT_MIP_LEVELS = 4
MAX_MIP_LEVELS = L.PREVIEW_MIP_MAX_LEVELS


def _check_degree(degree, who):
    if degree not in (0, 1, 2):
        raise NotImplementedError(f"{who}: the spherical-harmonic degree must be 0, 1 or 2 (got {degree!r})")
    return int(degree)


def sh_basis(dirs, degree):
    """The real spherical harmonics up to `degree` (0..2) at unit directions [..., 3] -> [..., (degree + 1)^2], in the order and signs of
    PlenOctrees: [C0, -C1 y, C1 z, -C1 x, C20 xy, C21 yz, C22 (2zz - xx - yy), C23 xz, C24 (xx - yy)].  Pure torch; the dtype of `dirs`."""
    degree = _check_degree(degree, "sh_basis")
    x, y, z = dirs[..., 0], dirs[..., 1], dirs[..., 2]
    out = [torch.full_like(x, SH_C0)]
    if degree >= 1:
        out += [-SH_C1 * y, SH_C1 * z, -SH_C1 * x]
    if degree >= 2:
        out += [SH_C2[0] * x * y, SH_C2[1] * y * z, SH_C2[2] * (2.0 * z * z - x * x - y * y), SH_C2[3] * x * z, SH_C2[4] * (x * x - y * y)]
    return torch.stack(out, -1)


def fit_sh(rgb, dirs, degree):
    """Least-squares coefficients of colours seen from K directions: rgb [M, K, 3], unit dirs [K, 3] -> [M, (degree + 1)^2, 3] (the
    dtype of `rgb`).  The float64 pseudo-inverse of the [K, (degree + 1)^2] basis matrix, applied as one float64 matmul."""
    degree = _check_degree(degree, "fit_sh")
    if rgb.dim() != 3 or rgb.shape[-1] != 3 or dirs.shape != (rgb.shape[1], 3):
        raise ValueError(f"fit_sh: expected rgb [M, K, 3] and dirs [K, 3], got {tuple(rgb.shape)} and {tuple(dirs.shape)}")
    basis = sh_basis(dirs.to(device=rgb.device, dtype=torch.float64), degree)
    if basis.shape[0] < basis.shape[1]:
        raise ValueError(f"fit_sh: {basis.shape[0]} directions do not determine the {basis.shape[1]} coefficients of degree {degree}")
    pinv = torch.linalg.pinv(basis.cpu()).to(rgb.device)              # [(degree + 1)^2, K]; a few hundred numbers, on the host
    return torch.matmul(pinv, rgb.to(torch.float64)).to(rgb.dtype)


def bake_directions(K=DEFAULT_N_DIRS):
    """K unit directions of a Fibonacci sphere, [K, 3] float64 on the host."""
    if K < 1:
        raise ValueError("bake_directions: K must be positive")
    i = torch.arange(K, dtype=torch.float64)
    z = 1.0 - (2.0 * i + 1.0) / K
    phi = i * (np.pi * (3.0 - np.sqrt(5.0)))
    r = torch.sqrt(torch.clamp(1.0 - z * z, min=0.0))
    return torch.stack([r * torch.cos(phi), r * torch.sin(phi), z], -1)


def _dims3(grid):
    dims = [int(d) for d in (grid if hasattr(grid, "__len__") else (grid,) * 3)]
    if len(dims) != 3:
        raise ValueError(f"the lattice has three sizes (nx, ny, nz), got {grid!r}")
    return tuple(dims)


def check_lattice(dims, who):
    """The lattices the library takes: at least 2 points per axis and 7 nx ny nz < 2^31 (the occupancy grid's rule)."""
    dims = _dims3(dims)
    if min(dims) < 2:
        raise ValueError(f"{who}: a lattice needs at least 2 points per axis (got {dims})")
    if 7 * dims[0] * dims[1] * dims[2] >= 2 ** 31:
        raise ValueError(f"{who}: the lattice {dims} is too large: 7 nx ny nz must stay below 2^31")
    return dims


def _box3(v):
    return tuple(float(np.float32(x)) for x in (v if hasattr(v, "__len__") else (v,) * 3))


def _check_space(space, far_radius, who):
    """(space, far_radius) of a lattice: (None, None) in world coordinates, ('contracted', R) with a finite R > 1 otherwise."""
    if space not in (None, "contracted"):
        raise ValueError(f"{who}: space must be None or 'contracted', got {space!r}")
    if space is None:
        if far_radius is not None:
            raise ValueError(f"{who}: far_radius belongs to space='contracted' (a lattice in world coordinates is cut by its box)")
        return None, None
    if far_radius is None or not (float(far_radius) > 1.0 and np.isfinite(float(far_radius))):
        raise ValueError(f"{who}: a contracted lattice needs far_radius, finite and > 1 (got {far_radius!r})")
    return space, float(np.float32(far_radius))


def _space_arrays(baked):
    """The two .npz keys a contracted lattice adds (a lattice in world coordinates keeps its key set)."""
    if baked.space is None:
        return {}
    return dict(space=np.array(baked.space), far_radius=np.float32(baked.far_radius))


def _stored_space(z):
    """(space, far_radius) of saved arrays."""
    if "space" not in z:
        return None, None
    return str(z["space"]), float(z["far_radius"])


def refuse_contracted(baked, who):
    """What is not implemented for a lattice of the contracted space (a pyramid of them, their gradient, tuning them)."""
    fields = baked.levels if isinstance(baked, BakedPyramid) else [baked]
    if any(getattr(b, "space", None) is not None for b in fields):
        raise NotImplementedError(f"{who}: a contracted lattice (space='contracted', the unbounded-scene model) is not supported here: "
                                  "a contracted pyramid is not implemented; the gradient and the tuning of a contracted lattice live in "
                                  "mipnerf_pl_amd.preview_tune360 (march_grad, TuneState360, tune_field; the command "
                                  "`python -m mipnerf_pl_amd.preview_tune360`)")


class BakedField:
    """A baked lattice: `rows` fp16 [nz, ny, nx, W] (W = 4 / 16 / 32 for degree 0 / 1 / 2; row[0] = sigma, row[1 + 3k + c] = coefficient k
    of channel c), `dims` = (nx, ny, nz), the box `lo` .. `hi` in (x, y, z) order, `degree`, `occupancy` (an `ops.Occupancy` over the
    same lattice, or None: every cell is marched) and the density `threshold` its bits were built with.  `space`: None -- the box lies in
    world coordinates (the bounded model) -- or 'contracted' -- in the contracted coordinates of the unbounded-scene model, with
    `far_radius` the world radius its rays are cut at (include/mipnerf_preview_360.h); `march` dispatches on it."""

    def __init__(self, rows, dims, lo, hi, degree, occupancy=None, threshold=None, space=None, far_radius=None):
        self.space, self.far_radius = _check_space(space, far_radius, "BakedField")
        self.degree = _check_degree(degree, "BakedField")
        self.dims = check_lattice(dims, "BakedField")
        self.lo, self.hi = _box3(lo), _box3(hi)
        if not all(h > l for l, h in zip(self.lo, self.hi)):
            raise ValueError(f"BakedField: the box needs hi > lo on every axis (got {self.lo} .. {self.hi})")
        nx, ny, nz = self.dims
        if rows.dtype != torch.float16 or tuple(rows.shape) != (nz, ny, nx, ROW_HALVES[self.degree]) or not rows.is_contiguous():
            raise ValueError(f"BakedField: rows must be contiguous fp16 [nz, ny, nx, W] = {(nz, ny, nx, ROW_HALVES[self.degree])}, "
                             f"got {rows.dtype} {tuple(rows.shape)}")
        if occupancy is not None and (tuple(occupancy.dims) != self.dims or tuple(occupancy.bits.shape) != (nz - 1, ny - 1, (nx + 30) // 32)):
            raise ValueError("BakedField: the occupancy grid must lie on the rows' lattice")
        self.rows, self.occupancy = rows, occupancy
        self.threshold = None if threshold is None else float(threshold)

    @property
    def nbytes(self) -> int:
        """Bytes of the rows and the occupancy words."""
        n = self.rows.numel() * 2
        return n + (self.occupancy.bits.numel() * 4 if self.occupancy is not None else 0)

    def baked_share(self) -> float:
        """Share of the lattice points that carry colour coefficients (a read-back)."""
        if self.rows.shape[-1] <= 1:
            return 0.0
        return float((self.rows[..., 1:4] != 0).any(-1).float().mean())         # the three DC coefficients

    def save(self, path):
        """Everything in one .npz (the rows as fp16, the bits as uint32)."""
        with open(path, "wb") as f:
            np.savez(f, **self._arrays())
        return path

    def _arrays(self):
        occ = self.occupancy
        arrays = dict(rows=self.rows.cpu().numpy(), dims=np.array(self.dims, np.int32), lo=np.array(self.lo, np.float32),
                      hi=np.array(self.hi, np.float32), degree=np.int32(self.degree),
                      threshold=np.float32(np.nan if self.threshold is None else self.threshold))
        if occ is not None:
            arrays["occupancy"] = occ.bits.cpu().numpy().view(np.uint32)
            arrays["dilate"] = np.int32(-1 if occ.dilate is None else occ.dilate)
        arrays.update(_space_arrays(self))
        return arrays

    @staticmethod
    def stored_space(path):
        """The space of a saved lattice or pyramid (None or 'contracted'), without reading its rows."""
        with np.load(path) as z:
            return str(z["space"]) if "space" in z.files else None

    @staticmethod
    def stored_degree(path) -> int:
        """The degree of a saved lattice, without reading its rows."""
        with np.load(path) as z:
            return int(z["degree"])

    @classmethod
    def load(cls, path, device="cuda"):
        with np.load(path) as z:
            if "sparse_rows" in z.files:
                raise ValueError(f"{path} holds a sparse lattice, not a dense one: load it with SparseField.load")
            if "rows" not in z.files:
                raise ValueError(f"{path} holds a pyramid of lattices, not a single one: load it with BakedPyramid.load")
            return cls._from_arrays({k: z[k] for k in z.files}, device)

    @staticmethod
    def _stored_occupancy(z, dims, lo, hi, device):
        """The `ops.Occupancy` of saved arrays (None when they hold none) and the threshold."""
        from .ops import Occupancy
        thr = float(z["threshold"])
        occ = None
        if "occupancy" in z:
            occ = Occupancy(torch.from_numpy(z["occupancy"].view(np.int32)).to(device).view(torch.uint32), dims, lo, hi,
                            space=_stored_space(z)[0])
            occ.threshold, occ.dilate = (None if np.isnan(thr) else thr), (None if int(z["dilate"]) < 0 else int(z["dilate"]))
        return occ, (None if np.isnan(thr) else thr)

    @classmethod
    def _from_arrays(cls, z, device):
        dims, lo, hi = tuple(int(v) for v in z["dims"]), z["lo"], z["hi"]
        rows = torch.from_numpy(z["rows"]).to(device)
        occ, thr = cls._stored_occupancy(z, dims, lo, hi, device)
        return cls(rows, dims, lo, hi, int(z["degree"]), occ, thr, *_stored_space(z))

    def to_sparse(self, stored=None):
        """The same lattice as a `SparseField`: mipnerf_preview_sparse_index on the occupancy words (or on the words of `stored`, an
        `ops.Occupancy` of the cells whose corners are kept: a level of a pyramid keeps more than its own occupied cells, see
        `pyramid_storage`), mipnerf_preview_sparse_gather on the rows.  Marching it gives the bytes marching this one gives.  Refused
        without an occupancy: every row would be stored."""
        if self.occupancy is None:
            raise ValueError("BakedField.to_sparse: a lattice without an occupancy grid marches every cell, so every row is read: it stays dense")
        table, m = index_table(self.occupancy if stored is None else stored)
        return SparseField(gather_rows(self.rows, table, m, self.degree), table, self.dims, self.lo, self.hi, self.degree, self.occupancy,
                           self.threshold, stored=stored, _table_is_ours=True, space=self.space, far_radius=self.far_radius)


def table_words(nx) -> int:
    """Table words per x-line of POINTS, ceil(nx / 32): not the occupancy grid's ceil((nx - 1) / 32)."""
    return (int(nx) + 31) // 32


def table_of_points(points):
    """The row table of include/mipnerf_preview_sparse.h restated in torch, on any device: int32 [nz, ny, words_p, 2] (the bits of uint32
    words) of the stored points bool [nz, ny, nx], and the stored count.  `SparseField` checks a foreign table against it; the tables the
    bake uses come from mipnerf_preview_sparse_index."""
    nz, ny, nx = points.shape
    wp = table_words(nx)
    bits = torch.zeros(nz, ny, wp * 32, dtype=torch.int64, device=points.device)
    bits[..., :nx] = points
    bits = bits.view(nz, ny, wp, 32)
    mask = (bits << torch.arange(32, dtype=torch.int64, device=points.device)).sum(-1)
    count = bits.sum(-1)
    rank = (torch.cumsum(count.reshape(-1), 0) - count.reshape(-1)).view(nz, ny, wp)
    mask = torch.where(mask >= 2 ** 31, mask - 2 ** 32, mask)           # the uint32 word's bits as an int32
    return torch.stack([mask, rank], -1).to(torch.int32).contiguous(), int(count.sum())


def index_table(occ):
    """mipnerf_preview_sparse_index: (table int32 [nz, ny, ceil(nx / 32), 2], M) of an `ops.Occupancy`; M is read back."""
    nx, ny, nz = occ.dims
    dev = occ.bits.device
    cdims = (C.c_int32 * 3)(nx, ny, nz)
    lib = L.preview_sparse_lib()
    table = torch.empty(nz, ny, table_words(nx), 2, dtype=torch.int32, device=dev)
    total = torch.zeros(1, dtype=torch.int32, device=dev)
    scratch = torch.empty(max(1, (int(lib.mipnerf_preview_sparse_scratch_bytes(cdims)) + 3) // 4), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        L.preview_sparse_check(lib.mipnerf_preview_sparse_index(cdims, occ.bits.data_ptr(), table.data_ptr(), total.data_ptr(),
                                                                scratch.data_ptr(), torch.cuda.current_stream().cuda_stream),
                               "preview_sparse_index")
    return table, int(total.item())


def gather_rows(dense_rows, table, m, degree):
    """mipnerf_preview_sparse_gather: the rows fp16 [m, W] of the stored points of dense rows [nz, ny, nx, W]."""
    nz, ny, nx, W = dense_rows.shape
    rows = torch.empty(m, W, dtype=torch.float16, device=dense_rows.device)
    if m > 0:
        with torch.cuda.device(dense_rows.device):
            L.preview_sparse_check(L.preview_sparse_lib().mipnerf_preview_sparse_gather(
                (C.c_int32 * 3)(nx, ny, nz), degree, table.data_ptr(), dense_rows.data_ptr(), rows.data_ptr(),
                torch.cuda.current_stream().cuda_stream), "preview_sparse_gather")
    return rows


def sparse_pack(sigma, coef, degree, out):
    """mipnerf_preview_sparse_pack: fp16 rows `out` [n, W] of sigma fp32 [n] and coef fp32 [n, (degree + 1)^2, 3], one stored point each."""
    degree = _check_degree(degree, "sparse_pack")
    n = sigma.numel()
    if sigma.dtype != torch.float32 or coef.dtype != torch.float32 or not sigma.is_contiguous() or not coef.is_contiguous() or \
            coef.numel() != n * (degree + 1) ** 2 * 3:
        raise ValueError("sparse_pack: sigma fp32 [n] and coef fp32 [n, (degree + 1)^2, 3], contiguous")
    if out.dtype != torch.float16 or tuple(out.shape) != (n, ROW_HALVES[degree]) or not out.is_contiguous():
        raise ValueError(f"sparse_pack: out must be contiguous fp16 [n, W] = {(n, ROW_HALVES[degree])}")
    with torch.cuda.device(sigma.device):
        L.preview_sparse_check(L.preview_sparse_lib().mipnerf_preview_sparse_pack(n, degree, sigma.data_ptr(), coef.data_ptr(), out.data_ptr(),
                                                                                  torch.cuda.current_stream().cuda_stream),
                               "preview_sparse_pack")
    return out


def cells_to_bits(cells):
    """The words of `ops.Occupancy` of cells bool [nz - 1, ny - 1, nx - 1]: uint32 [nz - 1, ny - 1, ceil((nx - 1) / 32)] on their device."""
    cz, cy, cx = cells.shape
    wx = (cx + 31) // 32
    bits = torch.zeros(cz, cy, wx * 32, dtype=torch.int64, device=cells.device)
    bits[..., :cx] = cells
    words = (bits.view(cz, cy, wx, 32) << torch.arange(32, dtype=torch.int64, device=cells.device)).sum(-1)
    return torch.where(words >= 2 ** 31, words - 2 ** 32, words).to(torch.int32).contiguous().view(torch.uint32)


# Two lattices over one box find the cell of a point with fp32 arithmetic each (lattice_sample.hpp): (x - lo) * inv_h carries a relative
# error of a few 1e-7, so a point within that distance of a cell face may land on either side of it.  Cells count as sharing a point when
# their intervals come closer than this share of the box edge: 40 times that error, and far below the 1 / 1024 of the smallest cell.
STORAGE_EPS = 1e-5


def _axis_overlap(n_to, n_from, device):
    """float [n_to - 1, n_from - 1]: 1 where cell a of n_to points and cell b of n_from points over one edge share a point (widened by
    STORAGE_EPS), formed in float64."""
    a = torch.arange(n_to, dtype=torch.float64) / (n_to - 1)
    b = torch.arange(n_from, dtype=torch.float64) / (n_from - 1)
    share = (a[:-1, None] < b[None, 1:] + STORAGE_EPS) & (b[None, :-1] < a[1:, None] + STORAGE_EPS)
    return share.to(device=device, dtype=torch.float32)


def pyramid_storage(occupancies):
    """The cells each level of a sparse pyramid must keep the corners of, as one `ops.Occupancy` per level.

    A sample between two levels is occupied when the bit of EITHER level's cell is set (P5 of include/mipnerf_preview_mip.h) and then
    reads BOTH levels, so a level is also read in cells whose own bit is clear: wherever a point of such a cell lies in an occupied cell
    of the level below or above.  Per level: its own occupied cells, plus every cell that shares a point with an occupied cell of a
    neighbouring level (the overlap per axis, widened by STORAGE_EPS for the fp32 index rule; three small matrix products per
    neighbour).  A single level keeps its own occupied cells: the grid itself is returned."""
    from .ops import Occupancy
    occupancies = list(occupancies)
    if len(occupancies) == 1:
        return occupancies
    cells = [occupied_cells(o) for o in occupancies]
    out = []
    for i, occ in enumerate(occupancies):
        keep = cells[i].clone()
        for j in (i - 1, i + 1):
            if not 0 <= j < len(occupancies):
                continue
            v = cells[j].to(torch.float32)
            ax, ay, az = (_axis_overlap(occ.dims[a], occupancies[j].dims[a], v.device) for a in range(3))
            v = torch.matmul(v, ax.t())                                             # [z', y', x]
            v = torch.matmul(ay, v)                                                 # [z', y, x]
            v = torch.matmul(az, v.reshape(v.shape[0], -1)).view(az.shape[0], ay.shape[0], ax.shape[0])
            keep |= v > 0
        stored = Occupancy(cells_to_bits(keep), occ.dims, occ.lo, occ.hi)
        stored.threshold, stored.dilate = occ.threshold, None
        out.append(stored)
    return out


def _covers(stored, needed) -> bool:
    """Whether every set bit of `needed` is set in `stored` (two `ops.Occupancy` over one lattice)."""
    return not bool((needed.bits.view(torch.int32) & ~stored.bits.view(torch.int32)).any())


class SparseField:
    """A baked lattice that stores only the rows a march reads (include/mipnerf_preview_sparse.h): `rows` fp16 [M, W], one per lattice
    point next to an occupied cell, in flat point order; `table` int32 [nz, ny, ceil(nx / 32), 2] (the bits of uint32 words: per 32 points
    of an x-line their stored bits and the number of stored points before them); `occupancy` (an `ops.Occupancy`, never None) and the
    rest as in `BakedField`.  Marching it gives the bytes marching the dense lattice with the same occupancy gives.

    `stored` (an `ops.Occupancy` over the same lattice, or None = `occupancy`): the cells whose corners have rows.  It holds at least the
    occupied cells; a level of a pyramid holds more (`pyramid_storage`).  The march reads `occupancy`; `stored` only says what the table
    was built from.  The table must be the one of `stored`'s bits: a constructor given a table recomputes it and refuses another."""

    def __init__(self, rows, table, dims, lo, hi, degree, occupancy, threshold=None, stored=None, _table_is_ours=False, space=None,
                 far_radius=None):
        self.space, self.far_radius = _check_space(space, far_radius, "SparseField")      # as in `BakedField`
        self.degree = _check_degree(degree, "SparseField")
        self.dims = check_lattice(dims, "SparseField")
        self.lo, self.hi = _box3(lo), _box3(hi)
        if not all(h > l for l, h in zip(self.lo, self.hi)):
            raise ValueError(f"SparseField: the box needs hi > lo on every axis (got {self.lo} .. {self.hi})")
        nx, ny, nz = self.dims
        if occupancy is None:
            raise ValueError("SparseField: a sparse lattice needs its occupancy grid (without one every row is read: use BakedField)")
        if tuple(occupancy.dims) != self.dims or tuple(occupancy.bits.shape) != (nz - 1, ny - 1, (nx + 30) // 32):
            raise ValueError("SparseField: the occupancy grid must lie on the rows' lattice")
        if stored is occupancy:
            stored = None
        if stored is not None:
            if tuple(stored.dims) != self.dims or stored.bits.shape != occupancy.bits.shape or stored.bits.device != occupancy.bits.device:
                raise ValueError("SparseField: the stored cells must lie on the rows' lattice")
            if not _covers(stored, occupancy):
                raise ValueError("SparseField: an occupied cell is not among the stored cells (a march would read rows that are not there)")
        if table.dtype != torch.int32 or tuple(table.shape) != (nz, ny, table_words(nx), 2) or not table.is_contiguous():
            raise ValueError(f"SparseField: table must be contiguous int32 [nz, ny, ceil(nx / 32), 2] = {(nz, ny, table_words(nx), 2)}, "
                             f"got {table.dtype} {tuple(table.shape)}")
        if rows.dtype != torch.float16 or rows.dim() != 2 or rows.shape[1] != ROW_HALVES[self.degree] or not rows.is_contiguous():
            raise ValueError(f"SparseField: rows must be contiguous fp16 [M, W], W = {ROW_HALVES[self.degree]}, got {rows.dtype} "
                             f"{tuple(rows.shape)}")
        if not (rows.device == table.device == occupancy.bits.device):
            raise ValueError("SparseField: rows, table and occupancy live on one device")
        if not _table_is_ours:
            cells = occupancy if stored is None else stored
            want, m = index_table(cells) if rows.is_cuda else table_of_points(baked_points(cells))
            if not torch.equal(want, table):
                raise ValueError("SparseField: the table is not the one of the stored cells' bits (a march would read rows of other points)")
            if rows.shape[0] != m:
                raise ValueError(f"SparseField: the stored cells have {m} corner points, rows holds {rows.shape[0]}")
        self.rows, self.table, self.occupancy, self.stored = rows, table, occupancy, stored
        self.threshold = None if threshold is None else float(threshold)

    @property
    def n_rows(self) -> int:
        return int(self.rows.shape[0])

    @property
    def nbytes(self) -> int:
        """Bytes of what a march reads: the rows, the table and the occupancy words."""
        return self.rows.numel() * 2 + self.table.numel() * 4 + self.occupancy.bits.numel() * 4

    @property
    def dense_nbytes(self) -> int:
        """Bytes the dense lattice takes: `BakedField.nbytes` of `to_dense()`."""
        nx, ny, nz = self.dims
        return nx * ny * nz * ROW_HALVES[self.degree] * 2 + self.occupancy.bits.numel() * 4

    def stored_share(self) -> float:
        """Share of the lattice points that have a row."""
        nx, ny, nz = self.dims
        return self.n_rows / float(nx * ny * nz)

    def baked_share(self) -> float:
        """Share of the lattice points that carry colour coefficients, as `BakedField.baked_share` (a read-back)."""
        if self.rows.shape[-1] <= 1 or self.n_rows == 0:
            return 0.0
        nx, ny, nz = self.dims
        return float((self.rows[:, 1:4] != 0).any(-1).sum()) / float(nx * ny * nz)

    def stored_points(self):
        """bool [nz, ny, nx]: the points that have a row (`baked_points` of the stored cells)."""
        return baked_points(self.occupancy if self.stored is None else self.stored)

    def to_dense(self):
        """A `BakedField` with the stored rows at their points and ZEROS elsewhere.  That is not what `bake_field` leaves at an unstored
        point (it keeps the point's sigma there), so the result equals the dense bake in the stored rows only -- which are the only rows
        a march with this occupancy reads."""
        nx, ny, nz = self.dims
        dense = torch.zeros(nz * ny * nx, ROW_HALVES[self.degree], dtype=torch.float16, device=self.rows.device)
        dense[self.stored_points().reshape(-1)] = self.rows
        return BakedField(dense.view(nz, ny, nx, -1), self.dims, self.lo, self.hi, self.degree, self.occupancy, self.threshold, self.space,
                          self.far_radius)

    def save(self, path):
        """Everything in one .npz with keys of its own (`sparse_rows` and `table` where a dense lattice has `rows`)."""
        with open(path, "wb") as f:
            np.savez(f, **self._arrays())
        return path

    def _arrays(self):
        occ = self.occupancy
        arrays = dict(sparse_rows=self.rows.cpu().numpy(), table=self.table.cpu().numpy().view(np.uint32), dims=np.array(self.dims, np.int32),
                      lo=np.array(self.lo, np.float32), hi=np.array(self.hi, np.float32), degree=np.int32(self.degree),
                      threshold=np.float32(np.nan if self.threshold is None else self.threshold),
                      occupancy=occ.bits.cpu().numpy().view(np.uint32), dilate=np.int32(-1 if occ.dilate is None else occ.dilate))
        if self.stored is not None:
            arrays["stored"] = self.stored.bits.cpu().numpy().view(np.uint32)
        arrays.update(_space_arrays(self))
        return arrays

    @classmethod
    def load(cls, path, device="cuda"):
        with np.load(path) as z:
            if "levels" in z.files:
                raise ValueError(f"{path} holds a pyramid of lattices, not a single one: load it with BakedPyramid.load")
            if "sparse_rows" not in z.files:
                raise ValueError(f"{path} holds a dense lattice, not a sparse one: load it with BakedField.load")
            return cls._from_arrays({k: z[k] for k in z.files}, device)

    @classmethod
    def _from_arrays(cls, z, device):
        dims, lo, hi = tuple(int(v) for v in z["dims"]), z["lo"], z["hi"]
        from .ops import Occupancy
        occ, thr = BakedField._stored_occupancy(z, dims, lo, hi, device)
        stored = None
        if "stored" in z:
            stored = Occupancy(torch.from_numpy(z["stored"].view(np.int32)).to(device).view(torch.uint32), dims, lo, hi,
                               space=_stored_space(z)[0])
        space, far_radius = _stored_space(z)
        return cls(torch.from_numpy(z["sparse_rows"]).to(device), torch.from_numpy(z["table"].view(np.int32)).to(device), dims, lo, hi,
                   int(z["degree"]), occ, thr, stored=stored, space=space, far_radius=far_radius)


def lattice_spacing(dims, lo, hi) -> float:
    """The smallest axis spacing of a lattice as the libraries form it: the fp32 (hi - lo) / float(n - 1), then the minimum."""
    lo32, hi32 = np.asarray(_box3(lo), np.float32), np.asarray(_box3(hi), np.float32)
    return float(((hi32 - lo32) / (np.asarray(_dims3(dims)) - 1).astype(np.float32)).min())


class BakedPyramid:
    """`levels`: 1 .. 8 `BakedField`s -- or 1 .. 8 `SparseField`s, never a mix -- over ONE box (lo and hi equal bit for bit) with one
    degree, the finest first; the smallest axis spacing increases strictly from level to level (rule P1 of
    include/mipnerf_preview_mip.h)."""

    def __init__(self, levels):
        levels = list(levels)
        if not 1 <= len(levels) <= MAX_MIP_LEVELS or not all(isinstance(b, (BakedField, SparseField)) for b in levels):
            raise ValueError(f"BakedPyramid: 1 .. {MAX_MIP_LEVELS} BakedField levels (got {len(levels)})")
        if len({isinstance(b, SparseField) for b in levels}) != 1:
            raise ValueError("BakedPyramid: the levels are all dense (BakedField) or all sparse (SparseField), not a mix: one kernel "
                             "instantiation marches them all")
        first = levels[0]
        if any(b.space is not None for b in levels):
            raise NotImplementedError("BakedPyramid: a contracted lattice (space='contracted') cannot be a level: a contracted pyramid is "
                                      "not implemented")
        for i, b in enumerate(levels[1:], 1):
            if np.asarray(b.lo, np.float32).tobytes() != np.asarray(first.lo, np.float32).tobytes() or \
                    np.asarray(b.hi, np.float32).tobytes() != np.asarray(first.hi, np.float32).tobytes():
                raise ValueError(f"BakedPyramid: level {i} spans {b.lo} .. {b.hi}, level 0 spans {first.lo} .. {first.hi}: one box for all")
            if b.degree != first.degree:
                raise ValueError(f"BakedPyramid: level {i} has degree {b.degree}, level 0 has degree {first.degree}")
            if b.rows.device != first.rows.device:
                raise ValueError("BakedPyramid: all levels live on one device")
        self.spacings = tuple(lattice_spacing(b.dims, b.lo, b.hi) for b in levels)
        if not all(a < b for a, b in zip(self.spacings, self.spacings[1:])):
            raise ValueError(f"BakedPyramid: the smallest spacing must increase strictly from level to level (got {self.spacings})")
        if isinstance(first, SparseField) and len(levels) > 1:
            for i, (b, need) in enumerate(zip(levels, pyramid_storage([b.occupancy for b in levels]))):
                if not _covers(b.occupancy if b.stored is None else b.stored, need):
                    raise ValueError(f"BakedPyramid: level {i} does not store the rows a sample between two levels reads (a level is read "
                                     "wherever its neighbour's cell is occupied): make its `stored` cells with pyramid_storage")
        self.levels = levels

    def __len__(self):
        return len(self.levels)

    lo = property(lambda self: self.levels[0].lo)
    hi = property(lambda self: self.levels[0].hi)
    degree = property(lambda self: self.levels[0].degree)
    device = property(lambda self: self.levels[0].rows.device)
    sparse = property(lambda self: isinstance(self.levels[0], SparseField))

    @property
    def nbytes(self) -> int:
        """Bytes of the rows and the occupancy words (and, when sparse, the tables) of every level."""
        return sum(b.nbytes for b in self.levels)

    @property
    def dense_nbytes(self) -> int:
        """Bytes the pyramid takes with dense levels."""
        return sum(b.dense_nbytes if self.sparse else b.nbytes for b in self.levels)

    def stored_share(self) -> float:
        """Share of the lattice points of all levels that have a row (1 for dense levels)."""
        if not self.sparse:
            return 1.0
        return sum(b.n_rows for b in self.levels) / float(sum(int(np.prod(b.dims)) for b in self.levels))

    def to_sparse(self):
        """Every level through `BakedField.to_sparse`, keeping the cells of `pyramid_storage`."""
        if any(b.occupancy is None for b in self.levels):
            raise ValueError("BakedPyramid.to_sparse: a level without an occupancy grid marches every cell, so every row is read: it stays dense")
        return BakedPyramid([b.to_sparse(stored) for b, stored in zip(self.levels, pyramid_storage([b.occupancy for b in self.levels]))])

    def save(self, path):
        """Every level in one .npz: `levels` and the shared `degree`, then the arrays of `BakedField.save` (or `SparseField.save`, and then
        `sparse` = 1 beside `levels`) of level i as `l<i>_<name>`."""
        arrays = dict(levels=np.int32(len(self.levels)), degree=np.int32(self.degree))
        if self.sparse:
            arrays["sparse"] = np.int32(1)
        for i, b in enumerate(self.levels):
            for k, v in b._arrays().items():
                arrays[f"l{i}_{k}"] = v
        with open(path, "wb") as f:
            np.savez(f, **arrays)
        return path

    @staticmethod
    def stored_levels(path):
        """The level count of a saved pyramid without reading its rows; None: the file holds a single `BakedField`."""
        with np.load(path) as z:
            return int(z["levels"]) if "levels" in z.files else None

    @staticmethod
    def stored_sparse(path) -> bool:
        """Whether a saved lattice or pyramid is sparse, without reading its rows."""
        with np.load(path) as z:
            return "sparse" in z.files or "sparse_rows" in z.files

    @classmethod
    def load(cls, path, device="cuda"):
        with np.load(path) as z:
            if "levels" not in z.files:
                raise ValueError("{0} holds a single lattice, not a pyramid: load it with {1}".format(
                    path, "SparseField.load" if "sparse_rows" in z.files else "BakedField.load"))
            kind = SparseField if "sparse" in z.files else BakedField
            return cls([kind._from_arrays({k[len(f"l{i}_"):]: z[k] for k in z.files if k.startswith(f"l{i}_")}, device)
                        for i in range(int(z["levels"]))])


def refuse_model(model_or_system, who, space=None):
    """The bake covers the bounded two-level model, and with space='contracted' the unbounded-scene two-level model; anything else is
    refused with the reason."""
    m = getattr(model_or_system, "mip_nerf", model_or_system)
    if space not in (None, "contracted"):
        raise ValueError(f"{who}: space must be None or 'contracted', got {space!r}")
    if space == "contracted" and not bool(getattr(m, "unbounded", False)):
        raise ValueError(f"{who}: space='contracted' bakes the unbounded-scene model (unbounded=True); this model is bounded: its lattice "
                         "lies in world coordinates (drop space=)")
    if space is None and bool(getattr(m, "unbounded", False)):
        raise NotImplementedError(f"{who}: unbounded=True models are not supported (their field lives in a contracted space; a contracted "
                                  "lattice is not implemented)")
    if int(getattr(m, "num_levels", 2)) != 2:
        raise NotImplementedError(f"{who}: only the two-level model is baked (num_levels = {m.num_levels}): the lattice stands for the "
                                  "field its fine level renders")


def occupied_cells(occ):
    """The bits of an `ops.Occupancy` as a bool tensor [nz - 1, ny - 1, nx - 1] on its device."""
    nx, ny, nz = occ.dims
    words = occ.bits.view(torch.int32)
    shifts = torch.arange(32, dtype=torch.int32, device=words.device)
    bits = (words[..., None] >> shifts) & 1                         # the arithmetic shift's sign copies are masked away
    return bits.reshape(nz - 1, ny - 1, -1)[..., :nx - 1].bool()


def baked_points(occ):
    """bool [nz, ny, nx]: the lattice points next to an occupied cell (any of the up to 8 cells around a point), so every corner of an
    occupied cell is among them."""
    nx, ny, nz = occ.dims
    cells = occupied_cells(occ)
    pts = torch.zeros(nz, ny, nx, dtype=torch.bool, device=cells.device)
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                pts[dz:dz + nz - 1, dy:dy + ny - 1, dx:dx + nx - 1] |= cells
    return pts


def lattice_gaussians(dims, lo, hi, cov_scale, index):
    """Means [M, 3] and variances [M, 3] (fp32, the device of `index`) of the lattice Gaussians at the flat point indices `index`, as
    `ops.density_grid` states them: mean = lo + float32(i) * h, variance = cov_scale * h * h / 12, h = (hi - lo) / float32(n - 1)."""
    nx, ny, nz = dims
    lo32, hi32 = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
    h = (hi32 - lo32) / np.array([nx - 1, ny - 1, nz - 1], np.float32)
    var = (np.float32(cov_scale) * h * h) / np.float32(12.0)
    dev = index.device
    ijk = torch.stack([index % nx, (index // nx) % ny, index // (nx * ny)], -1).to(torch.float32)
    means = torch.from_numpy(lo32).to(dev) + ijk * torch.from_numpy(h).to(dev)
    return means, torch.from_numpy(var).to(dev).expand(index.shape[0], 3).contiguous()


def pack_rows(sigma, coef, degree, mask=None, out=None):
    """mipnerf_preview_pack: fp16 rows [nz, ny, nx, W] of sigma fp32 [nz, ny, nx] and coef fp32 [nz, ny, nx, (degree + 1)^2, 3]; `mask`
    (uint8 / bool per point, optional): 0 = the colour coefficients are written as zeros."""
    degree = _check_degree(degree, "pack_rows")
    nz, ny, nx = sigma.shape
    nb = (degree + 1) ** 2
    if sigma.dtype != torch.float32 or coef.dtype != torch.float32 or not sigma.is_contiguous() or not coef.is_contiguous() or \
            coef.numel() != sigma.numel() * nb * 3:
        raise ValueError("pack_rows: sigma fp32 [nz, ny, nx] and coef fp32 [nz, ny, nx, (degree + 1)^2, 3], contiguous")
    if mask is not None:
        mask = mask.to(torch.uint8).contiguous()
        if mask.numel() != sigma.numel():
            raise ValueError("pack_rows: one mask byte per lattice point")
    if out is None:
        out = torch.empty(nz, ny, nx, ROW_HALVES[degree], dtype=torch.float16, device=sigma.device)
    cdims = (C.c_int32 * 3)(nx, ny, nz)
    with torch.cuda.device(sigma.device):
        L.preview_check(L.preview_lib().mipnerf_preview_pack(cdims, degree, sigma.data_ptr(), coef.data_ptr(),
                                                             None if mask is None else mask.data_ptr(), out.data_ptr(),
                                                             torch.cuda.current_stream().cuda_stream), "preview_pack")
    return out


def bake_field(model_or_system, grid=256, degree=1, lo=None, hi=None, threshold=0.01, dilate=1, n_dirs=DEFAULT_N_DIRS, cov_scale=1.0,
               precision=None, chunk=None, sparse=False, space=None, far_radius=None, _grids=None, _stored=None):
    """Bake the field of a bounded two-level model into a `BakedField` of `grid`^3 (or (nx, ny, nz)) points over lo .. hi; with
    `sparse=True` into a `SparseField`, the bytes of `bake_field(...).to_sparse()`, without ever allocating dense rows or dense
    coefficients: after sigma and the bits come the table (mipnerf_preview_sparse_index) and the stored points in slot order, and every
    chunk of them goes through `ops.field_at`, `fit_sh` and mipnerf_preview_sparse_pack straight into its rows.  (`bake_pyramid` hands
    in what it has made already: `_grids` = (sigma, bits) and `_stored` = the level's cells of `pyramid_storage`; a stored point that is
    not a baked point gets its sigma and zero coefficients, as in the dense rows.)

    sigma = `ops.density_grid`; bits = `ops.occupancy_grid(sigma, threshold, dilate)`; a point is baked iff any of the up to 8 cells around
    it is occupied; at the baked points `ops.field_at` runs once per direction of `bake_directions(n_dirs)` on the lattice Gaussian
    (variance cov_scale h^2 / 12), `chunk` points at a time (default 2^20), then `fit_sh` and mipnerf_preview_pack.  The MLP is reached
    through those public ops only.  `precision`: 'fp32' / 'bf16' (default: the model's).

    `space='contracted'` (with `far_radius`, finite and > 1) bakes the unbounded-scene model: the lattice spans lo .. hi of the CONTRACTED
    space (default [-2, 2]^3, all of it), sigma = `ops.density_grid(space='contracted', far_radius=far_radius)`, and `ops.field_at(space=
    'contracted')` runs on the lattice Gaussians (variance cov_scale h^2 / 12 in contracted coordinates) with world view directions.
    The result carries `space` and `far_radius`, and `march` sends it through mipnerf_preview_360_march."""
    from . import ops
    refuse_model(model_or_system, "bake_field", space)
    space, far_radius = _check_space(space, far_radius, "bake_field")
    degree = _check_degree(degree, "bake_field")
    dims = check_lattice(grid, "bake_field")
    if space is not None:
        lo, hi = -2.0 if lo is None else lo, 2.0 if hi is None else hi
    where = {} if space is None else dict(space=space, far_radius=far_radius)
    if lo is None or hi is None:
        raise ValueError("bake_field: give the box lo .. hi the lattice spans (the rays to be rendered are marched inside it only)")
    if (degree + 1) ** 2 > n_dirs:
        raise ValueError(f"bake_field: {n_dirs} directions do not determine the {(degree + 1) ** 2} coefficients of degree {degree}")
    chunk = (1 << 20) if chunk is None else int(chunk)
    if chunk < 1:
        raise ValueError("bake_field: chunk must be positive")
    lo, hi = _box3(lo), _box3(hi)
    nx, ny, nz = dims
    nb = (degree + 1) ** 2
    with torch.no_grad():
        if _grids is None:
            sigma = ops.density_grid(model_or_system, dims, lo, hi, cov_scale=cov_scale, precision=precision, **where)
            occ = ops.occupancy_grid(sigma, threshold, lo, hi, dilate=dilate)
            occ.space = space
        else:
            sigma, occ = _grids
        dev = sigma.device
        mask = baked_points(occ)
        dirs = bake_directions(n_dirs)
        dirs32 = dirs.to(device=dev, dtype=torch.float32)

        def coefficients(idx):
            means, var = lattice_gaussians(dims, lo, hi, cov_scale, idx)
            rgb = torch.empty(idx.numel(), n_dirs, 3, dtype=torch.float32, device=dev)
            for k in range(n_dirs):
                rgb[:, k] = ops.field_at(model_or_system, means, var, dirs32[k].expand(idx.numel(), 3), precision=precision, space=space)[:, :3]
            return fit_sh(rgb, dirs, degree)

        if sparse:
            table, m = index_table(occ if _stored is None else _stored)
            stored = mask if _stored is None else baked_points(_stored)
            index = torch.nonzero(stored.reshape(-1)).reshape(-1)       # flat order is slot order
            baked = None if _stored is None else mask.reshape(-1)[index]
            del mask, stored
            rows = torch.empty(m, ROW_HALVES[degree], dtype=torch.float16, device=dev)
            for c0 in range(0, m, chunk):
                idx = index[c0:c0 + chunk]
                if baked is None:
                    coef = coefficients(idx).contiguous()
                else:
                    coef = torch.zeros(idx.numel(), nb, 3, dtype=torch.float32, device=dev)
                    keep = baked[c0:c0 + chunk]
                    if bool(keep.any()):
                        coef[keep] = coefficients(idx[keep])
                sparse_pack(sigma.reshape(-1)[idx], coef, degree, rows[c0:c0 + chunk])
            return SparseField(rows, table, dims, lo, hi, degree, occ, threshold, stored=_stored, _table_is_ours=True, **where)
        rows = torch.empty(nz, ny, nx, ROW_HALVES[degree], dtype=torch.float16, device=dev)
        # dense coefficients only for a slab of z layers at a time (at least 2: the library's smallest lattice)
        layers = min(nz, max(2, (1 << 24) // (nx * ny)))
        starts = list(range(0, nz, layers))
        if len(starts) > 1 and nz - starts[-1] < 2:
            starts[-1] = nz - 2                                       # the last slab overlaps the one before it by a layer
        for z0 in starts:
            z1 = min(z0 + layers, nz)
            coef = torch.zeros(z1 - z0, ny, nx, nb, 3, dtype=torch.float32, device=dev)
            index = torch.nonzero(mask[z0:z1].reshape(-1)).reshape(-1) + z0 * ny * nx
            for c0 in range(0, index.numel(), chunk):
                idx = index[c0:c0 + chunk]
                coef.view(-1, nb, 3)[idx - z0 * ny * nx] = coefficients(idx)
            pack_rows(sigma[z0:z1], coef, degree, mask=mask[z0:z1], out=rows[z0:z1])
    return BakedField(rows, dims, lo, hi, degree, occ, threshold, **where)


def pyramid_dims(grid, levels, lo, hi):
    """The lattices of `bake_pyramid`: `grid`, then n_l = max(2, (n_{l-1} + 1) // 2) per axis, at most `levels` of them; the list ends early
    when the next lattice's smallest spacing would not be larger (every axis already at 2 points)."""
    if not 1 <= int(levels) <= MAX_MIP_LEVELS:
        raise ValueError(f"a pyramid has 1 .. {MAX_MIP_LEVELS} levels (got {levels})")
    out = [_dims3(grid)]
    while len(out) < int(levels):
        nxt = tuple(max(2, (n + 1) // 2) for n in out[-1])
        if not lattice_spacing(nxt, lo, hi) > lattice_spacing(out[-1], lo, hi):
            break
        out.append(nxt)
    return out


def bake_pyramid(model_or_system, grid=256, levels=DEFAULT_MIP_LEVELS, degree=1, lo=None, hi=None, **kwargs):
    """`bake_field` at `grid` and at each coarser lattice of `pyramid_dims`, over the same box and with the same arguments (`kwargs`:
    threshold, dilate, n_dirs, cov_scale, precision, chunk, sparse), as a `BakedPyramid`.  Every level is what `bake_field` returns at its
    dims: its lattice Gaussians have its own spacing, so a coarser level is the field pre-filtered at that spacing by the model's own
    integrated encoding.  Level 0 is baked first, so `bake_field`'s refusals come from `bake_field`.

    With `sparse=True` the levels are `SparseField`s and the result is `bake_pyramid(...).to_sparse()` byte for byte: sigma and the bits
    of every level come first (a level's stored cells depend on its neighbours' bits, `pyramid_storage`), then each level is baked into
    its compact rows."""
    if not 1 <= int(levels) <= MAX_MIP_LEVELS:
        raise ValueError(f"bake_pyramid: a pyramid has 1 .. {MAX_MIP_LEVELS} levels (got {levels})")
    if kwargs.get("space") is not None:
        raise NotImplementedError(f"bake_pyramid: space={kwargs['space']!r}: a contracted pyramid is not implemented (bake_field bakes a "
                                  "single contracted lattice)")
    if kwargs.get("sparse", False):
        from . import ops
        refuse_model(model_or_system, "bake_field")
        _check_degree(degree, "bake_field")
        if lo is None or hi is None:
            raise ValueError("bake_field: give the box lo .. hi the lattice spans (the rays to be rendered are marched inside it only)")
        all_dims = pyramid_dims(check_lattice(grid, "bake_field"), levels, lo, hi)
        how = {k: kwargs[k] for k in ("cov_scale", "precision") if k in kwargs}
        with torch.no_grad():
            grids = []
            for dims in all_dims:
                sigma = ops.density_grid(model_or_system, dims, _box3(lo), _box3(hi), **how)
                grids.append((sigma, ops.occupancy_grid(sigma, kwargs.get("threshold", 0.01), _box3(lo), _box3(hi), dilate=kwargs.get("dilate", 1))))
            keep = pyramid_storage([occ for _, occ in grids])
        return BakedPyramid([bake_field(model_or_system, grid=dims, degree=degree, lo=lo, hi=hi, _grids=g, _stored=(k if len(keep) > 1 else None),
                                        **kwargs) for dims, g, k in zip(all_dims, grids, keep)])
    first = bake_field(model_or_system, grid=grid, degree=degree, lo=lo, hi=hi, **kwargs)
    fields = [first]
    for dims in pyramid_dims(first.dims, levels, first.lo, first.hi)[1:]:
        fields.append(bake_field(model_or_system, grid=dims, degree=degree, lo=lo, hi=hi, **kwargs))
    return BakedPyramid(fields)


def _background(white_bkgd):
    if isinstance(white_bkgd, (bool, np.bool_, int)):
        return (1.0, 1.0, 1.0) if white_bkgd else (0.0, 0.0, 0.0)
    return tuple(float(v) for v in white_bkgd)


def _march_args(who, fields, tensors, background, step_scale, t_min, max_steps, out, steps, use_occupancy):
    """What `march` and `march_pyramid` (`who`, as the messages name it) do with their arguments: the checks of the flat ray `tensors`
    {name: tensor} and of `steps`, the outputs, one `PreviewField` struct per `BakedField` of `fields`, the `PreviewParams`."""
    B = tensors["origins"].shape[0]
    dev = fields[0].rows.device
    for name, t in tensors.items():
        shape = (B, 3) if name in ("origins", "directions") else (B,)
        if t.dtype != torch.float32 or not t.is_contiguous() or t.device != dev or t.numel() != int(np.prod(shape)):
            raise ValueError(f"{who}: {name} must be a contiguous fp32 tensor of {shape} on {dev}")
    if out is None:
        out = (torch.empty(B, 3, device=dev), torch.empty(B, device=dev), torch.empty(B, device=dev))
    if steps is not None and (steps.dtype != torch.int32 or steps.numel() != B or not steps.is_contiguous()):
        raise ValueError(f"{who}: steps must be a contiguous int32 tensor with one entry per ray")
    if not use_occupancy and any(isinstance(b, SparseField) for b in fields):
        raise ValueError(f"{who}: a sparse lattice has rows next to occupied cells only: it cannot be marched without its occupancy grid")
    structs = []
    for b in fields:
        occ = b.occupancy if use_occupancy else None
        structs.append(L.PreviewField((C.c_int32 * 3)(*b.dims), (C.c_float * 3)(*b.lo), (C.c_float * 3)(*b.hi), b.degree, b.rows.data_ptr(),
                                      None if occ is None else occ.bits.data_ptr()))
    params = L.PreviewParams(float(step_scale), float(t_min), int(max_steps), (C.c_float * 3)(*_background(background)))
    return B, dev, out, structs, params


def _march_sparse(who, fields, structs, params, footprint, B, dev, origins, directions, radii, near, far, out, steps, lod):
    """mipnerf_preview_sparse_march over the `SparseField`s `fields` (`structs`: their `PreviewField` structs from `_march_args`)."""
    rgb, acc, dist = out
    pyr = L.PreviewSparsePyramid()
    pyr.levels = len(fields)
    for i, (b, field) in enumerate(zip(fields, structs)):
        pyr.level[i] = L.PreviewSparseField(field, b.table.data_ptr(), b.n_rows)
    with torch.cuda.device(dev):
        L.preview_sparse_check(L.preview_sparse_lib().mipnerf_preview_sparse_march(
            C.byref(pyr), C.byref(params), float(footprint), B, origins.data_ptr(), directions.data_ptr(),
            None if radii is None else radii.data_ptr(), near.data_ptr(), far.data_ptr(), rgb.data_ptr(), acc.data_ptr(), dist.data_ptr(),
            None if steps is None else steps.data_ptr(), None if lod is None else lod.data_ptr(), torch.cuda.current_stream().cuda_stream), who)
    return rgb, acc, dist


def march(baked, origins, directions, near, far, background, step_scale=DEFAULT_STEP_SCALE, t_min=DEFAULT_T_MIN, max_steps=DEFAULT_MAX_STEPS,
          out=None, steps=None, use_occupancy=True):
    """mipnerf_preview_march on flat fp32 device tensors: origins / directions [B, 3], near / far [B] -> (rgb [B, 3], acc [B], distance
    [B]) (`out`: these three, preallocated).  `steps`: an int32 [B] tensor that receives the samples evaluated per ray.  A `SparseField`
    goes through mipnerf_preview_sparse_march as a pyramid of one level, with no radii and footprint 0: the same bytes.  A lattice of the
    contracted space (`baked.space == 'contracted'`, dense or sparse) goes through mipnerf_preview_360_march[_sparse]: `step_scale` then
    scales a step of the CONTRACTED space and the rays are cut by the ball of `baked.far_radius`, not by the box."""
    B, dev, (rgb, acc, dist), (field,), params = _march_args("march", [baked], dict(origins=origins, directions=directions, near=near, far=far),
                                                             background, step_scale, t_min, max_steps, out, steps, use_occupancy)
    if baked.space is not None:
        lib, sparse = L.preview_360_lib(), isinstance(baked, SparseField)
        arg = L.PreviewSparseField(field, baked.table.data_ptr(), baked.n_rows) if sparse else field
        with torch.cuda.device(dev):
            L.preview_360_check((lib.mipnerf_preview_360_march_sparse if sparse else lib.mipnerf_preview_360_march)(
                C.byref(arg), baked.far_radius, C.byref(params), B, origins.data_ptr(), directions.data_ptr(), near.data_ptr(), far.data_ptr(),
                rgb.data_ptr(), acc.data_ptr(), dist.data_ptr(), None if steps is None else steps.data_ptr(),
                torch.cuda.current_stream().cuda_stream), "preview_360_march_sparse" if sparse else "preview_360_march")
        return rgb, acc, dist
    if isinstance(baked, SparseField):
        return _march_sparse("preview_sparse_march", [baked], [field], params, 0.0, B, dev, origins, directions, None, near, far,
                             (rgb, acc, dist), steps, None)
    with torch.cuda.device(dev):
        L.preview_check(L.preview_lib().mipnerf_preview_march(C.byref(field), C.byref(params), B, origins.data_ptr(), directions.data_ptr(),
                                                              near.data_ptr(), far.data_ptr(), rgb.data_ptr(), acc.data_ptr(), dist.data_ptr(),
                                                              None if steps is None else steps.data_ptr(),
                                                              torch.cuda.current_stream().cuda_stream), "preview_march")
    return rgb, acc, dist


# ---- tuning the lattice through the renderer (include/mipnerf_preview_tune.h) --------------------------------------------------------
# Choices, not measurements: Adam's usual betas and eps; a density step of 0.2 against densities of tens to hundreds, a coefficient step
# of 0.01 against colours in [0, 1] (Plenoxels' ratio of the two is larger still).
DEFAULT_TUNE_LR_SIGMA = 0.2
DEFAULT_TUNE_LR_COLOUR = 0.01
DEFAULT_TUNE_BETAS = (0.9, 0.999)
DEFAULT_TUNE_EPS = 1e-8
DEFAULT_TUNE_BATCH = 65536
# A choice as well: the total variation's eps keeps the norm differentiable where a row equals its neighbours; 1e-4 is (1e-2)^2, small
# against squared differences of densities (tens) and of coefficients (tenths).  The three weights default to 0: the regulariser is off.
DEFAULT_TUNE_TV_EPS = 1e-4


def _refuse_tuning(baked, who):
    refuse_contracted(baked, who)
    if isinstance(baked, SparseField):
        raise NotImplementedError(f"{who}: a SparseField is not a tuning target (the gradient is scattered into dense rows): tune the dense "
                                  "BakedField, then .to_sparse()")
    if isinstance(baked, BakedPyramid):
        raise NotImplementedError(f"{who}: a BakedPyramid is not a tuning target (the gradient of the level mix is not implemented): "
                                  "tune a single BakedField")
    if not isinstance(baked, BakedField):
        raise TypeError(f"{who}: expected a BakedField, got {type(baked).__name__}")


def march_grad(baked, origins, directions, near, far, background, grad_rgb=None, grad_acc=None, target=None, loss_scale=None, grad_rows=None,
               step_scale=DEFAULT_STEP_SCALE, t_min=DEFAULT_T_MIN, max_steps=DEFAULT_MAX_STEPS, use_occupancy=True, out=None, counters=None):
    """mipnerf_preview_tune_grad: the march of `march` and its gradient with respect to the rows in one launch -> (grad_rows, rgb, acc).
    The loss side is `grad_rgb` [B, 3], or `target` [B, 3] with `loss_scale` (G = loss_scale * (rgb - target), rgb this launch's own);
    `grad_acc` [B] is optional.  `grad_rows` fp32 [nz, ny, nx, W] is ADDED INTO (None: a fresh zero tensor); rgb and acc are the bytes
    `march` gives (`out`: the two, preallocated).  `counters`: an int64 [2] tensor that is added to (samples, flushes).  The sums over
    rays use float atomics: two runs may differ in the last bits of grad_rows."""
    _refuse_tuning(baked, "march_grad")
    B, dev, _, (field,), params = _march_args("march_grad", [baked], dict(origins=origins, directions=directions, near=near, far=far),
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
        L.preview_tune_check(L.preview_tune_lib().mipnerf_preview_tune_grad(
            C.byref(field), C.byref(params), B, origins.data_ptr(), directions.data_ptr(), near.data_ptr(), far.data_ptr(), ptr(grad_rgb),
            ptr(target), 0.0 if loss_scale is None else float(loss_scale), ptr(grad_acc), rgb.data_ptr(), acc.data_ptr(), grad_rows.data_ptr(),
            ptr(counters), torch.cuda.current_stream().cuda_stream), "preview_tune_grad")
    return grad_rows, rgb, acc


def tune_adam(master, m, v, grad, rows, degree, mask, lr_sigma, lr_colour, beta1, beta2, eps, c1, c2):
    """mipnerf_preview_tune_adam on fp32 [..., W] tensors and the fp16 `rows` [..., W], in place: one Adam step on the used entries of every
    point whose `mask` byte (uint8 per point, or None) is not 0, the new rows rounded as `pack_rows` rounds them, grad cleared."""
    degree = _check_degree(degree, "tune_adam")
    W = ROW_HALVES[degree]
    n = rows.numel() // W
    for name, t in (("master", master), ("m", m), ("v", v), ("grad", grad)):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.shape != rows.shape or t.device != rows.device:
            raise ValueError(f"tune_adam: {name} must be a contiguous fp32 tensor of the rows' shape on their device")
    if rows.dtype != torch.float16 or not rows.is_contiguous() or rows.shape[-1] != W:
        raise ValueError(f"tune_adam: rows must be contiguous fp16 [..., {W}]")
    if mask is not None and (mask.dtype != torch.uint8 or mask.numel() != n or not mask.is_contiguous() or mask.device != rows.device):
        raise ValueError("tune_adam: one contiguous uint8 mask byte per point")
    with torch.cuda.device(rows.device):
        L.preview_tune_check(L.preview_tune_lib().mipnerf_preview_tune_adam(
            n, degree, master.data_ptr(), m.data_ptr(), v.data_ptr(), grad.data_ptr(), rows.data_ptr(), None if mask is None else mask.data_ptr(),
            float(lr_sigma), float(lr_colour), float(beta1), float(beta2), float(eps), float(c1), float(c2),
            torch.cuda.current_stream().cuda_stream), "preview_tune_adam")


def lattice_axis_scale(dims, lo, hi):
    """r_a = hmin / h_a of a lattice in fp32, h_a = (hi_a - lo_a) / float(n_a - 1) as the libraries form the spacings: 1 on a cubic lattice"""
    h = (np.asarray(hi, np.float32) - np.asarray(lo, np.float32)) / (np.asarray(dims) - 1).astype(np.float32)
    return (h.min() / h).astype(np.float32)


def tune_regularise(master, mask, dims, lo, hi, degree, grad, tv_sigma, tv_colour, sh_decay, tv_eps, n_points=None):
    """mipnerf_preview_reg_grad: ADD the gradient of `tv_sigma` x the total variation of the density, `tv_colour` x that of the colour
    coefficients and 0.5 `sh_decay` x the squared coefficients of k >= 1 into `grad`, each divided by `n_points`; master and grad fp32
    [nz, ny, nx, W], `mask` one uint8 per point or None.  `n_points` is the number of masked points, counted ONCE by the caller (this call
    does not synchronise); None stands for every point of the lattice and is refused with a mask.  A gather: two calls give the same bytes."""
    degree = _check_degree(degree, "tune_regularise")
    dims = check_lattice(dims, "tune_regularise")
    shape = (dims[2], dims[1], dims[0], ROW_HALVES[degree])
    for name, t in (("master", master), ("grad", grad)):
        if t.dtype != torch.float32 or not t.is_contiguous() or tuple(t.shape) != shape or t.device != master.device:
            raise ValueError(f"tune_regularise: {name} must be a contiguous fp32 tensor of {shape} on the master rows' device")
    n = dims[0] * dims[1] * dims[2]
    if mask is not None and (mask.dtype != torch.uint8 or mask.numel() != n or not mask.is_contiguous() or mask.device != master.device):
        raise ValueError("tune_regularise: one contiguous uint8 mask byte per point")
    if n_points is None:
        if mask is not None:
            raise ValueError("tune_regularise: with a mask, n_points (the number of masked points, counted once) must be given")
        n_points = n
    weights = [float(w) for w in (tv_sigma, tv_colour, sh_decay)]
    if not all(w >= 0 and np.isfinite(w) for w in weights) or not (tv_eps > 0 and np.isfinite(tv_eps)) or int(n_points) < 1:
        raise ValueError("tune_regularise: the weights must be finite and >= 0, tv_eps finite and > 0, n_points at least 1")
    scale = lattice_axis_scale(dims, lo, hi)
    with torch.cuda.device(master.device):
        L.preview_reg_check(L.preview_reg_lib().mipnerf_preview_reg_grad(
            (C.c_int32 * 3)(*dims), degree, (C.c_float * 3)(*[float(x) for x in scale]), master.data_ptr(),
            None if mask is None else mask.data_ptr(), grad.data_ptr(), *[w / int(n_points) for w in weights], float(tv_eps),
            torch.cuda.current_stream().cuda_stream), "preview_reg_grad")
    return grad


class TuneState:
    """What tuning a `BakedField` keeps beside it: fp32 master rows made from the fp16 rows, Adam's `m` and `v`, the gradient buffer and
    the point mask (`baked_points` of the occupancy: only points next to an occupied cell ever receive a gradient; None without an
    occupancy).  `step` updates `baked.rows` in place; the occupancy never changes.  The two learning rates are choices, not measurements.
    `tv_sigma`, `tv_colour`, `sh_decay` (default 0: off) weigh the regulariser of `tune_regularise`, per masked point; `tv_eps` is a choice."""

    def __init__(self, baked, lr_sigma=DEFAULT_TUNE_LR_SIGMA, lr_colour=DEFAULT_TUNE_LR_COLOUR, betas=DEFAULT_TUNE_BETAS, eps=DEFAULT_TUNE_EPS,
                 step_scale=DEFAULT_STEP_SCALE, t_min=DEFAULT_T_MIN, max_steps=DEFAULT_MAX_STEPS, tv_sigma=0.0, tv_colour=0.0, sh_decay=0.0,
                 tv_eps=DEFAULT_TUNE_TV_EPS):
        self._refuse(baked)
        if not (lr_sigma >= 0 and lr_colour >= 0 and 0 <= betas[0] < 1 and 0 <= betas[1] < 1 and eps >= 0):
            raise ValueError("TuneState: learning rates and eps must not be negative, the betas must lie in [0, 1)")
        if not all(w >= 0 and np.isfinite(w) for w in (tv_sigma, tv_colour, sh_decay)) or not (tv_eps > 0 and np.isfinite(tv_eps)):
            raise ValueError("TuneState: tv_sigma, tv_colour and sh_decay must be finite and >= 0, tv_eps finite and > 0")
        self.tv_sigma, self.tv_colour, self.sh_decay, self.tv_eps = float(tv_sigma), float(tv_colour), float(sh_decay), float(tv_eps)
        self._n_points = None        # the masked points, counted (one synchronisation) by the first regularised step
        self.baked = baked
        self.lr_sigma, self.lr_colour, self.betas, self.eps = float(lr_sigma), float(lr_colour), (float(betas[0]), float(betas[1])), float(eps)
        self.step_scale, self.t_min, self.max_steps = float(step_scale), float(t_min), int(max_steps)
        self.master = baked.rows.float()
        self.m, self.v, self.grad = torch.zeros_like(self.master), torch.zeros_like(self.master), torch.zeros_like(self.master)
        self.mask = None if baked.occupancy is None else baked_points(baked.occupancy).to(torch.uint8).contiguous()
        self.steps = 0
        self.counters = None         # an int64 [2] tensor here makes every step count its samples and flushes

    # the two things that depend on the space the lattice lives in (preview_tune360.TuneState360 overrides them): which lattices are
    # refused, and the call that marches a batch and adds its gradient into self.grad
    def _refuse(self, baked):
        _refuse_tuning(baked, "TuneState")

    def _march_grad(self, *args, **kwargs):
        return march_grad(*args, **kwargs)

    def step(self, rays, target, white_bkgd):
        """One step on a batch: `rays` (a `Rays` of [..., k] tensors), `target` [..., 3] -> the batch's mean squared error BEFORE the step,
        a 0-d device tensor.  mipnerf_preview_tune_grad in target mode with loss_scale = 2 / (3 B), then mipnerf_preview_tune_adam."""
        n = int(np.prod(rays.origins.shape[:-1]))
        o, d, near, far = (t.reshape(n, t.shape[-1]).float().contiguous() for t in (rays.origins, rays.directions, rays.near, rays.far))
        target = target.reshape(n, 3).float().contiguous()
        _, rgb, _ = self._march_grad(self.baked, o, d, near.reshape(n), far.reshape(n), white_bkgd, target=target, loss_scale=2.0 / (3.0 * n),
                                     grad_rows=self.grad, step_scale=self.step_scale, t_min=self.t_min, max_steps=self.max_steps,
                                     counters=self.counters)
        loss = ((rgb - target) ** 2).mean()
        self.steps += 1
        if self.regularised:
            tune_regularise(self.master, self.mask, self.baked.dims, self.baked.lo, self.baked.hi, self.baked.degree, self.grad, self.tv_sigma,
                            self.tv_colour, self.sh_decay, self.tv_eps, self.n_points)
        b1, b2 = self.betas
        tune_adam(self.master, self.m, self.v, self.grad, self.baked.rows, self.baked.degree, self.mask, self.lr_sigma, self.lr_colour, b1, b2,
                  self.eps, 1.0 / (1.0 - b1 ** self.steps), 1.0 / (1.0 - b2 ** self.steps))
        return loss

    @property
    def regularised(self) -> bool:
        return self.tv_sigma != 0.0 or self.tv_colour != 0.0 or self.sh_decay != 0.0

    @property
    def n_points(self) -> int:
        """the points the regulariser's weights are divided by: the masked ones (all without a mask), counted once"""
        if self._n_points is None:
            self._n_points = int(self.master[..., 0].numel() if self.mask is None else self.mask.sum())
        return self._n_points

    def state_dict(self):
        return dict(master=self.master, m=self.m, v=self.v, steps=self.steps, lr_sigma=self.lr_sigma, lr_colour=self.lr_colour,
                    betas=self.betas, eps=self.eps, tv_sigma=self.tv_sigma, tv_colour=self.tv_colour, sh_decay=self.sh_decay,
                    tv_eps=self.tv_eps)

    def load_state_dict(self, state):
        for k in ("master", "m", "v"):
            if tuple(state[k].shape) != tuple(self.master.shape):
                raise ValueError(f"TuneState.load_state_dict: {k} has shape {tuple(state[k].shape)}, the lattice {tuple(self.master.shape)}")
            getattr(self, k).copy_(state[k])
        self.steps = int(state["steps"])
        self.lr_sigma, self.lr_colour, self.eps = float(state["lr_sigma"]), float(state["lr_colour"]), float(state["eps"])
        self.betas = (float(state["betas"][0]), float(state["betas"][1]))
        for k in ("tv_sigma", "tv_colour", "sh_decay", "tv_eps"):      # a dict saved without them says nothing about them: they stay
            if k in state:
                setattr(self, k, float(state[k]))
        self.grad.zero_()
        self.baked.rows.copy_(pack_master(self.master, self.baked.degree))


def pack_master(master, degree):
    """fp32 master rows -> fp16 rows with the pack's rounding (sigma saturates at the fp16 maximum), pure torch."""
    rows = master.clone()
    rows[..., 0] = torch.clamp(rows[..., 0], max=65504.0)
    return rows.to(torch.float16)


def tune_field(baked, rays_and_targets, steps, white_bkgd=True, state=None, **kwargs):
    """`steps` steps of `TuneState.step` on `baked`: `rays_and_targets(step)` -> (Rays, target [B, 3]).  Returns (state, losses), the losses
    a [steps] device tensor of each batch's mean squared error before its step.  `kwargs` go to `TuneState`."""
    if steps < 1:
        raise ValueError("tune_field: at least one step")
    state = TuneState(baked, **kwargs) if state is None else state
    losses = []
    for k in range(int(steps)):
        rays, target = rays_and_targets(k)
        losses.append(state.step(rays, target, white_bkgd))
    return state, torch.stack(losses)


def photo_batches(train_dataset, batch, seed=0):
    """Batches of a train split: uniform pixel ids from a seeded device generator through `dataset.rays_at` -> (Rays, pixels [B, 3])."""
    dev = train_dataset.device if getattr(train_dataset, "device", None) is not None else torch.device("cuda", torch.cuda.current_device())
    gen = torch.Generator(device=dev)
    gen.manual_seed(int(seed))
    total = int(train_dataset.num_pixels)

    def draw(step):
        ids = torch.randint(0, total, (int(batch),), generator=gen, device=dev, dtype=torch.int64)
        rays, pixels = train_dataset.rays_at(ids)
        return rays, (None if pixels is None else pixels[..., :3])      # (a `PathPixels` has no photos: `mlp_batches` supplies the target)
    return draw


class PathPixels:
    """The pixels of the frames of a camera path (`datasets.RenderGen`) as one ray source: `num_pixels` and `rays_at(ids)` like a train
    split's, without photos.  `frames`: the indices of the frames to draw from (default: all)."""

    def __init__(self, path, frames=None):
        self.path, self.device = path, path.device
        self.frames = torch.as_tensor(list(range(len(path))) if frames is None else list(frames), dtype=torch.int64, device=self.device)
        counts = np.array([path.sizes[int(i)][0] * path.sizes[int(i)][1] for i in self.frames.tolist()], np.int64)
        self.offsets = torch.from_numpy(np.concatenate([[0], np.cumsum(counts)])).to(self.device)
        self.num_pixels = int(counts.sum())

    def rays_at(self, ids):
        ids = ids.to(self.device, torch.int64).reshape(-1)
        cam = torch.searchsorted(self.offsets, ids, right=True) - 1
        pix = ids - self.offsets[cam]
        return self.path.pixel_rays(self.frames[cam], pix), None


def mlp_batches(model, ray_source, batch, seed=0, white_bkgd=True, chunk=None):
    """The rays `photo_batches` would draw from `ray_source` (a train split or a `PathPixels`), with the target taken from the fine level of
    `model` under torch.no_grad() -> (Rays, rgb [B, 3])."""
    from .evaluate import DEFAULT_CHUNK
    from .model import GraphedFrame
    draw = photo_batches(ray_source, batch, seed)
    frame = []

    def batch_of(step):
        rays, _ = draw(step)
        with torch.no_grad():
            if not frame:
                frame.append(GraphedFrame(model, int(batch), DEFAULT_CHUNK if chunk is None else chunk, white_bkgd, rays.origins.device,
                                          capture=False))
            _, rgb, _ = frame[0](rays)
            return rays, rgb.reshape(int(batch), 3).clone()
    return batch_of


def march_pyramid(pyramid, origins, directions, radii, near, far, background, footprint=DEFAULT_FOOTPRINT, step_scale=DEFAULT_STEP_SCALE,
                  t_min=DEFAULT_T_MIN, max_steps=DEFAULT_MAX_STEPS, out=None, steps=None, lod=None, use_occupancy=True):
    """mipnerf_preview_mip_march (mipnerf_preview_sparse_march for a pyramid of `SparseField`s) on flat fp32 device tensors: origins / directions [B, 3], radii / near / far [B] -> (rgb [B, 3], acc [B],
    distance [B]) (`out`: these three, preallocated).  `steps`: an int32 [B] tensor that receives the samples evaluated per ray; `lod`: an
    fp32 [B] tensor that receives each ray's weighted mean level.  The step is `step_scale` times the spacing of level 0."""
    refuse_contracted(pyramid, "march_pyramid")
    B, dev, (rgb, acc, dist), structs, params = _march_args(
        "march_pyramid", pyramid.levels, dict(origins=origins, directions=directions, radii=radii, near=near, far=far), background, step_scale,
        t_min, max_steps, out, steps, use_occupancy)
    if lod is not None and (lod.dtype != torch.float32 or lod.numel() != B or not lod.is_contiguous() or lod.device != dev):
        raise ValueError("march_pyramid: lod must be a contiguous fp32 tensor with one entry per ray")
    if pyramid.sparse:
        return _march_sparse("preview_sparse_march", pyramid.levels, structs, params, footprint, B, dev, origins, directions, radii, near, far,
                             (rgb, acc, dist), steps, lod)
    pyr = L.PreviewPyramid()
    pyr.levels = len(structs)
    for i, field in enumerate(structs):
        pyr.level[i] = field
    with torch.cuda.device(dev):
        L.preview_mip_check(L.preview_mip_lib().mipnerf_preview_mip_march(
            C.byref(pyr), C.byref(params), float(footprint), B, origins.data_ptr(), directions.data_ptr(), radii.data_ptr(), near.data_ptr(),
            far.data_ptr(), rgb.data_ptr(), acc.data_ptr(), dist.data_ptr(), None if steps is None else steps.data_ptr(),
            None if lod is None else lod.data_ptr(), torch.cuda.current_stream().cuda_stream), "preview_mip_march")
    return rgb, acc, dist


def _march_rays(baked, rays, n, white_bkgd, footprint, step_scale, t_min, max_steps, **kw):
    """The `n` rays of `rays` (a `Rays` of [..., k] tensors) through `baked` by the entry point of its kind: `march` for a `BakedField`,
    `march_pyramid` with `rays.radii` and `footprint` for a `BakedPyramid` (`kw`: out, steps and, for a pyramid, lod)."""
    o, d, near, far = (t.reshape(n, t.shape[-1]).float().contiguous() for t in (rays.origins, rays.directions, rays.near, rays.far))
    if isinstance(baked, BakedPyramid):
        return march_pyramid(baked, o, d, rays.radii.reshape(n).float().contiguous(), near.reshape(n), far.reshape(n), white_bkgd, footprint,
                             step_scale, t_min, max_steps, **kw)
    return march(baked, o, d, near.reshape(n), far.reshape(n), white_bkgd, step_scale, t_min, max_steps, **kw)


def render_rays(baked, rays, white_bkgd, step_scale=DEFAULT_STEP_SCALE, t_min=DEFAULT_T_MIN, max_steps=DEFAULT_MAX_STEPS,
                footprint=DEFAULT_FOOTPRINT):
    """`rays` (a `Rays` of [..., k] tensors) marched through `baked`: (rgb [..., 3], distance [...], acc [...]).  A `BakedField` is
    marched with point samples by mipnerf_preview_march; a `BakedPyramid` by mipnerf_preview_mip_march with `rays.radii` and `footprint`.
    The defaults of `step_scale`, `t_min` and `footprint` are choices (see the top of this module), not measurements."""
    shape = rays.origins.shape[:-1]
    rgb, acc, dist = _march_rays(baked, rays, int(np.prod(shape)), white_bkgd, footprint, step_scale, t_min, max_steps)
    return rgb.reshape(*shape, 3), dist.reshape(shape), acc.reshape(shape)


class PreviewFrame:
    """One image size of a baked field or pyramid: static output buffers and the device buffers of the image bytes; `render` / `images`
    are shaped like `evaluate.FrameEvaluator`'s, so `evaluate.save_images` and the PNG kernels serve both.  A `BakedPyramid` is marched
    with the rays' radii and `footprint`, and the frame keeps a static `lod` buffer (each ray's weighted mean level)."""

    def __init__(self, baked, height, width, white_bkgd=True, step_scale=DEFAULT_STEP_SCALE, t_min=DEFAULT_T_MIN, max_steps=DEFAULT_MAX_STEPS,
                 footprint=DEFAULT_FOOTPRINT):
        from . import ops
        self.baked, self.h, self.w = baked, int(height), int(width)
        self.white_bkgd, self.step_scale, self.t_min, self.max_steps = white_bkgd, float(step_scale), float(t_min), int(max_steps)
        self.mip, self.footprint = isinstance(baked, BakedPyramid), float(footprint)
        n, dev = self.h * self.w, baked.device if self.mip else baked.rows.device
        self.lod = torch.zeros(n, dtype=torch.float32, device=dev) if self.mip else None
        self.out = (torch.empty(n, 3, device=dev), torch.empty(n, device=dev), torch.empty(n, device=dev))
        self.steps = torch.zeros(n, dtype=torch.int32, device=dev)
        self.vis_ws = torch.empty(ops.visualize_workspace_floats(n), dtype=torch.float32, device=dev)
        self.rgb_u8 = torch.empty(self.h, self.w, 3, dtype=torch.uint8, device=dev)
        self.dist_u8 = torch.empty(self.h, self.w, 3, dtype=torch.uint8, device=dev)
        self.acc_u8 = torch.empty(self.h, self.w, 3, dtype=torch.uint8, device=dev)

    def render(self, rays):
        """Rays [H, W, k] -> (rgb [H, W, 3], distance [H, W], acc [H, W]): views of the frame's static outputs."""
        kw = dict(lod=self.lod) if self.mip else {}
        rgb, acc, dist = _march_rays(self.baked, rays, self.h * self.w, self.white_bkgd, self.footprint, self.step_scale, self.t_min,
                                     self.max_steps, out=self.out, steps=self.steps, **kw)
        return rgb.view(self.h, self.w, 3), dist.view(self.h, self.w), acc.view(self.h, self.w)

    def images(self, rgb, dist, acc):
        from . import ops
        ops.image_to_u8(rgb, out=self.rgb_u8)
        ops.visualize_map(dist, out=self.dist_u8, workspace=self.vis_ws)
        ops.visualize_map(acc, out=self.acc_u8, workspace=self.vis_ws)
        return self.rgb_u8, self.dist_u8, self.acc_u8


# ---- the command -----------------------------------------------------------------------------------------------------------------
def build_parser():
    from .evaluate import DEFAULT_CHUNK
    from .render_video import CAMERA_ANGLE_X, _bool
    p = argparse.ArgumentParser(prog="python -m mipnerf_pl_amd.preview")
    p.add_argument("--ckpt", help="Path to ckpt.")
    p.add_argument("--out_dir", help="Output directory.", type=str, required=True)
    p.add_argument("--grid", help="lattice points per axis: one number, or NX NY NZ", type=int, nargs="+", default=[256], metavar="N")
    p.add_argument("--sh_degree", help="degree of the view-dependent colour (default 1, or the degree of --baked)", type=int, default=None)
    p.add_argument("--bound", help="the lattice spans [-B, B]^3 (default: the largest coordinate any ray of the cameras to be rendered reaches "
                   "between near and far, plus one cell)", type=float, default=None)
    p.add_argument("--threshold", help="a cell is marched when the density at one of its corners exceeds this; scene dependent", type=float,
                   default=0.01)
    p.add_argument("--dilate", help="occupied cells grow by this many cells in every direction", type=int, default=1)
    p.add_argument("--step", help="march step in units of the smallest cell edge (a choice: 0.5 keeps two samples per cell)", type=float,
                   default=DEFAULT_STEP_SCALE)
    p.add_argument("--t_min", help="stop a ray when its transmittance falls below this (a choice; 0: never)", type=float, default=DEFAULT_T_MIN)
    p.add_argument("--precision", help="MLP precision of the bake (default: the checkpoint's)", choices=["fp32", "bf16"], default=None)
    p.add_argument("--n_poses", help="poses on the spherical path", type=int, default=120)
    p.add_argument("--scale", help="pyramid levels of the spherical path", type=int, default=1)
    p.add_argument("--save_baked", help="write the baked lattice to <out_dir>/preview_spheric/<exp_name>/baked.npz", action="store_true")
    p.add_argument("--baked", help="render a lattice saved by --save_baked instead of baking one", type=str, default=None, metavar="FILE")
    p.add_argument("--data", help="--compare: path to the data whose test split is rendered both ways", default=None)
    p.add_argument("--compare", help="render the test split of --data from the lattice and with the MLP: mean PSNR of each against the photos "
                   "and of the lattice against the MLP", action="store_true")
    p.add_argument("--base_size", help="source image size: W H", type=int, nargs=2, default=[800, 800])
    p.add_argument("--camera_angle_x", help="camera_angle_x in source dataset", type=float, default=CAMERA_ANGLE_X)
    p.add_argument("--white_bkgd", help="Train set image background color.", type=_bool, default=True)
    p.add_argument("--chunk_size", help="--compare: chunk size of the MLP render", type=int, default=DEFAULT_CHUNK)
    p.add_argument("--n_dirs", help="view directions the colour is fitted to (a choice)", type=int, default=DEFAULT_N_DIRS)
    p.add_argument("--mip", help="anti-alias the preview with a pyramid of L lattices (1 .. 8), each with about half the points per axis of "
                   "the one before, the level of every sample chosen by the ray's cone radius; the bare flag means 4 levels (a choice: they "
                   "reach 8 times the finest spacing)", type=int, nargs="?", const=DEFAULT_MIP_LEVELS, default=None, metavar="L")
    p.add_argument("--sparse", help="store only the rows next to an occupied cell, behind a row table: the same pictures from a fraction of the "
                   "memory (with and without --mip)", action="store_true")
    p.add_argument("--footprint", help="--mip: the cone is footprint * radius * t wide (a choice: the default sqrt(3) is one pixel's width)",
                   type=float, default=None, metavar="F")
    p.add_argument("--tune", help="fine-tune the baked lattice through its own renderer for STEPS Adam steps before rendering: with --data "
                   "against the train split's photos (or the MLP's renders of those rays), without --data against the MLP's renders of random "
                   "pixels of the spherical path's own frames, i.e. ON THE RENDERED POSES; either way on the background of --white_bkgd, the "
                   "one the frames are rendered on.  A single dense lattice only; with --sparse the lattice is baked dense, tuned, then made sparse, so the peak memory is the dense bake's.  The float-atomic gradient sums "
                   "make two runs differ in the last bits", type=int, default=None, metavar="STEPS")
    p.add_argument("--tune_batch", help=f"--tune: rays per step (default {DEFAULT_TUNE_BATCH})", type=int, default=None, metavar="B")
    p.add_argument("--tune_lr_sigma", help=f"--tune: Adam step of the density entries (a choice, not a measurement: default "
                   f"{DEFAULT_TUNE_LR_SIGMA})", type=float, default=None)
    p.add_argument("--tune_lr_colour", help=f"--tune: Adam step of the colour coefficients (a choice, not a measurement: default "
                   f"{DEFAULT_TUNE_LR_COLOUR})", type=float, default=None)
    p.add_argument("--tune_target", help="--tune: what the lattice is tuned against (default: photos with --data, else mlp)",
                   choices=["photos", "mlp"], default=None)
    p.add_argument("--tune_seed", help="--tune: seed of the batch draws (default 0)", type=int, default=None)
    p.add_argument("--tune_tv_sigma", help="--tune: weight of the total variation of the density, per tuned point (default 0: off; a choice, "
                   "not a measurement: Adam rescales the gradient, so a weight counts only against the photometric gradient; on the one "
                   "scene of DESIGN 4.20, 1e-3 .. 1e-2 kept most of what held-out poses otherwise lose and 1e-1 cost more than it gave)", type=float, default=None, metavar="X")
    p.add_argument("--tune_tv_colour", help="--tune: weight of the total variation of the colour coefficients, per tuned point (default 0: off; "
                   "a choice, not a measurement)", type=float, default=None, metavar="X")
    p.add_argument("--tune_sh_decay", help="--tune: weight of 0.5 x the squared view-dependent coefficients (k >= 1), per tuned point (default "
                   "0: off; a choice, not a measurement)", type=float, default=None, metavar="X")
    p.add_argument("--tune_tv_eps", help=f"--tune: the eps under the total variation's root (a choice, not a measurement: default "
                   f"{DEFAULT_TUNE_TV_EPS})", type=float, default=None, metavar="X")
    p.add_argument("--space", help="'contracted': bake a llff / realdata360 checkpoint (the unbounded-scene model) into a lattice over the "
                   "contracted space and render the interpolated path through the poses of --data (required) to "
                   "<out_dir>/preview_path/<exp_name>/1/; --grid, --sh_degree, --sparse, --compare, --save_baked and --baked work as for a "
                   "bounded checkpoint, --bound is the half-width of the lattice in the contracted space (default 2, all of it)",
                   choices=["contracted"], default=None)
    p.add_argument("--far_radius", help="--space contracted: rays are cut, and the density is 0, beyond this distance from the centre (default: "
                   "the largest distance any ray of the frames to be rendered reaches, plus one cell's allowance)", type=float, default=None,
                   metavar="R")
    p.add_argument("--split", help="--space contracted: the split whose poses the path runs through (default test)", choices=["train", "test"],
                   default=None)
    p.add_argument("--n_views", help="--space contracted: three times the poses per pair of consecutive poses (default 30)", type=int, default=None)
    p.add_argument("--factor", help="--space contracted: the data set's shrink factor (default: the checkpoint's)", type=int, default=None)
    return p


TUNE_FLAGS = ("tune_batch", "tune_lr_sigma", "tune_lr_colour", "tune_target", "tune_seed", "tune_tv_sigma", "tune_tv_colour", "tune_sh_decay",
              "tune_tv_eps")


def refuse_tune_arguments(args):
    """What --tune and its flags refuse from the command line alone."""
    given = [f for f in TUNE_FLAGS if getattr(args, f) is not None]
    if args.tune is None:
        if given:
            raise SystemExit(f"--{given[0]} belongs to --tune STEPS: give --tune as well")
        return
    if args.tune < 1:
        raise SystemExit(f"--tune {args.tune}: at least one step")
    if args.mip is not None:
        raise SystemExit("--tune with --mip: a pyramid of lattices is not a tuning target (not implemented): drop one of them")
    if args.baked is not None and args.sparse:
        raise SystemExit("--tune with a sparse --baked file: sparse rows are not a tuning target (not implemented); tune the dense lattice "
                         "and give --sparse without --baked, or render the file without --tune")
    if args.tune_target == "photos" and args.data is None:
        raise SystemExit("--tune_target photos tunes against the train split of a data set: give --data")
    if args.tune_batch is not None and args.tune_batch < 1:
        raise SystemExit(f"--tune_batch {args.tune_batch}: at least one ray")
    for f in ("tune_lr_sigma", "tune_lr_colour", "tune_tv_sigma", "tune_tv_colour", "tune_sh_decay"):
        v = getattr(args, f)
        if v is not None and not (v >= 0 and np.isfinite(v)):
            raise SystemExit(f"--{f} {v}: must be finite and >= 0")
    if args.tune_tv_eps is not None and not (args.tune_tv_eps > 0 and np.isfinite(args.tune_tv_eps)):
        raise SystemExit(f"--tune_tv_eps {args.tune_tv_eps}: must be finite and > 0")


def refuse_space_arguments(args):
    """What --space and its flags refuse from the command line alone."""
    if args.space is None:
        for flag in ("far_radius", "split", "n_views", "factor"):
            if getattr(args, flag) is not None:
                raise SystemExit(f"--{flag} belongs to --space contracted: give --space as well")
        return
    args.split = "test" if args.split is None else args.split
    args.n_views = 30 if args.n_views is None else args.n_views
    if args.mip is not None:
        raise SystemExit("--space contracted with --mip: a contracted pyramid is not implemented: drop --mip")
    if args.tune is not None:
        raise SystemExit("--space contracted with --tune: this command does not tune a contracted lattice: drop --tune, tune with "
                         "`python -m mipnerf_pl_amd.preview_tune360` and render its file with --space contracted --baked")
    if args.far_radius is not None and not (args.far_radius > 1 and np.isfinite(args.far_radius)):
        raise SystemExit(f"--far_radius {args.far_radius}: must be finite and > 1")
    if args.bound is not None and args.bound > 2:
        raise SystemExit(f"--bound {args.bound}: the contracted space ends at 2")
    if args.n_views < 1:
        raise SystemExit(f"--n_views {args.n_views}: at least one")
    if args.data is None:
        raise SystemExit("--space contracted renders the interpolated path through the poses of a data set: give --data")


def refuse_baked_space(args):
    """--baked of a contracted lattice without --space contracted, or of a bounded one with it: refused after reading the file's keys."""
    if args.baked is None:
        return
    stored = BakedField.stored_space(args.baked)
    if stored != args.space:
        raise SystemExit("--baked {0} holds a lattice of {1}, {2}".format(
            args.baked, "world coordinates (a bounded scene)" if stored is None else f"the {stored} space",
            "--space contracted asks for a contracted one: drop --space" if stored is None else f"give --space {stored} to render it"))


def refuse_arguments(args):
    """Everything that can be refused from the command line alone, before any file is opened."""
    if len(args.grid) not in (1, 3):
        raise SystemExit(f"--grid {' '.join(str(g) for g in args.grid)}: give one number or NX NY NZ")
    dims = _dims3(args.grid if len(args.grid) == 3 else args.grid[0])
    if min(dims) < 2:
        raise SystemExit(f"--grid {' '.join(str(g) for g in args.grid)}: the lattice needs at least 2 points per axis")
    if 7 * dims[0] * dims[1] * dims[2] >= 2 ** 31:
        raise SystemExit(f"--grid {' '.join(str(g) for g in args.grid)}: too large: 7 nx ny nz must stay below 2^31")
    if args.sh_degree is not None and args.sh_degree not in (0, 1, 2):
        raise SystemExit(f"--sh_degree {args.sh_degree}: the degree must be 0, 1 or 2")
    if not args.step > 0:
        raise SystemExit(f"--step {args.step}: the step must be positive")
    if not 0 <= args.t_min < 1:
        raise SystemExit(f"--t_min {args.t_min}: must lie in [0, 1)")
    if args.bound is not None and not args.bound > 0:
        raise SystemExit(f"--bound {args.bound}: the half-width of the box must be positive")
    if args.compare and args.data is None:
        raise SystemExit("--compare renders the test split of a data set both ways: give --data")
    if args.baked is not None and args.save_baked:
        raise SystemExit("--save_baked writes the lattice this run bakes; --baked renders one that exists already: give one of them")
    if args.mip is not None and not 1 <= args.mip <= MAX_MIP_LEVELS:
        raise SystemExit(f"--mip {args.mip}: a pyramid has 1 .. {MAX_MIP_LEVELS} levels")
    if args.footprint is not None and args.mip is None:
        raise SystemExit("--footprint scales the cone that chooses a pyramid level: give --mip as well")
    if args.footprint is not None and not (args.footprint >= 0 and np.isfinite(args.footprint)):
        raise SystemExit(f"--footprint {args.footprint}: must be finite and >= 0")
    refuse_tune_arguments(args)
    refuse_space_arguments(args)
    if args.ckpt is None:
        raise SystemExit("give --ckpt: the checkpoint names the experiment (and is what --compare renders with the MLP)")
    return dims


def refuse_baked_degree(args):
    """--baked of another degree than --sh_degree, when both are given: refused after reading the file's degree alone."""
    if args.baked is None:
        return
    stored = BakedField.stored_degree(args.baked)
    if args.sh_degree is not None and args.sh_degree != stored:
        raise SystemExit(f"--baked {args.baked} holds a lattice of degree {stored}, --sh_degree asks for {args.sh_degree}: drop one of them")


def refuse_baked_levels(args):
    """--baked of a pyramid without --mip, or of another level count than --mip L: refused after reading the file's level count alone."""
    if args.baked is None:
        return
    stored = BakedPyramid.stored_levels(args.baked)
    if args.mip is None and stored is not None:
        raise SystemExit(f"--baked {args.baked} holds a pyramid of {stored} levels: give --mip {stored} to render it")
    if args.mip is not None and stored != args.mip:
        raise SystemExit("--baked {0} holds {1}, --mip asks for {2} levels: give --mip {3}".format(
            args.baked, "a single lattice" if stored is None else f"a pyramid of {stored} levels", args.mip,
            "nothing; drop --mip" if stored is None else stored))


def refuse_baked_kind(args):
    """--baked of a sparse file without --sparse, or of a dense one with it: refused after reading the file's key names alone."""
    if args.baked is None:
        return
    stored = BakedPyramid.stored_sparse(args.baked)
    if stored and not args.sparse:
        raise SystemExit(f"--baked {args.baked} holds sparse rows: give --sparse to render it")
    if args.sparse and not stored:
        raise SystemExit(f"--baked {args.baked} holds dense rows, --sparse asks for sparse ones: drop --sparse")


def refuse_checkpoint(system, space=None):
    """Captured-scene and unbounded checkpoints (unless `space='contracted'` names their lattice), bounded ones with it, and one-level
    models: refused before anything is moved to the device."""
    from .render_video import is_scene360
    unbounded = bool(getattr(system.mip_nerf, "unbounded", False))
    if space is None and (is_scene360(system.hparams) or unbounded):
        raise SystemExit("preview: this checkpoint holds a captured scene ({}); the baked lattice is implemented for bounded (Blender) "
                         "checkpoints only -- its rays leave any box and the unbounded-scene model lives in a contracted space.  Give "
                         "--space contracted (with --data) to bake the unbounded-scene model into a lattice over that space".format(
                             system.hparams.get("dataset_name")))
    if space is not None and not (is_scene360(system.hparams) and unbounded):
        raise SystemExit("preview: --space {0} bakes the unbounded-scene model of a llff / realdata360 checkpoint; this checkpoint ({1}) "
                         "holds a bounded model, whose lattice lies in world coordinates: drop --space".format(
                             space, system.hparams.get("dataset_name")))
    try:
        refuse_model(system, "preview", space)
    except NotImplementedError as e:
        raise SystemExit(str(e))


def _psnr(a, b):
    """PSNR of two [H, W, 3] images by the evaluation's own kernel."""
    from . import ops
    return float(ops.eval_errors(a, b)[0])


def _tune_command(args, system, baked, path, hp, dev):
    """--tune: the batch source, the steps and the `preview: tuned` line; returns the lattice to render (a `SparseField` with --sparse)."""
    from .datasets import dataset_dict
    batch = DEFAULT_TUNE_BATCH if args.tune_batch is None else args.tune_batch
    seed = 0 if args.tune_seed is None else args.tune_seed
    against = args.tune_target if args.tune_target is not None else ("photos" if args.data is not None else "mlp")
    white = bool(args.white_bkgd)         # the background the frames are rendered on: photos composited, MLP rendered and lattice tuned on it
    if args.data is not None:
        source = dataset_dict[hp["dataset_name"]](data_dir=args.data, split="train", white_bkgd=white, batch_type="all_images", device=dev)
    else:
        source = PathPixels(path)
    batches = photo_batches(source, batch, seed) if against == "photos" else \
        mlp_batches(system.mip_nerf, source, batch, seed, white, args.chunk_size)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    reg = {k: v for k, v in (("tv_sigma", args.tune_tv_sigma), ("tv_colour", args.tune_tv_colour), ("sh_decay", args.tune_sh_decay),
                             ("tv_eps", args.tune_tv_eps)) if v is not None}
    state, losses = tune_field(baked, batches, args.tune, white,
                               lr_sigma=DEFAULT_TUNE_LR_SIGMA if args.tune_lr_sigma is None else args.tune_lr_sigma,
                               lr_colour=DEFAULT_TUNE_LR_COLOUR if args.tune_lr_colour is None else args.tune_lr_colour,
                               step_scale=args.step, t_min=args.t_min, **reg)
    torch.cuda.synchronize()
    secs = time.perf_counter() - t0
    print("preview: tuned {0} steps of {1} rays against the {2} in {3:.2f} s ({4:.2f} ms per step), batch loss {5:.3e} -> {6:.3e}".format(
        args.tune, batch, "photos" if against == "photos" else "MLP", secs, 1e3 * secs / args.tune, float(losses[0]), float(losses[-1])))
    if state.regularised:
        print("preview: regularised with tv_sigma {0:g}, tv_colour {1:g}, sh_decay {2:g} (tv_eps {3:g}), each divided by the {4} tuned "
              "points".format(state.tv_sigma, state.tv_colour, state.sh_decay, state.tv_eps, state.n_points))
    return baked.to_sparse() if args.sparse else baked


def _contracted_command(args, argv, system, dims, dev):
    """--space contracted: the interpolated path of `render_video` through the poses of --data, every frame from a lattice over the
    contracted space; prints the `preview:` line and, with --compare, the PSNR line of the test split.  Returns the output folder."""
    from .datasets import PathGen, RealData360
    from .evaluate import FrameEvaluator, cull_far_radius, generate_video, save_images
    from .render_video import flag_given
    hp = system.hparams
    factor = args.factor if args.factor is not None else int(hp.get("factor", 4))
    white = bool(args.white_bkgd) if flag_given(argv, "--white_bkgd") else bool(hp["val.white_bkgd"])

    def split(name):
        return RealData360(args.data, split=name, white_bkgd=hp["val.white_bkgd"], batch_type="all_images" if name == "train" else "single_image",
                           factor=factor, device=dev)
    poses = split(args.split)
    path = PathGen(poses, args.n_views, device=dev)
    dataset = (poses if args.split == "test" else split("test")) if args.compare else None
    folder = os.path.join(args.out_dir, "preview_path", hp["exp_name"])
    os.makedirs(os.path.join(folder, "1"), exist_ok=True)
    with torch.no_grad():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if args.baked is not None:
            baked = (SparseField if args.sparse else BakedField).load(args.baked, dev)
            if args.far_radius is not None and float(np.float32(args.far_radius)) != baked.far_radius:
                raise SystemExit(f"--baked {args.baked} was baked with far radius {baked.far_radius:g}, --far_radius asks for {args.far_radius:g}: "
                                 "drop one of them")
        else:
            radius = args.far_radius
            if radius is None:
                if min(dims) < 4:
                    raise SystemExit("--grid: the default far radius needs at least 4 points per axis; give --far_radius")
                frames = [path[i] for i in range(len(path))] + ([dataset[i][0] for i in range(len(dataset))] if dataset is not None else [])
                radius = cull_far_radius(frames, min(dims))
            bound = 2.0 if args.bound is None else float(args.bound)
            baked = bake_field(system, grid=dims, degree=1 if args.sh_degree is None else args.sh_degree, lo=-bound, hi=bound,
                               threshold=args.threshold, dilate=args.dilate, n_dirs=args.n_dirs, precision=args.precision, sparse=args.sparse,
                               space=args.space, far_radius=radius)
        torch.cuda.synchronize()
        bake_ms = 1e3 * (time.perf_counter() - t0)
        if args.save_baked:
            print("preview: lattice saved to {}".format(baked.save(os.path.join(folder, "baked.npz"))))
        frames, times, samples, rays_seen = {}, [], 0, 0
        for idx in range(len(path)):
            h, w = path.sizes[idx]
            fr = frames.get((h, w))
            if fr is None:
                fr = frames[(h, w)] = PreviewFrame(baked, h, w, white, args.step, args.t_min)
            rays = path[idx]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fr.render(rays)
            torch.cuda.synchronize()
            times.append(1e3 * (time.perf_counter() - t0))
            samples, rays_seen = samples + int(fr.steps.sum()), rays_seen + h * w
            save_images(*fr.images(*out), os.path.join(folder, "1"), idx)
        generate_video(folder)
        tail = ", stored share {0:.4f}, sparse {1:.1f} MiB against {2:.1f} MiB dense".format(
            baked.stored_share(), baked.nbytes / 2 ** 20, baked.dense_nbytes / 2 ** 20) if args.sparse else ""
        print("preview: lattice {0} x {1} x {2}, degree {3}, baked share {4:.4f}, {5:.1f} MiB, {6} {7:.1f} ms, mean {8:.3f} ms per frame "
              "({9} frames), contracted, far radius {10:.4g}, mean {11:.1f} evaluated samples per ray".format(
                  *baked.dims, baked.degree, baked.baked_share(), baked.nbytes / 2 ** 20, "loaded in" if args.baked is not None else "baked in",
                  bake_ms, float(np.mean(times)), len(times), baked.far_radius, samples / max(rays_seen, 1)) + tail)
        if dataset is not None:
            both, p_baked, p_mlp, p_both = {}, [], [], []
            for idx in range(len(dataset)):
                rays, gt = dataset[idx]
                h, w = int(gt.shape[0]), int(gt.shape[1])
                if (h, w) not in both:
                    both[(h, w)] = (FrameEvaluator(system.mip_nerf, h, w, args.chunk_size, white, dev), PreviewFrame(baked, h, w, white, args.step, args.t_min))
                ev, fr = both[(h, w)]
                want, got = ev.render(rays)[0], fr.render(rays)[0]
                p_baked.append(_psnr(got, gt[..., :3]))
                p_mlp.append(_psnr(want, gt[..., :3]))
                p_both.append(_psnr(got, want))
            print("preview: mean PSNR over {0} test images: baked vs photos {1:.3f}, MLP vs photos {2:.3f}, baked vs MLP {3:.3f}".format(
                len(dataset), float(np.mean(p_baked)), float(np.mean(p_mlp)), float(np.mean(p_both))))
    return folder


def main(argv=None):
    from .evaluate import FrameEvaluator, cull_box, generate_video, save_images
    from .render_video import load_system
    args = build_parser().parse_args(argv)
    dims = refuse_arguments(args)
    refuse_baked_degree(args)
    refuse_baked_levels(args)
    refuse_baked_kind(args)
    refuse_baked_space(args)
    footprint = DEFAULT_FOOTPRINT if args.footprint is None else args.footprint
    system = load_system(args)
    refuse_checkpoint(system, args.space)
    dev = torch.device("cuda", torch.cuda.current_device())
    system = system.to(dev).eval()
    if args.space is not None:
        return _contracted_command(args, argv, system, dims, dev)
    hp = system.hparams
    exp_name = hp["exp_name"]
    from .datasets import RenderGen, dataset_dict
    focal = .5 * args.base_size[0] / np.tan(.5 * args.camera_angle_x)
    path = RenderGen(focal, args.base_size, args.scale, device=dev, n_poses=args.n_poses)
    dataset = None
    if args.compare:
        dataset = dataset_dict[hp["dataset_name"]](data_dir=args.data, split="test", white_bkgd=hp["val.white_bkgd"],
                                                  batch_type=hp["val.batch_type"], device=dev)
    folder = os.path.join(args.out_dir, "preview_spheric", exp_name)
    nums = len(path) // args.scale
    for i in range(args.scale):
        os.makedirs(os.path.join(folder, str(2 ** i)), exist_ok=True)
    with torch.no_grad():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        if args.baked is not None:
            single = SparseField if args.sparse else BakedField
            baked = single.load(args.baked, dev) if args.mip is None else BakedPyramid.load(args.baked, dev)
        else:
            bound = args.bound
            if bound is None:
                if min(dims) < 4:
                    raise SystemExit("--grid: the default box needs at least 4 points per axis; give --bound")
                frames = [path[i] for i in range(len(path))] + ([dataset[i][0] for i in range(len(dataset))] if dataset is not None else [])
                bound = cull_box(frames, min(dims))
            how = dict(grid=dims, degree=1 if args.sh_degree is None else args.sh_degree, lo=-float(bound), hi=float(bound),
                       threshold=args.threshold, dilate=args.dilate, n_dirs=args.n_dirs, precision=args.precision,
                       sparse=args.sparse and args.tune is None)           # --tune --sparse: baked dense, tuned, then made sparse
            baked = bake_field(system, **how) if args.mip is None else bake_pyramid(system, levels=args.mip, **how)
        torch.cuda.synchronize()
        bake_ms = 1e3 * (time.perf_counter() - t0)
        untuned = None
        if args.tune is not None:
            untuned = BakedField(baked.rows.clone(), baked.dims, baked.lo, baked.hi, baked.degree, baked.occupancy, baked.threshold) \
                if dataset is not None else None                            # --compare: the untuned rows beside the tuned ones
            baked = _tune_command(args, system, baked, path, hp, dev)
        if args.save_baked:
            print("preview: lattice saved to {}".format(baked.save(os.path.join(folder, "baked.npz"))))
        frames, times = {}, []
        lod_sum, lod_rays = 0.0, 0
        for idx in range(len(path)):
            h, w = path.sizes[idx]
            fr = frames.get((h, w))
            if fr is None:
                fr = frames[(h, w)] = PreviewFrame(baked, h, w, args.white_bkgd, args.step, args.t_min, footprint=footprint)
            rays = path[idx]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fr.render(rays)
            torch.cuda.synchronize()
            times.append(1e3 * (time.perf_counter() - t0))
            if fr.mip:
                hit = out[2].reshape(-1) > 0
                lod_sum, lod_rays = lod_sum + float(fr.lod[hit].sum()), lod_rays + int(hit.sum())
            save_images(*fr.images(*out), os.path.join(folder, str(int(args.base_size[0] / w))), idx % nums)
        generate_video(folder)
        # --sparse: the stored share and what the dense rows would take, after everything the line says without it
        tail = ", stored share {0:.4f}, sparse {1:.1f} MiB against {2:.1f} MiB dense".format(
            baked.stored_share(), baked.nbytes / 2 ** 20, baked.dense_nbytes / 2 ** 20) if args.sparse else ""
        if args.mip is None:
            print("preview: lattice {0} x {1} x {2}, degree {3}, baked share {4:.4f}, {5:.1f} MiB, {6} {7:.1f} ms, mean {8:.3f} ms per frame "
                  "({9} frames)".format(*baked.dims, baked.degree, baked.baked_share(), baked.nbytes / 2 ** 20,
                                        "loaded in" if args.baked is not None else "baked in", bake_ms, float(np.mean(times)), len(times)) + tail)
        else:
            print("preview: pyramid of {0} levels {1}, degree {2}, baked share {3:.4f}, {4:.1f} MiB, {5} {6:.1f} ms, mean {7:.3f} ms per frame "
                  "({8} frames), footprint {9:.4f}, mean lod {10:.3f} over {11} hit rays".format(
                      len(baked), ", ".join("{0} x {1} x {2}".format(*b.dims) for b in baked.levels), baked.degree,
                      baked.levels[0].baked_share(), baked.nbytes / 2 ** 20, "loaded in" if args.baked is not None else "baked in", bake_ms,
                      float(np.mean(times)), len(times), footprint, lod_sum / max(lod_rays, 1), lod_rays) + tail)
        if dataset is not None:
            white = bool(hp["val.white_bkgd"])
            single = baked if args.mip is None else baked.levels[0]
            mlp_frames, p_baked, p_mlp, p_both, p_mip, p_mip_both = {}, [], [], [], [], []
            untuned_frames, p_untuned, p_untuned_both = {}, [], []         # --tune: the lattice as it was baked, beside the tuned one
            for idx in range(len(dataset)):
                rays, gt = dataset[idx]
                h, w = int(gt.shape[0]), int(gt.shape[1])
                if (h, w) not in mlp_frames:
                    mlp_frames[(h, w)] = (FrameEvaluator(system.mip_nerf, h, w, args.chunk_size, white, dev),
                                          PreviewFrame(single, h, w, white, args.step, args.t_min),
                                          None if args.mip is None else PreviewFrame(baked, h, w, white, args.step, args.t_min,
                                                                                     footprint=footprint))
                ev, fr, fr_mip = mlp_frames[(h, w)]
                want = ev.render(rays)[0]
                got = fr.render(rays)[0]
                if fr_mip is not None:
                    mip = fr_mip.render(rays)[0]
                    p_mip.append(_psnr(mip, gt[..., :3]))
                    p_mip_both.append(_psnr(mip, want))
                p_baked.append(_psnr(got, gt[..., :3]))
                p_mlp.append(_psnr(want, gt[..., :3]))
                p_both.append(_psnr(got, want))
                if untuned is not None:
                    if (h, w) not in untuned_frames:
                        untuned_frames[(h, w)] = PreviewFrame(untuned, h, w, white, args.step, args.t_min)
                    before = untuned_frames[(h, w)].render(rays)[0]
                    p_untuned.append(_psnr(before, gt[..., :3]))
                    p_untuned_both.append(_psnr(before, want))
            if untuned is not None:
                print("preview: tuning moved the mean PSNR over {0} test images: vs photos {1:.3f} -> {2:.3f}, vs MLP {3:.3f} -> {4:.3f}".format(
                    len(dataset), float(np.mean(p_untuned)), float(np.mean(p_baked)), float(np.mean(p_untuned_both)), float(np.mean(p_both))))
            if args.mip is None:
                print("preview: mean PSNR over {0} test images: baked vs photos {1:.3f}, MLP vs photos {2:.3f}, baked vs MLP {3:.3f}".format(
                    len(dataset), float(np.mean(p_baked)), float(np.mean(p_mlp)), float(np.mean(p_both))))
            else:
                print("preview: mean PSNR over {0} test images: single lattice vs photos {1:.3f}, pyramid vs photos {2:.3f}, MLP vs photos "
                      "{3:.3f}, single lattice vs MLP {4:.3f}, pyramid vs MLP {5:.3f}".format(
                          len(dataset), float(np.mean(p_baked)), float(np.mean(p_mip)), float(np.mean(p_mlp)), float(np.mean(p_both)),
                          float(np.mean(p_mip_both))))
    return folder


if __name__ == "__main__":
    main()
