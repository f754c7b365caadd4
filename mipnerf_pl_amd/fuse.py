"""A mesh without a density threshold: rendered median depth fused into a truncated signed distance volume.

`extract_mesh` cuts the surface where the density crosses a number that depends on the scene.  The renderer already knows where the
surface is -- where a ray's fine weights pass one half -- so `fuse_mesh` renders a depth map per camera (`DepthFrame`: the chunk forwards
of a frame, the depth quantile kernel behind each), integrates the maps into a volume (`ops.TSDF`; rays without a depth carve free space,
which removes fog and floaters) and cuts the volume's zero level set (`ops.isosurface`).  Nothing in it depends on which model rendered the
depth, so one path serves the bounded and the unbounded-scene model.  The rules are those of include/mipnerf_fuse.h."""
from __future__ import annotations

from typing import Optional

import torch

from . import _lib as L
from . import ops
from .mesh import Mesh, _triple, default_box, lattice_variance
from .rays import Rays

DEFAULT_TRUNC_CELLS = 3.0      # a choice, not a measurement: the truncation distance in units of the largest lattice spacing


class DepthFrame:
    """Whole-frame depth quantiles: the chunk forwards `GraphedFrame._run_chunks` launches (`MipNerf._forward_native(out=, ws=)`), eagerly
    on the current stream, each followed by `ops.depth_quantile` on the chunk's fine `weights` and `t_samples`.  `__call__(rays)` takes
    flattened [n, k] rays and returns `depth` [n, Q] (+inf where a ray's opacity stays below the quantile); `rgb`, `dist` and `acc` [n] hold
    the fine level's other outputs.  The returned tensors are the frame's own buffers: valid until the next call."""

    def __init__(self, model, num_rays: int, chunk: int, white_bkgd: bool, device, quantiles=(0.5,)):
        self.quantiles = tuple(float(q) for q in quantiles)
        if not 1 <= len(self.quantiles) <= L.FUSE_MAX_QUANTILES or not all(0.0 < q < 1.0 for q in self.quantiles):
            raise ValueError(f"DepthFrame: 1 to {L.FUSE_MAX_QUANTILES} quantiles inside (0, 1), got {quantiles!r}")
        if num_rays < 1 or chunk < 1:
            raise ValueError("DepthFrame needs at least one ray and a positive chunk")
        self.model, self.n, self.chunk, self.white_bkgd, self.dev = model, int(num_rays), int(chunk), bool(white_bkgd), torch.device(device)
        levels = model.num_levels
        self._rgb = [torch.zeros(self.n, 3, device=self.dev) for _ in range(levels)]
        self._dist = [torch.zeros(self.n, device=self.dev) for _ in range(levels)]
        self._acc = [torch.zeros(self.n, device=self.dev) for _ in range(levels)]
        self.depth = torch.zeros(self.n, len(self.quantiles), device=self.dev)
        self._scratch = {}
        self._ws = None

    @property
    def rgb(self):
        return self._rgb[-1]

    @property
    def dist(self):
        return self._dist[-1]

    @property
    def acc(self):
        return self._acc[-1]

    def chunks(self):
        return [(lo, min(self.n, lo + self.chunk)) for lo in range(0, self.n, self.chunk)]

    def __call__(self, rays: Rays):
        if rays.origins.shape[0] != self.n:
            raise ValueError(f"DepthFrame built for {self.n} rays, got {rays.origins.shape[0]}")
        m, N = self.model, self.model.num_samples
        with torch.no_grad(), torch.cuda.device(self.dev):
            ctx = m.mlp.native(self.dev)
            need = int(L.lib().mipnerf_workspace_bytes(ctx.handle, min(self.n, self.chunk)))
            if self._ws is None or self._ws.numel() < need:
                self._ws = torch.empty(need, dtype=torch.uint8, device=self.dev)
            for lo, hi in self.chunks():
                b = hi - lo
                if b not in self._scratch:      # per-sample outputs of a chunk: read by the quantile kernel behind it, then reused
                    self._scratch[b] = [(torch.empty(b, N, device=self.dev), torch.empty(b, N + 1, device=self.dev))
                                        for _ in range(m.num_levels)]
                out = [(self._rgb[l][lo:hi], self._dist[l][lo:hi], self._acc[l][lo:hi], self._scratch[b][l][0], self._scratch[b][l][1])
                       for l in range(m.num_levels)]
                m._forward_native(Rays(*[x[lo:hi] for x in rays]), False, self.white_bkgd, out=out, ws=self._ws)
                ops.depth_quantile(out[-1][3], out[-1][4], self.quantiles, out=self.depth[lo:hi])
        return self.depth


def _model_of(system_or_model):
    model = getattr(system_or_model, "mip_nerf", system_or_model)
    if not hasattr(model, "_forward_native"):
        raise TypeError(f"fuse_mesh: expected a MipNeRFSystem or MipNerf, got {type(system_or_model).__name__}")
    return model


def check_fuse_arguments(trunc_cells, quantile, unseen="inside"):
    """the refusals `fuse_mesh` and the command line share, before anything is rendered"""
    if not 0.0 < float(quantile) < 1.0:
        raise ValueError(f"fuse_mesh: quantile must lie inside (0, 1), got {quantile!r}")
    if not (float(trunc_cells) > 0.0 and float(trunc_cells) < float("inf")):
        raise ValueError(f"fuse_mesh: trunc_cells must be finite and > 0, got {trunc_cells!r}")
    if unseen not in ("inside", "outside"):
        raise ValueError(f"fuse_mesh: unseen must be 'inside' or 'outside', got {unseen!r}")


def fuse_volume(system_or_model, cameras, grid=256, lo=None, hi=None, trunc_cells=DEFAULT_TRUNC_CELLS, quantile=0.5, carve=True, precision=None,
                chunk: Optional[int] = None, on_frame=None):
    """Render the depth quantile of every camera of `cameras` ([F, 32] `ops.camera_record` rows, modes 0 and 1) and integrate the maps, in
    order, into an `ops.TSDF` over the lattice: returns (tsdf, stats).  trunc = trunc_cells * max(h).  `on_frame(f, depth [H, W], frame)`
    is called after each render.  stats: `views`, `pixels`, `pixels_without_depth`."""
    from .evaluate import DEFAULT_CHUNK
    check_fuse_arguments(trunc_cells, quantile)
    model = _model_of(system_or_model)
    box = default_box(None)
    dims, lo, hi = _triple(grid, int), _triple(box[0] if lo is None else lo, float), _triple(box[1] if hi is None else hi, float)
    dev = next(model.parameters()).device
    cams = torch.as_tensor(cameras).detach().reshape(-1, 32).to(torch.float32)
    frames = ops.fuse_projection(cams)                     # refuses distorted cameras before anything is rendered
    h = [(hi[a] - lo[a]) / (dims[a] - 1) for a in range(3)]
    tsdf = ops.TSDF(dims, lo, hi, float(trunc_cells) * max(h), device=dev)
    cams_dev = cams.to(dev)
    before = model.precision
    if precision is not None:
        model.set_precision(precision)
    stats = dict(views=int(cams.shape[0]), pixels=0, pixels_without_depth=0)
    renderers, pending, missing = {}, [], torch.zeros((), dtype=torch.int64, device=dev)
    try:
        for f in range(cams.shape[0]):
            w_, h_ = int(cams[f, 21]), int(cams[f, 22])
            n = w_ * h_
            if n not in renderers:
                renderers[n] = DepthFrame(model, n, min(n, int(chunk or DEFAULT_CHUNK)), False, dev, (quantile,))
            rays = ops.generate_rays(cams_dev, cam_idx=torch.full((n,), f, dtype=torch.int32, device=dev),
                                     pix_idx=torch.arange(n, dtype=torch.int32, device=dev))
            depth = renderers[n](rays)[:, 0].clone()
            missing += torch.isinf(depth).sum()
            stats["pixels"] += n
            if on_frame is not None:
                on_frame(f, depth.reshape(h_, w_), renderers[n])
            pending.append((f, depth))
            if len(pending) == L.FUSE_FRAMES_PER_LAUNCH or f == cams.shape[0] - 1:      # one launch's frames at a time
                tsdf.integrate(frames[[k for k, _ in pending]], torch.cat([d for _, d in pending]), carve=carve)
                pending = []
    finally:
        model.precision = model.mlp.precision = before
    stats["pixels_without_depth"] = int(missing.item())
    return tsdf, stats


def mesh_of_volume(system_or_model, tsdf, unseen="inside", color=True, precision=None):
    """The zero level set of an `ops.TSDF` as a `mesh.Mesh` (its `sigma` holds the finalised lattice), coloured as `extract_mesh` colours:
    the field at each vertex as a Gaussian of the lattice's variance, seen along minus the normal (`space='world'` for an unbounded model)."""
    model = _model_of(system_or_model)
    with torch.no_grad():
        lattice = tsdf.lattice(unseen)
        vertices, normals, faces = ops.isosurface(lattice, 0.0, tsdf.lo, tsdf.hi)
        rgb = colors = None
        if color:
            space = "world" if bool(getattr(model, "unbounded", False)) else None
            var = torch.from_numpy(lattice_variance(tsdf.dims, tsdf.lo, tsdf.hi, 1.0)).to(vertices.device)
            rgb = ops.field_at(system_or_model, vertices, var.expand(vertices.shape[0], 3), -normals, precision=precision,
                               space=space)[:, :3].contiguous()
            colors = ops.image_to_u8(rgb) if rgb.numel() else torch.empty(0, 3, dtype=torch.uint8, device=rgb.device)
    return Mesh(vertices, normals, faces, colors, lattice, rgb)


def fuse_mesh(system_or_model, cameras, grid=256, lo=None, hi=None, trunc_cells=DEFAULT_TRUNC_CELLS, quantile=0.5, unseen="inside", carve=True,
              color=True, precision=None):
    """Depth maps of `cameras` -> truncated signed distance volume -> its zero level set -> vertex colours: a `mesh.Mesh` that needs no
    density threshold.  `grid`: points per axis, or (nx, ny, nz); lo / hi: the world box (default [-1.5, 1.5]^3, for the unbounded-scene
    model too: the volume lies in world space).  `quantile`: the opacity whose depth is the surface (0.5: the median depth).
    `trunc_cells`: the truncation distance in units of the largest lattice spacing (3 is a choice, not a measurement).  `unseen`: what a
    lattice point no camera updated is -- 'inside' (space carving, the default) or 'outside', which wraps the object in a second, inner
    shell wherever it is thicker than the truncation.  `carve=False`: rays without a depth do not free the space they cross."""
    check_fuse_arguments(trunc_cells, quantile, unseen)
    tsdf, _ = fuse_volume(system_or_model, cameras, grid, lo, hi, trunc_cells, quantile, carve, precision)
    return mesh_of_volume(system_or_model, tsdf, unseen, color, precision)
