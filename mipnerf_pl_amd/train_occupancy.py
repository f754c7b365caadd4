"""The occupancy grid of a field that is still training: `TrainOccupancy`.

Rendering builds its grid once, from a trained field (`evaluate.scene_occupancy`).  Training needs one that follows the field: every
`interval` steps the density lattice of the CURRENT field is taken (`ops.density_grid`, at the run's precision) and folded into a
running lattice, running = max(decay * running, fresh) per point, whose bits (`> threshold`, dilated) are what `ops.ray_span` tightens
the training rays with (`ops.occupancy_refresh`: one elementwise kernel and the bit passes of `ops.occupancy_grid`, in place, so a
captured training step reads the new grid at its next replay).  The untrained field's density softplus(raw - 1) lies above the default
threshold, so the grid starts full and empties as the field does: there is no warm-up setting.

What span training guarantees: what a live ray no longer samples lies only in cells whose 8 corners were at or below the threshold,
after decay-max and dilation, at the last refresh; a region that drifts above the threshold is sampled again from the next refresh on.
A dead ray keeps [near, far] and is still trained, so empty space stays supervised.

The settings are `config.TRAIN_OCCUPANCY_DEFAULTS` (`train.occupancy.*`); `decay` and `interval` are instant-ngp's choices, not
measurements of this project, and `threshold` is the rendering default (a foggy field needs a higher one).
"""
from __future__ import annotations

import torch

from . import config as cfg
from . import ops

BOUND_CONTRACTED = 2.0      # the grid of the unbounded-scene model spans all of the contracted space


def refresh_due(step, interval):
    """Whether the grid is refreshed BEFORE step `step` (0-based): every `interval` steps, the first time before step 0."""
    return int(step) % int(interval) == 0


def check_spaces(model, occupancy, who):
    """A bounded model needs a world grid and the unbounded-scene model a contracted one (`model.CulledFrame`'s rule and messages)."""
    unbounded, contracted = bool(getattr(model, "unbounded", False)), getattr(occupancy, "space", None) == "contracted"
    if unbounded and not contracted:
        raise NotImplementedError(f"{who}: unbounded=True models are not supported (their field lives in a contracted space) unless "
                                  "the occupancy grid lies there too: ops.field_occupancy(..., space='contracted')")
    if contracted and not unbounded:
        raise ValueError(f"{who}: the occupancy grid lies in the contracted space of unbounded=True models; this model is bounded")


class TrainOccupancy:
    """The box, the `ops.Occupancy` (bits in place), the fp32 running lattice (zeros at start) and the scratch words of one training run.

    `settings`: `config.train_occupancy_settings(hparams)`.  `space` None -- the bounded model, a world box [-bound, bound]^3 -- or
    'contracted' -- the unbounded-scene model, [-2, 2]^3 of the contracted space with the density 0 beyond |z| = 2 - 1 / far_radius."""

    def __init__(self, settings, bound, device, space=None, far_radius=None, precision=None):
        s = self.settings = dict(settings)
        if space not in (None, "contracted"):
            raise ValueError(f"TrainOccupancy: space must be None or 'contracted', got {space!r}")
        if space == "contracted" and not (far_radius is not None and 1.0 < float(far_radius) < float("inf")):
            raise ValueError(f"TrainOccupancy: a contracted grid needs a finite far_radius > 1 (got {far_radius})")
        g = int(s["grid"])
        self.dims, self.bound, self.space = (g, g, g), float(bound), space
        self.far_radius = None if space is None else float(far_radius)
        self.precision, self.dev = precision, torch.device(device)
        self.running = torch.zeros(g, g, g, dtype=torch.float32, device=self.dev)
        words = (g - 1, g - 1, (g - 1 + 31) // 32)
        bits = torch.zeros(words, dtype=torch.uint32, device=self.dev)
        self.scratch = torch.zeros(words, dtype=torch.uint32, device=self.dev) if int(s["dilate"]) > 0 else None
        self.occupancy = ops.Occupancy(bits, self.dims, (-self.bound,) * 3, (self.bound,) * 3, space=space)
        self.occupancy.threshold, self.occupancy.dilate = float(s["threshold"]), int(s["dilate"])
        self.refreshes = 0

    @classmethod
    def for_system(cls, system, hparams, device, precision=None):
        """The grid of a training run: the box from the training split's frames (`evaluate.cull_box`, or `train.occupancy.bound`) for the
        bounded model; the contracted space with `evaluate.cull_far_radius` of them (or `train.occupancy.far_radius`) for the
        unbounded-scene model.  Frames of distorted cameras are bounded over every pixel, as `evaluate.scene_occupancy` does."""
        from . import evaluate
        s = cfg.train_occupancy_settings(hparams)
        ds, unbounded = system.train_dataset, bool(getattr(system.mip_nerf, "unbounded", False))

        def frames():
            return (ds.image_rays(i)[0] for i in range(ds.n_examples))
        if unbounded:
            far = s["far_radius"]
            if far is None:
                far = evaluate.cull_far_radius(frames(), s["grid"], evaluate.distorted_frames(ds))
            return cls(s, BOUND_CONTRACTED if s["bound"] is None else s["bound"], device, "contracted", far, precision)
        bound = s["bound"]
        if bound is None:
            bound = evaluate.cull_box(frames(), s["grid"], evaluate.distorted_frames(ds))
        return cls(s, bound, device, None, None, precision)

    @property
    def span_samples(self):
        return self.settings["span_samples"]

    def refresh_due(self, step):
        return refresh_due(step, self.settings["interval"])

    def refresh(self, model):
        """`ops.density_grid` of the current field on the grid's lattice, in its space and at the run's precision, then
        `ops.occupancy_refresh`.  On the current stream; allocates the fresh lattice, so it stays outside a captured graph."""
        with torch.no_grad():
            kw = {} if self.space is None else dict(space=self.space, far_radius=self.far_radius)
            fresh = ops.density_grid(model, self.dims, -self.bound, self.bound, precision=self.precision, **kw)
            ops.occupancy_refresh(self.occupancy, fresh, self.running, self.settings["decay"], scratch=self.scratch)
        self.refreshes += 1
        return self.occupancy

    def rebuild_bits(self):
        """The bits of `running` as it is, into the grid's own words (mipnerf_occupancy_build)."""
        from . import _lib as L
        occ = self.occupancy
        _, cdims, _, _ = ops._lattice_args("occupancy_build", occ.dims, occ.lo, occ.hi)
        with torch.cuda.device(self.dev):
            L.check(L.lib().mipnerf_occupancy_build(cdims, self.running.data_ptr(), occ.threshold, occ.dilate, occ.bits.data_ptr(),
                                                    ops._ptr(self.scratch), ops._stream()), "occupancy_build")

    def checksum(self):
        """int64 device scalar: the sum of the grid's words (what the ranks of a run compare)."""
        return self.occupancy.bits.view(torch.int32).to(torch.int64).sum()

    # -- checkpoints ----------------------------------------------------------------------------------------------------
    def state_dict(self):
        s = self.settings
        return {"running": self.running.detach().cpu().clone(), "dims": tuple(self.dims), "bound": self.bound, "space": self.space,
                "far_radius": self.far_radius, "threshold": s["threshold"], "dilate": s["dilate"], "decay": s["decay"],
                "interval": s["interval"], "refreshes": self.refreshes}

    def check_state(self, sd):
        """Refuses a state whose dims, box or space are not this run's."""
        for name, mine, theirs in (("dims", tuple(self.dims), tuple(int(d) for d in sd["dims"])), ("box half-width", self.bound, float(sd["bound"])),
                                   ("space", self.space, sd["space"]), ("far radius", self.far_radius, sd["far_radius"])):
            if mine != theirs:
                raise ValueError(f"TrainOccupancy: the checkpoint's occupancy grid has {name} {theirs!r}, this run is configured for {mine!r}; "
                                 "resume with the train.occupancy.* settings of the run that wrote it")

    def load_state_dict(self, sd):
        """Takes `running` (and rebuilds the bits from it with THIS run's threshold and dilation)."""
        self.check_state(sd)
        running = sd["running"]
        if tuple(running.shape) != tuple(self.running.shape) or running.dtype != torch.float32:
            raise ValueError("TrainOccupancy: the checkpoint's running lattice does not have the shape of its dims")
        self.running.copy_(running)
        self.refreshes = int(sd.get("refreshes", 0))
        self.rebuild_bits()
