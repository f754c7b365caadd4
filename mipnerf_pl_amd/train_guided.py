"""Error-guided batch sampling: `TrainGuided` draws the training batches where the field is wrong.

A uniform permutation of all training pixels spends a third or more of every batch on background the field gets right after a few
hundred steps.  This sampler keeps a running squared error per image tile (tiles of `tile` x `tile` pixels are the CELLS) and draws every
pixel of a batch from the mixture

    P(cell c) = (1 - mix) * n_c / N  +  mix * n_c err_c / sum_k n_k err_k,     then a pixel uniformly inside the cell,

and multiplies the ray's `lossmult` by w_c = (n_c / N) / P(c), so the masked mean `sum m se / sum m` of the loss kernel stays a consistent
(self-normalised) estimator of the uniform mean; w <= (1 + 1e-5) / (1 - mix).  The rule in full -- integers wherever a sum crosses
cells, so two runs give the same bytes -- is the comment on `mipnerf_guided_*` in include/mipnerf_hip.h; tests/guided_fixture.py restates it
in numpy.  Everything runs on the device (`ops.guided_refresh`, `ops.guided_draw`, and `ops.guided_apply` / `ops.guided_accumulate`
inside the step), in place, so a captured training step sees a refresh at its next replay.

Every `interval` batches of an epoch, `refresh` folds the errors gathered since the last one into the map, rebuilds the cdf and draws the
pixel ids of the next `interval` batches straight into the trainer's order buffer, with their weights and cells into two rings of
`interval * batch_size` slots that the step reads at slot (b * batch_size + i) mod ring length.  The random integers come from the default
device generator, whose state the checkpoint saves: a resumed run continues bit for bit.

What is NOT guaranteed: `train/psnr` is the PSNR of a guided batch, not of uniform pixels; the distortion term stays an unweighted batch
mean; a cell never drawn keeps err = 1 (the start value), so nothing is starved: every cell keeps at least (1 - mix) of its uniform share.

The settings are `config.TRAIN_GUIDED_DEFAULTS` (`train.guided.*`): choices, not measurements of this project.
"""
from __future__ import annotations

import numpy as np
import torch

from . import config as cfg


def cell_table(sizes, tile):
    """int64 [n_images + 1, 4] of the images `sizes` = [(h, w), ...] cut into tiles of `tile` pixels: (first cell, first pixel, W, H) per
    image, cells numbered image by image and row-major inside one; the last row is (n_cells, n_pixels, 0, 0)."""
    tile = int(tile)
    if tile < 1:
        raise ValueError(f"cell_table: tile must be at least 1 pixel (got {tile})")
    rows, cell, pix = [], 0, 0
    for h, w in sizes:
        h, w = int(h), int(w)
        if h < 1 or w < 1:
            raise ValueError(f"cell_table: an image of {w} x {h} pixels")
        rows.append((cell, pix, w, h))
        cell += ((w + tile - 1) // tile) * ((h + tile - 1) // tile)
        pix += h * w
    if not rows:
        raise ValueError("cell_table: no image")
    rows.append((cell, pix, 0, 0))
    return np.asarray(rows, np.int64)


def refresh_due(batch_index, interval):
    """Whether the map is refreshed (and the next segment drawn) BEFORE batch `batch_index` of an epoch (0-based)."""
    return int(batch_index) % int(interval) == 0


def check_state(sd, tile, sizes):
    """Refuses a saved state of another tile or other image sizes."""
    theirs = [tuple(int(v) for v in s) for s in sd["sizes"]]
    mine = [tuple(int(v) for v in s) for s in sizes]
    if int(sd["tile"]) != int(tile):
        raise ValueError(f"TrainGuided: the checkpoint's error map has tile {int(sd['tile'])}, this run is configured for {int(tile)}; "
                         "resume with the train.guided.* settings of the run that wrote it")
    if theirs != mine:
        raise ValueError(f"TrainGuided: the checkpoint's error map covers {len(theirs)} images of other sizes than this run's {len(mine)} "
                         "training images; resume on the data set of the run that wrote it")


class TrainGuided:
    """The `ops.GuidedState` of one training run, its settings and the position of the segment drawn last.

    `settings`: `config.train_guided_settings(hparams)`; `sizes`: [(h, w)] of the training images in the order of the pixel ids;
    `batch_size`: rays per step."""
    COLUMNS = ("train/guided_ess", "train/guided_visited")

    def __init__(self, settings, sizes, batch_size, device):
        from . import ops
        s = self.settings = dict(settings)
        self.sizes = [(int(h), int(w)) for h, w in sizes]
        self.B = int(batch_size)
        self.dev = torch.device(device)
        self.state = ops.GuidedState(cell_table(self.sizes, s["tile"]), s["tile"], s["interval"] * self.B, self.dev)
        self.refreshes = 0
        self.segment = (0, 0)           # [lo, hi) of the order buffer filled by the last refresh

    @classmethod
    def for_system(cls, system, hparams, device):
        return cls(cfg.train_guided_settings(hparams), system.train_dataset.sizes, hparams["train.batch_size"], device)

    def refresh_due(self, batch_index):
        return refresh_due(batch_index, self.settings["interval"])

    def refresh(self, order, b, B=None, n_order=None):
        """Fold + mass + scan, then the draws of batches b .. b + interval - 1 into order[b * B : min((b + interval) * B, n_order)] and the
        rings.  On the current stream, in place; the random integers are drawn from the default device generator (an allocation: this
        stays outside a captured graph)."""
        from . import ops
        s, st = self.settings, self.state
        B = self.B if B is None else int(B)
        n_order = int(order.numel()) if n_order is None else int(n_order)
        if B != self.B:
            raise ValueError(f"TrainGuided.refresh: the rings were sized for batches of {self.B} rays (got {B})")
        lo, hi = int(b) * B, min((int(b) + s["interval"]) * B, n_order)
        if not 0 <= lo <= hi <= order.numel():
            raise ValueError(f"TrainGuided.refresh: batch {b} lies outside an order of {n_order} ids")
        with torch.no_grad():
            ops.guided_refresh(st, s["rate"], s["mix"])
            r = torch.randint(0, 1 << 32, (2, hi - lo), dtype=torch.int64, device=self.dev)
            ops.guided_draw(st, r, order[lo:hi], ring_start=lo % st.ring_len)
        self.refreshes += 1
        self.segment = (lo, hi)
        return order

    def stats(self, b, n_order):
        """(effective sample share (sum w)^2 / (n sum w^2) of batch b's weights, share of cells visited up to the last refresh): a host
        read-back of the ring and the header."""
        st = self.state
        lo, hi = int(b) * self.B, min((int(b) + 1) * self.B, int(n_order))
        if hi <= lo:
            return float("nan"), float("nan")
        slots = torch.arange(lo, hi, device=self.dev) % st.ring_len
        w = st.weight[slots].double()
        return float(w.sum() ** 2 / (w.numel() * (w * w).sum())), float(st.header[2]) / st.n_cells

    # -- checkpoints ----------------------------------------------------------------------------------------------------
    def state_dict(self, order):
        st, (lo, hi) = self.state, self.segment
        c = lambda t: t.detach().cpu().clone()      # noqa: E731
        return {"err": c(st.err), "sum": c(st.sum), "cnt": c(st.cnt), "seen": c(st.seen), "header": c(st.header), "weight": c(st.weight),
                "cell": c(st.cell), "segment": (lo, hi), "order": c(order[lo:hi]), "tile": st.tile, "sizes": list(self.sizes),
                "batch_size": self.B, "interval": self.settings["interval"], "refreshes": self.refreshes}

    def load_state_dict(self, sd, order):
        """Takes the map, the counters, both rings and the current segment of `order` (written in place)."""
        check_state(sd, self.state.tile, self.sizes)
        st = self.state
        if int(sd["batch_size"]) != self.B or int(sd["interval"]) != self.settings["interval"]:
            raise ValueError(f"TrainGuided: the checkpoint's rings were drawn for train.batch_size {int(sd['batch_size'])} and "
                             f"train.guided.interval {int(sd['interval'])}, this run has {self.B} and {self.settings['interval']}")
        for name in ("err", "sum", "cnt", "seen", "header", "weight", "cell"):
            mine, theirs = getattr(st, name), sd[name]
            if tuple(mine.shape) != tuple(theirs.shape) or mine.dtype != theirs.dtype:
                raise ValueError(f"TrainGuided: the checkpoint's `{name}` does not have the shape of this run's cell table")
            mine.copy_(theirs)
        lo, hi = (int(v) for v in sd["segment"])
        if not 0 <= lo <= hi <= order.numel() or sd["order"].numel() != hi - lo:
            raise ValueError("TrainGuided: the checkpoint's segment does not fit this run's epoch")
        order[lo:hi].copy_(sd["order"])
        self.segment, self.refreshes = (lo, hi), int(sd.get("refreshes", 0))
