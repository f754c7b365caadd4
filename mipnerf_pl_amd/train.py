"""The reference's train.py without Lightning: `python -m mipnerf_pl_amd.train`.

    python -m mipnerf_pl_amd.train --data_path DATA --out_dir OUT --dataset_name blender|multi_blender|llff|realdata360 [--factor 4]
        [--config FILE] [--precision bf16|fp32] [--no-graph] [--log_every_n_steps 50] [KEY VALUE ...]

What `Trainer(max_steps, val_check_interval, num_sanity_val_steps=1, limit_val_batches=val.sample_num)` + `ModelCheckpoint(save_last=True,
monitor='val/psnr', mode='max', save_top_k=2)` of Lightning 1.5 do for `MipNeRFSystem` (train.py:31-64), restated as a plain loop:

* bf16 (default): FlatAdam + DeviceMipLRDecay, and every full batch is ONE replay of `train_graph.GraphedTrainStep`, whose batch source is
  `ops.gather_train_batch`: the rays and gt of batch b come straight out of the epoch's order on the device, with b = (device step
  counter) - (device epoch base), so the host does nothing per step but replay.  The epoch's short last batch (DataLoader drop_last=False)
  is one eager native step with the same optimiser.
* fp32, or --no-graph: training_step -> backward -> optimiser step -> MipLRDecay, batch by batch.
* the epoch order is RayLoader's (seed + epoch, DistributedSampler padding and strided sharding); validation every `val.check_interval`
  batches of an epoch and after the last step, `val.sample_num` images each, one sanity image before the first step.
* out_dir/logs/<exp_name>/version_<k>/: metrics.csv (Lightning's CSVLogger columns), hparams.yaml, val images as PNGs;
  out_dir/ckpt/<exp_name>/: last.ckpt and the best two `epoch={e}-step={s}.ckpt` by val/psnr, with Lightning 1.5's checkpoint keys plus
  `mipnerf_trainer` (position in the epoch, RNG states, top-k record) for an exact resume (`checkpoint.resume_path`).
* `train.occupancy.enabled True` (off by default; `config.TRAIN_OCCUPANCY_DEFAULTS`): span training.  A `train_occupancy.TrainOccupancy`
  grid is refreshed from the current field before every step s with s % `train.occupancy.interval` == 0 (outside the graph, same
  stream), and every step -- the captured one through `GraphedTrainStep(occupancy=...)`, the eager ones through `Trainer._tighten` --
  samples each ray on its occupied span [near', far'] of `ops.ray_span` instead of [near, far]; a ray that touches nothing keeps
  [near, far].  metrics.csv gains `train/live_share` and `train/span_share`, the checkpoint's `mipnerf_trainer` entry gains `occupancy`
  (the running lattice and its settings) and a resumed run continues exactly.  Validation frames stay un-culled.
* `train.guided.enabled True` (off by default; `config.TRAIN_GUIDED_DEFAULTS`): error-guided batches.  The epoch's permutation is not
  drawn; before every batch b of an epoch with b % `train.guided.interval` == 0 a `train_guided.TrainGuided` folds the errors of the last
  batches into its per-tile map and draws the pixel ids of the next `interval` batches into the order buffer (outside the graph, same
  stream); every step -- the captured one through `GraphedTrainStep(guided=...)`, the eager ones through `ops.guided_apply` /
  `ops.guided_accumulate` with the host's batch index -- multiplies `lossmult` by the draws' importance weights and records the fine
  level's squared errors.  metrics.csv gains `train/guided_ess` and `train/guided_visited`, the checkpoint's `mipnerf_trainer` entry gains
  `guided` and a resumed run continues exactly.  Refused: `num_gpus` > 1 and `loss.disable_multiscale_loss True`.
* num_gpus > 1: the command starts one child process per rank (nccl when every rank has its own device, gloo otherwise); rank 0 alone
  logs and writes checkpoints.

`--dataset_name multi_blender` takes either a directory written by `python -m mipnerf_pl_amd.convert_blender_data` or a Blender scene
directory itself (`--data_path nerf_synthetic/lego`: no metadata.json, but transforms_{split}.json): then the four scales of every frame
are made on the device at start-up (`datasets.Multicam.from_blender`), no conversion step and no PNG is written; `eval` reads such a
checkpoint the same way.

`--dataset_name llff` (= `realdata360`) trains the unbounded-scene model on an LLFF / mip-NeRF-360 capture (`poses_bounds.npy`,
`sparse/0/cameras.bin`, `images_<factor>/` or, without it, `images/` shrunk by `--factor` on the device at start-up): `config.SCENE360_PRESET`
(nerf.unbounded, no white background, exp_name scene360) is layered under `--config` and the trailing pairs; `--factor` is stored as hparam `factor`.

`step` in metrics.csv and in checkpoint names is Lightning 1.5's `global_step` at that moment: the 0-based index of the last step taken.
"""
from __future__ import annotations

import argparse
import csv
import math
import os
import random
import subprocess
import sys
import time

import numpy as np
import torch

from . import config as cfg

PL_VERSION = "1.5.2"          # the reference's requirements.txt; the checkpoint format is that version's
TRAINER_KEY = "mipnerf_trainer"


# ---------------------------------------------------------------------------------------------------------------------
# the epoch schedule (pure functions)
# ---------------------------------------------------------------------------------------------------------------------
def local_count(n, world=1):
    """Pixels per rank of an epoch of n pixels: DistributedSampler pads to a multiple of the world size."""
    return (int(n) + int(world) - 1) // int(world)


def steps_per_epoch(n, batch_size, world=1):
    """Batches per epoch on every rank (DataLoader drop_last=False: the short last batch counts)."""
    return (local_count(n, world) + int(batch_size) - 1) // int(batch_size)


def last_batch_size(n, batch_size, world=1):
    """Rays in the epoch's last batch."""
    r = local_count(n, world) % int(batch_size)
    return r if r else int(batch_size)


def shard_order(order, rank=0, world=1):
    """DistributedSampler(drop_last=False) of one permutation: pad by wrapping around (repeating it when the pad exceeds it), then
    every world-th id from `rank`.  What datasets.RayLoader does."""
    n = int(order.numel())
    pad = local_count(n, world) * world - n
    if pad:
        order = order.repeat(pad // max(n, 1) + 2)[:n + pad]
    return order[rank::world]


def epoch_order(n, seed, epoch, rank=0, world=1, device=None, shuffle=True):
    """The rank's pixel ids of epoch `epoch`: RayLoader's permutation (a generator on the dataset's device seeded with seed + epoch),
    sharded as by shard_order."""
    if shuffle:
        g = torch.Generator(device=device)
        g.manual_seed(int(seed) + int(epoch))
        order = torch.randperm(int(n), device=device, generator=g)
    else:
        order = torch.arange(int(n), device=device)
    return shard_order(order, rank, world)


def should_validate(batch_idx, check_interval, global_step, max_steps):
    """After batch `batch_idx` of an epoch (0-based) with `global_step` steps taken: every `check_interval` batches, and once after
    the last step."""
    return (int(batch_idx) + 1) % int(check_interval) == 0 or int(global_step) >= int(max_steps)


class TopK:
    """ModelCheckpoint(monitor, mode='max', save_top_k=k) bookkeeping: which `epoch={e}-step={s}.ckpt` to write and which to delete.
    A NaN score counts as -inf, as in Lightning."""

    def __init__(self, k=2):
        self.k = int(k)
        self.best = {}                 # file name -> score

    @staticmethod
    def name(epoch, step):
        return f"epoch={int(epoch)}-step={int(step)}.ckpt"

    def update(self, score, epoch, step):
        """(name to write or None, [names to delete]) for a new score."""
        score = float(score)
        if math.isnan(score):
            score = -math.inf
        if self.k <= 0:
            return None, []
        name = self.name(epoch, step)
        if len(self.best) >= self.k:
            worst = min(self.best, key=self.best.get)
            if not score > self.best[worst]:
                return None, []
            del self.best[worst]
            self.best[name] = score
            return name, [] if worst == name else [worst]
        self.best[name] = score
        return name, []

    def state_dict(self):
        return {"k": self.k, "best": dict(self.best)}

    def load_state_dict(self, sd):
        self.k, self.best = int(sd["k"]), {str(k): float(v) for k, v in sd["best"].items()}


# ---------------------------------------------------------------------------------------------------------------------
# checkpoints
# ---------------------------------------------------------------------------------------------------------------------
def setup_seed(seed):
    """train.py:setup_seed."""
    torch.manual_seed(seed)
    torch.cuda.manual_seed_all(seed)
    np.random.seed(seed)
    random.seed(seed)
    torch.backends.cudnn.deterministic = True


def _cpu(x):
    if torch.is_tensor(x):
        return x.detach().cpu().clone()
    if isinstance(x, dict):
        return {k: _cpu(v) for k, v in x.items()}
    if isinstance(x, (list, tuple)):
        return type(x)(_cpu(v) for v in x)
    return x


def flat_adam_state_from_torch_adam(sd, system, optimizer):
    """`torch.optim.Adam(mip_nerf.parameters())` state (what the reference writes under Lightning) -> the state dict of FlatAdam:
    each parameter's moments land at that parameter's offset in the flat buffer, found by parameter identity."""
    params = list(system.mip_nerf.parameters())
    ids = sd["param_groups"][0]["params"]
    if len(ids) != len(params):
        raise ValueError(f"optimizer state covers {len(ids)} parameters, the model has {len(params)}")
    offset, off = {}, 0
    for p in optimizer.mlp.ordered_params():
        offset[id(p)] = off
        off += p.numel()
    exp_avg, exp_avg_sq, step = torch.zeros(off), torch.zeros(off), 0
    for idx, p in zip(ids, params):
        st = sd["state"].get(idx)
        if not st:
            continue
        if id(p) not in offset:
            raise ValueError("optimizer state names a parameter outside the MLP")
        o, n = offset[id(p)], p.numel()
        exp_avg[o:o + n] = st["exp_avg"].reshape(-1).float().cpu()
        exp_avg_sq[o:o + n] = st["exp_avg_sq"].reshape(-1).float().cpu()
        step = max(step, int(st["step"]))
    group = {k: v for k, v in sd["param_groups"][0].items() if k in ("lr", "betas", "eps", "initial_lr")}
    own = optimizer.param_groups[0]
    group = dict({k: v for k, v in own.items() if k != "params"}, **group, params=list(range(len(own["params"]))))
    return {"state": {0: {"step": torch.tensor(step, dtype=torch.int64), "exp_avg": exp_avg, "exp_avg_sq": exp_avg_sq}},
            "param_groups": [group]}


def _is_flat_adam_state(sd, optimizer):
    st = sd.get("state", {})
    flat_n = optimizer.mlp._flat_param.numel()
    return len(st) == 1 and next(iter(st.values()))["exp_avg"].numel() == flat_n


# ---------------------------------------------------------------------------------------------------------------------
# logging
# ---------------------------------------------------------------------------------------------------------------------
class CSVLog:
    """Lightning's CSVLogger layout: <save_dir>/<name>/version_<k>/{metrics.csv, hparams.yaml}; images go to .../images/."""
    COLUMNS = ("step", "lr", "train/loss", "train/psnr", "val/loss", "val/psnr")

    def __init__(self, save_dir, name, hparams, extra_columns=()):
        self.COLUMNS = tuple(self.COLUMNS) + tuple(extra_columns)
        root = os.path.join(save_dir, name)
        os.makedirs(root, exist_ok=True)
        versions = [int(d.split("_")[1]) for d in os.listdir(root) if d.startswith("version_") and d.split("_")[1].isdigit()]
        self.dir = os.path.join(root, f"version_{max(versions) + 1 if versions else 0}")
        self.image_dir = os.path.join(self.dir, "images")
        os.makedirs(self.image_dir, exist_ok=True)
        import yaml
        with open(os.path.join(self.dir, "hparams.yaml"), "w") as f:
            yaml.safe_dump({k: list(v) if isinstance(v, tuple) else v for k, v in hparams.items()}, f)
        self.path = os.path.join(self.dir, "metrics.csv")
        with open(self.path, "w", newline="") as f:
            csv.writer(f).writerow(self.COLUMNS)
        try:
            from torch.utils.tensorboard import SummaryWriter
            self.tb = SummaryWriter(self.dir)
        except Exception:  # noqa: BLE001 - tensorboard is optional
            self.tb = None

    def log(self, step, metrics):
        with open(self.path, "a", newline="") as f:
            csv.writer(f).writerow([step] + ["" if metrics.get(c) is None else repr(float(metrics[c])) for c in self.COLUMNS[1:]])
        if self.tb is not None:
            for k, v in metrics.items():
                self.tb.add_scalar(k, float(v), step)

    def image(self, tag, step, idx, u8):
        from PIL import Image
        arr = u8.cpu().numpy()
        Image.fromarray(arr).save(os.path.join(self.image_dir, f"{tag.replace('/', '_')}_step{int(step):07d}_{idx}.png"))
        if self.tb is not None:
            self.tb.add_image(f"{tag}/{idx}", arr, step, dataformats="HWC")

    def close(self):
        if self.tb is not None:
            self.tb.close()


def read_metrics(path):
    """metrics.csv -> list of dicts of floats (empty cells dropped)."""
    with open(path) as f:
        return [{k: float(v) for k, v in row.items() if v != ""} for row in csv.DictReader(f)]


# ---------------------------------------------------------------------------------------------------------------------
# the loop
# ---------------------------------------------------------------------------------------------------------------------
class Trainer:
    SPAN_COLUMNS = ("train/live_share", "train/span_share")     # logged only with train.occupancy.enabled

    def __init__(self, hparams, precision="bf16", use_graph=True, log_every_n_steps=50, rank=0, world=1, device=None, verbose=True):
        from .system import MipNeRFSystem
        self.hp = hp = dict(hparams)
        guided = cfg.check_train_guided(hp)["enabled"]        # refusals by key, before anything touches the device
        if guided and int(world) > 1:
            raise NotImplementedError("train.guided.enabled needs num_gpus 1: the error map is kept per run and is not shared between ranks")
        self.rank, self.world = int(rank), int(world)
        self.verbose = verbose and self.rank == 0
        self.dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.precision = precision
        self.graph_route = precision == "bf16" and bool(use_graph)
        self.log_every = max(1, int(log_every_n_steps))
        hp["precision"] = precision
        setup_seed(int(hp["seed"]))
        self.system = system = MipNeRFSystem(hp, precision=precision).to(self.dev)
        system.setup()
        system.enable_hip_graph(bool(use_graph))
        system.fused_adam = True
        system.device_lr_schedule = self.graph_route
        self.global_step, self.epoch, self.batch = 0, 0, 0
        self.topk = TopK(2)
        self._resume_ckpt = None
        self.occ, self._span = None, None
        self.guided, self._guided_sd = None, None
        if cfg.train_occupancy_settings(hp)["enabled"]:
            from .train_occupancy import TrainOccupancy, check_spaces
            self.occ = TrainOccupancy.for_system(system, hp, self.dev)
            check_spaces(system.mip_nerf, self.occ.occupancy, "train.occupancy")
        if hp.get("checkpoint.resume_path"):
            self._resume_ckpt = torch.load(hp["checkpoint.resume_path"], map_location="cpu", weights_only=False)
            system.load_state_dict(self._resume_ckpt["state_dict"], strict=True)
        opts, scheds = system.configure_optimizers()
        self.opt, self.sched = opts[0], scheds[0]["scheduler"]
        self.opt.grad_scale = 1.0 / self.world
        if self._resume_ckpt is not None:
            self._load_position(self._resume_ckpt)
        self.B = int(hp["train.batch_size"])
        ds = system.train_dataset
        self.n_local = local_count(len(ds), self.world)
        self.spe = steps_per_epoch(len(ds), self.B, self.world)
        self.last_bs = last_batch_size(len(ds), self.B, self.world)
        self.order = torch.zeros(self.n_local, dtype=torch.int64, device=self.dev)
        if guided:
            from .train_guided import TrainGuided
            self.guided = TrainGuided.for_system(system, hp, self.dev)
            if self._guided_sd is not None:
                self.guided.load_state_dict(self._guided_sd, self.order)
            # the eager routes record the fine level's colours: the one-call native step copies them out, the autograd route's forward hands them over
            system.mip_nerf.keep_fine_rgb = True
            system.mip_nerf.register_forward_hook(lambda m, args, ret: setattr(m, "last_fine_rgb", ret[-1][0].detach()))
        self.gstep = None
        if self.graph_route:
            self._make_graph_step()
        self.ckpt_dir = os.path.join(hp["out_dir"], "ckpt", hp["exp_name"])
        self.logger = None
        if self.rank == 0:
            os.makedirs(self.ckpt_dir, exist_ok=True)
            self.logger = CSVLog(os.path.join(hp["out_dir"], "logs"), hp["exp_name"], hp,
                                 extra_columns=(self.SPAN_COLUMNS if self.occ is not None else ())
                                 + (self.guided.COLUMNS if self.guided is not None else ()))

    # -- set-up ------------------------------------------------------------------------------------------------------
    def _make_graph_step(self):
        from . import ops
        from .train_graph import GraphedTrainStep
        opt, ds = self.opt, self.system.train_dataset
        if opt._dev_step is None:       # the batch source reads the device step counter from the first (warm-up) step on
            opt._dev_step = torch.full((1,), opt.steps, dtype=torch.int64, device=self.dev)
            opt._hyper = torch.zeros(4, dtype=torch.float32, device=self.dev)
        self.epoch_base = torch.zeros(1, dtype=torch.int64, device=self.dev)
        d = ds._need_device()

        def batch_source():
            ops.gather_train_batch(self.order, d["offsets"], d["cameras"], d["pixels"], opt._dev_step, self.epoch_base,
                                   step.rays, step.gt)
        occ = {} if self.occ is None else dict(occupancy=self.occ.occupancy, span_samples=self.occ.span_samples)
        if self.guided is not None:
            occ.update(guided=self.guided.state, guided_index=(opt._dev_step, self.epoch_base, self.n_local))
        step = GraphedTrainStep(self.system, opt, self.B, self.dev, use_graph=True, batch_source=batch_source, **occ)
        self.gstep = step

    def _capture(self):
        """Capture the step with the device RNG state unchanged: the capture's eager warm-up draws from the generator, and a resumed
        run captures at a different step than a straight one."""
        state = torch.cuda.get_rng_state(self.dev)
        self.gstep._capture()
        torch.cuda.set_rng_state(state, self.dev)

    def _load_position(self, ck):
        opt = self.opt
        sd = ck["optimizer_states"][0]
        opt.load_state_dict(sd if _is_flat_adam_state(sd, opt) else flat_adam_state_from_torch_adam(sd, self.system, opt))
        own = ck.get(TRAINER_KEY)
        if own is not None:
            self.global_step, self.epoch, self.batch = int(own["global_step"]), int(own["epoch"]), int(own["batch"])
            self.topk.load_state_dict(own["topk"])
            if self.occ is not None and own.get("occupancy") is not None:
                self.occ.load_state_dict(own["occupancy"])
            self._guided_sd = own.get("guided")         # loaded once the order buffer exists
            rng = own["rng"]
            torch.set_rng_state(rng["torch"])
            torch.cuda.set_rng_state(rng["cuda"], self.dev)
            np.random.set_state(rng["numpy"])
            random.setstate(rng["python"])
        else:           # a checkpoint of Lightning: its step count, the epoch it was in
            self.global_step, self.epoch = opt.steps, int(ck.get("epoch", 0))
            spe = steps_per_epoch(len(self.system.train_dataset), int(self.hp["train.batch_size"]), self.world)
            self.batch = max(0, min(self.global_step - self.epoch * spe, spe))
        self.sched.last_epoch = self.global_step
        lrs = self.sched.get_lr()
        for g, lr in zip(opt.param_groups, lrs):
            g["lr"] = lr
        self.sched._last_lr = list(lrs)

    # -- one step -----------------------------------------------------------------------------------------------------
    def _tighten(self, batch):
        """(rays, rgbs) with every ray's near / far replaced by its occupied span [near', far'] of `ops.ray_span` on the run's grid --
        what the captured step does in its static buffers, for the eager routes.  Keeps (live, first, last) for the log."""
        from . import ops
        rays, rgbs = batch
        m = self.system.mip_nerf
        self._span_n = int(self.occ.span_samples or m.num_samples)
        live, first, last, near, far = ops.ray_span(self.occ.occupancy, rays, self._span_n, disparity=m.disparity)
        self._span = (live, first, last)
        return rays._replace(near=near, far=far), rgbs

    def _span_stats(self):
        """(live share, span share) of the last step's batch, from the captured step's static buffers or the last `_tighten`."""
        if self._span is None:
            return self.gstep.span_stats()
        live, first, last = self._span
        live = live.bool()
        n = int(live.sum())
        share = float((last[live] - first[live] + 1).double().mean()) / self._span_n if n else float("nan")
        return n / float(max(live.numel(), 1)), share

    def _eager_step(self, b, bs):
        """One step off the graph: the epoch's short last batch on the graph route, every batch otherwise.  Returns (loss, psnr)."""
        system, opt = self.system, self.opt
        ids = self.order[b * self.B:b * self.B + bs]
        batch = system.train_dataset.rays_at(ids)
        if self.guided is not None:
            from . import ops
            ops.guided_apply(self.guided.state, batch[0].lossmult, self.n_local, batch=b, batch_size=self.B)
        if self.occ is not None:
            batch = self._tighten(batch)
        opt.zero_grad()
        if self.graph_route:
            loss = system.training_step_native(batch, b)
        else:
            # autograd would accumulate into the flat gradient views: start from no gradient, gather_foreign_grads (in
            # FlatAdam.step) then moves what the backward produced into the flat buffer
            for p in system.mip_nerf.parameters():
                p.grad = None
            loss = system.training_step(batch, b)
            loss.backward()
        if self.guided is not None:
            gt = batch[1][..., :3].contiguous()
            ops.guided_accumulate(self.guided.state, system.mip_nerf.last_fine_rgb.contiguous(), gt, self.n_local, batch=b, batch_size=self.B)
        if self.world > 1:
            import torch.distributed as dist
            system.mip_nerf.mlp.gather_foreign_grads()
            dist.all_reduce(system.mip_nerf.mlp._flat_grad, op=dist.ReduceOp.SUM)
        opt.step()
        if self.graph_route:
            # the captured step re-packs the MFMA weight streams at its END: re-pack the update of this eager step now, or the
            # next replay's forward would run on the weights from before it
            system.mip_nerf.mlp.native(self.dev)
        return loss.detach(), system.logged["train/psnr"]

    def _step(self, b):
        bs = self.B if b < self.spe - 1 else self.last_bs
        if self.graph_route and bs == self.B:
            if self.gstep.use_graph and self.gstep._graphs is None:
                self._capture()
            s = self.gstep()
            self._span = None           # the spans of this step are in the captured step's buffers
            return s[0], s[5]
        return self._eager_step(b, bs)

    # -- validation, checkpoints ---------------------------------------------------------------------------------------
    def validate(self, n_images, sanity=False):
        """`n_images` images of the val split through validation_step / validation_epoch_end (the split walks its images round-robin).
        Returns (val/loss, val/psnr) as floats; writes the GT|coarse|fine stack and the distance map of every image unless `sanity`."""
        from . import ops
        from .rays import Rays
        system, ds = self.system, self.system.val_dataset
        kept = {}
        render = system.render_image

        def render_and_keep(batch, return_distance=False):
            c, f, m, d = render(batch, return_distance=True)
            kept.update(c=c, f=f, d=d)
            return (c, f, m, d) if return_distance else (c, f, m)
        system.render_image = render_and_keep
        outs = []
        try:
            with torch.no_grad():
                for i in range(int(n_images)):
                    rays, img = ds[i]
                    batch = (Rays(*[t[None] for t in rays]), img[None])
                    outs.append(system.validation_step(batch, i))
                    if not sanity and self.logger is not None:
                        gt = img[..., :3]
                        stack = torch.cat([gt, kept["c"][0], kept["f"][0]], dim=1).contiguous()        # [H, 3W, 3]
                        self.logger.image("val/GT_coarse_fine", self.global_step - 1, i, ops.image_to_u8(stack))
                        self.logger.image("val/depth", self.global_step - 1, i, ops.visualize_map(kept["d"][0].contiguous()))
        finally:
            del system.render_image
        logged = getattr(system, "logged", None)
        if isinstance(logged, dict):
            system.validation_epoch_end(outs)
            return float(logged["val/loss"]), float(logged["val/psnr"])
        return (float(torch.stack([x["val/loss"] for x in outs]).mean()), float(torch.stack([x["val/psnr"] for x in outs]).mean()))

    def checkpoint(self):
        """Lightning 1.5's checkpoint dict, plus the trainer's own position / RNG states / top-k record."""
        sched = self.sched.state_dict()
        occ = {} if self.occ is None else {"occupancy": self.occ.state_dict()}
        if self.guided is not None:
            occ["guided"] = self.guided.state_dict(self.order)
        return {"epoch": self.epoch, "global_step": self.global_step, "pytorch-lightning_version": PL_VERSION,
                "state_dict": _cpu(self.system.state_dict()), "callbacks": {},
                "optimizer_states": [_cpu(self.opt.state_dict())], "lr_schedulers": [_cpu(sched)],
                "hparams_name": "hparams", "hyper_parameters": dict(self.system.hparams),
                TRAINER_KEY: {"global_step": self.global_step, "epoch": self.epoch, "batch": self.batch, "topk": self.topk.state_dict(),
                              "rng": {"torch": torch.get_rng_state(), "cuda": torch.cuda.get_rng_state(self.dev),
                                      "numpy": np.random.get_state(), "python": random.getstate()}, **occ}}

    def _save(self, val_psnr):
        name, drop = self.topk.update(val_psnr, self.epoch, self.global_step - 1)
        ck = self.checkpoint()
        if name is not None:
            torch.save(ck, os.path.join(self.ckpt_dir, name))
        for old in drop:
            path = os.path.join(self.ckpt_dir, old)
            if os.path.exists(path):
                os.remove(path)
        torch.save(ck, os.path.join(self.ckpt_dir, "last.ckpt"))

    def _say(self, msg):
        if self.verbose:
            print(f"[train] {msg}", flush=True)

    # -- the loop -----------------------------------------------------------------------------------------------------
    def fit(self, until=None):
        """Train to `optimizer.max_steps` (or stop after `until` steps in all, with the same schedule)."""
        hp, ds = self.hp, self.system.train_dataset
        max_steps, interval = int(hp["optimizer.max_steps"]), int(hp["val.check_interval"])
        stop = max_steps if until is None else min(int(until), max_steps)
        n_val = int(hp["val.sample_num"])
        if self.rank == 0:      # the sanity check leaves the random streams as they were (a resumed run runs one more of them)
            states = (torch.get_rng_state(), torch.cuda.get_rng_state(self.dev))
            self.validate(1, sanity=True)
            torch.set_rng_state(states[0])
            torch.cuda.set_rng_state(states[1], self.dev)
        t0 = time.time()
        while self.global_step < stop:
            if self.guided is None:     # (a guided run draws its order segment by segment, below)
                order = epoch_order(len(ds), int(hp["seed"]), self.epoch, self.rank, self.world, ds.device)
                self.order.copy_(order)
            if self.graph_route:
                self.epoch_base.fill_(self.opt.steps - self.batch)
            for b in range(self.batch, self.spe):
                if self.global_step >= stop:
                    break
                if self.occ is not None and (self.occ.refresh_due(self.global_step) or self.occ.refreshes == 0):
                    self.occ.refresh(self.system)       # from the field as it is BEFORE this step; the first one from the untrained field
                if self.guided is not None and self.guided.refresh_due(b):
                    self.guided.refresh(self.order, b, self.B, self.n_local)      # the errors up to batch b - 1; the ids of batches b .. b + interval - 1
                loss, psnr = self._step(b)
                self.sched.step()
                self.global_step += 1
                self.batch = b + 1
                if self.rank != 0:
                    continue
                if self.global_step % self.log_every == 0 or self.global_step >= max_steps:
                    lr = self.opt.last_lr() if self.graph_route else self.opt.param_groups[0]["lr"]
                    row = {"lr": lr, "train/loss": float(loss), "train/psnr": float(psnr)}
                    if self.occ is not None:
                        row.update(zip(self.SPAN_COLUMNS, self._span_stats()))
                    if self.guided is not None:
                        row.update(zip(self.guided.COLUMNS, self.guided.stats(b, self.n_local)))
                    self.logger.log(self.global_step - 1, row)
                    self._say(f"epoch {self.epoch} step {self.global_step}/{max_steps} loss {row['train/loss']:.5f} "
                              f"psnr {row['train/psnr']:.3f} lr {lr:.3g} ({(time.time() - t0) / max(self.global_step, 1) * 1e3:.2f} ms/step)")
                if should_validate(b, interval, self.global_step, max_steps):
                    vl, vp = self.validate(n_val)
                    self.logger.log(self.global_step - 1, {"val/loss": vl, "val/psnr": vp})
                    self._save(vp)
                    self._say(f"validation at step {self.global_step}: val/loss {vl:.5f} val/psnr {vp:.3f}")
            if self.batch >= self.spe:
                self.epoch += 1
                self.batch = 0
        torch.cuda.synchronize(self.dev)
        if self.world > 1:
            self._check_replicas()
        if self.logger is not None:
            self.logger.close()
        return self

    def _check_replicas(self):
        """Every rank's parameters and moments equal rank 0's (one broadcast at the end of training); with span training also a checksum
        of the occupancy grid's words, which every rank refreshes from its own replica."""
        import torch.distributed as dist
        mine = torch.cat([self.system.mip_nerf.mlp._flat_param, self.opt.exp_avg, self.opt.exp_avg_sq])
        ref = mine.clone()
        dist.broadcast(ref, 0)
        equal = torch.equal(mine, ref)
        if self.occ is not None:
            mine = self.occ.checksum().reshape(1)
            ref = mine.clone()
            dist.broadcast(ref, 0)
            equal = equal and torch.equal(mine, ref)
        same = torch.tensor([int(equal)], device=self.dev)
        dist.all_reduce(same, op=dist.ReduceOp.MIN)
        if not bool(same.item()):
            raise RuntimeError("[train] the replicas' parameters diverged")
        self._say(f"replicas identical on {self.world} ranks" + (" (occupancy grid included)" if self.occ is not None else ""))


# ---------------------------------------------------------------------------------------------------------------------
# command line
# ---------------------------------------------------------------------------------------------------------------------
def build_parser():
    p = argparse.ArgumentParser(prog="python -m mipnerf_pl_amd.train")
    p.add_argument("--data_path", help="data path (multi_blender: a converted directory, or a Blender scene directory to build the scales on the device).", type=str, required=True)
    p.add_argument("--out_dir", help="Output directory.", type=str, required=True)
    p.add_argument("--dataset_name", help="Single or multi data.", type=str, choices=["multi_blender", "blender", "llff", "realdata360"], required=True)
    p.add_argument("--factor", help="llff / realdata360: read images_<factor>/, or shrink images/ by it on the device.", type=int, default=4)
    p.add_argument("--config", help="Path to config file (default: the reference's configs/lego.yaml, built in).", default=None)
    p.add_argument("--precision", help="MLP precision", choices=["fp32", "bf16"], default="bf16")
    p.add_argument("--no-graph", dest="use_graph", help="run every step eagerly instead of replaying a captured hipGraph",
                   action="store_false")
    p.add_argument("--log_every_n_steps", help="read and log the training loss every N steps", type=int, default=50)
    p.add_argument("--child_timeout", help="seconds each rank of a num_gpus > 1 run may take", type=float, default=30 * 86400.0)
    p.add_argument("opts", nargs=argparse.REMAINDER, help="Modify hparams. Example: train.batch_size 1024 val.check_interval 500")
    return p


def _free_port():
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def launch_ranks(argv, world, timeout):
    """Start `world` children running this command as ranks 0..world-1 (fresh processes), wait for all of them, each under
    `timeout` seconds; a failing or overdue child ends the others.  Returns the worst exit status."""
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()), WORLD_SIZE=str(world))
    procs = []
    for r in range(world):
        e = dict(env, RANK=str(r), LOCAL_RANK=str(r), MIPNERF_TRAIN_CHILD="1")
        procs.append(subprocess.Popen([sys.executable, "-m", "mipnerf_pl_amd.train"] + list(argv), env=e))
    deadline, status = time.time() + timeout, 0
    while procs:
        for p in list(procs):
            rc = p.poll()
            if rc is None:
                continue
            procs.remove(p)
            if rc != 0:
                status = rc
        if status != 0 or time.time() > deadline:
            if status == 0:
                print(f"[train] a rank ran past --child_timeout ({timeout:g} s)", file=sys.stderr)
                status = 124
            for p in procs:
                p.kill()
            for p in procs:
                p.wait()
            break
        time.sleep(0.2)
    return status


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    args = build_parser().parse_args(argv)
    hp = cfg.resolve(args)
    cfg.check_train_guided(hp)          # before any rank is started
    world = int(hp["num_gpus"])
    if world > 1 and os.environ.get("MIPNERF_TRAIN_CHILD") != "1":
        rc = launch_ranks(argv, world, args.child_timeout)
        if rc != 0:
            raise SystemExit(f"[train] a rank failed (exit status {rc})")
        return None
    rank = int(os.environ.get("RANK", "0")) if world > 1 else 0
    if world > 1:
        import torch.distributed as dist
        own = torch.cuda.device_count() >= world and os.environ.get("MIPNERF_TRAIN_SHARE_GPU") != "1"
        dev = torch.device("cuda", rank if own else 0)
        torch.cuda.set_device(dev)
        dist.init_process_group("nccl" if own else "gloo", rank=rank, world_size=world)
    else:
        dev = torch.device("cuda", torch.cuda.current_device())
    try:
        trainer = Trainer(hp, precision=args.precision, use_graph=args.use_graph, log_every_n_steps=args.log_every_n_steps,
                          rank=rank, world=world, device=dev).fit()
    finally:
        if world > 1:
            import torch.distributed as dist
            dist.barrier()
            dist.destroy_process_group()
    return trainer


if __name__ == "__main__":
    main()
