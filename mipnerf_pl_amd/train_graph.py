"""The whole optimisation step of the hot path replayed from ONE captured hipGraph:

    random draws (torch device RNG, graph-safe) -> mipnerf_train_step (forward of both levels, loss incl. distloss, backward)
    -> Adam with the MipLRDecay schedule evaluated on the device (mipnerf_adam_step_scheduled) -> re-pack of the MFMA
    weight streams from the updated fp32 master parameters (mipnerf_set_params)

i.e. MipNeRFSystem.training_step + loss.backward() + optimizer.step() + scheduler.step() of the reference's loop
(nerf_system.py:70-76, 95-121) with no per-step host scalar: the step counter, learning rate and bias corrections live in
device memory.  With world_size > 1 the step is two graphs around one eager RCCL all-reduce of the flat gradient buffer
(SUM; the 1/world mean is folded into the Adam kernel): graph A = draws + forward + backward, graph B = Adam + re-pack.

With `occupancy` (an `ops.Occupancy`, e.g. the one `train_occupancy.TrainOccupancy` keeps fresh) the step trains every ray on its occupied
span: right after the batch source, `ops.ray_span` (inside the graph; it reads the grid's words where they live, so a refresh between two
replays is seen by the next one) writes `live`, `first`, `last`, `near_span`, `far_span`, and the step samples [near_span, far_span];
`self.rays.near` / `.far` keep the gathered values.  A dead ray keeps [near, far] and is still trained.

With `guided` (an `ops.GuidedState`, e.g. the one `train_guided.TrainGuided` refreshes) and `guided_index` = (step, epoch_base, n_order) --
the device batch index the batch source reads, and the length of its order -- the step weighs and records what an error-guided sampler drew:
`ops.guided_apply` right after the batch source (before `ops.ray_span`) multiplies `self.rays.lossmult` by the ring's importance weights,
the `out` argument of mipnerf_train_step copies the fine level's colours into the static `self.fine_rgb`, and `ops.guided_accumulate` after
it adds their squared errors to the state's integer counters -- inside the same graph (graph A of the collective form), before the optimiser
kernel advances the step counter.  Both read the rings where they live, so a refresh between two replays is seen by the next one.  Without
`guided` the object issues exactly the calls it issued before.

Inputs live in static buffers (`self.rays`, `self.gt`): write the next batch there (copy_ or device-side ray generation
straight into them) and call the object, or give a `batch_source`: a callable issued first inside the step (inside the captured
graph) that writes the batch itself, e.g. `ops.gather_train_batch` with the batch index read from the device (train.py).  Returns the static scalars tensor [6] = loss, mse_c, mse_f, distloss_c,
distloss_f, psnr_fine (valid until the next call).
"""
from __future__ import annotations

import ctypes as C
import os

import torch
import torch.distributed as dist

from . import _lib as L
from . import ops
from .rays import Rays


class GraphedTrainStep:
    def __init__(self, system, optimizer, num_rays: int, device: torch.device, use_graph: bool = True, batch_source=None,
                 occupancy=None, span_samples=None, guided=None, guided_index=None):
        from .optim import FlatAdam
        if not isinstance(optimizer, FlatAdam):
            raise TypeError("GraphedTrainStep needs the flat optimiser (system.fused_adam = True)")
        model = system.mip_nerf
        if model.precision != L.PREC_BF16:
            raise NotImplementedError("GraphedTrainStep is the bf16 native training path")
        self.system, self.model, self.opt = system, model, optimizer
        self.B, self.N, self.dev = int(num_rays), model.num_samples, device
        self.use_graph = bool(use_graph)
        self.batch_source = batch_source    # optional callable writing self.rays / self.gt on the device, issued first in _fwd_bwd
        self.world = dist.get_world_size() if dist.is_available() and dist.is_initialized() else 1
        # the collective form (graph A, all-reduce on the process group's communicator, graph B) is what every world > 1 run
        # uses; MIPNERF_FORCE_COLLECTIVE_PATH=1 takes it at world 1 too when a process group exists (a 1-rank RCCL
        # communicator is legal), so a single-GPU box exercises the two-graph + RCCL sequence end to end
        self.collective = self.world > 1 or (os.environ.get("MIPNERF_FORCE_COLLECTIVE_PATH") == "1"
                                             and dist.is_available() and dist.is_initialized())
        self.capture_error = None
        self.time_allreduce = False        # True: a HIP event pair around every all-reduce (allreduce_stats)
        self._ar_events = []
        optimizer.grad_scale = 1.0 / self.world
        optimizer._graph_driven = True      # its steps are graph replays: lr_schedule.DeviceMipLRDecay.step reads this
        self.rays = Rays(*[torch.zeros(self.B, k, device=device) for k in (3, 3, 3, 1, 1, 1, 1)])
        self.rays.directions[:, 2] = 1.0
        self.rays.viewdirs[:, 2] = 1.0
        self.rays.radii.fill_(1e-3)
        self.rays.lossmult.fill_(1.0)
        self.rays.near.fill_(2.0)
        self.rays.far.fill_(6.0)
        self.gt = torch.zeros(self.B, 3, device=device)
        self.scalars = torch.zeros(6, device=device)
        self.randomized = bool(system.train_randomized)
        self.white = bool(system.white_bkgd)
        self.hp = system.hparams
        self._graphs = None
        self._work = None
        mlp = model.mlp
        self.ctx = mlp.native(device)
        need = int(L.lib().mipnerf_train_workspace_bytes(self.ctx.handle, self.B))
        self.ws = self.ctx.scratch("train_step", need)
        mlp.gather_foreign_grads()
        self._rp = L.RaysPtrs(*[t.data_ptr() for t in self.rays])
        self.occupancy = occupancy
        if occupancy is not None:
            from .train_occupancy import check_spaces
            check_spaces(model, occupancy, "GraphedTrainStep")
            self.span_samples = int(span_samples or model.num_samples)
            if not 1 <= self.span_samples <= L.MAX_SAMPLES:
                raise ValueError(f"GraphedTrainStep: span_samples must be in [1, {L.MAX_SAMPLES}] (got {self.span_samples})")
            self.live = torch.zeros(self.B, dtype=torch.uint8, device=device)
            self.first = torch.zeros(self.B, dtype=torch.int32, device=device)
            self.last = torch.zeros(self.B, dtype=torch.int32, device=device)
            self.near_span = torch.zeros(self.B, 1, device=device)
            self.far_span = torch.zeros(self.B, 1, device=device)
            # the step reads near' / far' where it read near / far
            self._rp = L.RaysPtrs(*[t.data_ptr() for t in self.rays._replace(near=self.near_span, far=self.far_span)])
        self.guided, self._outs = guided, None
        if guided is not None:
            if batch_source is None or guided_index is None:
                raise ValueError("GraphedTrainStep: guided needs a batch_source (lossmult is re-written before it is weighted) and "
                                 "guided_index = (step, epoch_base, n_order)")
            self.guided_step, self.guided_base, self.guided_n_order = guided_index[0], guided_index[1], int(guided_index[2])
            self.fine_rgb = torch.zeros(self.B, 3, device=device)
            self._outs = (L.LevelOut * model.num_levels)()
            self._outs[model.num_levels - 1] = L.LevelOut(self.fine_rgb.data_ptr(), None, None, None, None)
        ptrs = [p.data_ptr() for p in mlp.ordered_params()]
        self._params = (C.c_void_p * len(ptrs))(*ptrs)

    # ---- the two halves ------------------------------------------------------------------------------------------------
    def _fwd_bwd(self):
        m, B, N = self.model, self.B, self.N
        if self.batch_source is not None:
            self.batch_source()
        if self.guided is not None:
            ops.guided_apply(self.guided, self.rays.lossmult, self.guided_n_order, self.guided_step, self.guided_base)
        if self.occupancy is not None:
            ops.ray_span(self.occupancy, self.rays, self.span_samples, disparity=m.disparity,
                         out=(self.live, self.first, self.last, self.near_span, self.far_span))
        t_rand = u_rand = dz = None
        if self.randomized:
            draws = torch.rand(2, B, N + 1, device=self.dev)        # one launch for both draws
            t_rand, u_rand = draws[0], draws[1]                     # mip.py:159 / mip.py:201
            if m.density_noise > 0:
                dz = torch.randn(m.num_levels, B, N, device=self.dev)   # mip_nerf.py:232-233
        flags = L.FLAG_WHITE_BKGD if self.white else 0
        L.check(L.lib().mipnerf_train_step(
            self.ctx.handle, B, C.byref(self._rp), self.gt.data_ptr(), None if t_rand is None else t_rand.data_ptr(),
            None if u_rand is None else u_rand.data_ptr(), None if dz is None else dz.data_ptr(), flags,
            float(self.hp['loss.coarse_loss_mult']), 0.01, int(bool(self.hp['loss.disable_multiscale_loss'])),
            self.ws.data_ptr(), self.ws.numel(), m.mlp._flat_grad.data_ptr(), 0, self.scalars.data_ptr(), self._outs, ops._stream()),
            "train_step")
        if self.guided is not None:
            ops.guided_accumulate(self.guided, self.fine_rgb, self.gt, self.guided_n_order, self.guided_step, self.guided_base)

    def _update(self):
        self.opt.launch_scheduled(count_on_host=False)
        # the packed bf16 / fp32 weight streams follow the master parameters inside the same graph
        L.check(L.lib().mipnerf_set_params(self.ctx.handle, self._params, ops._stream()), "mipnerf_set_params")

    def _capture(self):
        try:
            self._capture_impl()
        except RuntimeError as e:      # e.g. a collective library thread touching the device during a global-mode capture
            import sys
            print(f"[mipnerf_pl_amd] hipGraph capture of the training step failed ({e}); running it eagerly", file=sys.stderr)
            torch.cuda.synchronize()
            self.use_graph, self._graphs, self.capture_error = False, None, f"{type(e).__name__}: {e}"

    def _capture_impl(self):
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        snap = self._snapshot()
        with torch.cuda.stream(s):          # warm-up on a side stream (lazy initialisation of kernels / generators)
            self._fwd_bwd()
            self._update()
        torch.cuda.current_stream().wait_stream(s)
        torch.cuda.synchronize()
        self._restore(snap)                 # the warm-up must not count as a training step
        if not self.collective:
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, capture_error_mode="thread_local"):
                self._fwd_bwd()
                self._update()
            self._graphs = (g,)
        else:
            ga, gb = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
            # thread_local: RCCL's watchdog thread may query events while this thread captures
            with torch.cuda.graph(ga, capture_error_mode="thread_local"):
                self._fwd_bwd()
            with torch.cuda.graph(gb, capture_error_mode="thread_local"):
                self._update()
            self._graphs = (ga, gb)

    def _snapshot(self):
        mlp, st = self.model.mlp, self.opt.state[self.opt._key()]
        return (mlp._flat_param.clone(), st["exp_avg"].clone(), st["exp_avg_sq"].clone(),
                None if self.opt._dev_step is None else self.opt._dev_step.clone(),
                None if self.guided is None else (self.guided.sum.clone(), self.guided.cnt.clone()))

    def _restore(self, snap):
        mlp, st = self.model.mlp, self.opt.state[self.opt._key()]
        mlp._flat_param.copy_(snap[0])
        st["exp_avg"].copy_(snap[1])
        st["exp_avg_sq"].copy_(snap[2])
        if self.opt._dev_step is not None:
            self.opt._dev_step.fill_(int(st["step"]))
        if self.guided is not None:             # the warm-up's errors are not a training step's
            self.guided.sum.copy_(snap[4][0])
            self.guided.cnt.copy_(snap[4][1])
        L.check(L.lib().mipnerf_set_params(self.ctx.handle, self._params, ops._stream()), "mipnerf_set_params")

    def span_stats(self):
        """(live share, span share) of the last step's batch: the share of rays with an occupied frustum and the mean of
        (last - first + 1) / span_samples over them (NaN when none is live).  A host read-back of the static buffers."""
        live = self.live.bool()
        n = int(live.sum())
        share = float((self.last[live] - self.first[live] + 1).double().mean()) / self.span_samples if n else float("nan")
        return n / float(self.B), share

    def allreduce_stats(self):
        """(mean ms, count) of the event pairs recorded around the gradient all-reduce since the last call (synchronises)."""
        if not self._ar_events:
            return None, 0
        self._ar_events[-1][1].synchronize()
        ms = [a.elapsed_time(b) for a, b in self._ar_events]
        self._ar_events = []
        return sum(ms) / len(ms), len(ms)

    # ---- one optimisation step -----------------------------------------------------------------------------------------
    def __call__(self):
        mlp, st = self.model.mlp, self.opt.state[self.opt._key()]
        if not mlp.grads_are_flat():
            raise RuntimeError("GraphedTrainStep: the parameters / gradients are no longer views of the flat buffers")
        if self.use_graph and self._graphs is None:
            self._capture()          # may fall back to eager (sets use_graph False)
        if not self.collective:
            if self.use_graph:
                self._graphs[0].replay()
            else:
                self._fwd_bwd()
                self._update()
        else:
            if self.use_graph:
                self._graphs[0].replay()
            else:
                self._fwd_bwd()
            # one SUM all-reduce of the 2.45 MB flat gradient; c10d runs it on its own stream, ordered after the backward
            # by an event, so the host goes on (next batch's ray generation) while it is in flight; wait() orders the Adam
            # kernels behind it.  The mean (1 / world) is applied inside the Adam kernel.
            if self.time_allreduce and len(self._ar_events) < 4096:
                ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                ev[0].record()
                work = dist.all_reduce(mlp._flat_grad, op=dist.ReduceOp.SUM, async_op=True)
                work.wait()
                ev[1].record()             # on the launch stream, behind the all-reduce it now waits for
                self._ar_events.append(ev)
            else:
                work = dist.all_reduce(mlp._flat_grad, op=dist.ReduceOp.SUM, async_op=True)
                work.wait()
            if self.use_graph:
                self._graphs[1].replay()
            else:
                self._update()
        st["step"] += 1
        mlp._flat_grad_valid = False        # consumed: the next backward overwrites
        # master parameters changed behind torch's back (no version bump) and the streams were re-packed in the graph
        self.ctx._packed_key = tuple((p.data_ptr(), p._version) for p in mlp.ordered_params())
        return self.scalars
