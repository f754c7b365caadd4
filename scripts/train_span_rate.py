#!/usr/bin/env python3
"""Span training measured on one MI355X: what a training run costs and reaches with and without
`train.occupancy.enabled`, on the analytic multi-scale scene of tests/dataset_fixture.py (`write_multicam_scene`).

    python scripts/train_span_rate.py --data DIR [--runs A,B,C,D] [--steps 4000] [--batch 4096] [--out profiles/train_span_rate.json]
    python scripts/train_span_rate.py --kernel                      # the rate of k_lattice_decay_max beside a device copy
    python scripts/train_span_rate.py --write-scene DIR [--base 128]    # the scene (CPU only)

The runs: (A) off, 128 samples; (B) on, 128; (C) on, 64; (D) off, 64 -- the same seed, scene, schedule and number of steps.  Per run:
  step_ms          mean and median of the HIP-event pairs around every graph replay (the refresh lies outside them; the epoch's short
                   eager batch is not timed);
  refresh_ms       mean of the event pairs around every refresh (density lattice + decay-max + bits);
  amortised_ms     step_ms + refresh_ms / interval;
  curve            every `--sample-every` steps: live share and span share of that step's batch, occupied share of the grid;
  psnr / psnr_cull test PSNR of `evaluate.evaluate`, un-culled and with an occupancy grid of the trained field and tightened rays
                   (what `eval --cull --cull_tighten` does).
A run with the feature off uses nothing the feature added, so the same file times the parent commit's tree (`--runs A --no-eval`).
"""
import argparse
import json
import os
import statistics
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

RUNS = {"A": (False, 128), "B": (True, 128), "C": (True, 64), "D": (False, 64)}


def write_scene(root, base):
    from tests import dataset_fixture as fx
    return fx.write_multicam_scene(root, base=base)


def hparams(args, enabled, samples, out_dir):
    from mipnerf_pl_amd import config as cfg
    hp = dict(cfg.DEFAULTS, data_path=args.data, out_dir=out_dir, dataset_name="multi_blender", exp_name="span")
    hp.update({"train.batch_size": args.batch, "nerf.num_samples": samples, "val.check_interval": 10 ** 9, "val.sample_num": 1,
               "val.chunk_size": 8192, "optimizer.max_steps": args.steps, "optimizer.lr_init": 2e-3, "optimizer.lr_final": 2e-5,
               "optimizer.lr_delay_steps": max(1, args.steps // 20), "seed": args.seed})
    if enabled:
        hp.update({"train.occupancy.enabled": True, "train.occupancy.grid": args.grid, "train.occupancy.threshold": args.threshold,
                   "train.occupancy.interval": args.interval, "train.occupancy.decay": args.decay})
    return hp


def train(args, name, out_dir):
    """Trainer.fit's loop with event pairs around the replays and the refreshes (no validation, no checkpoint, no log)."""
    import torch
    from mipnerf_pl_amd.train import Trainer, epoch_order
    enabled, samples = RUNS[name]
    hp = hparams(args, enabled, samples, out_dir)
    tr = Trainer(hp, verbose=False, log_every_n_steps=10 ** 9)
    occ = getattr(tr, "occ", None)
    assert (occ is not None) == enabled and tr.graph_route
    ds = tr.system.train_dataset
    ev = lambda: torch.cuda.Event(enable_timing=True)      # noqa: E731
    steps, refreshes, curve = [], [], []
    while tr.global_step < args.steps:
        tr.order.copy_(epoch_order(len(ds), int(hp["seed"]), tr.epoch, 0, 1, ds.device))
        tr.epoch_base.fill_(tr.opt.steps - tr.batch)
        for b in range(tr.batch, tr.spe):
            if tr.global_step >= args.steps:
                break
            if occ is not None and occ.refresh_due(tr.global_step):
                e = (ev(), ev())
                e[0].record()
                occ.refresh(tr.system)
                e[1].record()
                refreshes.append(e)
            full = b < tr.spe - 1 or tr.last_bs == tr.B
            if full and tr.gstep._graphs is not None:
                e = (ev(), ev())
                e[0].record()
                tr._step(b)
                e[1].record()
                steps.append(e)
            else:               # the capture, or the short batch
                tr._step(b)
            tr.sched.step()
            tr.global_step += 1
            tr.batch = b + 1
            if occ is not None and full and tr.global_step % args.sample_every == 0:
                live, span = tr._span_stats()
                curve.append({"step": tr.global_step, "live_share": live, "span_share": span,
                              "occupied_share": occ.occupancy.occupied_fraction()})
        if tr.batch >= tr.spe:
            tr.epoch += 1
            tr.batch = 0
    torch.cuda.synchronize()
    ms = [a.elapsed_time(b) for a, b in steps[args.skip:]]
    out = {"enabled": enabled, "num_samples": samples, "steps": args.steps, "timed_replays": len(ms),
           "step_ms": statistics.fmean(ms), "step_ms_median": statistics.median(ms)}
    if refreshes:
        rms = [a.elapsed_time(b) for a, b in refreshes[1:]]         # the first one loads code objects
        out.update(refresh_ms=statistics.fmean(rms), refreshes=len(refreshes),
                   amortised_ms=out["step_ms"] + statistics.fmean(rms) / args.interval, curve=curve)
    else:
        out["amortised_ms"] = out["step_ms"]
    return tr, out


def evaluate_run(args, tr, out_dir, name):
    import numpy as np
    from mipnerf_pl_amd import evaluate
    from mipnerf_pl_amd.datasets import dataset_dict
    test = dataset_dict["multi_blender"](data_dir=args.data, split="test", white_bkgd=True, batch_type="single_image", device=tr.dev)
    psnr, _ = evaluate.evaluate(tr.system, test, out_dir, name, scale=4, chunk_size=8192, base_size=(args.base, args.base))
    occ = evaluate.scene_occupancy(tr.system, (test[i][0] for i in range(len(test))), grid=args.grid, threshold=args.threshold, verbose=False)
    cull, _ = evaluate.evaluate(tr.system, test, out_dir, name + "_cull", scale=4, chunk_size=8192, base_size=(args.base, args.base),
                                occupancy=occ, tighten=True)
    return {"psnr": float(np.mean(psnr)), "psnr_cull_tighten": float(np.mean(cull)), "eval_grid_occupied_share": occ.occupied_fraction()}


def kernel_rate(points=512, iters=10):
    """ms of mipnerf_occupancy_refresh and of mipnerf_occupancy_build alone on a points^3 lattice (dilate 0): the difference is
    k_lattice_decay_max, 12 B per point; beside a device-to-device copy of the same bytes (scripts/hbm_bw.py's figure)."""
    import torch
    from mipnerf_pl_amd import ops

    def window(fn):
        fn()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) / iters
    n = points ** 3
    fresh, running = torch.rand(points, points, points, device="cuda"), torch.rand(points, points, points, device="cuda")
    occ = ops.occupancy_grid(running, 0.5, -1.0, 1.0, dilate=0)
    out = {"points": n, "refresh_ms": [], "build_ms": [], "copy_ms": []}
    for _ in range(5):          # alternating
        out["refresh_ms"].append(window(lambda: ops.occupancy_refresh(occ, fresh, running, 0.95)))
        out["build_ms"].append(window(lambda: ops.occupancy_grid(running, 0.5, -1.0, 1.0, dilate=0)))
        out["copy_ms"].append(window(lambda: running.copy_(fresh)))
    r, bld, c = (statistics.median(out[k]) for k in ("refresh_ms", "build_ms", "copy_ms"))
    out.update(decay_max_ms=r - bld, decay_max_tb_s=12.0 * n / (r - bld) / 1e9, copy_tb_s=8.0 * n / c / 1e9)
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--data")
    p.add_argument("--write-scene")
    p.add_argument("--kernel", action="store_true")
    p.add_argument("--base", type=int, default=128)
    p.add_argument("--runs", default="A,B,C,D")
    p.add_argument("--steps", type=int, default=4000)
    p.add_argument("--batch", type=int, default=4096)
    p.add_argument("--seed", type=int, default=4)
    p.add_argument("--grid", type=int, default=128)
    p.add_argument("--threshold", type=float, default=0.01)
    p.add_argument("--interval", type=int, default=16)
    p.add_argument("--decay", type=float, default=0.95)
    p.add_argument("--skip", type=int, default=50, help="timed replays dropped at the start of a run")
    p.add_argument("--sample-every", type=int, default=200)
    p.add_argument("--no-eval", action="store_true")
    p.add_argument("--out", default=os.path.join(REPO, "profiles", "train_span_rate.json"))
    args = p.parse_args()
    if args.write_scene:
        print(write_scene(args.write_scene, args.base))
        return
    import torch
    assert torch.cuda.is_available(), "train_span_rate.py measures on a GPU"
    result = {"device": torch.cuda.get_device_name(0), "args": {k: v for k, v in vars(args).items() if k not in ("out", "data", "write_scene")}}
    if args.kernel:
        result["kernel"] = kernel_rate()
    else:
        result["runs"] = {}
        for name in args.runs.split(","):
            with tempfile.TemporaryDirectory() as tmp:
                tr, out = train(args, name, tmp)
                if not args.no_eval:
                    out.update(evaluate_run(args, tr, tmp, name))
            result["runs"][name] = out
            print(name, json.dumps({k: v for k, v in out.items() if k != "curve"}), flush=True)
            del tr
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print(json.dumps({k: v for k, v in result.items() if k != "runs"}))


if __name__ == "__main__":
    main()
