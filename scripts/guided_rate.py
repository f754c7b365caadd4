#!/usr/bin/env python3
"""Error-guided batch sampling measured on one MI355X: what `train.guided.enabled` costs and what it reaches, on the
analytic multi-scale scene of tests/dataset_fixture.py (the `--write-scene` of scripts/train_span_rate.py).

    python scripts/train_span_rate.py --write-scene DIR
    python scripts/guided_rate.py --data DIR [--parent DIR] [--steps 4000] [--batch 4096] [--out profiles/guided_rate.json]

Every run is a fresh child process (`--child`), one at a time, bf16, captured graph, the same seed, scene and schedule:
  off_cost   the feature off in this tree and, with `--parent DIR` (a built checkout of the parent commit), in that tree, alternating,
             `--repeats` each, no evaluation.  A run with the feature off uses nothing the feature added, so this file drives both trees.
             Criterion: |mean(this) - mean(parent)| of step_ms lies inside the spread between the parent's own repeats;
  quality    per seed of `--seeds`: off, and on with every `--mix` (mix 0 is the control: uniform draws with replacement through the
             sampler's whole path): step_ms; the HIP-event cost of a refresh split into fold + scan and draw (the random integers
             included); `evaluate.evaluate` test PSNR, uniform over all test pixels, at every `--eval-at` step.
step_ms: mean and median of the event pairs around every graph replay (refreshes and the epoch's short eager batch lie outside them), so
what the two in-graph kernels and the colour copy add to a step is step_ms(on) - step_ms(off).
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def hparams(args, out_dir):
    from mipnerf_pl_amd import config as cfg
    hp = dict(cfg.DEFAULTS, data_path=args.data, out_dir=out_dir, dataset_name="multi_blender", exp_name="guided")
    hp.update({"train.batch_size": args.batch, "nerf.num_samples": args.samples, "val.check_interval": 10 ** 9, "val.sample_num": 1,
               "val.chunk_size": 8192, "optimizer.max_steps": args.steps, "optimizer.lr_init": 2e-3, "optimizer.lr_final": 2e-5,
               "optimizer.lr_delay_steps": max(1, args.steps // 20), "seed": args.seed})
    if args.guided:
        hp.update({"train.guided.enabled": True, "train.guided.mix": args.guided_mix})
        for k in ("tile", "interval", "rate"):
            if getattr(args, k) is not None:
                hp["train.guided." + k] = getattr(args, k)
    return hp


def test_psnr(args, tr, out_dir, tag):
    import numpy as np
    from mipnerf_pl_amd import evaluate
    from mipnerf_pl_amd.datasets import dataset_dict
    test = dataset_dict["multi_blender"](data_dir=args.data, split="test", white_bkgd=True, batch_type="single_image", device=tr.dev)
    psnr, _ = evaluate.evaluate(tr.system, test, out_dir, tag, scale=4, chunk_size=8192, base_size=(args.base, args.base))
    return float(np.mean(psnr))


def child(args):
    """Trainer.fit's loop with event pairs around the replays and the two halves of a refresh (no validation, no checkpoint, no log)."""
    import torch
    from mipnerf_pl_amd.train import Trainer, epoch_order
    ev = lambda: torch.cuda.Event(enable_timing=True)      # noqa: E731
    eval_at = [int(s) for s in args.eval_at.split(",") if s] if args.eval_at else []
    with tempfile.TemporaryDirectory() as tmp:
        hp = hparams(args, tmp)
        tr = Trainer(hp, verbose=False, log_every_n_steps=10 ** 9)
        tgd = getattr(tr, "guided", None)
        assert (tgd is not None) == bool(args.guided) and tr.graph_route
        if tgd is not None:
            from mipnerf_pl_amd import ops
        ds = tr.system.train_dataset
        steps, folds, draws, psnr, ess = [], [], [], {}, []
        while tr.global_step < args.steps:
            if tgd is None:
                tr.order.copy_(epoch_order(len(ds), int(hp["seed"]), tr.epoch, 0, 1, ds.device))
            tr.epoch_base.fill_(tr.opt.steps - tr.batch)
            for b in range(tr.batch, tr.spe):
                if tr.global_step >= args.steps:
                    break
                if tgd is not None and tgd.refresh_due(b):      # TrainGuided.refresh, its two halves timed apart
                    s, st = tgd.settings, tgd.state
                    lo, hi = b * tr.B, min((b + s["interval"]) * tr.B, tr.n_local)
                    e = (ev(), ev(), ev())
                    e[0].record()
                    ops.guided_refresh(st, s["rate"], s["mix"])
                    e[1].record()
                    r = torch.randint(0, 1 << 32, (2, hi - lo), dtype=torch.int64, device=tr.dev)
                    ops.guided_draw(st, r, tr.order[lo:hi], ring_start=lo % st.ring_len)
                    e[2].record()
                    tgd.refreshes, tgd.segment = tgd.refreshes + 1, (lo, hi)
                    folds.append(e[:2])
                    draws.append(e[1:])
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
                if tgd is not None and tr.global_step % 500 == 0:
                    ess.append((tr.global_step,) + tgd.stats(b, tr.n_local))
                if tr.global_step in eval_at:
                    psnr[str(tr.global_step)] = test_psnr(args, tr, tmp, f"s{tr.global_step}")
            if tr.batch >= tr.spe:
                tr.epoch += 1
                tr.batch = 0
        torch.cuda.synchronize()
        ms = [a.elapsed_time(b) for a, b in steps[args.skip:]]
        out = {"guided": bool(args.guided), "steps": args.steps, "timed_replays": len(ms), "step_ms": statistics.fmean(ms),
               "step_ms_median": statistics.median(ms), "device": torch.cuda.get_device_name(0)}
        if tgd is not None:
            f = [a.elapsed_time(b) for a, b in folds[1:]]           # the first one loads code objects
            d = [a.elapsed_time(b) for a, b in draws[1:]]
            out.update(settings=tgd.settings, cells=tgd.state.n_cells, draws_per_refresh=tgd.state.ring_len, refreshes=len(folds),
                       fold_scan_ms=statistics.fmean(f), fold_scan_ms_median=statistics.median(f), draw_ms=statistics.fmean(d),
                       draw_ms_median=statistics.median(d),
                       amortised_ms=statistics.fmean(ms) + (statistics.fmean(f) + statistics.fmean(d)) / tgd.settings["interval"],
                       ess_visited=[{"step": s, "ess": e, "visited": v} for s, e, v in ess])
        if psnr:
            out["test_psnr"] = psnr
    print("RESULT " + json.dumps(out), flush=True)


def run_child(args, tree, extra, timeout):
    """One run in a fresh process of `tree` (this file, that tree's package): its result dict."""
    cmd = [sys.executable, os.path.abspath(__file__), "--child", "--tree", tree, "--data", args.data, "--steps", str(args.steps), "--batch",
           str(args.batch), "--samples", str(args.samples), "--seed", str(args.seed), "--skip", str(args.skip), "--base", str(args.base)] + extra
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, cwd=tree)
    if p.returncode != 0:
        raise SystemExit(f"a run failed (exit status {p.returncode}): {' '.join(cmd)}\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}")
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1]
    return json.loads(line[len("RESULT "):])


def main():
    global HERE
    p = argparse.ArgumentParser()
    p.add_argument("--data", required=True)
    p.add_argument("--parent", help="a built checkout of the parent commit, for the off-cost comparison")
    p.add_argument("--tree", default=HERE, help=argparse.SUPPRESS)
    p.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    p.add_argument("--guided", action="store_true", help=argparse.SUPPRESS)
    p.add_argument("--guided-mix", type=float, default=0.5, help=argparse.SUPPRESS)
    p.add_argument("--eval-at", default="1000,2000,4000")
    p.add_argument("--mix", default="0.0,0.5,0.9", help="the mixtures of the quality runs (0: uniform draws with replacement through the sampler)")
    p.add_argument("--tile", type=int)
    p.add_argument("--interval", type=int)
    p.add_argument("--rate", type=float)
    p.add_argument("--repeats", type=int, default=2)
    p.add_argument("--base", type=int, default=128)
    p.add_argument("--steps", type=int, default=4000)
    p.add_argument("--batch", type=int, default=4096)
    p.add_argument("--samples", type=int, default=128)
    p.add_argument("--seed", type=int, default=4, help="the seed of the off-cost runs")
    p.add_argument("--seeds", default="4,5", help="the seeds of the quality runs")
    p.add_argument("--skip", type=int, default=50, help="timed replays dropped at the start of a run")
    p.add_argument("--timeout", type=float, default=400.0, help="seconds a run may take")
    p.add_argument("--skip-quality", action="store_true")
    p.add_argument("--out", default=os.path.join(HERE, "profiles", "guided_rate.json"))
    args = p.parse_args()
    args.data = os.path.abspath(args.data)
    if args.child:
        HERE = os.path.abspath(args.tree)
        sys.path.insert(0, HERE)
        return child(args)
    result = {"args": {k: v for k, v in vars(args).items() if k not in ("out", "data", "parent", "tree", "child", "guided", "guided_mix")}}
    trees = [("this", HERE)] + ([("parent", os.path.abspath(args.parent))] if args.parent else [])
    off = {name: [] for name, _ in trees}
    for rep in range(args.repeats):
        for name, tree in trees:
            r = run_child(args, tree, ["--eval-at", ""], args.timeout)
            off[name].append({k: r[k] for k in ("step_ms", "step_ms_median", "timed_replays")})
            result["device"] = r["device"]
            print(f"off {name} #{rep}: {r['step_ms']:.4f} ms/step (median {r['step_ms_median']:.4f})", flush=True)
    result["off_cost"] = dict(off)
    if args.parent:
        mine, theirs = [r["step_ms"] for r in off["this"]], [r["step_ms"] for r in off["parent"]]
        diff, spread = statistics.fmean(mine) - statistics.fmean(theirs), max(theirs) - min(theirs)
        result["off_cost"].update(difference_ms=diff, parent_spread_ms=spread, inside_parent_spread=abs(diff) <= spread)
    else:
        result["off_cost"]["parent"] = "not measured (no --parent)"
    if not args.skip_quality:
        extra = [a for k in ("tile", "interval", "rate") if getattr(args, k) is not None for a in ("--" + k, str(getattr(args, k)))]
        result["quality"] = {}
        for seed in [int(s) for s in args.seeds.split(",")]:        # the spread between seeds is the noise a PSNR difference is read against
            args.seed = seed
            q = result["quality"][f"seed_{seed}"] = {"off": run_child(args, HERE, ["--eval-at", args.eval_at], args.timeout)}
            print(f"quality seed {seed} off:", json.dumps(q["off"]), flush=True)
            for mix in args.mix.split(","):
                r = run_child(args, HERE, ["--eval-at", args.eval_at, "--guided", "--guided-mix", mix] + extra, args.timeout)
                r["in_graph_added_ms"] = r["step_ms"] - q["off"]["step_ms"]
                q["mix_" + mix] = r
                print(f"quality seed {seed} mix {mix}:", json.dumps({k: v for k, v in r.items() if k != "ess_visited"}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
