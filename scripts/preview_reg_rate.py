#!/usr/bin/env python3
"""Measure the regulariser of the baked lattice's tuning on one MI355X, on the scene, the trained field and the helpers of
scripts/preview_tune_rate.py (the golden pose at 800 x 800, tests/golden/trained_field.npz, bf16 bake, the same HIP-event windows):

  reg_g<grid>_d<degree>    k_preview_reg_grad on the master rows of the bake, with the bake's point mask and without: kernel time, beside
                 k_preview_tune_adam on the same arrays and beside a device copy of the bytes the kernel must move (master once at every
                 point, grad read and written at the masked points; used entries only), and the ratios,
  step_g<grid>_d<degree>   wall time of `TuneState.step` on the batch of scripts/preview_tune_rate.py without and with the regulariser, in
                 one process, alternating; the figure profiles/preview_tune_rate.json holds for the step before the regulariser existed
                 is copied beside them.

Every GPU step is a child process under its own time limit; the first one that fails ends the run.

    python scripts/preview_reg_rate.py [--json profiles/preview_reg_rate.json] [--steps reg_g256_d0,...]
"""
import argparse
import json
import os
import subprocess
import sys
import time

HERE_REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = "reg_g256_d0,reg_g256_d1,reg_g256_d2,step_g256_d1"
WEIGHTS = (0.1, 0.1, 0.01)          # per masked point; the time does not depend on their size, only on which are non-zero
EPS = 1e-4


def step_reg(grid, degree):
    import torch
    from mipnerf_pl_amd import preview
    from scripts.preview_tune_rate import _scene, _window
    dev, model, baked, flat = _scene(grid, degree)
    state = preview.TuneState(baked)
    W = baked.rows.shape[-1]
    n = baked.rows.numel() // W
    used = 1 + 3 * (degree + 1) ** 2
    masked = int(state.mask.sum())
    args = (baked.dims, baked.lo, baked.hi, degree, state.grad, *WEIGHTS, EPS)
    adam = (0.0, 0.0, 0.9, 0.999, 1e-8, 10.0, 1000.0)
    out = dict(grid=grid, degree=degree, points=n, masked_points=masked, masked_in_share=masked / n, weights=WEIGHTS)
    for name, mask, count in (("masked", state.mask, masked), ("unmasked", None, n)):
        must = n * used * 4 + count * used * 4 * 2                # master once at every point (an upper bound with a mask), grad twice
        src = torch.empty(must // 2, dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        t_reg = _window(lambda: preview.tune_regularise(state.master, mask, *args, count))
        t_adam = _window(lambda: preview.tune_adam(state.master, state.m, state.v, state.grad, baked.rows, degree, mask, *adam))
        t_copy = _window(lambda: dst.copy_(src))
        state.grad.zero_()
        out[name] = dict(bytes_must_move=must, reg=t_reg, adam_same_arrays=t_adam, device_copy_same_bytes=t_copy,
                         reg_over_copy=t_reg["ms"] / t_copy["ms"], reg_over_adam=t_reg["ms"] / t_adam["ms"],
                         reg_GB_per_s=must / (t_reg["ms"] * 1e-3) / 1e9)
        del src, dst
    only = {}
    for key, w in (("tv_sigma_only", (WEIGHTS[0], 0.0, 0.0)), ("tv_colour_only", (0.0, WEIGHTS[1], 0.0)), ("sh_decay_only", (0.0, 0.0, WEIGHTS[2]))):
        if degree == 0 and key == "sh_decay_only":
            continue                                                # no entry decays at degree 0: the kernel returns at once
        only[key] = _window(lambda: preview.tune_regularise(state.master, state.mask, baked.dims, baked.lo, baked.hi, degree, state.grad, *w,
                                                            EPS, masked))["ms"]
    out["masked_one_weight_ms"] = only
    return out


def step_step(grid, degree):
    import torch
    from mipnerf_pl_amd import preview
    from scripts.preview_tune_rate import BATCH, _batch, _scene
    dev, model, baked, flat = _scene(grid, degree)
    rays, target = _batch(model, flat, dev)
    plain = preview.TuneState(baked, lr_sigma=0.0, lr_colour=0.0)          # timing only: the lattice stays what it is
    reg = preview.TuneState(baked, lr_sigma=0.0, lr_colour=0.0, tv_sigma=WEIGHTS[0], tv_colour=WEIGHTS[1], sh_decay=WEIGHTS[2], tv_eps=EPS)
    times = dict(plain=[], regularised=[])
    for state in (plain, reg):
        for _ in range(3):
            state.step(rays, target, True)
    for _ in range(5):                                                     # alternating windows of 20 steps
        for name, state in (("plain", plain), ("regularised", reg)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(20):
                state.step(rays, target, True)
            torch.cuda.synchronize()
            times[name].append(1e3 * (time.perf_counter() - t0) / 20)
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    out = dict(grid=grid, degree=degree, rays=BATCH, tuned_points=reg.n_points, ms_per_step_zero_weights=med(times["plain"]),
               ms_per_step_regularised=med(times["regularised"]), windows_zero_weights=times["plain"], windows_regularised=times["regularised"])
    before = os.path.join(HERE_REPO, "profiles", "preview_tune_rate.json")
    if os.path.exists(before):
        with open(before) as f:
            out["ms_per_step_before_the_regulariser_existed"] = json.load(f).get(f"step_g{grid}_d{degree}", {}).get("ms_per_step")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--step", default=None, help="internal: run one step in this process and print its JSON")
    ap.add_argument("--steps", default=STEPS, help="comma-separated steps")
    ap.add_argument("--step_timeout", type=int, default=300)
    args = ap.parse_args()
    if args.step:
        sys.path.insert(0, HERE_REPO)
        sys.path.insert(1, os.path.join(HERE_REPO, "tests"))
        kind, *rest = args.step.split("_")
        nums = [int(r[1:]) for r in rest]
        print("RESULT " + json.dumps(dict(reg=step_reg, step=step_step)[kind](*nums)))
        return 0
    res = {}
    if args.json and os.path.exists(args.json):       # a run of some steps keeps the others' results
        with open(args.json) as f:
            res = json.load(f)
    for st in [s for s in args.steps.split(",") if s]:
        cmd = [sys.executable, os.path.abspath(__file__), "--step", st]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.step_timeout, cwd=HERE_REPO)
        except subprocess.TimeoutExpired:
            print(f"{st}: time limit of {args.step_timeout} s; nothing more is started", file=sys.stderr)
            return 1
        if p.returncode != 0:
            print(f"{st}: exit status {p.returncode}; nothing more is started\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}", file=sys.stderr)
            return 1
        res[st] = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
        print(st, json.dumps(res[st]), flush=True)
        if args.json:                                 # kept step by step: a later step that fails loses nothing
            os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
            with open(args.json, "w") as f:
                json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
