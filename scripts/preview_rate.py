#!/usr/bin/env python3
"""Measure the baked-lattice preview renderer on one MI355X, on the golden 800 x 800 pose with the trained field the other
rate scripts use:

  parents   the MLP paths of the parent commit in the same run: the plain graphed frame and `--cull_adaptive --proposal_grid` (256^3),
            frame time and fine-rgb PSNR against the scene's ground truth (the helpers of scripts/proposal_rate.py).
  grid_N    N = 128, 256, 512: per degree 0 / 1 / 2 the bake (ms, MiB, baked share of the points), and per step_scale 0.5 / 1 the frame:
            ms with HIP events around replays of the captured march (warm; the median of 21 windows of at least 30 ms), mean evaluated
            samples per ray, PSNR against the scene and against the MLP's plain frame rendered in the same process.  Next to it the bytes
            the kernel asks for per evaluated sample (8 corner rows) against a device copy measured in the same process: what the frame
            would cost if every one of those bytes came from memory, and if the lattice were read exactly once.

Every GPU step is a child process under its own time limit; the first one that fails ends the run.

    python scripts/preview_rate.py [--json profiles/preview_rate.json] [--steps parents,grid_128,grid_256,grid_512]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE_REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRIDS = (128, 256, 512)
DEGREES = (0, 1, 2)
STEP_SCALES = (0.5, 1.0)
WINDOWS = 21
MIN_WINDOW_MS = 30.0


def step_parents(rounds=5, min_window_ms=300.0):
    from mipnerf_pl_amd import ops
    from mipnerf_pl_amd.evaluate import cull_box
    from scripts.proposal_rate import _frame, _measure, _setup
    flat, frame, chunk, N, n, gt, ref, dev, model, occ, outside = _setup("bf16")
    bound = cull_box([frame], 256)
    prop = ops.field_proposal(model, grid=256, lo=-bound, hi=bound)
    frames = {"graphed": _frame(model, n, chunk, dev, occ, outside, N, None),
              "cull_adaptive_proposal256": _frame(model, n, chunk, dev, occ, outside, N, dict(adaptive=True), prop)}
    return dict(precision="bf16", rays=n, chunk=chunk, samples=N, rounds=rounds, min_window_ms=min_window_ms, ref_psnr_vs_scene=ref,
                rows=_measure(frames, flat, gt, rounds, min_window_ms))


def _replay_ms(graph):
    """median over WINDOWS event windows of at least MIN_WINDOW_MS of replays, after a warm-up"""
    import torch
    for _ in range(5):
        graph.replay()
    torch.cuda.synchronize()

    def timed(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            graph.replay()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / reps
    reps = max(1, int(MIN_WINDOW_MS / max(timed(3), 1e-3)) + 1)
    all_ms = [timed(reps) for _ in range(WINDOWS)]
    return statistics.median(all_ms), all_ms, reps


def step_grid(size):
    import time
    import numpy as np
    import torch
    from mipnerf_pl_amd import preview
    from mipnerf_pl_amd.evaluate import cull_box
    from scripts.mesh_rate import window
    from scripts.proposal_rate import _frame, _setup
    from scripts.span_rate import _psnr
    flat, frame, chunk, N, n, gt, ref, dev, model, occ, outside = _setup("bf16")
    with torch.no_grad():
        mlp = _frame(model, n, chunk, dev, occ, outside, N, None)
        for _ in range(2):
            _, fine, _ = mlp(flat)
        mlp_rgb = fine.cpu().numpy().copy()
        del mlp
        src = torch.rand(1 << 28, device=dev)                       # 1 GiB read + 1 GiB written per copy
        dst = torch.empty_like(src)
        copy_ms = window(lambda: dst.copy_(src))[0]
        copy_gbps = 2 * src.numel() * 4 / copy_ms / 1e6
        del src, dst
        bound = cull_box([frame], size)
        out = dict(grid=size, bound=bound, precision="bf16", rays=n, windows=WINDOWS, min_window_ms=MIN_WINDOW_MS, mlp_psnr_vs_scene=_psnr(mlp_rgb, gt),
                   ref_psnr_vs_scene=ref, copy_GBps=copy_gbps, degrees={})
        preview.bake_field(model, grid=32, degree=1, lo=-bound, hi=bound)          # warms the context and every kernel of the bake
        o, d = flat.origins.float().contiguous(), flat.directions.float().contiguous()
        near, far = flat.near.reshape(-1).float().contiguous(), flat.far.reshape(-1).float().contiguous()
        for degree in DEGREES:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            baked = preview.bake_field(model, grid=size, degree=degree, lo=-bound, hi=bound)
            torch.cuda.synchronize()
            row_bytes = 2 * preview.ROW_HALVES[degree]
            res = dict(bake_ms=1e3 * (time.perf_counter() - t0), MiB=baked.nbytes / 2 ** 20, baked_share=baked.baked_share(),
                       occupied_share=baked.occupancy.occupied_fraction(), row_bytes=row_bytes, steps={})
            static = (torch.zeros(n, 3, device=dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev))
            steps = torch.zeros(n, dtype=torch.int32, device=dev)
            for ss in STEP_SCALES:
                args = (baked, o, d, near, far, True, ss, preview.DEFAULT_T_MIN, preview.DEFAULT_MAX_STEPS)
                preview.march(*args, out=static, steps=steps)
                torch.cuda.synchronize()
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    preview.march(*args, out=static, steps=steps)
                ms, all_ms, reps = _replay_ms(g)
                rgb = static[0].cpu().numpy()
                evaluated = int(steps.sum(dtype=torch.int64))
                asked = evaluated * 8 * row_bytes
                res["steps"][str(ss)] = dict(
                    frame_ms=ms, frame_ms_all=all_ms, replays_per_window=reps, mean_steps_per_ray=evaluated / n,
                    rays_with_samples=float((steps > 0).float().mean()), psnr_vs_scene=_psnr(rgb, gt), psnr_vs_mlp=_psnr(rgb, mlp_rgb),
                    bytes_asked_per_sample=8 * row_bytes, bytes_asked=asked, asked_GBps=asked / ms / 1e6,
                    ms_if_every_asked_byte_came_from_memory=asked / copy_gbps / 1e6,
                    ms_if_the_baked_rows_were_read_once=baked.baked_share() * size ** 3 * row_bytes / (copy_gbps / 2) / 1e6)
                del g
            out["degrees"][str(degree)] = res
            del baked, static, steps
            torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--step", default=None, help="internal: run one step in this process and print its JSON")
    ap.add_argument("--steps", default="parents," + ",".join(f"grid_{g}" for g in GRIDS), help="comma-separated steps to run")
    ap.add_argument("--step_timeout", type=int, default=300)
    args = ap.parse_args()
    if args.step:
        sys.path.insert(0, HERE_REPO)
        sys.path.insert(1, os.path.join(HERE_REPO, "tests"))
        res = step_parents() if args.step == "parents" else step_grid(int(args.step.partition("_")[2]))
        print("RESULT " + json.dumps(res))
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
        print(st, json.dumps(res[st])[:2000], flush=True)
        if args.json:                                 # kept step by step: a later step that fails loses nothing
            os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
            with open(args.json, "w") as f:
                json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
