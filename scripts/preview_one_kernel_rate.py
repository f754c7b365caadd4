#!/usr/bin/env python3
"""A/B of two builds of the preview libraries on one MI355X: the tree's own libmipnerf_preview.so and
libmipnerf_preview_mip.so against the pair of another build (the parent commit's, built from a copy of that commit), in ONE process, with
the method of scripts/preview_mip_rate.py: HIP events around replays of the captured call, warm, the median of 21 windows of at least
30 ms, every kernel timed once per round, so the builds alternate window by window.  The other build is loaded twice, from two copies of
its files, and timed against itself: the difference of those two medians is the spread of the day.

Frames: the golden pose at 800 x 800, 256^3 points, the trained field the other rate scripts use --
  plain_d1, plain_d2    mipnerf_preview_march at degree 1 and 2,
  mip4                  mipnerf_preview_mip_march over 4 levels at degree 1,
in the default box (`cull_box`) and, step `frames_bound1.5`, over [-1.5, 1.5]^3.

Every GPU step is a child process under its own time limit; the first one that fails ends the run.

    python scripts/preview_one_kernel_rate.py --other_preview A/libmipnerf_preview.so --other_mip A/libmipnerf_preview_mip.so
        [--json profiles/preview_one_kernel_rate.json] [--steps frames,frames_bound1.5]
"""
import argparse
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile

HERE_REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAMES = ("plain_d1", "plain_d2", "mip4")


def step_frames(other_preview, other_mip, bound=None):
    import torch
    from mipnerf_pl_amd import _lib as L
    from mipnerf_pl_amd import preview
    from scripts.cull_rate import golden_pose_rays
    from scripts.preview_mip_rate import GRID, LEVELS, MIN_WINDOW_MS, WINDOWS, _model_and_bound
    model, bound, _, _, dev = _model_and_bound(bound)
    flat = golden_pose_rays()[0]
    n = flat.origins.shape[0]
    o, d = flat.origins.float().contiguous(), flat.directions.float().contiguous()
    rad = flat.radii.reshape(-1).float().contiguous()
    near, far = flat.near.reshape(-1).float().contiguous(), flat.far.reshape(-1).float().contiguous()
    tail = (preview.DEFAULT_STEP_SCALE, preview.DEFAULT_T_MIN, preview.DEFAULT_MAX_STEPS)
    again = tempfile.mkdtemp()
    builds = {"new": (L.PREVIEW_LIB_PATH, L.PREVIEW_MIP_LIB_PATH), "other": (other_preview, other_mip),
              "other_again": (shutil.copy(other_preview, again), shutil.copy(other_mip, again))}
    out = dict(grid=GRID, levels=LEVELS, bound=bound, rays=n, precision="bf16", windows=WINDOWS, min_window_ms=MIN_WINDOW_MS, frames={})
    with torch.no_grad():
        pyr = preview.bake_pyramid(model, grid=GRID, levels=LEVELS, degree=1, lo=-bound, hi=bound)
        fields = {"plain_d1": pyr.levels[0], "plain_d2": preview.bake_field(model, grid=GRID, degree=2, lo=-bound, hi=bound), "mip4": pyr}
        graphs, bufs = {}, {}
        for build, paths in builds.items():
            L.PREVIEW_LIB_PATH, L.PREVIEW_MIP_LIB_PATH = paths                          # the binding loads the path it finds at the call
            for frame in FRAMES:
                static = (torch.zeros(n, 3, device=dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev))
                steps = torch.zeros(n, dtype=torch.int32, device=dev)
                if frame == "mip4":
                    call = lambda s=static, st=steps: preview.march_pyramid(pyr, o, d, rad, near, far, True, preview.DEFAULT_FOOTPRINT, *tail,  # noqa: E731
                                                                            out=s, steps=st)
                else:
                    call = lambda s=static, st=steps, f=fields[frame]: preview.march(f, o, d, near, far, True, *tail, out=s, steps=st)  # noqa: E731
                call()
                torch.cuda.synchronize()
                g = graphs[build, frame] = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    call()
                bufs[build, frame] = list(static) + [steps]

        def timed(graph, reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                graph.replay()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) / reps
        reps = {}
        for key, g in graphs.items():
            for _ in range(5):
                g.replay()
            torch.cuda.synchronize()
            reps[key] = max(1, int(MIN_WINDOW_MS / max(timed(g, 3), 1e-3)) + 1)
        times = {key: [] for key in graphs}
        for _ in range(WINDOWS):                                       # alternating: every round times every kernel of every build once
            for key, g in graphs.items():
                times[key].append(timed(g, reps[key]))
    for frame in FRAMES:
        ms = {b: statistics.median(times[b, frame]) for b in builds}
        spread = abs(ms["other"] - ms["other_again"])
        out["frames"][frame] = dict(
            ms=ms, ms_min={b: min(times[b, frame]) for b in builds}, ms_max={b: max(times[b, frame]) for b in builds},
            replays_per_window={b: reps[b, frame] for b in builds}, spread_ms=spread, new_over_other=ms["new"] / ms["other"],
            new_within_other_plus_spread=ms["new"] <= ms["other"] + spread,
            mean_steps_per_ray=float(bufs["new", frame][3].sum(dtype=torch.int64)) / n,
            same_bytes_as_other=all(torch.equal(a.view(torch.int32), b.view(torch.int32))
                                    for a, b in zip(bufs["new", frame], bufs["other", frame])))
    shutil.rmtree(again)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--other_preview", required=True, help="libmipnerf_preview.so of the build to compare with")
    ap.add_argument("--other_mip", required=True, help="libmipnerf_preview_mip.so of that build")
    ap.add_argument("--json", default=None)
    ap.add_argument("--step", default=None, help="internal: run one step in this process and print its JSON")
    ap.add_argument("--steps", default="frames,frames_bound1.5", help="comma-separated steps to run")
    ap.add_argument("--step_timeout", type=int, default=300)
    args = ap.parse_args()
    others = (os.path.abspath(args.other_preview), os.path.abspath(args.other_mip))
    if args.step:
        sys.path.insert(0, HERE_REPO)
        sys.path.insert(1, os.path.join(HERE_REPO, "tests"))
        print("RESULT " + json.dumps(step_frames(*others, float(args.step.partition("_bound")[2]) if "_bound" in args.step else None)))
        return 0
    res = {}
    for st in [s for s in args.steps.split(",") if s]:
        cmd = [sys.executable, os.path.abspath(__file__), "--other_preview", others[0], "--other_mip", others[1], "--step", st]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.step_timeout, cwd=HERE_REPO)
        except subprocess.TimeoutExpired:
            print(f"{st}: time limit of {args.step_timeout} s; nothing more is started", file=sys.stderr)
            return 1
        if p.returncode != 0:
            print(f"{st}: exit status {p.returncode}; nothing more is started\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}", file=sys.stderr)
            return 1
        res[st] = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
        print(st, json.dumps(res[st]["frames"]), flush=True)
        if args.json:                                 # kept step by step: a later step that fails loses nothing
            os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
            with open(args.json, "w") as f:
                json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
