#!/usr/bin/env python3
"""Measure the sparse row table of the baked preview on one MI355X, on the golden pose at 800 x 800 with the trained field
the other rate scripts use: per lattice size (256^3, 512^3) and degree (1, 2), for a single lattice and for a 4-level pyramid,

  bytes          what a march reads, dense against sparse, and the stored share of every level,
  to_sparse      index + gather of the dense bake (wall time, the read-back of the stored count included),
  bake           wall time and peak allocated bytes of `bake_field` / `bake_pyramid`, `sparse=True` against dense,
  march          kernel time of the sparse march against the dense one IN ONE PROCESS, ALTERNATING, with the method of
                 scripts/preview_one_kernel_rate.py: HIP events around replays of the captured call, warm, the median of 21 windows of at
                 least 30 ms, every graph timed once per round; `same_bytes`: the sparse outputs equal the dense ones,
  parent         with --other_preview / --other_mip (the parent commit's two libraries): the dense march of this tree against the
                 parent's, the parent loaded twice and timed against itself -- the difference of those two medians is the spread of the day.

Every GPU step is a child process under its own time limit; the first one that fails ends the run.

    python scripts/preview_sparse_rate.py [--other_preview A/libmipnerf_preview.so --other_mip A/libmipnerf_preview_mip.so]
        [--json profiles/preview_sparse_rate.json] [--steps g256_d1,g256_d2,g512_d1,g512_d2]
"""
import argparse
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

HERE_REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LEVELS = 4
WINDOWS = 21
MIN_WINDOW_MS = 30.0


def step(grid, degree, others):
    import torch
    from mipnerf_pl_amd import _lib as L
    from mipnerf_pl_amd import preview
    from mipnerf_pl_amd.evaluate import cull_box
    from scripts.cull_rate import DEV, golden_pose_rays
    from scripts.span_rate import trained_model
    flat, frame, _, N = golden_pose_rays()
    dev = torch.device(DEV)
    model, bound = trained_model("bf16", N), cull_box([frame], grid)
    n = flat.origins.shape[0]
    o, d = flat.origins.float().contiguous(), flat.directions.float().contiguous()
    rad = flat.radii.reshape(-1).float().contiguous()
    near, far = flat.near.reshape(-1).float().contiguous(), flat.far.reshape(-1).float().contiguous()
    tail = (preview.DEFAULT_STEP_SCALE, preview.DEFAULT_T_MIN, preview.DEFAULT_MAX_STEPS)
    how = dict(grid=grid, degree=degree, lo=-bound, hi=bound)
    out = dict(grid=grid, degree=degree, levels=LEVELS, bound=bound, rays=n, precision="bf16", windows=WINDOWS, min_window_ms=MIN_WINDOW_MS)

    def wall(fn):
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats(dev)
        before = torch.cuda.memory_allocated(dev)
        t0 = time.perf_counter()
        res = fn()
        torch.cuda.synchronize()
        return res, dict(ms=1e3 * (time.perf_counter() - t0), peak_allocated_MiB=(torch.cuda.max_memory_allocated(dev) - before) / 2 ** 20)

    with torch.no_grad():
        preview.bake_pyramid(model, grid=32, levels=3, degree=degree, lo=-bound, hi=bound, sparse=True)        # warms the context and every kernel
        preview.bake_pyramid(model, grid=32, levels=3, degree=degree, lo=-bound, hi=bound).to_sparse()
        fields = {}
        for shape, bake in (("single", preview.bake_field), ("pyramid", lambda *a, **k: preview.bake_pyramid(*a, levels=LEVELS, **k))):
            dense, t_dense = wall(lambda: bake(model, **how))
            sparse, t_sparse = wall(lambda: bake(model, sparse=True, **how))
            converted, t_conv = wall(dense.to_sparse)
            levels = sparse.levels if shape == "pyramid" else [sparse]
            same_rows = all(torch.equal(a.rows.view(torch.int16), b.rows.view(torch.int16)) and torch.equal(a.table, b.table)
                            for a, b in zip(levels, converted.levels if shape == "pyramid" else [converted]))
            del converted
            out[shape] = dict(bake_dense=t_dense, bake_sparse=t_sparse, to_sparse=t_conv, sparse_bake_equals_to_sparse=same_rows,
                              MiB_dense=dense.nbytes / 2 ** 20, MiB_sparse=sparse.nbytes / 2 ** 20, sparse_over_dense=sparse.nbytes / dense.nbytes,
                              stored_share_per_level=[b.stored_share() for b in levels],
                              occupied_points_share_per_level=[float(preview.baked_points(b.occupancy).float().mean()) for b in levels],
                              dims=[list(b.dims) for b in levels])
            fields[shape] = dict(dense=dense, sparse=sparse)
        torch.cuda.empty_cache()

        again = tempfile.mkdtemp()
        builds = {"dense": (L.PREVIEW_LIB_PATH, L.PREVIEW_MIP_LIB_PATH), "sparse": None}
        if others:
            builds.update(parent=others, parent_again=(shutil.copy(others[0], again), shutil.copy(others[1], again)))
        graphs, bufs = {}, {}
        for build, paths in builds.items():
            if paths is not None:
                L.PREVIEW_LIB_PATH, L.PREVIEW_MIP_LIB_PATH = paths                      # the binding loads the path it finds at the call
            for shape in ("single", "pyramid"):
                f = fields[shape]["sparse" if build == "sparse" else "dense"]
                static = (torch.zeros(n, 3, device=dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev))
                steps = torch.zeros(n, dtype=torch.int32, device=dev)
                if shape == "pyramid":
                    call = lambda s=static, st=steps, f=f: preview.march_pyramid(f, o, d, rad, near, far, True, preview.DEFAULT_FOOTPRINT, *tail,  # noqa: E731
                                                                                 out=s, steps=st)
                else:
                    call = lambda s=static, st=steps, f=f: preview.march(f, o, d, near, far, True, *tail, out=s, steps=st)  # noqa: E731
                call()
                torch.cuda.synchronize()
                g = graphs[build, shape] = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    call()
                bufs[build, shape] = list(static) + [steps]

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
        for _ in range(WINDOWS):                                       # alternating: every round times every graph once
            for key, g in graphs.items():
                times[key].append(timed(g, reps[key]))
    for shape in ("single", "pyramid"):
        ms = {b: statistics.median(times[b, shape]) for b in builds}
        same = lambda a, b: all(torch.equal(x.view(torch.int32), y.view(torch.int32)) for x, y in zip(bufs[a, shape], bufs[b, shape]))  # noqa: E731
        m = out[shape]["march"] = dict(ms=ms, ms_min={b: min(times[b, shape]) for b in builds}, ms_max={b: max(times[b, shape]) for b in builds},
                                       replays_per_window={b: reps[b, shape] for b in builds}, sparse_over_dense=ms["sparse"] / ms["dense"],
                                       sparse_same_bytes_as_dense=same("sparse", "dense"),
                                       mean_steps_per_ray=float(bufs["dense", shape][3].sum(dtype=torch.int64)) / n)
        if others:
            spread = abs(ms["parent"] - ms["parent_again"])
            m.update(spread_ms=spread, dense_over_parent=ms["dense"] / ms["parent"], dense_within_parent_plus_spread=ms["dense"] <= ms["parent"] + spread,
                     dense_same_bytes_as_parent=same("dense", "parent"))
    shutil.rmtree(again)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--other_preview", default=None, help="libmipnerf_preview.so of the parent commit's build")
    ap.add_argument("--other_mip", default=None, help="libmipnerf_preview_mip.so of that build")
    ap.add_argument("--json", default=None)
    ap.add_argument("--step", default=None, help="internal: run one step in this process and print its JSON")
    ap.add_argument("--steps", default="g256_d1,g256_d2,g512_d1,g512_d2", help="comma-separated steps g<grid>_d<degree>")
    ap.add_argument("--step_timeout", type=int, default=400)
    args = ap.parse_args()
    if (args.other_preview is None) != (args.other_mip is None):
        ap.error("give both --other_preview and --other_mip, or neither")
    others = (os.path.abspath(args.other_preview), os.path.abspath(args.other_mip)) if args.other_preview else None
    if args.step:
        sys.path.insert(0, HERE_REPO)
        sys.path.insert(1, os.path.join(HERE_REPO, "tests"))
        grid, degree = args.step.split("_")
        print("RESULT " + json.dumps(step(int(grid[1:]), int(degree[1:]), others)))
        return 0
    res = {}
    for st in [s for s in args.steps.split(",") if s]:
        cmd = [sys.executable, os.path.abspath(__file__), "--step", st]
        if others:
            cmd += ["--other_preview", others[0], "--other_mip", others[1]]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.step_timeout, cwd=HERE_REPO)
        except subprocess.TimeoutExpired:
            print(f"{st}: time limit of {args.step_timeout} s; nothing more is started", file=sys.stderr)
            return 1
        if p.returncode != 0:
            print(f"{st}: exit status {p.returncode}; nothing more is started\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}", file=sys.stderr)
            return 1
        res[st] = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
        print(st, json.dumps({k: res[st][k]["march"] for k in ("single", "pyramid")}), flush=True)
        if args.json:                                 # kept step by step: a later step that fails loses nothing
            os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
            with open(args.json, "w") as f:
                json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
