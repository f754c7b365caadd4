#!/usr/bin/env python3
"""Measure the empty-space skipping of whole frames on one MI355X:

  grid     the density lattice and the occupancy bits at 128^3 (bf16 field, dilate 1);
  kernels  classify, compact and scatter at 640,000 rays x 128 samples, per kernel from `rocprofv3 --kernel-trace --stats` in a run of
           its own;
  frames   the golden 800 x 800 pose through `GraphedFrame` (the captured graph: the baseline) and through `CulledFrame`, in one process,
           alternating, with (a) an all-occupied grid: the overhead of the path, (b) the trained field's grid at the whole-frame test's
           setting, (c) an analytic sphere grid sized so that 30-40 % of the rays are live.  (c) is a TIMING INPUT: it stands in for a
           Blender view, which this repository has no data for; the field it renders is still the trained one.

Every GPU step is a child process under its own time limit; the first one that fails ends the run.

    python scripts/cull_rate.py [--json profiles/cull_rate.json]        (also writes cull_kernel_stats.csv next to the JSON)
"""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(1, os.path.join(REPO, "tests"))
from scripts.mesh_rate import trained_model, window  # noqa: E402

RAYS, SAMPLES = 640000, 128
DEV = "cuda:0"


def golden_pose_rays():
    import numpy as np
    import torch
    from mipnerf_pl_amd import Rays
    from mipnerf_pl_amd.datasets import RenderGen
    g = np.load(os.path.join(REPO, "tests", "golden", "frame_c5_800x800.npz"))
    size = int(g["cfg_size"])
    rays = RenderGen(float(g["focal"]), [size, size], scales=1, device=torch.device(DEV))[int(g["cfg_pose"])]
    return Rays(*[t.reshape(size * size, -1).contiguous() for t in rays]), Rays(*rays), int(g["cfg_chunk"]), int(g["cfg_num_samples"])


def sphere_occupancy(radius, bound, grid=128):
    import torch
    from mipnerf_pl_amd import ops
    ax = torch.linspace(-bound, bound, grid, device=DEV)
    z, y, x = torch.meshgrid(ax, ax, ax, indexing="ij")
    return ops.occupancy_grid((radius - torch.sqrt(x * x + y * y + z * z)).contiguous(), 0.0, -bound, bound, dilate=0)


def step_grid():
    from mipnerf_pl_amd import ops
    model = trained_model("bf16")
    box = (-2.0, 2.0)
    lat_ms, _, _ = window(lambda: ops.density_grid(model, 128, *box))
    sigma = ops.density_grid(model, 128, *box)
    out = dict(grid=128, precision="bf16", lattice_ms=lat_ms)
    for d in (0, 1, 3):
        out[f"bits_dilate{d}_ms"], _, _ = window(lambda: ops.occupancy_grid(sigma, 0.03, *box, dilate=d))
    out["field_occupancy_ms"], _, _ = window(lambda: ops.field_occupancy(model, grid=128, lo=box[0], hi=box[1], threshold=0.03, dilate=1))
    out["occupied_fraction_thr0.03_dilate1"] = ops.occupancy_grid(sigma, 0.03, *box, dilate=1).occupied_fraction()
    return out


def step_kernels_target():
    """what the profiler watches: 20 rounds of classify + compact + scatter on the golden pose's 640,000 rays, 35 % live"""
    import torch
    from mipnerf_pl_amd import Rays, ops
    from mipnerf_pl_amd.evaluate import cull_box
    flat, frame, _, N = golden_pose_rays()
    assert flat.origins.shape[0] == RAYS and N == SAMPLES
    bound = cull_box([frame], 128)
    occ, share = sized_sphere(flat, bound, N)
    out_rays = Rays(*[torch.empty_like(t) for t in flat])
    index = torch.empty(RAYS, dtype=torch.int32, device=DEV)
    comp = [(torch.rand(RAYS, 3, device=DEV), torch.rand(RAYS, device=DEV), torch.rand(RAYS, device=DEV)) for _ in range(2)]
    full = [(torch.empty(RAYS, 3, device=DEV), torch.empty(RAYS, device=DEV), torch.empty(RAYS, device=DEV)) for _ in range(2)]
    for _ in range(20):
        live = ops.ray_occupancy(occ, flat, N)
        count = ops.compact_rays(live, flat, out_rays, index)
        ops.scatter_frame(index, count, comp, full, live, flat.near, True)
    torch.cuda.synchronize()
    return dict(live_share=share)


def sized_sphere(flat, bound, N, lo_share=0.30, hi_share=0.40):
    """an analytic sphere grid (128^3 over +-bound) whose radius leaves 30-40 % of the rays live: bisection on the radius"""
    from mipnerf_pl_amd import ops
    a, b = 0.05, bound
    for _ in range(30):
        r = 0.5 * (a + b)
        occ = sphere_occupancy(r, bound)
        share = float(ops.ray_occupancy(occ, flat, N).float().mean())
        if lo_share <= share <= hi_share:
            return occ, share
        a, b = (r, b) if share < lo_share else (a, r)
    raise RuntimeError(f"no sphere radius gives a live share in [{lo_share}, {hi_share}] (last {share})")


def step_kernels(stats_copy, timeout):
    """the profiler writes into a temporary directory; its per-kernel table is kept as `stats_copy` (None: not kept)"""
    import shutil
    import tempfile
    with tempfile.TemporaryDirectory(prefix="cull_rate_prof_") as prof:
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", prof, "-o", "cull", "--", sys.executable,
               os.path.abspath(__file__), "--step", "kernels_target"]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout)
        if p.returncode != 0:
            raise RuntimeError(f"rocprofv3 exit status {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-3000:]}")
        files = glob.glob(os.path.join(prof, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            raise RuntimeError("the profiler wrote no kernel_stats.csv")
        rows = {}
        with open(files[0]) as f:
            for r in csv.DictReader(f):
                for key in ("k_ray_occupancy", "k_compact_count", "k_compact_scan_blocks", "k_compact_gather", "k_scatter_frame"):
                    if key in r["Name"]:
                        rows[key] = dict(calls=int(r["Calls"]), average_us=float(r["AverageNs"]) / 1e3, min_us=float(r["MinNs"]) / 1e3,
                                         max_us=float(r["MaxNs"]) / 1e3)
        if stats_copy:
            shutil.copyfile(files[0], stats_copy)
    target = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    return dict(rays=RAYS, samples=SAMPLES, live_share=target["live_share"], kernels=rows,
                sum_average_us=sum(v["average_us"] for v in rows.values()),
                stats_file=os.path.basename(stats_copy) if stats_copy else None)


def step_frames(precision="bf16", rounds=5, frames_per_window=4):
    import torch
    from mipnerf_pl_amd import ops
    from mipnerf_pl_amd.evaluate import cull_box
    from mipnerf_pl_amd.model import CulledFrame, GraphedFrame
    flat, frame, chunk, N = golden_pose_rays()
    n = flat.origins.shape[0]
    model = trained_model(precision)
    assert model.num_samples == N
    dev = torch.device(DEV)
    bound = cull_box([frame], 128)
    sigma = ops.density_grid(model, 64, -2.0, 2.0)
    sphere, _ = sized_sphere(flat, bound, N)
    cases = {
        "all_occupied": (ops.occupancy_grid(sigma, -1.0, -2.0, 2.0, dilate=0), True),
        "trained_thr0.03_dilate0_64_pm2": (ops.occupancy_grid(sigma, 0.03, -2.0, 2.0, dilate=0), False),
        "sphere_timing_input": (sphere, True),
    }
    base = GraphedFrame(model, n, chunk, True, dev)
    eager = GraphedFrame(model, n, chunk, True, dev, capture=False)
    culled = {k: CulledFrame(model, n, chunk, True, dev, occ, outside_occupied=outside) for k, (occ, outside) in cases.items()}

    def timed(fr):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(frames_per_window):
            fr(flat)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / frames_per_window

    with torch.no_grad():
        for fr in [base, eager] + list(culled.values()):      # warm every shape the windows use
            for _ in range(2):
                fr(flat)
        torch.cuda.synchronize()
        times = {k: [] for k in ["graphed_frame", "eager_frame"] + list(culled)}
        for _ in range(rounds):                               # alternating: every round times every path once
            times["graphed_frame"].append(timed(base))
            times["eager_frame"].append(timed(eager))
            for k, fr in culled.items():
                times[k].append(timed(fr))
    med = {k: statistics.median(v) for k, v in times.items()}
    out = dict(precision=precision, rays=n, chunk=chunk, samples=N, rounds=rounds, frames_per_window=frames_per_window,
               baseline_ms=med["graphed_frame"], baseline_ms_all=times["graphed_frame"], eager_chunks_ms=med["eager_frame"],
               eager_chunks_ms_all=times["eager_frame"], baseline_ms_per_5pct_of_rays=0.05 * med["graphed_frame"], cases={})
    for k, fr in culled.items():
        out["cases"][k] = dict(live_share=fr.live_count / float(n), culled_ms=med[k], culled_ms_all=times[k],
                               ratio_to_baseline=med[k] / med["graphed_frame"], ms_over_baseline=med[k] - med["graphed_frame"],
                               occupied_fraction=fr.occupancy.occupied_fraction(), outside_occupied=fr.outside_occupied)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--step", default=None, help="internal: run one step in this process and print its JSON")
    ap.add_argument("--step_timeout", type=int, default=240)
    args = ap.parse_args()
    if args.step:
        res = {"grid": step_grid, "kernels_target": step_kernels_target, "frames_bf16": lambda: step_frames("bf16"),
               "frames_fp32": lambda: step_frames("fp32", rounds=3, frames_per_window=2)}[args.step]()
        print("RESULT " + json.dumps(res))
        return 0
    res = {}
    stats_copy = None
    if args.json:           # the profiler's per-kernel table goes next to the JSON
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        stats_copy = os.path.join(os.path.dirname(os.path.abspath(args.json)), "cull_kernel_stats.csv")
    for st in ("grid", "kernels", "frames_bf16", "frames_fp32"):
        try:
            if st == "kernels":
                r = step_kernels(stats_copy, args.step_timeout)
            else:
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", st], capture_output=True, text=True, timeout=args.step_timeout)
                if p.returncode != 0:
                    print(f"{st}: exit status {p.returncode}; nothing more is started\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}", file=sys.stderr)
                    return 1
                r = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
        except subprocess.TimeoutExpired:
            print(f"{st}: time limit of {args.step_timeout} s; nothing more is started", file=sys.stderr)
            return 1
        except RuntimeError as e:
            print(f"{st}: {e}; nothing more is started", file=sys.stderr)
            return 1
        res[st] = r
        print(st, json.dumps(r), flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
