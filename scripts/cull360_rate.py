#!/usr/bin/env python3
"""Measure empty-space skipping for the unbounded-scene model in the contracted space on one MI355X:

  sweep    the culled share of the 1000 golden rays of full360_1000x96 and of the frame below over density thresholds 0.01 .. 30 on the
           trained field's 64^3 and 128^3 grids (dilate 1): what tests/test_gpu_cull360.py took its threshold from;
  kernels  `k_ray_occupancy_360` and `k_ray_span_360` per ray beside the bounded `k_ray_occupancy` / `k_ray_span` in the same process,
           alternating, at 650,496 rays x 128 samples (the 54,208 captured rays of scene360_rays twelve times over) on a sphere grid of
           128^3 -- contracted coordinates for the 360 pair, a world box that holds every ray for the bounded pair (a TIMING INPUT: the
           bounded kernels walk the same rays linearly in t);
  frames   the 54,208 captured rays as one frame of the trained field (96 samples, chunk 8192): un-culled (the captured graph and the
           eager chunks), all-occupied (the overhead of the path), culled at the sweep's threshold, and tightened, alternating.

Every GPU step is a child process under its own time limit; the first one that fails ends the run.

    python scripts/cull360_rate.py [--json profiles/cull360_rate.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(1, os.path.join(REPO, "scripts"))
from mesh_rate import window  # noqa: E402  (one timing rule for all the rate scripts)

DEV = "cuda:0"
SAMPLES = 96                  # the golden rays' count
THRESHOLD = 0.5               # tests/test_gpu_cull360.py FRAME_THRESHOLD
THRESHOLDS = (0.01, 0.03, 0.1, 0.3, 0.5, 1.0, 2.0, 3.0, 5.0, 10.0, 30.0)


def trained_model(precision, num_samples=SAMPLES):
    import numpy as np
    import torch
    from mipnerf_pl_amd import MipNerf
    f = np.load(os.path.join(REPO, "tests", "golden", "trained_field_360.npz"))
    bias = float(np.load(os.path.join(REPO, "tests", "golden", "full360_1000x96.npz"))["density_bias"])
    m = MipNerf(num_samples=num_samples, unbounded=True, precision=precision, density_bias=bias)
    m.load_state_dict({"mlp." + k[2:]: torch.from_numpy(f[k].copy()) for k in f.files if k.startswith("p_")}, strict=True)
    return m.to(DEV).eval()


def golden_rays(name, repeat=1):
    import numpy as np
    import torch
    from mipnerf_pl_amd import Rays
    g = np.load(os.path.join(REPO, "tests", "golden", name + ".npz"))
    return Rays(*[torch.from_numpy(np.ascontiguousarray(np.tile(g["rays_" + k], (repeat, 1)))).to(DEV) for k in Rays._fields])


def far_radius_of(rays, grid):
    reach = (rays.origins.double() + rays.far.double() * rays.directions.double()).norm(dim=1).max()
    return float(reach) * (grid - 1) / (grid - 3)


def step_sweep():
    from mipnerf_pl_amd import ops
    model = trained_model("fp32")
    sets = {"full360_1000x96": golden_rays("full360_1000x96"), "scene360_rays": golden_rays("scene360_rays")}
    out = {}
    for grid in (64, 128):
        R = max(far_radius_of(r, grid) for r in sets.values())
        sigma = ops.density_grid(model, grid, -2.0, 2.0, space="contracted", far_radius=R, precision="fp32")
        rows = []
        for thr in THRESHOLDS:
            occ = ops.occupancy_grid(sigma, thr, -2.0, 2.0, dilate=1)
            occ.space = "contracted"
            row = dict(threshold=thr, occupied_fraction=occ.occupied_fraction())
            for name, rays in sets.items():
                row["culled_share_" + name] = 1.0 - float(ops.ray_occupancy(occ, rays, SAMPLES).float().mean())
            rows.append(row)
        out[f"grid{grid}"] = dict(far_radius=R, density_max=float(sigma.max()), density_median=float(sigma.median()), rows=rows)
    return out


def sphere_grid(grid, lo, hi, centre, radius, space):
    import torch
    from mipnerf_pl_amd import ops
    ax = torch.linspace(lo, hi, grid, device=DEV)
    z, y, x = torch.meshgrid(ax, ax, ax, indexing="ij")
    lat = radius - torch.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2)
    occ = ops.occupancy_grid(lat.contiguous(), 0.0, lo, hi, dilate=0)
    occ.space = space
    return occ


def step_kernels(rounds=5):
    import torch
    from mipnerf_pl_amd import ops
    N = 128
    rays = golden_rays("scene360_rays", repeat=12)
    n = int(rays.origins.shape[0])
    ends = torch.cat([rays.origins + rays.near * rays.directions, rays.origins + rays.far * rays.directions])
    bound = float(ends.abs().max()) * 1.05 + 1.0
    grids = {"contracted": sphere_grid(128, -2.0, 2.0, (0.3, -0.2, 0.25), 0.6, "contracted"),
             "world": sphere_grid(128, -bound, bound, (0.3, -0.2, 0.25), 0.6, None)}
    live = torch.empty(n, dtype=torch.uint8, device=DEV)
    bufs = (live, torch.empty(n, dtype=torch.int32, device=DEV), torch.empty(n, dtype=torch.int32, device=DEV),
            torch.empty(n, 1, device=DEV), torch.empty(n, 1, device=DEV))
    times = {f"{k}_{s}": [] for k in ("k_ray_occupancy", "k_ray_span") for s in grids}
    shares = {}
    for _ in range(rounds):                                   # alternating: every round times every kernel once
        for s, occ in grids.items():
            times[f"k_ray_occupancy_{s}"].append(window(lambda: ops.ray_occupancy(occ, rays, N, out=live))[0] * 1e3)
            shares[s] = float(live.float().mean())
            times[f"k_ray_span_{s}"].append(window(lambda: ops.ray_span(occ, rays, N, out=bufs))[0] * 1e3)
    out = dict(rays=n, samples=N, rounds=rounds, world_bound=bound, live_share=shares)
    for k, v in times.items():
        med = statistics.median(v)
        out[k] = dict(us=med, us_all=v, ns_per_ray=med * 1e3 / n)
    out["k_ray_occupancy_360_over_bounded"] = out["k_ray_occupancy_contracted"]["us"] / out["k_ray_occupancy_world"]["us"]
    out["k_ray_span_360_over_bounded"] = out["k_ray_span_contracted"]["us"] / out["k_ray_span_world"]["us"]
    return out


def step_frames(precision, rounds=5, frames_per_window=2):
    import torch
    from mipnerf_pl_amd import ops
    from mipnerf_pl_amd.model import CulledFrame, GraphedFrame
    rays = golden_rays("scene360_rays")
    n, chunk, grid = int(rays.origins.shape[0]), 8192, 128
    model = trained_model(precision)
    dev = torch.device(DEV)
    R = far_radius_of(rays, grid)
    sigma = ops.density_grid(model, grid, -2.0, 2.0, space="contracted", far_radius=R)

    def occupancy(thr):
        occ = ops.occupancy_grid(sigma, thr, -2.0, 2.0, dilate=1)
        occ.space = "contracted"
        return occ

    frames = {"graphed_frame": GraphedFrame(model, n, chunk, True, dev), "eager_frame": GraphedFrame(model, n, chunk, True, dev, capture=False),
              "all_occupied": CulledFrame(model, n, chunk, True, dev, occupancy(-1.0)),
              "culled": CulledFrame(model, n, chunk, True, dev, occupancy(THRESHOLD)),
              "tightened": CulledFrame(model, n, chunk, True, dev, occupancy(THRESHOLD), tighten=True)}

    def timed(fr):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(frames_per_window):
            fr(rays)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / frames_per_window

    times = {k: [] for k in frames}
    with torch.no_grad():
        for fr in frames.values():                            # warm every shape the windows use
            for _ in range(2):
                fr(rays)
        torch.cuda.synchronize()
        for _ in range(rounds):                               # alternating: every round times every path once
            for k, fr in frames.items():
                times[k].append(timed(fr))
    med = {k: statistics.median(v) for k, v in times.items()}
    out = dict(precision=precision, rays=n, chunk=chunk, samples=SAMPLES, grid=grid, far_radius=R, threshold=THRESHOLD, dilate=1, rounds=rounds,
               frames_per_window=frames_per_window, field_occupancy_ms=window(lambda: ops.field_occupancy(
                   model, grid=grid, threshold=THRESHOLD, dilate=1, space="contracted", far_radius=R))[0], cases={})
    for k, fr in frames.items():
        row = dict(ms=med[k], ms_all=times[k], ratio_to_graphed_frame=med[k] / med["graphed_frame"], ratio_to_eager_frame=med[k] / med["eager_frame"])
        if isinstance(fr, CulledFrame):
            row.update(live_share=fr.live_count / float(n), occupied_fraction=fr.occupancy.occupied_fraction(), span_share=fr.span_share)
        out["cases"][k] = row
    out["overhead_all_occupied_over_eager"] = med["all_occupied"] / med["eager_frame"] - 1.0
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--step", default=None, help="internal: run one step in this process and print its JSON")
    ap.add_argument("--step_timeout", type=int, default=240)
    args = ap.parse_args()
    steps = {"sweep": step_sweep, "kernels": step_kernels, "frames_bf16": lambda: step_frames("bf16"),
             "frames_fp32": lambda: step_frames("fp32", rounds=3, frames_per_window=1)}
    if args.step:
        print("RESULT " + json.dumps(steps[args.step]()))
        return 0
    res = {}
    for st in steps:
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", st], capture_output=True, text=True, timeout=args.step_timeout)
        except subprocess.TimeoutExpired:
            print(f"{st}: time limit of {args.step_timeout} s; nothing more is started", file=sys.stderr)
            return 1
        if p.returncode != 0:
            print(f"{st}: exit status {p.returncode}; nothing more is started\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}", file=sys.stderr)
            return 1
        res[st] = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
        print(st, json.dumps(res[st]), flush=True)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
