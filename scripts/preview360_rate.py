#!/usr/bin/env python3
"""Measure the contracted-space preview on one MI355X, on the field trained on the scene of tests/scene360_fixture.py
(tests/golden/trained_field_360.npz) and the 54,208 captured rays of tests/golden/scene360_rays.npz taken as one frame:

  per lattice 128^3 / 256^3 / 512^3 over [-2, 2]^3 of the contracted space and per degree 0 / 1 / 2 (one child process each):
    bake      `bake_field(space='contracted')` once, after an untimed bake at 16^3 that warms the process up: milliseconds, bytes dense
              and sparse, stored share
    march     mipnerf_preview_360_march and mipnerf_preview_360_march_sparse, alternating, milliseconds per frame
    samples   the samples per ray inside the box (marched without the occupancy grid) and the evaluated ones (with it)
    mlp       the same rays through the MLP in the same process (`model.GraphedFrame`, what `FrameEvaluator` renders with; bf16 and fp32)
    psnr      the lattice's frame against the fp32 MLP's frame and against the photos; the MLP's against the photos

No threshold is fixed in advance: the numbers are what they are.  Every GPU step is a child process under its own time limit; the first
one that fails ends the run.

    python scripts/preview360_rate.py [--json profiles/preview360_rate.json] [--grids 128 256 512]
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
from cull360_rate import DEV, far_radius_of, golden_rays, trained_model  # noqa: E402  (one trained field for the 360 rate scripts)
from mesh_rate import window  # noqa: E402  (one timing rule for all the rate scripts)

THRESHOLD = 0.5               # the culling threshold of this field (tests/test_gpu_cull360.py FRAME_THRESHOLD)
CHUNK = 8192
WHITE = (1.0, 1.0, 1.0)       # the field was trained on a white background (scripts/make_golden_360.py)


def psnr(a, b):
    import torch
    return float(-10.0 * torch.log10(((a - b) ** 2).mean()))


def step_field(grid, degree, rounds=3):
    import numpy as np
    import torch
    from mipnerf_pl_amd import preview
    from mipnerf_pl_amd.model import GraphedFrame
    dev = torch.device(DEV)
    rays = golden_rays("scene360_rays")
    photos = torch.from_numpy(np.load(os.path.join(REPO, "tests", "golden", "scene360_rays.npz"))["rgb"]).to(dev)
    n = int(rays.origins.shape[0])
    R = far_radius_of(rays, grid)
    o, d = rays.origins.contiguous(), rays.directions.contiguous()
    near, far = rays.near.reshape(n).contiguous(), rays.far.reshape(n).contiguous()
    out = dict(grid=grid, degree=degree, rays=n, far_radius=R, threshold=THRESHOLD, dilate=1, step_scale=preview.DEFAULT_STEP_SCALE,
               t_min=preview.DEFAULT_T_MIN)
    with torch.no_grad():
        mlp = {}
        for precision in ("bf16", "fp32"):
            frame = GraphedFrame(trained_model(precision), n, CHUNK, True, dev)
            for _ in range(2):
                rgb = frame(rays)[1].reshape(n, 3).clone()
            times = []
            for _ in range(rounds):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                frame(rays)
                e1.record()
                e1.synchronize()
                times.append(e0.elapsed_time(e1))
            mlp[precision] = rgb
            out[f"mlp_{precision}_ms"] = statistics.median(times)
            out[f"mlp_{precision}_psnr_vs_photos"] = psnr(rgb, photos)
            del frame
        model = trained_model("fp32")
        # warm-up, not timed: the MLP context, the workspaces and the first launches of every kernel of the bake, on a 16^3 lattice
        preview.bake_field(model, grid=16, degree=degree, threshold=THRESHOLD, dilate=1, space="contracted", far_radius=R)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dense = preview.bake_field(model, grid=grid, degree=degree, threshold=THRESHOLD, dilate=1, space="contracted", far_radius=R)
        e1.record()
        e1.synchronize()
        out["bake_ms"] = e0.elapsed_time(e1)
        sparse = dense.to_sparse()
        out.update(dense_bytes=dense.nbytes, sparse_bytes=sparse.nbytes, stored_share=sparse.stored_share(), baked_share=dense.baked_share(),
                   occupied_fraction=dense.occupancy.occupied_fraction())
        bufs = (torch.empty(n, 3, device=dev), torch.empty(n, device=dev), torch.empty(n, device=dev))
        steps = torch.zeros(n, dtype=torch.int32, device=dev)
        times = {"dense": [], "sparse": []}
        for _ in range(rounds):                                   # alternating: every round times both storages once
            for name, field in (("dense", dense), ("sparse", sparse)):
                times[name].append(window(lambda: preview.march(field, o, d, near, far, WHITE, out=bufs, steps=steps))[0])
        for name, v in times.items():
            out[f"march_{name}_ms"] = statistics.median(v)
            out[f"march_{name}_ms_all"] = v
        preview.march(sparse, o, d, near, far, WHITE, out=bufs, steps=steps)
        rgb_sparse = bufs[0].clone()
        preview.march(dense, o, d, near, far, WHITE, out=bufs, steps=steps)
        out["sparse_equals_dense"] = bool(torch.equal(rgb_sparse.view(torch.int32), bufs[0].view(torch.int32)))
        out["evaluated_per_ray"] = float(steps.float().mean())
        out["evaluated_per_ray_max"] = int(steps.max())
        out["acc_mean"] = float(bufs[1].mean())
        out["psnr_vs_mlp_fp32"] = psnr(bufs[0], mlp["fp32"])
        out["psnr_vs_mlp_bf16"] = psnr(bufs[0], mlp["bf16"])
        out["psnr_vs_photos"] = psnr(bufs[0], photos)
        preview.march(dense, o, d, near, far, WHITE, t_min=0.0, out=bufs, steps=steps, use_occupancy=False)
        out["samples_per_ray"] = float(steps.float().mean())
        out["samples_per_ray_max"] = int(steps.max())
        out["ns_per_evaluated_sample_dense"] = out["march_dense_ms"] * 1e6 / max(out["evaluated_per_ray"] * n, 1.0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--grids", type=int, nargs="+", default=[128, 256, 512])
    ap.add_argument("--step", default=None, help="internal: run one step (GRID:DEGREE) in this process and print its JSON")
    ap.add_argument("--step_timeout", type=int, default=300)
    args = ap.parse_args()
    if args.step:
        grid, degree = (int(v) for v in args.step.split(":"))
        print("RESULT " + json.dumps(step_field(grid, degree)))
        return 0
    res = {}
    for grid in args.grids:
        for degree in (0, 1, 2):
            st = f"{grid}:{degree}"
            try:
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", st], capture_output=True, text=True,
                                   timeout=args.step_timeout)
            except subprocess.TimeoutExpired:
                print(f"{st}: time limit of {args.step_timeout} s; nothing more is started", file=sys.stderr)
                return 1
            if p.returncode != 0:
                print(f"{st}: exit status {p.returncode}; nothing more is started\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}", file=sys.stderr)
                return 1
            res[f"grid{grid}_degree{degree}"] = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
            print(st, json.dumps(res[f"grid{grid}_degree{degree}"]), flush=True)
            if args.json:                                          # after every step: a later failure keeps what was measured
                os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
                with open(args.json, "w") as f:
                    json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
