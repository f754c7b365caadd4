#!/usr/bin/env python3
"""Measure adaptive sample counts for whole frames on one MI355X, on the golden 800 x 800 pose:

  kernels  `ops.bucket_rays` (default ladder) against `ops.compact_rays`, and `ops.gather_frame` against `ops.scatter_frame`, in the same
           process, alternating, per 640,000 rays; HIP events, windows of at least 0.3 s.  Both partitions end in a read-back and a stream
           synchronisation, which the windows include.
  frames   in one process, alternating: `CulledFrame` (the path as it was), `tighten=True`, `adaptive=True` with the default ladder, and
           `adaptive=True` with the ladder (N,) -- the tightened frame through the new route: its difference to `tighten=True` is the pure
           overhead of the route.  Per path the frame time, the fine-rgb PSNR against the scene's ground truth, the live share, the span
           share, the sample share and the bucket counts.  On the trained field's grid and on the analytic sphere grid of
           scripts/span_rate.py (a TIMING INPUT: it stands in for an object-centred Blender view; its pictures mean nothing).
  parent   `--parent DIR` (a built checkout of the parent commit): that checkout's scripts/span_rate.py frames step, for the parent's
           culled and tightened frame times on the same machine.

The expectation the frames are held against: frame time roughly proportional to live share x sample share, i.e. adaptive / tightened
close to the sample share.

Every GPU step is a child process under its own time limit; the first one that fails ends the run.

    python scripts/adaptive_rate.py [--json profiles/adaptive_rate.json] [--parent DIR]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(1, os.path.join(REPO, "tests"))
from scripts.cull_rate import DEV, RAYS, SAMPLES, golden_pose_rays  # noqa: E402
from scripts.mesh_rate import window  # noqa: E402
from scripts.span_rate import _psnr, grids, trained_model  # noqa: E402


def step_kernels(rounds=5):
    import torch
    from mipnerf_pl_amd import Rays, ops
    flat, frame, _, N = golden_pose_rays()
    assert flat.origins.shape[0] == RAYS and N == SAMPLES
    ladder = ops.sample_ladder(N)
    rows = RAYS + 64 * len(ladder)
    out = dict(rays=RAYS, samples=N, ladder=list(ladder), rounds=rounds, min_window_ms=300.0, grids={})
    for name, (occ, outside) in grids(flat, frame, N).items():
        live, first, last, near, far = ops.ray_span(occ, flat, N, outside_occupied=outside)
        src = flat._replace(near=near, far=far)
        comp_rays = Rays(*[torch.empty(rows, t.shape[1], device=DEV) for t in flat])
        comp_n = Rays(*[t[:RAYS] for t in comp_rays])
        index = torch.empty(RAYS, dtype=torch.int32, device=DEV)
        slot = torch.empty(RAYS, dtype=torch.int32, device=DEV)
        comp = [(torch.rand(rows, 3, device=DEV), torch.rand(rows, device=DEV), torch.rand(rows, device=DEV)) for _ in range(2)]
        full = [(torch.empty(RAYS, 3, device=DEV), torch.empty(RAYS, device=DEV), torch.empty(RAYS, device=DEV)) for _ in range(2)]
        count = ops.compact_rays(live, src, comp_n, index)
        counts = ops.bucket_rays(live, first, last, src, N, ladder, comp_rays, slot)
        assert sum(counts) == count
        t = dict(compact_rays=[], bucket_rays=[], scatter_frame=[], gather_frame=[])
        for _ in range(rounds):                 # alternating: every round times all four once
            t["compact_rays"].append(window(lambda: ops.compact_rays(live, src, comp_n, index))[0] * 1e3)
            t["bucket_rays"].append(window(lambda: ops.bucket_rays(live, first, last, src, N, ladder, comp_rays, slot))[0] * 1e3)
            t["scatter_frame"].append(window(lambda: ops.scatter_frame(index, count, comp, full, live, flat.near, True))[0] * 1e3)
            t["gather_frame"].append(window(lambda: ops.gather_frame(slot, comp, full, flat.near, True))[0] * 1e3)
        res = dict(outside_occupied=outside, live_share=count / float(RAYS), bucket_counts=counts)
        for k, v in t.items():
            res[k + "_us"], res[k + "_us_all"] = statistics.median(v), v
        res["bucket_over_compact"] = res["bucket_rays_us"] / res["compact_rays_us"]
        res["gather_over_scatter"] = res["gather_frame_us"] / res["scatter_frame_us"]
        out["grids"][name] = res
    return out


def step_frames(precision="bf16", rounds=5, min_window_ms=300.0):
    import numpy as np
    import torch
    from mipnerf_pl_amd.model import CulledFrame
    flat, frame, chunk, N = golden_pose_rays()
    n = flat.origins.shape[0]
    g = np.load(os.path.join(REPO, "tests", "golden", "frame_c5_800x800.npz"))
    gt = g["gt_u8"].astype(np.float32).reshape(n, 3) / 255.0
    dev = torch.device(DEV)
    model = trained_model(precision, N)
    paths = (("culled", {}), ("tightened", dict(tighten=True)), ("adaptive", dict(adaptive=True)),
             ("adaptive_top_only", dict(adaptive=True, ladder=(N,))))
    out = dict(precision=precision, rays=n, chunk=chunk, span_samples=N, rounds=rounds, min_window_ms=min_window_ms,
               ref_psnr_vs_scene=float(g["psnr_fine"]), grids={})

    def timed(fr, frames):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(frames):
            fr(flat)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / frames

    for name, (occ, outside) in grids(flat, frame, N).items():
        frames = {tag: CulledFrame(model, n, chunk, True, dev, occ, outside_occupied=outside, span_samples=N, **kw) for tag, kw in paths}
        res = {}
        with torch.no_grad():
            for tag, fr in frames.items():      # warm every shape the windows use; the second frame's pixels give the PSNR
                for _ in range(2):
                    _, fine, _ = fr(flat)
                res[tag] = dict(psnr_vs_scene=_psnr(fine.cpu().numpy(), gt), live_share=fr.live_count / float(n), span_share=fr.span_share)
                if fr.adaptive:
                    res[tag].update(sample_share=fr.sample_share, ladder=list(fr.ladder), bucket_counts=list(fr.bucket_counts),
                                    chunk_forwards=sum(-(-c // chunk) for c in fr.bucket_counts))
                else:
                    res[tag].update(chunk_forwards=-(-fr.live_count // chunk))
            torch.cuda.synchronize()
            per_window = {tag: max(1, int(min_window_ms / timed(fr, 1)) + 1) for tag, fr in frames.items()}
            times = {tag: [] for tag in frames}
            for _ in range(rounds):             # alternating: every round times every path once
                for tag, fr in frames.items():
                    times[tag].append(timed(fr, per_window[tag]))
        for tag in frames:
            res[tag].update(frame_ms=statistics.median(times[tag]), frame_ms_all=times[tag], frames_per_window=per_window[tag])
        for tag in frames:
            res[tag]["ratio_to_tightened"] = res[tag]["frame_ms"] / res["tightened"]["frame_ms"]
        res["adaptive"]["expected_ratio_to_tightened"] = res["adaptive"]["sample_share"]
        res["adaptive_top_only"]["overhead_ms"] = res["adaptive_top_only"]["frame_ms"] - res["tightened"]["frame_ms"]
        if name == "sphere_timing_input":       # the sphere is no model of this field: its pictures mean nothing
            for tag in frames:
                res[tag]["psnr_vs_scene"] = None
        out["grids"][name] = dict(outside_occupied=outside, paths=res)
        del frames
    return out


def step_parent(parent, precision, timeout):
    """the parent checkout's own span_rate frames step: its culled_128 / tightened_128 frame times per grid"""
    p = subprocess.run([sys.executable, os.path.join(parent, "scripts", "span_rate.py"), "--step", "frames_" + precision], cwd=parent,
                       capture_output=True, text=True, timeout=timeout)
    if p.returncode != 0:
        raise RuntimeError(f"parent step: exit status {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-3000:]}")
    full = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    out = dict(precision=precision, grids={})
    for name, gr in full["grids"].items():
        out["grids"][name] = {tag: {k: gr["paths"][tag][k] for k in ("frame_ms", "frame_ms_all", "psnr_vs_scene", "live_share")}
                              for tag in ("culled_128", "tightened_128")}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--step", default=None, help="internal: run one step in this process and print its JSON")
    ap.add_argument("--steps", default="kernels,frames_bf16,frames_fp32", help="comma-separated steps to run")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: adds the steps parent_bf16,parent_fp32")
    ap.add_argument("--step_timeout", type=int, default=240)
    args = ap.parse_args()
    if args.step:
        if args.step.startswith("parent_"):
            res = step_parent(args.parent, args.step[7:], args.step_timeout - 10)
        else:
            res = {"kernels": step_kernels, "frames_bf16": lambda: step_frames("bf16"),
                   "frames_fp32": lambda: step_frames("fp32", rounds=3)}[args.step]()
        print("RESULT " + json.dumps(res))
        return 0
    res = {}
    if args.json and os.path.exists(args.json):       # a run of some steps keeps the others' results
        with open(args.json) as f:
            res = json.load(f)
    steps = args.steps.split(",") + (["parent_bf16", "parent_fp32"] if args.parent and "parent" not in args.steps else [])
    for st in steps:
        cmd = [sys.executable, os.path.abspath(__file__), "--step", st, "--step_timeout", str(args.step_timeout)]
        if args.parent:
            cmd += ["--parent", os.path.abspath(args.parent)]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.step_timeout)
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
