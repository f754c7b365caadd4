#!/usr/bin/env python3
"""Measure the tightening of culled rays to their occupied span on one MI355X:

  kernels  `k_ray_span` against the unchanged `k_ray_occupancy` in the same process, alternating, at 640,000 rays x 128 samples (the
           golden pose), on the trained field's grid (whole-frame test's setting) and on an analytic sphere grid sized so that 30-40 % of
           the rays are live; HIP events, windows of at least 0.3 s; the mean span share of both grids.  The sphere grid is a TIMING
           INPUT, as in scripts/cull_rate.py: it stands in for an object-centred Blender view.
  frames   the golden 800 x 800 pose, in one process, alternating: `CulledFrame` (the path as it was), `tighten=True` at 128 samples,
           `tighten=True` rendered with 64 samples (span_samples stays 128), and untightened at 64 samples; per path the frame time
           and the fine-rgb PSNR against the scene's ground truth.  Trained grid; the times also on the sphere grid.

Every GPU step is a child process under its own time limit; the first one that fails ends the run.

    python scripts/span_rate.py [--json profiles/span_rate.json]
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
from scripts.cull_rate import DEV, RAYS, SAMPLES, golden_pose_rays, sized_sphere  # noqa: E402
from scripts.mesh_rate import window  # noqa: E402


def trained_model(precision, num_samples=SAMPLES):
    import numpy as np
    import torch
    from mipnerf_pl_amd import MipNerf
    f = np.load(os.path.join(REPO, "tests", "golden", "trained_field.npz"))
    m = MipNerf(num_samples=num_samples, precision=precision)
    m.load_state_dict({"mlp." + k[2:]: torch.from_numpy(f[k].copy()) for k in f.files if k.startswith("p_")}, strict=True)
    return m.to(DEV).eval()


def grids(flat, frame, N):
    """{name: (occupancy, outside_occupied)}: the trained field's grid of the whole-frame test and the sphere timing input"""
    from mipnerf_pl_amd import ops
    from mipnerf_pl_amd.evaluate import cull_box
    sigma = ops.density_grid(trained_model("fp32"), 64, -2.0, 2.0)
    sphere, _ = sized_sphere(flat, cull_box([frame], 128), N)
    return {"trained_thr0.03_dilate0_64_pm2": (ops.occupancy_grid(sigma, 0.03, -2.0, 2.0, dilate=0), False),
            "sphere_timing_input": (sphere, True)}


def span_share(first, last, N):
    live = last >= first
    return float((last[live] - first[live] + 1).double().mean().item() / N) if bool(live.any()) else float("nan")


def step_kernels(rounds=5):
    import torch
    from mipnerf_pl_amd import ops
    flat, frame, _, N = golden_pose_rays()
    assert flat.origins.shape[0] == RAYS and N == SAMPLES
    out = dict(rays=RAYS, samples=N, rounds=rounds, min_window_ms=300.0, grids={})
    for name, (occ, outside) in grids(flat, frame, N).items():
        live = torch.empty(RAYS, dtype=torch.uint8, device=DEV)
        bufs = (torch.empty(RAYS, dtype=torch.uint8, device=DEV), torch.empty(RAYS, dtype=torch.int32, device=DEV),
                torch.empty(RAYS, dtype=torch.int32, device=DEV), torch.empty(RAYS, 1, device=DEV), torch.empty(RAYS, 1, device=DEV))
        t_occ, t_span = [], []
        for _ in range(rounds):                 # alternating: every round times both kernels once
            t_occ.append(window(lambda: ops.ray_occupancy(occ, flat, N, outside_occupied=outside, out=live))[0] * 1e3)
            t_span.append(window(lambda: ops.ray_span(occ, flat, N, outside_occupied=outside, out=bufs))[0] * 1e3)
        assert torch.equal(live, bufs[0])
        a, b = statistics.median(t_occ), statistics.median(t_span)
        out["grids"][name] = dict(outside_occupied=outside, live_share=float(live.float().mean()), span_share=span_share(bufs[1], bufs[2], N),
                                  occupied_fraction=occ.occupied_fraction(), k_ray_occupancy_us=a, k_ray_occupancy_us_all=t_occ,
                                  k_ray_span_us=b, k_ray_span_us_all=t_span, ratio=b / a)
    return out


def _psnr(a, b):
    import numpy as np
    return float(-10.0 * np.log10(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2) + 1e-30))


def step_frames(precision="bf16", rounds=5, min_window_ms=300.0):
    import numpy as np
    import torch
    from mipnerf_pl_amd.model import CulledFrame
    flat, frame, chunk, N = golden_pose_rays()
    n = flat.origins.shape[0]
    g = np.load(os.path.join(REPO, "tests", "golden", "frame_c5_800x800.npz"))
    gt = g["gt_u8"].astype(np.float32).reshape(n, 3) / 255.0
    dev = torch.device(DEV)
    models = {128: trained_model(precision, 128), 64: trained_model(precision, 64)}
    paths = (("culled_128", 128, False), ("tightened_128", 128, True), ("tightened_64", 64, True), ("culled_64", 64, False))
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
        frames = {tag: CulledFrame(models[s], n, chunk, True, dev, occ, outside_occupied=outside, tighten=t, span_samples=N) for tag, s, t in paths}
        res = {}
        with torch.no_grad():
            for tag, fr in frames.items():      # warm every shape the windows use; the second frame's pixels give the PSNR
                for _ in range(2):
                    _, fine, _ = fr(flat)
                res[tag] = dict(psnr_vs_scene=_psnr(fine.cpu().numpy(), gt), live_share=fr.live_count / float(n), span_share=fr.span_share)
            torch.cuda.synchronize()
            # frames per window: enough of them for a window of min_window_ms, from one timed frame per path
            per_window = {tag: max(1, int(min_window_ms / timed(fr, 1)) + 1) for tag, fr in frames.items()}
            times = {tag: [] for tag in frames}
            for _ in range(rounds):             # alternating: every round times every path once
                for tag, fr in frames.items():
                    times[tag].append(timed(fr, per_window[tag]))
        for tag in frames:
            res[tag].update(frame_ms=statistics.median(times[tag]), frame_ms_all=times[tag], frames_per_window=per_window[tag])
        for tag in frames:
            res[tag]["ratio_to_culled_128"] = res[tag]["frame_ms"] / res["culled_128"]["frame_ms"]
        if name == "sphere_timing_input":       # the sphere is no model of this field: its pictures mean nothing
            for tag in frames:
                res[tag]["psnr_vs_scene"] = None
        out["grids"][name] = dict(outside_occupied=outside, paths=res)
        del frames
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--step", default=None, help="internal: run one step in this process and print its JSON")
    ap.add_argument("--steps", default="kernels,frames_bf16,frames_fp32", help="comma-separated steps to run")
    ap.add_argument("--step_timeout", type=int, default=240)
    args = ap.parse_args()
    if args.step:
        res = {"kernels": step_kernels, "frames_bf16": lambda: step_frames("bf16"),
               "frames_fp32": lambda: step_frames("fp32", rounds=3)}[args.step]()
        print("RESULT " + json.dumps(res))
        return 0
    res = {}
    if args.json and os.path.exists(args.json):       # a run of some steps keeps the others' results
        with open(args.json) as f:
            res = json.load(f)
    for st in args.steps.split(","):
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
