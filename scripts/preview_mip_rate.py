#!/usr/bin/env python3
"""Measure the preview over a cone-radius pyramid of lattices on one MI355X, on the golden pose with the trained field the
other rate scripts use, 256^3 points, degree 1, `--mip 4`:

  bake      the bake of the single lattice and of the 4-level pyramid (ms, MiB, the levels' sizes), each after a warm-up bake.
  frames    at image scales 1, 2, 4 and 8 (800, 400, 200 and 100 pixels a side; the cameras of `RenderGen(scales=4)`), in ONE process:
            kernel time per frame of mipnerf_preview_march, of mipnerf_preview_mip_march with L = 1 and of the full pyramid (HIP events
            around replays of the captured call; warm; the median of 21 windows of at least 30 ms; the three are timed alternating, window
            by window), the mean lod over hit rays, the share of the in-box ray length on which two levels are blended (s_0 < w < s_3;
            from the rays, in float64), mean evaluated samples per ray, and the PSNR of both pictures against the MLP's frame of the same
            size rendered in the same process and against the scene (the golden photo, box-averaged to the size).
            The box is the one `preview` takes by default (`cull_box`: everything the camera's rays reach between near and far, +-3.49).
  frames_bound1.5   the same with the lattices over [-1.5, 1.5]^3 (`--bound 1.5`, a choice: the synthetic scenes' objects lie inside it),
            where a cell is 2.3 times smaller and the footprints reach further up the pyramid.

Every GPU step is a child process under its own time limit; the first one that fails ends the run.

    python scripts/preview_mip_rate.py [--json profiles/preview_mip_rate.json] [--steps bake,frames,frames_bound1.5]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE_REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRID = 256
DEGREE = 1
LEVELS = 4
SCALES = (1, 2, 4, 8)
WINDOWS = 21
MIN_WINDOW_MS = 30.0


def _model_and_bound(bound=None):
    import torch
    from mipnerf_pl_amd.evaluate import cull_box
    from scripts.cull_rate import DEV, golden_pose_rays
    from scripts.span_rate import trained_model
    flat, frame, chunk, N = golden_pose_rays()
    return trained_model("bf16", N), cull_box([frame], GRID) if bound is None else float(bound), chunk, N, torch.device(DEV)


def step_bake():
    import time
    import torch
    from mipnerf_pl_amd import preview
    model, bound, _, _, _ = _model_and_bound()
    out = dict(grid=GRID, degree=DEGREE, levels=LEVELS, bound=bound, precision="bf16")
    with torch.no_grad():
        preview.bake_pyramid(model, grid=32, levels=3, degree=DEGREE, lo=-bound, hi=bound)        # warms the context and every kernel
        for tag, bake in (("single", lambda: preview.bake_field(model, grid=GRID, degree=DEGREE, lo=-bound, hi=bound)),
                          ("pyramid", lambda: preview.bake_pyramid(model, grid=GRID, levels=LEVELS, degree=DEGREE, lo=-bound, hi=bound))):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            baked = bake()
            torch.cuda.synchronize()
            out[tag] = dict(bake_ms=1e3 * (time.perf_counter() - t0), MiB=baked.nbytes / 2 ** 20)
            if tag == "pyramid":
                out[tag].update(dims=[list(b.dims) for b in baked.levels], spacings=list(baked.spacings),
                                MiB_per_level=[b.nbytes / 2 ** 20 for b in baked.levels],
                                baked_share_per_level=[b.baked_share() for b in baked.levels])
            del baked
            torch.cuda.empty_cache()
    return out


def _blend_length_share(pyr, o, d, rad, near, far, footprint):
    """share of the rays' in-box length on which s_0 < w = footprint * radius * t < s_{L-1}, in float64 (the slab test of rule 2)"""
    import torch
    o, d, k = o.double(), d.double(), float(footprint) * rad.double()
    lo, hi = torch.tensor(pyr.lo, dtype=torch.float64, device=o.device), torch.tensor(pyr.hi, dtype=torch.float64, device=o.device)
    t0, t1 = (lo - o) / d, (hi - o) / d
    ta = torch.maximum(near.double(), torch.minimum(t0, t1).amax(-1))
    tb = torch.minimum(far.double(), torch.maximum(t0, t1).amin(-1))
    inside = (tb - ta).clamp(min=0.0)
    a = torch.maximum(ta, pyr.spacings[0] / k)
    b = torch.minimum(tb, pyr.spacings[-1] / k)
    return float((b - a).clamp(min=0.0).sum() / inside.sum())


def step_frames(bound=None):
    import numpy as np
    import torch
    from mipnerf_pl_amd import preview
    from mipnerf_pl_amd.datasets import RenderGen
    from mipnerf_pl_amd.model import GraphedFrame
    from scripts.span_rate import _psnr
    model, bound, chunk, N, dev = _model_and_bound(bound)
    g = np.load(os.path.join(HERE_REPO, "tests", "golden", "frame_c5_800x800.npz"))
    size, pose = int(g["cfg_size"]), int(g["cfg_pose"])
    gt_full = g["gt_u8"].astype(np.float64).reshape(size, size, 3) / 255.0
    n_poses = 120
    path = RenderGen(float(g["focal"]), [size, size], scales=len(SCALES), device=dev, n_poses=n_poses)
    footprint = preview.DEFAULT_FOOTPRINT
    out = dict(grid=GRID, degree=DEGREE, levels=LEVELS, bound=bound, precision="bf16", footprint=footprint, windows=WINDOWS,
               min_window_ms=MIN_WINDOW_MS, step_scale=preview.DEFAULT_STEP_SCALE, t_min=preview.DEFAULT_T_MIN, scales={})
    with torch.no_grad():
        pyr = preview.bake_pyramid(model, grid=GRID, levels=LEVELS, degree=DEGREE, lo=-bound, hi=bound)
        one = preview.BakedPyramid(pyr.levels[:1])
        single = pyr.levels[0]
        out["dims"], out["spacings"] = [list(b.dims) for b in pyr.levels], list(pyr.spacings)
        for li, scale in enumerate(SCALES):
            rays = path[li * n_poses + pose]
            h, w = path.sizes[li * n_poses + pose]
            n = h * w
            flat = type(rays)(*[t.reshape(n, -1).contiguous() for t in rays])
            gt = gt_full.reshape(h, scale, w, scale, 3).mean((1, 3)).reshape(n, 3)
            mlp = GraphedFrame(model, n, min(chunk, n), True, dev)
            for _ in range(2):
                _, fine, _ = mlp(flat)
            mlp_rgb = fine.cpu().numpy().copy()
            del mlp
            o, d = flat.origins.float().contiguous(), flat.directions.float().contiguous()
            rad = flat.radii.reshape(-1).float().contiguous()
            near, far = flat.near.reshape(-1).float().contiguous(), flat.far.reshape(-1).float().contiguous()
            tail = (preview.DEFAULT_STEP_SCALE, preview.DEFAULT_T_MIN, preview.DEFAULT_MAX_STEPS)
            calls, graphs, bufs = {}, {}, {}
            for tag in ("plain", "mip_L1", "mip"):
                static = (torch.zeros(n, 3, device=dev), torch.zeros(n, device=dev), torch.zeros(n, device=dev))
                steps, lod = torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, device=dev)
                if tag == "plain":
                    calls[tag] = lambda s=static, st=steps: preview.march(single, o, d, near, far, True, *tail, out=s, steps=st)
                else:
                    which = one if tag == "mip_L1" else pyr
                    calls[tag] = lambda s=static, st=steps, ld=lod, p=which: preview.march_pyramid(p, o, d, rad, near, far, True, footprint, *tail,
                                                                                                   out=s, steps=st, lod=ld)
                calls[tag]()
                torch.cuda.synchronize()
                graphs[tag] = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graphs[tag]):
                    calls[tag]()
                bufs[tag] = (static, steps, lod)

            def timed(graph, reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(reps):
                    graph.replay()
                e1.record()
                e1.synchronize()
                return e0.elapsed_time(e1) / reps
            reps = {}
            for tag, gr in graphs.items():
                for _ in range(5):
                    gr.replay()
                torch.cuda.synchronize()
                reps[tag] = max(1, int(MIN_WINDOW_MS / max(timed(gr, 3), 1e-3)) + 1)
            times = {tag: [] for tag in graphs}
            for _ in range(WINDOWS):                                   # alternating: every round times every kernel once
                for tag, gr in graphs.items():
                    times[tag].append(timed(gr, reps[tag]))
            res = dict(height=h, width=w, rays=n, mlp_psnr_vs_scene=_psnr(mlp_rgb, gt),
                       blend_share_of_in_box_length=_blend_length_share(pyr, o, d, rad, near, far, footprint), kernels={})
            for tag in graphs:
                static, steps, lod = bufs[tag]
                rgb = static[0].cpu().numpy()
                hit = static[1] > 0
                res["kernels"][tag] = dict(frame_ms=statistics.median(times[tag]), frame_ms_min=min(times[tag]), frame_ms_max=max(times[tag]),
                                           replays_per_window=reps[tag], mean_steps_per_ray=float(steps.sum(dtype=torch.int64)) / n,
                                           psnr_vs_scene=_psnr(rgb, gt), psnr_vs_mlp=_psnr(rgb, mlp_rgb),
                                           mean_lod_over_hit_rays=float(lod[hit].mean()) if tag != "plain" and bool(hit.any()) else 0.0)
            res["mip_L1_equals_plain_bytes"] = all(torch.equal(a.view(torch.int32), b.view(torch.int32))
                                                   for a, b in zip(list(bufs["plain"][0]) + [bufs["plain"][1]], list(bufs["mip_L1"][0]) + [bufs["mip_L1"][1]]))
            res["mip_L1_minus_plain_ms"] = res["kernels"]["mip_L1"]["frame_ms"] - res["kernels"]["plain"]["frame_ms"]
            out["scales"][str(scale)] = res
            del graphs, bufs, calls
            torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--step", default=None, help="internal: run one step in this process and print its JSON")
    ap.add_argument("--steps", default="bake,frames,frames_bound1.5", help="comma-separated steps to run")
    ap.add_argument("--step_timeout", type=int, default=300)
    args = ap.parse_args()
    if args.step:
        sys.path.insert(0, HERE_REPO)
        sys.path.insert(1, os.path.join(HERE_REPO, "tests"))
        res = step_bake() if args.step == "bake" else step_frames(float(args.step.partition("_bound")[2]) if "_bound" in args.step else None)
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
        print(st, json.dumps(res[st])[:3000], flush=True)
        if args.json:                                 # kept step by step: a later step that fails loses nothing
            os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
            with open(args.json, "w") as f:
                json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
