#!/usr/bin/env python3
"""Measure the density lattice as the proposal level on one MI355X, on the golden 800 x 800 pose:

  kernel    `ops.lattice_density` alone per 640,000 x 128 samples on 128^3, 256^3 and 512^3 lattices over `cull_box` of the frame, next to
            a device copy of the bytes it writes (16 per sample); and the lattice build time (`ops.field_proposal`) in bf16 and fp32.
            HIP events, windows of at least 0.3 s.
  frames    in one process, alternating: the frame without the keyword and with proposals at 128^3, 256^3 and 512^3, each as
            `GraphedFrame` and as `CulledFrame` plain, tightened and adaptive (the trained field's grid of scripts/span_rate.py).  Per
            row the frame time and the fine-rgb PSNR against the scene's ground truth.
  default   the frames WITHOUT the keyword only, from the checkout `--root DIR` (default: this one).  With `--parent DIR` (a built
            checkout of the parent commit) the run alternates parent, this, parent, this: the two parent runs give the spread the parent
            shows against itself, which the difference between the commits is held against.

Every GPU step is a child process under its own time limit; the first one that fails ends the run.

    python scripts/proposal_rate.py [--json profiles/proposal_rate.json] [--parent DIR]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

HERE_REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LATTICES = (128, 256, 512)
MODES = (("graphed", None), ("cull", {}), ("cull_tighten", dict(tighten=True)), ("cull_adaptive", dict(adaptive=True)))


def use_root(root):
    """import the package, the tests' helpers and the other scripts from the checkout `root`"""
    sys.path.insert(0, root)
    sys.path.insert(1, os.path.join(root, "tests"))


def _timed(fr, flat, frames):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(frames):
        fr(flat)
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / frames


def _measure(frames, flat, gt, rounds, min_window_ms):
    """{tag: frame_ms, psnr, ...} of the frame objects `frames`, timed alternating: every round times every row once"""
    import torch
    from scripts.span_rate import _psnr
    res = {}
    with torch.no_grad():
        for tag, fr in frames.items():          # warm every shape the windows use; the second frame's pixels give the PSNR
            for _ in range(2):
                _, fine, _ = fr(flat)
            res[tag] = dict(psnr_vs_scene=_psnr(fine.cpu().numpy(), gt))
            if hasattr(fr, "live_count"):
                res[tag]["live_share"] = fr.live_count / float(flat.origins.shape[0])
        torch.cuda.synchronize()
        per_window = {tag: max(1, int(min_window_ms / _timed(fr, flat, 1)) + 1) for tag, fr in frames.items()}
        times = {tag: [] for tag in frames}
        for _ in range(rounds):
            for tag, fr in frames.items():
                times[tag].append(_timed(fr, flat, per_window[tag]))
    for tag in frames:
        res[tag].update(frame_ms=statistics.median(times[tag]), frame_ms_all=times[tag], frames_per_window=per_window[tag])
    return res


def _frame(model, n, chunk, dev, occ, outside, N, mode_kw, proposal=None):
    from mipnerf_pl_amd.model import CulledFrame, GraphedFrame
    kw = {} if proposal is None else dict(proposal=proposal)       # a parent checkout has no such keyword
    if mode_kw is None:
        return GraphedFrame(model, n, chunk, True, dev, **kw)
    return CulledFrame(model, n, chunk, True, dev, occ, outside_occupied=outside, span_samples=N, **dict(mode_kw, **kw))


def _setup(precision):
    import numpy as np
    import torch
    from scripts.cull_rate import DEV, golden_pose_rays
    from scripts.span_rate import grids, trained_model
    flat, frame, chunk, N = golden_pose_rays()
    n = flat.origins.shape[0]
    g = np.load(os.path.join(sys.path[0], "tests", "golden", "frame_c5_800x800.npz"))
    gt = g["gt_u8"].astype(np.float32).reshape(n, 3) / 255.0
    occ, outside = grids(flat, frame, N)["trained_thr0.03_dilate0_64_pm2"]
    return flat, frame, chunk, N, n, gt, float(g["psnr_fine"]), torch.device(DEV), trained_model(precision, N), occ, outside


def step_default(precision, rounds, min_window_ms=300.0):
    flat, frame, chunk, N, n, gt, ref, dev, model, occ, outside = _setup(precision)
    frames = {tag: _frame(model, n, chunk, dev, occ, outside, N, kw) for tag, kw in MODES}
    return dict(precision=precision, checkout="this" if os.path.samefile(sys.path[0], HERE_REPO) else "parent", rays=n, chunk=chunk, rounds=rounds, ref_psnr_vs_scene=ref,
                rows=_measure(frames, flat, gt, rounds, min_window_ms))


def step_frames(precision, rounds, min_window_ms=300.0):
    import torch
    from mipnerf_pl_amd import ops
    from mipnerf_pl_amd.evaluate import cull_box
    flat, frame, chunk, N, n, gt, ref, dev, model, occ, outside = _setup(precision)
    out = dict(precision=precision, rays=n, chunk=chunk, samples=N, rounds=rounds, min_window_ms=min_window_ms, ref_psnr_vs_scene=ref,
               lattices={})
    for size in (None,) + LATTICES:
        prop = None
        if size is not None:
            bound = cull_box([frame], size)
            prop = ops.field_proposal(model, grid=size, lo=-bound, hi=bound)
        frames = {tag: _frame(model, n, chunk, dev, occ, outside, N, kw, prop) for tag, kw in MODES}
        rows = _measure(frames, flat, gt, rounds, min_window_ms)
        out["lattices"]["none" if size is None else str(size)] = dict(bound=None if size is None else bound, rows=rows)
        del frames, prop
        torch.cuda.empty_cache()
    base = out["lattices"]["none"]["rows"]
    for size in LATTICES:
        for tag, row in out["lattices"][str(size)]["rows"].items():
            row["ratio_to_two_level"] = row["frame_ms"] / base[tag]["frame_ms"]
            row["psnr_gap_to_two_level"] = row["psnr_vs_scene"] - base[tag]["psnr_vs_scene"]
    return out


def step_kernel(rounds=5):
    import time
    import torch
    from mipnerf_pl_amd import ops
    from mipnerf_pl_amd.evaluate import cull_box
    from scripts.cull_rate import DEV, RAYS, SAMPLES, golden_pose_rays
    from scripts.mesh_rate import window
    from scripts.span_rate import trained_model
    flat, frame, _, N = golden_pose_rays()
    assert flat.origins.shape[0] == RAYS and N == SAMPLES
    t = ops.sample_t(N, flat.near, flat.far, False, False)
    src = torch.rand(RAYS, N, 4, device=DEV)
    dst = torch.empty_like(src)
    out = dict(rays=RAYS, samples=N, bytes_written=RAYS * N * 16, rounds=rounds, min_window_ms=300.0, lattices={})
    models = {p: trained_model(p, N) for p in ("bf16", "fp32")}
    for size in LATTICES:
        bound = cull_box([frame], size)
        build = {}
        for p, m in models.items():
            ms = []
            for _ in range(3):                      # the first build also warms the context
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                prop = ops.field_proposal(m, grid=size, lo=-bound, hi=bound)
                torch.cuda.synchronize()
                ms.append(1e3 * (time.perf_counter() - t0))
            build[p + "_build_ms"], build[p + "_build_ms_all"] = min(ms[1:]), ms
        k, c = [], []
        for _ in range(rounds):                     # alternating: every round times both once
            k.append(window(lambda: ops.lattice_density(prop, t, flat.origins, flat.directions, flat.radii))[0] * 1e3)
            c.append(window(lambda: dst.copy_(src))[0] * 1e3)
        res = dict(bound=bound, lattice_bytes=size ** 3 * 4, lattice_density_us=statistics.median(k), lattice_density_us_all=k,
                   copy_us=statistics.median(c), copy_us_all=c, **build)
        res["lattice_density_over_copy"] = res["lattice_density_us"] / res["copy_us"]
        out["lattices"][str(size)] = res
        del prop
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--step", default=None, help="internal: run one step in this process and print its JSON")
    ap.add_argument("--steps", default="kernel,frames_bf16,frames_fp32", help="comma-separated steps to run")
    ap.add_argument("--root", default=HERE_REPO, help="internal: the checkout a default_* step imports")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: adds the alternating default_* steps")
    ap.add_argument("--step_timeout", type=int, default=400)
    args = ap.parse_args()
    if args.step:
        use_root(os.path.abspath(args.root))
        name, _, precision = args.step.partition("_")
        if name == "kernel":
            res = step_kernel()
        else:
            res = (step_default if name == "default" else step_frames)(precision, rounds=5 if precision == "bf16" else 3)
        print("RESULT " + json.dumps(res))
        return 0
    res = {}
    if args.json and os.path.exists(args.json):       # a run of some steps keeps the others' results
        with open(args.json) as f:
            res = json.load(f)
    steps = [(st, st, HERE_REPO) for st in args.steps.split(",") if st]
    if args.parent:
        for p in ("bf16", "fp32"):
            for tag, root in (("parent_a", args.parent), ("this_a", HERE_REPO), ("parent_b", args.parent), ("this_b", HERE_REPO)):
                steps.append((f"default_{p}_{tag}", f"default_{p}", root))
    for key, st, root in steps:
        cmd = [sys.executable, os.path.abspath(__file__), "--step", st, "--root", os.path.abspath(root)]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=args.step_timeout, cwd=os.path.abspath(root))
        except subprocess.TimeoutExpired:
            print(f"{key}: time limit of {args.step_timeout} s; nothing more is started", file=sys.stderr)
            return 1
        if p.returncode != 0:
            print(f"{key}: exit status {p.returncode}; nothing more is started\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}", file=sys.stderr)
            return 1
        res[key] = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
        print(key, json.dumps(res[key]), flush=True)
        if args.json:                                 # kept step by step: a later step that fails loses nothing
            os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
            with open(args.json, "w") as f:
                json.dump(res, f, indent=1)
    if args.parent:                                   # the commits' difference next to the parent's own spread, per row
        for p in ("bf16", "fp32"):
            rows = {k: res[f"default_{p}_{k}"]["rows"] for k in ("parent_a", "parent_b", "this_a", "this_b")}
            cmp_ = {}
            for tag in rows["parent_a"]:
                pa, pb, ta, tb = (rows[k][tag]["frame_ms"] for k in ("parent_a", "parent_b", "this_a", "this_b"))
                cmp_[tag] = dict(parent_ms=[pa, pb], this_ms=[ta, tb], parent_spread_ms=abs(pa - pb),
                                 difference_ms=(ta + tb) / 2 - (pa + pb) / 2)
            res[f"default_{p}_comparison"] = cmp_
            print(f"default_{p}_comparison", json.dumps(cmp_))
        if args.json:
            with open(args.json, "w") as f:
                json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
