#!/usr/bin/env python3
"""Measure the proposal density of the unbounded-scene model on one MI355X: the trained fixture field
(tests/golden/trained_field_360.npz), the 54,208-ray frame of DESIGN 4.9 (tests/golden/scene360_rays.npz) at 96 samples and the 1000
golden rays of tests/golden/full360_1000x96.npz; 5 HIP-event windows of at least 0.3 s each per row (thousands of calls of the kernel),
medians with the smallest and the largest window beside them; no kernel trace.

  kernel_<prec>    per pyramid (grid 64 / 128 / 256 x levels 1 .. 4 of the field at this precision): the build time of the pyramid,
                   k_lattice_density_360 on the whole frame, beside a device copy of the bytes it writes (16 per sample) and beside the
                   work it stands in for -- cast_ipe_360 + the MLP pass of the coarse level on the same samples, chunk by chunk through
                   the stage entry points -- and which levels the frame's samples select;
  quality_<prec>   the fine level's colour on the 1000 golden rays when the coarse density comes from a pyramid: grid 64 / 128 x levels
                   1 / 3, footprint 0.5 / 1 / 2 and cov_scale 1 / 4 at grid 128; PSNR against the two-level frame of the same model, and
                   of both against the golden file's own fine colour (the 360 oracle's two-level forward).  The levels are composed here through
                   the stage entry points, as MipNerf._forward_native(proposal=) composes them (sample_t_360 ->
                   lattice_density_360 -> volumetric_rendering_packed -> resample_t on the inverse-depth posts -> 1 / t_inv ->
                   cast_ipe_360 -> mlp -> volumetric_rendering_packed); the same composition with the MLP as the coarse level is
                   compared with MipNerf._forward_native first, so that the numbers say something about the lattice and not the script.

  frame_<prec>     the whole 54,208-ray frame: two-level (captured and eager) against frames with a pyramid (never captured), plain and on top
                   of the contracted occupancy, plain and tightened; windows of at least 0.3 s, rows alternating, medians.

Every GPU step is a child process under its own time limit; the first one that fails ends the run.

    python scripts/proposal360_rate.py [--json profiles/proposal360_rate.json] [--steps kernel_bf16,...]
"""
import argparse
import json
import os
import subprocess
import sys
import time

HERE_REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = "kernel_bf16,kernel_fp32,quality_fp32,quality_bf16,frame_bf16,frame_fp32"
N = 96
CHUNK = 8192


def _psnr(a, b):
    import torch
    mse = float(((a.double() - b.double()) ** 2).mean())
    return float("inf") if mse == 0.0 else float(-10.0 * torch.log10(torch.tensor(mse)))


def _window(call, windows=5, min_ms=300.0):
    """median ms per call over `windows` windows of at least `min_ms`, HIP events around the calls of a window"""
    import statistics
    import torch

    def timed(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            call()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / reps
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    reps = max(1, int(min_ms / max(timed(3), 1e-3)) + 1)
    times = [timed(reps) for _ in range(windows)]
    return dict(ms=statistics.median(times), ms_min=min(times), ms_max=max(times), calls_per_window=reps)


def _levels_hist(grid, rays):
    """samples of the frame per pyramid level (the level rule on the host, at the device's own covariances)"""
    import numpy as np
    import proposal360_fixture as qx
    import torch
    from mipnerf_pl_amd import ops
    _, t = ops.sample_t_360(N, rays.near, rays.far, False)
    _, covs = ops.cast_rays_360(t, rays.origins, rays.directions, rays.radii, contracted=True)
    trace = (covs[..., 0, 0] + covs[..., 1, 1]) + covs[..., 2, 2]
    w = (grid.footprint * 2.0 * torch.sqrt(trace)).cpu().numpy().astype(np.float32)
    l, g = qx.mip_level_f32(np.asarray(grid.spacing, np.float32), w)
    return dict(per_level=np.bincount(l.ravel(), minlength=len(grid)).tolist(), mixed=int((g > 0).sum()),
                footprint_cells_of_level0=[float(np.percentile(w, p)) / grid.spacing[0] for p in (1, 50, 99)])


def step_kernel(precision):
    import torch
    import test_gpu_cull360 as C3
    from mipnerf_pl_amd import Rays, ops
    model = C3.model360(precision, N)
    full = C3.G.to_dev(C3.G.rays_of({k: v for k, v in C3.G.load_golden("scene360_rays").items() if k.startswith("rays_")}))
    B = full.origins.shape[0]
    far_radius = C3.frame_far_radius()
    _, t = ops.sample_t_360(N, full.near, full.far, False)
    src = torch.empty(B * N * 16, dtype=torch.uint8, device=t.device)
    dst = torch.empty_like(src)
    out = dict(rays=B, samples=N, far_radius=far_radius, device_copy_same_bytes=_window(lambda: dst.copy_(src)))
    del src, dst
    venc = ops.pos_enc(full.viewdirs, 0, model.deg_view)

    def coarse_mlp_pass():
        for lo in range(0, B, CHUNK):
            r = Rays(*[x[lo:lo + CHUNK] for x in full])
            enc = ops.cast_ipe_360(t[lo:lo + CHUNK], r.origins, r.directions, r.radii, model.min_deg_point, model.max_deg_point,
                                   precision=model.precision)
            model.mlp(enc, venc[lo:lo + CHUNK], return_activated=True)
    with torch.no_grad():
        out["coarse_level_cast_ipe_360_and_mlp"] = _window(coarse_mlp_pass)
    for n in (64, 128, 256):
        for levels in (1, 2, 3, 4):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            with torch.no_grad():
                grid = ops.field_proposal_360(model, grid=n, levels=levels, far_radius=far_radius)
            torch.cuda.synchronize()
            build_ms = 1e3 * (time.perf_counter() - t0)
            tk = _window(lambda: ops.lattice_density_360(grid, t, full.origins, full.directions, full.radii))
            out[f"g{n}_l{levels}"] = dict(build_ms=build_ms, kernel=tk, ns_per_sample=1e6 * tk["ms"] / (B * N),
                                          kernel_over_copy=tk["ms"] / out["device_copy_same_bytes"]["ms"], **_levels_hist(grid, full))
            del grid
    return out


def _compose(model, rays, coarse):
    """both levels through the stage entry points; coarse(t0) -> packed [B, N, 4] (colour, density) of level 0"""
    import torch
    from mipnerf_pl_amd import ops
    t_inv0, t0 = ops.sample_t_360(N, rays.near, rays.far, False)
    w0 = ops.volumetric_rendering_packed(coarse(t0), t0, rays.directions, True)[3]
    t_inv1 = ops.resample_t(t_inv0, w0, False, model.resample_padding)
    t1 = torch.reciprocal(t_inv1)
    enc = ops.cast_ipe_360(t1, rays.origins, rays.directions, rays.radii, model.min_deg_point, model.max_deg_point, precision=model.precision)
    _, _, act = model.mlp(enc, ops.pos_enc(rays.viewdirs, 0, model.deg_view), return_activated=True)
    return ops.volumetric_rendering_packed(act, t1, rays.directions, True)[0], t1


def step_quality(precision):
    import torch
    import test_gpu_cull360 as C3
    from mipnerf_pl_amd import ops
    model = C3.model360(precision, N)
    g, rays = C3.ray_set(C3.FRAME_SET)
    golden = torch.from_numpy(C3.G.load_golden(C3.FRAME_SET)["l1_rgb"]).to(rays.origins.device)
    far_radius = C3.frame_far_radius()
    venc = ops.pos_enc(rays.viewdirs, 0, model.deg_view)

    def coarse_mlp(t0):
        enc = ops.cast_ipe_360(t0, rays.origins, rays.directions, rays.radii, model.min_deg_point, model.max_deg_point, precision=model.precision)
        return model.mlp(enc, venc, return_activated=True)[2]

    def coarse_lattice(grid):
        def f(t0):
            sigma = ops.lattice_density_360(grid, t0, rays.origins, rays.directions, rays.radii)
            return torch.cat([torch.zeros(*sigma.shape, 3, device=sigma.device), sigma[..., None]], dim=-1).contiguous()
        return f
    with torch.no_grad():
        two = model._forward_native(rays, False, True)
        rgb, t1 = _compose(model, rays, coarse_mlp)
        out = dict(rays=int(golden.shape[0]), far_radius=far_radius,
                   composition_equals_forward=dict(fine_rgb=bool(torch.equal(rgb, two[1][0])), fine_t=bool(torch.equal(t1, two[1][4])),
                                                   max_abs_rgb=float((rgb - two[1][0]).abs().max())),
                   two_level_psnr_vs_golden=_psnr(two[1][0], golden), rows=[])
        configs = [(n, lv, 1.0, 1.0) for n in (64, 128) for lv in (1, 3)]
        configs += [(128, lv, fp, cs) for lv in (1, 3) for fp in (0.5, 1.0, 2.0) for cs in (1.0, 4.0) if (fp, cs) != (1.0, 1.0)]
        configs += [(256, 1, 1.0, 1.0), (256, 3, 1.0, 1.0)]
        for n, lv, fp, cs in configs:
            grid = ops.field_proposal_360(model, grid=n, levels=lv, far_radius=far_radius, cov_scale=cs, footprint=fp)
            rgb, t1 = _compose(model, rays, coarse_lattice(grid))
            out["rows"].append(dict(grid=n, levels=lv, footprint=fp, cov_scale=cs, psnr_vs_two_level=_psnr(rgb, two[1][0]),
                                    psnr_vs_golden=_psnr(rgb, golden), max_abs_vs_two_level=float((rgb - two[1][0]).abs().max())))
            del grid
    return out


def step_frame(precision):
    """the 54,208-ray frame at 96 samples in 8192-ray chunks: the two-level frame (captured, and eager as the proposal frames are) against
    frames with a pyramid (never captured), plain and on top of the contracted occupancy (plain and tightened); rows alternate inside one
    process, windows of at least 0.3 s, medians"""
    import statistics
    import torch
    import test_gpu_cull360 as C3
    from mipnerf_pl_amd import ops
    from mipnerf_pl_amd.model import CulledFrame, GraphedFrame
    model = C3.model360(precision, N)
    full = C3.G.to_dev(C3.G.rays_of({k: v for k, v in C3.G.load_golden("scene360_rays").items() if k.startswith("rays_")}))
    B, dev = full.origins.shape[0], torch.device(C3.DEV)
    far_radius = C3.frame_far_radius()
    occ = C3.frame_occupancy(C3.FRAME_THRESHOLD)
    rows = {"two_level_captured": GraphedFrame(model, B, CHUNK, True, dev), "two_level_eager": GraphedFrame(model, B, CHUNK, True, dev, capture=False),
            "two_level_culled": CulledFrame(model, B, CHUNK, True, dev, occ), "two_level_tightened": CulledFrame(model, B, CHUNK, True, dev, occ, tighten=True)}
    for n, lv in ((64, 1), (128, 1), (128, 3), (256, 1), (256, 3)):
        grid = ops.field_proposal_360(model, grid=n, levels=lv, far_radius=far_radius)
        rows[f"proposal_g{n}_l{lv}"] = GraphedFrame(model, B, CHUNK, True, dev, proposal=grid)
        if (n, lv) == (128, 3):
            rows[f"proposal_g{n}_l{lv}_culled"] = CulledFrame(model, B, CHUNK, True, dev, occ, proposal=grid)
            rows[f"proposal_g{n}_l{lv}_tightened"] = CulledFrame(model, B, CHUNK, True, dev, occ, tighten=True, proposal=grid)

    def timed(frame, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            frame(full)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / reps
    reps, times = {}, {k: [] for k in rows}
    with torch.no_grad():
        for k, f in rows.items():
            f(full)
            reps[k] = max(1, int(300.0 / max(timed(f, 2), 1e-3)) + 1)
        for _ in range(5):
            for k, f in rows.items():
                times[k].append(timed(f, reps[k]))
    out = dict(rays=B, samples=N, chunk=CHUNK, far_radius=far_radius)
    for k in rows:
        out[k] = dict(ms=statistics.median(times[k]), ms_min=min(times[k]), ms_max=max(times[k]), frames_per_window=reps[k])
    for k in rows:
        if k.startswith("proposal"):
            base = "two_level_culled" if k.endswith("culled") else "two_level_tightened" if k.endswith("tightened") else "two_level_captured"
            out[k]["over_" + base] = out[k]["ms"] / out[base]["ms"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--step", default=None, help="internal: run one step in this process and print its JSON")
    ap.add_argument("--steps", default=STEPS, help="comma-separated steps")
    ap.add_argument("--step_timeout", type=int, default=240)
    args = ap.parse_args()
    if args.step:
        sys.path.insert(0, HERE_REPO)
        sys.path.insert(1, os.path.join(HERE_REPO, "tests"))
        kind, precision = args.step.split("_")
        print("RESULT " + json.dumps(dict(kernel=step_kernel, quality=step_quality, frame=step_frame)[kind](precision)))
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
        print(st, json.dumps(res[st]), flush=True)
        if args.json:                                 # kept step by step: a later step that fails loses nothing
            os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
            with open(args.json, "w") as f:
                json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
