#!/usr/bin/env python3
"""Measure the depth-fusion path on one MI355X; 5 HIP-event windows of at least 0.3 s each per row, medians with the
smallest and the largest window beside them; no kernel trace.

  integrate   k_fuse_integrate on a 256^3 lattice over [-1.5, 1.5]^3 with 800 x 800 depth maps (analytic depths of a sphere of radius 0.9
              seen from radius 4), 1, 8 and 32 frames per call (a call of more than MIPNERF_FUSE_FRAMES_PER_LAUNCH frames is split into
              launches of that many; the committed figures were taken with the constant at 32): time per call and per frame, beside a
              device copy that moves the state's bytes (16 B per point: 8 read, 8 written) in the same process;
  quantile    k_depth_quantile on 640,000 x 128 samples (Q = 1 and Q = 3), beside a device copy of the 8 bytes per sample it reads;
  command     what `python -m mipnerf_pl_amd.fuse_mesh` does on the golden scene (tests/golden/trained_field.npz, 64 samples, fp32):
              24 look-at views of 200 x 200 pixels into a 128^3 lattice, split into rendering, quantile, integration and isosurface; the
              fused mesh's vertices, faces and Euler characteristic beside `extract_mesh`'s at threshold 5 on the same lattice.

Every GPU step is a child process under its own time limit; the first one that fails ends the run.

    python scripts/fuse_rate.py [--json profiles/fuse_rate.json] [--steps integrate,quantile,command]
"""
import argparse
import json
import os
import subprocess
import sys
import time

HERE_REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = "integrate,quantile,command"


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


def _sphere_views(n, size, seed=0):
    """(cameras [n, 32] float32, depth flat float32, offsets): look-at views of the sphere of tests/isosurface_fixture.py from radius 4"""
    import numpy as np
    import fuse_fixture as fx
    import isosurface_fixture as ix
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    focal = 0.5 * size / np.tan(np.radians(50.0) / 2)
    cams = np.stack([fx.camera_row(fx.look_at(ix.CENTRE + 4.0 * v, ix.CENTRE), size, size, 0.5, 8.0, focal=focal) for v in d])
    depth, offsets = fx.sphere_depths(cams)
    return cams, depth, offsets


def step_integrate():
    import torch
    from mipnerf_pl_amd import _lib as L
    from mipnerf_pl_amd import ops
    dev = torch.device("cuda:0")
    n, size = 256, 800
    per_launch = L.FUSE_FRAMES_PER_LAUNCH
    cams, depth, offsets = _sphere_views(32, size)
    frames = ops.fuse_projection(cams).to(dev)
    depth, offsets = torch.from_numpy(depth).to(dev), torch.from_numpy(offsets).to(dev)
    vol = ops.TSDF(n, -1.5, 1.5, 3.0 * 3.0 / (n - 1), device=dev)
    src = torch.empty(n ** 3 * 8, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    out = dict(lattice=n, image=size, points=n ** 3, frames_per_launch_constant=per_launch,
               device_copy_16_bytes_per_point=_window(lambda: dst.copy_(src)))
    del src, dst
    for k in (1, 8, 32):
        fr, off = frames[:k].contiguous(), offsets[:k].contiguous()
        # the entry point itself: `TSDF.integrate` checks the frames on the host first, which synchronises
        row = _window(lambda: L.fuse_check(L.fuse_lib().mipnerf_fuse_integrate(
            vol.cdims, vol.clo, vol.chi, vol.trunc, 1, k, fr.data_ptr(), off.data_ptr(), depth.data_ptr(), depth.numel(), vol.sum.data_ptr(),
            vol.count.data_ptr(), torch.cuda.current_stream().cuda_stream)))
        row.update(ms_per_frame=row["ms"] / k, launch_over_copy=row["ms"] / out["device_copy_16_bytes_per_point"]["ms"],
                   point_frames_per_ns=n ** 3 * k / (row["ms"] * 1e6))
        out[f"frames_{k}"] = row
    out["updated_share_of_the_lattice"] = float((vol.count > 0).float().mean())
    return out


def step_quantile():
    import torch
    from mipnerf_pl_amd import ops
    dev = torch.device("cuda:0")
    B, N = 640000, 128
    g = torch.Generator(device=dev).manual_seed(0)
    centre = torch.rand(B, 1, device=dev, generator=g) * N
    w = torch.exp(-0.5 * ((torch.arange(N, device=dev)[None] - centre) / 4.0) ** 2)
    w = (w / w.sum(1, keepdim=True) * torch.rand(B, 1, device=dev, generator=g)).contiguous()      # opacity 0 .. 1: half the rays have a median
    t = torch.sort(2.0 + 4.0 * torch.rand(B, N + 1, device=dev, generator=g), dim=1).values.contiguous()
    src = torch.empty(B * N * 8, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    out = dict(rays=B, samples=N, device_copy_8_bytes_per_sample=_window(lambda: dst.copy_(src)))
    del src, dst
    for name, q in (("q1", 0.5), ("q3", (0.05, 0.5, 0.95))):
        buf = ops.depth_quantile(w, t, q)
        row = _window(lambda: ops.depth_quantile(w, t, q, out=buf))
        row.update(kernel_over_copy=row["ms"] / out["device_copy_8_bytes_per_sample"]["ms"], gbytes_per_s_read=B * (2 * N + 1) * 4 / (row["ms"] * 1e6))
        out[name] = row
    out["rays_with_a_median"] = float(torch.isfinite(ops.depth_quantile(w, t, 0.5)).float().mean())
    return out


def step_command():
    import numpy as np
    import torch
    import fuse_fixture as fx
    import gpu_util as G
    import isosurface_fixture as ix
    from mipnerf_pl_amd import ops
    from mipnerf_pl_amd.fuse import DepthFrame, mesh_of_volume
    from mipnerf_pl_amd.mesh import extract_mesh
    dev = torch.device("cuda:0")
    f = G.load_golden("trained_field")
    model = G.make_model({k[2:]: f[k] for k in f if k.startswith("p_")}, 64, "fp32").eval()
    views, size, grid = 24, 200, 128
    rng = np.random.default_rng(0)
    d = rng.normal(size=(views, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    focal = 0.5 * size / np.tan(0.5 * 0.6911112070083618)
    cams = torch.from_numpy(np.stack([fx.camera_row(fx.look_at(4.0 * v, (0, 0, 0)), size, size, 2.0, 6.0, focal=focal) for v in d]))
    frames = ops.fuse_projection(cams)
    n = size * size
    frame = DepthFrame(model, n, 12288, False, dev)
    lo, hi = (-1.5,) * 3, (1.5,) * 3
    vol = ops.TSDF(grid, lo, hi, 3.0 * 3.0 / (grid - 1), device=dev)
    cams_dev = cams.to(dev)

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return r, 1e3 * (time.perf_counter() - t0)
    rays = [ops.generate_rays(cams_dev, cam_idx=torch.full((n,), k, dtype=torch.int32, device=dev),
                              pix_idx=torch.arange(n, dtype=torch.int32, device=dev)) for k in range(views)]
    frame(rays[0])                                                  # warm-up: packing, workspace
    depths, render_ms = [], 0.0
    for k in range(views):
        dk, ms = clock(lambda: frame(rays[k])[:, 0].clone())
        depths.append(dk)
        render_ms += ms
    w, t = frame._scratch[min(n, 12288)][-1]
    quantile = _window(lambda: ops.depth_quantile(w, t, 0.5), min_ms=100.0)
    chunks = len(frame.chunks())
    _, integrate_ms = clock(lambda: vol.integrate(frames, torch.cat(depths)))
    mesh, iso_ms = clock(lambda: mesh_of_volume(model, vol, color=False))
    _, colour_ms = clock(lambda: mesh_of_volume(model, vol, color=True))
    ref = extract_mesh(model, grid=grid, lo=lo, hi=hi, threshold=5.0, color=False, precision="fp32")

    def figures(m):
        v, fc = m.vertices.cpu().numpy(), m.faces.cpu().numpy()
        return dict(vertices=len(v), faces=len(fc), euler=ix.euler_characteristic(len(v), fc), closed=bool(ix.is_closed(fc)))
    return dict(views=views, image=size, samples=64, lattice=grid, chunk=12288,
                depth_frames_ms=render_ms, of_which_quantile_ms_estimated=quantile["ms"] * views * n / w.shape[0], chunks_per_frame=chunks,
                quantile_kernel_on_one_chunk=quantile, integrate_ms=integrate_ms,
                finalise_and_isosurface_ms=iso_ms, the_same_with_vertex_colours_ms=colour_ms,
                unseen_share=float((vol.count == 0).float().mean()),
                pixels_without_depth=float(torch.isinf(torch.cat(depths)).float().mean()),
                fused=figures(mesh), extract_mesh_threshold_5=figures(ref))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--step", default=None, help="internal: run one step in this process and print its JSON")
    ap.add_argument("--steps", default=STEPS, help="comma-separated steps")
    ap.add_argument("--step_timeout", type=int, default=150)
    args = ap.parse_args()
    if args.step:
        sys.path.insert(0, HERE_REPO)
        sys.path.insert(1, os.path.join(HERE_REPO, "tests"))
        print("RESULT " + json.dumps(dict(integrate=step_integrate, quantile=step_quantile, command=step_command)[args.step]()))
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
