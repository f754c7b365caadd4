#!/usr/bin/env python3
"""Measure the distorted camera models of the ray generator on one MI355X:

  frames   `generate_rays` on a 1600 x 1200 frame (1,920,000 rays) for camera modes 1 (pix2cam pinhole), 2 (radial-tangential) and 3
           (equidistant fisheye), from a float32 and from a float64 table, alternating in one process: ns per ray;
  batches  `gather_train_batch` at 8192 rays over 24 images of 1600 x 1200 for an all-mode-1 and an all-mode-2 camera table, 64 launches
           captured in one graph (as the training step holds it) and the replay divided by 64;
  parent   mode 1 of `--parent_lib` (a library built from the parent revision, which knows no other mode) beside this revision's, both
           entry points on the same inputs, alternating, with the outputs compared bit for bit (skipped without the option);
  radii    the float32 table's radii against the float64 table's at 1600 x 1200, f = 1250, largest relative difference, per mode.

The entry points are called bare (ctypes, preallocated outputs) inside HIP-event windows of at least 300 ms, so a figure is the kernel
plus its launch, not the Python wrapper.  Every GPU step is a child process under its own time limit; the first one that fails ends the run.

    python scripts/camera_models_rate.py [--parent_lib path/to/libmipnerf_hip_parent.so] [--json profiles/camera_models_rate.json]
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
W, H, F = 1600, 1200, 1250.0
MODES = {"mode1_pinhole": ("pinhole", None), "mode2_radial": ("radial", (-0.15, 0.04, 1e-3, -2e-3)),
         "mode3_fisheye": ("fisheye", (-0.03, 0.01, -0.004, 0.001))}
ROUNDS = 5


def record(model, coeffs, dtype, pose_seed=0):
    import numpy as np
    from mipnerf_pl_amd import ops
    rng = np.random.RandomState(pose_seed)
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    pose = np.concatenate([q, rng.normal(size=(3, 1))], axis=1)
    K = np.array([[F, 0.0, 0.5 * W + 3.3], [0.0, F + 5.0, 0.5 * H - 2.1], [0.0, 0.0, 1.0]])
    p2c = np.linalg.inv(K)
    p2c[1:, :] *= -1
    kw = {} if model == "pinhole" else dict(model=model, distortion=coeffs)
    return ops.camera_record(pose, W, H, 0.5, 9.0, pix2cam=p2c, dtype=dtype, **kw)


def _summary(times_ms, rays):
    med = statistics.median(times_ms)
    return dict(us=med * 1e3, us_all=[t * 1e3 for t in times_ms], ns_per_ray=med * 1e6 / rays, bytes_per_ray_written=52,
                write_gb_per_s=52 * rays / (med * 1e-3) / 1e9)


def _handle(path=None):
    """(ctypes handle, RaysPtrs) of this revision's library, or of the library at `path` bound by hand: the parent revision's symbol
    table lacks mipnerf_num_camera_modes, so the package's binding would refuse it"""
    import ctypes as C
    from mipnerf_pl_amd import _lib as L
    if path is None:
        return L.lib()
    h = C.CDLL(path)
    assert not hasattr(h, "mipnerf_num_camera_modes"), "--parent_lib knows the new entry point: not a parent build"
    for name in ("mipnerf_generate_rays", "mipnerf_generate_rays_f64", "mipnerf_gather_train_batch"):
        fn = getattr(h, name)
        fn.restype, fn.argtypes = L.SIGNATURES[name]
    return h


def frame_call(h, table, n):
    """the bare entry point into preallocated outputs (a ctypes call costs a few us, the kernel tens): (closure, outputs)"""
    import ctypes as C
    import torch
    from mipnerf_pl_amd import _lib as L
    out = [torch.empty(n, k, device=DEV) for k in (3, 3, 3, 1, 1, 1, 1)]
    rp = L.RaysPtrs(*[t.data_ptr() for t in out])
    fn = h.mipnerf_generate_rays_f64 if table.dtype == torch.float64 else h.mipnerf_generate_rays

    def call():
        assert fn(n, table.data_ptr(), None, None, C.byref(rp), torch.cuda.current_stream().cuda_stream) == 0
    call.keep = (out, rp, table)
    return call, out


def batch_call(h, model, coeffs, B, launches=64):
    """`launches` consecutive batches of `gather_train_batch` captured in one graph, as the training step holds it: the closure replays
    the graph once, so its time / launches is one launch without the host's share"""
    import ctypes as C
    import torch
    from mipnerf_pl_amd import _lib as L
    order, offsets, cams, pixels, step, base, rays, gt = a = _batch_inputs(model, coeffs, B=B)
    rb = L.RaysPtrs(*[t.data_ptr() for t in rays])

    def one():
        assert h.mipnerf_gather_train_batch(B, order.numel(), order.data_ptr(), offsets.numel() - 1, offsets.data_ptr(), cams.data_ptr(),
                                            pixels.data_ptr(), step.data_ptr(), base.data_ptr(), C.byref(rb), gt.data_ptr(),
                                            torch.cuda.current_stream().cuda_stream) == 0
    one()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(launches):
            one()
    call = g.replay
    return call, (a, rb, g), rays, gt


def step_frames():
    import torch
    n = W * H
    h = _handle()
    calls = {f"{k}_{p}": frame_call(h, record(m, c, dt).reshape(1, 32).to(DEV), n)[0] for k, (m, c) in MODES.items()
             for p, dt in (("f32", torch.float32), ("f64", torch.float64))}
    times = {k: [] for k in calls}
    for _ in range(ROUNDS):                                    # alternating: every round times every table once
        for k, fn in calls.items():
            times[k].append(window(fn)[0])
    out = dict(rays=n, width=W, height=H, rounds=ROUNDS, cases={k: _summary(v, n) for k, v in times.items()})
    for p in ("f32", "f64"):
        for k in ("mode2_radial", "mode3_fisheye"):
            out[f"{k}_over_mode1_{p}"] = out["cases"][f"{k}_{p}"]["us"] / out["cases"][f"mode1_pinhole_{p}"]["us"]
    return out


def _batch_inputs(model, coeffs, n_images=24, B=8192):
    import torch
    from mipnerf_pl_amd.rays import Rays
    table = torch.stack([record(model, coeffs, torch.float32, pose_seed=i) for i in range(n_images)]).to(DEV)
    offsets = (torch.arange(n_images + 1, dtype=torch.int64) * (W * H)).to(DEV)
    P = n_images * W * H
    g = torch.Generator(device=DEV).manual_seed(1)
    order = torch.randint(0, P, (64 * B,), device=DEV, generator=g, dtype=torch.int64)
    pixels = torch.rand(P, 3, device=DEV, generator=g)
    rays = Rays(*[torch.empty(B, k, device=DEV) for k in (3, 3, 3, 1, 1, 1, 1)])
    gt = torch.empty(B, 3, device=DEV)
    step = torch.full((1,), 7, dtype=torch.int64, device=DEV)
    base = torch.zeros(1, dtype=torch.int64, device=DEV)
    return order, offsets, table, pixels, step, base, rays, gt


LAUNCHES = 64


def step_batches():
    B = 8192
    h = _handle()
    held = {k: batch_call(h, *MODES[k], B=B, launches=LAUNCHES) for k in ("mode1_pinhole", "mode2_radial")}
    times = {k: [] for k in held}
    for _ in range(ROUNDS):
        for k, v in held.items():
            times[k].append(window(v[0])[0] / LAUNCHES)
    out = dict(rays=B, images=24, rounds=ROUNDS, launches_per_graph=LAUNCHES, cases={k: _summary(v, B) for k, v in times.items()})
    out["mode2_over_mode1"] = out["cases"]["mode2_radial"]["us"] / out["cases"]["mode1_pinhole"]["us"]
    return out


def step_parent(path):
    """mode 1 through the parent revision's library beside this revision's, in the same process, alternating"""
    import torch
    n, B = W * H, 8192
    hp, hn = _handle(path), _handle()
    table = record("pinhole", None, torch.float32).reshape(1, 32).to(DEV)
    (fp, op), (fn, on) = frame_call(hp, table, n), frame_call(hn, table, n)
    bp, bn = batch_call(hp, "pinhole", None, B, LAUNCHES), batch_call(hn, "pinhole", None, B, LAUNCHES)
    for f in (fp, fn, bp[0], bn[0]):
        f()
    torch.cuda.synchronize()
    same = all(bool(torch.equal(a, b)) for a, b in zip(op, on)) and all(bool(torch.equal(a, b)) for a, b in zip(bp[2], bn[2])) \
        and bool(torch.equal(bp[3], bn[3]))
    cases = {"frame_parent": (fp, n, 1), "frame_new": (fn, n, 1), "batch_parent": (bp[0], B, LAUNCHES), "batch_new": (bn[0], B, LAUNCHES)}
    times = {k: [] for k in cases}
    for _ in range(ROUNDS):
        for k, (f, _, per) in cases.items():
            times[k].append(window(f)[0] / per)
    res = dict(rounds=ROUNDS, mode1_bits_equal=same, launches_per_graph=LAUNCHES, cases={k: _summary(times[k], cases[k][1]) for k in cases})
    res["frame_new_over_parent"] = res["cases"]["frame_new"]["us"] / res["cases"]["frame_parent"]["us"]
    res["batch_new_over_parent"] = res["cases"]["batch_new"]["us"] / res["cases"]["batch_parent"]["us"]
    return res


def step_radii():
    import torch
    from mipnerf_pl_amd import ops
    out = {}
    for k, (m, c) in MODES.items():
        r32 = ops.generate_rays(record(m, c, torch.float32).reshape(1, 32).to(DEV)).radii.double()
        r64 = ops.generate_rays(record(m, c, torch.float64).reshape(1, 32).to(DEV)).radii.double()
        rel = ((r32 - r64).abs() / r64)
        out[k] = dict(max_rel=float(rel.max()), mean_rel=float(rel.mean()))
    return dict(width=W, height=H, focal=F, radii_float32_table_vs_float64_table=out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--parent_lib", default=None, help="libmipnerf_hip.so built from the parent revision (MIPNERF_LIB_NAME=... python -m mipnerf_pl_amd.build there)")
    ap.add_argument("--step", default=None, help="internal: run one step in this process and print its JSON")
    ap.add_argument("--step_timeout", type=int, default=150)
    args = ap.parse_args()
    steps = {"frames": step_frames, "batches": step_batches, "radii": step_radii}
    if args.parent_lib:
        steps["parent"] = lambda: step_parent(os.path.abspath(args.parent_lib))
    if args.step:
        print("RESULT " + json.dumps(steps[args.step]()))
        return 0
    res = {}
    for st in steps:
        cmd = [sys.executable, os.path.abspath(__file__), "--step", st] + (["--parent_lib", args.parent_lib] if args.parent_lib else [])
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
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
