#!/usr/bin/env python3
"""Measure the mesh extraction: the density lattice at 256^3 and 512^3 in bf16 and fp32 next to the MLP kernels ALONE on
the same number of points (`mipnerf_time_mlp`, same process; the figure is lattice time over MLP-alone time), and the isosurface
extraction of a 512^3 sphere and of the trained field's 512^3 density with the bytes that must move over the time.

Every GPU step is a child process under its own time limit; the first one that fails ends the run.  HIP events, warm-up, and timed
windows of at least a few hundred milliseconds (short steps are repeated inside one window).

    python scripts/mesh_rate.py [--json profiles/mesh_rate.json] [--sizes 256 512]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(1, os.path.join(REPO, "tests"))

HBM_PEAK_TB_S = 8.0          # MI355X HBM3E, specification
HBM_COPY_TB_S = 6.29         # float4 device copy measured on MI355X (79 % of the specification)
CHUNK = 1 << 18              # ops.density_grid's default chunk
BOX = ((-1.5,) * 3, (1.5,) * 3)


def window(fn, min_ms=300.0, max_reps=1024):
    """milliseconds per call of fn: one warm-up, then calls in ONE event window that is at least min_ms long"""
    import torch
    fn()
    torch.cuda.synchronize()
    reps = 1
    while True:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        ms = e0.elapsed_time(e1)
        if ms >= min_ms or reps >= max_reps:
            return ms / reps, reps, ms
        reps = min(max_reps, max(reps * 2, int(reps * min_ms / max(ms, 1e-3)) + 1))


def trained_model(precision):
    import numpy as np
    import torch
    from mipnerf_pl_amd import MipNerf
    f = np.load(os.path.join(REPO, "tests", "golden", "trained_field.npz"))
    m = MipNerf(num_samples=128, precision=precision)
    m.load_state_dict({"mlp." + k[2:]: torch.from_numpy(f[k].copy()) for k in f.files if k.startswith("p_")}, strict=True)
    return m.to("cuda:0").eval()


def step_density(size, precision):
    import torch
    from mipnerf_pl_amd import _lib as L
    from mipnerf_pl_amd import ops
    model = trained_model(precision)
    prec = model.precision
    n = size ** 3
    ms, reps, win = window(lambda: ops.density_grid(model, (size,) * 3, *BOX, chunk=CHUNK))
    # the MLP kernels alone on the same number of points: n / CHUNK launches of CHUNK points (n is a multiple of CHUNK here)
    assert n % CHUNK == 0
    dt = torch.bfloat16 if prec == L.PREC_BF16 else torch.float32
    enc = torch.randn(CHUNK, 96, device="cuda:0").to(dt)
    venc = torch.zeros(1, 32, device="cuda:0", dtype=dt)
    out = torch.empty(CHUNK, 4, device="cuda:0")
    ctx = model.mlp.native(torch.device("cuda:0"))
    per = C.c_float()
    iters = n // CHUNK
    stream = torch.cuda.current_stream().cuda_stream
    for _ in range(2):       # the first call warms up
        L.check(L.lib().mipnerf_time_mlp(ctx.handle, CHUNK, CHUNK, enc.data_ptr(), venc.data_ptr(), prec, out.data_ptr(), iters, C.byref(per),
                                         stream), "time_mlp")
    mlp_ms = per.value * iters
    return dict(size=size, precision=precision, points=n, chunk=CHUNK, lattice_ms=ms, window_ms=win, calls_in_window=reps, mlp_alone_ms=mlp_ms,
                lattice_over_mlp=ms / mlp_ms, points_per_s=n / ms * 1e3)


def step_extract(kind, size):
    import torch
    from mipnerf_pl_amd import ops
    n = size ** 3
    if kind == "sphere":
        g = torch.linspace(-1.5, 1.5, size, device="cuda:0")
        z, y, x = torch.meshgrid(g, g, g, indexing="ij")
        grid, thr = (0.81 - ((x - 0.13) ** 2 + (y + 0.07) ** 2 + (z - 0.21) ** 2)).contiguous(), 0.0
        del x, y, z
    else:
        grid, thr = ops.density_grid(trained_model("bf16"), (size,) * 3, *BOX), 5.0
    out = {}

    def run():
        out["mesh"] = ops.isosurface(grid, thr, *BOX)
    ms, reps, win = window(run)
    V, F = out["mesh"][0].shape[0], out["mesh"][2].shape[0]
    # bytes that must move: the lattice read once, the mask (1 byte per point) and the vertex bases (4 bytes per point) written and read
    # once each, the outputs written (positions and normals 12 bytes per vertex each, 12 bytes per face)
    moved = 4 * n + 2 * n + 8 * n + 24 * V + 12 * F
    return dict(field=kind, size=size, points=n, vertices=V, faces=F, inside_share=float((grid > thr).float().mean()), ms=ms, window_ms=win,
                calls_in_window=reps, bytes=moved, tb_per_s=moved / ms / 1e9, share_of_hbm_peak=moved / ms / 1e9 / HBM_PEAK_TB_S,
                share_of_measured_copy=moved / ms / 1e9 / HBM_COPY_TB_S)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--step", default=None, help="internal: run one step in this process and print its JSON")
    ap.add_argument("--step_timeout", type=int, default=240)
    args = ap.parse_args()
    if args.step:
        kind, size, prec = args.step.split(":")
        res = step_density(int(size), prec) if kind == "density" else step_extract(kind, int(size))
        print("RESULT " + json.dumps(res))
        return 0
    steps = [f"density:{s}:{p}" for s in args.sizes for p in ("bf16", "fp32")] + [f"sphere:{max(args.sizes)}:-", f"trained:{max(args.sizes)}:-"]
    res = dict(hbm_peak_tb_s=HBM_PEAK_TB_S, hbm_measured_copy_tb_s=HBM_COPY_TB_S, density=[], extraction=[])
    for st in steps:
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", st], capture_output=True, text=True, timeout=args.step_timeout)
        except subprocess.TimeoutExpired:
            print(f"{st}: time limit of {args.step_timeout} s; nothing more is started", file=sys.stderr)
            return 1
        if p.returncode != 0:
            print(f"{st}: exit status {p.returncode}; nothing more is started\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}", file=sys.stderr)
            return 1
        r = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
        res["density" if st.startswith("density") else "extraction"].append(r)
        print(st, json.dumps(r), flush=True)
    print(json.dumps(res))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
