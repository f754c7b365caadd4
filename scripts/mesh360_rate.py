#!/usr/bin/env python3
"""Measure the density lattice of the unbounded-scene model: at 256^3 and 512^3 in bf16 and fp32 the lattice time
(`ops.density_grid(space="contracted")`) next to the MLP kernels ALONE on the same number of points (`mipnerf_time_mlp`, same process --
in bf16 that entry point runs the two-kernel form on row-major rows, the lattice the one-kernel form on fragments) and the lattice
encoder ALONE; and the one condition the encoder has to meet, against existing code in the same process: per point at 2^22 points it
takes no more than 1.10 x what k_cast_ipe_360_tile takes per sample at 2^22 samples, in the same layout and dtype (it stores the same bytes
and does less arithmetic per point; the 10 % covers the +-4 % spread between boxes).

Every GPU step is a child process under its own time limit; the first one that fails ends the run.  HIP events, warm-up, and timed
windows of at least 0.3 s (short steps are repeated inside one window).

    python scripts/mesh360_rate.py [--json profiles/mesh360_rate.json] [--sizes 256 512]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(1, os.path.join(REPO, "scripts"))

from mesh_rate import window  # noqa: E402  (one timing rule for both scripts)

CHUNK = 1 << 18              # ops.density_grid's default chunk
BOX = ((-2.0,) * 3, (2.0,) * 3)
ENCODER_LIMIT = 1.10
LAYOUTS = {"rows_fp32": ("fp32", False), "rows_bf16": ("bf16", False), "fragments_bf16": ("bf16", True)}


def trained_model(precision):
    import numpy as np
    import torch
    from mipnerf_pl_amd import MipNerf
    f = np.load(os.path.join(REPO, "tests", "golden", "trained_field_360.npz"))
    bias = float(np.load(os.path.join(REPO, "tests", "golden", "full360_1000x96.npz"))["density_bias"])
    m = MipNerf(num_samples=128, unbounded=True, precision=precision, density_bias=bias)
    m.load_state_dict({"mlp." + k[2:]: torch.from_numpy(f[k].copy()) for k in f.files if k.startswith("p_")}, strict=True)
    return m.to("cuda:0").eval()


def step_density(size, precision):
    import torch
    from mipnerf_pl_amd import _lib as L
    from mipnerf_pl_amd import ops
    model = trained_model(precision)
    prec = model.precision
    n = size ** 3
    ms, reps, win = window(lambda: ops.density_grid(model, (size,) * 3, *BOX, chunk=CHUNK, space="contracted"))
    # the MLP kernels alone on the same number of points: n / CHUNK launches of CHUNK points (n is a multiple of CHUNK here)
    assert n % CHUNK == 0
    dt = torch.bfloat16 if prec == L.PREC_BF16 else torch.float32
    enc = torch.randn(CHUNK, 672, device="cuda:0").to(dt)
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
    # the lattice encoder alone, chunk by chunk as the lattice call issues it (fragments in bf16)
    frag = prec == L.PREC_BF16

    def encode():
        for first in range(0, n, CHUNK):
            ops.lattice_ipe_360((size,) * 3, *BOX, 1.0, "contracted", 0, 16, precision=prec, fragments=frag, first=first, count=CHUNK)
    enc_ms, _, _ = window(encode)
    return dict(size=size, precision=precision, points=n, chunk=CHUNK, lattice_ms=ms, window_ms=win, calls_in_window=reps, mlp_alone_ms=mlp_ms,
                mlp_alone_form="two kernels on rows" if frag else "fp32 kernel on rows", encoder_alone_ms=enc_ms,
                encoder_bytes_per_point=672 * (2 if frag else 4), encoder_tb_per_s=n * 672 * (2 if frag else 4) / enc_ms / 1e9,
                lattice_over_mlp=ms / mlp_ms, points_per_s=n / ms * 1e3)


def step_encoder(layout):
    """the new lattice encoder per point against k_cast_ipe_360_tile per sample, 2^22 of each, same layout and dtype, same process"""
    import torch
    from mipnerf_pl_amd import _lib as L
    from mipnerf_pl_amd import ops
    precision, frag = LAYOUTS[layout]
    prec = {"fp32": L.PREC_FP32, "bf16": L.PREC_BF16}[precision]
    dims, n = (256, 128, 128), 1 << 22
    B, N = 1 << 15, 128
    g = torch.Generator(device="cuda:0").manual_seed(0)
    o = torch.rand(B, 3, device="cuda:0", generator=g) - 0.5
    d = torch.nn.functional.normalize(torch.randn(B, 3, device="cuda:0", generator=g), dim=1)
    r = torch.full((B, 1), 1e-3, device="cuda:0")
    _, t = ops.sample_t_360(N, torch.full((B, 1), 0.2, device="cuda:0"), torch.full((B, 1), 20.0, device="cuda:0"), False)
    res = {}
    for space in ("contracted", "world"):
        ms, reps, win = window(lambda: ops.lattice_ipe_360(dims, *BOX, 1.0, space, 0, 16, precision=prec, fragments=frag))
        res["lattice_" + space] = dict(ms=ms, ns_per_point=ms * 1e6 / n, window_ms=win, calls_in_window=reps)
    ms, reps, win = window(lambda: ops.cast_ipe_360(t, o, d, r, 0, 16, contracted=True, precision=prec, fragments=frag))
    res["cast_ipe_360_tile"] = dict(ms=ms, ns_per_sample=ms * 1e6 / (B * N), window_ms=win, calls_in_window=reps)
    worst = max(res["lattice_contracted"]["ms"], res["lattice_world"]["ms"]) / ms
    bytes_ = n * 672 * (2 if precision == "bf16" else 4)
    return dict(layout=layout, points=n, ratio_to_cast_ipe_360_tile=worst, limit=ENCODER_LIMIT, condition_met=worst <= ENCODER_LIMIT,
                store_tb_per_s=bytes_ / res["lattice_contracted"]["ms"] / 1e9, **res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--sizes", type=int, nargs="+", default=[256, 512])
    ap.add_argument("--step", default=None, help="internal: run one step in this process and print its JSON")
    ap.add_argument("--step_timeout", type=int, default=240)
    args = ap.parse_args()
    if args.step:
        kind, a, b = args.step.split(":")
        res = step_density(int(a), b) if kind == "density" else step_encoder(a)
        print("RESULT " + json.dumps(res))
        return 0
    steps = [f"encoder:{k}:-" for k in LAYOUTS] + [f"density:{s}:{p}" for s in args.sizes for p in ("bf16", "fp32")]
    res = dict(encoder=[], density=[])
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
        res[st.split(":")[0]].append(r)
        print(st, json.dumps(r), flush=True)
    res["encoder_condition_met"] = all(r["condition_met"] for r in res["encoder"])
    print(json.dumps(res))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
