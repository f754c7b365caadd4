#!/usr/bin/env python3
"""Measure the tuning of the contracted preview lattice on one MI355X, on the field trained on the scene of
tests/scene360_fixture.py (tests/golden/trained_field_360.npz) and its 54,208 captured rays (tests/golden/scene360_rays.npz: 7 views of
88 x 88 pixels with their photos), the field, rays, far radius and lattices of DESIGN 4.19's table.  One child process per point, each
under its own time limit; the first one that fails ends the run; the JSON is rewritten after every point.

  rate_g<grid>_d<degree>    k_preview_360_tune_grad on 65,536 rays drawn uniformly (seed 0) from the captured ones, target mode against the
                            MLP's render: milliseconds, the forward k_preview_360 alone on the same rays, the debug counters (samples,
                            flushes), added bytes per second (a flush adds 8 corner rows x the used entries x 4 bytes); the whole step
                            (gradient, Adam) with the batch and its target at hand, and with the MLP's render of the batch inside the step
  quality_g<grid>_<bake>    degree 1; bake threshold 0.5 (`t0.5`, DESIGN 4.19's) or 0 (`t0`: every cell with a positive density at a
                            corner, i.e. everything inside the far ball).  THE SPLIT: the MLP was trained on all 7 views, so there is no
                            view it has not seen; the lattice is tuned on views 0 - 5 and every PSNR is taken on view 6, which no tuning
                            step draws from.  Per target (photos / the fp32 MLP's render) and per regulariser (off / --tv_sigma TV_SIGMA):
                            PSNR of view 6 against its photo and against the MLP's frame, untuned, after 500 and after 2000 steps of
                            BATCH rays; mean acc; march ms of the whole 54,208-ray frame untuned, tuned, and after reoccupy(0.5).

    python scripts/preview_tune360_rate.py [--json profiles/preview_tune360_rate.json] [--grids 128 256] [--only rate|quality]
"""
import argparse
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(1, os.path.join(REPO, "scripts"))
from cull360_rate import DEV, far_radius_of, golden_rays, trained_model  # noqa: E402  (one trained field for the 360 rate scripts)
from mesh_rate import window  # noqa: E402  (one timing rule for all the rate scripts)

BATCH = 65536
TUNE_BATCH = 32768            # a choice: the 6 training views hold 46,464 rays
VIEW = 88 * 88                # rays per view of the capture
TV_SIGMA = 1e-3               # a choice, the one value tried: the low end of what DESIGN 4.20 found useful
CHUNK = 8192
WHITE = (1.0, 1.0, 1.0)       # the field was trained on a white background


def psnr(a, b):
    import torch
    return float(-10.0 * torch.log10(((a - b) ** 2).mean()))


def _flat(rays):
    n = int(rays.origins.shape[0])
    return rays.origins.contiguous(), rays.directions.contiguous(), rays.near.reshape(n).contiguous(), rays.far.reshape(n).contiguous()


def _mlp_render(model, rays, dev):
    import torch
    from mipnerf_pl_amd.model import GraphedFrame
    n = int(rays.origins.shape[0])
    with torch.no_grad():
        return GraphedFrame(model, n, CHUNK, True, dev, capture=False)(rays)[1].reshape(n, 3).clone()


def step_rate(grid, degree):
    import torch
    from mipnerf_pl_amd import Rays, preview, preview_tune360 as pt
    from mipnerf_pl_amd.model import GraphedFrame
    dev = torch.device(DEV)
    every = golden_rays("scene360_rays")
    R = far_radius_of(every, grid)
    model = trained_model("fp32")
    with torch.no_grad():
        baked = preview.bake_field(model, grid=grid, degree=degree, threshold=0.5, dilate=1, space="contracted", far_radius=R)
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    ids = torch.randint(0, every.origins.shape[0], (BATCH,), generator=gen, device=dev)
    rays = Rays(*[t[ids].contiguous() for t in every])
    bf16 = trained_model("bf16")
    frame = GraphedFrame(bf16, BATCH, CHUNK, True, dev, capture=False)
    with torch.no_grad():
        target = frame(rays)[1].reshape(BATCH, 3).clone()
    o, d, near, far = _flat(rays)
    grad = torch.zeros(baked.rows.shape, dtype=torch.float32, device=dev)
    out = (torch.empty(BATCH, 3, device=dev), torch.empty(BATCH, device=dev))
    counters = torch.zeros(2, dtype=torch.int64, device=dev)
    scale = 2.0 / (3.0 * BATCH)
    pt.march_grad(baked, o, d, near, far, WHITE, target=target, loss_scale=scale, grad_rows=grad, out=out, counters=counters)
    torch.cuda.synchronize()
    samples, flushes = counters.tolist()
    march_out = (torch.empty(BATCH, 3, device=dev), torch.empty(BATCH, device=dev), torch.empty(BATCH, device=dev))
    preview.march(baked, o, d, near, far, WHITE, out=march_out)
    same = bool(torch.equal(out[0], march_out[0]) and torch.equal(out[1], march_out[1]))
    t_grad = window(lambda: pt.march_grad(baked, o, d, near, far, WHITE, target=target, loss_scale=scale, grad_rows=grad, out=out))
    t_march = window(lambda: preview.march(baked, o, d, near, far, WHITE, out=march_out))
    state = pt.TuneState360(baked)

    def step_with_mlp():
        with torch.no_grad():
            state.step(rays, frame(rays)[1].reshape(BATCH, 3), WHITE)
    t_step = window(lambda: state.step(rays, target, WHITE))
    t_step_mlp = window(step_with_mlp, max_reps=64)
    used = 1 + 3 * (degree + 1) ** 2
    added = flushes * 8 * used * 4
    return dict(grid=grid, degree=degree, rays=BATCH, far_radius=R, tune_grad_ms=t_grad[0], march_alone_ms=t_march[0],
                backward_over_forward=t_grad[0] / t_march[0], contributing_samples=samples, flushes=flushes,
                flushes_per_sample=flushes / max(samples, 1), added_bytes=added, added_TB_per_s=added / (t_grad[0] * 1e-3) / 1e12,
                same_rgb_as_march=same, step_ms=t_step[0], step_with_mlp_target_ms=t_step_mlp[0],
                masked_in_share=float(state.mask.float().mean()))


def step_quality(grid, bake):
    import torch
    from mipnerf_pl_amd import Rays, preview, preview_tune360 as pt
    dev = torch.device(DEV)
    every = golden_rays("scene360_rays")
    import numpy as np
    photos = torch.from_numpy(np.load(os.path.join(REPO, "tests", "golden", "scene360_rays.npz"))["rgb"]).to(dev)
    n = int(every.origins.shape[0])
    assert n == 7 * VIEW
    R = far_radius_of(every, grid)
    threshold = 0.5 if bake == "t0.5" else 0.0
    model = trained_model("fp32")
    mlp = _mlp_render(model, every, dev)
    with torch.no_grad():
        fresh = preview.bake_field(model, grid=grid, degree=1, threshold=threshold, dilate=1, space="contracted", far_radius=R)
    held = slice(6 * VIEW, 7 * VIEW)
    o, d, near, far = _flat(every)
    bufs = (torch.empty(n, 3, device=dev), torch.empty(n, device=dev), torch.empty(n, device=dev))
    out = dict(grid=grid, bake_threshold=threshold, far_radius=R, occupied_fraction=fresh.occupancy.occupied_fraction(),
               mlp_vs_photos_held_out=psnr(mlp[held], photos[held]), mlp_vs_photos_all=psnr(mlp, photos), tune_batch=TUNE_BATCH,
               tv_sigma_when_on=TV_SIGMA)

    def score(field):
        preview.march(field, o, d, near, far, WHITE, out=bufs)
        return dict(vs_photos=psnr(bufs[0][held], photos[held]), vs_mlp=psnr(bufs[0][held], mlp[held]),
                    vs_photos_tuned_views=psnr(bufs[0][:6 * VIEW], photos[:6 * VIEW]), acc_mean=float(bufs[1].mean()),
                    acc_mean_held_out=float(bufs[1][held].mean()))
    out["untuned"] = score(fresh)
    out["untuned"]["march_ms"] = window(lambda: preview.march(fresh, o, d, near, far, WHITE, out=bufs))[0]
    for target_name, targets in (("photos", photos), ("mlp", mlp)):
        for tv in (0.0, TV_SIGMA):
            baked = preview.BakedField(fresh.rows.clone(), fresh.dims, fresh.lo, fresh.hi, 1, fresh.occupancy, fresh.threshold, fresh.space,
                                       fresh.far_radius)
            gen = torch.Generator(device=dev)
            gen.manual_seed(0)

            def batches(k):
                ids = torch.randint(0, 6 * VIEW, (TUNE_BATCH,), generator=gen, device=dev)
                return Rays(*[t[ids].contiguous() for t in every]), targets[ids].contiguous()
            key = f"{target_name}_tv{tv:g}"
            state, losses = pt.tune_field(baked, batches, 500, WHITE, tv_sigma=tv)
            res = {"after_500": score(baked)}
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            _, more = pt.tune_field(baked, batches, 1500, WHITE, state=state)
            e1.record()
            e1.synchronize()
            res["after_2000"] = score(baked)
            res["ms_per_step"] = e0.elapsed_time(e1) / 1500
            res["batch_loss"] = [float(losses[0]), float(losses[-1]), float(more[-1])]
            res["after_2000"]["march_ms"] = window(lambda: preview.march(baked, o, d, near, far, WHITE, out=bufs))[0]
            share = pt.reoccupy(baked, 0.5, dilate=1)
            res["reoccupied_0.5"] = dict(score(baked), occupied_fraction=share,
                                         march_ms=window(lambda: preview.march(baked, o, d, near, far, WHITE, out=bufs))[0])
            out[key] = res
            del state, baked
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--grids", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--only", choices=["rate", "quality"], default=None)
    ap.add_argument("--step", default=None, help="internal: run one point (rate:GRID:DEGREE or quality:GRID:BAKE) in this process")
    ap.add_argument("--step_timeout", type=int, default=420)
    args = ap.parse_args()
    if args.step:
        kind, grid, what = args.step.split(":")
        print("RESULT " + json.dumps(step_rate(int(grid), int(what)) if kind == "rate" else step_quality(int(grid), what)))
        return 0
    points = []
    if args.only != "quality":
        points += [(f"rate_g{g}_d{deg}", f"rate:{g}:{deg}") for g in args.grids for deg in (0, 1, 2)]
    if args.only != "rate":
        points += [(f"quality_g{g}_{b}", f"quality:{g}:{b}") for g in args.grids for b in ("t0.5", "t0")]
    res = {}
    if args.json and os.path.exists(args.json):
        with open(args.json) as f:
            res = json.load(f)
    for name, st in points:
        try:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", st], capture_output=True, text=True,
                               timeout=args.step_timeout)
        except subprocess.TimeoutExpired:
            print(f"{st}: time limit of {args.step_timeout} s; nothing more is started", file=sys.stderr)
            return 1
        if p.returncode != 0:
            print(f"{st}: exit status {p.returncode}; nothing more is started\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}", file=sys.stderr)
            return 1
        res[name] = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
        print(name, json.dumps(res[name]), flush=True)
        if args.json:
            os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
            with open(args.json, "w") as f:
                json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
