#!/usr/bin/env python3
"""Measure tuning the baked preview's lattice on one MI355X, on the scene, the trained field and the helpers the other
preview rate scripts use (the golden pose at 800 x 800, tests/golden/trained_field.npz, bf16 bake):

  grad_g<grid>_d<degree>   k_preview_tune_grad on a batch of 65,536 uniformly drawn rays of the golden frame, target = the MLP's render of
                 those rays: kernel time (HIP events around repeated calls, warm, the median of 11 windows of at least 30 ms), the march
                 alone on the same rays beside it, the samples and flushes of the debug counters, atomic wave instructions and added bytes
                 per second (a flush is 1 / 2 / 4 instructions; an instruction carries 4 bytes per active lane),
  adam_g<grid>_d<degree>   k_preview_tune_adam with the point mask and without, against a device copy of the bytes the unmasked pass moves,
  step_g<grid>_d<degree>   wall time of `TuneState.step` (gradient + Adam + the loss) on the same batch,
  quality_g<grid>_p<poses> degree 1: `--tune`'s loop (target = the MLP, random pixels of the EVEN poses of a <poses>-pose spherical path
                 at scale 4) for 500 and 2000 steps; PSNR of the tuned and the untuned lattice on at most 12 of the ODD (held-out) poses and
                 on at most 6 of the poses tuned on, against the MLP's frames AND against the scene: the field was trained on the procedural
                 scene of tests/dataset_fixture.py, whose float64 quadrature (`_render_scene`, the one behind the golden frame's `gt_u8`)
                 gives ground truth along any frame's rays,
  photos_g<grid>_p<poses>  the same lattice, poses and figures with target = the photos: `photo_batches` on the train split the field was
                 trained on (`write_multicam_scene`: 24 random views at 64, 32, 16 and 8 pixels), the default of `--tune --data`.

Every GPU step is a child process under its own time limit; the first one that fails ends the run.

    python scripts/preview_tune_rate.py [--json profiles/preview_tune_rate.json] [--steps grad_g256_d0,...]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE_REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WINDOWS = 11
MIN_WINDOW_MS = 30.0
BATCH = 65536
STEPS = "grad_g256_d0,grad_g256_d1,grad_g256_d2,adam_g256_d1,step_g256_d1,quality_g128_p24,quality_g256_p24,quality_g256_p120,photos_g128_p24,photos_g256_p24"


def _window(call):
    """median ms per call over WINDOWS windows of at least MIN_WINDOW_MS, HIP events around the calls of a window"""
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
    reps = max(1, int(MIN_WINDOW_MS / max(timed(3), 1e-3)) + 1)
    times = [timed(reps) for _ in range(WINDOWS)]
    return dict(ms=statistics.median(times), ms_min=min(times), ms_max=max(times), calls_per_window=reps)


def _scene(grid, degree):
    import torch
    from mipnerf_pl_amd import preview
    from mipnerf_pl_amd.evaluate import cull_box
    from scripts.cull_rate import DEV, golden_pose_rays
    from scripts.span_rate import trained_model
    flat, frame, _, N = golden_pose_rays()
    model, bound = trained_model("bf16", N), cull_box([frame], grid)
    with torch.no_grad():
        baked = preview.bake_field(model, grid=grid, degree=degree, lo=-bound, hi=bound)
    return torch.device(DEV), model, baked, flat


def _batch(model, flat, dev):
    """BATCH uniformly drawn rays of the golden frame and the MLP's render of them"""
    import torch
    from mipnerf_pl_amd import Rays
    from mipnerf_pl_amd.evaluate import DEFAULT_CHUNK
    from mipnerf_pl_amd.model import GraphedFrame
    gen = torch.Generator(device=dev)
    gen.manual_seed(0)
    ids = torch.randint(0, flat.origins.shape[0], (BATCH,), generator=gen, device=dev)
    rays = Rays(*[t[ids].contiguous() for t in flat])
    with torch.no_grad():
        target = GraphedFrame(model, BATCH, DEFAULT_CHUNK, True, dev, capture=False)(rays)[1].clone()
    return rays, target


def step_grad(grid, degree):
    import torch
    from mipnerf_pl_amd import preview
    dev, model, baked, flat = _scene(grid, degree)
    rays, target = _batch(model, flat, dev)
    o, d = rays.origins.float().contiguous(), rays.directions.float().contiguous()
    near, far = rays.near.reshape(-1).float().contiguous(), rays.far.reshape(-1).float().contiguous()
    grad = torch.zeros(baked.rows.shape, dtype=torch.float32, device=dev)
    out = (torch.empty(BATCH, 3, device=dev), torch.empty(BATCH, device=dev))
    counters = torch.zeros(2, dtype=torch.int64, device=dev)
    scale = 2.0 / (3.0 * BATCH)
    preview.march_grad(baked, o, d, near, far, True, target=target, loss_scale=scale, grad_rows=grad, out=out, counters=counters)
    torch.cuda.synchronize()
    samples, flushes = counters.tolist()
    steps = torch.zeros(BATCH, dtype=torch.int32, device=dev)
    march_out = (torch.empty(BATCH, 3, device=dev), torch.empty(BATCH, device=dev), torch.empty(BATCH, device=dev))
    preview.march(baked, o, d, near, far, True, out=march_out, steps=steps)
    t_grad = _window(lambda: preview.march_grad(baked, o, d, near, far, True, target=target, loss_scale=scale, grad_rows=grad, out=out))
    t_march = _window(lambda: preview.march(baked, o, d, near, far, True, out=march_out))
    per_flush = {0: 1, 1: 2, 2: 4}[degree]
    used = 1 + 3 * (degree + 1) ** 2
    added = flushes * 8 * used * 4                                  # 8 corner rows, the used entries, 4 bytes
    evaluated = int(steps.sum(dtype=torch.int64))
    return dict(grid=grid, degree=degree, rays=BATCH, tune_grad=t_grad, march_alone=t_march, evaluated_samples=evaluated,
                contributing_samples=samples, flushes=flushes, flushes_per_sample=flushes / max(samples, 1),
                atomic_instructions=flushes * per_flush, atomic_instructions_per_sample=flushes * per_flush / max(samples, 1),
                atomic_instructions_per_sample_without_combining=per_flush, added_bytes=added,
                added_GB_per_s=added / (t_grad["ms"] * 1e-3) / 1e9, samples_per_s=samples / (t_grad["ms"] * 1e-3),
                same_rgb_as_march=bool(torch.equal(out[0], march_out[0]) and torch.equal(out[1], march_out[1])),
                rays_with_gradient=int(((out[0] - target) != 0).any(-1).sum()))


def step_adam(grid, degree):
    import torch
    from mipnerf_pl_amd import preview
    dev, model, baked, flat = _scene(grid, degree)
    state = preview.TuneState(baked)
    W = baked.rows.shape[-1]
    n = baked.rows.numel() // W
    used = 1 + 3 * (degree + 1) ** 2
    moved = n * used * (4 * 4 * 2 + 2)                               # master, m, v, grad read and written; rows written
    src = torch.empty(moved // 2, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    args = (state.lr_sigma, state.lr_colour, 0.9, 0.999, 1e-8, 10.0, 1000.0)
    t_mask = _window(lambda: preview.tune_adam(state.master, state.m, state.v, state.grad, baked.rows, degree, state.mask, *args))
    t_all = _window(lambda: preview.tune_adam(state.master, state.m, state.v, state.grad, baked.rows, degree, None, *args))
    t_copy = _window(lambda: dst.copy_(src))
    return dict(grid=grid, degree=degree, points=n, masked_in_share=float(state.mask.float().mean()), bytes_moved_unmasked=moved,
                adam_masked=t_mask, adam_unmasked=t_all, device_copy_same_bytes=t_copy, unmasked_over_copy=t_all["ms"] / t_copy["ms"],
                masked_over_unmasked=t_mask["ms"] / t_all["ms"], unmasked_GB_per_s=moved / (t_all["ms"] * 1e-3) / 1e9)


def step_step(grid, degree):
    import torch
    from mipnerf_pl_amd import preview
    dev, model, baked, flat = _scene(grid, degree)
    rays, target = _batch(model, flat, dev)
    state = preview.TuneState(baked, lr_sigma=0.0, lr_colour=0.0)          # timing only: the lattice stays what it is
    for _ in range(3):
        state.step(rays, target, True)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(50):
        state.step(rays, target, True)
    torch.cuda.synchronize()
    return dict(grid=grid, degree=degree, rays=BATCH, ms_per_step=1e3 * (time.perf_counter() - t0) / 50)


def _path_setup(grid, n_poses):
    """The <n_poses>-pose spherical path at scale 4, the trained field, the held-out (ODD) and tuned-on (EVEN) poses that are measured, the
    MLP's frames of them and the SCENE's: `dataset_fixture._render_scene`, the float64 quadrature of the procedural scene the field was
    trained on, along each frame's own rays, composited on white and rounded to 8 bits as the golden frame's `gt_u8` is."""
    from concurrent.futures import ThreadPoolExecutor
    import dataset_fixture as fx
    import numpy as np
    import torch
    from mipnerf_pl_amd.datasets import RenderGen
    from mipnerf_pl_amd.evaluate import DEFAULT_CHUNK, FrameEvaluator, cull_box
    from scripts.cull_rate import DEV
    from scripts.span_rate import trained_model
    g = np.load(os.path.join(HERE_REPO, "tests", "golden", "frame_c5_800x800.npz"))
    dev = torch.device(DEV)
    size = int(g["cfg_size"]) // 4
    path = RenderGen(float(g["focal"]) / 4, [size, size], scales=1, device=dev, n_poses=n_poses)
    model = trained_model("bf16", int(g["cfg_num_samples"]))
    frames = [path[i] for i in range(len(path))]
    bound = cull_box(frames, grid)
    odd, even = list(range(1, len(path), 2)), list(range(0, len(path), 2))
    held, seen = odd[::max(1, len(odd) // 12)][:12], even[::max(1, len(even) // 6)][:6]
    with torch.no_grad():
        ev = FrameEvaluator(model, size, size, DEFAULT_CHUNK, True, dev)
        mlp = {i: ev.render(frames[i])[0].clone() for i in held + seen}
    def scene_frame(od):
        gt = np.empty((size, size, 3), np.float64)
        for r0 in range(0, size, 40):
            rgb, alpha = fx._render_scene(od[0][r0:r0 + 40], od[1][r0:r0 + 40], float(path.near), float(path.far))
            gt[r0:r0 + 40] = rgb * alpha[..., None] + (1.0 - alpha[..., None])
        return np.round(255.0 * np.clip(gt, 0, 1)).astype(np.float32) / 255.0
    rays = [(frames[i].origins.double().cpu().numpy(), frames[i].directions.double().cpu().numpy()) for i in held + seen]
    with ThreadPoolExecutor(max_workers=8) as pool:              # numpy on the host: a few seconds per frame
        scene = {i: torch.from_numpy(img).to(dev) for i, img in zip(held + seen, pool.map(scene_frame, rays))}
    info = dict(grid=grid, degree=1, image=size, poses=len(path), train_poses=len(even), held_out_poses_measured=len(held),
                train_poses_measured=len(seen), batch=BATCH, bound=bound)
    return dev, model, path, frames, bound, even, held, seen, mlp, scene, size, info


def _tune_and_score(out, model, baked, batches, frames, held, seen, mlp, scene, size):
    """500 and 2000 steps of `tune_field` on `batches`; the PSNR of the untuned and the tuned lattice against the MLP's frames and against
    the scene's, on the held-out poses and on the poses `seen`; the MLP's own PSNR against the scene beside them."""
    import numpy as np
    import torch
    from mipnerf_pl_amd import ops, preview
    mean = lambda img, ref, ids: float(np.mean([float(ops.eval_errors(img[i], ref[i])[0]) for i in ids]))  # noqa: E731

    def psnr(baked):
        fr = preview.PreviewFrame(baked, size, size, True)
        got = {i: fr.render(frames[i])[0].clone() for i in held + seen}
        return dict(vs_mlp=dict(held_out=mean(got, mlp, held), tuned_on=mean(got, mlp, seen)),
                    vs_scene=dict(held_out=mean(got, scene, held), tuned_on=mean(got, scene, seen)))
    with torch.no_grad():
        out["mlp_vs_scene_psnr"] = dict(held_out=mean(mlp, scene, held), tuned_on=mean(mlp, scene, seen))
        out["untuned_psnr"] = psnr(baked)
        state, done = None, 0
        for total in (500, 2000):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            state, losses = preview.tune_field(baked, lambda k, base=done: batches(base + k), total - done, True, state=state)
            torch.cuda.synchronize()
            out[f"steps_{total}"] = dict(tuned_psnr=psnr(baked), seconds_for_these_steps=time.perf_counter() - t0,
                                         first_batch_loss=float(losses[0]), last_batch_loss=float(losses[-1]))
            done = total
    return out


def step_quality(grid, n_poses):
    import torch
    from mipnerf_pl_amd import preview
    dev, model, path, frames, bound, even, held, seen, mlp, scene, size, out = _path_setup(grid, n_poses)
    with torch.no_grad():
        baked = preview.bake_field(model, grid=grid, degree=1, lo=-bound, hi=bound)
    batches = preview.mlp_batches(model, preview.PathPixels(path, frames=even), BATCH, 0, True)
    out["target"] = "mlp, random pixels of the even poses of the path"
    return _tune_and_score(out, model, baked, batches, frames, held, seen, mlp, scene, size)


def step_photos(grid, n_poses):
    import tempfile
    import dataset_fixture as fx
    import torch
    from mipnerf_pl_amd import preview
    from mipnerf_pl_amd.datasets import Multicam
    dev, model, path, frames, bound, even, held, seen, mlp, scene, size, out = _path_setup(grid, n_poses)
    with tempfile.TemporaryDirectory() as root:
        train = Multicam(fx.write_multicam_scene(root), "train", True, "all_images", device=dev)
    with torch.no_grad():
        baked = preview.bake_field(model, grid=grid, degree=1, lo=-bound, hi=bound)
    out.update(target="photos: the train split the field was trained on (24 views at 64, 32, 16 and 8 pixels, all four sizes drawn alike)",
               train_pixels=int(train.num_pixels))
    out["note"] = "no pose of the path is in the train split: 'tuned_on' names the same even poses as the quality steps, all held out here"
    return _tune_and_score(out, model, baked, preview.photo_batches(train, BATCH, 0), frames, held, seen, mlp, scene, size)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--step", default=None, help="internal: run one step in this process and print its JSON")
    ap.add_argument("--steps", default=STEPS, help="comma-separated steps")
    ap.add_argument("--step_timeout", type=int, default=300)
    args = ap.parse_args()
    if args.step:
        sys.path.insert(0, HERE_REPO)
        sys.path.insert(1, os.path.join(HERE_REPO, "tests"))
        kind, *rest = args.step.split("_")
        nums = [int(r[1:]) for r in rest]
        fn = dict(grad=step_grad, adam=step_adam, step=step_step, quality=step_quality, photos=step_photos)[kind]
        print("RESULT " + json.dumps(fn(*nums)))
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
