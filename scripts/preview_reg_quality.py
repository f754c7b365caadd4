#!/usr/bin/env python3
"""Does the regulariser recover what tuning the baked lattice loses on held-out poses?  The two failing experiments of
DESIGN 4.18, unchanged (the set-up, the poses, the batches and the scoring are scripts/preview_tune_rate.py's, by import), each repeated
with the regulariser on:

  quality_g<grid>_p<poses>  degree 1, tuned against the MLP on random pixels of the EVEN poses of a <poses>-pose spherical path at scale 4,
                 500 and 2000 steps; PSNR on at most 12 ODD (held-out) poses and at most 6 poses tuned on, against the MLP's frames and
                 against the scene,
  photos_g<grid>_p<poses>   the same lattice and figures, tuned against the photos of the train split the field was trained on.

Every configuration starts from the same bake (the rows are restored) and draws the same batches.  `none` is 4.18's run; `tv_sigma=X`,
`tv_colour=X`, `sh_decay=X` switch one weight on; `all=X` all three.  The weights are per tuned point, as `--tune_tv_sigma` etc. take them.
A 256^3 mlp step sweeps every weight over SWEEP, the other steps measure each weight at MID only.

Every GPU step is a child process under its own time limit; the first one that fails ends the run.

    python scripts/preview_reg_quality.py [--json profiles/preview_reg_quality.json] [--steps quality_g256_p24,...]
"""
import argparse
import json
import os
import subprocess
import sys
import time

HERE_REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = "quality_g256_p24,quality_g128_p24,photos_g256_p24,photos_g128_p24"
SWEEP = (1e-3, 1e-2, 1e-1)
MID = 1e-2
NAMES = ("tv_sigma", "tv_colour", "sh_decay")


def configs(full):
    out = [("none", {})]
    for name in NAMES:
        out += [(f"{name}={w:g}", {name: w}) for w in (SWEEP if full else (MID,))]
    return out + [(f"all={MID:g}", {name: MID for name in NAMES})]


def _score_all(out, baked, batches, frames, held, seen, mlp, scene, size, full):
    import numpy as np
    import torch
    from mipnerf_pl_amd import ops, preview
    mean = lambda img, ref, ids: float(np.mean([float(ops.eval_errors(img[i], ref[i])[0]) for i in ids]))  # noqa: E731

    def psnr():
        fr = preview.PreviewFrame(baked, size, size, True)
        got = {i: fr.render(frames[i])[0].clone() for i in held + seen}
        return dict(vs_mlp=dict(held_out=mean(got, mlp, held), tuned_on=mean(got, mlp, seen)),
                    vs_scene=dict(held_out=mean(got, scene, held), tuned_on=mean(got, scene, seen)))
    rows0 = baked.rows.clone()
    with torch.no_grad():
        out["mlp_vs_scene_psnr"] = dict(held_out=mean(mlp, scene, held), tuned_on=mean(mlp, scene, seen))
        out["untuned_psnr"] = psnr()
        out["runs"] = {}
        for name, kw in configs(full):
            baked.rows.copy_(rows0)
            state, done, res = None, 0, dict(weights=kw)
            for total in (500, 2000):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                state, losses = preview.tune_field(baked, lambda k, base=done: batches(base + k), total - done, True, state=state, **kw)
                torch.cuda.synchronize()
                res[f"steps_{total}"] = dict(tuned_psnr=psnr(), seconds_for_these_steps=time.perf_counter() - t0,
                                             first_batch_loss=float(losses[0]), last_batch_loss=float(losses[-1]))
                done, kw = total, {}                                  # (the state carries the weights from here on)
            res["tuned_points"] = state.n_points
            out["runs"][name] = res
            print(name, json.dumps(res), file=sys.stderr, flush=True)
    return out


def step_quality(grid, n_poses):
    import torch
    from mipnerf_pl_amd import preview
    from scripts.preview_tune_rate import BATCH, _path_setup
    dev, model, path, frames, bound, even, held, seen, mlp, scene, size, out = _path_setup(grid, n_poses)
    with torch.no_grad():
        baked = preview.bake_field(model, grid=grid, degree=1, lo=-bound, hi=bound)
    # one batch source per configuration: every run draws the same rays
    out["target"] = "mlp, random pixels of the even poses of the path"
    fresh = lambda: preview.mlp_batches(model, preview.PathPixels(path, frames=even), BATCH, 0, True)  # noqa: E731
    return _score_all(out, baked, _Restart(fresh), frames, held, seen, mlp, scene, size, grid == 256)


def step_photos(grid, n_poses):
    import tempfile
    import dataset_fixture as fx
    import torch
    from mipnerf_pl_amd import preview
    from mipnerf_pl_amd.datasets import Multicam
    from scripts.preview_tune_rate import BATCH, _path_setup
    dev, model, path, frames, bound, even, held, seen, mlp, scene, size, out = _path_setup(grid, n_poses)
    with tempfile.TemporaryDirectory() as root:
        train = Multicam(fx.write_multicam_scene(root), "train", True, "all_images", device=dev)
    with torch.no_grad():
        baked = preview.bake_field(model, grid=grid, degree=1, lo=-bound, hi=bound)
    out.update(target="photos: the train split the field was trained on (24 views at 64, 32, 16 and 8 pixels)", train_pixels=int(train.num_pixels))
    out["note"] = "no pose of the path is in the train split: 'tuned_on' names the same even poses as the quality steps, all held out here"
    return _score_all(out, baked, _Restart(lambda: preview.photo_batches(train, BATCH, 0)), frames, held, seen, mlp, scene, size, False)


class _Restart:
    """a batch source that starts its seeded draws again whenever step 0 is asked for: every configuration sees the same batches"""

    def __init__(self, fresh):
        self.fresh, self.draw = fresh, None

    def __call__(self, step):
        if step == 0 or self.draw is None:
            self.draw = self.fresh()
        return self.draw(step)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", default=None)
    ap.add_argument("--step", default=None, help="internal: run one step in this process and print its JSON")
    ap.add_argument("--steps", default=STEPS, help="comma-separated steps")
    ap.add_argument("--step_timeout", type=int, default=600)
    args = ap.parse_args()
    if args.step:
        sys.path.insert(0, HERE_REPO)
        sys.path.insert(1, os.path.join(HERE_REPO, "tests"))
        kind, *rest = args.step.split("_")
        nums = [int(r[1:]) for r in rest]
        print("RESULT " + json.dumps(dict(quality=step_quality, photos=step_photos)[kind](*nums)))
        return 0
    res = {}
    if args.json and os.path.exists(args.json):       # a run of some steps keeps the others' results
        with open(args.json) as f:
            res = json.load(f)
    for st in [s for s in args.steps.split(",") if s]:
        cmd = [sys.executable, os.path.abspath(__file__), "--step", st]
        try:
            p = subprocess.run(cmd, stdout=subprocess.PIPE, text=True, timeout=args.step_timeout, cwd=HERE_REPO)      # progress goes to stderr
        except subprocess.TimeoutExpired:
            print(f"{st}: time limit of {args.step_timeout} s; nothing more is started", file=sys.stderr)
            return 1
        if p.returncode != 0:
            print(f"{st}: exit status {p.returncode}; nothing more is started\n{p.stdout[-2000:]}", file=sys.stderr)
            return 1
        res[st] = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
        if args.json:                                 # kept step by step: a later step that fails loses nothing
            os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
            with open(args.json, "w") as f:
                json.dump(res, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
