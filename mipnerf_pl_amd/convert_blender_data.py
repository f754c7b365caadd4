"""Blender scenes -> the multi-scale data set (datasets/convert_blender_data.py of the reference), pyramid on the device.

    python -m mipnerf_pl_amd.convert_blender_data --blender_dir nerf_synthetic --out_dir multiscale [--object_name lego]
                                                  [--n_down 4] [--device cuda:0] [--workers 16]

Per scene and split (train, val, test): `transforms_{split}.json` and its RGBA PNGs are read, the decoded frames go to the device
in batches of bounded size, `ops.box_pyramid` (kernels_pyramid.hip) makes every level of every frame in one launch, and the
bytes come back to be written as `images_{split}/{i:03d}_d{j}.png`; one `metadata.json` per scene with the reference's keys, key
order, nesting and values.  PNG decoding / encoding stays on the host (`--workers` threads, at most 16); the metadata is float64
host arithmetic exactly as in the reference.  `datasets.Multicam` reads the result -- or skips the files altogether
(`Multicam.from_blender`, used automatically when `--data_path` is a Blender directory).

The reference keeps the pyramid in float32 from level to level and writes each level with a truncating np.uint8(img * 255); the
kernel follows its summation order, so the PNGs decode to the same bytes (tests/golden/pyramid_48x40.npz)."""
import argparse
import json
import os
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

SPLITS = ("train", "val", "test")
MAX_WORKERS = 16
BATCH_BYTES = 64 << 20          # decoded source bytes per upload; the device holds ~5.3 x this (bytes + float32 rows of all levels)
NEAR, FAR = 2.0, 6.0


def read_transforms(basedir, split):
    """(PNG paths, camera-to-world matrices as nested lists, camera_angle_x) of one split (convert_blender_data.py:10-31)."""
    with open(os.path.join(basedir, f"transforms_{split}.json")) as fp:
        meta = json.load(fp)
    files = [os.path.join(basedir, fr["file_path"] + ".png") for fr in meta["frames"]]
    return files, [fr["transform_matrix"] for fr in meta["frames"]], float(meta["camera_angle_x"])


def check_frames(files, n_down):
    """(height, width) shared by `files`, read from the PNG headers; ValueError naming the file when a frame is not RGBA, differs in
    size from the first one (the reference fails in np.stack) or does not halve exactly n_down - 1 times (it fails in reshape)."""
    from PIL import Image
    from . import _lib as L
    if not 1 <= int(n_down) <= L.MAX_PYRAMID_LEVELS:
        raise ValueError(f"n_down must be in [1, {L.MAX_PYRAMID_LEVELS}], got {n_down}")
    t = 1 << (int(n_down) - 1)
    size = None
    for f in files:
        with Image.open(f) as im:
            w, h, mode = im.width, im.height, im.mode
        if mode != "RGBA":
            raise ValueError(f"{f}: expected an RGBA image, got mode {mode}")
        if h % t or w % t:
            raise ValueError(f"{f}: {w} x {h} is not divisible by 2^(n_down-1) = {t}; {n_down} levels cannot be made")
        if size is not None and (h, w) != size:
            raise ValueError(f"{f}: {w} x {h} differs from the first frame's {size[1]} x {size[0]}")
        size = (h, w)
    if size is None:
        raise ValueError("no frames")
    return size


def split_metadata(split, cams, height, width, camera_angle_x, n_down):
    """The `metadata.json` entry of one split (convert_blender_data.py:53-107), float64 as there."""
    focal = .5 * width / np.tan(.5 * camera_angle_x)
    meta = {k: [] for k in ("file_path", "cam2world", "width", "height", "focal", "label", "near", "far", "lossmult")}
    for i, cam in enumerate(cams):
        c2w = np.asarray(cam, dtype=np.float64).tolist()
        for j in range(n_down):
            meta["file_path"].append("images_{}/{:03d}_d{}.png".format(split, i, j))
            meta["cam2world"].append(c2w)
            meta["width"].append(width >> j)
            meta["height"].append(height >> j)
            meta["focal"].append(focal / 2 ** j)
            meta["label"].append(j)
            meta["near"].append(NEAR)
            meta["far"].append(FAR)
            meta["lossmult"].append(4. ** j)
    f = np.array(meta["focal"])
    cx, cy = np.array(meta["width"]) * .5, np.array(meta["height"]) * .5
    zero, one = np.zeros_like(cx), np.ones_like(cx)
    k_inv = np.array([[one / f, zero, -cx / f],
                      [zero, -one / f, cy / f],
                      [zero, zero, -one]])
    meta["pix2cam"] = np.moveaxis(k_inv, -1, 0).tolist()
    return meta


def scene_metadata(basedir, n_down):
    """{split: metadata} of a Blender scene directory and {split: PNG paths}; every frame is checked before anything is computed."""
    metas, files = {}, {}
    for split in SPLITS:
        files[split], cams, angle = read_transforms(basedir, split)
        h, w = check_frames(files[split], n_down)
        metas[split] = split_metadata(split, cams, h, w, angle, n_down)
    return metas, files


def _decode(fname):
    from PIL import Image
    with open(fname, "rb") as fp:
        a = np.array(Image.open(fp))
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 4:
        raise ValueError(f"{fname}: expected 8-bit RGBA, got {a.dtype} {a.shape}")
    return a


def _encode(job):
    from PIL import Image
    fname, arr = job
    with open(fname, "wb") as fp:
        Image.fromarray(arr).save(fp)


def _workers(workers):
    return max(1, min(int(workers), MAX_WORKERS))


def frame_batches(files, height, width, pool):
    """Decoded frames [n_b, H, W, 4] uint8 in order, at most BATCH_BYTES each: (index of the first frame, array)."""
    per = max(1, BATCH_BYTES // (height * width * 4))
    for lo in range(0, len(files), per):
        yield lo, np.stack(list(pool.map(_decode, files[lo:lo + per])))


def convert_to_nerfdata(basedir, newdir, n_down, device=None, workers=MAX_WORKERS, stats=None):
    """One scene (convert_blender_data.py:40-117).  `stats` (a dict) receives the seconds spent in decode / device / encode."""
    import torch
    from . import ops
    device = torch.device(device if device is not None else "cuda")
    if device.type != "cuda":
        raise RuntimeError("convert_blender_data: the pyramid is made by the HIP kernel; need a HIP device (there is no host fallback)")
    metas, files = scene_metadata(basedir, n_down)              # raises before anything is written
    t = dict(decode=0.0, device=0.0, encode=0.0)
    os.makedirs(newdir, exist_ok=True)
    with ThreadPoolExecutor(_workers(workers)) as pool, torch.cuda.device(device):
        for split in SPLITS:
            print("Split", split)
            os.makedirs(os.path.join(newdir, f"images_{split}"), exist_ok=True)
            h, w = metas[split]["height"][0], metas[split]["width"][0]
            batches = frame_batches(files[split], h, w, pool)
            while True:
                t0 = time.perf_counter()
                item = next(batches, None)
                t1 = time.perf_counter()
                t["decode"] += t1 - t0
                if item is None:
                    break
                lo, frames = item
                levels, _ = ops.box_pyramid(torch.from_numpy(frames).to(device), n_down)
                levels = [lv.cpu().numpy() for lv in levels]          # synchronises
                t2 = time.perf_counter()
                t["device"] += t2 - t1
                jobs = [(os.path.join(newdir, metas[split]["file_path"][(lo + i) * n_down + j]), levels[j][i])
                        for i in range(frames.shape[0]) for j in range(n_down)]
                list(pool.map(_encode, jobs))
                t["encode"] += time.perf_counter() - t2
    with open(os.path.join(newdir, "metadata.json"), "w") as fp:
        json.dump(metas, fp, ensure_ascii=False, indent=4)
    if stats is not None:
        for k, v in t.items():
            stats[k] = stats.get(k, 0.0) + v
    return t


def main(argv=None):
    parser = argparse.ArgumentParser(prog="python -m mipnerf_pl_amd.convert_blender_data", description=__doc__.split("\n\n")[0])
    parser.add_argument("--blender_dir", help="data root path", type=str, required=True)
    parser.add_argument("--object_name", help="Which object you want to make multi scale (default: every scene directory)", type=str, default=None)
    parser.add_argument("--out_dir", help="Output directory.", type=str, required=True)
    parser.add_argument("--n_down", help="Number of scales you want to make.", type=int, default=4)
    parser.add_argument("--device", help="HIP device that runs the pyramid kernel", type=str, default="cuda:0")
    parser.add_argument("--workers", help=f"host threads for PNG decode / encode (at most {MAX_WORKERS})", type=int, default=MAX_WORKERS)
    args = parser.parse_args(argv)
    os.makedirs(args.out_dir, exist_ok=True)
    scenes = os.listdir(args.blender_dir) if args.object_name is None else [args.object_name]
    dirs = [d for d in (os.path.join(args.blender_dir, f) for f in sorted(scenes)) if os.path.isdir(d)]
    print(dirs)
    stats = {}
    t0 = time.perf_counter()
    for basedir in dirs:
        newdir = os.path.join(args.out_dir, os.path.basename(basedir))
        print("Converting from", basedir, "to", newdir)
        convert_to_nerfdata(basedir, newdir, args.n_down, device=args.device, workers=args.workers, stats=stats)
    print("done in {:.2f} s: decode {:.2f} s, device (upload, kernel, download) {:.2f} s, encode {:.2f} s".format(
        time.perf_counter() - t0, stats.get("decode", 0.0), stats.get("device", 0.0), stats.get("encode", 0.0)))
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
