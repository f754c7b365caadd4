#!/usr/bin/env python3
"""Measure the box shrink of captured images: `ops.area_downscale` for 100 images of 1297 x 840 x 3 at factor 4 and of
800 x 800 x 3 at factor 2 (HIP events around single launches: warm-up, then --repeats timed launches; median, min, max; inputs
resident), each alternated in the same loop with a plain device copy that moves the same number of bytes, and with --loader the wall
time of the loader's images/ fallback (`datasets.RealData360` on a written capture of 100 JPEGs of 1297 x 840) split into decode /
upload / kernel.

    python scripts/downscale_bw.py [--repeats 30] [--loader] [--json FILE]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(1, os.path.join(REPO, "tests"))

CASES = ((100, 840, 1297, 3, 4), (100, 800, 800, 3, 2))          # images, height, width, channels, factor


def event_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def summary(ms, moved):
    med = statistics.median(ms)
    return dict(median_ms=med, min_ms=min(ms), max_ms=max(ms), repeats=len(ms), bytes=moved, tb_per_s_median=moved / med / 1e9,
                tb_per_s_best=moved / min(ms) / 1e9)


def measure(ops, dev, n, H, W, C, F, repeats):
    gen = torch.Generator(device=dev).manual_seed(0)
    src = torch.randint(0, 256, (n, H, W, C), dtype=torch.uint8, device=dev, generator=gen)
    h, w = H // F, W // F
    out = torch.empty(n * h * w, 3, dtype=torch.float32, device=dev)
    moved = n * (H * W * C + 12 * h * w)                        # every source byte read once, every row written once
    a = torch.empty(moved // 8, dtype=torch.float32, device=dev).fill_(1.0)       # a copy that moves the same bytes (read + write)
    b = torch.empty_like(a)
    kernel, copy = (lambda: ops.area_downscale(src, F, out)), (lambda: b.copy_(a))
    for _ in range(5):
        kernel()
        copy()
    torch.cuda.synchronize()
    k_ms, c_ms = [], []
    for _ in range(repeats):                                    # alternated: both see the same clocks and the same neighbours
        k_ms.append(event_ms(kernel))
        c_ms.append(event_ms(copy))
    res = dict(images=n, height=H, width=W, channels=C, factor=F, kernel=summary(k_ms, moved), device_copy=summary(c_ms, 2 * a.numel() * 4))
    res["fraction_of_copy"] = res["kernel"]["tb_per_s_median"] / res["device_copy"]["tb_per_s_median"]
    return res


def write_capture(root, n, H, W):
    """An LLFF directory with images/ only: n JPEGs of smooth colour + noise (decode cost of a photograph, not of white noise)."""
    import dataset_fixture as fx
    from PIL import Image
    fx.write_llff(root, seed=3, n=n, w=2, h=2, factor=1)          # poses, bounds and the camera file; its 2 x 2 images are replaced
    os.rename(os.path.join(root, "images_1"), os.path.join(root, "images"))
    rng = np.random.RandomState(0)
    y, x = np.mgrid[0:H, 0:W]
    for i, f in enumerate(sorted(os.listdir(os.path.join(root, "images")))):
        os.remove(os.path.join(root, "images", f))
        base = np.stack([np.sin(x / 97.0 + i) * np.cos(y / 61.0), np.sin(y / 83.0 - i), np.cos((x + y) / 120.0 + 0.3 * i)], -1)
        img = np.clip(127.5 + 100.0 * base + rng.normal(0.0, 12.0, size=(H, W, 3)), 0, 255).astype(np.uint8)
        Image.fromarray(img).save(os.path.join(root, "images", f[:-4] + ".jpg"), quality=92)
    return root


def measure_loader(ops, dev, n, H, W, F):
    from mipnerf_pl_amd import datasets as D
    with tempfile.TemporaryDirectory() as tmp:
        root = write_capture(os.path.join(tmp, "capture"), n, H, W)
        files, _, shrink = D.realdata360_files(root, "train", F)
        assert shrink
        t0 = time.perf_counter()
        frames = D.decode_u8(files)
        t1 = time.perf_counter()
        src = torch.from_numpy(frames).to(dev)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        ops.area_downscale(src, F)
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        del src
        ds = D.RealData360(root, split="train", factor=F, device=dev)
        torch.cuda.synchronize()
        t4 = time.perf_counter()
        return dict(images_in_split=len(files), height=H, width=W, factor=F, decode_s=t1 - t0, upload_s=t2 - t1, kernel_s=t3 - t2,
                    dataset_wall_s=t4 - t3, pixels=ds.num_pixels, host_threads=min(16, len(files)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--loader", action="store_true")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    from mipnerf_pl_amd import ops
    dev = torch.device("cuda:0")
    res = dict(device=torch.cuda.get_device_name(0), cases=[measure(ops, dev, *c, args.repeats) for c in CASES])
    if args.loader:
        n, H, W, _, F = CASES[0]
        res["loader"] = measure_loader(ops, dev, n, H, W, F)
    print(json.dumps(res))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
