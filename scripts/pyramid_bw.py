#!/usr/bin/env python3
"""Measure the multi-scale converter: the pyramid kernel's time and achieved bytes/s for 100 frames of 800 x 800 at
four levels (HIP events around single launches: warm-up, then --repeats timed launches; median, min, max), next to a plain device copy
of the same footprint on the same box in the same run, and with --command the wall time of `convert_blender_data` on the test
fixture scaled up to 100 + 100 + 200 frames of 800 x 800 with its decode / device / encode split.

    python scripts/pyramid_bw.py [--frames 100] [--size 800] [--levels 4] [--repeats 30] [--command] [--json FILE]
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


def timed(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms), repeats=repeats)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--size", type=int, default=800)
    ap.add_argument("--levels", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--command", action="store_true")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    from mipnerf_pl_amd import ops
    dev = torch.device("cuda:0")
    n, s, lv = args.frames, args.size, args.levels
    ppi = sum((s >> j) ** 2 for j in range(lv))
    gen = torch.Generator(device=dev).manual_seed(0)
    src = torch.randint(0, 256, (n, s, s, 4), dtype=torch.uint8, device=dev, generator=gen)
    out_u8 = torch.empty(4 * n * ppi, dtype=torch.uint8, device=dev)
    out_rgb = torch.empty(n * ppi, 3, dtype=torch.float32, device=dev)
    res = dict(frames=n, size=s, levels=lv, device=torch.cuda.get_device_name(0))
    for tag, rgb in (("bytes_and_rows", out_rgb), ("bytes_only", None)):
        moved = n * (4 * s * s + 4 * ppi + (12 * ppi if rgb is not None else 0))             # read once, every output written once
        r = timed(lambda: ops.box_pyramid(src, lv, white_bkgd=True if rgb is not None else None, out_u8=out_u8, out_rgb=rgb), 5, args.repeats)
        r.update(bytes=moved, tb_per_s_median=moved / r["median_ms"] / 1e9, tb_per_s_best=moved / r["min_ms"] / 1e9)
        res[tag] = r
    a = torch.empty(n * (2 * s * s + 8 * ppi) // 4, dtype=torch.float32, device=dev).fill_(1.0)   # copy of the same footprint (read + write)
    b = torch.empty_like(a)
    r = timed(lambda: b.copy_(a), 5, args.repeats)
    moved = 2 * a.numel() * 4
    r.update(bytes=moved, tb_per_s_median=moved / r["median_ms"] / 1e9, tb_per_s_best=moved / r["min_ms"] / 1e9)
    res["device_copy"] = r
    del a, b, src, out_u8, out_rgb
    if args.command:
        import dataset_fixture as fx
        from mipnerf_pl_amd import convert_blender_data as conv
        with tempfile.TemporaryDirectory() as tmp:
            t0 = time.perf_counter()
            root = fx.write_blender(os.path.join(tmp, "in", "scene"), seed=5, counts=(("train", 100), ("val", 100), ("test", 200)), w=s, h=s)
            res["fixture_write_s"] = time.perf_counter() - t0
            stats = {}
            t0 = time.perf_counter()
            conv.convert_to_nerfdata(root, os.path.join(tmp, "out", "scene"), lv, device=dev, stats=stats)
            res["command"] = dict(wall_s=time.perf_counter() - t0, frames=400, **stats)
    print(json.dumps(res))
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
