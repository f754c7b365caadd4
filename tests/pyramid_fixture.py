"""Inputs and the stated rule of the multi-scale converter tests (TEST INFRASTRUCTURE, shared by scripts/make_golden_pyramid.py,
tests/test_pyramid_cpu.py and tests/test_gpu_pyramid.py).

Two Blender-format roots: `random` = dataset_fixture.write_blender(seed=5, w=48, h=40) (random RGBA bytes; 40 -> 20 -> 10 -> 5
rows, so four levels is the deepest legal pyramid), `binary` = the same frames and poses with alpha forced to 0 / 255 on 70 % of
the pixels (what a rendered Blender frame looks like: mostly empty or opaque)."""
import glob
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import dataset_fixture as fx  # noqa: E402

W, H, N_DOWN, SEED = 48, 40, 4, 5
ROOTS = ("random", "binary")
SPLITS = ("train", "val", "test")


def binarise_alpha(root, seed=6, share=0.7):
    """Rewrite every PNG below `root` (sorted order) with alpha = 0 or 255 on `share` of its pixels."""
    from PIL import Image
    rng = np.random.RandomState(seed)
    for f in sorted(glob.glob(os.path.join(root, "*", "*.png"))):
        a = np.array(Image.open(f))
        hit = rng.rand(*a.shape[:2]) < share
        a[..., 3] = np.where(hit, np.where(rng.rand(*a.shape[:2]) < 0.5, 0, 255), a[..., 3]).astype(np.uint8)
        Image.fromarray(a).save(f)
    return root


def write_roots(tmp):
    """{name: Blender directory} of the two roots below `tmp`."""
    out = {"random": fx.write_blender(os.path.join(str(tmp), "random", "scene"), seed=SEED, w=W, h=H)}
    out["binary"] = binarise_alpha(fx.write_blender(os.path.join(str(tmp), "binary", "scene"), seed=SEED, w=W, h=H))
    return out


def read_frames(root, split):
    """[n, H, W, 4] uint8: the frames of one split in transforms order."""
    import json
    from PIL import Image
    with open(os.path.join(root, f"transforms_{split}.json")) as fp:
        meta = json.load(fp)
    return np.stack([np.array(Image.open(os.path.join(root, fr["file_path"] + ".png"))) for fr in meta["frames"]])


def rule_pyramid(src_u8, n_levels):
    """The converter's rule restated in numpy: float32 level 0 = byte / 255; the next level is the mean of each 2 x 2 block of the
    UNQUANTISED level, summed ((p00 + p01) + p10) + p11 in float32 and divided by 4; every level is written as trunc(v * 255).
    src_u8 [..., H, W, 4] -> list of uint8 [..., H / 2^j, W / 2^j, 4]."""
    v = src_u8.astype(np.float32) / np.float32(255.0)
    out = []
    for j in range(n_levels):
        out.append((v * np.float32(255.0)).astype(np.uint8))
        if j + 1 < n_levels:
            p00, p01, p10, p11 = v[..., 0::2, 0::2, :], v[..., 0::2, 1::2, :], v[..., 1::2, 0::2, :], v[..., 1::2, 1::2, :]
            v = (((p00 + p01) + p10) + p11) / np.float32(4.0)
    return out


def rule_pixels(levels_u8, white_bkgd):
    """What load_multicam makes of the written bytes: [n, P_img, 3] float32 per image (levels of one image concatenated)."""
    rows = []
    for lv in levels_u8:
        q = lv.astype(np.float32) / np.float32(255.0)
        rgb = q[..., :3] * q[..., 3:] + (np.float32(1.0) - q[..., 3:]) if white_bkgd else q[..., :3]
        rows.append(rgb.reshape(lv.shape[0], -1, 3))
    return np.concatenate(rows, axis=1)
