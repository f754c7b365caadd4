"""A captured-scene directory as COLMAP / LLFF tooling leaves it -- `images/` only -- of the LEARNABLE unbounded procedural scene of
tests/dataset_fixture.py, and the stated rule of the device box shrink (TEST INFRASTRUCTURE, shared by tests/test_scene360_cli_cpu.py
and tests/test_gpu_scene360.py)."""
import os
import struct

import numpy as np

from tests.dataset_fixture import SCENE360, _look_at_pose, _png, render_scene360

VIEWS, WIDTH, HEIGHT, STEPS, SEED = 16, 80, 60, 512, 91          # 16 views: images 0 and 8 are the test split; 14 x 40 x 30 train pixels at factor 2


def rule_area_downscale(src_u8, factor):
    """include/mipnerf_hip.h `mipnerf_area_downscale` in numpy: src [n, H, W, C] uint8 -> (q [n, h, w, 3] uint8, float32 q / 255)."""
    n, H, W, _ = src_u8.shape
    F = int(factor)
    h, w = H // F, W // F
    s = src_u8[:, :h * F, :w * F, :3].astype(np.int64).reshape(n, h, F, w, F, 3).sum(axis=(2, 4))
    q = (2 * s + F * F) // (2 * F * F)
    assert q.min() >= 0 and q.max() <= 255
    return q.astype(np.uint8), q.astype(np.float32) / np.float32(255.0)


def write_scene360_llff(root, views=VIEWS, w=WIDTH, h=HEIGHT, steps=STEPS, seed=SEED):
    """LLFF layout with images/ only: views of the unbounded scene from inside its sky shell, looking at the origin, rendered without a
    white background through the pixel -> ray rule of datasets.load_realdata360 (directions = R K^-1 (x + .5, y + .5, 1) with the y and
    z rows of K^-1 negated); poses in LLFF axis order with per-view bounds; one PINHOLE camera in sparse/0/cameras.bin."""
    S = SCENE360
    rng = np.random.RandomState(seed)
    focal = 0.5 * w / np.tan(0.5 * S["fov"])
    cx, cy = 0.5 * w, 0.5 * h
    K_inv = np.linalg.inv(np.array([[focal, 0.0, cx], [0.0, focal, cy], [0.0, 0.0, 1.0]]))
    K_inv[1:, :] *= -1
    x, y = np.meshgrid(np.arange(w, dtype=np.float64) + 0.5, np.arange(h, dtype=np.float64) + 0.5, indexing="xy")
    cam_dirs = np.stack([x, y, np.ones_like(x)], -1) @ K_inv.T                    # [h, w, 3]
    rows = []
    for i in range(views):
        c2w = _look_at_pose(rng, radius=rng.uniform(*S["radius"]))
        near, far = rng.uniform(*S["near"]), rng.uniform(*S["far"])
        dirs = cam_dirs @ c2w[:3, :3].T
        origins = np.broadcast_to(c2w[:3, 3], dirs.shape)
        rgb = np.concatenate([render_scene360(origins[r:r + 8], dirs[r:r + 8], near, far, steps=steps, white_bkgd=False)
                              for r in range(0, h, 8)], 0)
        _png(os.path.join(root, "images", f"view_{i:03d}.png"), np.round(255.0 * rgb).astype(np.uint8))
        llff = np.concatenate([-c2w[:3, 1:2], c2w[:3, 0:1], c2w[:3, 2:3], c2w[:3, 3:4], np.array([[h], [w], [focal]])], axis=1)
        rows.append(np.concatenate([llff.reshape(-1), [near, far]]))
    np.save(os.path.join(root, "poses_bounds.npy"), np.stack(rows))
    os.makedirs(os.path.join(root, "sparse", "0"), exist_ok=True)
    with open(os.path.join(root, "sparse", "0", "cameras.bin"), "wb") as f:
        f.write(struct.pack("<Q", 1))
        f.write(struct.pack("<iiQQ", 1, 1, w, h))
        f.write(struct.pack("<dddd", focal, focal, cx, cy))
    return root
