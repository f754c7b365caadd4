#!/usr/bin/env python3
"""Generate tests/golden/render_path_llff.npz: the reference's render path (hjxwhy/mipnerf_pl, utils/vis.py `gen_render_path`) through
the train and the test poses that `datasets.load_realdata360` returns for `tests/dataset_fixture.write_llff`.

Run (only possible in the build container, where the reference checkout is mounted; MIPNERF_REFERENCE overrides its path; needs scipy):

    cd /tmp && PYTHONDONTWRITEBYTECODE=1 python3 -B <repo>/scripts/make_golden_path.py

utils/vis.py imports cv2 and torchvision at module level and cannot be imported here, so the SOURCE of that one function is cut out
of the file with `ast` and executed with numpy and scipy's `Rotation` in scope; the text is never stored.  Stored -- data only:
    {split}_poses       the input camera-to-world matrices, float64 [n, 3, 4]   (8 train, 2 test)
    {split}_path        gen_render_path(poses, 30), float64 [n * 10, 4, 4]
    {split}_euler       the extrinsic-xyz Euler angles in degrees of the inputs (to show the fixture is clear of gimbal lock)"""
import ast
import os
import sys
import tempfile
import warnings

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("MIPNERF_REFERENCE", "/root/reference")
sys.dont_write_bytecode = True
sys.path.insert(0, REPO)
sys.path.insert(1, os.path.join(REPO, "tests"))

import numpy as np  # noqa: E402
from scipy.spatial.transform import Rotation  # noqa: E402

import dataset_fixture as fx  # noqa: E402
from mipnerf_pl_amd.datasets import load_realdata360  # noqa: E402

N_VIEWS = 30


def reference_function(name):
    path = os.path.join(REF, "utils", "vis.py")
    with open(path) as f:
        tree = ast.parse(f.read())
    node = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == name)
    scope = {"np": np, "R": Rotation}
    exec(compile(ast.Module(body=[node], type_ignores=[]), path, "exec"), scope)
    return scope[name]


def main():
    gen = reference_function("gen_render_path")
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        root = fx.write_llff(os.path.join(tmp, "llff"))
        for split in ("train", "test"):
            _, _, info = load_realdata360(root, split, True, 4)
            poses = np.asarray(info["camtoworlds"], np.float64)
            with warnings.catch_warnings():
                warnings.simplefilter("error")              # scipy warns at gimbal lock: the golden must not be made there
                path = gen(poses, N_VIEWS)
                euler = Rotation.from_matrix(poses[:, :3, :3]).as_euler("xyz", degrees=True)
            assert path.shape == (len(poses) * (N_VIEWS // 3), 4, 4) and path.dtype == np.float64
            rot = path[:, :3, :3]
            print(f"{split}: {len(poses)} poses -> {len(path)}; |middle angle| <= {np.abs(euler[:, 1]).max():.1f} deg; "
                  f"orthonormal to {np.abs(rot @ rot.transpose(0, 2, 1) - np.eye(3)).max():.1e}")
            out[f"{split}_poses"], out[f"{split}_path"], out[f"{split}_euler"] = poses, path, euler
    path = os.path.join(REPO, "tests", "golden", "render_path_llff.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, {len(out)} arrays, numpy {np.__version__}")


if __name__ == "__main__":
    main()
