#!/usr/bin/env python3
"""Generate tests/golden/pyramid_48x40.npz by running the UNMODIFIED reference converter (hjxwhy/mipnerf_pl,
datasets/convert_blender_data.py) and its own `Multicam` class on the two Blender roots of tests/pyramid_fixture.py.

Run (only possible in the build container, where the reference checkout is mounted; MIPNERF_REFERENCE overrides its path):

    cd /tmp && PYTHONDONTWRITEBYTECODE=1 python3 -B <repo>/scripts/make_golden_pyramid.py

Stored -- data only, no program text of the reference:
    {root}_files                  the relative paths of every PNG the converter wrote, sorted
    {root}_png_{k}                the decoded RGBA bytes of file k of that list
    {root}_metadata               the text of metadata.json
    {root}_pixels_wb{0,1}         `Multicam(converted, 'train', white_bkgd).images`: float32 [P, 3] (binary root: wb1 only)
    rays_{field}                  `Multicam(converted, 'train').rays` of the random root, [P, k] as produced (the poses of both roots
                                  are the same, the rays do not depend on the pixel values)
Import recipe as in make_golden.py: an empty `cv2` stub (datasets.py imports it; Multicam never calls it), the reference first
on sys.path so that its `datasets/` package wins."""
import io
import os
import sys
import tempfile
import types

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("MIPNERF_REFERENCE", "/root/reference")
sys.dont_write_bytecode = True
sys.modules.setdefault("cv2", types.ModuleType("cv2"))
sys.path.insert(0, REF)
sys.path.insert(1, os.path.join(REPO, "tests"))

import numpy as np  # noqa: E402
from PIL import Image  # noqa: E402

from datasets import convert_blender_data as ref_conv  # noqa: E402  (reference)
from datasets.datasets import Multicam as RefMulticam  # noqa: E402  (reference)

import pyramid_fixture as pf  # noqa: E402


def main():
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        roots = pf.write_roots(tmp)
        for name in pf.ROOTS:
            new = os.path.join(tmp, "converted", name)
            stdout, sys.stdout = sys.stdout, io.StringIO()          # the converter prints every array shape
            try:
                ref_conv.convert_to_nerfdata(roots[name], new, pf.N_DOWN)
            finally:
                sys.stdout = stdout
            files = sorted(os.path.relpath(os.path.join(d, f), new) for d, _, fs in os.walk(new) for f in fs if f.endswith(".png"))
            out[f"{name}_files"] = np.array(files)
            for k, f in enumerate(files):
                img = Image.open(os.path.join(new, f))
                assert img.mode == "RGBA"
                out[f"{name}_png_{k}"] = np.array(img)
            with open(os.path.join(new, "metadata.json")) as fp:
                out[f"{name}_metadata"] = np.array(fp.read())
            for wb in ((1, 0) if name == "random" else (1,)):
                ds = RefMulticam(new, "train", bool(wb), "all_images")
                assert ds.images.dtype == np.float32
                out[f"{name}_pixels_wb{wb}"] = ds.images
                if name == "random" and wb:
                    for k in ds.rays._fields:
                        out[f"rays_{k}"] = np.asarray(getattr(ds.rays, k))     # as produced: float32, radii float64
    path = os.path.join(REPO, "tests", "golden", "pyramid_48x40.npz")
    np.savez_compressed(path, **out)
    print(f"wrote {path}: {os.path.getsize(path)} bytes, {len(out)} arrays, numpy {np.__version__}")


if __name__ == "__main__":
    main()
