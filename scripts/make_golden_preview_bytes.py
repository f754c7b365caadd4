#!/usr/bin/env python3
"""Record tests/golden/preview_march_bytes.npz: every output array of mipnerf_preview_march and mipnerf_preview_mip_march on the cases of
tests/preview_bytes_fixture.py, on one MI355X.  The committed file was recorded on the last tree whose two entry points had a march
kernel each, before they were folded into one; tests/test_gpu_preview_bytes.py compares later trees with it byte for byte, so run this
again only to record a deliberate change of the marching rules.

    python scripts/make_golden_preview_bytes.py [OUT.npz]
"""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(1, os.path.join(REPO, "tests"))

import numpy as np  # noqa: E402

import preview_bytes_fixture as bf  # noqa: E402


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(REPO, "tests", "golden", bf.GOLDEN)
    arrays = {}
    for name in bf.case_names():
        for k, v in bf.run_case(name).items():
            arrays[f"{name}_{k}"] = v
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "wb") as f:
        np.savez_compressed(f, **arrays)
    hit = sum(int((arrays[f"{n}_steps"] > 0).sum()) for n in bf.case_names())
    print(f"{path}: {len(arrays)} arrays of {len(bf.case_names())} cases, {os.path.getsize(path)} bytes, {hit} rays with samples")


if __name__ == "__main__":
    main()
