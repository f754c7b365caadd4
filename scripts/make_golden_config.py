#!/usr/bin/env python3
"""Generate tests/golden/config_lego_merged.json with the UNMODIFIED reference's configs/config.py (hjxwhy/mipnerf_pl): the flat dict
`load(configs/lego.yaml)` gives, then the same dict after `merge_from_list` of OPTS below.  tests/golden/config_lego.yaml is the
reference's configs/lego.yaml, committed as the input.  Python types are kept in the JSON by tagging tuples and None (JSON has lists
and null only).

Run from outside the repository, with a checkout of the reference:

    PYTHONDONTWRITEBYTECODE=1 python3 -B scripts/make_golden_config.py PATH_TO_REFERENCE_CHECKOUT
"""
import json
import os
import sys

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "config_lego_merged.json")
OPTS = ["train.batch_size", "1024", "optimizer.lr_init", "1e-3", "val.check_interval", "50", "nerf.ray_shape", "cylinder",
        "checkpoint.resume_path", "None", "exp_name", "lego_small", "new.key", "[1, 2]", "nerf.density_noise", "1.", "seed", "abc def"]


def tag(v):
    if isinstance(v, tuple):
        return {"tuple": [tag(x) for x in v]}
    if v is None:
        return {"none": True}
    return v


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    ref = os.path.abspath(sys.argv[1])
    sys.path.insert(0, ref)
    from configs import config as cfg       # the reference module, unmodified
    base = cfg.load(os.path.join(ref, "configs", "lego.yaml"))
    merged = dict(base)
    cfg.merge_from_list(merged, list(OPTS))
    doc = {"opts": OPTS,
           "loaded": {k: [type(v).__name__, tag(v)] for k, v in base.items()},
           "merged": {k: [type(v).__name__, tag(v)] for k, v in merged.items()}}
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
    print(f"wrote {OUT}: {len(base)} keys loaded, {len(merged)} after the merge")


if __name__ == "__main__":
    main()
