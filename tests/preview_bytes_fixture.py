"""The cases of tests/golden/preview_march_bytes.npz (TEST INFRASTRUCTURE, shared by scripts/make_golden_preview_bytes.py, which recorded
the file on the tree that still had one march kernel per entry point, and tests/test_gpu_preview_bytes.py, which holds every later tree
to those bytes): mipnerf_preview_march and mipnerf_preview_mip_march on the shared test scene -- the 257 rays of
preview_fixture.scene_rays (the hand-made degenerate ones included), the three levels and the radii of preview_mip_fixture -- at two
march settings, on hollow rows with and without occupancy grids, and once on opaque rows with an early stop."""
import numpy as np
import torch

import preview_fixture as pf
import preview_mip_fixture as mf

DEV = "cuda:0"
GOLDEN = "preview_march_bytes.npz"
BACKGROUND = (0.0, 0.25, 0.5)
SETTINGS = ((0.5, 0.0, 4096), (0.1, 1e-3, 150))          # (step_scale, t_min, max_steps): one block of 64 samples / three and a cap
THRESHOLD = 5.0                                          # of the occupancy grids: the hollow half of every level is clear
PLAIN_ARRAYS = ("rgb", "acc", "distance", "steps")
MIP_ARRAYS = PLAIN_ARRAYS + ("lod",)


def _field(rows, dims, degree, occupancy=None):
    from mipnerf_pl_amd import preview
    return preview.BakedField(torch.from_numpy(np.ascontiguousarray(rows)).to(DEV), dims, pf.LO, pf.HI, degree, occupancy)


def _grid(rows):
    from mipnerf_pl_amd import ops
    return ops.occupancy_grid(torch.from_numpy(rows[..., 0].astype(np.float32)).to(DEV), THRESHOLD, pf.LO, pf.HI, dilate=0)


def case_names():
    """every case, in the order `run_case` is cheapest to walk"""
    names = []
    for kind in ("plain", "mip"):
        for degree in (0, 1, 2):
            for occ in (0, 1):
                names += [f"{kind}_d{degree}_occ{occ}_s{s}" for s in range(len(SETTINGS))]
    return names + ["mip_d2_opaque"]


def run_case(name):
    """{array name: numpy array} of one case; steps and lod start from a value no ray can produce"""
    from mipnerf_pl_amd import preview
    o, d, tn, tf = [torch.from_numpy(a).to(DEV) for a in pf.scene_rays()]
    steps = torch.full((pf.N_RAYS,), -7, dtype=torch.int32, device=DEV)
    if name == "mip_d2_opaque":
        kind, degree, occ, setting, kw = "mip", 2, False, (0.1, 1e-2, 4096), dict(opaque=True)
    else:
        kind, degree, occ, s = name.split("_")
        degree, occ, setting, kw = int(degree[1:]), occ == "occ1", SETTINGS[int(s[1:])], dict(hollow=True)
    if kind == "plain":
        rows, _ = pf.random_rows(degree, **kw)
        rgb, acc, dist = preview.march(_field(rows, pf.DIMS, degree, _grid(rows) if occ else None), o, d, tn, tf, BACKGROUND, *setting,
                                       steps=steps)
        out = (rgb, acc, dist, steps)
    else:
        levels = [r for r, _ in mf.scene_levels(degree, **kw)]
        pyr = preview.BakedPyramid([_field(r, dims, degree, _grid(r) if occ else None) for r, dims in zip(levels, mf.LEVEL_DIMS)])
        lod = torch.full((pf.N_RAYS,), -7.0, device=DEV)
        rgb, acc, dist = preview.march_pyramid(pyr, o, d, torch.from_numpy(mf.scene_radii()).to(DEV), tn, tf, BACKGROUND, mf.FOOTPRINT,
                                               *setting, steps=steps, lod=lod)
        out = (rgb, acc, dist, steps, lod)
    torch.cuda.synchronize()
    return {k: t.cpu().numpy() for k, t in zip(MIP_ARRAYS, out)}
