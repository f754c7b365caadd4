"""GPU: the preview over a cone-radius pyramid of lattices (libmipnerf_preview_mip.so, mipnerf_pl_amd.preview) --
mipnerf_preview_mip_march against the float64 fixture of tests/preview_mip_fixture.py on the smallest shapes that can still go wrong
(three lattices of 8 x 9 x 10, 5 x 5 x 6 and 3 x 3 x 4 points with contents of their own over a non-cubic box, 257 rays, seeded radii
that spread the footprints over all four regimes), over several 64-sample blocks, with per-level occupancy grids, rule P7 bit for bit
against mipnerf_preview_march, the early stop, NaN containment, determinism and graph capture, the anti-aliasing scene, `bake_pyramid`
against `bake_field`, and the command end to end.

Bounds: those of test_gpu_preview.py (rgb 5e-5, acc 5e-5, distance 2e-4 times max(1, far)) on the rays the fixture does not call
fragile, `steps` equal, lod within 1e-4 L; fragile rays only have to be finite and in range.  test_preview_mip_cpu.py asserts the
fixture's own conditions (at most 10 % fragile, all four regimes) without a GPU."""
import os
import re

import numpy as np
import pytest
import torch

import preview_fixture as pf
import preview_mip_fixture as mf

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = dict(rgb=5e-5, acc=5e-5, distance=2e-4)
WHITE = (1.0, 1.0, 1.0)
F = np.float32


@pytest.fixture(scope="module")
def rays():
    return pf.scene_rays()


@pytest.fixture(scope="module")
def radii():
    return mf.scene_radii()


def _field(rows, dims, degree, occupancy=None, lo=pf.LO, hi=pf.HI):
    from mipnerf_pl_amd import preview
    return preview.BakedField(torch.from_numpy(np.ascontiguousarray(rows)).to(DEV), dims, lo, hi, degree, occupancy)


def _pyramid(levels, degree, occupancy=None, dims=mf.LEVEL_DIMS, lo=pf.LO, hi=pf.HI):
    from mipnerf_pl_amd import preview
    occupancy = [None] * len(levels) if occupancy is None else occupancy
    return preview.BakedPyramid([_field(r, d, degree, o, lo, hi) for r, d, o in zip(levels, dims, occupancy)])


def gpu_march(pyramid, rays, radii, step_scale=0.5, t_min=0.0, max_steps=4096, background=WHITE, footprint=mf.FOOTPRINT):
    from mipnerf_pl_amd import preview
    o, d, tn, tf = [torch.from_numpy(a).to(DEV) for a in rays]
    rad = torch.from_numpy(np.ascontiguousarray(radii, F)).to(DEV)
    steps = torch.full((o.shape[0],), -7, dtype=torch.int32, device=DEV)
    lod = torch.full((o.shape[0],), -7.0, device=DEV)
    rgb, acc, dist = preview.march_pyramid(pyramid, o, d, rad, tn, tf, background, footprint, step_scale, t_min, max_steps, steps=steps, lod=lod)
    torch.cuda.synchronize()
    return rgb.cpu().numpy(), acc.cpu().numpy(), dist.cpu().numpy(), steps.cpu().numpy(), lod.cpu().numpy()


def gpu_plain(field, rays, step_scale=0.5, t_min=0.0, max_steps=4096, background=WHITE):
    from mipnerf_pl_amd import preview
    o, d, tn, tf = [torch.from_numpy(a).to(DEV) for a in rays]
    steps = torch.full((o.shape[0],), -7, dtype=torch.int32, device=DEV)
    rgb, acc, dist = preview.march(field, o, d, tn, tf, background, step_scale, t_min, max_steps, steps=steps)
    torch.cuda.synchronize()
    return rgb.cpu().numpy(), acc.cpu().numpy(), dist.cpu().numpy(), steps.cpu().numpy()


def fixture_march(levels, degree, rays, radii, step_scale=0.5, t_min=0.0, max_steps=4096, background=WHITE, occupancy=None,
                  footprint=mf.FOOTPRINT):
    return mf.march(levels, pf.LO, pf.HI, degree, rays[0], rays[1], radii, rays[2], rays[3], footprint, step_scale, t_min, max_steps,
                    background, occupancy)


def compare(got, want, rays, n_levels, what):
    """non-fragile rays inside the fp32 bounds with equal steps; fragile ones finite and in range"""
    rgb, acc, dist, steps, lod, fragile = want[:6]
    near, far = rays[2], rays[3]
    assert fragile.mean() <= 0.10, what
    ok = ~fragile
    err = dict(rgb=np.abs(got[0] - rgb)[ok].max(), acc=np.abs(got[1] - acc)[ok].max(),
               distance=(np.abs(got[2] - dist) / np.maximum(1.0, far))[ok].max())
    lod_err = np.abs(got[4] - lod)[ok].max()
    print(what, "fragile", int(fragile.sum()), "of", fragile.size, " ".join(f"{k}={v:.3e}" for k, v in err.items()), f"lod={lod_err:.3e}")
    assert np.array_equal(got[3][ok], steps[ok]), (what, np.flatnonzero((got[3] != steps) & ok))
    for k, v in err.items():
        assert v <= TOL[k], (what, k, v)
    assert lod_err <= 1e-4 * n_levels, (what, lod_err)
    f = fragile
    assert np.isfinite(got[0][f]).all() and (got[0][f] >= 0).all() and (got[0][f] <= 1).all()
    assert (got[1][f] >= 0).all() and (got[1][f] <= 1 + 1e-6).all()
    assert (got[2][f] >= near[f]).all() and (got[2][f] <= far[f]).all()
    assert (got[4][f] >= 0).all() and (got[4][f] <= n_levels - 1 + 1e-5).all()


@pytest.mark.parametrize("degree", [0, 1, 2])
def test_march_against_the_fixture(rays, radii, degree):
    levels = [r for r, _ in mf.scene_levels(degree)]
    want = fixture_march(levels, degree, rays, radii)
    got = gpu_march(_pyramid(levels, degree), rays, radii)
    compare(got, want, rays, 3, f"degree {degree}")
    assert 0.3 < want[4][want[1] > 0].mean() < 1.7                      # the levels really are mixed
    # the hand-made misses, exactly
    for b in list(range(pf.N_RAYS - 8, pf.N_RAYS)) + [pf.N_RAYS - 11]:
        assert got[3][b] == 0 and got[1][b] == 0 and (got[0][b] == 1).all() and got[4][b] == 0, b
        assert got[2][b] == (rays[2][b] if np.isfinite(rays[2][b]) else rays[3][b]), b
    # a radius that is negative or not finite is a miss (P2); another background
    bad = radii.copy()
    bad[:3] = [-1e-3, np.nan, np.inf]
    want = fixture_march(levels, degree, rays, bad, background=(0.0, 0.25, 0.5))
    got = gpu_march(_pyramid(levels, degree), rays, bad, background=(0.0, 0.25, 0.5))
    compare(got, want, rays, 3, f"degree {degree}, coloured background")
    assert (got[3][:3] == 0).all() and (got[1][:3] == 0).all() and np.array_equal(got[0][:3], np.tile(np.array([0.0, 0.25, 0.5], F), (3, 1)))


@pytest.mark.parametrize("degree,step_scale,max_steps", [(1, 0.1, 4096), (2, 0.1, 70), (0, 0.1, 128)])
def test_march_over_several_blocks_of_64_samples_and_a_step_cap(rays, radii, degree, step_scale, max_steps):
    """a fifth of the step gives up to 166 samples per ray: three blocks of the kernel's march, each with its own run of levels, the
    transmittance carried from one to the next, and a cap that ends a ray inside its second block / at a block's end"""
    levels = [r for r, _ in mf.scene_levels(degree)]
    want = fixture_march(levels, degree, rays, radii, step_scale, 0.0, max_steps)
    assert want[3].max() == min(max_steps, 166) and (want[3] > 64).mean() > 0.2
    compare(gpu_march(_pyramid(levels, degree), rays, radii, step_scale=step_scale, max_steps=max_steps), want, rays, 3,
            f"degree {degree}, {max_steps} steps")


@pytest.mark.parametrize("dilate", [0, 1])
def test_march_with_per_level_occupancy_grids(rays, radii, dilate):
    """hollow rows: every level has clear cells of its own, so P5's OR decides samples whose own level is clear and whose next is not"""
    from mipnerf_pl_amd import ops
    degree = 1
    levels = [r for r, _ in mf.scene_levels(degree, hollow=True)]
    occ = [ops.occupancy_grid(torch.from_numpy(r[..., 0].astype(F)).to(DEV), 5.0, pf.LO, pf.HI, dilate=dilate) for r in levels]
    words = [o.bits.cpu().numpy().view(np.uint32) for o in occ]
    assert 0.2 < occ[0].occupied_fraction() < 0.95          # (dilated, the few cells of the coarse levels may all be occupied)
    want = fixture_march(levels, degree, rays, radii, occupancy=words)
    own = fixture_march(levels, degree, rays, radii, occupancy=[words[0], None, None])
    free = fixture_march(levels, degree, rays, radii)
    assert (want[3] < free[3]).mean() > 0.1                  # conditions on the inputs: the grids clear samples on many rays,
    assert dilate == 1 or not np.array_equal(want[3], own[3])        # and (undilated) the coarse levels' bits decide some of them
    compare(gpu_march(_pyramid(levels, degree, occ), rays, radii), want, rays, 3, f"occupancy on every level, dilate {dilate}")
    mixed = [occ[0], None, occ[2]]
    want = fixture_march(levels, degree, rays, radii, occupancy=[words[0], None, words[2]])
    compare(gpu_march(_pyramid(levels, degree, mixed), rays, radii), want, rays, 3, f"occupancy on levels 0 and 2, dilate {dilate}")
    # use_occupancy=False marches every cell
    from mipnerf_pl_amd import preview
    o, d, tn, tf = [torch.from_numpy(a).to(DEV) for a in rays]
    steps = torch.zeros(pf.N_RAYS, dtype=torch.int32, device=DEV)
    preview.march_pyramid(_pyramid(levels, degree, occ), o, d, torch.from_numpy(radii).to(DEV), tn, tf, WHITE, mf.FOOTPRINT, 0.5, 0.0, 4096,
                          steps=steps, use_occupancy=False)
    assert np.array_equal(steps.cpu().numpy()[~free[5]], free[3][~free[5]])


@pytest.mark.parametrize("degree", [0, 1, 2])
@pytest.mark.parametrize("with_occupancy", [False, True])
def test_one_level_and_zero_radii_are_the_plain_march_bit_for_bit(rays, radii, degree, with_occupancy):
    """P7: every ray, fragile or not"""
    from mipnerf_pl_amd import ops
    levels = [r for r, _ in mf.scene_levels(degree, hollow=True)]
    occ = ops.occupancy_grid(torch.from_numpy(levels[0][..., 0].astype(F)).to(DEV), 5.0, pf.LO, pf.HI, dilate=0) if with_occupancy else None
    field = _field(levels[0], mf.LEVEL_DIMS[0], degree, occ)
    for step_scale, t_min, cap in ((0.5, 0.0, 4096), (0.1, 1e-3, 150)):
        plain = gpu_plain(field, rays, step_scale, t_min, cap, (0.0, 0.25, 0.5))
        assert plain[3].max() > 20
        one = gpu_march(_pyramid(levels[:1], degree, [occ]), rays, radii, step_scale, t_min, cap, (0.0, 0.25, 0.5))
        zero = gpu_march(_pyramid(levels, degree, [occ, None, None]), rays, 0.0 * radii, step_scale, t_min, cap, (0.0, 0.25, 0.5))
        nofoot = gpu_march(_pyramid(levels, degree, [occ, None, None]), rays, radii, step_scale, t_min, cap, (0.0, 0.25, 0.5), footprint=0.0)
        for name, got in (("L = 1", one), ("radii 0", zero), ("footprint 0", nofoot)):
            for a, b in zip(got[:4], plain):
                assert a.tobytes() == b.tobytes(), (name, step_scale)
            assert (got[4] == 0).all()


def test_early_stop_shortens_opaque_rays_and_costs_at_most_t_min(rays, radii):
    levels = [r for r, _ in mf.scene_levels(2, opaque=True)]
    pyr = _pyramid(levels, 2)
    full = gpu_march(pyr, rays, radii, step_scale=0.1)
    cut = gpu_march(pyr, rays, radii, step_scale=0.1, t_min=1e-2)
    hit = full[3] > 0
    assert hit.sum() > 200
    assert (cut[3] <= full[3]).all() and (cut[3][hit] < full[3][hit]).mean() >= 0.5
    assert np.abs(cut[0] - full[0]).max() <= 1e-2 and np.abs(cut[1] - full[1]).max() <= 1e-2
    want = fixture_march(levels, 2, rays, radii, 0.1, 1e-2)
    assert (np.abs(cut[3] - want[3]) <= 1)[~want[5]].all()          # T crosses t_min at the same sample, or at a neighbour when it is close


def test_a_nan_row_in_level_1_poisons_only_the_rays_that_read_it(rays, radii):
    levels = [r.copy() for r, _ in mf.scene_levels(1)]
    clean = gpu_march(_pyramid(levels, 1), rays, radii)
    levels[1][3, 2, 2, 0] = np.nan
    levels[1][1, 3, 3, 5] = np.nan
    want = fixture_march(levels, 1, rays, radii)
    got = gpu_march(_pyramid(levels, 1), rays, radii)
    bad = np.isnan(want[1]) | np.isnan(want[0]).any(-1)
    sure = ~want[5]
    assert 0 < bad.sum() < 200
    assert (np.isnan(got[0]).any(-1) == bad)[sure].all() and np.isnan(got[2][np.isnan(want[2]) & sure]).all()
    same = ~bad & sure
    assert np.array_equal(got[0][same], clean[0][same]) and np.array_equal(got[3][sure], clean[3][sure])
    zero = gpu_march(_pyramid(levels, 1), rays, 0.0 * radii)            # the same rays with radii 0 never read level 1
    assert np.isfinite(zero[0]).all() and np.isfinite(zero[1]).all() and np.isfinite(zero[2][np.isfinite(rays[2])]).all()


def test_two_runs_and_a_captured_replay_give_the_same_bytes(rays, radii):
    from mipnerf_pl_amd import preview
    levels = [r for r, _ in mf.scene_levels(2)]
    pyr = _pyramid(levels, 2)
    o, d, tn, tf = [torch.from_numpy(a).to(DEV) for a in rays]
    rad = torch.from_numpy(radii).to(DEV)
    outs = []
    for _ in range(2):
        steps = torch.zeros(pf.N_RAYS, dtype=torch.int32, device=DEV)
        lod = torch.zeros(pf.N_RAYS, device=DEV)
        outs.append([t.clone() for t in preview.march_pyramid(pyr, o, d, rad, tn, tf, WHITE, mf.FOOTPRINT, 0.1, 1e-3, 4096, steps=steps, lod=lod)]
                    + [steps, lod])
    for a, b in zip(*outs):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    static = (torch.zeros(pf.N_RAYS, 3, device=DEV), torch.zeros(pf.N_RAYS, device=DEV), torch.zeros(pf.N_RAYS, device=DEV))
    steps = torch.zeros(pf.N_RAYS, dtype=torch.int32, device=DEV)
    lod = torch.zeros(pf.N_RAYS, device=DEV)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        preview.march_pyramid(pyr, o, d, rad, tn, tf, WHITE, mf.FOOTPRINT, 0.1, 1e-3, 4096, out=static, steps=steps, lod=lod)
    for t in static:
        t.zero_()
    g.replay()
    torch.cuda.synchronize()
    for a, b in zip(outs[0], list(static) + [steps, lod]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_the_pyramid_anti_aliases_the_scene_of_the_issue():
    """the scene of test_preview_mip_cpu.py through the kernels.  A picture within `tol` of the fixture's per channel has a mean squared
    error against the truth within 2 sqrt(MSE) tol + tol^2 of the fixture's (|a^2 - b^2| = |a - b| |a + b| per entry, Cauchy-Schwarz over
    the mean)."""
    from mipnerf_pl_amd import preview
    tol = TOL["rgb"]
    levels = mf.aa_levels()
    pyr = _pyramid(levels, 0, dims=mf.AA_DIMS, lo=mf.AA_LO, hi=mf.AA_HI)
    for res in (12, 24):
        o, d, rad, tn, tf = [torch.from_numpy(a).to(DEV) for a in mf.aa_rays(res)]
        truth = mf.aa_truth(res)
        want_plain, want_mip = mf.aa_reference(res)
        plain = preview.march(pyr.levels[0], o, d, tn, tf, WHITE, 0.5, 0.0, 4096)[0].double().cpu().numpy()
        mip = preview.march_pyramid(pyr, o, d, rad, tn, tf, WHITE, mf.FOOTPRINT, 0.5, 0.0, 4096)[0].double().cpu().numpy()
        mse_plain, mse_mip = float(((plain - truth) ** 2).mean()), float(((mip - truth) ** 2).mean())
        print(f"{res} x {res}: MSE plain {mse_plain:.4e} (fixture {want_plain:.4e}), pyramid {mse_mip:.4e} (fixture {want_mip:.4e}), "
              f"ratio {mse_mip / mse_plain:.4f}")
        assert abs(mse_plain - want_plain) <= 2 * np.sqrt(want_plain) * tol + tol * tol
        assert abs(mse_mip - want_mip) <= 2 * np.sqrt(want_mip) * tol + tol * tol
        if res == 12:
            assert mse_mip < 0.5 * mse_plain
        else:
            assert abs(mse_mip - mse_plain) <= 1e-3 * mse_plain


def _model(num_samples=16, seed=0):
    from mipnerf_pl_amd import MipNerf
    from oracle import mipnerf_oracle as orc
    model = MipNerf(num_samples=num_samples, precision="fp32")
    params = orc.make_params(seed=seed, density_gain=40.0)
    model.load_state_dict({"mlp." + k: torch.from_numpy(v.copy()) for k, v in params.items()})
    return model.to(DEV).eval()


def test_bake_pyramid_is_bake_field_at_every_level(tmp_path):
    from mipnerf_pl_amd import Rays, ops, preview
    model = _model()
    lo, hi = (-1.0, -1.1, -1.2), (1.1, 1.2, 1.3)
    with torch.no_grad():
        sigma = ops.density_grid(model, (24, 24, 24), lo, hi)
    how = dict(degree=1, lo=lo, hi=hi, threshold=float(torch.quantile(sigma.reshape(-1), 0.9)), dilate=1, precision="fp32")
    pyr = preview.bake_pyramid(model, grid=24, levels=3, **how)
    assert [b.dims for b in pyr.levels] == [(24,) * 3, (12,) * 3, (6,) * 3] and pyr.nbytes == sum(b.nbytes for b in pyr.levels)
    for b in pyr.levels:
        want = preview.bake_field(model, grid=b.dims, **how)
        assert torch.equal(b.rows.view(torch.int16), want.rows.view(torch.int16))
        assert torch.equal(b.occupancy.bits.view(torch.int32), want.occupancy.bits.view(torch.int32))
        assert b.lo == want.lo and b.hi == want.hi and b.threshold == want.threshold
    path = pyr.save(str(tmp_path / "pyr.npz"))
    assert preview.BakedPyramid.stored_levels(path) == 3
    again = preview.BakedPyramid.load(path, DEV)
    for a, b in zip(again.levels, pyr.levels):
        assert torch.equal(a.rows.view(torch.int16), b.rows.view(torch.int16)) and a.dims == b.dims
        assert torch.equal(a.occupancy.bits.view(torch.int32), b.occupancy.bits.view(torch.int32))
    # render_rays: a BakedField takes the path it took, a BakedPyramid the new one
    o, d, tn, tf = [torch.from_numpy(a).to(DEV) for a in pf.scene_rays()]
    rad = torch.from_numpy(mf.scene_radii()).to(DEV)
    rays = Rays(o.view(-1, 3), d.view(-1, 3), d.view(-1, 3), rad.view(-1, 1), torch.ones_like(rad).view(-1, 1), tn.view(-1, 1), tf.view(-1, 1))
    direct = preview.march(pyr.levels[0], o, d, tn, tf, True)
    rgb, dist, acc = preview.render_rays(pyr.levels[0], rays, True)
    for a, b in zip((rgb, acc, dist), direct):
        assert a.shape == b.shape and a.view(torch.int32).equal(b.view(torch.int32))
    direct = preview.march_pyramid(again, o, d, rad, tn, tf, True, footprint=1.0)
    rgb, dist, acc = preview.render_rays(pyr, rays, True, footprint=1.0)
    for a, b in zip((rgb, acc, dist), direct):
        assert a.view(torch.int32).equal(b.view(torch.int32))
    assert float(acc.max()) > 0.5
    # a frame of a pyramid keeps a static lod buffer
    frame = preview.PreviewFrame(pyr, 1, pf.N_RAYS, True)
    assert frame.lod.shape == (pf.N_RAYS,) and preview.PreviewFrame(pyr.levels[0], 1, pf.N_RAYS, True).lod is None
    shaped = Rays(*[t.view(1, pf.N_RAYS, -1) for t in rays])
    out = frame.render(shaped)
    want = preview.march_pyramid(pyr, o, d, rad, tn, tf, True)
    assert out[0].reshape(-1, 3).view(torch.int32).equal(want[0].view(torch.int32)) and float(frame.lod.max()) > 0


def _pngs(root):
    out = {}
    for d, _, fs in os.walk(root):
        for f in fs:
            if f.endswith(".png") and f[:5].isdigit():
                with open(os.path.join(d, f), "rb") as fh:
                    out[os.path.relpath(os.path.join(d, f), root)] = fh.read()
    return out


def test_the_command_end_to_end_with_mip(tmp_path, capsys):
    """python -m mipnerf_pl_amd.preview --mip 3 on a checkpoint written by MipNeRFSystem: the PNGs and the `preview:` line naming 3 levels,
    --save_baked then --baked with the same PNG bytes, --compare with its five PSNRs, and the output directory without --mip as it is today."""
    from dataset_fixture import write_blender
    from mipnerf_pl_amd import preview
    from mipnerf_pl_amd.system import DEFAULT_HPARAMS, MipNeRFSystem
    from oracle import mipnerf_oracle as orc
    hp = dict(DEFAULT_HPARAMS)
    hp.update({"nerf.num_samples": 32, "exp_name": "cli", "val.batch_type": "single_image", "dataset_name": "blender"})
    system = MipNeRFSystem(hp, precision="fp32")
    system.load_state_dict({"mip_nerf.mlp." + k: torch.from_numpy(v.copy()) for k, v in orc.make_params(seed=5, density_gain=40.0).items()}, strict=True)
    ckpt = str(tmp_path / "last.ckpt")
    system.save_checkpoint(ckpt)
    common = ["--ckpt", ckpt, "--grid", "24", "--n_poses", "2", "--scale", "1", "--base_size", "16", "16", "--precision", "fp32"]
    out = str(tmp_path / "a")
    folder = preview.main(common + ["--out_dir", out, "--mip", "3", "--save_baked"])
    assert folder == os.path.join(out, "preview_spheric", "cli")
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("preview:")]
    assert re.fullmatch(r"preview: pyramid of 3 levels 24 x 24 x 24, 12 x 12 x 12, 6 x 6 x 6, degree 1, baked share [0-9.]+, [0-9.]+ MiB, "
                        r"baked in [0-9.]+ ms, mean [0-9.]+ ms per frame \(2 frames\), footprint 1.7321, mean lod [0-9.]+ over [0-9]+ hit rays",
                        lines[-1]), lines
    first = _pngs(folder)
    names = sorted(os.path.join("1", f"{i:05d}_{t}.png") for i in range(2) for t in ("rgb", "dist", "acc"))
    assert sorted(first) == names
    baked = os.path.join(folder, "baked.npz")
    assert preview.BakedPyramid.stored_levels(baked) == 3
    out_b = str(tmp_path / "b")
    preview.main(common + ["--out_dir", out_b, "--mip", "3", "--baked", baked])
    assert "loaded in" in capsys.readouterr().out
    assert _pngs(os.path.join(out_b, "preview_spheric", "cli")) == first
    with pytest.raises(SystemExit, match="pyramid of 3 levels"):
        preview.main(common + ["--out_dir", str(tmp_path / "x"), "--baked", baked])
    # without --mip: the files and the line of today
    out_c = str(tmp_path / "c")
    folder_c = preview.main(common + ["--out_dir", out_c, "--save_baked"])
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("preview:")]
    assert re.fullmatch(r"preview: lattice 24 x 24 x 24, degree 1, baked share [0-9.]+, [0-9.]+ MiB, baked in [0-9.]+ ms, "
                        r"mean [0-9.]+ ms per frame \(2 frames\)", lines[-1]), lines
    assert sorted(_pngs(folder_c)) == names and preview.BakedPyramid.stored_levels(os.path.join(folder_c, "baked.npz")) is None
    assert sorted(os.listdir(folder_c)) == sorted(os.listdir(folder))
    data = write_blender(str(tmp_path / "data"), seed=6, counts=(("test", 2),), w=16, h=16)
    preview.main(common + ["--out_dir", str(tmp_path / "d"), "--mip", "3", "--data", data, "--compare"])
    text = capsys.readouterr().out
    m = re.search(r"preview: mean PSNR over 2 test images: single lattice vs photos ([0-9.]+), pyramid vs photos ([0-9.]+), MLP vs photos "
                  r"([0-9.]+), single lattice vs MLP ([0-9.]+), pyramid vs MLP ([0-9.]+)", text)
    assert m, text
    print("PSNR single / pyramid / MLP vs photos, single / pyramid vs MLP:", m.groups())
    assert all(np.isfinite(float(v)) for v in m.groups())
