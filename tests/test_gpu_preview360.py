"""GPU: the contracted-space preview (libmipnerf_preview_360.so, mipnerf_pl_amd.preview with space='contracted') --
mipnerf_preview_360_march against the float64 fixture of tests/preview360_fixture.py on the smallest shapes that can still go wrong (a
9 x 10 x 11 lattice over a non-cubic box of the contracted space, far radius 8, 270 rays), over several blocks of 64 samples, under a
step cap, with an occupancy grid, in uniform fog (which pins the world length of every sample), sparse against dense, determinism and
graph capture, `bake_field(space='contracted')` against the public ops it is made of, and the command end to end.

Bounds: the project's fp32 bounds (__graft_entry__.py: rgb 5e-5, acc 5e-5, distance 2e-4 times max(1, far)) on the rays the fixture does
not call fragile; `steps` equal.  Fragile rays (a sample within 1e-4 of a cell of a cell or box face, or the last sample / the first missing
one within 1e-4 s of wb) only have to be finite and inside [0, 1] / [near, far]; at most 10 % of the rays are fragile."""
import os
import re

import numpy as np
import pytest
import torch

import preview360_fixture as pf

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = dict(rgb=5e-5, acc=5e-5, distance=2e-4)
BG = (0.2, 0.9, 0.4)


@pytest.fixture(scope="module")
def rays():
    return pf.scene_rays()


def _words(words, lo=pf.LO, hi=pf.HI, dims=pf.DIMS):
    from mipnerf_pl_amd.ops import Occupancy
    return Occupancy(torch.from_numpy(words.view(np.int32)).to(DEV).view(torch.uint32), dims, lo, hi, space="contracted")


def _baked(rows, degree, occupancy=None, lo=pf.LO, hi=pf.HI):
    from mipnerf_pl_amd import preview
    return preview.BakedField(torch.from_numpy(np.ascontiguousarray(rows)).to(DEV), pf.DIMS, lo, hi, degree, occupancy, space="contracted",
                              far_radius=pf.FAR_RADIUS)


def gpu_march(baked, rays, step_scale=0.5, t_min=0.0, max_steps=4096, background=BG):
    from mipnerf_pl_amd import preview
    o, d, tn, tf = [torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in rays]
    steps = torch.full((o.shape[0],), -7, dtype=torch.int32, device=DEV)
    rgb, acc, dist = preview.march(baked, o, d, tn, tf, background, step_scale, t_min, max_steps, steps=steps)
    torch.cuda.synchronize()
    return rgb.cpu().numpy(), acc.cpu().numpy(), dist.cpu().numpy(), steps.cpu().numpy()


def compare(got, want, rays, what):
    """non-fragile rays inside the fp32 bounds with equal steps; fragile ones finite and in range"""
    rgb, acc, dist, steps, fragile = want
    near, far = rays[2], rays[3]
    assert fragile.mean() <= 0.10, what
    ok = ~fragile
    err = dict(rgb=np.abs(got[0] - rgb)[ok].max(), acc=np.abs(got[1] - acc)[ok].max(),
               distance=(np.abs(got[2] - dist) / np.maximum(1.0, far))[ok].max())
    print(what, "fragile", int(fragile.sum()), "of", fragile.size, " ".join(f"{k}={v:.3e}" for k, v in err.items()))
    assert np.array_equal(got[3][ok], steps[ok]), (what, np.flatnonzero(got[3] != steps))
    for k, v in err.items():
        assert v <= TOL[k], (what, k, v)
    f = fragile
    assert np.isfinite(got[0][f]).all() and (got[0][f] >= 0).all() and (got[0][f] <= 1).all()
    assert (got[1][f] >= 0).all() and (got[1][f] <= 1 + 1e-6).all()
    assert (got[2][f] >= near[f]).all() and (got[2][f] <= far[f]).all()


@pytest.mark.parametrize("degree", [0, 1, 2])
def test_march_against_the_fixture(rays, degree):
    rows, _ = pf.random_rows(degree)
    want = pf.march(rows, pf.LO, pf.HI, degree, pf.FAR_RADIUS, *rays, 0.5, 0.0, 4096, BG)
    got = gpu_march(_baked(rows, degree), rays)
    compare(got, want, rays, f"degree {degree}")
    hit = np.array([pf.Ray(rays[0][b], rays[1][b], rays[2][b], rays[3][b], pf.FAR_RADIUS).hit for b in range(pf.N_RAYS)])
    assert hit.sum() == pf.N_SEEDED + 3 and (want[3][hit] > 0).sum() > 200
    miss = ~hit                                                     # written as rule 2 of mipnerf_preview.h writes a miss
    assert np.array_equal(got[0][miss], np.tile(np.array(BG, np.float32), (miss.sum(), 1))) and (got[1][miss] == 0).all()
    assert (got[3][miss] == 0).all()
    tn, tf = rays[2][miss], rays[3][miss]
    assert np.array_equal(got[2][miss], np.where(np.isfinite(tn), tn, np.where(np.isfinite(tf), tf, 0.0)).astype(np.float32))


@pytest.mark.parametrize("degree,t_min,max_steps", [(1, 0.0, 4096), (2, 1e-3, 4096), (0, 0.0, 70)])
def test_march_over_several_blocks_of_64_samples_and_a_step_cap(rays, degree, t_min, max_steps):
    """step_scale 0.05: the rays span several blocks of 64 samples; max_steps = 70 ends a ray inside its second block"""
    rows, _ = pf.random_rows(degree)
    want = pf.march(rows, pf.LO, pf.HI, degree, pf.FAR_RADIUS, *rays, 0.05, t_min, max_steps, BG)
    got = gpu_march(_baked(rows, degree), rays, 0.05, t_min, max_steps)
    compare(got, want, rays, f"degree {degree} step 0.05 t_min {t_min} max_steps {max_steps}")
    if max_steps == 4096 and t_min == 0.0:
        assert (want[3] > 64).mean() >= 0.20 and (want[3] > 128).any()
    if max_steps == 70:
        s = pf.lattice_step(pf.DIMS, pf.LO, pf.HI, 0.05)
        counts = np.array([pf.Ray(rays[0][b], rays[1][b], rays[2][b], rays[3][b], pf.FAR_RADIUS).samples(s, 4096)["w"].size
                           if b < pf.N_SEEDED + 3 else 0 for b in range(pf.N_RAYS)])
        assert (counts > 70).mean() >= 0.20 and want[3].max() <= 70          # the cap binds


def test_march_with_an_occupancy_grid(rays):
    """hollow rows: the cells at contracted x < -0.5 are clear; six more rays stay at x < -1.5, so every one of their samples is clear"""
    rows, sigma = pf.random_rows(1, hollow=True)
    words = pf.occupancy_words(sigma)
    k = np.arange(6, dtype=np.float32)
    extra = (np.stack([np.full(6, -1.5, np.float32), 0.1 * k, np.full(6, 0.2, np.float32)], -1),
             np.stack([np.full(6, -1.0, np.float32), 0.05 * k, np.full(6, 0.1, np.float32)], -1), np.full(6, 0.05, np.float32),
             np.full(6, 30.0, np.float32))
    more = tuple(np.concatenate([a, b]) for a, b in zip(rays, extra))
    want = pf.march(rows, pf.LO, pf.HI, 1, pf.FAR_RADIUS, *more, 0.5, 0.0, 4096, BG, words)
    free = pf.march(rows, pf.LO, pf.HI, 1, pf.FAR_RADIUS, *more, 0.5, 0.0, 4096, BG, None)
    assert (want[3][-6:] == 0).all() and (free[3][-6:] > 0).all() and (want[3] < free[3]).sum() > 50
    got = gpu_march(_baked(rows, 1, _words(words)), more)
    compare(got, want, more, "occupancy")
    assert np.array_equal(got[0][-6:], np.tile(np.array(BG, np.float32), (6, 1))) and (got[1][-6:] == 0).all()
    # the skipped rows hold zeros only: without the grid the picture is the same within the bounds, the step counts are not
    compare(gpu_march(_baked(rows, 1), more), free, more, "no occupancy")


def test_uniform_fog_pins_the_world_length_of_every_sample(rays):
    """sigma = 0.3 everywhere in a box that holds the whole contracted space: acc = 1 - exp(-0.3 (lb - la)) on every hit ray, whatever
    the step -- a sample's world length delta_i is wrong anywhere, or the deltas do not partition [la, lb], and this fails"""
    lo, hi = (-2.0, -2.0, -2.0), (2.0, 2.0, 2.0)
    rows = pf.fog_rows(1)
    o, d, tn, tf = rays
    want = np.zeros(pf.N_RAYS)
    hit = np.zeros(pf.N_RAYS, bool)
    for b in range(pf.N_RAYS):
        r = pf.Ray(o[b], d[b], tn[b], tf[b], pf.FAR_RADIUS)
        hit[b] = r.hit
        if r.hit:
            want[b] = 1.0 - np.exp(-float(np.float16(0.3)) * (r.lb - r.la))
    for step_scale in (0.5, 0.05):
        rgb, acc, dist, steps = gpu_march(_baked(rows, 1, lo=lo, hi=hi), rays, step_scale, 0.0, 4096, (0.0, 0.0, 0.0))
        err = np.abs(acc - want)
        print(f"fog, step_scale {step_scale}: max |acc - closed form| {err.max():.3e} over {int(hit.sum())} hit rays")
        assert (steps[hit] > 0).all()
        assert err.max() <= 5e-5
        colour = rows[0, 0, 0, 1:4].astype(np.float64) * 0.28209479177387814          # the fp16 coefficients times Y_0
        assert np.abs(rgb - want[:, None] * colour).max() <= 5e-5


def test_sparse_equals_dense_byte_for_byte(rays):
    from mipnerf_pl_amd import preview
    for degree in (0, 1, 2):
        rows, sigma = pf.random_rows(degree, hollow=True)
        dense = _baked(rows, degree, _words(pf.occupancy_words(sigma)))
        sparse = dense.to_sparse()
        assert isinstance(sparse, preview.SparseField) and sparse.space == "contracted" and sparse.far_radius == pf.FAR_RADIUS
        assert 0 < sparse.n_rows < int(np.prod(pf.DIMS))
        for step_scale, t_min in ((0.5, 0.0), (0.05, 1e-3)):
            a, b = gpu_march(dense, rays, step_scale, t_min), gpu_march(sparse, rays, step_scale, t_min)
            for x, y in zip(a, b):
                assert np.array_equal(x.view(np.int32), y.view(np.int32)), (degree, step_scale)
            assert (a[3] > 0).sum() > 100


def test_two_runs_and_a_captured_replay_give_the_same_bytes(rays):
    from mipnerf_pl_amd import preview
    rows, _ = pf.random_rows(2)
    baked = _baked(rows, 2)
    o, d, tn, tf = [torch.from_numpy(a).to(DEV) for a in rays]
    outs = []
    for _ in range(2):
        steps = torch.zeros(pf.N_RAYS, dtype=torch.int32, device=DEV)
        outs.append([t.clone() for t in preview.march(baked, o, d, tn, tf, BG, 0.05, 1e-3, 4096, steps=steps)] + [steps])
    for a, b in zip(*outs):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    static = (torch.zeros(pf.N_RAYS, 3, device=DEV), torch.zeros(pf.N_RAYS, device=DEV), torch.zeros(pf.N_RAYS, device=DEV))
    steps = torch.zeros(pf.N_RAYS, dtype=torch.int32, device=DEV)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        preview.march(baked, o, d, tn, tf, BG, 0.05, 1e-3, 4096, out=static, steps=steps)
    for t in static:
        t.zero_()
    g.replay()
    torch.cuda.synchronize()
    for a, b in zip(outs[0], list(static) + [steps]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def _model():
    from mipnerf_pl_amd import MipNerf
    torch.manual_seed(3)
    return MipNerf(num_samples=16, precision="fp32", unbounded=True).to(DEV).eval()


def test_bake_field_contracted_is_made_of_the_public_ops(rays, tmp_path):
    from mipnerf_pl_amd import ops, preview
    model = _model()
    dims, R = (12, 12, 12), 8.0
    with torch.no_grad():
        sigma = ops.density_grid(model, dims, -2.0, 2.0, space="contracted", far_radius=R)
    threshold = float(torch.quantile(sigma.reshape(-1), 0.9))
    baked = preview.bake_field(model, grid=12, degree=1, threshold=threshold, dilate=0, precision="fp32", space="contracted", far_radius=R)
    assert baked.space == "contracted" and baked.far_radius == R and baked.lo == (-2.0,) * 3 and baked.hi == (2.0,) * 3
    assert baked.occupancy.space == "contracted" and tuple(baked.rows.shape) == (12, 12, 12, 16)
    rows = baked.rows.cpu().numpy()
    assert np.array_equal(rows[..., 0].view(np.uint16), sigma.half().cpu().numpy().view(np.uint16))
    occ = ops.occupancy_grid(sigma, threshold, -2.0, 2.0, dilate=0)
    assert torch.equal(occ.bits.view(torch.int32), baked.occupancy.bits.view(torch.int32))
    pts = preview.baked_points(occ)
    assert 0.02 < float(pts.float().mean()) < 0.98
    assert np.array_equal((rows[..., 1:] != 0).any(-1), pts.cpu().numpy())
    index = torch.nonzero(pts.reshape(-1)).reshape(-1)
    means, var = preview.lattice_gaussians(dims, baked.lo, baked.hi, 1.0, index)
    h = np.float32(4.0) / np.float32(11.0)
    assert np.allclose(var.cpu().numpy(), h * h / np.float32(12.0), rtol=1e-6, atol=0)      # the variance in contracted coordinates
    dirs = preview.bake_directions(32)
    with torch.no_grad():
        rgb = torch.stack([ops.field_at(model, means, var, dirs[k].float().to(DEV).expand(index.numel(), 3), precision="fp32",
                                        space="contracted")[:, :3] for k in range(32)], 1)
    want = preview.fit_sh(rgb, dirs, 1).half().cpu().numpy().reshape(-1, 12)
    assert np.array_equal(rows[pts.cpu().numpy()][:, 1:13].view(np.uint16), want.view(np.uint16))
    # sparse=True: the same bytes as the dense bake made sparse, tagged alike
    sparse = preview.bake_field(model, grid=12, degree=1, threshold=threshold, dilate=0, precision="fp32", space="contracted", far_radius=R,
                                sparse=True)
    assert sparse.space == "contracted" and torch.equal(sparse.rows.view(torch.int16), baked.to_sparse().rows.view(torch.int16))
    again = preview.BakedField.load(baked.save(str(tmp_path / "baked.npz")), DEV)
    assert again.space == "contracted" and again.far_radius == R and torch.equal(again.rows.view(torch.int16), baked.rows.view(torch.int16))
    # its march, against the fixture on the baked rows
    words = baked.occupancy.bits.cpu().numpy().view(np.uint32)
    want = pf.march(rows, baked.lo, baked.hi, 1, R, *rays, 0.5, 0.0, 4096, BG, words)
    got = gpu_march(baked, rays)
    compare(got, want, rays, "baked 12^3")
    assert (want[3] > 0).sum() > 50
    from types import SimpleNamespace
    frame = preview.render_rays(baked, SimpleNamespace(origins=torch.from_numpy(rays[0]).to(DEV), directions=torch.from_numpy(rays[1]).to(DEV),
                                                       near=torch.from_numpy(rays[2]).to(DEV)[:, None], far=torch.from_numpy(rays[3]).to(DEV)[:, None]),
                                BG)
    assert np.array_equal(frame[0].cpu().numpy().view(np.int32), got[0].view(np.int32))          # render_rays dispatches on the tag
    for call in (lambda: preview.bake_pyramid(model, grid=12, space="contracted", far_radius=R), lambda: preview.TuneState(baked)):
        with pytest.raises(NotImplementedError, match="contracted"):
            call()
    with pytest.raises(NotImplementedError, match="unbounded=True models are not supported"):
        preview.bake_field(model, grid=12, lo=-2.0, hi=2.0)


def _pngs(root):
    out = {}
    for d, _, fs in os.walk(root):
        for f in fs:
            if f.endswith(".png") and f[:5].isdigit():
                with open(os.path.join(d, f), "rb") as fh:
                    out[os.path.relpath(os.path.join(d, f), root)] = fh.read()
    return out


def test_the_command_end_to_end(tmp_path, capsys):
    """python -m mipnerf_pl_amd.preview --space contracted on a llff checkpoint of the unbounded-scene model and the capture of
    tests/scene360_fixture.py: the PNGs of the interpolated path and the `preview:` line, --save_baked then --baked with the same PNG
    bytes, --sparse with its stored share in the line, --compare with its three PSNRs (no threshold: the baked picture is not the
    MLP's), and the refusal that needs the checkpoint."""
    import scene360_fixture as sf
    from mipnerf_pl_amd import preview
    from mipnerf_pl_amd.system import DEFAULT_HPARAMS, MipNeRFSystem
    data = sf.write_scene360_llff(str(tmp_path / "scene"), views=6, w=24, h=18, steps=32)
    hp = dict(DEFAULT_HPARAMS)
    hp.update({"nerf.num_samples": 16, "nerf.unbounded": True, "exp_name": "cli360", "val.batch_type": "single_image", "dataset_name": "llff",
               "factor": 2, "val.white_bkgd": False, "train.white_bkgd": False})
    torch.manual_seed(4)
    ckpt = str(tmp_path / "last.ckpt")
    MipNeRFSystem(hp, precision="fp32").save_checkpoint(ckpt)
    common = ["--ckpt", ckpt, "--data", data, "--grid", "16", "--n_views", "6", "--precision", "fp32", "--threshold", "-1", "--space", "contracted"]
    out = str(tmp_path / "a")
    folder = preview.main(common + ["--out_dir", out, "--save_baked"])
    assert folder == os.path.join(out, "preview_path", "cli360")
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("preview:")]
    m = re.fullmatch(r"preview: lattice 16 x 16 x 16, degree 1, baked share 1\.0000, [0-9.]+ MiB, baked in [0-9.]+ ms, mean [0-9.]+ ms per frame "
                     r"\((\d+) frames\), contracted, far radius ([0-9.e+]+), mean ([0-9.]+) evaluated samples per ray", lines[-1])
    assert m, lines
    n_frames = int(m.group(1))
    assert n_frames >= 1 and float(m.group(2)) > 1.0 and float(m.group(3)) > 10.0      # a threshold of -1 marches every cell
    first = _pngs(folder)
    assert sorted(first) == sorted(os.path.join("1", f"{i:05d}_{t}.png") for i in range(n_frames) for t in ("rgb", "dist", "acc"))
    from PIL import Image
    assert np.array(Image.open(os.path.join(folder, "1", "00000_rgb.png"))).shape == (9, 12, 3)          # the data's size at factor 2
    baked = os.path.join(folder, "baked.npz")
    assert preview.BakedField.stored_space(baked) == "contracted"
    out_b = str(tmp_path / "b")
    preview.main(common + ["--out_dir", out_b, "--baked", baked])
    assert "loaded in" in capsys.readouterr().out
    assert _pngs(os.path.join(out_b, "preview_path", "cli360")) == first
    preview.main(common + ["--out_dir", str(tmp_path / "s"), "--sparse", "--far_radius", m.group(2)])
    assert "stored share 1.0000" in capsys.readouterr().out
    preview.main(common + ["--out_dir", str(tmp_path / "c"), "--compare"])
    text = capsys.readouterr().out
    p = re.search(r"preview: mean PSNR over (\d+) test images: baked vs photos ([0-9.]+), MLP vs photos ([0-9.]+), baked vs MLP ([0-9.]+)", text)
    assert p, text
    print("PSNR baked / MLP / baked-vs-MLP:", p.groups()[1:])
    assert all(np.isfinite(float(v)) for v in p.groups()[1:])
    # refused once the checkpoint is read, before any device work: no --space on this checkpoint, a bounded file with --space
    with pytest.raises(SystemExit, match="captured scene.*--space contracted"):
        preview.main(["--ckpt", ckpt, "--out_dir", str(tmp_path / "r")])
    assert not os.path.exists(str(tmp_path / "r"))
