"""GPU: the baked-lattice preview renderer (libmipnerf_preview.so, mipnerf_pl_amd.preview) -- mipnerf_preview_march against the float64
fixture of tests/preview_fixture.py on the smallest shapes that can still go wrong (an 8 x 9 x 10 lattice over a non-cubic box, 257 rays,
step_scale 0.5), with and without an occupancy grid, the early stop, determinism and graph capture, mipnerf_preview_pack byte for byte,
`bake_field` against the public ops it is made of, and the command end to end.

Bounds: the project's fp32 bounds (__graft_entry__.py: rgb 5e-5, acc 5e-5, distance 2e-4 times max(1, far)) on the rays the fixture does
not call fragile; `steps` equal.  Fragile rays (a sample within 1e-4 h of a cell face, or the last sample within 1e-4 dt of the interval's
end) may land in another cell or gain a sample in fp32: they only have to be finite and inside [0, 1] / [near, far].  At most 10 % of the
rays are fragile (3 of 257 with the fixture's seed; test_preview_cpu.py asserts the condition without a GPU)."""
import os

import numpy as np
import pytest
import torch

import preview_fixture as pf

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = dict(rgb=5e-5, acc=5e-5, distance=2e-4)
WHITE = (1.0, 1.0, 1.0)


@pytest.fixture(scope="module")
def rays():
    return pf.scene_rays()


def _baked(rows, degree, occupancy=None):
    from mipnerf_pl_amd import preview
    return preview.BakedField(torch.from_numpy(np.ascontiguousarray(rows)).to(DEV), pf.DIMS, pf.LO, pf.HI, degree, occupancy)


def gpu_march(baked, rays, step_scale=0.5, t_min=0.0, max_steps=4096, background=WHITE):
    from mipnerf_pl_amd import preview
    o, d, tn, tf = [torch.from_numpy(a).to(DEV) for a in rays]
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
    want = pf.march(rows, pf.LO, pf.HI, degree, *rays, 0.5, 0.0, 4096, WHITE)
    got = gpu_march(_baked(rows, degree), rays)
    compare(got, want, rays, f"degree {degree}")
    # the hand-made misses, exactly: a NaN origin, |d| = 0, a non-finite near, far <= near, a non-finite direction, near beyond / far before the box
    for b in list(range(pf.N_RAYS - 8, pf.N_RAYS)) + [pf.N_RAYS - 11]:
        assert got[3][b] == 0 and got[1][b] == 0 and (got[0][b] == 1).all(), b
        assert got[2][b] == (rays[2][b] if np.isfinite(rays[2][b]) else rays[3][b]), b
    # another background
    want = pf.march(rows, pf.LO, pf.HI, degree, *rays, 0.5, 0.0, 4096, (0.0, 0.25, 0.5))
    compare(gpu_march(_baked(rows, degree), rays, background=(0.0, 0.25, 0.5)), want, rays, f"degree {degree}, coloured background")


@pytest.mark.parametrize("degree,step_scale,max_steps", [(1, 0.1, 4096), (2, 0.1, 70), (0, 0.1, 128)])
def test_march_over_several_blocks_of_64_samples_and_a_step_cap(rays, degree, step_scale, max_steps):
    """step_scale 0.5 gives at most 33 samples per ray on this lattice: one block of the kernel's march.  A fifth of the step gives up to
    166: three blocks, the transmittance carried from one to the next, and a cap that ends a ray inside its second block / at a block's end."""
    rows, _ = pf.random_rows(degree)
    want = pf.march(rows, pf.LO, pf.HI, degree, *rays, step_scale, 0.0, max_steps, WHITE)
    assert want[3].max() == min(max_steps, 166) and (want[3] > 64).mean() > 0.2
    compare(gpu_march(_baked(rows, degree), rays, step_scale=step_scale, max_steps=max_steps), want, rays, f"degree {degree}, {max_steps} steps")


@pytest.mark.parametrize("dilate", [0, 1])
def test_march_with_an_occupancy_grid(rays, dilate):
    from mipnerf_pl_amd import ops
    degree = 1
    rows, _ = pf.random_rows(degree, hollow=True)
    sigma = torch.from_numpy(rows[..., 0].astype(np.float32)).to(DEV)
    occ = ops.occupancy_grid(sigma, 5.0, pf.LO, pf.HI, dilate=dilate)
    words = occ.bits.cpu().numpy().view(np.uint32)
    share = occ.occupied_fraction()
    assert 0.3 < share < 0.9
    want = pf.march(rows, pf.LO, pf.HI, degree, *rays, 0.5, 0.0, 4096, WHITE, occupancy=words)
    got = gpu_march(_baked(rows, degree, occ), rays)
    compare(got, want, rays, f"occupancy, dilate {dilate}")
    free = pf.march(rows, pf.LO, pf.HI, degree, *rays, 0.5, 0.0, 4096, WHITE)
    skipped = (want[3] == 0) & (free[3] > 0) & ~want[4]              # in the box, every sample in a clear cell
    assert skipped.sum() >= 3 and (want[3] < free[3]).mean() > 0.3
    assert (got[3][skipped] == 0).all() and (got[1][skipped] == 0).all() and (got[0][skipped] == 1).all()
    assert np.array_equal(got[2][skipped], rays[2][skipped])
    # the same field with a null grid marches every cell
    compare(gpu_march(_baked(rows, degree), rays), free, rays, "occupancy null")


def test_early_stop_shortens_opaque_rays_and_costs_at_most_t_min(rays):
    rows, _ = pf.random_rows(2, opaque=True)
    baked = _baked(rows, 2)
    full = gpu_march(baked, rays, step_scale=0.1)
    cut = gpu_march(baked, rays, step_scale=0.1, t_min=1e-2)
    hit = full[3] > 0
    assert hit.sum() > 200
    assert (cut[3] <= full[3]).all() and (cut[3][hit] < full[3][hit]).mean() >= 0.5
    # the rest of the ray weighs at most T < t_min in every output the weights sum into
    assert np.abs(cut[0] - full[0]).max() <= 1e-2 and np.abs(cut[1] - full[1]).max() <= 1e-2
    want = pf.march(rows, pf.LO, pf.HI, 2, *rays, 0.1, 1e-2, 4096, WHITE)
    assert (np.abs(cut[3] - want[3]) <= 1)[~want[4]].all()          # T crosses t_min at the same sample, or at a neighbour when it is close


def test_a_nan_row_poisons_only_the_rays_through_it(rays):
    rows, _ = pf.random_rows(1)
    clean = gpu_march(_baked(rows, 1), rays)
    rows = rows.copy()
    rows[4, 4, 3, 0] = np.nan
    rows[7, 2, 5, 3] = np.nan
    want = pf.march(rows, pf.LO, pf.HI, 1, *rays, 0.5, 0.0, 4096, WHITE)
    got = gpu_march(_baked(rows, 1), rays)
    bad = np.isnan(want[1]) | np.isnan(want[0]).any(-1)
    sure = ~want[4]
    assert bad.sum() > 0
    assert (np.isnan(got[0]).any(-1) == bad)[sure].all()
    assert np.isnan(got[2][np.isnan(want[2]) & sure]).all()
    same = ~bad & sure
    assert np.array_equal(got[0][same], clean[0][same]) and np.array_equal(got[3][sure], clean[3][sure])


def test_two_runs_and_a_captured_replay_give_the_same_bytes(rays):
    from mipnerf_pl_amd import preview
    rows, _ = pf.random_rows(2)
    baked = _baked(rows, 2)
    o, d, tn, tf = [torch.from_numpy(a).to(DEV) for a in rays]
    outs = []
    for _ in range(2):
        steps = torch.zeros(pf.N_RAYS, dtype=torch.int32, device=DEV)
        outs.append([t.clone() for t in preview.march(baked, o, d, tn, tf, WHITE, 0.1, 1e-3, 4096, steps=steps)] + [steps])
    for a, b in zip(*outs):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    static = (torch.zeros(pf.N_RAYS, 3, device=DEV), torch.zeros(pf.N_RAYS, device=DEV), torch.zeros(pf.N_RAYS, device=DEV))
    steps = torch.zeros(pf.N_RAYS, dtype=torch.int32, device=DEV)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        preview.march(baked, o, d, tn, tf, WHITE, 0.1, 1e-3, 4096, out=static, steps=steps)
    for t in static:
        t.zero_()
    g.replay()
    torch.cuda.synchronize()
    for a, b in zip(outs[0], list(static) + [steps]):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))


@pytest.mark.parametrize("degree", [0, 1, 2])
def test_pack_equals_the_numpy_packing_byte_for_byte(degree):
    from mipnerf_pl_amd import preview
    rng = np.random.default_rng(degree)
    nx, ny, nz = 7, 5, 3
    nb = (degree + 1) ** 2
    sigma = rng.uniform(0, 50, (nz, ny, nx)).astype(np.float32)
    sigma.reshape(-1)[:8] = [1e6, 65504.0, 65519.0, 65520.0, np.inf, 0.0, 6e-8, np.nan]
    coef = rng.normal(0, 3, (nz, ny, nx, nb, 3)).astype(np.float32)
    coef.reshape(-1)[:6] = [1e6, -1e6, np.nan, 2.0 ** -25, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11]      # inf, -inf, NaN, a tie to zero, ties to even
    mask = rng.uniform(size=(nz, ny, nx)) < 0.6
    for m in (None, mask):
        got = preview.pack_rows(torch.from_numpy(sigma).to(DEV), torch.from_numpy(coef).to(DEV), degree,
                                mask=None if m is None else torch.from_numpy(m).to(DEV))
        assert got.dtype == torch.float16 and tuple(got.shape) == (nz, ny, nx, pf.ROW_HALVES[degree])
        got = got.cpu().numpy()
        want = pf.pack_rows(sigma, coef, degree, m)
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(got), nan) and np.array_equal(got.view(np.uint16)[~nan], want.view(np.uint16)[~nan])
        assert got.reshape(-1, got.shape[-1])[0, 0] == np.float16(65504.0) and np.isfinite(got[..., 0].reshape(-1)[:5]).all()      # saturated, not inf
        assert (got[..., 1 + 3 * nb:] == 0).all()
        if m is not None:
            assert (got[~m][:, 1:] == 0).all() and np.array_equal(got[~m][:, 0].view(np.uint16), want[~m][:, 0].view(np.uint16))


def _model(num_samples=16, seed=0, **kw):
    from mipnerf_pl_amd import MipNerf
    from oracle import mipnerf_oracle as orc
    model = MipNerf(num_samples=num_samples, precision="fp32", **kw)
    if not kw:
        params = orc.make_params(seed=seed, density_gain=40.0)
        model.load_state_dict({"mlp." + k: torch.from_numpy(v.copy()) for k, v in params.items()})
    return model.to(DEV).eval()


def test_bake_field_is_made_of_the_public_ops(tmp_path):
    from mipnerf_pl_amd import ops, preview
    model = _model()
    dims, lo, hi = (10, 11, 12), (-1.0, -1.1, -1.2), (1.1, 1.2, 1.3)
    nx, ny, nz = dims
    with torch.no_grad():
        sigma = ops.density_grid(model, dims, lo, hi)
    threshold = float(torch.quantile(sigma.reshape(-1), 0.97))      # a few raw-occupied cells, whether the field is smooth or noisy
    baked = preview.bake_field(model, grid=dims, degree=1, lo=lo, hi=hi, threshold=threshold, dilate=0, precision="fp32")
    assert baked.dims == dims and baked.degree == 1 and baked.threshold == threshold and tuple(baked.rows.shape) == (nz, ny, nx, 16)
    assert baked.nbytes == nz * ny * nx * 32 + baked.occupancy.bits.numel() * 4
    rows = baked.rows.cpu().numpy()
    assert np.array_equal(rows[..., 0].view(np.uint16), sigma.half().cpu().numpy().view(np.uint16))
    # the baked set: some adjacent cell occupied, from the words
    occ = ops.occupancy_grid(sigma, threshold, lo, hi, dilate=0)
    words = occ.bits.cpu().numpy().view(np.uint32)
    assert np.array_equal(words, baked.occupancy.bits.cpu().numpy().view(np.uint32))
    cells = np.array([[[pf.occupancy_bit(words, i, j, k) for i in range(nx - 1)] for j in range(ny - 1)] for k in range(nz - 1)])
    pts = np.zeros((nz, ny, nx), bool)
    for k in range(nz):
        for j in range(ny):
            for i in range(nx):
                pts[k, j, i] = cells[max(k - 1, 0):k + 1, max(j - 1, 0):j + 1, max(i - 1, 0):i + 1].any()
    assert 0.02 < pts.mean() < 0.98
    assert np.array_equal((rows[..., 1:] != 0).any(-1), pts)           # unbaked points are zero (and no baked point is all zeros)
    assert abs(baked.baked_share() - pts.mean()) < 1e-6
    # the coefficients: field_at per direction at the lattice Gaussians, fit_sh, rounded to fp16
    F = np.float32
    h = (np.array(hi, F) - np.array(lo, F)) / (np.array(dims) - 1).astype(F)
    kk, jj, ii = np.nonzero(pts)
    means = np.array(lo, F) + np.stack([ii, jj, kk], -1).astype(F) * h
    var = np.broadcast_to((F(1.0) * h * h) / F(12.0), means.shape).copy()
    dirs = preview.bake_directions(32)
    mt, vt = torch.from_numpy(means).to(DEV), torch.from_numpy(var).to(DEV)
    with torch.no_grad():
        rgb = torch.stack([ops.field_at(model, mt, vt, dirs[k].float().to(DEV).expand(len(ii), 3), precision="fp32")[:, :3] for k in range(32)], 1)
    want = preview.fit_sh(rgb, dirs, 1).half().cpu().numpy().reshape(-1, 12)
    assert np.array_equal(rows[pts][:, 1:13].view(np.uint16), want.view(np.uint16))
    assert (rows[..., 13:] == 0).all()
    # one .npz, equal bytes
    path = baked.save(str(tmp_path / "baked.npz"))
    again = preview.BakedField.load(path, DEV)
    assert torch.equal(again.rows.view(torch.int16), baked.rows.view(torch.int16)) and again.dims == dims and again.lo == baked.lo
    assert torch.equal(again.occupancy.bits.view(torch.int32), baked.occupancy.bits.view(torch.int32)) and again.threshold == baked.threshold
    # and it renders: rays through the box give the same bytes from both
    rays = pf.scene_rays()
    o, d, tn, tf = [torch.from_numpy(a).to(DEV) for a in rays]
    a = preview.march(baked, o, d, tn, tf, WHITE)
    b = preview.march(again, o, d, tn, tf, WHITE)
    assert all(torch.equal(x, y) or (torch.isnan(x) == torch.isnan(y)).all() for x, y in zip(a, b))
    assert float(a[1].max()) > 0.5


def test_bake_field_refuses_unbounded_and_one_level_models():
    from mipnerf_pl_amd import preview
    for model, word in ((_model(unbounded=True), "unbounded=True"), (_model(num_levels=1), "two-level")):
        with pytest.raises(NotImplementedError, match=word):
            preview.bake_field(model, grid=8, lo=-1.0, hi=1.0)


def _pngs(root):
    out = {}
    for d, _, fs in os.walk(root):
        for f in fs:
            if f.endswith(".png") and f[:5].isdigit():
                with open(os.path.join(d, f), "rb") as fh:
                    out[os.path.relpath(os.path.join(d, f), root)] = fh.read()
    return out


def test_the_command_end_to_end(tmp_path, capsys):
    """python -m mipnerf_pl_amd.preview on a checkpoint written by MipNeRFSystem (made as tests/test_gpu_eval.py makes one): the PNGs and
    the `preview:` line, --save_baked then --baked with the same PNG bytes, --data --compare with its three PSNRs (no threshold: the
    baked picture is not the MLP's)."""
    import re
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
    folder = preview.main(common + ["--out_dir", out, "--save_baked"])
    assert folder == os.path.join(out, "preview_spheric", "cli")
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("preview:")]
    assert re.fullmatch(r"preview: lattice 24 x 24 x 24, degree 1, baked share [0-9.]+, [0-9.]+ MiB, baked in [0-9.]+ ms, "
                        r"mean [0-9.]+ ms per frame \(2 frames\)", lines[-1]), lines
    first = _pngs(folder)
    assert sorted(first) == sorted(os.path.join("1", f"{i:05d}_{t}.png") for i in range(2) for t in ("rgb", "dist", "acc"))
    from PIL import Image
    assert np.array(Image.open(os.path.join(folder, "1", "00000_rgb.png"))).shape == (16, 16, 3)
    baked = os.path.join(folder, "baked.npz")
    assert os.path.exists(baked)
    out_b = str(tmp_path / "b")
    preview.main(common + ["--out_dir", out_b, "--baked", baked])
    assert "loaded in" in capsys.readouterr().out
    assert _pngs(os.path.join(out_b, "preview_spheric", "cli")) == first
    data = write_blender(str(tmp_path / "data"), seed=6, counts=(("test", 2),), w=16, h=16)
    preview.main(common + ["--out_dir", str(tmp_path / "c"), "--data", data, "--compare"])
    text = capsys.readouterr().out
    m = re.search(r"preview: mean PSNR over 2 test images: baked vs photos ([0-9.]+), MLP vs photos ([0-9.]+), baked vs MLP ([0-9.]+)", text)
    assert m, text
    print("PSNR baked / MLP / baked-vs-MLP:", m.groups())
    assert all(np.isfinite(float(v)) for v in m.groups())
