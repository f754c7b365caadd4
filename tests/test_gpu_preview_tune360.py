"""GPU: tuning the contracted preview lattice (libmipnerf_preview_tune_360.so, mipnerf_pl_amd.preview_tune360) --
mipnerf_preview_tune_360_grad against the float64 fixture of tests/preview_tune360_fixture.py on the scene of tests/preview360_fixture.py
(a 9 x 10 x 11 lattice over a non-cubic box of the contracted space, far radius 8, 270 rays with a ragged last block; step 0.05 gives up
to 271 counted samples per ray, so carries, the carried edge and combined runs cross block boundaries), its exact structure, convergence
through `TuneState360.step`, `reoccupy`, and the command end to end.

Bound of the gradient: scaled error |got - want| / (A_e + 1e-3 max_e A_e) <= preview_tune360_fixture.LIMIT, 4 x what the fixture's own
float32 run shows against its float64 run on the same inputs (test_preview_tune360_cpu.py measures it without a GPU), on the rays the
fixture does not call fragile.  The sums over rays are float atomics: two launches may differ in the last bits, so nothing that crosses
rays is compared bit for bit."""
import os
import re

import numpy as np
import pytest
import torch

import preview360_fixture as pf
import preview_tune360_fixture as tf

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32
WHITE = (1.0, 1.0, 1.0)
R = tf.R


@pytest.fixture(scope="module")
def rays():
    return pf.scene_rays()


def _occupancy(words):
    from mipnerf_pl_amd import ops
    occ = ops.Occupancy(torch.from_numpy(np.ascontiguousarray(words).view(np.int32)).to(DEV).view(torch.uint32), pf.DIMS, pf.LO, pf.HI,
                        space="contracted")
    occ.threshold, occ.dilate = 0.0, 0
    return occ


def _baked(rows, degree, words=None):
    from mipnerf_pl_amd import preview
    return preview.BakedField(torch.from_numpy(np.ascontiguousarray(rows)).to(DEV), pf.DIMS, pf.LO, pf.HI, degree,
                              None if words is None else _occupancy(words), space="contracted", far_radius=R)


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def gpu_grad(baked, rays, step, t_min, background, select=None, grad_rows=None, counters=None, **side):
    """(grad_rows, rgb, acc) as numpy, of the rays `select` (default: all)"""
    from mipnerf_pl_amd import preview_tune360 as pt
    pick = lambda a: a if select is None or a is None or np.isscalar(a) else a[select]
    o, d, tn, tf_ = [_dev(pick(a)) for a in rays]
    side = {k: (v if np.isscalar(v) else _dev(pick(v))) for k, v in side.items()}
    grad, rgb, acc = pt.march_grad(baked, o, d, tn, tf_, background, step_scale=step, t_min=t_min, max_steps=4096, grad_rows=grad_rows,
                                   counters=counters, **side)
    torch.cuda.synchronize()
    return grad.cpu().numpy(), rgb.cpu().numpy(), acc.cpu().numpy()


@pytest.mark.parametrize("degree", [0, 1, 2])
def test_rgb_and_acc_are_the_march_bit_for_bit(rays, degree):
    from mipnerf_pl_amd import preview, preview_tune360 as pt
    G, ga, target = tf.loss_inputs(n=pf.N_RAYS)
    o, d, tn, tf_ = [_dev(a) for a in rays]
    for hollow in (False, True):
        rows = tf.scene_rows(degree, hollow=hollow)
        baked = _baked(rows, degree, tf.occupancy_of(rows) if hollow else None)
        for step, t_min in ((0.5, 0.0), (0.05, 1e-3)):
            want = preview.march(baked, o, d, tn, tf_, tf.BG, step, t_min, 4096)
            for side in (dict(grad_rgb=_dev(G), grad_acc=_dev(ga)), dict(target=_dev(target), loss_scale=0.5)):
                _, rgb, acc = pt.march_grad(baked, o, d, tn, tf_, tf.BG, step_scale=step, t_min=t_min, max_steps=4096, **side)
                assert torch.equal(rgb, want[0]) and torch.equal(acc, want[1]), (degree, hollow, step, sorted(side))
            assert float(want[1].max()) > 0.5


@pytest.mark.parametrize("degree", [0, 1, 2])
def test_gradient_against_the_fixture(rays, degree):
    for case, (step, t_min, hollow) in enumerate(tf.CASES):
        rows, words, ok = tf.case_inputs(degree, case)
        baked = _baked(rows, degree, words)
        for mode in tf.MODES:
            want = tf.reference(degree, case, mode)
            got, rgb, acc = gpu_grad(baked, rays, step, t_min, tf.BG, select=ok, **tf.loss_side(mode))
            err = float(tf.scaled_error(got, want["grad"], want["A"]).max())
            print(f"degree {degree} step {step} t_min {t_min} hollow {hollow} {mode}: scaled error {err:.3e} (limit {tf.LIMIT[mode]:.2e}, "
                  f"ratio {err / tf.LIMIT[mode]:.2f})")
            assert err <= tf.LIMIT[mode], (degree, tf.CASES[case], mode, err)
            assert (got[want["count"] == 0] == 0.0).all()                    # entries nothing contributes to: exactly 0.0
            assert np.abs(rgb - want["rgb"][ok]).max() <= 5e-5 and np.abs(acc - want["acc"][ok]).max() <= 5e-5


def test_exact_structure(rays):
    from mipnerf_pl_amd import preview
    G, ga, target = tf.loss_inputs(n=pf.N_RAYS)
    misses = np.array([b for b in range(pf.N_RAYS) if not pf.Ray(rays[0][b], rays[1][b], rays[2][b], rays[3][b], R).hit])
    assert len(misses) == 10
    for degree in (0, 1, 2):
        rows = tf.scene_rows(degree)
        baked = _baked(rows, degree)
        # G = 0 (and no grad_acc) leaves a pre-filled grad_rows bitwise unchanged
        filled = torch.from_numpy(np.random.default_rng(1).normal(size=rows.shape).astype(F)).to(DEV)
        before = filled.clone()
        gpu_grad(baked, rays, 0.5, 0.0, WHITE, grad_rows=filled, grad_rgb=np.zeros((pf.N_RAYS, 3), F))
        assert torch.equal(filled.view(torch.int32), before.view(torch.int32))
        # the rays that miss (C2), alone: nothing is added
        got, rgb, acc = gpu_grad(baked, rays, 0.5, 0.0, WHITE, select=misses, grad_rows=filled, grad_rgb=G, grad_acc=ga)
        assert torch.equal(filled.view(torch.int32), before.view(torch.int32)) and (acc == 0).all() and (rgb == 1).all()
        # a non-finite G or g_a adds nothing either
        bad_G = G.copy()
        bad_G[::2, 1] = np.nan
        bad_G[1::2, 0] = np.inf
        gpu_grad(baked, rays, 0.5, 0.0, WHITE, grad_rows=filled, grad_rgb=bad_G)
        assert torch.equal(filled.view(torch.int32), before.view(torch.int32))
        bad_ga = np.full(pf.N_RAYS, np.nan, F)
        gpu_grad(baked, rays, 0.5, 0.0, WHITE, grad_rows=filled, grad_rgb=G, grad_acc=bad_ga)
        assert torch.equal(filled.view(torch.int32), before.view(torch.int32))
        # the output accumulates: two launches equal the sum (one ray: its adds arrive in a fixed order)
        one = np.array([4])                                          # at step 0.05 this ray has more than 128 counted samples
        first, _, _ = gpu_grad(baked, rays, 0.05, 0.0, WHITE, select=one, grad_rgb=G, grad_acc=ga)
        assert np.count_nonzero(first) > 8
        twice = torch.zeros(rows.shape, dtype=torch.float32, device=DEV)
        gpu_grad(baked, rays, 0.05, 0.0, WHITE, select=one, grad_rows=twice, grad_rgb=G, grad_acc=ga)
        gpu_grad(baked, rays, 0.05, 0.0, WHITE, select=one, grad_rows=twice, grad_rgb=G, grad_acc=ga)
        # (a ray's cells share corner rows, so an entry is a running sum of up to 8 flushes and ((a + b) + a) + b is not 2 (a + b) to
        # the bit: 16 roundings of a running sum below 2 A_e, each at most 2^-24 of it, bound the distance by 2^-19 A_e)
        A = tf.march_grad(rows, pf.LO, pf.HI, degree, R, *rays, 0.05, 0.0, 4096, WHITE, grad_rgb=G, grad_acc=ga, rays=one)
        assert A["steps"][4] > 128                                   # the ray passes two block boundaries
        twice = twice.cpu().numpy()
        assert (np.abs(twice - 2 * first.astype(np.float64)) <= 2.0 ** -19 * A["A"]).all() and (twice[A["count"] == 0] == 0).all()
        assert np.abs(twice).sum() > 1.5 * np.abs(first).sum()
        # the pad entries are never written
        gpu_grad(baked, rays, 0.5, 0.0, WHITE, grad_rows=filled, grad_rgb=G, grad_acc=ga)
        assert torch.equal(filled[..., tf.USED[degree]:], before[..., tf.USED[degree]:]) and not torch.equal(filled, before)
        # a single ray: grad_rgb and grad_acc scaled by 2 give exactly twice the gradient
        double, _, _ = gpu_grad(baked, rays, 0.05, 0.0, WHITE, select=one, grad_rgb=F(2) * G, grad_acc=F(2) * ga)
        assert np.array_equal(double, F(2) * first)
        # target mode equals grad mode fed loss_scale * (rgb - target) from the march's own rgb, bit for bit
        o, d, tn, tf_ = [_dev(a[one]) for a in rays]
        rgb = preview.march(baked, o, d, tn, tf_, WHITE, 0.05, 0.0, 4096)[0].cpu().numpy()
        fed = F(0.37) * (rgb - target[one])
        a, _, _ = gpu_grad(baked, [r[one] for r in rays], 0.05, 0.0, WHITE, target=target[one], loss_scale=0.37)
        b, _, _ = gpu_grad(baked, [r[one] for r in rays], 0.05, 0.0, WHITE, grad_rgb=fed)
        assert np.array_equal(a, b) and np.count_nonzero(a) > 8


def test_counters_count_samples_and_runs(rays):
    """the debug counters against the fixture: samples that added something and flushes (runs of consecutive samples in one cell)"""
    for case in (0, 2):
        rows, words, ok = tf.case_inputs(1, case)
        want = tf.reference(1, case, "grad")
        counters = torch.zeros(2, dtype=torch.int64, device=DEV)
        step, t_min, _ = tf.CASES[case]
        gpu_grad(_baked(rows, 1, words), rays, step, t_min, tf.BG, select=ok, counters=counters, **tf.loss_side("grad"))
        samples, flushes = tf.runs({b: want["cells"][int(b)] for b in ok})
        print(f"step {step}: {samples} samples, {flushes} flushes: {flushes / samples:.3f} flushes per sample")
        assert counters.tolist() == [samples, flushes] and flushes < samples


def test_a_nan_row_spoils_its_rays_and_adds_nothing(rays):
    degree = 1
    rows = tf.scene_rows(degree).copy()
    rows[5, 5, 4, 0] = np.float16(np.nan)
    rows[6, 3, 6, 7] = np.float16(np.nan)
    G, ga, _ = tf.loss_inputs(n=pf.N_RAYS)
    fragile = pf.march(rows, pf.LO, pf.HI, degree, R, *rays, 0.5, 0.0, 4096, tf.BG)[4]
    ok = np.flatnonzero(~fragile)
    want = tf.march_grad(rows, pf.LO, pf.HI, degree, R, *rays, 0.5, 0.0, 4096, tf.BG, grad_rgb=G, grad_acc=ga, rays=ok)
    spoiled = ~np.isfinite(want["rgb"][ok]).all(-1)
    assert 5 <= spoiled.sum() < len(ok) // 2
    got, rgb, acc = gpu_grad(_baked(rows, degree), rays, 0.5, 0.0, tf.BG, select=ok, grad_rgb=G, grad_acc=ga)
    assert np.array_equal(~np.isfinite(rgb).all(-1), spoiled) and np.isfinite(got).all()
    assert float(tf.scaled_error(got, want["grad"], want["A"]).max()) <= tf.LIMIT["grad"]
    assert (got[want["count"] == 0] == 0.0).all()


def _rays_of(rays, ok):
    from mipnerf_pl_amd.rays import Rays
    o, d, tn, tf_ = [_dev(a[ok]) for a in rays]
    z = torch.zeros(len(ok), 1, device=DEV)
    return Rays(o, d, d, z, z, tn[:, None], tf_[:, None])


def test_convergence_the_state_reoccupy_and_the_sparse_form(rays):
    """the recipe of test_preview_tune360_cpu.py (the reference alone reaches CONVERGENCE_RATIO of the starting loss in 40 steps) through
    `TuneState360.step`: at most 10 x that ratio, the bounded test's factor (0.05 against 0.0047)"""
    from mipnerf_pl_amd import preview, preview_tune360 as pt
    teacher = tf.scene_rows(1)
    want = pf.march(teacher, pf.LO, pf.HI, 1, R, *rays, 0.5, 1e-3, 4096, WHITE)
    ok = np.flatnonzero(~want[4])
    target = _dev(want[0].astype(F)[ok])
    student = tf.student_rows(teacher, 1)
    every = tf.occupancy_of(np.ones_like(student))                             # every cell occupied: the mask keeps every point
    baked = _baked(student, 1, every)
    batch = _rays_of(rays, ok)
    state, losses = pt.tune_field(baked, lambda k: (batch, target), 41, WHITE, lr_sigma=0.2, lr_colour=0.02, t_min=1e-3)
    losses = losses.cpu().numpy()
    print(f"loss {losses[0]:.3e} -> {losses[40]:.3e} (ratio {losses[40] / losses[0]:.4f}, the reference alone {tf.CONVERGENCE_RATIO})")
    assert abs(losses[0] - 1.027e-3) < 2e-5 and losses[40] <= 10 * tf.CONVERGENCE_RATIO * losses[0]
    assert isinstance(state, pt.TuneState360) and state.steps == 41 and not bool(state.grad.any())
    assert torch.equal(preview.pack_master(state.master, 1), baked.rows) and not torch.equal(baked.rows, _dev(student))
    # the state round-trips
    again = pt.TuneState360(_baked(student, 1, every))
    again.load_state_dict(state.state_dict())
    assert torch.equal(again.baked.rows, baked.rows) and again.steps == 41
    # a regularised step goes through preview.tune_regularise and still moves the rows
    reg = pt.TuneState360(_baked(student, 1, every), tv_sigma=1e-2, t_min=1e-3)
    reg.step(batch, target, WHITE)
    assert reg.regularised and reg.n_points == student[..., 0].size and not torch.equal(reg.baked.rows, _dev(student))
    # reoccupy on a tuned hollow lattice: the words of its own sigma; its sparse march equals its dense march bit for bit
    rows = tf.scene_rows(1, hollow=True)
    hollow = _baked(rows, 1, tf.occupancy_of(rows))
    pt.tune_field(hollow, lambda k: (batch, target), 3, WHITE, t_min=1e-3)
    assert not torch.equal(hollow.rows, _dev(rows))
    sigma = hollow.rows[..., 0].float().cpu().numpy()
    share = pt.reoccupy(hollow, 0.3, dilate=0)
    words = hollow.occupancy.bits.cpu().numpy().view(np.uint32)
    expect = pf.occupancy_words(sigma, 0.3)
    assert np.array_equal(words, expect) and hollow.occupancy.space == "contracted" and hollow.threshold == 0.3
    cells = (pf.DIMS[0] - 1) * (pf.DIMS[1] - 1) * (pf.DIMS[2] - 1)
    assert abs(share - int(np.unpackbits(expect.view(np.uint8)).sum()) / cells) < 1e-12 and 0.05 < share < 0.95
    o, d, tn, tf_ = [_dev(a) for a in rays]
    dense = preview.march(hollow, o, d, tn, tf_, WHITE)
    sparse = preview.march(hollow.to_sparse(), o, d, tn, tf_, WHITE)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(sparse, dense))


def test_the_other_kinds_are_refused_on_the_device(rays):
    from mipnerf_pl_amd import preview, preview_tune360 as pt
    rows = tf.scene_rows(1, hollow=True)
    baked = _baked(rows, 1, tf.occupancy_of(rows))
    o, d, tn, tf_ = [_dev(a) for a in rays]
    G = torch.zeros(pf.N_RAYS, 3, device=DEV)
    with pytest.raises(NotImplementedError, match="SparseField is not a tuning target"):
        pt.march_grad(baked.to_sparse(), o, d, tn, tf_, WHITE, grad_rgb=G)
    with pytest.raises(NotImplementedError, match="SparseField is not a tuning target"):
        pt.TuneState360(baked.to_sparse())
    world = preview.BakedField(baked.rows, pf.DIMS, pf.LO, pf.HI, 1)
    with pytest.raises(ValueError, match=r"preview\.march_grad"):
        pt.march_grad(world, o, d, tn, tf_, WHITE, grad_rgb=G)
    with pytest.raises(NotImplementedError, match=r"contracted.*preview_tune360"):
        preview.march_grad(baked, o, d, tn, tf_, WHITE, grad_rgb=G)
    with pytest.raises(ValueError, match=r"out\[0\] \(rgb\) must be a contiguous fp32 tensor"):
        pt.march_grad(baked, o, d, tn, tf_, WHITE, grad_rgb=G, out=(torch.empty(3, 3, device=DEV), torch.empty(pf.N_RAYS, device=DEV)))


def test_the_command_end_to_end(tmp_path, capsys):
    """python -m mipnerf_pl_amd.preview_tune360 on a llff checkpoint of the unbounded-scene model and the capture of
    tests/scene360_fixture.py: 3 steps of 512 rays with --compare; the two lines, the saved contracted lattice with changed rows, and the
    unchanged `preview --space contracted --baked` renders it"""
    import scene360_fixture as sf
    from mipnerf_pl_amd import preview, preview_tune360 as pt
    from mipnerf_pl_amd.system import DEFAULT_HPARAMS, MipNeRFSystem
    data = sf.write_scene360_llff(str(tmp_path / "scene"), views=6, w=24, h=18, steps=32)
    hp = dict(DEFAULT_HPARAMS)
    hp.update({"nerf.num_samples": 16, "nerf.unbounded": True, "exp_name": "cli360", "val.batch_type": "single_image", "dataset_name": "llff",
               "factor": 2, "val.white_bkgd": False, "train.white_bkgd": False})
    torch.manual_seed(4)
    ckpt = str(tmp_path / "last.ckpt")
    MipNeRFSystem(hp, precision="fp32").save_checkpoint(ckpt)
    bake = ["--grid", "16", "--precision", "fp32", "--threshold", "-1"]
    common = ["--ckpt", ckpt, "--data", data]
    # the untuned lattice, saved by the preview command itself
    preview.main(common + ["--space", "contracted", "--n_views", "6", "--out_dir", str(tmp_path / "u"), "--save_baked"] + bake)
    untuned = preview.BakedField.load(os.path.join(str(tmp_path / "u"), "preview_path", "cli360", "baked.npz"), DEV)
    capsys.readouterr()
    out = str(tmp_path / "t")
    folder = pt.main(common + ["--out_dir", out, "--steps", "3", "--batch", "512", "--compare", "--far_radius", repr(untuned.far_radius)] + bake)
    assert folder == os.path.join(out, "preview_tune360", "cli360")
    lines = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("preview_tune360:")]
    m = re.fullmatch(r"preview_tune360: tuned 3 steps of 512 rays against the photos in [0-9.]+ s \([0-9.]+ ms per step\), batch loss "
                     r"([0-9.e+-]+) -> ([0-9.e+-]+)", lines[0])
    assert m and all(np.isfinite(float(v)) and float(v) > 0 for v in m.groups()), lines
    c = re.fullmatch(r"preview_tune360: tuning moved the mean PSNR over (\d+) test images: vs photos ([0-9.]+) -> ([0-9.]+), vs MLP ([0-9.]+) -> "
                     r"([0-9.]+)", lines[1])
    assert c and int(c.group(1)) >= 1 and all(np.isfinite(float(v)) for v in c.groups()[1:]), lines
    print("PSNR vs photos before / after, vs MLP before / after:", c.groups()[1:])
    saved = os.path.join(folder, "baked.npz")
    assert lines[-1] == f"preview_tune360: lattice saved to {saved}"
    assert preview.BakedField.stored_space(saved) == "contracted"
    tuned = preview.BakedField.load(saved, DEV)
    assert tuned.space == "contracted" and tuned.far_radius == untuned.far_radius and tuned.dims == (16, 16, 16) and tuned.degree == 1
    assert not torch.equal(tuned.rows, untuned.rows) and torch.equal(tuned.occupancy.bits, untuned.occupancy.bits)
    rendered = preview.main(common + ["--space", "contracted", "--n_views", "6", "--out_dir", str(tmp_path / "r"), "--baked", saved])
    assert "loaded in" in capsys.readouterr().out and os.path.exists(os.path.join(rendered, "1", "00000_rgb.png"))
    # --baked FILE tunes that file further; --target mlp, --reoccupy and --sparse: the file is a sparse contracted lattice
    pt.main(common + ["--out_dir", str(tmp_path / "s"), "--steps", "2", "--batch", "512", "--baked", saved, "--target", "mlp", "--tv_sigma", "1e-3",
                      "--reoccupy", "0.0", "--sparse"])
    text = capsys.readouterr().out
    assert "against the MLP" in text and "regularised with tv_sigma 0.001" in text and "occupancy rebuilt from the tuned density" in text
    again = preview.SparseField.load(os.path.join(str(tmp_path / "s"), "preview_tune360", "cli360", "baked.npz"), DEV)
    assert again.space == "contracted" and again.far_radius == untuned.far_radius
    # refused once the checkpoint is read: a bounded checkpoint
    hp["nerf.unbounded"], hp["dataset_name"] = False, "blender"
    bounded = str(tmp_path / "bounded.ckpt")
    MipNeRFSystem(hp, precision="fp32").save_checkpoint(bounded)
    with pytest.raises(SystemExit, match="bounded model"):
        pt.main(["--ckpt", bounded, "--data", data, "--out_dir", str(tmp_path / "x"), "--steps", "3"])
    assert not os.path.exists(str(tmp_path / "x"))
