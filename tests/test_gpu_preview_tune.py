"""GPU: tuning the baked preview's lattice (libmipnerf_preview_tune.so, mipnerf_pl_amd.preview) -- mipnerf_preview_tune_grad against the
float64 fixture of tests/preview_tune_fixture.py on the scene of the other preview tests (an 8 x 9 x 10 lattice over a non-cubic box, 257
rays; step 0.1 gives three 64-sample blocks per ray, so carries and combined runs cross block boundaries), its exact structure,
mipnerf_preview_tune_adam byte for byte against the host build of csrc/preview_tune.hpp, convergence through `TuneState.step`, and the
command end to end.

Bound of the gradient: scaled error |got - want| / (A_e + 1e-3 max_e A_e) <= preview_tune_fixture.LIMIT, 4 x what the fixture's own
float32 run shows against its float64 run on the same inputs (3.8e-5 with a given grad_rgb, 1.52e-4 in target mode;
test_preview_tune_cpu.py measures it without a GPU), on the rays the fixture does not call fragile.  The sums over rays are float atomics:
two launches may differ in the last bits, so nothing that crosses rays is compared bit for bit."""
import os
import re

import numpy as np
import pytest
import torch

import preview_fixture as pf
import preview_tune_fixture as tf

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32
WHITE = (1.0, 1.0, 1.0)


@pytest.fixture(scope="module")
def rays():
    return pf.scene_rays()


def _occupancy(words):
    from mipnerf_pl_amd import ops
    occ = ops.Occupancy(torch.from_numpy(np.ascontiguousarray(words).view(np.int32)).to(DEV).view(torch.uint32), pf.DIMS, pf.LO, pf.HI)
    occ.threshold, occ.dilate = 0.0, 0
    return occ


def _baked(rows, degree, words=None):
    from mipnerf_pl_amd import preview
    return preview.BakedField(torch.from_numpy(np.ascontiguousarray(rows)).to(DEV), pf.DIMS, pf.LO, pf.HI, degree,
                              None if words is None else _occupancy(words))


def _dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def gpu_grad(baked, rays, step, t_min, background, select=None, grad_rows=None, counters=None, **side):
    """(grad_rows, rgb, acc) as numpy, of the rays `select` (default: all)"""
    from mipnerf_pl_amd import preview
    pick = lambda a: a if select is None or a is None or np.isscalar(a) else a[select]
    o, d, tn, tf_ = [_dev(pick(a)) for a in rays]
    side = {k: (v if np.isscalar(v) else _dev(pick(v))) for k, v in side.items()}
    grad, rgb, acc = preview.march_grad(baked, o, d, tn, tf_, background, step_scale=step, t_min=t_min, max_steps=4096, grad_rows=grad_rows,
                                        counters=counters, **side)
    torch.cuda.synchronize()
    return grad.cpu().numpy(), rgb.cpu().numpy(), acc.cpu().numpy()


@pytest.mark.parametrize("degree", [0, 1, 2])
def test_rgb_and_acc_are_the_march_bit_for_bit(rays, degree):
    from mipnerf_pl_amd import preview
    G, ga, target = tf.loss_inputs()
    o, d, tn, tf_ = [_dev(a) for a in rays]
    for hollow in (False, True):
        rows, _ = pf.random_rows(degree, hollow=hollow)
        baked = _baked(rows, degree, tf.occupancy_of(rows) if hollow else None)
        for step, t_min in ((0.5, 0.0), (0.1, 1e-3)):
            want = preview.march(baked, o, d, tn, tf_, tf.BG, step, t_min, 4096)
            for side in (dict(grad_rgb=_dev(G), grad_acc=_dev(ga)), dict(target=_dev(target), loss_scale=0.5)):
                _, rgb, acc = preview.march_grad(baked, o, d, tn, tf_, tf.BG, step_scale=step, t_min=t_min, max_steps=4096, **side)
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
            print(f"degree {degree} step {step} t_min {t_min} hollow {hollow} {mode}: scaled error {err:.3e} (limit {tf.LIMIT[mode]:.2e})")
            assert err <= tf.LIMIT[mode], (degree, tf.CASES[case], mode, err)
            assert (got[want["count"] == 0] == 0.0).all()                    # entries nothing contributes to: exactly 0.0
            assert np.abs(rgb - want["rgb"][ok]).max() <= 5e-5 and np.abs(acc - want["acc"][ok]).max() <= 5e-5


def test_exact_structure(rays):
    from mipnerf_pl_amd import preview
    G, ga, target = tf.loss_inputs()
    for degree in (0, 1, 2):
        rows = tf.scene_rows(degree)
        baked = _baked(rows, degree)
        # G = 0 (and no grad_acc) leaves a pre-filled grad_rows bitwise unchanged
        filled = torch.from_numpy(np.random.default_rng(1).normal(size=rows.shape).astype(F)).to(DEV)
        before = filled.clone()
        gpu_grad(baked, rays, 0.5, 0.0, WHITE, grad_rows=filled, grad_rgb=np.zeros((pf.N_RAYS, 3), F))
        assert torch.equal(filled.view(torch.int32), before.view(torch.int32))
        # the hand-made rays that miss or carry a NaN, alone: nothing is added
        steps = pf.march(rows, pf.LO, pf.HI, degree, *rays, 0.5, 0.0, 4096, WHITE)[3]
        hand = np.arange(pf.N_RAYS - 17, pf.N_RAYS)
        misses = hand[steps[hand] == 0]
        assert len(misses) >= 9
        got, rgb, acc = gpu_grad(baked, rays, 0.5, 0.0, WHITE, select=misses, grad_rows=filled, grad_rgb=G, grad_acc=ga)
        assert torch.equal(filled.view(torch.int32), before.view(torch.int32)) and (acc == 0).all() and (rgb == 1).all()
        # a non-finite G or g_a adds nothing either
        bad_G = G.copy()
        bad_G[::2, 1] = np.nan
        bad_G[1::2, 0] = np.inf
        gpu_grad(baked, rays, 0.5, 0.0, WHITE, grad_rows=filled, grad_rgb=bad_G)
        assert torch.equal(filled.view(torch.int32), before.view(torch.int32))
        # the output accumulates: two launches equal the sum (one ray: its adds arrive in a fixed order)
        one = np.array([3])
        first, _, _ = gpu_grad(baked, rays, 0.5, 0.0, WHITE, select=one, grad_rgb=G, grad_acc=ga)
        assert np.count_nonzero(first) > 8
        twice = torch.zeros(rows.shape, dtype=torch.float32, device=DEV)
        gpu_grad(baked, rays, 0.5, 0.0, WHITE, select=one, grad_rows=twice, grad_rgb=G, grad_acc=ga)
        gpu_grad(baked, rays, 0.5, 0.0, WHITE, select=one, grad_rows=twice, grad_rgb=G, grad_acc=ga)
        # (a ray's cells share corner rows, so an entry is a running sum of up to 8 flushes and ((a + b) + a) + b is not 2 (a + b) to
        # the bit: 16 roundings of a running sum below 2 A_e, each at most 2^-24 of it, bound the distance by 2^-19 A_e)
        A = tf.march_grad(rows, pf.LO, pf.HI, degree, *rays, 0.5, 0.0, 4096, WHITE, grad_rgb=G, grad_acc=ga, rays=one)
        twice = twice.cpu().numpy()
        assert (np.abs(twice - 2 * first.astype(np.float64)) <= 2.0 ** -19 * A["A"]).all() and (twice[A["count"] == 0] == 0).all()
        assert np.abs(twice).sum() > 1.5 * np.abs(first).sum()
        # the pad entries are never written
        assert torch.equal(filled[..., tf.USED[degree]:], before[..., tf.USED[degree]:])
        # a single ray: grad_rgb and grad_acc scaled by 2 give exactly twice the gradient
        double, _, _ = gpu_grad(baked, rays, 0.5, 0.0, WHITE, select=one, grad_rgb=F(2) * G, grad_acc=F(2) * ga)
        assert np.array_equal(double, F(2) * first)
        # target mode equals grad mode fed loss_scale * (rgb - target) from the march's own rgb, bit for bit
        o, d, tn, tf_ = [_dev(a[one]) for a in rays]
        rgb = preview.march(baked, o, d, tn, tf_, WHITE, 0.5, 0.0, 4096)[0].cpu().numpy()
        fed = F(0.37) * (rgb - target[one])
        a, _, _ = gpu_grad(baked, [r[one] for r in rays], 0.5, 0.0, WHITE, target=target[one], loss_scale=0.37)
        b, _, _ = gpu_grad(baked, [r[one] for r in rays], 0.5, 0.0, WHITE, grad_rgb=fed)
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
    rows[4, 4, 3, 0] = np.float16(np.nan)
    rows[5, 2, 5, 7] = np.float16(np.nan)
    G, ga, _ = tf.loss_inputs()
    fragile = pf.march(rows, pf.LO, pf.HI, degree, *rays, 0.5, 0.0, 4096, tf.BG)[4]
    ok = np.flatnonzero(~fragile)
    want = tf.march_grad(rows, pf.LO, pf.HI, degree, *rays, 0.5, 0.0, 4096, tf.BG, grad_rgb=G, grad_acc=ga, rays=ok)
    spoiled = ~np.isfinite(want["rgb"][ok]).all(-1)
    assert 5 <= spoiled.sum() < len(ok) // 2
    got, rgb, acc = gpu_grad(_baked(rows, degree), rays, 0.5, 0.0, tf.BG, select=ok, grad_rgb=G, grad_acc=ga)
    assert np.array_equal(~np.isfinite(rgb).all(-1), spoiled) and np.isfinite(got).all()
    assert float(tf.scaled_error(got, want["grad"], want["A"]).max()) <= tf.LIMIT["grad"]
    assert (got[want["count"] == 0] == 0.0).all()


def _same_bits(a, b):
    """equal bit for bit, except that a NaN only has to be a NaN (the one NaN gradient of `adam_inputs` spreads to its m, v, master and
    row entry, and which sign a subtraction leaves on a NaN differs between the device and the host)"""
    nan = np.isnan(b)
    bits = np.uint32 if a.dtype == np.float32 else np.uint16
    return a.dtype == b.dtype and np.array_equal(np.isnan(a), nan) and np.array_equal(a.view(bits)[~nan], b.view(bits)[~nan])


@pytest.mark.parametrize("degree", [0, 1, 2])
def test_adam_is_the_host_build_byte_for_byte(degree):
    from mipnerf_pl_amd import preview
    import test_preview_tune_cpu as cpu
    hm = cpu.host()
    n = 8 * 9 * 10
    for mask_on in (True, False):
        want, mask = cpu.adam_inputs(degree, n)
        got = [_dev(a) for a in want]
        mask_d = _dev(mask) if mask_on else None
        for step in (1, 2):
            c1, c2 = tf.bias_corrections(0.9, 0.999, step)
            scalars = (0.2, 0.01, 0.9, 0.999, 1e-8, c1, c2)
            cpu.host_adam(hm, *want, mask if mask_on else None, degree, scalars)
            preview.tune_adam(*got, degree, mask_d, *scalars)
            torch.cuda.synchronize()
            for a, b, name in zip(got, want, ("master", "m", "v", "grad", "rows")):
                assert _same_bits(a.cpu().numpy(), b), (degree, mask_on, step, name)
            fresh = np.random.default_rng(step).normal(size=want[3].shape).astype(F)
            want[3][...] = fresh
            got[3].copy_(_dev(fresh))


def _rays_of(rays, ok):
    from mipnerf_pl_amd.rays import Rays
    o, d, tn, tf_ = [_dev(a[ok]) for a in rays]
    z = torch.zeros(len(ok), 1, device=DEV)
    return Rays(o, d, d, z, z, tn[:, None], tf_[:, None])


def test_convergence_and_the_sparse_form_of_a_tuned_lattice(rays):
    """the recipe of test_preview_tune_cpu.py (the reference alone reaches 0.0047 of the starting loss in 40 steps) through
    `TuneState.step`: <= 0.05, the slack for fp32 gradients and their arrival order"""
    from mipnerf_pl_amd import preview
    teacher = tf.scene_rows(1)
    want = pf.march(teacher, pf.LO, pf.HI, 1, *rays, 0.5, 1e-3, 4096, WHITE)
    ok = np.flatnonzero(~want[4])
    target = _dev(want[0].astype(F)[ok])
    student = tf.student_rows(teacher, 1)
    baked = _baked(student, 1, tf.occupancy_of(np.ones_like(student)))          # every cell occupied: the mask keeps every point
    batch = _rays_of(rays, ok)
    state, losses = preview.tune_field(baked, lambda k: (batch, target), 41, WHITE, lr_sigma=0.2, lr_colour=0.02, t_min=1e-3)
    losses = losses.cpu().numpy()
    print(f"loss {losses[0]:.3e} -> {losses[40]:.3e} (ratio {losses[40] / losses[0]:.4f})")
    assert abs(losses[0] - 1.518e-3) < 2e-5 and losses[40] <= 0.05 * losses[0]
    assert state.steps == 41 and not bool(state.grad.any()) and torch.equal(preview.pack_master(state.master, 1), baked.rows)
    assert not torch.equal(baked.rows, _dev(student))
    # the state round-trips, and a tuned lattice still has its sparse form: the occupancy never changed
    again = preview.TuneState(_baked(student, 1, tf.occupancy_of(np.ones_like(student))))
    again.load_state_dict(state.state_dict())
    assert torch.equal(again.baked.rows, baked.rows) and again.steps == 41
    rows = tf.scene_rows(1, hollow=True)
    hollow = _baked(rows, 1, tf.occupancy_of(rows))
    preview.tune_field(hollow, lambda k: (batch, target), 3, WHITE, t_min=1e-3)
    assert not torch.equal(hollow.rows, _dev(rows))
    o, d, tn, tf_ = [_dev(a) for a in rays]
    dense = preview.march(hollow, o, d, tn, tf_, WHITE)
    sparse = preview.march(hollow.to_sparse(), o, d, tn, tf_, WHITE)
    assert all(torch.equal(a.view(torch.int32), b.view(torch.int32)) for a, b in zip(sparse, dense))


def test_sparse_fields_and_pyramids_are_refused(rays):
    from mipnerf_pl_amd import preview
    rows = tf.scene_rows(1, hollow=True)
    baked = _baked(rows, 1, tf.occupancy_of(rows))
    o, d, tn, tf_ = [_dev(a) for a in rays]
    G = torch.zeros(pf.N_RAYS, 3, device=DEV)
    for thing, name in ((baked.to_sparse(), "SparseField"), (preview.BakedPyramid([baked]), "BakedPyramid")):
        with pytest.raises(NotImplementedError, match=f"{name} is not a tuning target"):
            preview.march_grad(thing, o, d, tn, tf_, WHITE, grad_rgb=G)
        with pytest.raises(NotImplementedError, match=f"{name} is not a tuning target"):
            preview.TuneState(thing)


def test_preallocated_outputs_are_checked_before_the_launch(rays):
    """`out=(rgb, acc)` of another size, dtype or layout is refused like every other tensor argument: the kernel writes B rays into it"""
    from mipnerf_pl_amd import preview
    baked = _baked(tf.scene_rows(1), 1)
    o, d, tn, tf_ = [_dev(a) for a in rays]
    B = pf.N_RAYS
    G = torch.zeros(B, 3, device=DEV)
    good = (torch.empty(B, 3, device=DEV), torch.empty(B, device=DEV))
    for bad, which in (((torch.empty(B - 1, 3, device=DEV), good[1]), "rgb"), ((good[0], torch.empty(B - 1, device=DEV)), "acc"),
                       ((torch.empty(B, 3, device=DEV, dtype=torch.float16), good[1]), "rgb"), ((good[0], torch.empty(B)), "acc"),
                       ((torch.empty(3, B, device=DEV).t(), good[1]), "rgb")):
        with pytest.raises(ValueError, match=rf"march_grad: out\[[01]\] \({which}\) must be a contiguous fp32 tensor"):
            preview.march_grad(baked, o, d, tn, tf_, WHITE, grad_rgb=G, out=bad)
    _, rgb, acc = preview.march_grad(baked, o, d, tn, tf_, WHITE, grad_rgb=G, out=good)
    assert rgb is good[0] and acc is good[1]


def test_path_pixels_are_the_frames_own_rays():
    """`PathPixels.rays_at` (through `RenderGen.pixel_rays`) gives the rays `path[i]` gives for the same pixels, frame subset included"""
    from mipnerf_pl_amd import preview
    from mipnerf_pl_amd.datasets import RenderGen
    path = RenderGen(20.0, [6, 5], scales=1, device=torch.device(DEV), n_poses=4)
    src = preview.PathPixels(path, frames=[1, 3])
    assert src.num_pixels == 2 * 30
    ids = torch.tensor([0, 29, 30, 47, 59], device=DEV)
    got, pixels = src.rays_at(ids)
    assert pixels is None
    for k, (frame, pix) in enumerate(((1, 0), (1, 29), (3, 0), (3, 17), (3, 29))):
        want = path[frame]
        for g, w in zip(got, want):
            assert torch.equal(g[k], w.reshape(30, -1)[pix])


def test_the_command_end_to_end(tmp_path, capsys):
    """`--tune 3 --tune_batch 512` on the tiny checkpoint of test_gpu_preview.py's command test prints the tuned line and writes frames;
    the same command without --tune prints what it printed before; --tune --sparse saves a sparse lattice; --data --compare adds its line"""
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
    plain = r"preview: lattice 24 x 24 x 24, degree 1, baked share [0-9.]+, [0-9.]+ MiB, baked in [0-9.]+ ms, mean [0-9.]+ ms per frame \(2 frames\)"
    tuned = r"preview: tuned 3 steps of 512 rays against the (photos|MLP) in [0-9.]+ s \([0-9.]+ ms per step\), batch loss [0-9.e+-]+ -> [0-9.e+-]+"

    def lines():
        return [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("preview:")]

    folder = preview.main(common + ["--out_dir", str(tmp_path / "a")])
    out = lines()
    assert len(out) == 1 and re.fullmatch(plain, out[0]), out
    folder = preview.main(common + ["--out_dir", str(tmp_path / "b"), "--tune", "3", "--tune_batch", "512", "--save_baked"])
    out = lines()
    assert len(out) == 3 and re.fullmatch(tuned, out[0]) and " MLP " in out[0] and "lattice saved to" in out[1] and re.fullmatch(plain, out[2]), out
    pngs = sorted(f for f in os.listdir(os.path.join(folder, "1")) if f.endswith(".png") and f[:5].isdigit())
    assert pngs == sorted(f"{i:05d}_{t}.png" for i in range(2) for t in ("rgb", "dist", "acc"))
    saved = preview.BakedField.load(os.path.join(folder, "baked.npz"), DEV)
    untuned = preview.BakedField.load(os.path.join(preview.main(common + ["--out_dir", str(tmp_path / "c"), "--save_baked"]), "baked.npz"), DEV)
    lines()
    assert saved.dims == untuned.dims and not torch.equal(saved.rows, untuned.rows)                     # the tuned lattice is what is saved
    assert torch.equal(saved.occupancy.bits.view(torch.int32), untuned.occupancy.bits.view(torch.int32))
    # --tune --sparse: baked dense, tuned, then made sparse; with --data the photos are the default target and --compare gains a line
    data = write_blender(str(tmp_path / "data"), seed=6, counts=(("train", 2), ("test", 2)), w=16, h=16)
    folder = preview.main(common + ["--out_dir", str(tmp_path / "d"), "--tune", "3", "--tune_batch", "512", "--sparse", "--save_baked", "--data", data,
                                    "--compare", "--tune_lr_sigma", "0.1", "--tune_lr_colour", "0.005", "--tune_seed", "2"])
    out = lines()
    assert re.fullmatch(tuned, out[0]) and " photos " in out[0], out
    assert preview.BakedPyramid.stored_sparse(os.path.join(folder, "baked.npz"))
    assert any(re.fullmatch(r"preview: tuning moved the mean PSNR over 2 test images: vs photos [0-9.]+ -> [0-9.]+, vs MLP [0-9.]+ -> [0-9.]+", ln)
               for ln in out), out
    assert any(ln.startswith("preview: mean PSNR over 2 test images: baked vs photos") for ln in out) and "stored share" in " ".join(out)
