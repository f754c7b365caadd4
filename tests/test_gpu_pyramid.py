"""The multi-scale converter on the device: ops.box_pyramid (kernels_pyramid.hip), the convert_blender_data command and
Multicam.from_blender against what the unmodified reference converter wrote and its Multicam class read back
(tests/golden/pyramid_48x40.npz) -- bytes and float32 pixels compared for equality, no tolerance; rays with the tolerance
tests/test_gpu_datasets.py uses for the Multicam train split."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import pyramid_fixture as pf  # noqa: E402
from gpu_util import record  # noqa: E402

pytestmark = pytest.mark.gpu
G = np.load(os.path.join(HERE, "golden", "pyramid_48x40.npz"))
DEV = "cuda:0"
RAY_TOL = 3e-6          # test_gpu_datasets.py::test_train_split_every_ray, the "multicam_train" row


@pytest.fixture(scope="module")
def roots(tmp_path_factory):
    return pf.write_roots(tmp_path_factory.mktemp("pyr"))


def golden_png(name, rel):
    files = list(G[f"{name}_files"])
    return G[f"{name}_png_{files.index(rel)}"]


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def check_against_rule(src, n_levels, white, rgb_row_offset=0):
    """ops.box_pyramid on `src` [n, H, W, 4] uint8 (numpy) equals the numpy rule: bytes and pixel rows, all levels."""
    from mipnerf_pl_amd import ops
    want = pf.rule_pyramid(src, n_levels)
    u8, rgb = ops.box_pyramid(torch.from_numpy(src).to(DEV), n_levels, white_bkgd=white, rgb_row_offset=rgb_row_offset)
    torch.cuda.synchronize()
    assert len(u8) == len(rgb) == n_levels
    for j in range(n_levels):
        assert int(np.count_nonzero(u8[j].cpu().numpy() != want[j])) == 0, (src.shape, n_levels, j)
    rows = torch.from_numpy(pf.rule_pixels(want, white))                                   # [n, PPI, 3]
    got = torch.cat([r.reshape(src.shape[0], -1, 3) for r in rgb], dim=1).cpu()
    assert same_bits(got, rows), (src.shape, n_levels, white)


@pytest.mark.parametrize("name", pf.ROOTS)
def test_fixture_frames_equal_the_reference_converter(roots, name):
    from mipnerf_pl_amd import ops
    for split in pf.SPLITS:
        frames = pf.read_frames(roots[name], split)
        for wb in ((1, 0) if name == "random" else (1,)):
            u8, rgb = ops.box_pyramid(torch.from_numpy(frames).to(DEV), pf.N_DOWN, white_bkgd=bool(wb))
            for i in range(frames.shape[0]):
                for j in range(pf.N_DOWN):
                    want = golden_png(name, f"images_{split}/{i:03d}_d{j}.png")
                    assert int(np.count_nonzero(u8[j][i].cpu().numpy() != want)) == 0, (name, split, i, j)
            if split == "train":
                got = torch.cat([r.reshape(frames.shape[0], -1, 3) for r in rgb], dim=1).reshape(-1, 3).cpu()
                assert same_bits(got, torch.from_numpy(G[f"{name}_pixels_wb{wb}"])), (name, wb)
    # without pixel rows: the same bytes, no float output
    u8b, none = ops.box_pyramid(torch.from_numpy(frames).to(DEV), pf.N_DOWN)
    assert none is None and all(torch.equal(a, b) for a, b in zip(u8, u8b))


def test_full_size_batch_and_tile_edges():
    rng = np.random.RandomState(11)
    big = rng.randint(0, 256, size=(3, 800, 800, 4)).astype(np.uint8)
    big[1, ..., 3] = np.where(rng.rand(800, 800) < 0.7, np.where(rng.rand(800, 800) < 0.5, 0, 255), big[1, ..., 3])
    big[2, :400] = 255                                                                      # constant regions: every level stays 255 / 0
    big[2, 400:, :, 3] = 0
    check_against_rule(big, 4, True)
    check_against_rule(big[:1], 4, False)
    check_against_rule(rng.randint(0, 256, size=(1, 8, 24, 4)).astype(np.uint8), 4, True)   # one row of three 8 x 8 blocks
    check_against_rule(rng.randint(0, 256, size=(1, 8, 24, 4)).astype(np.uint8), 1, True)
    check_against_rule(rng.randint(0, 256, size=(2, 5, 7, 4)).astype(np.uint8), 1, False)   # one level: any size
    check_against_rule(rng.randint(0, 256, size=(2, 6, 10, 4)).astype(np.uint8), 2, True)
    check_against_rule(rng.randint(0, 256, size=(2, 12, 20, 4)).astype(np.uint8), 3, True)
    check_against_rule(rng.randint(0, 256, size=(2, 40, 48, 4)).astype(np.uint8), 4, True, rgb_row_offset=1)      # rows off the 16-byte grid
    check_against_rule(rng.randint(0, 256, size=(2, 40, 48, 4)).astype(np.uint8), 4, True, rgb_row_offset=2)
    check_against_rule(rng.randint(0, 256, size=(2, 64, 96, 4)).astype(np.uint8), 6, True)                        # second pass over the scratch
    check_against_rule(rng.randint(0, 256, size=(1, 128, 256, 4)).astype(np.uint8), 8, False)


def test_rows_outside_the_batch_are_untouched():
    from mipnerf_pl_amd import ops
    rng = np.random.RandomState(12)
    src = torch.from_numpy(rng.randint(0, 256, size=(2, 16, 24, 4)).astype(np.uint8)).to(DEV)
    ppi = 16 * 24 + 8 * 12 + 4 * 6
    out = torch.full((5 + 2 * ppi + 7, 3), -3.0, device=DEV)
    ops.box_pyramid(src, 3, white_bkgd=True, out_rgb=out, rgb_row_offset=5)
    assert bool((out[:5] == -3.0).all()) and bool((out[5 + 2 * ppi:] == -3.0).all())
    assert bool(((out[5:5 + 2 * ppi] >= 0.0) & (out[5:5 + 2 * ppi] <= 1.0)).all())
    with pytest.raises(ValueError):
        ops.box_pyramid(src, 5)
    with pytest.raises(ValueError):
        ops.box_pyramid(src, 3, out_rgb=out, rgb_row_offset=13)


def test_command_line_on_the_fixture_directory(roots, tmp_path):
    for name in pf.ROOTS:
        out = tmp_path / name
        run = subprocess.run([sys.executable, "-m", "mipnerf_pl_amd.convert_blender_data", "--blender_dir", os.path.dirname(roots[name]),
                              "--out_dir", str(out), "--object_name", "scene", "--n_down", str(pf.N_DOWN), "--device", DEV, "--workers", "4"],
                             capture_output=True, text=True, timeout=300, cwd=REPO)
        assert run.returncode == 0, run.stdout[-3000:] + run.stderr[-3000:]
        new = str(out / "scene")
        files = sorted(os.path.relpath(os.path.join(d, f), new) for d, _, fs in os.walk(new) for f in fs)
        assert files == sorted(list(G[f"{name}_files"]) + ["metadata.json"])
        from PIL import Image
        for k, rel in enumerate(G[f"{name}_files"]):
            img = Image.open(os.path.join(new, rel))
            assert img.mode == "RGBA"
            assert np.array_equal(np.array(img), G[f"{name}_png_{k}"]), rel
        with open(os.path.join(new, "metadata.json")) as fp:
            got = json.load(fp)
        want = json.loads(str(G[f"{name}_metadata"]))
        assert got == want and all(list(got[s]) == list(want[s]) for s in want)
    # a size that does not halve: ValueError naming the file, nothing written
    import dataset_fixture as fx
    from mipnerf_pl_amd import convert_blender_data as conv
    bad = fx.write_blender(str(tmp_path / "bad" / "scene"), seed=1, w=12, h=10)
    with pytest.raises(ValueError, match=r"r_0\.png"):
        conv.convert_to_nerfdata(bad, str(tmp_path / "bad_out"), 3, device=DEV)
    assert not os.path.exists(str(tmp_path / "bad_out"))


@pytest.mark.parametrize("wb", [True, False])
def test_multicam_from_blender_equals_the_converted_directory(roots, tmp_path, wb):
    from mipnerf_pl_amd import convert_blender_data as conv
    from mipnerf_pl_amd import datasets as D
    conv.convert_to_nerfdata(roots["random"], str(tmp_path / "conv"), pf.N_DOWN, device=DEV, workers=4)
    ref = D.Multicam(str(tmp_path / "conv"), "train", white_bkgd=wb, batch_type="all_images", device=DEV)
    a = D.Multicam.from_blender(roots["random"], "train", white_bkgd=wb, batch_type="all_images", n_down=pf.N_DOWN, device=DEV)
    b = D.Multicam(roots["random"], "train", white_bkgd=wb, batch_type="all_images", device=DEV)         # no metadata.json: the fallback
    ids = torch.from_numpy(np.random.RandomState(3).randint(0, ref.num_pixels, size=1000)).to(DEV)
    r0, p0 = ref.rays_at(ids)
    for ds in (a, b):
        assert ds.blender and ds.images is None
        assert torch.equal(ds.cameras, ref.cameras) and ds.sizes == ref.sizes and np.array_equal(ds.offsets, ref.offsets)
        assert len(ds) == len(ref) == 3 * sum((pf.H >> j) * (pf.W >> j) for j in range(pf.N_DOWN))
        assert same_bits(ds._dev["pixels"], ref._dev["pixels"])
        r1, p1 = ds.rays_at(ids)
        assert same_bits(p1, p0) and all(same_bits(x, y) for x, y in zip(r1, r0))
    # ... and against the reference's own Multicam on the reference-converted directory
    assert same_bits(a._dev["pixels"].cpu(), torch.from_numpy(G[f"random_pixels_wb{int(wb)}"]))
    rays, _ = a[torch.arange(len(a))]
    worst = 0.0
    for k in rays._fields:
        got = getattr(rays, k).double().cpu().numpy()
        want = np.asarray(G[f"rays_{k}"], np.float64).reshape(got.shape)
        err = float(np.max(np.abs(got - want) / (1.0 + np.abs(want))))
        worst = max(worst, err)
        assert err <= RAY_TOL, (k, err)
    record("pyramid/from_blender_rays", max_rel_err=worst, tol=RAY_TOL)
    # image splits work the same way
    t = D.Multicam(roots["random"], "test", white_bkgd=wb, batch_type="single_image", device=DEV)
    tr = D.Multicam(str(tmp_path / "conv"), "test", white_bkgd=wb, batch_type="single_image", device=DEV)
    assert len(t) == len(tr) == 2 * pf.N_DOWN
    for i in (0, 3, 7):
        (ra, ia), (rb, ib) = t[i], tr[i]
        assert same_bits(ia, ib) and all(same_bits(x, y) for x, y in zip(ra, rb))


def test_system_sets_up_multi_blender_off_a_blender_directory(roots):
    from mipnerf_pl_amd.system import DEFAULT_HPARAMS, MipNeRFSystem
    hp = dict(DEFAULT_HPARAMS)
    hp.update({"dataset_name": "multi_blender", "data_path": roots["binary"], "train.batch_size": 48, "train.batch_type": "all_images",
               "val.batch_type": "single_image", "val.chunk_size": 64, "nerf.num_samples": 32})
    torch.manual_seed(0)
    system = MipNeRFSystem(hp).to(DEV)
    system.setup("fit")
    assert system.train_dataset.blender and len(system.train_dataset) == 3 * (40 * 48 + 20 * 24 + 10 * 12 + 5 * 6)
    rays, pix = next(iter(system.train_dataloader()))
    loss = system.training_step((rays, pix), 0)
    assert np.isfinite(float(loss.detach())) and set(rays.lossmult.unique().tolist()) <= {1.0, 4.0, 16.0, 64.0}


def test_train_and_eval_commands_off_a_blender_directory(roots, tmp_path):
    """`train --dataset_name multi_blender --data_path <Blender scene>` and `eval` on its checkpoint, no conversion step."""
    out = tmp_path / "out"

    def run(args, timeout):
        r = subprocess.run([sys.executable, "-m"] + args, capture_output=True, text=True, timeout=timeout, cwd=REPO)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    run(["mipnerf_pl_amd.train", "--data_path", roots["binary"], "--out_dir", str(out), "--dataset_name", "multi_blender",
         "--log_every_n_steps", "2", "exp_name", "ms", "train.batch_size", "256", "nerf.num_samples", "32", "optimizer.max_steps", "6",
         "optimizer.lr_delay_steps", "0", "val.check_interval", "1000", "val.sample_num", "1", "val.chunk_size", "4096"], 600)
    ck = out / "ckpt" / "ms" / "last.ckpt"
    assert ck.exists() and not os.path.exists(os.path.join(roots["binary"], "metadata.json"))
    run(["mipnerf_pl_amd.eval", "--ckpt", str(ck), "--data", roots["binary"], "--out_dir", str(out), "--scale", "1", "--chunk_size", "4096"], 300)
    psnrs = (out / "test" / "ms" / "psnrs.txt").read_text().split()
    assert len(psnrs) == 2 * pf.N_DOWN and all(np.isfinite(float(v)) for v in psnrs)


def test_capture_and_replay():
    from mipnerf_pl_amd import ops
    rng = np.random.RandomState(13)
    n, h, w, levels = 2, 40, 48, 4
    ppi = sum((h >> j) * (w >> j) for j in range(levels))
    src = torch.zeros(n, h, w, 4, dtype=torch.uint8, device=DEV)
    out_u8 = torch.zeros(4 * n * ppi, dtype=torch.uint8, device=DEV)
    out_rgb = torch.zeros(n * ppi, 3, device=DEV)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.box_pyramid(src, levels, white_bkgd=True, out_u8=out_u8, out_rgb=out_rgb)      # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        ops.box_pyramid(src, levels, white_bkgd=True, out_u8=out_u8, out_rgb=out_rgb)
    for _ in range(2):
        fresh = torch.from_numpy(rng.randint(0, 256, size=(n, h, w, 4)).astype(np.uint8)).to(DEV)
        src.copy_(fresh)
        graph.replay()
        torch.cuda.synchronize()
        eager_u8, eager_rgb = ops.box_pyramid(fresh, levels, white_bkgd=True)
        assert torch.equal(out_u8, torch.cat([e.reshape(-1) for e in eager_u8]))
        got = out_rgb.reshape(n, ppi, 3)
        assert same_bits(got, torch.cat([r.reshape(n, -1, 3) for r in eager_rgb], dim=1))
        want = pf.rule_pyramid(fresh.cpu().numpy(), levels)
        assert all(np.array_equal(e.cpu().numpy(), wj) for e, wj in zip(eager_u8, want))
