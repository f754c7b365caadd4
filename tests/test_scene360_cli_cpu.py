"""CPU (no GPU): the command-line side of captured, unbounded scenes (`--dataset_name llff | realdata360`): the configuration preset,
the interpolated render path against the reference's (tests/golden/render_path_llff.npz, scripts/make_golden_path.py), the host side of
the loader's images/ fallback, the stated rule of the device box shrink and its C ABI."""
import argparse
import os
import re

import numpy as np
import pytest
import torch

from mipnerf_pl_amd import config as cfg
from mipnerf_pl_amd import datasets as D
from mipnerf_pl_amd import train as T
from tests import dataset_fixture as fx
from tests import scene360_fixture as sf

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRESET = {"nerf.unbounded": True, "train.white_bkgd": False, "val.white_bkgd": False, "exp_name": "scene360"}


# ---- parser / configuration ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["llff", "realdata360"])
def test_scene360_command_line_resolves_to_the_preset(name):
    a = T.build_parser().parse_args(["--data_path", "d", "--out_dir", "o", "--dataset_name", name, "--factor", "2"])
    hp = cfg.resolve(a)
    want = dict(cfg.DEFAULTS, **PRESET)
    for k, v in want.items():
        assert hp[k] == v and type(hp[k]) is type(v), k
    assert hp["factor"] == 2 and hp["dataset_name"] == name and hp["data_path"] == "d"
    assert set(hp) == set(want) | set(vars(a))
    assert cfg.SCENE360_PRESET == PRESET and cfg.SCENE360_DATASETS == ("llff", "realdata360")
    assert T.build_parser().parse_args(["--data_path", "d", "--out_dir", "o", "--dataset_name", name]).factor == 4


def test_config_file_and_trailing_pairs_override_the_preset(tmp_path):
    p = tmp_path / "c.yaml"
    p.write_text("exp_name: garden\ntrain:\n  white_bkgd: True\nnerf:\n  num_samples: 96\n")
    a = T.build_parser().parse_args(["--data_path", "d", "--out_dir", "o", "--dataset_name", "llff", "--config", str(p),
                                     "val.white_bkgd", "True", "nerf.unbounded", "False"])
    hp = cfg.resolve(a)
    assert hp["exp_name"] == "garden" and hp["train.white_bkgd"] is True and hp["nerf.num_samples"] == 96      # file over preset
    assert hp["val.white_bkgd"] is True and hp["nerf.unbounded"] is False                                      # pairs over preset
    a = T.build_parser().parse_args(["--data_path", "d", "--out_dir", "o", "--dataset_name", "llff", "--config", str(p)])
    hp = cfg.resolve(a)
    assert hp["val.white_bkgd"] is False and hp["nerf.unbounded"] is True                                      # the rest of the preset stays


@pytest.mark.parametrize("name", ["blender", "multi_blender"])
def test_blender_command_lines_resolve_as_before_plus_factor(name):
    a = T.build_parser().parse_args(["--data_path", "d", "--out_dir", "o", "--dataset_name", name, "train.batch_size", "64"])
    before = dict(cfg.DEFAULTS, **{"train.batch_size": 64}, data_path="d", out_dir="o", dataset_name=name, config=None, precision="bf16",
                  use_graph=True, log_every_n_steps=50, child_timeout=30 * 86400.0, opts=["train.batch_size", "64"])
    assert cfg.resolve(a) == dict(before, factor=4)
    assert "nerf.unbounded" not in cfg.resolve(a)
    assert cfg.resolve(argparse.Namespace(config=None, opts=[])) == cfg.DEFAULTS | {"config": None, "opts": []}


def test_eval_and_render_video_flags():
    from mipnerf_pl_amd import eval as E
    from mipnerf_pl_amd import render_video as RV
    a = RV.build_parser().parse_args(["--ckpt", "c", "--out_dir", "o", "--scale", "1"])
    assert (a.path, a.data, a.split, a.n_views, a.factor) == (None, None, "test", 30, None)
    a = RV.build_parser().parse_args(["--ckpt", "c", "--out_dir", "o", "--scale", "1", "--path", "interp", "--data", "d", "--split", "train",
                                      "--n_views", "6", "--factor", "2"])
    assert (a.path, a.data, a.split, a.n_views, a.factor) == ("interp", "d", "train", 6, 2)
    assert E.build_parser().parse_args(["--out_dir", "o", "--scale", "1", "--factor", "8"]).factor == 8
    assert RV.flag_given(["--white_bkgd", "False"], "--white_bkgd") and RV.flag_given(["--white_bkgd=1"], "--white_bkgd")
    assert not RV.flag_given(["--white", "x"], "--white_bkgd")
    assert RV.is_scene360({"dataset_name": "llff"}) and RV.is_scene360({"dataset_name": "realdata360"})
    assert not RV.is_scene360({"dataset_name": "blender"}) and not RV.is_scene360({})


# ---- the interpolated path against the reference ------------------------------------------------------------------------------
def test_render_path_equals_the_reference(tmp_path):
    g = np.load(os.path.join(REPO, "tests", "golden", "render_path_llff.npz"))
    root = fx.write_llff(str(tmp_path / "llff"))
    for split, n in (("train", 8), ("test", 2)):
        poses = np.asarray(D.load_realdata360(root, split, True, 4)[2]["camtoworlds"], np.float64)
        assert poses.shape == (n, 3, 4) and np.array_equal(poses, g[f"{split}_poses"])       # the golden was made from these poses
        want = g[f"{split}_path"]
        got = D.gen_render_path(poses, 30)
        assert got.dtype == np.float64 and got.shape == want.shape == (n * 10, 4, 4)
        # float64, entries <= ~12, a dozen trig / multiply steps: round-off ~1e-15; 1e-9 separates same formula from another formula
        assert np.abs(got - want).max() <= 1e-9
        # the comparison means something only clear of gimbal lock (middle Euler angle +-90 degrees)
        euler = np.stack([D._matrix_to_euler_xyz(m[:3, :3]) for m in poses])
        assert np.abs(euler[:, 1]).max() < 80.0 and np.abs(g[f"{split}_euler"][:, 1]).max() < 80.0
        assert np.abs(euler - g[f"{split}_euler"]).max() <= 1e-9
        # every segment starts on its pose: the position as is, the rotation projected onto the nearest orthogonal matrix (the loader's
        # poses come from float32 files, orthonormal to a few float32 ulps of 1: 6e-8 each, so 1e-6 bounds the projection's move)
        assert np.abs(got[::10, :3, 3] - poses[:, :, 3]).max() <= 1e-12 and np.abs(got[::10, :3, :3] - poses[:, :, :3]).max() <= 1e-6
        assert D.gen_render_path(poses, 6).shape == (n * 2, 4, 4)


def test_euler_round_trip_and_the_first_pose_unwrap():
    rng = np.random.RandomState(0)
    for _ in range(20):
        e = rng.uniform([-180, -80, -180], [180, 80, 180])
        assert np.abs(D._matrix_to_euler_xyz(D._euler_xyz_to_matrix(e)) - e).max() <= 1e-9
    # an angle more than 180 degrees from the FIRST pose's gets + 360 whatever the sign, exactly as upstream writes it
    poses = np.tile(np.eye(4), (2, 1, 1))
    poses[0, :3, :3], poses[1, :3, :3] = D._euler_xyz_to_matrix([0, 0, -170.0]), D._euler_xyz_to_matrix([0, 0, 170.0])
    z = D._matrix_to_euler_xyz(D.gen_render_path(poses, 9)[1, :3, :3])[2]
    assert abs(z - (2 * -170.0 + (170.0 + 360.0)) / 3) < 1e-9            # -170 -> 530: the long way round, 63.33 degrees
    poses = poses[::-1].copy()
    z = D._matrix_to_euler_xyz(D.gen_render_path(poses, 9)[1, :3, :3])[2]
    assert abs(z - (2 * 170.0 + (-170.0 + 360.0)) / 3) < 1e-9            # 170 -> 190: the short way, 176.67 degrees


# ---- loader, host side ----------------------------------------------------------------------------------------------------------
def test_loader_errors_are_the_old_ones(tmp_path):
    root = fx.write_llff(str(tmp_path / "llff"))
    with pytest.raises(ValueError, match=r"RealData360 needs factor > 0"):
        D.load_realdata360(root, "train", True, 0)
    with pytest.raises(ValueError, match=r"RealData360 needs factor > 0"):
        D.load_realdata360(root, "train", True, -2)
    missing = os.path.join(root, "images_2")
    with pytest.raises(ValueError, match=re.escape(f"Image folder {missing} does not exist.")):
        D.load_realdata360(root, "train", True, 2)              # neither images_2/ nor images/
    os.remove(os.path.join(root, "images_4", "img_009.png"))
    with pytest.raises(RuntimeError, match=r"Mismatch between imgs 9 and poses 10"):
        D.load_realdata360(root, "train", True, 4)


def test_fallback_chooses_the_split_by_sorted_file_name_before_decoding(tmp_path, monkeypatch):
    root = fx.write_llff(str(tmp_path / "llff"))
    os.rename(os.path.join(root, "images_4"), os.path.join(root, "images"))
    names = sorted(os.listdir(os.path.join(root, "images")))
    # written in another order than sorted: rename so that creation order and name order differ
    for k, old in enumerate(names):
        os.rename(os.path.join(root, "images", old), os.path.join(root, "images", f"{(7 * k) % 10:02d}_{old}"))
    names = sorted(os.listdir(os.path.join(root, "images")))
    test_files, n, shrink = D.realdata360_files(root, "test", 2)
    train_files, n2, _ = D.realdata360_files(root, "train", 2)
    assert shrink and n == n2 == 10
    assert [os.path.basename(f) for f in test_files] == [names[0], names[8]]
    assert [os.path.basename(f) for f in train_files] == [names[i] for i in (1, 2, 3, 4, 5, 6, 7, 9)]
    assert D.realdata360_files(fx.write_llff(str(tmp_path / "b")), "test", 4)[2] is False          # images_4/ exists: nothing changes
    seen = {}

    def fake_shrink(files, factor, device):
        seen.update(files=list(files), factor=factor)
        return torch.zeros(len(files), 9 // factor, 14 // factor, 3)
    monkeypatch.setattr(D, "_shrink_on_device", fake_shrink)
    pixels, records, info = D.load_realdata360(root, "test", True, 2)
    assert seen == {"files": test_files, "factor": 2}                    # only the split's files are decoded
    assert pixels.shape == (2 * 4 * 7, 3) and len(records) == 2 and info["sizes"] == [(4, 7), (4, 7)] and (info["h"], info["w"]) == (4, 7)
    K = D.read_colmap_pinhole(os.path.join(root, "sparse", "0", "cameras.bin"))
    assert np.array_equal(info["K"][:2], K[:2] / 2) and float(records[0][21]) == 7.0 and float(records[0][22]) == 4.0
    os.remove(test_files[0])
    with pytest.raises(RuntimeError, match=r"Mismatch between imgs 9 and poses 10"):       # the count check counts ALL files
        D.load_realdata360(root, "train", True, 2)


def test_fallback_without_a_device_raises(tmp_path):
    root = fx.write_llff(str(tmp_path / "llff"))
    os.rename(os.path.join(root, "images_4"), os.path.join(root, "images"))
    with pytest.raises(RuntimeError, match="no host fallback"):
        D.load_realdata360(root, "train", True, 2, device=None)


# ---- the box-shrink rule and its entry point ------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [1, 2, 3, 4, 8, 16])
def test_integer_rule_is_the_mean_rounded_half_up(F):
    rng = np.random.RandomState(F)
    src = rng.randint(0, 256, size=(2, 37, 53, 4)).astype(np.uint8)
    q, rows = sf.rule_area_downscale(src, F)
    h, w = 37 // F, 53 // F
    mean = src[:, :h * F, :w * F, :3].astype(np.float64).reshape(2, h, F, w, F, 3).mean(axis=(2, 4))
    assert q.shape == (2, h, w, 3) and np.array_equal(q, np.floor(mean + 0.5).astype(np.uint8))
    assert rows.dtype == np.float32 and np.array_equal(np.round(rows * 255).astype(np.uint8), q)
    if F == 1:
        assert np.array_equal(q, src[..., :3])


def test_area_downscale_is_declared_exported_and_validates():
    from mipnerf_pl_amd import _lib as L
    from mipnerf_pl_amd import build, ops
    if not os.path.exists(L.LIB_PATH):
        build.build(verbose=False)
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "mipnerf_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+mipnerf_area_downscale\s*\(", hdr) and re.search(r"#define\s+MIPNERF_MAX_DOWNSCALE_FACTOR\s+16\b", hdr)
    assert len(L.SIGNATURES["mipnerf_area_downscale"][1]) == 9 and L.MAX_DOWNSCALE_FACTOR == 16
    assert ("kernels_downscale.hip", ["-ffp-contract=off"]) in build.UNITS
    lib = L.lib()
    assert lib.mipnerf_abi_version() == 6
    # argument validation happens before any HIP call
    for n, H, W, C, F, src, out, off in ((1, 8, 8, 3, 0, 16, 16, 0), (1, 8, 8, 3, 17, 16, 16, 0), (1, 8, 8, 2, 2, 16, 16, 0), (0, 8, 8, 3, 2, 16, 16, 0),
                                         (1, 1, 8, 3, 2, 16, 16, 0), (1, 8, 8, 3, 2, None, 16, 0), (1, 8, 8, 3, 2, 16, None, 0),
                                         (1, 8, 8, 3, 2, 16, 16, -1), (1, 8, 8, 3, 2, 24, 16, 0)):
        assert lib.mipnerf_area_downscale(n, H, W, C, F, src, out, off, None) == L.E_INVALID, (n, H, W, C, F, src, out, off)
        assert b"area_downscale" in lib.mipnerf_last_error()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.area_downscale(torch.zeros(1, 4, 4, 3, dtype=torch.uint8), 2)
