"""Distorted COLMAP camera models, the parts that need no GPU: the readers of cameras.bin / images.bin, `ops.camera_record`, the
load-time round-trip check, the loader's per-image records and refusals, `PathGen`'s pinhole records, the all-pixel cull defaults on host
tensors, and csrc/camera_models.hpp run on the CPU under AddressSanitizer / UBSan against the float64 restatement
(camera_models_fixture.py)."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import camera_models_fixture as cm
import dataset_fixture as dsf
from mipnerf_pl_amd import _lib, datasets, ops
from mipnerf_pl_amd.rays import Rays

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
SIX = ("SIMPLE_PINHOLE", "PINHOLE", "SIMPLE_RADIAL", "RADIAL", "OPENCV", "OPENCV_FISHEYE")


def _params(name):
    return cm.colmap_params(name, (-0.15, 0.04, 1e-3, -2e-3))


# ---- readers ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SIX)
def test_read_colmap_cameras_every_model(tmp_path, name):
    fname = str(tmp_path / "sparse" / "0" / "cameras.bin")
    cm.write_cameras_bin(fname, [(7, name, 640, 480, _params(name))])
    assert datasets.read_colmap_cameras(fname) == [(7, name, 640, 480, tuple(_params(name)))]
    K, model, coeffs = datasets.colmap_intrinsics(name, _params(name))
    want_K = cm.K.copy()
    if name in ("SIMPLE_PINHOLE", "SIMPLE_RADIAL", "RADIAL"):                       # one focal length
        want_K[1, 1] = want_K[0, 0]
    assert np.array_equal(K, want_K)
    want = {"SIMPLE_PINHOLE": ("pinhole", (0, 0, 0, 0)), "PINHOLE": ("pinhole", (0, 0, 0, 0)), "SIMPLE_RADIAL": ("radial", (-0.15, 0, 0, 0)),
            "RADIAL": ("radial", (-0.15, 0.04, 0, 0)), "OPENCV": ("radial", (-0.15, 0.04, 1e-3, -2e-3)),
            "OPENCV_FISHEYE": ("fisheye", (-0.15, 0.04, 1e-3, -2e-3))}[name]
    assert (model, tuple(coeffs)) == want


def test_read_colmap_cameras_two_models_in_one_file(tmp_path):
    fname = str(tmp_path / "cameras.bin")
    a, b = cm.colmap_params("SIMPLE_RADIAL", (-0.12, 0, 0, 0)), cm.colmap_params("OPENCV_FISHEYE", (0.05, -0.01, 0.002, 0.0))
    cm.write_cameras_bin(fname, [(3, "SIMPLE_RADIAL", 37, 29, a), (9, "OPENCV_FISHEYE", 37, 29, b)])
    assert datasets.read_colmap_cameras(fname) == [(3, "SIMPLE_RADIAL", 37, 29, tuple(a)), (9, "OPENCV_FISHEYE", 37, 29, tuple(b))]


@pytest.mark.parametrize("name,count", [("FULL_OPENCV", 12), ("FOV", 5), ("THIN_PRISM_FISHEYE", 12)])
def test_read_colmap_cameras_refuses_other_models_by_name(tmp_path, name, count):
    fname = str(tmp_path / "cameras.bin")
    cm.write_cameras_bin(fname, [(1, "PINHOLE", 64, 48, _params("PINHOLE")), (2, name, 64, 48, (1.0,) * count)])
    with pytest.raises(NotImplementedError, match=name):
        datasets.read_colmap_cameras(fname)


def test_pinhole_K_is_read_colmap_pinhole(tmp_path):
    root = dsf.write_llff(str(tmp_path / "llff"))
    fname = os.path.join(root, "sparse", "0", "cameras.bin")
    (cam,) = datasets.read_colmap_cameras(fname)
    K, model, coeffs = datasets.colmap_intrinsics(cam[1], cam[4])
    assert cam[1] == "PINHOLE" and model == "pinhole"
    assert K.tobytes() == datasets.read_colmap_pinhole(fname).tobytes()


def test_read_colmap_image_cameras(tmp_path):
    fname = str(tmp_path / "sparse" / "0" / "images.bin")
    cm.write_images_bin(fname, [(1, 4, "b.png"), (2, 9, "a with space.JPG"), (3, 4, "c.png")], points=5)
    assert datasets.read_colmap_image_cameras(fname) == {"b.png": 4, "a with space.JPG": 9, "c.png": 4}


# ---- camera_record ---------------------------------------------------------------------------------------------------------------------
def test_camera_record_layout():
    assert _lib.num_camera_modes() == 4
    pose, p2c = cm.c2w(), cm.pix2cam()
    for dtype in (torch.float32, torch.float64):
        base = ops.camera_record(pose, cm.W, cm.H, 0.5, 7.0, pix2cam=p2c, dtype=dtype)
        for model, mode in (("radial", 2.0), ("fisheye", 3.0)):
            rec = ops.camera_record(pose, cm.W, cm.H, 0.5, 7.0, pix2cam=p2c, dtype=dtype, model=model, distortion=(-0.3, 0.1, 2e-3, 1e-3))
            assert rec.shape == (32,) and rec.dtype == dtype
            assert float(rec[26]) == mode
            assert torch.equal(rec[28:32], torch.tensor([-0.3, 0.1, 2e-3, 1e-3], dtype=dtype))
            assert torch.equal(rec[:26], base[:26]) and float(rec[27]) == 0.0
        assert float(ops.camera_record(pose, 3, 2, 1, 2, pix2cam=p2c, model="radial")[28:32].abs().sum()) == 0.0


def test_camera_record_default_is_unchanged():
    pose, p2c = cm.c2w(), cm.pix2cam()
    for dtype in (torch.float32, torch.float64):
        old = torch.zeros(32, dtype=dtype)                               # the record as it was before the models existed
        old[0:12] = torch.as_tensor(pose, dtype=dtype).reshape(-1)
        old[12:21] = torch.as_tensor(p2c, dtype=dtype).reshape(-1)
        old[21], old[22], old[23], old[24], old[25], old[26] = float(cm.W), float(cm.H), 0.5, 7.0, 1.0, 1.0
        assert torch.equal(ops.camera_record(pose, cm.W, cm.H, 0.5, 7.0, pix2cam=p2c, dtype=dtype), old)
        assert torch.equal(ops.camera_record(pose, cm.W, cm.H, 0.5, 7.0, pix2cam=p2c, dtype=dtype, model="pinhole", distortion=(0, 0, 0, 0)), old)
    blender = ops.camera_record(pose, 8, 6, 2.0, 6.0, focal=11.0)
    assert float(blender[26]) == 0.0 and float(blender[27]) == 11.0 and float(blender[28:32].abs().sum()) == 0.0


def test_camera_record_errors():
    pose, p2c = cm.c2w(), cm.pix2cam()
    with pytest.raises(ValueError, match="pix2cam"):
        ops.camera_record(pose, 8, 6, 2, 6, focal=11.0, model="radial", distortion=(0.1, 0, 0, 0))
    with pytest.raises(ValueError, match="pix2cam"):
        ops.camera_record(pose, 8, 6, 2, 6, focal=11.0, distortion=(0.1, 0, 0, 0))
    with pytest.raises(ValueError, match="4 coefficients"):
        ops.camera_record(pose, 8, 6, 2, 6, pix2cam=p2c, model="radial", distortion=(0.1, 0.2))
    with pytest.raises(ValueError, match="4 coefficients"):
        ops.camera_record(pose, 8, 6, 2, 6, pix2cam=p2c, model="fisheye", distortion=(0.1, 0.2, 0.3, 0.4, 0.5))
    with pytest.raises(ValueError, match=r"last row"):
        ops.camera_record(pose, 8, 6, 2, 6, pix2cam=np.linalg.inv(cm.K), model="radial", distortion=(0.1, 0, 0, 0))   # rows not negated
    with pytest.raises(ValueError, match="model"):
        ops.camera_record(pose, 8, 6, 2, 6, pix2cam=p2c, model="fov", distortion=(0.1, 0, 0, 0))
    with pytest.raises(ValueError, match="pinhole"):
        ops.camera_record(pose, 8, 6, 2, 6, pix2cam=p2c, distortion=(0.1, 0, 0, 0))


def test_c_header_declares_the_entry_point():
    text = open(os.path.join(REPO, "include", "mipnerf_hip.h")).read()
    assert "int mipnerf_num_camera_modes(void);" in text and "#define MIPNERF_CAMERA_FLOATS 32" in text
    assert "mipnerf_num_camera_modes" in _lib.SIGNATURES


# ---- load-time round trip --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(len(cm.PARAM_SETS)), ids=cm.PARAM_IDS)
def test_round_trip_accepts_the_test_sets(case):
    name, model, coeffs = cm.PARAM_SETS[case]
    assert datasets.round_trip_error(model, coeffs, cm.K, cm.W, cm.H) <= 1e-6
    datasets.check_invertible(1, name, model, coeffs, cm.K, cm.W, cm.H)
    # the host solve is the restatement's: same undistorted points at every pixel
    xd, yd = cm.normalised_points(extra_row=False)
    if model == "radial":
        xu, yu = datasets.undistort_points(model, coeffs, xd, yd)
        rx, ry = cm.undistort_radial(coeffs, xd, yd)
        assert np.abs(xu - rx).max() <= 1e-14 and np.abs(yu - ry).max() <= 1e-14
        bx, by = datasets.distort_points(model, coeffs, rx, ry)
        assert np.abs(bx - xd).max() <= 1e-14 and np.abs(by - yd).max() <= 1e-14
    else:
        th, thd = datasets.undistort_points(model, coeffs, xd, yd)
        assert np.abs(th - cm.undistort_fisheye(coeffs, thd)).max() <= 1e-14
        bx, by = datasets.distort_points(model, coeffs, np.tan(th) * xd / thd, np.tan(th) * yd / thd)
        assert np.abs(bx - xd).max() <= 1e-14 and np.abs(by - yd).max() <= 1e-14


def test_round_trip_refuses_a_strong_barrel(tmp_path):
    name, model, coeffs = cm.STRONG_BARREL
    assert not datasets.round_trip_error(model, coeffs, cm.K, cm.W, cm.H) <= 1e-6
    with pytest.raises(ValueError, match=r"camera 5 \(SIMPLE_RADIAL.*undistort the capture with COLMAP"):
        datasets.check_invertible(5, name, model, coeffs, cm.K, cm.W, cm.H)
    root = str(tmp_path / "barrel")
    cm.write_capture(root, [(5, name, cm.W, cm.H, cm.colmap_params(name, coeffs))], w=cm.W, h=cm.H, folder="images_1")
    with pytest.raises(ValueError, match="camera 5.*undistort the capture with COLMAP"):
        datasets.load_realdata360(root, "train", factor=1)


# ---- the loader ------------------------------------------------------------------------------------------------------------------------
def test_pinhole_capture_loads_as_before(tmp_path):
    root = dsf.write_llff(str(tmp_path / "llff"))
    for split in ("train", "test"):
        images, records, info = datasets.load_realdata360(root, split, factor=4)
        K = datasets.read_colmap_pinhole(os.path.join(root, "sparse", "0", "cameras.bin"))
        K[:2, :] /= 4
        K_inv = np.linalg.inv(K)
        K_inv[1:, :] *= -1
        assert info["K"].tobytes() == K.tobytes() and info["K_inv"].tobytes() == K_inv.tobytes()
        h, w = info["h"], info["w"]
        for rec, pose, bd in zip(records, info["camtoworlds"], info["bds"]):
            assert torch.equal(rec, ops.camera_record(pose, w, h, float(bd[0]), float(bd[1]), pix2cam=K_inv))
        assert info["models"] == ["PINHOLE"] * len(records) and not info["distortion"].any()
        assert info["Ks"].shape == (len(records), 3, 3) and all(k.tobytes() == K.tobytes() for k in info["Ks"])


def test_distorted_capture_records(tmp_path):
    root = str(tmp_path / "radial")
    cam = (1, "SIMPLE_RADIAL", 32, 24, (40.0, 16.3, 11.8, -0.12))
    cm.write_capture(root, [cam], w=16, h=12, folder="images_2")
    images, records, info = datasets.load_realdata360(root, "train", factor=2)
    assert len(records) == 7 and info["models"] == ["SIMPLE_RADIAL"] * 7
    K = np.array([[20.0, 0, 8.15], [0, 20.0, 5.9], [0, 0, 1]])                    # divided by the factor; k1 is not
    assert np.allclose(info["K"], K, rtol=0, atol=1e-15) and np.array_equal(info["distortion"], np.tile([-0.12, 0, 0, 0], (7, 1)))
    for rec in records:
        assert float(rec[26]) == 2.0 and torch.equal(rec[28:32], torch.tensor([-0.12, 0, 0, 0], dtype=torch.float32))
        assert rec[18:21].tolist() == [0.0, 0.0, -1.0]
    ds = datasets.RealData360(root, "test", batch_type="single_image", factor=2, device=None)
    assert ds.models == ["SIMPLE_RADIAL"] * 2 and ds.Ks.shape == (2, 3, 3) and ds.distortion.shape == (2, 4)
    path = datasets.PathGen(ds, n_views=3)
    assert path.cameras.shape[1] == 32 and bool((path.cameras[:, 26] == 1.0).all()) and not bool(path.cameras[:, 27:32].any())


def _two_camera_capture(root, **kw):
    cams = [(3, "SIMPLE_RADIAL", 16, 12, (20.0, 8.2, 5.9, -0.12)), (8, "OPENCV_FISHEYE", 16, 12, (19.0, 19.5, 7.9, 6.1, 0.05, -0.01, 0.002, 0.0))]
    ids = [3, 8, 8, 3, 8, 3, 3, 8, 3]
    return cams, ids, cm.write_capture(root, cams, image_cameras=ids, folder="images_1", **kw)


def test_two_cameras_give_per_image_records(tmp_path):
    root = str(tmp_path / "two")
    cams, ids, _ = _two_camera_capture(root)
    for split, sel in (("train", [1, 2, 3, 4, 5, 6, 7]), ("test", [0, 8])):
        _, records, info = datasets.load_realdata360(root, split, factor=1)
        assert info["models"] == [{3: "SIMPLE_RADIAL", 8: "OPENCV_FISHEYE"}[ids[i]] for i in sel]
        for rec, K, i in zip(records, info["Ks"], sel):
            radial = ids[i] == 3
            assert float(rec[26]) == (2.0 if radial else 3.0)
            assert rec[28:32].tolist() == pytest.approx([-0.12, 0, 0, 0] if radial else [0.05, -0.01, 0.002, 0.0], rel=1e-7)
            assert K[0, 0] == (20.0 if radial else 19.0) and K[1, 2] == (5.9 if radial else 6.1)
            K_inv = np.linalg.inv(K)
            K_inv[1:, :] *= -1
            assert torch.equal(rec[12:21], torch.as_tensor(K_inv, dtype=torch.float32).reshape(-1))
        assert info["K"][0, 0] == 20.0                                              # K / K_inv stay the file's first camera's


def test_two_cameras_without_images_bin(tmp_path):
    root = str(tmp_path / "two")
    _two_camera_capture(root)
    os.remove(os.path.join(root, "sparse", "0", "images.bin"))
    with pytest.raises(FileNotFoundError, match=r"sparse.0.images\.bin"):
        datasets.load_realdata360(root, "train", factor=1)


def test_cameras_of_differing_sizes_are_refused(tmp_path):
    root = str(tmp_path / "sizes")
    cams = [(1, "PINHOLE", 16, 12, (20.0, 20.0, 8.0, 6.0)), (2, "PINHOLE", 32, 24, (40.0, 40.0, 16.0, 12.0))]
    cm.write_capture(root, cams, image_cameras=[1, 2] * 4 + [1], folder="images_1")
    with pytest.raises(ValueError, match="differ in image size.*16x12.*32x24"):
        datasets.load_realdata360(root, "train", factor=1)


def test_unknown_model_refuses_the_capture(tmp_path):
    root = str(tmp_path / "fov")
    cm.write_capture(root, [(1, "FOV", 16, 12, (20.0, 20.0, 8.0, 6.0, 0.9))], folder="images_1")
    with pytest.raises(NotImplementedError, match="FOV"):
        datasets.load_realdata360(root, "train", factor=1)


# ---- cull defaults on host tensors -----------------------------------------------------------------------------------------------------
def _frame(model, coeffs):
    r = cm.rays(model, coeffs)
    o = np.broadcast_to(cm.c2w()[:, 3], r["directions"].shape)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32))                 # noqa: E731
    one = np.ones((cm.H, cm.W, 1))
    return Rays(t(o), t(r["directions"]), t(r["viewdirs"]), t(r["radii"][..., None]), t(one), t(cm.NEAR * one), t(cm.FAR * one))


def test_cull_defaults_cover_every_pixel_of_a_distorted_frame():
    from mipnerf_pl_amd.evaluate import corner_ray_bound, corner_ray_radius, cull_box, cull_far_radius
    frame = _frame("radial", (0.08, 0.0, 0.0, 0.0))               # pincushion: the far end points bulge between the corners' chords
    ends = [frame.origins.double() + t * frame.directions.double() for t in (cm.NEAR, cm.FAR)]
    every_bound = max(float(e.abs().max()) for e in ends)
    every_radius = max(float(e.norm(dim=-1).max()) for e in ends)
    pin = _frame("pinhole", (0, 0, 0, 0))
    for frames, flags in (([frame], True), ([frame], [True]), ([pin, frame], [False, True])):
        assert corner_ray_bound(frames, flags) >= every_bound * (1 - 1e-6)
        assert corner_ray_radius(frames, flags) >= every_radius * (1 - 1e-6)
    assert cull_box([frame], 32, True) == corner_ray_bound([frame], True) * 31 / 29
    assert cull_far_radius([frame], 32, True) == corner_ray_radius([frame], True) * 31 / 29
    # pinhole frames keep the corner rule and its values, flagged or not
    assert corner_ray_bound([pin], [False]) == corner_ray_bound([pin]) and corner_ray_radius([pin], False) == corner_ray_radius([pin])
    assert corner_ray_bound([pin, frame], [False, True]) >= corner_ray_bound([pin])


# ---- csrc/camera_models.hpp on the CPU, sanitised --------------------------------------------------------------------------------------
def test_header_on_the_cpu_under_sanitizers(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler")
    exe = str(tmp_path / "camera_models_host")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(HERE, "hostmath", "camera_models_host.cpp"), "-o", exe])
    xd, yd = cm.normalised_points(extra_row=True)                      # every pixel and the row the last radii reach for
    lines = [str(len(cm.PARAM_SETS))]
    for _, model, coeffs in cm.PARAM_SETS:
        c = cm.camera_directions(model, coeffs, xd, yd).reshape(-1, 3)
        lines.append("{} {!r} {!r} {!r} {!r} {}".format(2 if model == "radial" else 3, *[float(v) for v in coeffs], c.shape[0]))
        lines += ["{!r} {!r} {!r} {!r} {!r}".format(float(a), float(b), *[float(v) for v in row]) for a, b, row in zip(xd.ravel(), yd.ravel(), c)]
    points = tmp_path / "points.txt"
    points.write_text("\n".join(lines) + "\n")
    # float64: 8 steps reach the 60-step solution to 3e-16 (a few ulps of a number below 1.3); float32: the restatement in float32
    # numpy measures 2.5e-7 on the directions at this shape, and the camera-space points are the same size
    run = subprocess.run([exe, str(points), "1e-14", "1e-6"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    print(run.stdout)
    assert run.returncode == 0, run.stdout
    assert run.stdout.strip().endswith("ok") and run.stdout.count("set ") == len(cm.PARAM_SETS)
