"""GPU: rendered depth fused into a truncated signed distance volume (libmipnerf_fuse.so) -- k_fuse_integrate and k_fuse_finalise bit for bit
against the float32 restatement of tests/fuse_fixture.py, k_depth_quantile by the bracket test against the float64 restatement, the
projection rows against the rays `ops.generate_rays` makes, an analytic sphere through `ops.TSDF` and `ops.isosurface`, `DepthFrame`,
`fuse_mesh` and the command line on the trained fields."""
import os

import numpy as np
import pytest
import torch

import fuse_fixture as fx
import gpu_util as G
from mipnerf_pl_amd import _lib as L

pytestmark = pytest.mark.gpu
DEV = G.DEV
F = np.float32
BOX = ((-1.5,) * 3, (1.5,) * 3)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def same_bits(t, a):
    t = t.cpu().numpy()
    return t.shape == a.shape and np.array_equal(t.view(np.uint32), np.asarray(a, F).view(np.uint32))


# ---- rules T and F ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("carve", [True, False])
@pytest.mark.parametrize("lattice", range(len(fx.LATTICES)))
def test_integration_and_finalise_equal_the_float32_restatement_bit_for_bit(lattice, carve):
    from mipnerf_pl_amd import ops
    dims, lo, hi = fx.LATTICES[lattice]
    trunc = 0.35
    zero = np.zeros(dims[::-1], F)
    for num_frames in (1, 3, L.FUSE_FRAMES_PER_LAUNCH + 1):
        cams = fx.frame_cameras(num_frames, seed=lattice)
        depth, offsets = fx.frame_depths(cams, seed=num_frames)
        frames = ops.fuse_projection(cams)
        want = fx.integrate_f32(dims, lo, hi, trunc, carve, frames.numpy(), offsets, depth, zero, zero)
        vol = ops.TSDF(dims, lo, hi, trunc, device=DEV).integrate(frames, dev(depth), dev(offsets), carve=carve)
        assert same_bits(vol.sum, want[0]) and same_bits(vol.count, want[1]), num_frames
        assert (want[1] > 0).any() and (want[1] == 0).any()
        # offsets left out: the images lie one behind the other; two runs give the same bytes
        again = ops.TSDF(dims, lo, hi, trunc, device=DEV).integrate(frames.to(DEV), dev(depth), carve=carve)
        assert torch.equal(again.sum, vol.sum) and torch.equal(again.count, vol.count)
        # frame by frame, and split in two calls: the same bytes
        single = ops.TSDF(dims, lo, hi, trunc, device=DEV)
        for f in range(num_frames):
            single.integrate(frames[f:f + 1], dev(depth), dev(offsets[f:f + 1]), carve=carve)
        assert torch.equal(single.sum, vol.sum) and torch.equal(single.count, vol.count)
        if num_frames > 2:
            k = num_frames // 2
            split = ops.TSDF(dims, lo, hi, trunc, device=DEV)
            split.integrate(frames[:k], dev(depth), dev(offsets[:k]), carve=carve).integrate(frames[k:], dev(depth), dev(offsets[k:]), carve=carve)
            assert torch.equal(split.sum, vol.sum) and torch.equal(split.count, vol.count)
        for unseen in ("inside", "outside"):
            assert same_bits(vol.lattice(unseen), fx.finalise_f32(want[0], want[1], unseen))


def test_integration_reads_nothing_outside_the_depth_buffer():
    """a frame whose image does not lie inside the buffer is refused by `TSDF.integrate`; the entry point itself skips such pixels"""
    import ctypes as C
    from mipnerf_pl_amd import ops
    dims, lo, hi = fx.LATTICES[1]
    cams = fx.frame_cameras(2)
    depth, offsets = fx.frame_depths(cams)
    frames = ops.fuse_projection(cams)
    vol = ops.TSDF(dims, lo, hi, 0.35, device=DEV)
    with pytest.raises(ValueError, match="inside the depth buffer"):
        vol.integrate(frames, dev(depth[:-1]), dev(offsets))
    with pytest.raises(ValueError, match="inside the depth buffer"):
        vol.integrate(frames, dev(depth), dev(offsets + 1))
    with pytest.raises(ValueError, match="one offset per frame"):
        vol.integrate(frames, dev(depth), dev(offsets[:1]))
    # the second frame's image cut off after its first row: those pixels count as not there
    W = int(cams[1, 21])
    short = depth[:offsets[1] + W]
    fr, off, dp = frames.to(DEV), dev(offsets), dev(short)
    L.fuse_check(L.fuse_lib().mipnerf_fuse_integrate((C.c_int32 * 3)(*dims), (C.c_float * 3)(*lo), (C.c_float * 3)(*hi), 0.35, 1, 2, fr.data_ptr(),
                                                     off.data_ptr(), dp.data_ptr(), dp.numel(), vol.sum.data_ptr(), vol.count.data_ptr(),
                                                     torch.cuda.current_stream().cuda_stream))
    cut = depth.copy()
    cut[offsets[1] + W:] = np.nan                                  # a NaN pixel is skipped as well
    want = fx.integrate_f32(dims, lo, hi, 0.35, True, frames.numpy(), offsets, cut, np.zeros(dims[::-1], F), np.zeros(dims[::-1], F))
    assert same_bits(vol.sum, want[0]) and same_bits(vol.count, want[1])


# ---- rule D ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", fx.QUANTILE_NS)
def test_depth_quantile_kernel_inside_the_bracket(N):
    from mipnerf_pl_amd import ops
    B = 18                                                          # not a multiple of a workgroup's four rays
    for cls in fx.QUANTILE_CLASSES:
        for j, q in enumerate(fx.QUANTILES):
            w, t = fx.quantile_rays(N, cls, B=B, seed=1000 * N + j, q=q)
            one = ops.depth_quantile(dev(w), dev(t), q)
            three = ops.depth_quantile(dev(w), dev(t), fx.QUANTILES)
            assert tuple(one.shape) == (B,) and tuple(three.shape) == (B, 3)
            assert torch.equal(one, three[:, j])
            got = three.cpu().numpy()
            for k, qk in enumerate(fx.QUANTILES):
                assert fx.quantile_bracket(w, t, float(F(qk)), got[:, k]).all(), (N, cls, q, qk)
            if cls in ("empty", "zero"):
                assert np.isinf(got).all() and (got > 0).all()
            assert (got[:, 1:] >= got[:, :-1]).all()                # D(q) does not decrease with q (+inf included)


def test_depth_quantile_of_a_rendered_golden():
    from mipnerf_pl_amd import ops
    g = G.load_golden("fwd_c1_256x64_trained")
    w, t = g["wb1_l1_weights"], g["wb1_l1_t_samples"]
    got = ops.depth_quantile(dev(w), dev(t), fx.QUANTILES).cpu().numpy()
    for k, q in enumerate(fx.QUANTILES):
        assert fx.quantile_bracket(w, t, float(F(q)), got[:, k]).all()
    acc = g["wb1_l1_acc"]
    clear = np.abs(acc - 0.5) > 1e-4
    assert np.array_equal(np.isfinite(got[:, 1])[clear], (acc > 0.5)[clear]) and np.isfinite(got[:, 1]).any()
    four = ops.depth_quantile(dev(w), dev(t), (0.05, 0.5, 0.95, 0.99))
    assert torch.equal(four[:, :3], dev(got))
    with pytest.raises(ValueError, match="quantiles"):
        ops.depth_quantile(dev(w), dev(t), (0.1, 0.2, 0.3, 0.4, 0.5))
    with pytest.raises(ValueError, match=r"\(0, 1\)"):
        ops.depth_quantile(dev(w), dev(t), 1.0)
    with pytest.raises(ValueError, match="expected weights"):
        ops.depth_quantile(dev(w), dev(t[:, :-1]), 0.5)


# ---- rule P ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_projection_round_trip_of_generated_rays(mode):
    """p = o + t d of the rays the device generates comes back to its pixel centre and its t; the rays are float32, so the bound is the
    float32 rounding of d (2^-24 relative, times the focal length in pixels) and not the 1e-4 px of the float64 test"""
    from mipnerf_pl_amd import ops
    W, H, near, far = 14, 9, 0.5, 6.0
    c2w = fx.look_at((1.7, -2.1, 1.3), (0.1, 0.2, -0.1))
    rec = fx.camera_row(c2w, W, H, near, far, focal=15.4) if mode == 0 else \
        fx.camera_row(c2w, W, H, near, far, pix2cam=fx.pix2cam_of(15.4, 14.9, 7.3, 4.2, skew=0.03))
    rays = ops.generate_rays(dev(rec[None]))
    o, d = rays.origins.cpu().numpy().astype(np.float64), rays.directions.cpu().numpy().astype(np.float64)
    P = ops.fuse_projection(rec[None])[0].numpy().astype(np.float64)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    for t in (near, 3.0, far):
        p = o + t * d
        a, b, tt = [(P[4 * r:4 * r + 3] * p).sum(-1) + P[4 * r + 3] for r in range(3)]
        err = max(float(np.abs(a / tt - (xx.reshape(-1) + 0.5)).max()), float(np.abs(b / tt - (yy.reshape(-1) + 0.5)).max()))
        assert err <= 1e-4 and float(np.abs(tt / t - 1).max()) <= 1e-6


# ---- an analytic sphere through the device path ------------------------------------------------------------------------------------------
def test_sphere_fused_on_the_device_is_a_closed_sphere():
    from mipnerf_pl_amd import ops
    dims, lo, hi, h, trunc = fx.sphere_lattice()
    cams = fx.sphere_cameras()
    depth, offsets = fx.sphere_depths(cams)
    vol = ops.TSDF(dims, lo, hi, trunc, device=DEV).integrate(ops.fuse_projection(cams), dev(depth), dev(offsets))
    v, n, faces = ops.isosurface(vol.lattice(), 0.0, lo, hi)
    figures = fx.check_sphere_mesh(v.cpu().numpy(), faces.cpu().numpy())
    assert figures["vertices"] > 3000
    import isosurface_fixture as ix
    out = (v.cpu().numpy() - ix.CENTRE) / np.linalg.norm(v.cpu().numpy() - ix.CENTRE, axis=1, keepdims=True)
    assert float((out * n.cpu().numpy()).sum(1).min()) > 0.5                        # the normals point out of the sphere
    v2, _, f2 = ops.isosurface(vol.lattice("outside"), 0.0, lo, hi)
    assert ix.euler_characteristic(len(v2), f2.cpu().numpy()) != 2


# ---- DepthFrame, fuse_mesh and the command on the trained fields -----------------------------------------------------------------------
def trained_params(name="trained_field"):
    f = G.load_golden(name)
    return {k[2:]: f[k] for k in f if k.startswith("p_")}


def look_at_cameras(n, size, seed=0, radius=4.0):
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    focal = 0.5 * size / np.tan(0.5 * 0.6911112070083618)
    return np.stack([fx.camera_row(fx.look_at(radius * v, (0, 0, 0)), size, size, 2.0, 6.0, focal=focal) for v in d])


def test_depth_frame_is_the_quantile_of_the_chunk_forwards():
    from mipnerf_pl_amd import ops
    from mipnerf_pl_amd.fuse import DepthFrame
    from mipnerf_pl_amd.rays import Rays
    model = G.make_model(trained_params(), 64, "fp32").eval()
    cams = dev(look_at_cameras(6, 24))
    n, chunk, q = 24 * 24, 250, 0.5                                # chunks of 250, 250 and 76 rays
    frame = DepthFrame(model, n, chunk, True, torch.device(DEV), quantiles=(q, 0.9))
    assert frame.chunks() == [(0, 250), (250, 500), (500, 576)]
    finite = 0
    for f in range(6):
        rays = ops.generate_rays(cams, cam_idx=torch.full((n,), f, dtype=torch.int32, device=DEV),
                                 pix_idx=torch.arange(n, dtype=torch.int32, device=DEV))
        depth = frame(rays).clone()
        acc = frame.acc.clone()
        for lo, hi in frame.chunks():
            with torch.no_grad():
                ret = model._forward_native(Rays(*[x[lo:hi] for x in rays]), False, True)
            assert torch.equal(depth[lo:hi], ops.depth_quantile(ret[-1][3], ret[-1][4], (q, 0.9)))
            assert torch.equal(acc[lo:hi], ret[-1][2])
        clear = (acc - q).abs() > 1e-4
        assert torch.equal(torch.isfinite(depth[:, 0])[clear], (acc > q)[clear])
        assert bool((depth[:, 1] >= depth[:, 0]).all())
        finite += int(torch.isfinite(depth[:, 0]).sum())
    assert 0 < finite < 6 * n                                       # the views hold object and background


def _system(params, precision="fp32", **hparams):
    from mipnerf_pl_amd.system import DEFAULT_HPARAMS, MipNeRFSystem
    hp = dict(DEFAULT_HPARAMS)
    hp.update({"nerf.num_samples": 32, "exp_name": "exp", "val.batch_type": "single_image"})
    hp.update(hparams)
    system = MipNeRFSystem(hp, precision=precision)
    missing, unexpected = system.load_state_dict({"mip_nerf.mlp." + k: torch.from_numpy(v.copy()) for k, v in params.items()}, strict=True)
    assert not missing and not unexpected
    return system.to(DEV).eval()


def hand_composition(system, cams, dims, lo, hi, trunc_cells=3.0, quantile=0.5, unseen="inside", carve=True):
    """the public ops one after the other: generate_rays -> DepthFrame -> TSDF.integrate -> TSDF.lattice -> isosurface"""
    from mipnerf_pl_amd import ops
    from mipnerf_pl_amd.fuse import DepthFrame
    cams = torch.as_tensor(cams, dtype=torch.float32)
    h = max((hi[a] - lo[a]) / (dims[a] - 1) for a in range(3))
    vol = ops.TSDF(dims, lo, hi, trunc_cells * h, device=DEV)
    frames = ops.fuse_projection(cams)
    depths = []
    for f in range(len(cams)):
        n = int(cams[f, 21]) * int(cams[f, 22])
        rays = ops.generate_rays(cams.to(DEV), cam_idx=torch.full((n,), f, dtype=torch.int32, device=DEV),
                                 pix_idx=torch.arange(n, dtype=torch.int32, device=DEV))
        depths.append(DepthFrame(system.mip_nerf, n, n, False, torch.device(DEV), (quantile,))(rays)[:, 0].clone())
        vol.integrate(frames[f:f + 1], depths[-1], carve=carve)
    lattice = vol.lattice(unseen)
    return (lattice,) + tuple(ops.isosurface(lattice, 0.0, lo, hi)) + (vol, depths)


def test_fuse_mesh_is_the_hand_composition_of_the_public_ops(tmp_path):
    from mipnerf_pl_amd.fuse import fuse_mesh
    from mipnerf_pl_amd.mesh import read_ply, write_ply
    system = _system(trained_params())
    cams = look_at_cameras(8, 24, seed=3)
    dims = (24, 22, 20)
    mesh = fuse_mesh(system, cams, grid=dims, lo=BOX[0], hi=BOX[1], precision="fp32")
    lattice, v, nrm, faces, vol, depths = hand_composition(system, cams, dims, *BOX)
    assert torch.equal(mesh.sigma, lattice) and torch.equal(mesh.vertices, v) and torch.equal(mesh.normals, nrm) and torch.equal(mesh.faces, faces)
    assert len(v) > 100 and mesh.colors.dtype == torch.uint8 and mesh.colors.shape == v.shape and torch.isfinite(mesh.rgb).all()
    assert float((vol.count == 0).float().mean()) < 1.0 and any(bool(torch.isinf(d).any()) for d in depths)
    path = write_ply(str(tmp_path / "m.ply"), mesh.vertices, mesh.normals, mesh.faces, mesh.colors)
    rv, rn, rf, rc = read_ply(path)
    assert np.array_equal(rv, v.cpu().numpy()) and np.array_equal(rf, faces.cpu().numpy()) and np.array_equal(rc, mesh.colors.cpu().numpy())
    bare = fuse_mesh(system, cams, grid=dims, lo=BOX[0], hi=BOX[1], precision="fp32", color=False, unseen="outside", carve=False)
    want = hand_composition(system, cams, dims, *BOX, unseen="outside", carve=False)
    assert bare.colors is None and bare.rgb is None and torch.equal(bare.sigma, want[0]) and torch.equal(bare.faces, want[3])
    assert system.mip_nerf.precision == L.PREC_FP32
    with pytest.raises(NotImplementedError, match="camera mode 2"):
        bad = cams.copy()
        bad[0, 12:21], bad[0, 26] = fx.pix2cam_of(30, 30, 12, 12).reshape(-1), 2
        fuse_mesh(system, bad, grid=dims)


def test_command_line_end_to_end(tmp_path, capsys):
    import dataset_fixture as dx
    from mipnerf_pl_amd import fuse_mesh as cli
    from mipnerf_pl_amd.datasets import Blender
    from mipnerf_pl_amd.fuse import fuse_mesh
    from mipnerf_pl_amd.mesh import read_ply
    system = _system(trained_params(), dataset_name="blender", exp_name="cli")
    ckpt, data, out = str(tmp_path / "last.ckpt"), dx.write_blender(str(tmp_path / "data"), counts=(("train", 5), ("val", 1), ("test", 1))), \
        str(tmp_path / "out")
    system.save_checkpoint(ckpt)
    path = cli.main(["--ckpt", ckpt, "--data", data, "--out_dir", out, "--grid", "20", "18", "16", "--precision", "fp32", "--save_tsdf",
                     "--save_depth"])
    assert path == os.path.join(out, "mesh", "cli", "fused_20x18x16.ply") and os.path.exists(path)
    cams = Blender(data, split="train", white_bkgd=True, device=torch.device(DEV)).cameras
    assert tuple(cams.shape) == (5, 32)
    mesh = fuse_mesh(system, cams, grid=(20, 18, 16), lo=BOX[0], hi=BOX[1], precision="fp32")
    rv, rn, rf, rc = read_ply(path)
    assert np.array_equal(rv, mesh.vertices.cpu().numpy()) and np.array_equal(rn, mesh.normals.cpu().numpy())
    assert np.array_equal(rf, mesh.faces.cpu().numpy()) and np.array_equal(rc, mesh.colors.cpu().numpy())
    vol = np.load(os.path.join(out, "mesh", "cli", "tsdf_20x18x16.npy"))
    assert vol.shape == (16, 18, 20) and np.array_equal(vol, mesh.sigma.cpu().numpy())
    assert sorted(os.listdir(os.path.join(out, "mesh", "cli", "depth"))) == [f"{i:05d}_depth.png" for i in range(5)]
    line = capsys.readouterr().out.splitlines()[-1]
    assert line.startswith(f"{path}: 5 views, {len(rv)} vertices, {len(rf)} faces, ") and "lattice points unseen (called inside)" in line
    assert "of the pixels without a depth (opacity below 0.5)" in line
    # every second camera; no colours; nothing else written
    out2 = str(tmp_path / "out2")
    path2 = cli.main(["--ckpt", ckpt, "--data", data, "--out_dir", out2, "--grid", "20", "18", "16", "--precision", "fp32", "--every", "2",
                      "--no_color"])
    rv2, _, rf2, rc2 = read_ply(path2)
    mesh2 = fuse_mesh(system, cams[::2], grid=(20, 18, 16), lo=BOX[0], hi=BOX[1], precision="fp32", color=False)
    assert rc2 is None and np.array_equal(rv2, mesh2.vertices.cpu().numpy()) and np.array_equal(rf2, mesh2.faces.cpu().numpy())
    assert capsys.readouterr().out.splitlines()[-1].startswith(f"{path2}: 3 views, ")
    assert os.listdir(os.path.join(out2, "mesh", "cli")) == ["fused_20x18x16.ply"]
    # a split without frames is refused before anything is rendered or written
    out3 = str(tmp_path / "out3")
    os.makedirs(str(tmp_path / "empty"))
    empty = dx.write_blender(str(tmp_path / "empty"), counts=(("train", 0), ("val", 1), ("test", 1)))
    with pytest.raises(SystemExit, match="has no frames to fuse"):
        cli.main(["--ckpt", ckpt, "--data", empty, "--out_dir", out3, "--grid", "9"])
    assert not os.path.exists(out3)


def test_an_unbounded_checkpoint_runs_end_to_end(tmp_path, capsys):
    import dataset_fixture as dx
    from mipnerf_pl_amd import fuse_mesh as cli
    from mipnerf_pl_amd.datasets import PathGen, RealData360
    from mipnerf_pl_amd.fuse import fuse_mesh
    from mipnerf_pl_amd.mesh import read_ply
    bias = float(G.load_golden("full360_1000x96")["density_bias"])
    system = _system(trained_params("trained_field_360"), **{"nerf.unbounded": True, "nerf.density_bias": bias, "dataset_name": "llff",
                                                            "exp_name": "cli360", "factor": 4})
    ckpt, data, out = str(tmp_path / "last.ckpt"), dx.write_llff(str(tmp_path / "data")), str(tmp_path / "out")
    system.save_checkpoint(ckpt)
    path = cli.main(["--ckpt", ckpt, "--data", data, "--out_dir", out, "--grid", "17", "--precision", "fp32", "--save_tsdf"])
    assert path == os.path.join(out, "mesh", "cli360", "fused_17x17x17.ply")
    dataset = RealData360(data, split="train", white_bkgd=bool(system.hparams["val.white_bkgd"]), factor=4, device=torch.device(DEV))
    cams = PathGen(dataset, poses=dataset.camtoworlds, device=torch.device(DEV)).cameras
    assert cams.shape[0] == len(dataset.camtoworlds) > 0 and bool((cams[:, 26] == 1).all())
    mesh = fuse_mesh(system, cams, grid=17, precision="fp32")
    rv, rn, rf, rc = read_ply(path)
    assert np.array_equal(rv, mesh.vertices.cpu().numpy()) and np.array_equal(rf, mesh.faces.cpu().numpy())
    vol = np.load(os.path.join(out, "mesh", "cli360", "tsdf_17x17x17.npy"))
    assert vol.shape == (17, 17, 17) and np.array_equal(vol, mesh.sigma.cpu().numpy()) and (np.abs(vol) <= 1).all()
    assert f"{cams.shape[0]} views" in capsys.readouterr().out.splitlines()[-1]
    if len(rv):
        assert rc.shape == rv.shape and np.isfinite(rv).all()
