"""GPU: the image kernels (kernels_vis.hip) byte-exact against numpy / torch restatements of utils/vis.py, and the device loops of eval.py
(mipnerf_pl_amd.evaluate) and render_video.py (mipnerf_pl_amd.render_video) end to end on small synthetic scenes."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def np_visualize_depth(x):
    """vis.py:visualize_depth up to the colour lookup, numpy float32 as there: nan_to_num, min / max, (x - mi) / max(ma - mi, 1e-8),
    (255 * x).astype(np.uint8) (NaN -> 0, what that cast gives on x86), then the row of the table the reference writes."""
    from mipnerf_pl_amd.colormap import jet_written
    x = np.nan_to_num(np.asarray(x, np.float32))
    mi, ma = np.min(x), np.max(x)
    with np.errstate(all="ignore"):
        x = (x - mi) / max(ma - mi, 1e-8)
        v = 255 * x
    assert v.dtype == np.float32
    return jet_written()[np.where(np.isnan(v), 0, v).astype(np.uint8)]


def _maps():
    rng = np.random.default_rng(5)
    m = {"random": rng.normal(3.0, 1.5, (37, 53)).astype(np.float32),
         "single_pixel": np.array([[4.25]], np.float32),
         "constant": np.full((9, 14), 3.5, np.float32),
         "range_below_1e-8": (np.float32(1e-3) + np.float32(1e-10) * rng.integers(0, 40, (11, 7))).astype(np.float32),
         "acc_like": np.clip(rng.uniform(-0.2, 1.2, (31, 29)), 0, 1).astype(np.float32)}
    a = rng.uniform(2.0, 6.0, (23, 19)).astype(np.float32)
    a[3, 4], a[10, 2], a[20, 18] = np.nan, np.inf, np.nan
    m["nan_and_+inf"] = a
    b = rng.uniform(2.0, 6.0, (23, 19)).astype(np.float32)
    b[0, 0], b[7, 7], b[22, 18] = -np.inf, np.nan, np.inf          # range overflows to inf: most pixels 0, the +inf one NaN -> 0
    m["nan_and_+-inf"] = b
    c = rng.uniform(2.0, 6.0, (17, 12)).astype(np.float32)
    c[5, 5] = -np.inf
    m["-inf"] = c
    big = rng.uniform(2.0, 6.0, (800, 800)).astype(np.float32)
    big[799, 799], big[0, 1], big[400, 3] = 9.0, 0.5, np.nan     # extremes in the first and the last partial blocks
    m["800x800"] = big
    return m


@pytest.mark.parametrize("name", list(_maps()))
def test_visualize_map_byte_exact_eager_and_in_graph(name):
    from mipnerf_pl_amd import ops
    x = _maps()[name]
    want = np_visualize_depth(x)
    xd = torch.from_numpy(x).to(DEV)
    got = ops.visualize_map(xd).cpu().numpy()
    assert got.shape == x.shape + (3,) and got.dtype == np.uint8
    bad = np.argwhere(np.any(got != want, -1))
    assert bad.size == 0, (name, bad[:5], got[tuple(bad[0])], want[tuple(bad[0])])
    # the same two launches captured in a hipGraph with static buffers
    out = torch.zeros(*x.shape, 3, dtype=torch.uint8, device=DEV)
    ws = torch.empty(ops.visualize_workspace_floats(x.size), device=DEV)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.visualize_map(xd, out=out, workspace=ws)
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), got)


def test_image_to_u8_byte_exact():
    from mipnerf_pl_amd import ops
    rng = np.random.default_rng(9)
    x = rng.uniform(-0.5, 1.5, (41, 67, 3)).astype(np.float32)
    edges = np.array([0.0, 1.0, -1e-30, 1 + 1e-7, 0.5 / 255, np.nextafter(np.float32(0.5 / 255), np.float32(0)), 127.5 / 255, 3e38, -3e38],
                     np.float32)
    x.reshape(-1)[:edges.size] = edges
    t = torch.from_numpy(x)
    want = t.clamp(0.0, 1.0).mul(255).add(0.5).clamp(0, 255).to(torch.uint8).numpy()      # save_image_tensor + torchvision save_image
    got = ops.image_to_u8(t.to(DEV)).cpu().numpy()
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    out = torch.empty(41, 67, 3, dtype=torch.uint8, device=DEV)
    xd = t.to(DEV)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.image_to_u8(xd, out=out)
    g.replay()
    assert np.array_equal(out.cpu().numpy(), want)


def _system(params, num_samples, precision="fp32"):
    from mipnerf_pl_amd.system import DEFAULT_HPARAMS, MipNeRFSystem
    hp = dict(DEFAULT_HPARAMS)
    hp.update({"nerf.num_samples": num_samples, "exp_name": "exp", "val.batch_type": "single_image"})
    system = MipNeRFSystem(hp, precision=precision)
    missing, unexpected = system.load_state_dict({"mip_nerf.mlp." + k: torch.from_numpy(v.copy()) for k, v in params.items()}, strict=True)
    assert not missing and not unexpected
    return system.to(DEV).eval()


def _read(path):
    from PIL import Image
    return np.array(Image.open(path))


def _files(root):
    out = {}
    for d, _, fs in os.walk(root):
        for f in fs:
            with open(os.path.join(d, f), "rb") as fh:
                out[os.path.relpath(os.path.join(d, f), root)] = fh.read()
    return out


def test_single_scale_eval_against_oracle(tmp_path):
    from dataset_fixture import write_blender
    from mipnerf_pl_amd.datasets import Blender
    from mipnerf_pl_amd.evaluate import FrameEvaluator, evaluate
    from oracle import mipnerf_oracle as orc
    data = write_blender(str(tmp_path / "data"), seed=4, counts=(("test", 3),), w=24, h=20)
    params = orc.make_params(seed=0, density_gain=40.0)
    system = _system(params, 64)
    ds = Blender(data, split="test", white_bkgd=True, batch_type="single_image", device=torch.device(DEV))
    out_g, out_e = str(tmp_path / "graph"), str(tmp_path / "eager")
    # chunk 200 of 480 rays: two full chunks and a ragged one
    psnrs, ssims = evaluate(system, ds, out_g, "exp", scale=1, save_image=True, chunk_size=200, base_size=(24, 20))
    evaluate(system, ds, out_e, "exp", scale=1, save_image=True, chunk_size=200, base_size=(24, 20), use_graph=False)
    folder = os.path.join(out_g, "test", "exp")
    assert open(os.path.join(folder, "psnrs.txt")).read() == " ".join(str(v) for v in psnrs)
    assert open(os.path.join(folder, "ssims.txt")).read() == " ".join(str(v) for v in ssims)
    pngs = sorted(f for f in os.listdir(os.path.join(folder, "1")) if f[:5].isdigit())
    assert pngs == sorted(f"{i:05d}_{t}.png" for i in range(3) for t in ("rgb", "dist", "acc"))
    # graph and eager runs write identical files
    fg, fe = _files(out_g), _files(out_e)
    assert fg.keys() == fe.keys() and all(fg[k] == fe[k] for k in fg)
    ev = FrameEvaluator(system.mip_nerf, 20, 24, 200, True, torch.device(DEV))
    for i in range(3):
        rays, gt = ds[i]
        ret = orc.mipnerf_forward(params, orc.Rays(*[t.reshape(-1, t.shape[-1]).cpu().numpy() for t in rays]), False, True, num_samples=64)
        o_psnr, o_ssim = orc.eval_errors(ret[-1][0].reshape(20, 24, 3), gt.cpu().numpy())
        assert abs(psnrs[i] - float(o_psnr)) < 1e-4 and abs(ssims[i] - float(o_ssim)) < 1e-5, (i, psnrs[i], o_psnr, ssims[i], o_ssim)
        # the PNGs hold the kernels' bytes
        imgs = [t.cpu().numpy() for t in ev.images(*ev.render(rays))]
        for tag, want in zip(("rgb", "dist", "acc"), imgs):
            assert np.array_equal(_read(os.path.join(folder, "1", f"{i:05d}_{tag}.png")), want), (i, tag)
        rgb, dist, acc = ev.render(rays)
        assert np.array_equal(imgs[1], np_visualize_depth(dist.cpu().numpy())) and np.array_equal(imgs[2], np_visualize_depth(acc.cpu().numpy()))
        assert np.abs(acc.cpu().numpy().reshape(-1) - ret[-1][2].reshape(-1)).max() < 5e-5


def test_multi_scale_eval_layout_and_summary(tmp_path):
    from dataset_fixture import write_multicam_scene
    from mipnerf_pl_amd.datasets import Multicam
    from mipnerf_pl_amd.evaluate import evaluate, summarize_results
    from oracle import mipnerf_oracle as orc
    data = write_multicam_scene(str(tmp_path / "data"), seed=3, counts=(("test", 2),), base=32, scales=4)
    system = _system(orc.make_params(seed=1, density_gain=40.0), 32)
    ds = Multicam(data, split="test", white_bkgd=True, batch_type="single_image", device=torch.device(DEV))
    assert ds.sizes == [(32 // 2 ** j, 32 // 2 ** j) for _ in range(2) for j in range(4)]
    out = str(tmp_path / "out")
    psnrs, ssims = evaluate(system, ds, out, "ms", scale=4, save_image=True, chunk_size=256, base_size=(32, 32))
    folder = os.path.join(out, "test", "ms")
    assert sorted(d for d in os.listdir(folder) if os.path.isdir(os.path.join(folder, d))) == ["1", "2", "4", "8"]
    for j, d in enumerate(["1", "2", "4", "8"]):
        pngs = sorted(f for f in os.listdir(os.path.join(folder, d)) if f[:5].isdigit())
        assert pngs == sorted(f"{n:05d}_{t}.png" for n in range(2) for t in ("rgb", "dist", "acc")), d      # n advances every 4 images
        assert _read(os.path.join(folder, d, "00001_rgb.png")).shape == (32 >> j, 32 >> j, 3)
    p, s = np.array(psnrs).reshape(2, 4).mean(0), np.array(ssims).reshape(2, 4).mean(0)
    summary = summarize_results(out, ["ms"], 4)
    assert summary.split(" | ")[:2] == [" ".join(f"{v:0.4f}" for v in p), " ".join(f"{v:0.4f}" for v in s)]
    assert all(np.isfinite(psnrs)) and all(0 < v <= 1 for v in ssims)


def test_spheric_render_frames(tmp_path):
    from mipnerf_pl_amd.datasets import RenderGen
    from mipnerf_pl_amd.model import GraphedFrame
    from mipnerf_pl_amd.render_video import CAMERA_ANGLE_X, render_video
    from oracle import mipnerf_oracle as orc
    system = _system(orc.make_params(seed=2, density_gain=40.0), 32)
    folder = render_video(system, str(tmp_path), "exp", 2, base_size=(24, 24), n_poses=3, chunk_size=160)
    assert folder == os.path.join(str(tmp_path), "render_spheric", "exp")
    focal = .5 * 24 / np.tan(.5 * CAMERA_ANGLE_X)
    rg = RenderGen(focal, (24, 24), 2, device=torch.device(DEV), n_poses=3)
    assert len(rg) == 6 and rg.sizes == [(24, 24)] * 3 + [(12, 12)] * 3
    frames = {}
    for i in range(6):
        h, w = rg.sizes[i]
        f = os.path.join(folder, "1" if w == 24 else "2", f"{i % 3:05d}_rgb.png")
        got = _read(f)
        assert got.shape == (h, w, 3)
        if (h, w) not in frames:
            frames[(h, w)] = GraphedFrame(system.mip_nerf, h * w, 160, True, torch.device(DEV))
        rays = rg[i]
        with torch.no_grad():
            _, fine, _ = frames[(h, w)](type(rays)(*[t.reshape(h * w, -1) for t in rays]))
        want = fine.cpu().reshape(h, w, 3).clamp(0.0, 1.0).mul(255).add(0.5).clamp(0, 255).to(torch.uint8).numpy()
        assert np.array_equal(got, want), i
        for tag in ("dist", "acc"):
            assert _read(f.replace("_rgb", "_" + tag)).shape == (h, w, 3)


def test_eval_command_line_end_to_end(tmp_path, capsys):
    """python -m mipnerf_pl_amd.eval on a checkpoint written by MipNeRFSystem: load_from_checkpoint, the test split of
    hparams['dataset_name'], the same metric files as calling evaluate() directly, and the summary line."""
    from dataset_fixture import write_blender
    from mipnerf_pl_amd import eval as eval_cli
    from mipnerf_pl_amd.datasets import Blender
    from mipnerf_pl_amd.evaluate import evaluate, summarize_results
    from oracle import mipnerf_oracle as orc
    data = write_blender(str(tmp_path / "data"), seed=6, counts=(("test", 2),), w=16, h=16)
    system = _system(orc.make_params(seed=5, density_gain=40.0), 32)
    system.hparams.update({"dataset_name": "blender", "exp_name": "cli"})
    ckpt = str(tmp_path / "last.ckpt")
    system.save_checkpoint(ckpt)
    out = str(tmp_path / "out")
    summary = eval_cli.main(["--ckpt", ckpt, "--data", data, "--out_dir", out, "--scale", "1", "--save_image", "--chunk_size", "100",
                             "--precision", "fp32", "--base_size", "16", "16"])
    assert capsys.readouterr().out.splitlines()[-2:] == ["PSNR | SSIM | Average", summary]
    assert summary == summarize_results(out, ["cli"], 1)
    assert sorted(f for f in os.listdir(os.path.join(out, "test", "cli", "1")) if f[:5].isdigit()) == \
        sorted(f"{i:05d}_{t}.png" for i in range(2) for t in ("rgb", "dist", "acc"))
    ds = Blender(data, split="test", white_bkgd=True, batch_type="single_image", device=torch.device(DEV))
    psnrs, _ = evaluate(system, ds, str(tmp_path / "direct"), "cli", chunk_size=100, base_size=(16, 16))
    assert open(os.path.join(out, "test", "cli", "psnrs.txt")).read() == " ".join(str(v) for v in psnrs)
    assert eval_cli.main(["--ckpt", ckpt, "--out_dir", out, "--scale", "1", "--summa_only"]) == summary
