"""CPU (no GPU): the host side of the test-set evaluation and the spherical render (mipnerf_pl_amd.evaluate / .eval / .render_video)
-- the summary string of utils/metrics.py:summarize_results, the JET table of the visualisation kernel, the eval.py file layout, the
animated-PNG video fallback and both command lines."""
import math
import os
import sys

import numpy as np
import pytest

from mipnerf_pl_amd import colormap, evaluate

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _write_scene(root, exp, psnrs, ssims):
    d = os.path.join(root, "test", exp)
    os.makedirs(d, exist_ok=True)
    with open(os.path.join(d, "psnrs.txt"), "w") as f:
        f.write(" ".join(str(v) for v in psnrs))
    with open(os.path.join(d, "ssims.txt"), "w") as f:
        f.write(" ".join(str(v) for v in ssims))


def _avg_avg(psnr, ssim):
    mse = math.exp(-0.1 * math.log(10.0) * psnr)
    return math.exp(0.5 * (math.log(mse) + math.log(math.sqrt(1.0 - ssim))))


def test_summarize_results_one_bucket(tmp_path):
    _write_scene(str(tmp_path), "lego", [30.0, 32.0, 34.0], [0.90, 0.92, 0.97])
    _write_scene(str(tmp_path), "ship", [20.0, 22.0], [0.80, 0.84])
    psnr = (32.0 + 21.0) / 2            # per-scene means, then the mean over scenes
    ssim = (0.93 + 0.82) / 2
    want = f"{psnr:0.4f} | {ssim:0.4f} | {_avg_avg(psnr, ssim):0.4f}"
    assert evaluate.summarize_results(str(tmp_path), ["lego", "ship"], 1) == want
    assert want == "26.5000 | 0.8750 | 0.0281"


def test_summarize_results_four_buckets(tmp_path):
    # two views x four scales, in the multi-scale test set's order (view-major): bucket j = every 4th value from j
    p = [30.0, 28.0, 26.0, 24.0, 32.0, 30.0, 28.0, 20.0]
    s = [0.95, 0.90, 0.85, 0.80, 0.97, 0.92, 0.87, 0.70]
    _write_scene(str(tmp_path), "ms", p, s)
    pb = [31.0, 29.0, 27.0, 22.0]
    sb = [0.96, 0.91, 0.86, 0.75]
    avg = _avg_avg(sum(pb) / 4, sum(sb) / 4)
    want = " | ".join([" ".join(f"{v:0.4f}" for v in pb), " ".join(f"{v:0.4f}" for v in sb), f"{avg:0.4f}"])
    assert evaluate.summarize_results(str(tmp_path), ["ms"], 4) == want
    assert want.startswith("31.0000 29.0000 27.0000 22.0000 | 0.9600 0.9100 0.8600 0.7500 | ")


def test_jet_table_endpoints_segments_and_channel_swap():
    rgb, written = colormap.jet_rgb(), colormap.jet_written()
    assert rgb.shape == written.shape == (256, 3) and written.dtype == np.uint8
    # what the reference writes is OpenCV's BGR row read as RGB: the channels of the jet ramp swapped
    assert np.array_equal(written, rgb[:, ::-1])
    assert tuple(written[0]) == (128, 0, 0) and tuple(written[255]) == (0, 0, 128)
    assert tuple(rgb[0]) == (0, 0, 128) and tuple(rgb[255]) == (128, 0, 0)       # the jet proper: dark blue .. dark red
    r, g, b = (rgb[:, c].astype(int) for c in range(3))
    # Octave's jet(256) breakpoints x = 1/8, 3/8, 5/8, 7/8 of i / 255 fall between i = 31|32, 95|96, 159|160, 223|224
    assert np.all(np.diff(b[:32]) > 0) and np.all(b[32:96] == 255) and np.all(np.diff(b[96:160]) < 0) and np.all(b[160:] == 0)
    assert np.all(g[:32] == 0) and np.all(np.diff(g[32:96]) > 0) and np.all(g[96:160] == 255) and np.all(np.diff(g[160:224]) < 0)
    assert np.all(g[224:] == 0)
    assert np.all(r[:96] == 0) and np.all(np.diff(r[96:160]) > 0) and np.all(r[160:224] == 255) and np.all(np.diff(r[224:]) < 0)
    # slope 4 per entry (4 * 255 / 255) inside every ramp
    assert set(np.diff(r[97:159]).tolist()) == {4} and set(np.diff(b[1:31]).tolist()) == {4}


def test_committed_jet_header_is_the_generator_output():
    with open(colormap.HEADER) as f:
        assert f.read() == colormap.header_text()


def test_jet_table_equals_opencv():
    cv2 = pytest.importorskip("cv2")
    lut = cv2.applyColorMap(np.arange(256, dtype=np.uint8).reshape(256, 1), cv2.COLORMAP_JET).reshape(256, 3)
    assert np.array_equal(lut, colormap.jet_written())          # cv2's BGR bytes = what PIL stores as RGB


def test_image_slots_follow_eval_py():
    # single scale: one image per n, all in directory 1 (base 800 / W 800)
    assert evaluate.image_slots([(800, 800)] * 3, 1, 800) == [(0, "1"), (1, "1"), (2, "1")]
    # multi-scale test set: each view at W = 64, 32, 16, 8; n advances every 4 images
    sizes = [(64 // 2 ** j, 64 // 2 ** j) for _ in range(3) for j in range(4)]
    slots = evaluate.image_slots(sizes, 4, 64)
    assert [n for n, _ in slots] == [0] * 4 + [1] * 4 + [2] * 4
    assert [d for _, d in slots] == ["1", "2", "4", "8"] * 3


def test_write_metrics_one_line_each(tmp_path):
    evaluate.write_metrics(str(tmp_path), [np.float32(31.25), 29.5], [0.5, np.float32(0.875)])
    assert open(tmp_path / "psnrs.txt").read() == "31.25 29.5"
    assert open(tmp_path / "ssims.txt").read() == "0.5 0.875"


def test_generate_video_falls_back_to_animated_png(tmp_path, monkeypatch, capsys):
    from PIL import Image
    monkeypatch.setitem(sys.modules, "imageio", None)        # `import imageio` raises ImportError
    rng = np.random.default_rng(0)
    frames = {1: [rng.integers(0, 256, (6, 8, 3), dtype=np.uint8) for _ in range(3)],
              2: [rng.integers(0, 256, (3, 4, 3), dtype=np.uint8) for _ in range(3)]}
    for s, fr in frames.items():
        os.makedirs(tmp_path / str(s))
        for i, f in enumerate(fr):
            Image.fromarray(f).save(tmp_path / str(s) / f"{i:05d}_rgb.png")
            Image.fromarray(255 - f).save(tmp_path / str(s) / f"{i:05d}_dist.png")     # not a video frame
    written = evaluate.generate_video(str(tmp_path))
    assert written == [str(tmp_path / "1" / "video_1.png"), str(tmp_path / "2" / "video_2.png")]
    assert "animated PNG" in capsys.readouterr().out
    for s, path in zip((1, 2), written):
        want = frames[s] + frames[s][::-1]                     # forward, then reverse
        im = Image.open(path)
        got = []
        for k in range(im.n_frames):
            im.seek(k)
            # PIL folds identical consecutive frames into one of the summed duration: expand at 40 fps = 25 ms per frame
            got += [np.array(im.convert("RGB"))] * int(round(im.info["duration"] / 25.0))
        assert len(got) == len(want) and all(np.array_equal(a, b) for a, b in zip(got, want))


def test_eval_command_line():
    from mipnerf_pl_amd.eval import build_parser
    a = build_parser().parse_args(["--ckpt", "c.ckpt", "--data", "d", "--out_dir", "o", "--scale", "4", "--save_image"])
    assert (a.ckpt, a.data, a.out_dir, a.scale, a.save_image, a.summa_only) == ("c.ckpt", "d", "o", 4, True, False)
    assert (a.chunk_size, a.white_bkgd, a.base_size, a.precision, a.use_graph) == (12288, True, [800, 800], None, True)
    a = build_parser().parse_args(["--out_dir", "o", "--scale", "1", "--summa_only", "--precision", "bf16", "--no-graph",
                                   "--white_bkgd", "False", "--chunk_size", "8192", "--base_size", "64", "64"])
    assert (a.summa_only, a.precision, a.use_graph, a.white_bkgd, a.chunk_size, a.base_size) == (True, "bf16", False, False, 8192, [64, 64])
    for bad in (["--out_dir", "o", "--scale", "2"], ["--scale", "1"], ["--out_dir", "o"]):
        with pytest.raises(SystemExit):
            build_parser().parse_args(bad)


def test_render_video_command_line():
    from mipnerf_pl_amd.render_video import CAMERA_ANGLE_X, build_parser
    a = build_parser().parse_args(["--ckpt", "c", "--out_dir", "o", "--scale", "4"])
    assert (a.scale, a.camera_angle_x, a.gen_video_only, a.render_images_dir, a.n_poses) == (4, CAMERA_ANGLE_X, False, None, 120)
    assert CAMERA_ANGLE_X == 0.6911112070083618
    a = build_parser().parse_args(["--out_dir", "o", "--scale", "2", "--gen_video_only", "--render_images_dir", "r", "--n_poses", "3",
                                   "--camera_angle_x", "0.5", "--precision", "fp32", "--no-graph"])
    assert (a.gen_video_only, a.render_images_dir, a.n_poses, a.camera_angle_x, a.precision, a.use_graph) == (True, "r", 3, 0.5, "fp32", False)
    with pytest.raises(SystemExit):
        build_parser().parse_args(["--out_dir", "o"])


def test_render_video_gen_video_only_needs_a_directory(tmp_path, monkeypatch):
    from mipnerf_pl_amd import render_video
    monkeypatch.setitem(sys.modules, "imageio", None)
    with pytest.raises(SystemExit):
        render_video.main(["--out_dir", str(tmp_path), "--scale", "1", "--gen_video_only"])
    from PIL import Image
    os.makedirs(tmp_path / "1")
    Image.fromarray(np.zeros((2, 2, 3), np.uint8)).save(tmp_path / "1" / "00000_rgb.png")
    assert render_video.main(["--out_dir", str(tmp_path), "--scale", "1", "--gen_video_only", "--render_images_dir", str(tmp_path)]) == \
        [str(tmp_path / "1" / "video_1.png")]


def test_eval_summa_only_reads_the_checkpoint_and_the_metric_files(tmp_path, capsys):
    from mipnerf_pl_amd import eval as eval_cli
    from mipnerf_pl_amd.system import DEFAULT_HPARAMS, MipNeRFSystem
    hp = dict(DEFAULT_HPARAMS)
    hp.update({"exp_name": "lego", "dataset_name": "blender"})
    MipNeRFSystem(hp).save_checkpoint(str(tmp_path / "last.ckpt"))
    _write_scene(str(tmp_path), "lego", [30.0, 32.0, 34.0], [0.90, 0.92, 0.97])
    summary = eval_cli.main(["--ckpt", str(tmp_path / "last.ckpt"), "--out_dir", str(tmp_path), "--scale", "1", "--summa_only"])
    assert summary == evaluate.summarize_results(str(tmp_path), ["lego"], 1) and summary.startswith("32.0000 | 0.9300 | ")
    assert capsys.readouterr().out.splitlines()[-2:] == ["PSNR | SSIM | Average", summary]
