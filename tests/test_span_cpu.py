"""CPU (no GPU): the span fixture against first principles on a tiny grid, the agreement of the header, the binding and the docstrings on
the span rules, argument validation of mipnerf_ray_span, and the command-line flags of tightened culling."""
import os
import re

import numpy as np
import pytest

import occupancy_fixture as fx
import span_fixture as sx

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the fixture from first principles ------------------------------------------------------------------------------------
def test_span_of_axis_aligned_rays_through_one_cell():
    """9^3 points over [0, 8]^3 (h = 1): the only occupied cell is (i, j, k) = (3, 4, 5), x in [3, 4).  N = 16, near 0, far 1, so
    t_i = i / 16 and a ray o + t d with d = (7, 0, 0) has its fence posts at x_i = o_x + 0.4375 i.  Frustum i covers
    [x_i - rho, x_{i+1} + rho] with rho = radius * t_{i+1}; it hits iff floor of the low end is <= 3 and floor of the high end is >= 3."""
    dims, lo, hi = (9, 9, 9), (0.0,) * 3, (8.0,) * 3
    occ = np.zeros((8, 8, 8), bool)
    occ[5, 4, 3] = True

    def run(o, d, radius=1e-4, **kw):
        o, d = np.asarray([o], np.float64), np.asarray([d], np.float64)
        live, first, last = sx.span(occ, dims, lo, hi, o, d, np.full((1, 1), radius), np.zeros((1, 1)), np.ones((1, 1)), 16, **kw)
        assert bool(live[0]) == bool(fx.classify(occ, dims, lo, hi, o, d, np.full((1, 1), radius), np.zeros((1, 1)), np.ones((1, 1)), 16, **kw)[0])
        return bool(live[0]), int(first[0]), int(last[0])
    # x_i = 0.5 + 0.4375 i: x_5 = 2.6875 (+ rho < 3), x_6 = 3.125 -> the first frustum whose high end reaches 3 is i = 5;
    # x_8 = 4.0 exactly: with rho = 1e-4 * 9 / 16 its low end 4 - rho is still in cell 3 -> last = 8; x_9 = 4.4375 is past the cell
    assert run((0.5, 4.5, 5.5), (7.0, 0, 0)) == (True, 5, 8)
    # a ray of zero width: frustum 8 starts at 4.0, which is cell 4 -> last = 7: the widening by rho is what made it 8
    assert run((0.5, 4.5, 5.5), (7.0, 0, 0), radius=0.0) == (True, 5, 7)
    # radius 1: rho = (i + 1) / 16.  High end 0.5 + 0.5 (i + 1) >= 3 from i = 4; low end 0.4375 + 0.375 i < 4 up to i = 9 (3.8125; i = 10: 4.1875)
    assert run((0.5, 4.5, 5.5), (7.0, 0, 0), radius=1.0, outside_occupied=False) == (True, 4, 9)
    # ... and that wide a cone leaves the grid at its far end: high end 0.5 + 0.5 (i + 1) >= 8 from i = 14, which counts when outside is occupied
    assert run((0.5, 4.5, 5.5), (7.0, 0, 0), radius=1.0, outside_occupied=True) == (True, 4, 15)
    # the same cone scaled down to nothing is the zero-width ray
    assert run((0.5, 4.5, 5.5), (7.0, 0, 0), radius=1.0, cone_scale=0.0) == (True, 5, 7)
    # towards -x from 7.5: x_i = 7.5 - 0.4375 i; x_8 = 4.0 (- rho: cell 3) -> first = 7; x_10 = 3.125, x_11 = 2.6875 (+ rho < 3) -> last = 10
    assert run((7.5, 4.5, 5.5), (-7.0, 0, 0)) == (True, 7, 10)
    # one row beside the cell: dead, first = N, last = -1
    assert run((0.5, 5.5, 5.5), (7.0, 0, 0)) == (False, 16, -1)
    # a ray that stops inside the cell: x_16 = 3.5 -> the span runs to the last frustum
    assert run((0.5, 4.5, 5.5), (3.0, 0, 0)) == (True, 13, 15)          # 0.5 + 0.1875 i >= 3 from fence post 14: frustum 13
    # a ray that leaves the grid: x_i = 0.5 + 0.5625 i passes 8 (cell index 8 > 7) at fence post 14 (8.375; x_13 = 7.8125): frusta 13 .. 15
    assert run((0.5, 0.5, 0.5), (9.0, 0, 0), outside_occupied=True) == (True, 13, 15)
    assert run((0.5, 0.5, 0.5), (9.0, 0, 0), outside_occupied=False) == (False, 16, -1)
    # a ray that starts outside the box: x_i = -1.5 + 0.5 i; x_3 = 0 (- rho < 0): frusta 0 .. 3 reach outside; the cell is met by the high
    # end from fence post 9 (3.0): frustum 8, and by the low end up to x_11 = 4.0 (- rho): frustum 11
    assert run((-1.5, 4.5, 5.5), (8.0, 0, 0), outside_occupied=True) == (True, 0, 11)
    assert run((-1.5, 4.5, 5.5), (8.0, 0, 0), outside_occupied=False) == (True, 8, 11)
    # the margin moves the answer where an interval ends 5e-4 h past a face.  radius 0.1: rho = 0.00625 (i + 1); from o_x = 0.1255 the low
    # end of frustum 9 is 0.1255 + 0.4375 * 9 - 0.0625 = 4.0005: cell 4, may-hit with the margin 1e-3 h, not must-hit.  The high end
    # 0.1255 + 0.44375 (i + 1) reaches 3 at i = 6 (3.23; i = 5: 2.79) whatever the margin
    assert run((0.1255, 4.5, 5.5), (7.0, 0, 0), radius=0.1) == (True, 6, 8)
    assert run((0.1255, 4.5, 5.5), (7.0, 0, 0), radius=0.1, margin=1e-3) == (True, 6, 9)
    assert run((0.1255, 4.5, 5.5), (7.0, 0, 0), radius=0.1, margin=-1e-3) == (True, 6, 8)


def test_span_of_a_hit_matrix():
    hit = np.zeros((5, 7), bool)
    hit[0, 3] = True
    hit[1, [0, 6]] = True
    hit[2, :] = True
    hit[4, [2, 3, 5]] = True
    live, first, last = sx.span_of(hit)
    assert live.tolist() == [True, True, True, False, True]
    assert first.tolist() == [3, 0, 0, 7, 2] and last.tolist() == [3, 6, 6, -1, 5]
    assert sx.span_share(first, last, 7) == pytest.approx((1 + 7 + 7 + 4) / 4.0 / 7.0)
    assert np.isnan(sx.span_share(np.array([7]), np.array([-1]), 7))


# ---- one statement of the rules ----------------------------------------------------------------------------------------------
def _squash(s):
    return re.sub(r"[\s*]+", " ", s)


def test_header_binding_and_docstrings_agree_on_the_span_rules():
    from mipnerf_pl_amd import _lib as L
    from mipnerf_pl_amd import model, ops
    hdr = open(os.path.join(REPO, "include", "mipnerf_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\bmipnerf_ray_span\s*\(", code) and "mipnerf_ray_span" in L.SIGNATURES
    assert len(L.SIGNATURES["mipnerf_ray_span"][1]) == len(L.SIGNATURES["mipnerf_ray_occupancy"][1]) + 4
    proto = re.search(r"int mipnerf_ray_span\(([^)]*)\)", code).group(1)
    assert len(proto.split(",")) == len(L.SIGNATURES["mipnerf_ray_span"][1]) == 16
    # after mipnerf_ray_occupancy's rules, before the compaction's
    assert hdr.index("mipnerf_ray_occupancy: live") < hdr.index("mipnerf_ray_span: the occupied span") < hdr.index("mipnerf_compact_rays: an exclusive scan")
    h = _squash(hdr)
    for name, doc in (("ops.ray_span", ops.ray_span.__doc__), ("CulledFrame", model.CulledFrame.__doc__)):
        d = _squash(doc)
        for phrase in ["first = the smallest hitting frustum index, last = the largest", "near' = t_first and far' = t_{last + 1}",
                       "first = N, last = -1, near' = near and far' = far", "cells whose 8 lattice corners are at or below the threshold, after dilation",
                       "frusta cover [near, far] for any N", "NOT"]:
            assert phrase in h, phrase
            assert phrase in d, (name, phrase)
    assert "byte for byte" in h and "byte for byte" in _squash(ops.ray_span.__doc__)
    assert "may each be NULL" in h and "Does not allocate or synchronise" in h[h.index("mipnerf_ray_span: the occupied span"):h.index("mipnerf_compact_rays: an exclusive scan")]
    doc = _squash(model.CulledFrame.__doc__)
    assert "span_samples" in doc and "tighten=True" in doc and "span_share" in doc and "original near" in doc
    import inspect
    sig = inspect.signature(model.CulledFrame.__init__)
    assert sig.parameters["tighten"].default is False and sig.parameters["span_samples"].default is None
    sig = inspect.signature(ops.ray_span)
    assert [sig.parameters[k].default for k in ("disparity", "outside_occupied", "cone_scale", "out")] == [False, True, 1.0, None]


def test_ray_span_validates_its_arguments_without_a_gpu():
    import ctypes as C
    from mipnerf_pl_amd import _lib as L
    lib = L.lib()
    dims, lo, hi = (C.c_int32 * 3)(8, 8, 8), (C.c_float * 3)(-1, -1, -1), (C.c_float * 3)(1, 1, 1)
    rp = L.RaysPtrs()
    tail = (16, 16, 16, 16, 16, None)
    assert lib.mipnerf_ray_span(dims, lo, hi, 16, 4, 0, C.byref(rp), 0, 1, 1.0, *tail) == L.E_INVALID and "ray_span" in L.last_error()
    assert lib.mipnerf_ray_span(dims, lo, hi, 16, 4, L.MAX_SAMPLES + 1, C.byref(rp), 0, 1, 1.0, *tail) == L.E_INVALID
    assert lib.mipnerf_ray_span(dims, hi, lo, 16, 4, 64, C.byref(rp), 0, 1, 1.0, *tail) == L.E_INVALID and "hi > lo" in L.last_error()
    assert lib.mipnerf_ray_span(dims, lo, hi, 16, 4, 64, C.byref(rp), 0, 1, 1.0, *tail) == L.E_INVALID and "null" in L.last_error()
    assert lib.mipnerf_ray_span(dims, lo, hi, 16, 4, 64, None, 0, 1, 1.0, *tail) == L.E_INVALID
    assert lib.mipnerf_ray_span(dims, lo, hi, 16, -1, 64, C.byref(rp), 0, 1, 1.0, *tail) == L.E_INVALID
    assert lib.mipnerf_ray_span(dims, lo, hi, 16, 4, 64, C.byref(rp), 0, 1, float("nan"), *tail) == L.E_INVALID and "cone_scale" in L.last_error()
    bad = (C.c_int32 * 3)(1, 8, 8)
    assert lib.mipnerf_ray_span(bad, lo, hi, 16, 4, 64, C.byref(rp), 0, 1, 1.0, *tail) == L.E_INVALID
    # zero rays: nothing to do, whatever the pointers
    assert lib.mipnerf_ray_span(dims, lo, hi, 16, 0, 64, C.byref(rp), 0, 1, 1.0, None, None, None, None, None, None) == L.OK
    assert lib.mipnerf_ray_span(dims, lo, hi, None, 0, 64, None, 0, 1, 1.0, None, None, None, None, None, None) == L.OK


# ---- command line ------------------------------------------------------------------------------------------------------------
def test_tighten_flags_and_their_defaults_on_both_command_lines():
    from mipnerf_pl_amd import eval as eval_cli
    from mipnerf_pl_amd import render_video
    for parser in (eval_cli.build_parser(), render_video.build_parser()):
        a = parser.parse_args(["--out_dir", "o", "--scale", "1"])
        assert a.cull_tighten is False and a.render_samples is None and a.cull_span_samples is None and a.cull is False
        a = parser.parse_args(["--out_dir", "o", "--scale", "1", "--cull", "--cull_tighten", "--render_samples", "64", "--cull_span_samples", "96"])
        assert a.cull is True and a.cull_tighten is True and a.render_samples == 64 and a.cull_span_samples == 96
        text = _squash(parser.format_help())
        assert "--cull_tighten" in text and "--render_samples" in text and "--cull_span_samples" in text
        assert "Not the untightened frame" in text


def test_cull_tighten_without_cull_is_refused_before_anything_is_loaded(tmp_path):
    from mipnerf_pl_amd import eval as eval_cli
    from mipnerf_pl_amd import render_video
    missing = str(tmp_path / "no_such.ckpt")               # never opened: the refusal comes first
    with pytest.raises(SystemExit, match="--cull_tighten.*--cull"):
        eval_cli.main(["--ckpt", missing, "--data", str(tmp_path), "--out_dir", str(tmp_path / "o"), "--scale", "1", "--cull_tighten"])
    with pytest.raises(SystemExit, match="--cull_tighten.*--cull"):
        render_video.main(["--ckpt", missing, "--out_dir", str(tmp_path / "o"), "--scale", "1", "--cull_tighten"])
    assert not os.path.exists(str(tmp_path / "o"))
    from types import SimpleNamespace
    render_video.refuse_tighten_without_cull(SimpleNamespace(cull=True, cull_tighten=True))
    render_video.refuse_tighten_without_cull(SimpleNamespace(cull=False, cull_tighten=False))


def test_span_samples_stay_the_checkpoints_when_the_render_count_changes():
    from types import SimpleNamespace
    from mipnerf_pl_amd import render_video
    system = SimpleNamespace(hparams={"nerf.num_samples": 64}, checkpoint_num_samples=128)        # rebuilt with --render_samples 64
    assert render_video.cli_span_samples(SimpleNamespace(cull_span_samples=None), system) == 128
    assert render_video.cli_span_samples(SimpleNamespace(cull_span_samples=96), system) == 96
    plain = SimpleNamespace(hparams={"nerf.num_samples": 128})
    assert render_video.cli_span_samples(SimpleNamespace(cull_span_samples=None), plain) == 128


def test_render_samples_rebuilds_the_system_with_the_same_parameters(tmp_path):
    import torch
    from mipnerf_pl_amd import render_video
    from mipnerf_pl_amd.system import DEFAULT_HPARAMS, MipNeRFSystem
    hp = dict(DEFAULT_HPARAMS)
    hp.update({"nerf.num_samples": 32, "exp_name": "cli", "val.batch_type": "single_image", "dataset_name": "blender"})
    torch.manual_seed(0)
    ckpt = str(tmp_path / "last.ckpt")
    MipNeRFSystem(hp, precision="fp32").save_checkpoint(ckpt)
    parser = render_video.build_parser()
    same = render_video.load_system(parser.parse_args(["--ckpt", ckpt, "--out_dir", "o", "--scale", "1"]))
    other = render_video.load_system(parser.parse_args(["--ckpt", ckpt, "--out_dir", "o", "--scale", "1", "--render_samples", "16"]))
    assert same.mip_nerf.num_samples == 32 and same.checkpoint_num_samples == 32
    assert other.mip_nerf.num_samples == 16 and other.checkpoint_num_samples == 32 and other.hparams["nerf.num_samples"] == 16
    a, b = same.state_dict(), other.state_dict()
    assert a.keys() == b.keys() and all(torch.equal(a[k], b[k]) for k in a)
