"""CPU (no GPU): the brute-force fixture of the occupancy rules against first principles on tiny grids, the agreement of the header, the
binding and the docstrings on those rules, the command-line flags and the corner-ray bound of the default box."""
import os
import re

import numpy as np
import pytest
import torch

import occupancy_fixture as fx

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRY_POINTS = ["mipnerf_occupancy_words", "mipnerf_occupancy_build", "mipnerf_ray_occupancy", "mipnerf_compact_rays_workspace_bytes",
                    "mipnerf_compact_rays", "mipnerf_scatter_frame"]


# ---- the fixture from first principles ------------------------------------------------------------------------------------
def test_a_single_hot_corner_occupies_exactly_the_cells_that_touch_it():
    for point in [(2, 3, 1), (0, 0, 0), (4, 5, 6), (0, 3, 6)]:          # (k, j, i): interior, two corners of the lattice, an edge
        lat = np.zeros((5, 6, 7), np.float32)
        lat[point] = 1.0
        occ = fx.raw_occupied(lat, 0.5)
        assert occ.shape == (4, 5, 6)
        want = set()
        for k in range(4):
            for j in range(5):
                for i in range(6):
                    if point[0] in (k, k + 1) and point[1] in (j, j + 1) and point[2] in (i, i + 1):
                        want.add((k, j, i))
        assert set(map(tuple, np.argwhere(occ))) == want and 1 <= len(want) <= 8
    # a value equal to the threshold is not occupied, NaN is, -inf is not, +inf is
    lat = np.zeros((3, 3, 3), np.float32)
    lat[1, 1, 1] = 0.5
    assert not fx.raw_occupied(lat, 0.5).any()
    for v, want in ((np.nan, True), (np.inf, True), (-np.inf, False)):
        lat[1, 1, 1] = v
        assert fx.raw_occupied(lat, 0.5).all() == want and fx.raw_occupied(lat, 0.5).any() == want


@pytest.mark.parametrize("d", [0, 1, 2, 3])
def test_dilation_reaches_chebyshev_distance_d_and_no_further(d):
    occ = np.zeros((9, 8, 11), bool)
    seeds = [(4, 4, 5), (0, 7, 10)]
    for s in seeds:
        occ[s] = True
    got = fx.dilate(occ, d)
    kk, jj, ii = np.meshgrid(np.arange(9), np.arange(8), np.arange(11), indexing="ij")
    want = np.zeros_like(occ)
    for s in seeds:
        want |= np.maximum(np.maximum(np.abs(kk - s[0]), np.abs(jj - s[1])), np.abs(ii - s[2])) <= d
    assert np.array_equal(got, want)
    assert got.sum() == want.sum() and (d == 0) == np.array_equal(got, occ)


def test_packing_is_bit_i_and_31_of_word_i_shift_5_with_zero_padding():
    rng = np.random.default_rng(0)
    for cx in (1, 5, 31, 32, 33, 64, 70):
        occ = rng.random((2, 3, cx)) < 0.5
        words = fx.pack(occ)
        assert words.dtype == np.uint32 and words.shape == (2, 3, (cx + 31) // 32)
        for i in range(cx):
            assert np.array_equal((words[:, :, i >> 5] >> np.uint32(i & 31)) & 1, occ[:, :, i])
        assert np.unpackbits(words.view(np.uint8)).sum() == occ.sum()             # nothing in the padding
        assert np.array_equal(fx.unpack(words, cx), occ)
    one = np.zeros((1, 1, 40), bool)
    one[0, 0, 33] = True
    assert fx.pack(one).tolist() == [[[0, 2]]]


def test_classification_of_axis_aligned_rays_through_one_cell():
    """9^3 points over [0, 8]^3 (h = 1): the only occupied cell is (i, j, k) = (3, 4, 5); rays along +x with a tiny radius"""
    dims, lo, hi = (9, 9, 9), (0.0,) * 3, (8.0,) * 3
    occ = np.zeros((8, 8, 8), bool)
    occ[5, 4, 3] = True
    def run(o, d, near=0.0, far=1.0, **kw):
        o, d = np.asarray([o], np.float64), np.asarray([d], np.float64)
        return bool(fx.classify(occ, dims, lo, hi, o, d, np.full((1, 1), 1e-4), np.full((1, 1), near), np.full((1, 1), far), 16, **kw)[0])
    assert run((0.5, 4.5, 5.5), (7.0, 0, 0))                         # through the cell
    assert not run((0.5, 5.5, 5.5), (7.0, 0, 0))                     # one row beside it
    assert not run((0.5, 4.5, 5.5), (2.0, 0, 0))                     # stops at x = 2.5, short of the cell
    assert run((0.5, 4.5, 5.5), (2.6, 0, 0))                         # reaches x = 3.1
    assert not run((4.5, 4.5, 5.5), (3.0, 0, 0))                     # starts past it
    # the cone widens the box: rho = radius * t reaches the cell from the row beside it
    o, d = np.asarray([[0.5, 5.5, 5.5]]), np.asarray([[7.0, 0.0, 0.0]])
    wide = fx.classify(occ, dims, lo, hi, o, d, np.full((1, 1), 2.0), np.zeros((1, 1)), np.ones((1, 1)), 16)
    assert wide[0]
    assert not fx.classify(occ, dims, lo, hi, o, d, np.full((1, 1), 2.0), np.zeros((1, 1)), np.ones((1, 1)), 16, cone_scale=1e-4)[0]
    # a ray that leaves the grid: occupied outside or clipped away
    assert run((0.5, 0.5, 0.5), (9.0, 0, 0), outside_occupied=True)
    assert not run((0.5, 0.5, 0.5), (9.0, 0, 0), outside_occupied=False)
    assert not run((0.5, 0.5, 0.5), (7.0, 0, 0), outside_occupied=True)        # stays inside (x <= 7.5): nothing occupied on its way
    # the margin: a ray 5e-4 h below the face y = 5 of the cell's row is may-live, not must-live
    assert run((0.5, 5.0005, 5.5), (7.0, 0, 0), margin=1e-3) and not run((0.5, 5.0005, 5.5), (7.0, 0, 0), margin=-1e-3)
    t = fx.fence_posts([2.0], [6.0], 4)
    assert np.array_equal(t, [[2.0, 3.0, 4.0, 5.0, 6.0]])
    assert np.allclose(fx.fence_posts([2.0], [6.0], 2, disparity=True), [[2.0, 3.0, 6.0]])


def test_compaction_and_scatter_fixture():
    live = np.array([0, 1, 1, 0, 1], np.uint8)
    rays = [np.arange(15, dtype=np.float32).reshape(5, 3), np.arange(5, dtype=np.float32).reshape(5, 1)]
    idx, (a, b) = fx.compact(live, rays)
    assert idx.tolist() == [1, 2, 4] and a.tolist() == [[3, 4, 5], [6, 7, 8], [12, 13, 14]] and b.ravel().tolist() == [1, 2, 4]
    comp = [(np.full((3, 3), 0.25, np.float32), np.array([7, 8, 9], np.float32), np.array([.5, .6, .7], np.float32))]
    (rgb, dist, acc), = fx.scatter(idx, comp, 5, live, np.full((5, 1), 2.0, np.float32), True)
    assert rgb[:, 0].tolist() == [1, .25, .25, 1, .25] and dist.tolist() == [2, 7, 8, 2, 9] and np.allclose(acc, [0, .5, .6, 0, .7])
    (rgb, _, _), = fx.scatter(idx, comp, 5, live, np.full((5, 1), 2.0, np.float32), False)
    assert rgb[:, 2].tolist() == [0, .25, .25, 0, .25]


# ---- one statement of the rules ----------------------------------------------------------------------------------------------
def _squash(s):
    return re.sub(r"[\s*]+", " ", s)


def test_header_binding_build_and_docstrings_agree():
    from mipnerf_pl_amd import _lib as L
    from mipnerf_pl_amd import build, model, ops
    hdr = open(os.path.join(REPO, "include", "mipnerf_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NEW_ENTRY_POINTS:
        assert re.search(r"\b" + name + r"\s*\(", code), name
        assert name in L.SIGNATURES, name
    assert ("kernels_occupancy.hip", ["-ffp-contract=off"]) in build.UNITS
    h = _squash(hdr)
    docs = _squash(" ".join([ops.Occupancy.__doc__, ops.occupancy_grid.__doc__, ops.ray_occupancy.__doc__, ops.compact_rays.__doc__,
                             ops.scatter_frame.__doc__, model.CulledFrame.__doc__]))
    # the rules, word for word where both state them
    for phrase in ["bit i & 31 of word i >> 5", "Chebyshev distance", "> threshold or is NaN", "p0 = o + t_i d", "p1 = o + t_{i+1} d",
                   "rho = cone_scale radii t_{i+1}", "floor((x - lo) / h)", "all-zero weights"]:
        assert phrase in h, phrase
        assert phrase in docs, phrase
    assert "[nz - 1, ny - 1, ceil((nx - 1) / 32)]" in h and "[nz - 1, ny - 1, ceil((nx - 1) / 32)]" in docs
    assert "padding bits are 0" in h and "padding bits are 0" in docs
    assert "8-byte read-back" in h and "8-byte read-back" in docs and "cannot be captured" in h
    assert "acc = 0" in h and "distance = near" in h and "acc = 0" in docs and "distance = near" in docs
    # the word count the header states is the one the library computes (host-only call)
    lib = L.lib()
    for nx, ny, nz in [(2, 2, 2), (33, 5, 4), (34, 5, 4), (65, 3, 3), (128, 128, 128)]:
        assert lib.mipnerf_occupancy_words(nx, ny, nz) == (nz - 1) * (ny - 1) * ((nx - 1 + 31) // 32)
    assert lib.mipnerf_occupancy_words(1, 5, 5) == 0 and lib.mipnerf_occupancy_words(1024, 1024, 1024) == 0
    assert lib.mipnerf_compact_rays_workspace_bytes(-1) == 0 and lib.mipnerf_compact_rays_workspace_bytes(640000) >= 256 + 4 * 625


def test_entry_points_validate_their_arguments_without_a_gpu():
    import ctypes as C
    from mipnerf_pl_amd import _lib as L
    lib = L.lib()
    dims, lo, hi = (C.c_int32 * 3)(8, 8, 8), (C.c_float * 3)(-1, -1, -1), (C.c_float * 3)(1, 1, 1)
    assert lib.mipnerf_occupancy_build(dims, None, 0.5, 0, None, None, None) == L.E_INVALID
    assert lib.mipnerf_occupancy_build(dims, 16, 0.5, -1, 16, None, None) == L.E_INVALID and "dilate" in L.last_error()
    assert lib.mipnerf_occupancy_build(dims, 16, 0.5, 1, 16, None, None) == L.E_INVALID and "scratch" in L.last_error()
    assert lib.mipnerf_occupancy_build(dims, 16, float("nan"), 0, 16, None, None) == L.E_INVALID
    rp = L.RaysPtrs()
    assert lib.mipnerf_ray_occupancy(dims, lo, hi, 16, 4, 0, C.byref(rp), 0, 1, 1.0, 16, None) == L.E_INVALID
    assert lib.mipnerf_ray_occupancy(dims, lo, hi, 16, 4, L.MAX_SAMPLES + 1, C.byref(rp), 0, 1, 1.0, 16, None) == L.E_INVALID
    assert lib.mipnerf_ray_occupancy(dims, hi, lo, 16, 4, 64, C.byref(rp), 0, 1, 1.0, 16, None) == L.E_INVALID and "hi > lo" in L.last_error()
    assert lib.mipnerf_ray_occupancy(dims, lo, hi, 16, 4, 64, C.byref(rp), 0, 1, 1.0, 16, None) == L.E_INVALID        # null ray fields
    assert lib.mipnerf_ray_occupancy(dims, lo, hi, 16, 0, 64, C.byref(rp), 0, 1, 1.0, None, None) == L.OK             # zero rays: nothing to do
    count = C.c_int64(7)
    assert lib.mipnerf_compact_rays(0, None, None, None, None, None, 0, C.byref(count), None) == L.OK and count.value == 0
    assert lib.mipnerf_compact_rays(4, None, None, None, None, None, 0, C.byref(count), None) == L.E_INVALID
    assert lib.mipnerf_scatter_frame(4, 5, 2, None, None, None, 1, None, None, None) == L.E_INVALID                   # count > n
    assert lib.mipnerf_scatter_frame(4, 0, 9, None, None, None, 1, None, None, None) == L.E_INVALID and "num_levels" in L.last_error()
    assert lib.mipnerf_scatter_frame(0, 0, 2, None, None, None, 1, None, None, None) == L.OK


# ---- command line ------------------------------------------------------------------------------------------------------------
def test_cull_flags_and_their_defaults_on_both_command_lines():
    from mipnerf_pl_amd import eval as eval_cli
    from mipnerf_pl_amd import render_video
    for parser, extra in ((eval_cli.build_parser(), ["--scale", "1"]), (render_video.build_parser(), ["--scale", "1"])):
        a = parser.parse_args(["--out_dir", "o"] + extra)
        assert a.cull is False and a.cull_grid == 128 and a.cull_threshold == 0.01 and a.cull_dilate == 1 and a.cull_bound is None
        a = parser.parse_args(["--out_dir", "o", "--cull", "--cull_grid", "64", "--cull_threshold", "0.1", "--cull_dilate", "0", "--cull_bound", "4.5"] + extra)
        assert a.cull is True and (a.cull_grid, a.cull_threshold, a.cull_dilate, a.cull_bound) == (64, 0.1, 0, 4.5)
        assert "scene dependent" in parser.format_help()
    # without --cull no occupancy is built, whatever the other flags say
    a = render_video.build_parser().parse_args(["--out_dir", "o", "--scale", "1", "--cull_grid", "8"])
    assert render_video.cli_occupancy(a, None, None) is None


def test_cull_refuses_the_unbounded_model():
    from types import SimpleNamespace
    from mipnerf_pl_amd import render_video
    from mipnerf_pl_amd.evaluate import scene_occupancy
    unbounded = SimpleNamespace(mip_nerf=SimpleNamespace(unbounded=True))
    bounded = SimpleNamespace(mip_nerf=SimpleNamespace(unbounded=False))
    with pytest.raises(SystemExit, match="unbounded"):
        render_video.refuse_unbounded_cull(SimpleNamespace(cull=True), unbounded)
    render_video.refuse_unbounded_cull(SimpleNamespace(cull=False), unbounded)
    render_video.refuse_unbounded_cull(SimpleNamespace(cull=True), bounded)
    with pytest.raises(NotImplementedError, match="unbounded"):
        scene_occupancy(unbounded, bound=1.0)


def _pinhole_rays(pose, focal, w, h, near, far):
    """Blender-style pinhole rays of one camera, [h, w, k] float32 tensors (pixel centres, -z forward)"""
    from mipnerf_pl_amd import Rays
    x, y = np.meshgrid(np.arange(w, dtype=np.float32) + .5, np.arange(h, dtype=np.float32) + .5, indexing="xy")
    cam = np.stack([(x - w * .5) / focal, -(y - h * .5) / focal, -np.ones_like(x)], -1)
    d = (cam @ pose[:3, :3].T).astype(np.float32)
    o = np.broadcast_to(pose[:3, 3].astype(np.float32), d.shape).copy()
    v = d / np.linalg.norm(d, axis=-1, keepdims=True)
    one = np.ones_like(d[..., :1])
    return Rays(*[torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)) for a in (o, d, v, 1e-3 * one, one, near * one, far * one)])


def test_corner_ray_bound_against_all_pixels():
    from mipnerf_pl_amd.evaluate import corner_ray_bound, cull_box
    rng = np.random.default_rng(3)
    frames = []
    for _ in range(5):
        q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        pose = np.concatenate([q, rng.uniform(-4, 4, (3, 1))], 1)
        frames.append(_pinhole_rays(pose, focal=rng.uniform(10, 30), w=13, h=9, near=rng.uniform(0.5, 2.0), far=rng.uniform(5.0, 7.0)))
    brute = 0.0
    for r in frames:
        for t in (r.near, r.far):
            brute = max(brute, float((r.origins.double() + t.double() * r.directions.double()).abs().max()))
    got = corner_ray_bound(frames)
    assert got == pytest.approx(brute, rel=1e-6)           # the corner pixels are pixels: the maximum over all of them is a corner's
    # one frame at a time, too: no pixel's end point lies past its own frame's corners
    for r in frames:
        b = corner_ray_bound([r])
        for t in (r.near, r.far):
            assert float((r.origins + t * r.directions).abs().max()) <= b * (1 + 1e-6)
    # plus one cell of the box itself: B = B0 + 2 B / (grid - 1)
    B = cull_box(frames, 128)
    assert B == pytest.approx(got + 2 * B / 127, rel=1e-12) and B > got
    with pytest.raises(ValueError):
        cull_box(frames, 3)
