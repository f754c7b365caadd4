"""CPU (no GPU): empty-space skipping for the unbounded-scene model in the contracted space -- the bounding rule of include/mipnerf_hip.h
(mipnerf_ray_occupancy_360) as tests/cull360_fixture.py restates it in float64 and as csrc/raymath360.hpp states it for host and device
(built with g++ -ffp-contract=off), the shared inverse-depth fence posts, the new entry points' bindings and argument checks, and the
command-line flags and refusals that need no device.

Ray sets: 600 rays spread evenly over tests/golden/scene360_rays.npz and the 600 adversarial rays of cull360_fixture.adversarial_rays
(origins 0.01 .. 3 from the centre, 100 aimed through the centre, near 0.05, far 1e4); N = 64 and 128; cone_scale 1 and 8.

Bounds.  (a) none: a sampled point of a frustum, contracted in float64, lies inside the float64 box, with no allowance, and inside the
fp32 host build's box to the bound of (b).  (b) 16 fp32 ulps of 2 (the largest contracted coordinate), 16 * 2^-22 = 3.8e-6, on every bound
of every frustum; measured 1.4 to 6.2 ulps.  The rule has one discontinuity, the case rmin >= 1: a frustum whose float64 rmin lies within
1e-5 of 1 (fp32 rounding of |o + tc d| - rho is about 1e-7 there) may take either case in fp32, and is held to the fixture's box of one
of the two.  (c) bit for bit."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import cull360_fixture as cx

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
SRC = os.path.join(HERE, "hostmath", "cullbox360.cpp")
SO = os.path.join(HERE, "hostmath", "_cullbox360.so")
ULP2 = 2.0 ** -22                       # the fp32 spacing in [2, 4)
NEW_ENTRY_POINTS = ("mipnerf_ray_occupancy_360", "mipnerf_ray_span_360")


def golden(name):
    return np.load(os.path.join(HERE, "golden", name + ".npz"))


def ray_set(name):
    if name == "golden":
        g = golden("scene360_rays")
        idx = np.linspace(0, g["rays_origins"].shape[0] - 1, 600).astype(np.int64)
        return tuple(np.ascontiguousarray(g["rays_" + k][idx], np.float32) for k in ("origins", "directions", "radii", "near", "far"))
    return cx.adversarial_rays()


@pytest.fixture(scope="module")
def cb():
    hdrs = [os.path.join(REPO, "mipnerf_pl_amd", "csrc", h) for h in ("raymath.hpp", "raymath360.hpp")]
    if (not os.path.exists(SO)) or os.path.getmtime(SO) < max(os.path.getmtime(f) for f in [SRC] + hdrs):
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", SRC, "-o", SO])
    return C.CDLL(SO)


def p(a):
    return a.ctypes.data_as(C.c_void_p)


CASES = [(name, N, cs) for name in ("golden", "adversarial") for N in (64, 128) for cs in (1.0, 8.0)]


# ---- (a) the rule is conservative -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,N,cone_scale", CASES)
def test_no_contracted_point_of_a_frustum_leaves_its_box(cb, name, N, cone_scale):
    o, d, r, near, far = ray_set(name)
    assert len(o) == 600
    got_lo, got_hi = np.empty((600, N, 3), np.float32), np.empty((600, N, 3), np.float32)
    cb.cb_boxes(600, N, p(o), p(d), p(r), p(near), p(far), C.c_float(cone_scale), p(got_lo), p(got_hi))
    if name == "adversarial":
        assert (np.abs(np.cross(o[::6].astype(np.float64), d[::6].astype(np.float64))).max(axis=1) < 1e-6).sum() == 100      # through the centre
    t = cx.fence_posts(near, far, N)
    lo, hi, rmin = cx.frustum_box(t[:, :-1], t[:, 1:], o, d, r, cone_scale)
    assert np.isfinite(lo).all() and np.isfinite(hi).all() and (lo <= hi).all()
    assert (rmin >= 1).any() and (rmin < 1).any()                                      # both cases of the rule are there
    rng = np.random.default_rng(N + int(cone_scale))
    worst = worst32 = -np.inf
    for c0 in range(0, len(o), 100):
        sl = slice(c0, c0 + 100)
        z = cx.contract(cx.sample_frusta(t[sl, :-1], t[sl, 1:], o[sl], d[sl], r[sl], cone_scale, 400, rng))       # [100, N, 400, 3]
        worst = max(worst, float((lo[sl][:, :, None, :] - z).max()), float((z - hi[sl][:, :, None, :]).max()))
        worst32 = max(worst32, float((got_lo[sl][:, :, None, :] - z).max()), float((z - got_hi[sl][:, :, None, :]).max()))
    print(f"cull360 rule {name} N {N} cone_scale {cone_scale}: worst slack {worst:.3e} (negative: inside); of the fp32 host build {worst32:.3e}")
    assert worst <= 0.0
    assert worst32 <= 16 * ULP2                                                        # the fp32 box: the same, to the bound of (b)


# ---- (b) the MIP_HD function is the rule ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,N,cone_scale", CASES)
def test_host_build_of_the_rule_agrees_with_the_fixture(cb, name, N, cone_scale):
    o, d, r, near, far = ray_set(name)
    n = len(o)
    got_lo, got_hi = np.empty((n, N, 3), np.float32), np.empty((n, N, 3), np.float32)
    cb.cb_boxes(n, N, p(o), p(d), p(r), p(near), p(far), C.c_float(cone_scale), p(got_lo), p(got_hi))
    t = cx.fence_posts(near, far, N)
    args = (t[:, :-1], t[:, 1:], o, d, r, cone_scale)
    lo, hi, rmin = cx.frustum_box(*args)
    err = np.maximum(np.abs(got_lo - lo), np.abs(got_hi - hi)).max(axis=-1)            # [n, N]
    edge = np.abs(rmin - 1.0) <= 1e-5
    if edge.any():                                                                     # either case of the rule, whole
        for branch in ("outside", "mixed"):
            blo, bhi, _ = cx.frustum_box(*args, branch=branch)
            other = np.maximum(np.abs(got_lo - blo), np.abs(got_hi - bhi)).max(axis=-1)
            err = np.where(edge, np.minimum(err, other), err)
    print(f"cull360 host build {name} N {N} cone_scale {cone_scale}: max error {err.max() / ULP2:.2f} fp32 ulps of 2; "
          f"{int(edge.sum())} frusta within 1e-5 of the case boundary")
    assert int(edge.sum()) <= 8
    assert err.max() <= 16 * ULP2


def test_host_build_gives_nan_boxes_for_values_that_are_not_finite(cb):
    o = np.array([[np.nan, 0, 0], [0.5, 0, 0], [0.5, 0, 0], [0.5, 0.1, 0]], np.float32)
    d = np.array([[0, 0, 1], [0, np.nan, 1], [0, 0, 1], [0, 0, 1]], np.float32)
    r = np.full((4, 1), 1e-3, np.float32)
    near = np.array([[1], [1], [np.nan], [1]], np.float32)
    far = np.full((4, 1), 10.0, np.float32)
    lo, hi = np.empty((4, 5, 3), np.float32), np.empty((4, 5, 3), np.float32)
    cb.cb_boxes(4, 5, p(o), p(d), p(r), p(near), p(far), C.c_float(1.0), p(lo), p(hi))
    assert np.isnan(lo[:3]).all() and np.isnan(hi[:3]).all()
    assert np.isfinite(lo[3]).all() and np.isfinite(hi[3]).all()
    flo, fhi, _ = cx.frustum_box(*[cx.fence_posts(near, far, 5)[:, s] for s in (slice(0, 5), slice(1, 6))], o, d, r)
    assert np.isnan(flo[:3]).all() and np.isnan(fhi[:3]).all()


# ---- (c) the fence posts are the sampler's ----------------------------------------------------------------------------------------
def test_host_fence_posts_are_the_pinned_ones_bit_for_bit(cb):
    g = golden("pin360_24x64")
    N = int(g["num_samples"])
    near, far = np.ascontiguousarray(g["rays_near"]), np.ascontiguousarray(g["rays_far"])
    n = len(near)
    t_inv, t = np.empty((n, N + 1), np.float32), np.empty((n, N + 1), np.float32)
    cb.cb_fence_posts(n, N, p(near), p(far), p(t_inv), p(t))
    assert g["det_t_inv"].shape == t_inv.shape and t_inv.tobytes() == np.ascontiguousarray(g["det_t_inv"]).tobytes()
    assert t.tobytes() == (np.float32(1.0) / g["det_t_inv"]).astype(np.float32).tobytes()
    assert np.abs(t - cx.fence_posts(near, far, N)).max() <= 4e-7 * float(far.max())


def test_sampler_and_classifiers_share_one_fence_post_function():
    csrc = os.path.join(REPO, "mipnerf_pl_amd", "csrc")
    sampler = open(os.path.join(csrc, "kernels_360.hip")).read()
    body = sampler[sampler.index("k_sample_along_rays_360("):sampler.index("enc360_index")]
    assert "level0_t_inv_360(" in body and "torch_linspace_at" not in body
    occ = open(os.path.join(csrc, "kernels_occupancy.hip")).read()
    assert "level0_t_360(" in occ and "contracted_frustum_box(" in occ
    for k in ("k_ray_occupancy_360", "k_ray_span_360", "k_ray_occupancy", "k_ray_span"):
        assert re.search(r"\b" + k + r"\(", occ), k
    assert occ.count("occ_box_test(") == 2                                             # its definition and the one call


# ---- (d) bindings, argument checks, refusals and command lines --------------------------------------------------------------------
def test_bindings_and_argument_checks_without_a_gpu():
    from mipnerf_pl_amd import _lib as L
    hdr = open(os.path.join(REPO, "include", "mipnerf_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NEW_ENTRY_POINTS:
        assert name in L.SIGNATURES and re.search(r"\b" + name + r"\s*\(", code), name
    # the bounded signatures without `disparity`
    assert len(L.SIGNATURES["mipnerf_ray_occupancy_360"][1]) == len(L.SIGNATURES["mipnerf_ray_occupancy"][1]) - 1 == 11
    assert len(L.SIGNATURES["mipnerf_ray_span_360"][1]) == len(L.SIGNATURES["mipnerf_ray_span"][1]) - 1 == 15
    for name in NEW_ENTRY_POINTS:
        proto = re.search(r"int " + name + r"\(([^)]*)\)", code).group(1)
        assert len(proto.split(",")) == len(L.SIGNATURES[name][1]) and "disparity" not in proto
    assert hdr.index("mipnerf_ray_span: the occupied span") < hdr.index("mipnerf_ray_occupancy_360 / mipnerf_ray_span_360") \
        < hdr.index("mipnerf_compact_rays: an exclusive scan")
    text = re.sub(r"[\s*]+", " ", hdr)
    for phrase in ("rmin = rc - rho", "rmax = max(|p0|, |p1|) + rho", "sag = 1 - sqrt(max(0, (1 + u0.u1) / 2))", "e = sag + rho / rmin",
                   "F = rmax > 1 ? 2 - 1 / rmax : rmax", "There is no disparity argument", "Neither call allocates or synchronises"):
        assert phrase in text, phrase
    lib = L.lib()
    assert lib.mipnerf_abi_version() == 6                                              # the ABI only grows
    dims, lo, hi = (C.c_int32 * 3)(8, 8, 8), (C.c_float * 3)(-2, -2, -2), (C.c_float * 3)(2, 2, 2)
    rp = L.RaysPtrs()
    for name, tail in (("mipnerf_ray_occupancy_360", (16, None)), ("mipnerf_ray_span_360", (16, 16, 16, 16, 16, None))):
        f = getattr(lib, name)
        short = name[len("mipnerf_"):]
        assert f(dims, lo, hi, 16, 4, 0, C.byref(rp), 1, 1.0, *tail) == L.E_INVALID and short in L.last_error()
        assert f(dims, lo, hi, 16, 4, L.MAX_SAMPLES + 1, C.byref(rp), 1, 1.0, *tail) == L.E_INVALID
        assert f(dims, hi, lo, 16, 4, 64, C.byref(rp), 1, 1.0, *tail) == L.E_INVALID and "hi > lo" in L.last_error()
        assert f(dims, lo, hi, 16, 4, 64, C.byref(rp), 1, 1.0, *tail) == L.E_INVALID and "null" in L.last_error()
        assert f(dims, lo, hi, 16, 4, 64, None, 1, 1.0, *tail) == L.E_INVALID
        assert f(dims, lo, hi, 16, -1, 64, C.byref(rp), 1, 1.0, *tail) == L.E_INVALID
        assert f(dims, lo, hi, 16, 4, 64, C.byref(rp), 1, float("nan"), *tail) == L.E_INVALID and "cone_scale" in L.last_error()
        assert f((C.c_int32 * 3)(1, 8, 8), lo, hi, 16, 4, 64, C.byref(rp), 1, 1.0, *tail) == L.E_INVALID
        none = (None,) * len(tail)
        assert f(dims, lo, hi, 16, 0, 64, C.byref(rp), 1, 1.0, *none) == L.OK                 # zero rays: nothing to do, whatever the pointers
        assert f(dims, lo, hi, None, 0, 64, None, 1, 1.0, *none) == L.OK


def test_ops_and_frame_refusals_without_a_gpu():
    import torch
    from mipnerf_pl_amd import MipNerf, Rays, ops
    from mipnerf_pl_amd.model import CulledFrame
    sig = inspect.signature(ops.Occupancy.__init__)
    assert list(sig.parameters)[-1] == "space" and sig.parameters["space"].default is None
    sig = inspect.signature(ops.field_occupancy)
    assert sig.parameters["space"].default is None and "far_radius" in sig.parameters
    unb, bnd = MipNerf(num_samples=8, unbounded=True), MipNerf(num_samples=8)
    with pytest.raises(NotImplementedError, match="unbounded=True models are not supported"):          # as before: no space
        ops.field_occupancy(unb, grid=8, lo=-1.0, hi=1.0)
    with pytest.raises(ValueError, match="a world box cannot hold an unbounded ray"):
        ops.field_occupancy(unb, grid=8, space="world")
    with pytest.raises(ValueError, match="unbounded=True"):                                            # a bounded model and a space
        ops.field_occupancy(bnd, grid=8, space="contracted")
    with pytest.raises(ValueError, match="far_radius"):
        ops.field_occupancy(unb, grid=8, space="contracted", far_radius=1.0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):                                         # on the host: past the checks, no further
        ops.field_occupancy(unb, grid=8, space="contracted", far_radius=30.0)
    with pytest.raises(ValueError, match="space"):
        ops.Occupancy(torch.zeros(7, 7, 1, dtype=torch.int32), (8, 8, 8), (-2,) * 3, (2,) * 3, space="world")
    bits = torch.zeros(7, 7, 1, dtype=torch.int32)
    world = ops.Occupancy(bits, (8, 8, 8), (-2,) * 3, (2,) * 3)
    contracted = ops.Occupancy(bits, (8, 8, 8), (-2,) * 3, (2,) * 3, space="contracted")
    assert world.space is None and contracted.space == "contracted"
    rays = Rays(*[torch.zeros(2, k) for k in (3, 3, 3, 1, 1, 1, 1)])
    for f in (ops.ray_occupancy, ops.ray_span):
        with pytest.raises(ValueError, match="disparity"):
            f(contracted, rays, 8, disparity=True)
    dev = torch.device("cpu")
    with pytest.raises(NotImplementedError, match="unbounded=True models are not supported"):
        CulledFrame(unb, 4, 4, True, dev, world)
    with pytest.raises(ValueError, match="contracted space"):
        CulledFrame(bnd, 4, 4, True, dev, contracted)
    for doc in (ops.ray_occupancy.__doc__, ops.ray_span.__doc__, CulledFrame.__doc__, ops.field_occupancy.__doc__):
        assert "contracted" in doc


def test_scene_occupancy_and_the_default_far_radius():
    import torch
    from types import SimpleNamespace
    from mipnerf_pl_amd import Rays
    from mipnerf_pl_amd.evaluate import corner_ray_radius, cull_far_radius, scene_occupancy
    unbounded = SimpleNamespace(mip_nerf=SimpleNamespace(unbounded=True))
    bounded = SimpleNamespace(mip_nerf=SimpleNamespace(unbounded=False))
    with pytest.raises(NotImplementedError, match="unbounded"):
        scene_occupancy(unbounded, bound=1.0)
    with pytest.raises(ValueError, match="bounded model"):
        scene_occupancy(bounded, space="contracted", far_radius=30.0)
    with pytest.raises(ValueError, match="world box"):
        scene_occupancy(unbounded, space="world", far_radius=30.0)
    with pytest.raises(ValueError, match="far_radius"):
        scene_occupancy(unbounded, space="contracted")
    # a pinhole frame: the corner rays reach farthest
    h, w, focal, far = 9, 13, 10.0, 20.0
    ys, xs = torch.meshgrid(torch.arange(h, dtype=torch.float64), torch.arange(w, dtype=torch.float64), indexing="ij")
    d = torch.stack([(xs - w / 2 + 0.5) / focal, -(ys - h / 2 + 0.5) / focal, -torch.ones_like(xs)], -1).float()
    o = torch.tensor([0.3, -2.0, 1.0]).expand(h, w, 3).contiguous()
    one = torch.ones(h, w, 1)
    frame = Rays(o, d, d / d.norm(dim=-1, keepdim=True), 1e-3 * one, one, 0.5 * one, far * one)
    reach = float(torch.maximum((o + far * d).double().norm(dim=-1), (o + 0.5 * d).double().norm(dim=-1)).max())
    assert corner_ray_radius([frame]) == pytest.approx(reach, rel=1e-12)
    assert cull_far_radius([frame], 128) == pytest.approx(reach * 127 / 125, rel=1e-12)
    assert cull_far_radius([frame, frame], 32) == pytest.approx(reach * 31 / 29, rel=1e-12)
    with pytest.raises(ValueError, match="at least 4"):
        cull_far_radius([frame], 3)


def test_cull_space_flags_on_both_command_lines(tmp_path):
    from types import SimpleNamespace
    from mipnerf_pl_amd import eval as eval_cli
    from mipnerf_pl_amd import render_video
    for parser in (eval_cli.build_parser(), render_video.build_parser()):
        a = parser.parse_args(["--out_dir", "o", "--scale", "1"])
        assert a.cull_space is None and a.cull_far_radius is None
        a = parser.parse_args(["--out_dir", "o", "--scale", "1", "--cull", "--cull_space", "contracted", "--cull_far_radius", "30"])
        assert a.cull is True and a.cull_space == "contracted" and a.cull_far_radius == 30.0
        with pytest.raises(SystemExit):
            parser.parse_args(["--out_dir", "o", "--scale", "1", "--cull", "--cull_space", "world"])
        text = re.sub(r"\s+", " ", parser.format_help())
        assert "--cull_space" in text and "--cull_far_radius" in text
    unbounded = SimpleNamespace(mip_nerf=SimpleNamespace(unbounded=True))
    bounded = SimpleNamespace(mip_nerf=SimpleNamespace(unbounded=False))
    with pytest.raises(SystemExit, match=r"unbounded.*--cull_space contracted"):       # the message names the flag
        render_video.refuse_unbounded_cull(SimpleNamespace(cull=True, cull_space=None), unbounded)
    render_video.refuse_unbounded_cull(SimpleNamespace(cull=True, cull_space="contracted"), unbounded)
    render_video.refuse_unbounded_cull(SimpleNamespace(cull=False, cull_space=None), unbounded)
    with pytest.raises(SystemExit, match="bounded model"):
        render_video.refuse_unbounded_cull(SimpleNamespace(cull=True, cull_space="contracted"), bounded)
    # the flags of a grid without --cull: refused before anything is loaded
    missing = str(tmp_path / "no_such.ckpt")
    for extra in (["--cull_space", "contracted"], ["--cull_far_radius", "30"]):
        with pytest.raises(SystemExit, match="--cull"):
            eval_cli.main(["--ckpt", missing, "--data", str(tmp_path), "--out_dir", str(tmp_path / "o"), "--scale", "1"] + extra)
        with pytest.raises(SystemExit, match="--cull"):
            render_video.main(["--ckpt", missing, "--out_dir", str(tmp_path / "o"), "--scale", "1"] + extra)
    with pytest.raises(SystemExit, match="--cull_space contracted"):
        render_video.main(["--ckpt", missing, "--out_dir", str(tmp_path / "o"), "--scale", "1", "--cull", "--cull_far_radius", "30"])
    assert not os.path.exists(str(tmp_path / "o"))
    # without --cull nothing is built; the flags reach scene_occupancy
    assert render_video.cli_occupancy(SimpleNamespace(cull=False), None, None) is None
    seen = {}
    real = render_video.scene_occupancy
    try:
        render_video.scene_occupancy = lambda system, frames, **kw: seen.update(kw, frames=frames) or "occ"
        a = render_video.build_parser().parse_args(["--out_dir", "o", "--scale", "1", "--cull", "--cull_space", "contracted", "--cull_grid", "64"])
        assert render_video.cli_occupancy(a, None, "frames") == "occ"
        assert seen["space"] == "contracted" and seen["far_radius"] is None and seen["frames"] == "frames" and seen["bound"] is None and seen["grid"] == 64
        a = render_video.build_parser().parse_args(["--out_dir", "o", "--scale", "1", "--cull", "--cull_space", "contracted", "--cull_far_radius", "30"])
        render_video.cli_occupancy(a, None, "frames")
        assert seen["far_radius"] == 30.0 and seen["frames"] is None
    finally:
        render_video.scene_occupancy = real
