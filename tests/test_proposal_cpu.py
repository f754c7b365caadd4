"""CPU (no GPU): the density lattice as the proposal level -- the trilinear lookup csrc/lattice_sample.hpp states for host and device
(built with g++ -O2 -ffp-contract=off from tests/hostmath/proposal.cpp) against tests/proposal_fixture.py: bit for bit against the
float32 restatement, within a derived bound against the float64 one; the two new entry points' declarations, bindings, exports and
argument checks without a device; the build unit; the command-line flags and refusals."""
import ctypes as C
import inspect
import os
import re
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import proposal_fixture as px

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
SRC = os.path.join(HERE, "hostmath", "proposal.cpp")
SO = os.path.join(HERE, "hostmath", "_proposal.so")
F = np.float32
LATTICES = [(2, 2, 2), (5, 7, 9), (33, 33, 33)]                      # [nz, ny, nx]
BOXES = {(2, 2, 2): ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)), (5, 7, 9): ((-1.5, -0.7, 0.25), (2.25, 1.3, 4.0)),
         (33, 33, 33): ((-4.1234, -4.1234, -4.1234), (4.1234, 4.1234, 4.1234))}


@pytest.fixture(scope="module")
def hm():
    hdrs = [os.path.join(REPO, "mipnerf_pl_amd", "csrc", h) for h in ("raymath.hpp", "lattice_sample.hpp")]
    if (not os.path.exists(SO)) or os.path.getmtime(SO) < max(os.path.getmtime(f) for f in [SRC] + hdrs):
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", SRC, "-o", SO])
    return C.CDLL(SO)


def host_trilinear(hm, lattice, lo, hi, xyz):
    lat = np.ascontiguousarray(lattice, F)
    nz, ny, nx = lat.shape
    pts = np.ascontiguousarray(xyz, F).reshape(-1, 3)
    lo, hi = np.asarray(lo, F), np.asarray(hi, F)
    out = np.full(pts.shape[0], -7.0, F)
    as_p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    hm.hm_lattice_trilinear(as_p(lat), nx, ny, nz, as_p(lo), as_p(hi), C.c_longlong(pts.shape[0]), as_p(pts), as_p(out))
    return out


def same_bits(a, b):
    """bit for bit, a NaN matching any NaN (its payload is not part of the rule)"""
    a, b = np.asarray(a, F), np.asarray(b, F)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.uint32), b[~nan].view(np.uint32))


# ---- the lookup ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", LATTICES)
def test_host_function_equals_the_float32_restatement_bit_for_bit(hm, shape):
    lo, hi = BOXES[shape]
    lat = px.random_lattice(shape, seed=sum(shape))
    pts = np.concatenate([px.box_points(lo, hi, seed=1), px.nonfinite_points(lo, hi)])
    got, want = host_trilinear(hm, lat, lo, hi, pts), px.trilinear_f32(lat, lo, hi, pts)
    assert same_bits(got, want)
    assert (got >= 0).all()                                          # non-negative corners give a non-negative value
    assert (got[-len(px.nonfinite_points(lo, hi)):] == 0).all()      # a non-finite coordinate gives 0


@pytest.mark.parametrize("shape", LATTICES)
def test_faces_edges_and_corners_take_the_lattice_values(hm, shape):
    """a point ON a lattice point returns that value exactly (f = 0 or f = 1 on every axis), a point outside the box the edge value"""
    lo, hi = BOXES[shape]
    nz, ny, nx = shape
    lat = px.random_lattice(shape, seed=5)
    ends = [(lo[a], hi[a]) for a in range(3)]
    pts = np.array([[x, y, z] for x in ends[0] for y in ends[1] for z in ends[2]], F)
    idx = [(k, j, i) for i in (0, nx - 1) for j in (0, ny - 1) for k in (0, nz - 1)]
    want = np.array([lat[k, j, i] for (k, j, i) in idx], F)
    assert same_bits(host_trilinear(hm, lat, lo, hi, pts), want)
    span = np.asarray(hi, F) - np.asarray(lo, F)
    out = np.where(pts == np.asarray(lo, F), pts - span, pts + span).astype(F)       # beyond the same corners
    assert same_bits(host_trilinear(hm, lat, lo, hi, out), want)


def test_a_nan_in_the_lattice_propagates_and_only_from_its_cells(hm):
    shape = (5, 7, 9)
    lo, hi = BOXES[shape]
    lat = px.random_lattice(shape, seed=3)
    lat[2, 3, 4] = np.nan
    pts = px.box_points(lo, hi, seed=2)
    got, want = host_trilinear(hm, lat, lo, hi, pts), px.trilinear_f32(lat, lo, hi, pts)
    assert same_bits(got, want) and np.isnan(got).any() and not np.isnan(got).all()


@pytest.mark.parametrize("shape", LATTICES)
def test_host_function_against_float64_within_the_rounding_of_u(hm, shape):
    """Bound, with eps = 2^-24 (the unit roundoff of fp32), n the largest axis, S = max - min of the lattice, A = max |lattice|.
    The inputs (x, lo, hi, the lattice) are float32 in both, so only the arithmetic differs.
      u:  hi - lo, the division (n - 1) / (hi - lo), x - lo and the product each round once: u_32 = u (1 + e)^4, and after the clamp
          |u| <= n - 1, so |u_32 - u_64| <= du = 4.01 eps (n - 1) (the .01 covers the higher-order terms).
      f:  i0 <= u <= i0 + 1 <= 2 i0 for i0 >= 1, so u - float(i0) is exact (Sterbenz; for i0 = 0 it is u itself): f carries du and no more.
      value: the trilinear interpolant is continuous across cells and, along one axis, linear with a slope that is a convex combination of
          differences of two lattice values, |slope| <= S per unit of u.  Moving u by du on each of the 3 axes moves it by <= 3 du S,
          whether or not the float32 u falls into the neighbouring cell.
      blend: 1 - f rounds once (error <= eps), each step (1 - f) a + f b rounds two products and a sum: <= eps A (1 + (1 - f) + f + 1)
          = 3 eps A per step up to higher-order terms, and a convex combination does not amplify what it is handed: 3 steps, <= 10 eps A.
    bound = 3 * 4.01 eps (n - 1) S + 10 eps A."""
    lo, hi = BOXES[shape]
    lat = px.random_lattice(shape, seed=11 + sum(shape))
    pts = px.box_points(lo, hi, seed=4)
    got = host_trilinear(hm, lat, lo, hi, pts).astype(np.float64)
    want = px.trilinear_f64(lat, lo, hi, pts)
    eps = 2.0 ** -24
    S, A = float(lat.max()) - float(lat.min()), float(np.abs(lat).max())
    bound = 3 * 4.01 * eps * (max(shape) - 1) * S + 10 * eps * A
    err = float(np.abs(got - want).max())
    print(f"lattice {shape}: max |fp32 - fp64| = {err:.3e}, bound {bound:.3e}")
    assert err <= bound


# ---- C ABI -----------------------------------------------------------------------------------------------------------------------
NEW_ENTRY_POINTS = ("mipnerf_lattice_density", "mipnerf_forward_proposal")


def test_entry_points_are_declared_bound_and_exported():
    from mipnerf_pl_amd import _lib as L
    lib = L.lib()
    hdr = open(os.path.join(REPO, "include", "mipnerf_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in NEW_ENTRY_POINTS:
        proto = re.search(r"int " + name + r"\(([^)]*)\)", code).group(1)
        assert len(proto.split(",")) == len(L.SIGNATURES[name][1]), name
        assert hasattr(lib, name)
    assert len(L.SIGNATURES["mipnerf_lattice_density"][1]) == 12 and len(L.SIGNATURES["mipnerf_forward_proposal"][1]) == 15
    assert len(L.SIGNATURES) == 93
    assert lib.mipnerf_abi_version() == 6
    h = re.sub(r"[\s*]+", " ", hdr)
    for phrase in ["i0 = min(int(floorf(u)), n - 2)", "inv_h = float(n - 1) / (hi - lo)", "A non-finite coordinate gives 0",
                   "the background times (1 - acc)", "Does not allocate or synchronise", "mipnerf_workspace_bytes and no more"]:
        assert phrase in h, phrase


def _grid(dims=(8, 8, 8), lo=(-1, -1, -1), hi=(1, 1, 1)):
    return (C.c_int32 * 3)(*dims), (C.c_float * 3)(*lo), (C.c_float * 3)(*hi)


def test_lattice_density_validates_its_arguments_without_a_gpu():
    from mipnerf_pl_amd import _lib as L
    lib = L.lib()
    dims, lo, hi = _grid()

    def call(dims=dims, lo=lo, hi=hi, lattice=16, B=4, N=64, t=16, o=16, d=16, r=16, out=16):
        return lib.mipnerf_lattice_density(dims, lo, hi, lattice, B, N, t, o, d, r, out, None)
    for kw in (dict(dims=None), dict(lo=None), dict(hi=None), dict(lattice=None), dict(t=None), dict(o=None), dict(d=None), dict(r=None),
               dict(out=None)):
        assert call(**kw) == L.E_INVALID and "lattice_density" in L.last_error() and "null" in L.last_error(), kw
    for bad in ((1, 8, 8), (8, 1, 8), (8, 8, 1), (0, 8, 8)):
        assert call(dims=_grid(dims=bad)[0]) == L.E_INVALID and "at least 2 points" in L.last_error(), bad
    assert call(lo=hi, hi=lo) == L.E_INVALID and "hi > lo" in L.last_error()
    assert call(hi=_grid(hi=(1, -1, 1))[2]) == L.E_INVALID and "hi > lo" in L.last_error()          # hi == lo on one axis
    assert call(hi=_grid(hi=(1, float("nan"), 1))[2]) == L.E_INVALID
    for n in (0, -1, L.MAX_SAMPLES + 1):
        assert call(N=n) == L.E_INVALID and "num_samples" in L.last_error(), n
    assert call(B=-1) == L.E_INVALID and call(B=1 << 31) == L.E_INVALID
    # zero rays: nothing to do, whatever the ray pointers
    assert call(B=0, t=None, o=None, d=None, r=None, out=None) == L.OK


def test_forward_proposal_validates_the_lattice_without_a_gpu():
    from mipnerf_pl_amd import _lib as L
    lib = L.lib()
    dims, lo, hi = _grid()
    rp, outs = L.RaysPtrs(), (L.LevelOut * 2)()

    def call(ctx=None, dims=dims, lo=lo, hi=hi, lattice=16):
        return lib.mipnerf_forward_proposal(ctx, 4, C.byref(rp), dims, lo, hi, lattice, None, None, 0, L.PREC_FP32, 16, 1 << 20, outs, None)
    for kw in (dict(dims=None), dict(lo=None), dict(hi=None), dict(lattice=None)):
        assert call(**kw) == L.E_INVALID and "forward_proposal" in L.last_error() and "null" in L.last_error(), kw
    assert call(dims=_grid(dims=(8, 1, 8))[0]) == L.E_INVALID and "at least 2 points" in L.last_error()
    assert call(lo=hi, hi=lo) == L.E_INVALID and "hi > lo" in L.last_error()
    assert call() == L.E_INVALID and "ctx" in L.last_error()                 # a good lattice and no context


def test_the_unit_is_built_without_contraction_and_is_not_a_per_ray_kernel():
    from mipnerf_pl_amd import build
    assert ("kernels_proposal.hip", ["-ffp-contract=off"]) in build.UNITS
    src = open(os.path.join(REPO, "mipnerf_pl_amd", "csrc", "kernels_proposal.hip")).read()
    assert "template <int K" not in src and "hipFuncSetAttribute" not in src
    assert re.search(r"__global__[^;{]*\bk_lattice_density\(", src)
    assert "conical_frustum_to_gaussian(" in src and "lattice_trilinear(" in src and "make_float4(" in src
    hdr = open(os.path.join(REPO, "mipnerf_pl_amd", "csrc", "lattice_sample.hpp")).read()
    assert "MIP_HD float lattice_trilinear(" in hdr and " / " not in re.sub(r"//.*", "", hdr)      # no division on the device
    capi = open(os.path.join(REPO, "mipnerf_pl_amd", "csrc", "capi.hip")).read()
    levels = capi[capi.index("static int forward_levels("):capi.index("int mipnerf_forward(")]
    assert levels.count("mip::launch_composite_resample(") == 1                                               # one level loop, shared
    stage = capi[capi.index("int mipnerf_composite_resample("):capi.index("int mipnerf_composite_train(")]
    assert stage.count("mip::launch_composite_resample(") == 1 and capi.count("mip::launch_composite_resample(") == 2   # and the stage entry point


# ---- Python surface --------------------------------------------------------------------------------------------------------------
def test_keywords_and_their_defaults():
    from mipnerf_pl_amd import evaluate, model, ops, render_video
    assert list(inspect.signature(ops.ProposalGrid.__init__).parameters) == ["self", "lattice", "lo", "hi"]
    sig = inspect.signature(ops.field_proposal)
    assert list(sig.parameters) == ["model_or_system", "grid", "lo", "hi", "cov_scale", "precision"] and sig.parameters["grid"].default == 256
    assert list(inspect.signature(ops.lattice_density).parameters) == ["grid", "t_samples", "origins", "directions", "radii"]
    for fn in (model.MipNerf._forward_native, model.GraphedFrame.__init__, model.CulledFrame.__init__, evaluate.FrameEvaluator.__init__,
               evaluate.evaluate, render_video.render_video, render_video.render_path):
        assert inspect.signature(fn).parameters["proposal"].default is None, fn
    names = list(inspect.signature(model.CulledFrame.__init__).parameters)
    assert names[-3:] == ["proposal", "adaptive", "ladder"]
    sig = inspect.signature(evaluate.scene_proposal)
    assert list(sig.parameters)[:4] == ["system", "frames", "grid", "bound"] and sig.parameters["bound"].default is None
    for doc in (model.GraphedFrame.__doc__, model.CulledFrame.__doc__, model.MipNerf._forward_native.__doc__):
        d = re.sub(r"\s+", " ", doc)
        assert "silhouette against the background, not a coarse render" in d


def test_unbounded_and_one_level_models_are_refused_before_any_device_work():
    from mipnerf_pl_amd import evaluate, ops
    for m in (SimpleNamespace(unbounded=True, num_levels=2), SimpleNamespace(unbounded=False, num_levels=1)):
        with pytest.raises(NotImplementedError, match="unbounded=True|two-level"):
            ops._refuse_proposal_model(m, "x")
    ops._refuse_proposal_model(SimpleNamespace(unbounded=False, num_levels=2), "x")
    with pytest.raises(NotImplementedError, match="unbounded=True"):
        evaluate.scene_proposal(SimpleNamespace(mip_nerf=SimpleNamespace(unbounded=True)), None, 64, 1.0)


# ---- command line ----------------------------------------------------------------------------------------------------------------
def test_proposal_flags_and_their_defaults_on_both_command_lines():
    from mipnerf_pl_amd import eval as eval_cli
    from mipnerf_pl_amd import render_video
    base = ["--out_dir", "o", "--scale", "1"]
    for parser in (eval_cli.build_parser(), render_video.build_parser()):
        a = parser.parse_args(base)
        assert a.proposal_grid is None and a.proposal_bound is None and a.cull is False
        a = parser.parse_args(base + ["--proposal_grid"])
        assert a.proposal_grid == 256 and a.proposal_bound is None
        a = parser.parse_args(base + ["--proposal_grid", "128", "--proposal_bound", "4.5", "--cull", "--cull_adaptive"])
        assert a.proposal_grid == 128 and a.proposal_bound == 4.5 and a.cull is True and a.cull_adaptive is True
        text = re.sub(r"\s+", " ", parser.format_help())
        assert "--proposal_grid [N]" in text and "--proposal_bound" in text and "Not the two-level frame" in text


def test_proposal_refusals_come_before_anything_is_loaded_or_rendered(tmp_path):
    from mipnerf_pl_amd import eval as eval_cli
    from mipnerf_pl_amd import render_video
    missing = str(tmp_path / "no_such.ckpt")               # never opened: the refusal comes first
    out = str(tmp_path / "o")
    with pytest.raises(SystemExit, match="--proposal_bound.*--proposal_grid"):
        eval_cli.main(["--ckpt", missing, "--data", str(tmp_path), "--out_dir", out, "--scale", "1", "--proposal_bound", "4"])
    with pytest.raises(SystemExit, match="--proposal_bound.*--proposal_grid"):
        render_video.main(["--ckpt", missing, "--out_dir", out, "--scale", "1", "--proposal_bound", "4"])
    with pytest.raises(SystemExit, match="at least 4 points"):
        render_video.main(["--ckpt", missing, "--out_dir", out, "--scale", "1", "--proposal_grid", "3"])
    with pytest.raises(SystemExit, match="must be positive"):
        render_video.main(["--ckpt", missing, "--out_dir", out, "--scale", "1", "--proposal_grid", "--proposal_bound", "0"])
    assert not os.path.exists(out)
    on = SimpleNamespace(proposal_grid=256, proposal_bound=None)
    for name in ("llff", "realdata360"):
        with pytest.raises(SystemExit, match="--proposal_grid.*captured scene.*" + name):
            render_video.refuse_scene360_proposal(on, SimpleNamespace(hparams={"dataset_name": name}, mip_nerf=SimpleNamespace(unbounded=True)))
    with pytest.raises(SystemExit, match="--proposal_grid"):
        render_video.refuse_scene360_proposal(on, SimpleNamespace(hparams={"dataset_name": "blender"}, mip_nerf=SimpleNamespace(unbounded=True)))
    blender = SimpleNamespace(hparams={"dataset_name": "blender"}, mip_nerf=SimpleNamespace(unbounded=False))
    render_video.refuse_scene360_proposal(on, blender)
    render_video.refuse_scene360_proposal(SimpleNamespace(proposal_grid=None, proposal_bound=None),
                                          SimpleNamespace(hparams={"dataset_name": "llff"}, mip_nerf=SimpleNamespace(unbounded=True)))
    render_video.refuse_proposal_without_grid(SimpleNamespace(proposal_grid=64, proposal_bound=2.0))
    assert render_video.cli_proposal(SimpleNamespace(proposal_grid=None, proposal_bound=None), blender, None) is None


def test_a_scene360_checkpoint_is_refused_by_both_commands_before_rendering(tmp_path):
    from mipnerf_pl_amd import eval as eval_cli
    from mipnerf_pl_amd import render_video
    from mipnerf_pl_amd.config import SCENE360_PRESET
    from mipnerf_pl_amd.system import DEFAULT_HPARAMS, MipNeRFSystem
    hp = dict(DEFAULT_HPARAMS)
    hp.update(SCENE360_PRESET)
    hp.update({"nerf.num_samples": 16, "exp_name": "cli360", "dataset_name": "llff"})
    ckpt = str(tmp_path / "last.ckpt")
    MipNeRFSystem(hp, precision="fp32").save_checkpoint(ckpt)
    out = str(tmp_path / "o")
    with pytest.raises(SystemExit, match="--proposal_grid.*captured scene"):
        eval_cli.main(["--ckpt", ckpt, "--data", str(tmp_path), "--out_dir", out, "--scale", "1", "--proposal_grid"])
    with pytest.raises(SystemExit, match="--proposal_grid.*captured scene"):
        render_video.main(["--ckpt", ckpt, "--data", str(tmp_path), "--out_dir", out, "--scale", "1", "--proposal_grid", "64"])
    assert not os.path.exists(out)
