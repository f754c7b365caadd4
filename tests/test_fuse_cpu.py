"""CPU (no GPU): rendered depth fused into a truncated signed distance volume -- the rules csrc/fuse_rules.hpp states for host and device
against tests/fuse_fixture.py: the host build of the integration (mipnerf_fuse_integrate_host) bit for bit against the float32 restatement,
the projection rows against the reference's pixel-to-direction formula in float64, the depth quantile (built with g++ -O2
-ffp-contract=off from tests/hostmath/fuse.cpp) by the bracket test against a float64 restatement, the whole pipeline on an analytic
sphere in numpy; the eleventh library's declarations, bindings, exports and argument checks without a device; the build units; the
command line's refusals."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import fuse_fixture as fx
import isosurface_fixture as ix
from mipnerf_pl_amd import _lib as L

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
CSRC = os.path.join(REPO, "mipnerf_pl_amd", "csrc")
F = np.float32


@pytest.fixture(scope="module")
def hm():
    src, so = os.path.join(HERE, "hostmath", "fuse.cpp"), os.path.join(HERE, "hostmath", "_fuse.so")
    hdrs = [os.path.join(CSRC, h) for h in ("fuse_rules.hpp", "raymath.hpp")]
    if (not os.path.exists(so)) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in [src] + hdrs):
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", src, "-o", so])
    return C.CDLL(so)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.FUSE_LIB_PATH):
        from mipnerf_pl_amd import build
        build.build(verbose=False)
    return L.fuse_lib()


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _err(lib):
    return (lib.mipnerf_fuse_last_error() or b"").decode()


def projection(lib, cams):
    cams = np.ascontiguousarray(cams, F).reshape(-1, 32)
    frames = np.zeros((len(cams), 16), F)
    for rec, out in zip(cams, frames):
        assert lib.mipnerf_fuse_projection(_p(rec), _p(out)) == L.OK, _err(lib)
    return frames


def integrate_host(lib, dims, lo, hi, trunc, carve, frames, offsets, depth, state=None):
    s, c = (np.zeros(dims[::-1], F), np.zeros(dims[::-1], F)) if state is None else (state[0].copy(), state[1].copy())
    frames, offsets, depth = np.ascontiguousarray(frames, F), np.ascontiguousarray(offsets, np.int64), np.ascontiguousarray(depth, F)
    rc = lib.mipnerf_fuse_integrate_host((C.c_int32 * 3)(*dims), (C.c_float * 3)(*lo), (C.c_float * 3)(*hi), trunc, int(carve), len(frames),
                                         _p(frames), _p(offsets), _p(depth), depth.size, _p(s), _p(c))
    assert rc == L.OK, _err(lib)
    return s, c


def same_bits(a, b):
    a, b = np.asarray(a, F), np.asarray(b, F)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


# ---- rules T and F ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("carve", [True, False])
@pytest.mark.parametrize("num_frames", [1, 3, L.FUSE_FRAMES_PER_LAUNCH + 1])
@pytest.mark.parametrize("lattice", range(len(fx.LATTICES)))
def test_host_integration_equals_the_float32_restatement_bit_for_bit(lib, hm, lattice, num_frames, carve):
    dims, lo, hi = fx.LATTICES[lattice]
    trunc = 0.35
    cams = fx.frame_cameras(num_frames, seed=lattice)
    frames = projection(lib, cams)
    depth, offsets = fx.frame_depths(cams, seed=num_frames)
    assert {int(c[26]) for c in cams} == ({0, 1} if num_frames > 2 else {0}) and hm.hm_frames_per_launch() == L.FUSE_FRAMES_PER_LAUNCH
    got = integrate_host(lib, dims, lo, hi, trunc, carve, frames, offsets, depth)
    want = fx.integrate_f32(dims, lo, hi, trunc, carve, frames, offsets, depth, np.zeros(dims[::-1], F), np.zeros(dims[::-1], F))
    assert same_bits(got[0], want[0]) and same_bits(got[1], want[1])
    # the cases the rule names are all there: updated and untouched points, truncated (d == 1) and signed distances of both signs
    assert (got[1] > 0).any() and (got[1] == 0).any()
    if num_frames >= 3:
        x, y, z = fx.lattice_points_f32(dims, lo, hi)
        P = frames[:, :12].reshape(-1, 3, 4)
        t = P[:, 2, 0, None, None, None] * x + P[:, 2, 1, None, None, None] * y + P[:, 2, 2, None, None, None] * z + P[:, 2, 3, None, None, None]
        assert (t <= 0).any() and (t > frames[:, 15, None, None, None]).any()            # behind a camera; beyond far
        with np.errstate(all="ignore"):
            u = (P[:, 0, 0, None, None, None] * x + P[:, 0, 1, None, None, None] * y + P[:, 0, 2, None, None, None] * z + P[:, 0, 3, None, None, None]) / t
        assert ((t > 0.5) & ((u < 0) | (u >= frames[:, 12, None, None, None]))).any()      # outside the image
        assert np.isinf(depth).any() and np.isnan(depth).any() and (depth == 0).any() and (depth < 0).any()
    # F single-frame calls give the same bytes
    state = (np.zeros(dims[::-1], F), np.zeros(dims[::-1], F))
    for f in range(num_frames):
        state = integrate_host(lib, dims, lo, hi, trunc, carve, frames[f:f + 1], offsets[f:f + 1], depth, state)
    assert same_bits(state[0], got[0]) and same_bits(state[1], got[1])
    # rule F on the host build against the restatement, both fills
    for unseen, fill in (("inside", 1.0), ("outside", -1.0)):
        out = np.zeros(dims[::-1], F)
        hm.hm_finalise(C.c_longlong(out.size), _p(got[0]), _p(got[1]), C.c_float(fill), _p(out))
        assert same_bits(out, fx.finalise_f32(got[0], got[1], unseen))
        assert (out[got[1] == 0] == fill).all() and (np.abs(out[got[1] > 0]) <= 1).all()


def test_carving_changes_only_points_that_see_a_free_ray(lib):
    dims, lo, hi = fx.LATTICES[0]
    cams = fx.frame_cameras(3)
    frames = projection(lib, cams)
    depth, offsets = fx.frame_depths(cams)
    on = integrate_host(lib, dims, lo, hi, 0.35, True, frames, offsets, depth)
    off = integrate_host(lib, dims, lo, hi, 0.35, False, frames, offsets, depth)
    assert (on[1] >= off[1]).all() and (on[1] > off[1]).any()
    more = on[1] - off[1]
    # each free ray added d = 1; the sums hold a few terms of size <= 1, so their difference is off by a few float32 roundings at most
    assert np.abs((on[0] - off[0]) - more).max() <= 8 * 2.0 ** -24 * float(on[1].max())
    assert same_bits(on[0][more == 0], off[0][more == 0])


# ---- rule P ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
def test_projection_brings_every_pixel_centre_back(lib, mode):
    W, H, near, far = 14, 9, 0.5, 6.0
    c2w = fx.look_at((1.7, -2.1, 1.3), (0.1, 0.2, -0.1))
    rec = fx.camera_row(c2w, W, H, near, far, focal=15.4) if mode == 0 else \
        fx.camera_row(c2w, W, H, near, far, pix2cam=fx.pix2cam_of(15.4, 14.9, 7.3, 4.2, skew=0.03))
    P = projection(lib, rec[None])[0].astype(np.float64)
    assert P[12:16].tolist() == [W, H, near, far]
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    worst_px = worst_t = 0.0
    for t in (near, 0.5 * (near + far), far):
        p = fx.pixel_point_f64(rec, xx, yy, np.full(xx.shape, t))
        a, b, tt = [(P[4 * r:4 * r + 3] * p).sum(-1) + P[4 * r + 3] for r in range(3)]
        worst_px = max(worst_px, float(np.abs(a / tt - (xx + 0.5)).max()), float(np.abs(b / tt - (yy + 0.5)).max()))
        worst_t = max(worst_t, float(np.abs(tt / t - 1.0).max()))
    print(f"mode {mode}: pixel error {worst_px:.2e} px, relative t error {worst_t:.2e}")
    assert worst_px <= 1e-4 and worst_t <= 1e-6


def test_projection_refuses_what_it_cannot_invert(lib):
    out = np.zeros(16, F)
    rec = fx.camera_row(fx.look_at((3, 0, 0), (0, 0, 0)), 8, 6, 1, 5, pix2cam=fx.pix2cam_of(9, 9, 4, 3))
    for mode, name in ((2, "radial-tangential"), (3, "fisheye")):
        bad = rec.copy()
        bad[26] = mode
        assert lib.mipnerf_fuse_projection(_p(bad), _p(out)) == L.E_UNSUPPORTED
        assert f"camera mode {mode}" in _err(lib) and name in _err(lib) and "ideal pinhole frames of the capture's K" in _err(lib) and "PathGen" in _err(lib)
    bad = rec.copy()
    bad[26] = 7
    assert lib.mipnerf_fuse_projection(_p(bad), _p(out)) == L.E_INVALID and "unknown camera mode" in _err(lib)
    bad = rec.copy()
    bad[20] = 1.0
    assert lib.mipnerf_fuse_projection(_p(bad), _p(out)) == L.E_INVALID and "(0, 0, -1)" in _err(lib)
    bad = rec.copy()
    bad[12:18] = 0
    assert lib.mipnerf_fuse_projection(_p(bad), _p(out)) == L.E_INVALID and "inverse" in _err(lib)
    for k, v in ((21, 0), (22, -3), (21, 7.5), (22, np.nan)):
        bad = rec.copy()
        bad[k] = v
        assert lib.mipnerf_fuse_projection(_p(bad), _p(out)) == L.E_INVALID and "width and height" in _err(lib)
    bad = fx.camera_row(fx.look_at((3, 0, 0), (0, 0, 0)), 8, 6, 1, 5, focal=0.0)
    assert lib.mipnerf_fuse_projection(_p(bad), _p(out)) == L.E_INVALID and "focal" in _err(lib)
    assert lib.mipnerf_fuse_projection(None, _p(out)) == L.E_INVALID and lib.mipnerf_fuse_projection(_p(rec), None) == L.E_INVALID


# ---- rule D ----------------------------------------------------------------------------------------------------------------------------
def host_quantile(hm, w, t, qs):
    w, t, qs = np.ascontiguousarray(w, F), np.ascontiguousarray(t, F), np.ascontiguousarray(qs, F)
    out = np.full((w.shape[0], len(qs)), -7.0, F)
    hm.hm_depth_quantile(C.c_longlong(w.shape[0]), w.shape[1], _p(w), _p(t), len(qs), _p(qs), _p(out))
    return out


@pytest.mark.parametrize("cls", fx.QUANTILE_CLASSES)
@pytest.mark.parametrize("N", fx.QUANTILE_NS)
def test_depth_quantile_of_the_host_rule_and_a_float32_emulation_inside_the_bracket(hm, N, cls):
    for j, q in enumerate(fx.QUANTILES):
        w, t = fx.quantile_rays(N, cls, B=40, seed=1000 * N + j, q=q)
        got = host_quantile(hm, w, t, fx.QUANTILES)[:, j]
        q32 = float(F(q))
        assert fx.quantile_bracket(w, t, q32, got).all(), (N, cls, q)
        assert fx.quantile_bracket(w, t, q32, fx.quantile_f32seq(w, t, q32)).all(), (N, cls, q, "float32 emulation")
        # the host rule sums in the restatement's order: it IS the float64 restatement wherever the float32 rounding of the result allows
        want = fx.quantile_f64(w, t, q32)
        assert np.array_equal(np.isinf(got), np.isinf(want))
        fin = np.isfinite(want)
        assert np.allclose(got[fin], want[fin], rtol=2.0 ** -23, atol=0)
        if cls in ("empty", "zero"):
            assert np.isinf(got).all() and (got > 0).all()
        if cls in ("opaque", "surface") and q <= 0.5:
            assert np.isfinite(got).all()
        if cls == "edge":
            assert np.isfinite(want).any()
        assert ((got >= t[:, 0]) & ((got <= t[:, -1]) | np.isinf(got))).all()


def test_depth_quantile_is_monotone_in_q_and_ignores_nan_and_negative_weights(hm):
    w, t = fx.quantile_rays(64, "soft", B=16, seed=5)
    assert np.isnan(w).any() and (w < 0).any()
    d = host_quantile(hm, w, t, (0.05, 0.2, 0.25, 0.29))
    assert (np.diff(d, axis=1) >= 0).all()
    clean = np.where(w > 0, w, F(0)).astype(F)
    assert same_bits(host_quantile(hm, clean, t, (0.05, 0.2, 0.25, 0.29)), d)


# ---- the pipeline on an analytic sphere, in numpy ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sphere_volume(lib):
    dims, lo, hi, h, trunc = fx.sphere_lattice()
    cams = fx.sphere_cameras()
    depth, offsets = fx.sphere_depths(cams)
    frames = projection(lib, cams)
    s, c = fx.integrate_f32(dims, lo, hi, trunc, True, frames, offsets, depth, np.zeros(dims[::-1], F), np.zeros(dims[::-1], F))
    return dims, lo, hi, s, c


def test_sphere_fused_in_numpy_is_a_closed_sphere(sphere_volume):
    dims, lo, hi, s, c = sphere_volume
    cams = fx.sphere_cameras()
    assert len(cams) == fx.SPHERE_VIEWS and (c == 0).any() and (c > 0).any()
    views = (cams[:, :12].reshape(-1, 3, 4)[:, :, 3] - ix.CENTRE) / fx.SPHERE_RADIUS
    assert np.allclose(np.linalg.norm(views, axis=1), 1.0, atol=1e-6) and fx.view_obliquity(views) <= fx.SPHERE_MAX_OBLIQUITY
    m = ix.marching_tets(fx.finalise_f32(s, c, "inside"), 0.0, lo, hi)
    figures = fx.check_sphere_mesh(m["vertices"], m["faces"])
    assert figures["vertices"] > 3000


def test_unseen_points_called_outside_wrap_the_sphere_in_an_inner_shell(sphere_volume):
    """the recorded reason for unseen='inside': the points deeper than trunc behind every view's surface are never updated"""
    dims, lo, hi, s, c = sphere_volume
    m = ix.marching_tets(fx.finalise_f32(s, c, "outside"), 0.0, lo, hi)
    chi = ix.euler_characteristic(len(m["vertices"]), m["faces"])
    print("unseen='outside': Euler characteristic", chi, "volume error", ix.enclosed_volume(m["vertices"], m["faces"]) / ix.SPHERE_VOLUME - 1.0)
    assert chi != 2


# ---- the eleventh library: declarations, bindings, exports, argument checks ------------------------------------------------------------
NAMES = ["mipnerf_fuse_abi_version", "mipnerf_fuse_depth_quantile", "mipnerf_fuse_finalise", "mipnerf_fuse_integrate",
         "mipnerf_fuse_integrate_host", "mipnerf_fuse_last_error", "mipnerf_fuse_projection"]


def _header(comments=False):
    text = open(os.path.join(REPO, "include", "mipnerf_fuse.h")).read()
    return text if comments else re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return sorted(line.split()[-1] for line in out.splitlines() if line.strip())


def test_header_bindings_and_dynamic_symbols_are_one_set(lib):
    declared = sorted(set(re.findall(r"\b(mipnerf_[a-z0-9_]+)\s*\(", _header())))
    assert declared == sorted(L.FUSE_SIGNATURES) == NAMES
    assert _exports(L.FUSE_LIB_PATH) == declared
    for name, (_, args) in L.FUSE_SIGNATURES.items():
        proto = re.search(r"\b" + name + r"\s*\(([^)]*)\)", _header()).group(1).strip()
        assert (0 if proto in ("", "void") else proto.count(",") + 1) == len(args), (name, proto)
    assert lib.mipnerf_fuse_abi_version() == 1 == L.FUSE_ABI
    for macro, value in (("MAX_QUANTILES", L.FUSE_MAX_QUANTILES), ("FRAME_FLOATS", L.FUSE_FRAME_FLOATS),
                         ("FRAMES_PER_LAUNCH", L.FUSE_FRAMES_PER_LAUNCH)):
        assert int(re.search(r"#define MIPNERF_FUSE_" + macro + r" (\d+)", _header()).group(1)) == value
    assert L.FUSE_MAX_QUANTILES == 4 and L.FUSE_FRAME_FLOATS == 16
    text = re.sub(r"\s+", " ", re.sub(r"\n \*", "\n", _header(comments=True)))
    for rule in ("D1 w'_i = fmaxf(w_i, 0.0f)", "D2 P_i = sum_{j <= i} w'_j in double", "ONE array of inclusive prefixes",
                 "D4 no interval qualifies", "P = cam2pix [R^T | -R^T o]", "T1 p = lo + float(i) * h", "a = (P00 x + P01 y) + (P02 z + P03)",
                 "near_f < t <= far_f", "T3 D = depth[offset_f + v * W_f + u]", "T5 otherwise s = D - t", "T6 sum += d; count += 1.0f",
                 "No atomics", "count > 0 ? -(sum / count) : fill", "never allocates and never synchronises"):
        assert rule in text, rule


def test_the_other_ten_libraries_keep_their_tables(lib):
    assert len(L.SIGNATURES) == 93
    for table in (L.SIGNATURES, L.DIAG_SIGNATURES, L.PREVIEW_SIGNATURES, L.PREVIEW_MIP_SIGNATURES, L.PREVIEW_SPARSE_SIGNATURES,
                  L.PREVIEW_TUNE_SIGNATURES, L.PREVIEW_360_SIGNATURES, L.PREVIEW_REG_SIGNATURES, L.PREVIEW_TUNE_360_SIGNATURES,
                  L.PROPOSAL_360_SIGNATURES):
        assert not set(table) & set(L.FUSE_SIGNATURES)
        assert not any(n.startswith("mipnerf_fuse_") for n in table)
    assert all(n.startswith("mipnerf_fuse_") for n in L.FUSE_SIGNATURES)
    assert not any("fuse" in n for n in _exports(L.LIB_PATH))
    assert len(L.PROPOSAL_360_SIGNATURES) == 4 and len(L.PREVIEW_SIGNATURES) == 4 and len(L.DIAG_SIGNATURES) == 3


def test_entry_points_validate_their_arguments_without_a_gpu(lib):
    err = lambda: _err(lib)  # noqa: E731
    i3, f3 = C.c_int32 * 3, C.c_float * 3

    def quantile(B=4, N=64, w=16, t=16, nq=1, q=(0.5,), out=16):
        return lib.mipnerf_fuse_depth_quantile(B, N, w, t, nq, None if q is None else (C.c_float * 4)(*q), out, None)
    for kw in (dict(w=None), dict(t=None), dict(out=None), dict(q=None)):
        assert quantile(**kw) == L.E_INVALID and "null" in err(), kw
    for n in (0, -1, L.MAX_SAMPLES + 1):
        assert quantile(N=n) == L.E_INVALID and "num_samples" in err(), n
    for nq in (0, -1, 5):
        assert quantile(nq=nq) == L.E_INVALID and "num_quantiles" in err(), nq
    for q in (0.0, 1.0, -0.1, 1.5, float("nan")):
        assert quantile(q=(q,)) == L.E_INVALID and "(0, 1)" in err(), q
    assert quantile(nq=2, q=(0.5, 1.0)) == L.E_INVALID and "(0, 1)" in err()
    assert quantile(B=-1) == L.E_INVALID and quantile(B=1 << 31) == L.E_INVALID
    assert quantile(B=0, w=None, t=None, out=None, nq=4, q=(0.1, 0.2, 0.3, 0.4)) == L.OK        # zero rays: nothing to do

    def volume(fn, dims=(9, 8, 7), lo=(-1, -1, -1), hi=(1, 1, 1), trunc=0.1, F_=2, fr=16, off=16, depth=16, count=100, s=16, c=16, nulls=()):
        args = [None if "dims" in nulls else i3(*dims), None if "lo" in nulls else f3(*lo), None if "hi" in nulls else f3(*hi), trunc, 1, F_, fr,
                off, depth, count, s, c]
        return fn(*(args + [None] if fn is lib.mipnerf_fuse_integrate else args))
    for fn, who in ((lib.mipnerf_fuse_integrate, "fuse_integrate: "), (lib.mipnerf_fuse_integrate_host, "fuse_integrate_host: ")):
        for kw in (dict(fr=None), dict(off=None), dict(depth=None), dict(s=None), dict(c=None), dict(nulls=("dims",)), dict(nulls=("lo",)),
                   dict(nulls=("hi",))):
            assert volume(fn, **kw) == L.E_INVALID and "null" in err() and err().startswith(who), kw
        for bad in ((1, 9, 9), (9, 1, 9), (9, 9, 1), (0, 9, 9)):
            assert volume(fn, dims=bad) == L.E_INVALID and "at least 2 points" in err(), bad
        assert volume(fn, lo=(1, 1, 1), hi=(-1, -1, -1)) == L.E_INVALID and "hi > lo" in err()
        assert volume(fn, hi=(1, -1, 1)) == L.E_INVALID and "hi > lo" in err()                 # hi == lo on one axis
        assert volume(fn, hi=(1, float("nan"), 1)) == L.E_INVALID
        assert volume(fn, dims=(1024, 1024, 512)) == L.E_INVALID and "2^31" in err()
        assert volume(fn, dims=(675, 675, 674)) == L.E_INVALID and "2^31" in err()             # just above 2^31 / 7
        assert volume(fn, dims=(675, 674, 674), F_=0) == L.OK                                  # just below; zero frames: nothing to do
        for trunc in (0.0, -1.0, float("inf"), float("nan")):
            assert volume(fn, trunc=trunc) == L.E_INVALID and "trunc" in err(), trunc
        assert volume(fn, F_=-1) == L.E_INVALID and "frame count" in err()
        assert volume(fn, count=-1) == L.E_INVALID and "depth count" in err()
        assert volume(fn, F_=0, fr=None, off=None, depth=None) == L.OK

    def finalise(dims=(9, 8, 7), s=16, c=16, fill=1.0, out=16):
        return lib.mipnerf_fuse_finalise(None if dims is None else i3(*dims), s, c, fill, out, None)
    for kw in (dict(dims=None), dict(s=None), dict(c=None), dict(out=None)):
        assert finalise(**kw) == L.E_INVALID and "null" in err(), kw
    assert finalise(dims=(1, 8, 7)) == L.E_INVALID and "at least 2 points" in err()
    assert finalise(dims=(1024, 1024, 512)) == L.E_INVALID and "2^31" in err()
    for fill in (0.0, 0.5, float("nan")):
        assert finalise(fill=fill) == L.E_INVALID and "fill" in err(), fill


def test_the_build_units_are_compiled_without_contraction_into_an_eleventh_library():
    from mipnerf_pl_amd import build as b
    assert [u for u, _ in b.FUSE_UNITS] == ["kernels_fuse.hip", "fuse_capi.hip"]
    assert all("-ffp-contract=off" in flags for _, flags in b.FUSE_UNITS)
    assert os.path.basename(b.FUSE_LIB) == "libmipnerf_fuse.so" == os.path.basename(L.FUSE_LIB_PATH)
    assert not any("fuse" in u for u, _ in b.UNITS + b.DIAG_UNITS + b.PREVIEW_UNITS + b.PREVIEW_MIP_UNITS + b.PREVIEW_SPARSE_UNITS +
                   b.PREVIEW_TUNE_UNITS + b.PREVIEW_360_UNITS + b.PREVIEW_REG_UNITS + b.PREVIEW_TUNE_360_UNITS + b.PROPOSAL_360_UNITS)
    src = open(os.path.join(REPO, "mipnerf_pl_amd", "build.py")).read()
    assert '"include", "mipnerf_fuse.h"' in src and "os.path.exists(FUSE_LIB)" in src
    rules = re.sub(r"//.*", "", open(os.path.join(CSRC, "fuse_rules.hpp")).read())
    for fn in ("quantile_weight(", "quantile_crosses(", "quantile_depth(", "fuse_point(", "fuse_row(", "fuse_frame_update(", "fuse_finalise_value("):
        assert re.search(r"MIP_HD \w+ " + re.escape(fn), rules), fn
    unit = re.sub(r"//.*", "", open(os.path.join(CSRC, "kernels_fuse.hip")).read())
    for kernel in ("k_depth_quantile", "k_fuse_integrate", "k_fuse_finalise"):
        assert re.search(r"\b" + kernel + r"\(", unit), kernel
    assert "for_lane_bucket(" in unit and "wave_incl_scan_dpp(" in unit and "kDppWaveShr1" in unit and "__ballot(" in unit
    assert "__shared__" not in unit and "atomic" not in unit and "hipFuncSetAttribute" not in unit
    # the kernels restate no rule: the arithmetic of D, T and F lives in the header alone
    assert not re.search(r"floorf|fminf|fmaxf|trunc \*|/ trunc", unit)
    for fn in ("quantile_weight(", "quantile_crosses(", "quantile_depth(", "fuse_frame_update(", "fuse_finalise_value("):
        assert fn in unit, fn
    capi = re.sub(r"//.*", "", open(os.path.join(CSRC, "fuse_capi.hip")).read())
    assert "fuse_frame_update(" in capi and "fuse_projection_row(" in capi and "hipMalloc" not in capi and "Synchronize" not in capi


# ---- Python surface and the command line ---------------------------------------------------------------------------------------------
def test_names_signatures_and_defaults():
    from mipnerf_pl_amd import fuse, ops
    assert list(inspect.signature(ops.depth_quantile).parameters)[:3] == ["weights", "t_samples", "q"]
    assert inspect.signature(ops.depth_quantile).parameters["q"].default == 0.5
    assert list(inspect.signature(ops.fuse_projection).parameters) == ["cameras"]
    assert list(inspect.signature(ops.TSDF.__init__).parameters)[:5] == ["self", "dims", "lo", "hi", "trunc"]
    sig = inspect.signature(ops.TSDF.integrate)
    assert list(sig.parameters) == ["self", "frames", "depth", "offsets", "carve"] and sig.parameters["carve"].default is True
    assert inspect.signature(ops.TSDF.lattice).parameters["unseen"].default == "inside"
    sig = inspect.signature(fuse.DepthFrame.__init__)
    assert list(sig.parameters) == ["self", "model", "num_rays", "chunk", "white_bkgd", "device", "quantiles"]
    assert sig.parameters["quantiles"].default == (0.5,)
    sig = inspect.signature(fuse.fuse_mesh)
    assert list(sig.parameters) == ["system_or_model", "cameras", "grid", "lo", "hi", "trunc_cells", "quantile", "unseen", "carve", "color",
                                    "precision"]
    assert [sig.parameters[k].default for k in list(sig.parameters)[2:]] == [256, None, None, 3.0, 0.5, "inside", True, True, None]
    assert "a choice, not a measurement" in re.sub(r"\s+", " ", fuse.fuse_mesh.__doc__)
    for bad in (dict(quantile=0.0), dict(quantile=1.0), dict(trunc_cells=0.0), dict(trunc_cells=float("nan")), dict(unseen="both")):
        kw = dict(trunc_cells=3.0, quantile=0.5, unseen="inside")
        kw.update(bad)
        with pytest.raises(ValueError):
            fuse.check_fuse_arguments(**kw)
    with pytest.raises(ValueError, match="quantiles"):
        fuse.DepthFrame(None, 4, 4, False, "cpu", quantiles=(0.1, 0.2, 0.3, 0.4, 0.5))
    with pytest.raises(ValueError, match="quantiles"):
        fuse.DepthFrame(None, 4, 4, False, "cpu", quantiles=(1.0,))
    # the projection is host only: it runs here, and it refuses a distorted camera by name
    rec = fx.camera_row(fx.look_at((3, 0, 0), (0, 0, 0)), 8, 6, 1, 5, focal=9.0)
    frames = ops.fuse_projection(rec[None])
    assert tuple(frames.shape) == (1, 16) and frames.device.type == "cpu" and frames[0, 12:].tolist() == [8, 6, 1, 5]
    rec[12:21], rec[26] = fx.pix2cam_of(9, 9, 4, 3).reshape(-1), 3
    with pytest.raises(NotImplementedError, match="fisheye.*PathGen"):
        ops.fuse_projection(rec[None])


def test_command_line_flags_and_refusals_before_any_file_is_written(tmp_path):
    from mipnerf_pl_amd import fuse_mesh as cli
    a = cli.build_parser().parse_args(["--out_dir", "o"])
    assert (a.split, a.every, a.scale, a.grid, a.bound, a.aabb, a.trunc_cells, a.quantile, a.unseen, a.carve, a.color, a.save_depth, a.save_tsdf,
            a.precision) == ("train", 1, 1, [256], 1.5, None, 3.0, 0.5, "inside", True, True, False, False, None)
    a = cli.build_parser().parse_args(["--out_dir", "o", "--grid", "9", "8", "7", "--no_carve", "--no_color", "--unseen", "outside", "--save_tsdf",
                                       "--save_depth", "--aabb", "0", "0", "0", "1", "2", "3"])
    assert (a.grid, a.carve, a.color, a.unseen, a.save_tsdf, a.save_depth) == ([9, 8, 7], False, False, "outside", True, True)
    assert cli.lattice_of(a) == ((9, 8, 7), (0.0, 0.0, 0.0), (1.0, 2.0, 3.0))
    text = re.sub(r"\s+", " ", cli.build_parser().format_help())
    assert "a choice, not a measurement" in text and "--save_tsdf" in text and "--every" in text
    missing, out = str(tmp_path / "no_such.ckpt"), str(tmp_path / "o")               # never opened: the refusal comes first
    base = ["--ckpt", missing, "--data", str(tmp_path), "--out_dir", out]
    for extra, msg in ((["--quantile", "0"], "--quantile must lie inside"), (["--quantile", "1"], "--quantile must lie inside"),
                       (["--quantile", "1.5"], "--quantile must lie inside"), (["--trunc_cells", "0"], "--trunc_cells must be finite and > 0"),
                       (["--trunc_cells", "-2"], "--trunc_cells must be finite and > 0"), (["--every", "0"], "--every must be at least 1"),
                       (["--grid", "9", "9"], "--grid takes one number or three")):
        with pytest.raises(SystemExit, match=msg):
            cli.main(base + extra)
    with pytest.raises(SystemExit, match="give --data"):
        cli.main(["--ckpt", missing, "--out_dir", out])
    assert not os.path.exists(out)
