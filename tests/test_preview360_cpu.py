"""CPU (no GPU): the contracted-space preview -- the seventh library's declarations, bindings, exports and argument checks without a
device; the float64 fixture (tests/preview360_fixture.py) against the host build of csrc/preview_march_360.hpp (g++ -O2
-ffp-contract=off from tests/hostmath/preview_360.cpp) and against the bounded fixture inside the unit ball; the properties of the warp
(inverse, step bound, sample count, partition); the Python-side refusals and the .npz round trip."""
import ctypes as C
import os
import re
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import preview360_fixture as pf
import preview_fixture as bounded
from mipnerf_pl_amd import _lib as L
from mipnerf_pl_amd import preview as pv

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
SRC = os.path.join(HERE, "hostmath", "preview_360.cpp")
SO = os.path.join(HERE, "hostmath", "_preview_360.so")
F = np.float32
TOL = dict(rgb=5e-5, acc=5e-5, distance=2e-4)          # the project's fp32 bounds (__graft_entry__.py); distance times max(1, far)
FRAGILE_CAP = 0.10
BG = (0.2, 0.9, 0.4)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.PREVIEW_360_LIB_PATH):
        from mipnerf_pl_amd import build
        build.build(verbose=False)
    return L.preview_360_lib()


@pytest.fixture(scope="module")
def hm():
    hdrs = [os.path.join(REPO, "mipnerf_pl_amd", "csrc", h) for h in ("raymath.hpp", "lattice_sample.hpp", "preview_march.hpp",
                                                                      "preview_march_360.hpp")]
    if (not os.path.exists(SO)) or os.path.getmtime(SO) < max(os.path.getmtime(f) for f in [SRC] + hdrs):
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", SRC, "-o", SO])
    return C.CDLL(SO)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def host_march(hm, rows, degree, rays, step_scale, t_min, max_steps, background, occupancy=None, lo=pf.LO, hi=pf.HI, far_radius=pf.FAR_RADIUS):
    o, d, tn, tf = rays
    nz, ny, nx, _ = rows.shape
    B = o.shape[0]
    bits = np.ascontiguousarray(rows).view(np.uint16)
    rgb, acc, dist, steps = np.zeros((B, 3), F), np.zeros(B, F), np.zeros(B, F), np.zeros(B, np.int32)
    lo, hi, bg = np.array(lo, F), np.array(hi, F), np.array(background, F)
    hm.hm_preview360_march(_p(bits), _p(occupancy), nx, ny, nz, _p(lo), _p(hi), degree, C.c_float(far_radius), C.c_float(step_scale),
                           C.c_float(t_min), max_steps, _p(bg), C.c_longlong(B), _p(o), _p(d), _p(tn), _p(tf), _p(rgb), _p(acc), _p(dist),
                           _p(steps))
    return rgb, acc, dist, steps


def host_samples(hm, o, d, tn, tf, s, max_steps=1 << 20, far_radius=pf.FAR_RADIUS, cap=1 << 16):
    z, t, delta = np.zeros((cap, 3), F), np.zeros(cap, F), np.zeros(cap, F)
    n = hm.hm_preview360_samples(C.c_float(far_radius), C.c_float(s), max_steps, _p(np.asarray(o, F)), _p(np.asarray(d, F)), C.c_float(tn),
                                 C.c_float(tf), cap, _p(z), _p(t), _p(delta))
    return n, z[:max(n, 0)], t[:max(n, 0)], delta[:max(n, 0)]


def compare(got, want, far, what):
    """`got` (rgb, acc, dist, steps) against the fixture's `want` (..., fragile): steps equal and the outputs within TOL on the rays that
    are not fragile; returns the share of fragile rays."""
    rgb, acc, dist, steps = got
    w_rgb, w_acc, w_dist, w_steps, fragile = want
    ok = ~fragile
    assert np.array_equal(steps[ok], w_steps[ok]), (what, np.nonzero(ok & (steps != w_steps))[0][:8])
    e_rgb, e_acc = np.abs(rgb[ok] - w_rgb[ok]).max(), np.abs(acc[ok] - w_acc[ok]).max()
    e_dist = (np.abs(dist[ok] - w_dist[ok]) / np.maximum(1.0, far[ok])).max()
    print(f"{what}: max |err| rgb {e_rgb:.3e} acc {e_acc:.3e} distance / max(1, far) {e_dist:.3e}, fragile {int(fragile.sum())} of {fragile.size}")
    assert e_rgb <= TOL["rgb"] and e_acc <= TOL["acc"] and e_dist <= TOL["distance"], what
    return fragile.mean()


# ---- the seventh library: declarations, bindings, exports, checks -------------------------------------------------------------------
def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "mipnerf_preview_360.h")).read(), flags=re.S)


def test_header_bindings_and_dynamic_symbols_are_one_set(lib):
    declared = sorted(set(re.findall(r"\b(mipnerf_[a-z0-9_]+)\s*\(", _header())))
    assert declared == sorted(L.PREVIEW_360_SIGNATURES) == ["mipnerf_preview_360_abi_version", "mipnerf_preview_360_last_error",
                                                             "mipnerf_preview_360_march", "mipnerf_preview_360_march_sparse"]
    out = subprocess.run(["nm", "-D", "--defined-only", L.PREVIEW_360_LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert sorted(line.split()[-1] for line in out.splitlines() if line.strip()) == declared
    for name, (_, args) in L.PREVIEW_360_SIGNATURES.items():
        proto = re.search(r"\b" + name + r"\s*\(([^)]*)\)", _header()).group(1).strip()
        count = 0 if proto in ("", "void") else proto.count(",") + 1
        assert count == len(args), (name, proto)
    assert lib.mipnerf_preview_360_abi_version() == 1 == L.PREVIEW_360_ABI


def test_the_other_libraries_keep_their_entry_points():
    assert len(L.PREVIEW_360_SIGNATURES) == 4 and not set(L.PREVIEW_360_SIGNATURES) & (
        set(L.SIGNATURES) | set(L.PREVIEW_SIGNATURES) | set(L.PREVIEW_MIP_SIGNATURES) | set(L.PREVIEW_SPARSE_SIGNATURES) | set(L.PREVIEW_TUNE_SIGNATURES))
    assert len(L.SIGNATURES) == 93 and len(L.PREVIEW_SIGNATURES) == 4 and len(L.PREVIEW_MIP_SIGNATURES) == 3
    assert len(L.PREVIEW_SPARSE_SIGNATURES) == 7 and len(L.PREVIEW_TUNE_SIGNATURES) == 4
    for table in (L.SIGNATURES, L.PREVIEW_SIGNATURES, L.PREVIEW_MIP_SIGNATURES, L.PREVIEW_SPARSE_SIGNATURES, L.PREVIEW_TUNE_SIGNATURES):
        assert not any("360_march" in n or "preview_360" in n for n in table)


def test_the_build_registers_the_library_with_no_contraction():
    from mipnerf_pl_amd import build
    assert [u for u, _ in build.PREVIEW_360_UNITS] == ["kernels_preview_360.hip", "preview_360_capi.hip"]
    assert all("-ffp-contract=off" in f for _, f in build.PREVIEW_360_UNITS)
    assert os.path.basename(build.PREVIEW_360_LIB) == "libmipnerf_preview_360.so"


def _field(dims=pf.DIMS, lo=pf.LO, hi=pf.HI, degree=1, rows=0x1000, occ=None):
    return L.PreviewField((C.c_int32 * 3)(*dims), (C.c_float * 3)(*lo), (C.c_float * 3)(*hi), degree, rows, occ)


def _params(step_scale=0.5, t_min=0.0, max_steps=64, background=(1.0, 1.0, 1.0)):
    return L.PreviewParams(step_scale, t_min, max_steps, (C.c_float * 3)(*background))


def test_every_entry_point_validates_before_any_hip_call(lib):
    """No device here: a call that reached the HIP runtime would fail with code 3, not with 1 / 2 and a message naming the entry point."""
    P = 0x1000        # never dereferenced: the checks come first

    def march(field, params, R=8.0, n=4, ptrs=(P,) * 7):
        return lib.mipnerf_preview_360_march(C.byref(field) if field is not None else None, R, C.byref(params) if params is not None else None,
                                             n, *ptrs, None, None)

    def sparse(field, params, R=8.0, n=4, ptrs=(P,) * 7, table=0x2000, n_rows=10):
        s = L.PreviewSparseField(field, table, n_rows)
        return lib.mipnerf_preview_360_march_sparse(C.byref(s), R, C.byref(params), n, *ptrs, None, None)

    bad = [
        (lambda: march(None, _params()), L.E_INVALID), (lambda: march(_field(), None), L.E_INVALID),
        (lambda: march(_field(rows=None), _params()), L.E_INVALID), (lambda: march(_field(dims=(1, 9, 10)), _params()), L.E_INVALID),
        (lambda: march(_field(dims=(1024, 1024, 1024)), _params()), L.E_INVALID),
        (lambda: march(_field(hi=(pf.LO[0], 2.0, 1.8)), _params()), L.E_INVALID),
        (lambda: march(_field(degree=3), _params()), L.E_UNSUPPORTED),
        (lambda: march(_field(), _params(), R=1.0), L.E_INVALID), (lambda: march(_field(), _params(), R=0.5), L.E_INVALID),
        (lambda: march(_field(), _params(), R=float("inf")), L.E_INVALID), (lambda: march(_field(), _params(), R=float("nan")), L.E_INVALID),
        (lambda: march(_field(), _params(step_scale=0.0)), L.E_INVALID), (lambda: march(_field(), _params(max_steps=0)), L.E_INVALID),
        (lambda: march(_field(), _params(t_min=1.0)), L.E_INVALID), (lambda: march(_field(), _params(), n=-1), L.E_INVALID),
        (lambda: march(_field(), _params(), ptrs=(P, P, None, P, P, P, P)), L.E_INVALID),
        (lambda: march(_field(rows=0x1008), _params()), L.E_INVALID),
        (lambda: sparse(_field(occ=0x3000), _params(), R=1.0), L.E_INVALID),
        (lambda: sparse(_field(occ=None), _params()), L.E_INVALID), (lambda: sparse(_field(occ=0x3000), _params(), table=None), L.E_INVALID),
        (lambda: sparse(_field(occ=0x3000), _params(), table=0x2004), L.E_INVALID),
        (lambda: sparse(_field(occ=0x3000), _params(), n_rows=-1), L.E_INVALID),
        (lambda: sparse(_field(occ=0x3000), _params(), n_rows=9 * 10 * 11 + 1), L.E_INVALID),
        (lambda: sparse(_field(occ=0x3000, degree=5), _params()), L.E_UNSUPPORTED),
    ]
    for call, code in bad:
        assert call() == code
        assert lib.mipnerf_preview_360_last_error().decode().startswith("preview_360_march")
    assert march(_field(), _params(), n=0, ptrs=(None,) * 7) == 0          # n_rays == 0 is ok whatever the ray pointers
    assert sparse(_field(occ=0x3000), _params(), n=0, ptrs=(None,) * 7) == 0


# ---- the host build against the fixture ----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rays():
    return pf.scene_rays()


def test_the_scene_has_the_rays_it_promises(hm, rays):
    o, d, tn, tf = rays
    assert o.shape == (pf.N_RAYS, 3) and pf.N_RAYS == 270
    hits = [pf.Ray(o[b], d[b], tn[b], tf[b], pf.FAR_RADIUS) for b in range(pf.N_RAYS)]
    consts = np.zeros(10, F)                                        # the header's C2 / C3 agree with the fixture's on every ray
    for b, r in enumerate(hits):
        assert bool(hm.hm_preview360_ray(C.c_float(pf.FAR_RADIUS), _p(o[b]), _p(d[b]), C.c_float(tn[b]), C.c_float(tf[b]), _p(consts))) == r.hit
        if r.hit:
            want = np.array([r.len, r.tc, r.p2, r.p, r.c, r.ts, r.la - r.tc, r.lb - r.tc, r.wa, r.wb])
            assert np.abs(consts - want).max() <= 2e-6 * max(1.0, float(np.abs(want).max())), b
    assert [r.hit for r in hits[pf.N_SEEDED:]] == [True] * 3 + [False] * 10
    assert sum(r.hit for r in hits[:pf.N_SEEDED]) >= 250
    centre, below, above = hits[pf.N_SEEDED:pf.N_SEEDED + 3]
    assert centre.p < 1e-6 and 0.0 < below.ts < 0.1 and above.ts == 0.0
    assert {round(float(np.linalg.norm(v)), 3) for v in d[:pf.N_SEEDED]} == {0.5, 1.0, 2.0}


@pytest.mark.parametrize("with_occupancy", [False, True])
@pytest.mark.parametrize("degree", [0, 1, 2])
def test_host_build_matches_the_fixture(hm, rays, degree, with_occupancy):
    rows, sigma = pf.random_rows(degree, hollow=with_occupancy)
    occ = pf.occupancy_words(sigma) if with_occupancy else None
    for step_scale, t_min, max_steps in ((0.5, 0.0, 4096), (0.1, 1e-3, 4096)):
        want = pf.march(rows, pf.LO, pf.HI, degree, pf.FAR_RADIUS, *rays, step_scale, t_min, max_steps, BG, occ)
        got = host_march(hm, rows, degree, rays, step_scale, t_min, max_steps, BG, occ)
        share = compare(got, want, rays[3], f"degree {degree} occupancy {with_occupancy} step {step_scale}")
        assert share <= FRAGILE_CAP
        assert (want[3] > 0).sum() > 150                      # the comparison is not about empty rays
        if with_occupancy:
            free = pf.march(rows, pf.LO, pf.HI, degree, pf.FAR_RADIUS, *rays, step_scale, t_min, max_steps, BG, None)
            assert (want[3] < free[3]).any()                  # the grid skips samples somewhere


def test_a_miss_is_written_as_rule_2_writes_it(hm, rays):
    rows, _ = pf.random_rows(1)
    rgb, acc, dist, steps = host_march(hm, rows, 1, rays, 0.5, 0.0, 4096, BG)
    o, d, tn, tf = rays
    for b in range(pf.N_SEEDED + 3, pf.N_RAYS):
        assert np.array_equal(rgb[b], np.array(BG, F)) and acc[b] == 0.0 and steps[b] == 0
        assert dist[b] == (tn[b] if np.isfinite(tn[b]) else tf[b] if np.isfinite(tf[b]) else 0.0)


# ---- the warp ------------------------------------------------------------------------------------------------------------------------
def _probe_rays():
    """origins and unit directions with p from 0 to beyond P_FLAT: through the centre, close to it, at |m| = 0.5, 1, 2, P_FLAT +- 1e-3, 3, 6"""
    e, q = pf.UNIT_E, pf.UNIT_Q
    return [(p * q - 4.0 * e, e) for p in (0.0, 1e-7, 1e-4, 0.5, 1.0, 2.0, pf.P_FLAT - 1e-3, pf.P_FLAT + 1e-3, 3.0, 6.0)]


def test_the_inverse_warp_returns_the_arclength(hm):
    tau = np.concatenate([np.linspace(-8.0, 8.0, 4001), [-1e-6, 0.0, 1e-6]]).astype(F)
    for o, u in _probe_rays():
        w, back = np.zeros_like(tau), np.full_like(tau, np.nan)
        hm.hm_preview360_roundtrip(C.c_float(64.0), _p(o.astype(F)), _p(u.astype(F)), C.c_float(-50.0), C.c_float(50.0), tau.size, _p(tau), _p(w),
                                   _p(back))
        assert np.all(np.diff(w[:4001]) >= 0.0)                # W does not decrease
        assert np.array_equal(w[:4001], -w[:4001][::-1])      # and is odd
        err = np.abs(back - tau) / np.maximum(1.0, np.abs(tau))
        assert err.max() <= 1e-5, (float(np.linalg.norm(o)), float(err.max()))
        r = pf.Ray(o.astype(F), u.astype(F), -50.0, 50.0, 64.0)
        assert np.abs(w - r.W(tau.astype(np.float64))).max() <= 2e-6 * max(1.0, float(np.abs(w).max()))      # the fixture states the same W


def test_consecutive_samples_stay_within_one_step_and_the_count_follows_the_arclength(hm, rays):
    o, d, tn, tf = rays
    long_rays = singles = 0
    for step_scale in (0.5, 0.1):
        s = pf.lattice_step(pf.DIMS, pf.LO, pf.HI, step_scale)
        worst_step, worst_ratio = 0.0, 0.0
        for b in range(pf.N_RAYS):
            n, z, t, delta = host_samples(hm, o[b], d[b], tn[b], tf[b], s)
            ray = pf.Ray(o[b], d[b], tn[b], tf[b], pf.FAR_RADIUS)
            assert (n >= 0) == ray.hit
            if n < 0:
                continue
            # C4: every hit ray has a sample and the deltas partition [la, lb], also on a ray with the one midpoint sample
            assert n >= 1, b
            singles += n == 1
            assert abs(float(delta.astype(np.float64).sum()) - (ray.lb - ray.la)) <= 1e-5 * (ray.lb - ray.la), b
            if n < 2:
                continue
            worst_step = max(worst_step, float(np.linalg.norm(np.diff(z.astype(np.float64), axis=0), axis=1).max()) / s)
            # the contracted arclength of [la, lb], in float64 on a polyline 16 times finer than the march
            fine = pf.contract(ray.o + ((ray.tc + ray.V(np.linspace(ray.wa, ray.wb, 16 * n + 1))) / ray.len)[:, None] * ray.d)
            length = float(np.linalg.norm(np.diff(fine, axis=0), axis=1).sum())
            if length > 10.0 * s:
                long_rays += 1
                worst_ratio = max(worst_ratio, n * s / length)
            assert np.all(np.diff(t) > 0.0)
        print(f"step_scale {step_scale}: largest contracted step {worst_step:.5f} s, largest samples * s / arclength {worst_ratio:.3f}")
        assert worst_step <= 1.0 + 1e-4
        assert worst_ratio <= 1.5
    assert long_rays > 300 and singles >= 1          # the scene holds rays of a single sample (shorter than 1.5 steps)


def test_inside_the_unit_ball_the_march_is_the_bounded_one(hm):
    """A segment inside the unit ball: contract is the identity and W' = 1, so with a length that is a whole number of steps (the
    bounded march gives its last sample a whole step as well) both fixtures and the host build agree on the same rows."""
    rng = np.random.default_rng(3)
    s = pf.lattice_step(pf.DIMS, pf.LO, pf.HI, 0.5)
    B = 32
    o = rng.normal(size=(B, 3))
    o *= (rng.uniform(0.0, 0.3, (B, 1)) / np.linalg.norm(o, axis=-1, keepdims=True))
    d = rng.normal(size=(B, 3))
    d *= rng.choice([0.5, 1.0, 2.0], (B, 1)) / np.linalg.norm(d, axis=-1, keepdims=True)
    o, d = o.astype(F), d.astype(F)
    length = np.linalg.norm(d.astype(np.float64), axis=-1)
    tn = np.full(B, 0.05, F)
    tf = (tn + rng.integers(1, 4, B) * s / length).astype(F)          # 1 .. 3 whole steps: the segment ends inside |x| < 0.3 + 0.1 + 0.6
    rays = (o, d, tn, tf)
    for degree in (0, 2):
        rows, _ = pf.random_rows(degree)
        want = bounded.march(rows, pf.LO, pf.HI, degree, *rays, 0.5, 0.0, 4096, BG)
        assert not want[4].any() and (want[3] > 0).all()
        mine = pf.march(rows, pf.LO, pf.HI, degree, pf.FAR_RADIUS, *rays, 0.5, 0.0, 4096, BG)
        for got, name in ((mine[:4], "fixture"), (host_march(hm, rows, degree, rays, 0.5, 0.0, 4096, BG), "host build")):
            compare(got, want, tf, f"inside the unit ball, degree {degree}, {name} against the bounded fixture")


# ---- Python: refusals and the .npz round trip ----------------------------------------------------------------------------------------
def _cpu_field(degree=1, space=None, far_radius=None, occupancy=True):
    from mipnerf_pl_amd.ops import Occupancy
    rows, sigma = pf.random_rows(degree, hollow=True)
    occ = None
    if occupancy:
        words = torch.from_numpy(pf.occupancy_words(sigma).view(np.int32)).view(torch.uint32)
        occ = Occupancy(words, pf.DIMS, pf.LO, pf.HI, space=space)
        occ.threshold, occ.dilate = 0.0, 0
    return pv.BakedField(torch.from_numpy(rows), pf.DIMS, pf.LO, pf.HI, degree, occ, 0.0 if occupancy else None, space=space,
                         far_radius=far_radius)


def test_fields_carry_their_space_and_bounded_files_keep_their_keys(tmp_path):
    plain = _cpu_field()
    assert plain.space is None and plain.far_radius is None
    path = plain.save(str(tmp_path / "plain.npz"))
    with np.load(path) as z:
        assert sorted(z.files) == ["degree", "dilate", "dims", "hi", "lo", "occupancy", "rows", "threshold"]
    assert pv.BakedField.stored_space(path) is None
    field = _cpu_field(space="contracted", far_radius=8.0)
    path = field.save(str(tmp_path / "c.npz"))
    with np.load(path) as z:
        assert sorted(z.files) == ["degree", "dilate", "dims", "far_radius", "hi", "lo", "occupancy", "rows", "space", "threshold"]
    assert pv.BakedField.stored_space(path) == "contracted"
    back = pv.BakedField.load(path, "cpu")
    assert back.space == "contracted" and back.far_radius == 8.0 and back.occupancy.space == "contracted"
    assert torch.equal(back.rows, field.rows) and torch.equal(back.occupancy.bits.view(torch.int32), field.occupancy.bits.view(torch.int32))
    for kw in (dict(space="world", far_radius=8.0), dict(space="contracted"), dict(space="contracted", far_radius=1.0),
               dict(space="contracted", far_radius=float("inf")), dict(far_radius=8.0)):
        with pytest.raises(ValueError):
            _cpu_field(**kw)


def test_sparse_fields_carry_their_space(tmp_path):
    field = _cpu_field(space="contracted", far_radius=8.0)
    table, m = pv.table_of_points(pv.baked_points(field.occupancy))
    rows = field.rows.reshape(-1, field.rows.shape[-1])[pv.baked_points(field.occupancy).reshape(-1)].contiguous()
    sparse = pv.SparseField(rows, table, pf.DIMS, pf.LO, pf.HI, 1, field.occupancy, 0.0, space="contracted", far_radius=8.0)
    path = sparse.save(str(tmp_path / "s.npz"))
    with np.load(path) as z:
        assert "space" in z.files and "far_radius" in z.files
    back = pv.SparseField.load(path, "cpu")
    assert back.space == "contracted" and back.far_radius == 8.0 and torch.equal(back.rows, sparse.rows)
    dense = back.to_dense()
    assert dense.space == "contracted" and dense.far_radius == 8.0
    plain = pv.SparseField(rows, table, pf.DIMS, pf.LO, pf.HI, 1, _cpu_field().occupancy, 0.0)
    with np.load(plain.save(str(tmp_path / "p.npz"))) as z:
        assert sorted(z.files) == ["degree", "dilate", "dims", "hi", "lo", "occupancy", "sparse_rows", "table", "threshold"]


def test_what_is_not_implemented_for_a_contracted_lattice_says_so():
    field = _cpu_field(space="contracted", far_radius=8.0)
    t = torch.zeros(4, 3)
    with pytest.raises(NotImplementedError, match="contracted"):
        pv.BakedPyramid([field])
    with pytest.raises(NotImplementedError, match="contracted"):
        pv.march_grad(field, t, t, t[:, 0], t[:, 0], (1.0, 1.0, 1.0), grad_rgb=t)
    with pytest.raises(NotImplementedError, match="contracted"):
        pv.tune_field(field, lambda k: None, 1)
    with pytest.raises(NotImplementedError, match="contracted"):
        pv.TuneState(field)
    fake = pv.BakedPyramid.__new__(pv.BakedPyramid)          # the constructor refuses such levels itself
    fake.levels = [field]
    with pytest.raises(NotImplementedError, match="contracted"):
        pv.march_pyramid(fake, t, t, t[:, 0], t[:, 0], t[:, 0], (1.0, 1.0, 1.0))
    unbounded = SimpleNamespace(unbounded=True, num_levels=2)
    with pytest.raises(NotImplementedError, match="contracted pyramid"):
        pv.bake_pyramid(unbounded, grid=8, space="contracted", far_radius=8.0)


def test_models_are_refused_as_before_without_space_and_by_kind_with_it():
    unbounded, bounded_model = SimpleNamespace(unbounded=True, num_levels=2), SimpleNamespace(unbounded=False, num_levels=2)
    for call in (lambda: pv.bake_field(unbounded, grid=8, lo=-1, hi=1), lambda: pv.bake_pyramid(unbounded, grid=8, lo=-1, hi=1),
                 lambda: pv.refuse_model(unbounded, "preview")):
        with pytest.raises(NotImplementedError, match=r"unbounded=True models are not supported \(their field lives in a contracted space; a "
                                                      r"contracted lattice is not implemented\)"):
            call()
    pv.refuse_model(unbounded, "preview", "contracted")
    with pytest.raises(ValueError, match="this model is bounded"):
        pv.bake_field(bounded_model, grid=8, space="contracted", far_radius=8.0)
    with pytest.raises(NotImplementedError, match="two-level"):
        pv.bake_field(SimpleNamespace(unbounded=True, num_levels=3), grid=8, space="contracted", far_radius=8.0)
    with pytest.raises(ValueError, match="far_radius"):
        pv.bake_field(unbounded, grid=8, space="contracted")
    with pytest.raises(ValueError, match="far_radius belongs to space='contracted'"):
        pv.bake_field(bounded_model, grid=8, lo=-1, hi=1, far_radius=8.0)
    with pytest.raises(ValueError, match="space must be None or 'contracted'"):
        pv.bake_field(unbounded, grid=8, space="world", far_radius=8.0)


def _system(dataset_name, unbounded):
    return SimpleNamespace(hparams={"dataset_name": dataset_name}, mip_nerf=SimpleNamespace(unbounded=unbounded, num_levels=2))


def test_the_command_refuses_before_any_device_work(tmp_path):
    with pytest.raises(SystemExit, match="captured scene.*--space contracted"):
        pv.refuse_checkpoint(_system("realdata360", True))
    with pytest.raises(SystemExit, match="bounded model"):
        pv.refuse_checkpoint(_system("blender", False), space="contracted")
    with pytest.raises(SystemExit, match="bounded model"):
        pv.refuse_checkpoint(_system("llff", False), "contracted")
    pv.refuse_checkpoint(_system("realdata360", True), space="contracted")
    pv.refuse_checkpoint(_system("llff", True), "contracted")
    pv.refuse_checkpoint(_system("blender", False))

    def parse(*extra):
        return pv.build_parser().parse_args(["--ckpt", "c.ckpt", "--out_dir", str(tmp_path)] + list(extra))
    args = parse("--space", "contracted", "--data", "d", "--far_radius", "30", "--sparse", "--compare")
    pv.refuse_arguments(args)
    assert args.split == "test" and args.n_views == 30 and args.factor is None          # the defaults of --space contracted
    for extra, what in ((("--space", "contracted", "--data", "d", "--mip"), "--mip"), (("--space", "contracted", "--data", "d", "--tune", "3"), "--tune"),
                        (("--space", "contracted"), "give --data"), (("--far_radius", "8"), "--far_radius belongs to --space"),
                        (("--split", "train"), "--split belongs to --space"), (("--n_views", "6"), "--n_views belongs to --space"),
                        (("--factor", "2"), "--factor belongs to --space"),
                        (("--space", "contracted", "--data", "d", "--far_radius", "1"), "finite and > 1"),
                        (("--space", "contracted", "--data", "d", "--bound", "3"), "ends at 2")):
        with pytest.raises(SystemExit, match=what):
            pv.refuse_arguments(parse(*extra))
    with pytest.raises(SystemExit):
        parse("--space", "world")
    plain, contracted = str(tmp_path / "plain.npz"), str(tmp_path / "c.npz")
    _cpu_field().save(plain)
    _cpu_field(space="contracted", far_radius=8.0).save(contracted)
    with pytest.raises(SystemExit, match="drop --space"):
        pv.refuse_baked_space(parse("--space", "contracted", "--data", "d", "--baked", plain))
    with pytest.raises(SystemExit, match="give --space contracted"):
        pv.refuse_baked_space(parse("--baked", contracted))
    pv.refuse_baked_space(parse("--baked", plain))
    pv.refuse_baked_space(parse("--space", "contracted", "--data", "d", "--baked", contracted))
