"""CPU (no GPU): the proposal density of the unbounded-scene model -- rules Q1 - Q4 that csrc/lattice_sample_360.hpp states for host and
device (built with g++ -O2 -ffp-contract=off from tests/hostmath/proposal360.cpp) against tests/proposal360_fixture.py: bit for bit
against the float32 restatement, within a derived bound against the float64 one, L = 1 bit for bit the single-lattice lookup; the tenth
library's declarations, bindings, exports and argument checks without a device; the build units; the Python names."""
import ctypes as C
import inspect
import os
import re
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest

import proposal360_fixture as qx
import proposal_fixture as px
from mipnerf_pl_amd import _lib as L

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
CSRC = os.path.join(REPO, "mipnerf_pl_amd", "csrc")
F = np.float32
LO, HI = qx.LO, qx.HI
FOOTPRINTS = (1.0, 0.5, 2.0)


def _build(src, so, hdrs):
    src, so = os.path.join(HERE, "hostmath", src), os.path.join(HERE, "hostmath", so)
    hdrs = [os.path.join(CSRC, h) for h in hdrs]
    if (not os.path.exists(so)) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in [src] + hdrs):
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", src, "-o", so])
    return C.CDLL(so)


@pytest.fixture(scope="module")
def hm():
    return _build("proposal360.cpp", "_proposal360.so", ("raymath.hpp", "raymath360.hpp", "lattice_sample.hpp", "preview_march.hpp",
                                                         "preview_mip.hpp", "lattice_sample_360.hpp"))


@pytest.fixture(scope="module")
def hm1():
    """the existing host build of the single-lattice lookup (tests/test_proposal_cpu.py)"""
    return _build("proposal.cpp", "_proposal.so", ("raymath.hpp", "lattice_sample.hpp"))


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _pyramid_args(lattices, lo, hi):
    lats = [np.ascontiguousarray(g, F) for g in lattices]
    dims = np.ascontiguousarray([(g.shape[2], g.shape[1], g.shape[0]) for g in lats], np.int32)
    ptrs = (C.c_void_p * len(lats))(*[g.ctypes.data for g in lats])
    return lats, dims, ptrs, np.asarray(lo, F), np.asarray(hi, F)


def host_spacing(hm, lattices, lo=LO, hi=HI):
    lats, dims, ptrs, lo, hi = _pyramid_args(lattices, lo, hi)
    out = np.zeros(len(lats), F)
    hm.hm_pyramid_spacing(len(lats), _p(dims), ptrs, _p(lo), _p(hi), _p(out))
    return out


def host_density(hm, lattices, footprint, mean, cov, lo=LO, hi=HI):
    lats, dims, ptrs, lo, hi = _pyramid_args(lattices, lo, hi)
    mean, cov = np.ascontiguousarray(mean, F).reshape(-1, 3), np.ascontiguousarray(cov, F).reshape(-1, 6)
    n = mean.shape[0]
    out, lvl, g = np.full(n, -7.0, F), np.full(n, -1, np.int32), np.full(n, -7.0, F)
    hm.hm_pyramid_density(len(lats), _p(dims), ptrs, _p(lo), _p(hi), C.c_float(footprint), C.c_longlong(n), _p(mean), _p(cov), _p(out), _p(lvl),
                          _p(g))
    return out, lvl, g


def host_density_sample(hm, lattices, footprint, t0, t1, o, d, radius, lo=LO, hi=HI):
    lats, dims, ptrs, lo, hi = _pyramid_args(lattices, lo, hi)
    a = [np.ascontiguousarray(x, F) for x in (t0, t1, o, d, radius)]
    n = a[0].shape[0]
    out = np.full(n, -7.0, F)
    hm.hm_pyramid_density_sample(len(lats), _p(dims), ptrs, _p(lo), _p(hi), C.c_float(footprint), C.c_longlong(n), *[_p(x) for x in a], _p(out))
    return out


def host_gauss(hm, t0, t1, o, d, radius):
    a = [np.ascontiguousarray(x, F) for x in (t0, t1, o, d, radius)]
    n = a[0].shape[0]
    mean, cov = np.zeros((n, 3), F), np.zeros((n, 6), F)
    hm.hm_gauss_contracted(C.c_longlong(n), *[_p(x) for x in a], _p(mean), _p(cov))
    return mean, cov


def same_bits(a, b):
    """bit for bit, a NaN matching any NaN (its payload is not part of the rule)"""
    a, b = np.asarray(a, F), np.asarray(b, F)
    nan = np.isnan(a)
    return a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.uint32), b[~nan].view(np.uint32))


def _cases(lattices, footprint, seed):
    """(mean, cov): every footprint case of the fixture at random means inside the ball of radius 2"""
    cov = qx.covariances_for(qx.spacings(lattices, LO, HI), footprint, seed)
    rng = np.random.default_rng(seed + 1)
    mean = rng.normal(size=(len(cov), 3))
    mean = (mean / np.linalg.norm(mean, axis=1, keepdims=True) * (1.999 * rng.random((len(cov), 1)) ** (1 / 3))).astype(F)
    return mean, cov


# ---- the rule ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(qx.PYRAMIDS))
def test_spacings_are_the_largest_axis_spacing_in_float32(hm, name):
    lattices = qx.random_pyramid(name, seed=1)
    got = host_spacing(hm, lattices)
    assert same_bits(got, qx.spacings(lattices, LO, HI)) and (np.diff(got) > 0).all()
    if name == "L2":                                       # (5, 7, 9): nz = 5 is the coarsest axis
        assert got[0] == F(4.0) / F(4.0) and got[1] == F(4.0) / F(2.0)
    if name == "L4":
        assert got.tolist() == [0.125, 0.25, 0.5, 1.0]


@pytest.mark.parametrize("footprint", FOOTPRINTS)
@pytest.mark.parametrize("name", list(qx.PYRAMIDS))
def test_host_function_equals_the_float32_restatement_bit_for_bit(hm, name, footprint):
    lattices = qx.random_pyramid(name, seed=3)
    mean, cov = _cases(lattices, footprint, seed=len(lattices))
    got, lvl, g = host_density(hm, lattices, footprint, mean, cov)
    want, wl, wg = qx.pyramid_f32(lattices, LO, HI, footprint, mean, cov)
    assert np.array_equal(lvl, wl) and same_bits(g, wg)
    assert same_bits(got, want) and (got >= 0).all()
    n = len(lattices)
    assert set(np.unique(lvl)) == set(range(n))                                      # every level is selected
    if n > 1:
        for k in range(n - 1):
            assert ((lvl == k) & (g > 0)).any(), k                                   # and every pair of levels is mixed
        assert ((lvl == n - 1) & (g == 0)).any() and ((lvl == 0) & (g == 0)).any()
    else:
        assert (g == 0).all()


def test_a_footprint_exactly_on_a_spacing_reads_that_level_alone(hm):
    """L4 over [-2, 2]^3: spacings 2^-3 .. 2^0, and cov_xx = (s / 2)^2 gives w = 2 sqrt(cov_xx) = s without rounding"""
    lattices = qx.random_pyramid("L4", seed=5)
    s = qx.spacings(lattices, LO, HI)
    cov = np.zeros((4, 6), F)
    cov[:, 0] = (s / F(2)) ** 2
    assert np.array_equal(qx.footprint_f32(1.0, cov), s)
    mean = np.array([[0.3, -1.1, 0.7]] * 4, F)
    got, lvl, g = host_density(hm, lattices, 1.0, mean, cov)
    assert lvl.tolist() == [0, 1, 2, 3] and (g == 0).all()
    want = [px.trilinear_f32(lattices[k], LO, HI, mean[k:k + 1])[0] for k in range(4)]
    assert same_bits(got, np.asarray(want, F))
    # off-diagonal entries are not part of the yardstick
    cov[:, [1, 2, 4]] = 9.0
    assert same_bits(host_density(hm, lattices, 1.0, mean, cov)[0], got)


@pytest.mark.parametrize("name", list(qx.PYRAMIDS))
def test_footprint_zero_and_a_nan_covariance_read_level_zero(hm, name):
    lattices = qx.random_pyramid(name, seed=7)
    mean, cov = _cases(lattices, 1.0, seed=9)
    plain = px.trilinear_f32(lattices[0], LO, HI, mean)
    got, lvl, g = host_density(hm, lattices, 0.0, mean, cov)
    assert (lvl == 0).all() and (g == 0).all() and same_bits(got, plain)
    bad = cov.copy()
    bad[::3, 0], bad[1::3, 3], bad[2::3, 5] = np.nan, np.nan, -1e30               # NaN entries; a negative trace: sqrtf gives NaN
    got, lvl, g = host_density(hm, lattices, 1.0, mean, bad)
    assert (lvl == 0).all() and (g == 0).all() and same_bits(got, plain)
    assert same_bits(qx.pyramid_f32(lattices, LO, HI, 1.0, mean, bad)[0], plain)
    huge = cov.copy()
    huge[:, 0] = np.inf                                                              # w = inf: the last level
    got, lvl, g = host_density(hm, lattices, 1.0, mean, huge)
    assert (lvl == len(lattices) - 1).all() and same_bits(got, px.trilinear_f32(lattices[-1], LO, HI, mean))


@pytest.mark.parametrize("name", list(qx.PYRAMIDS))
def test_a_non_finite_mean_gives_zero(hm, name):
    lattices = [np.full_like(g, np.nan) for g in qx.random_pyramid(name, seed=11)]   # anything loaded would show
    mean = px.nonfinite_points(LO, HI)
    cov = np.resize(qx.covariances_for(qx.spacings(lattices, LO, HI), 1.0, seed=2, per_case=1), (len(mean), 6))
    got, _, _ = host_density(hm, lattices, 1.0, mean, cov)
    assert (got == 0).all() and same_bits(got, qx.pyramid_f32(lattices, LO, HI, 1.0, mean, cov)[0])


def test_a_nan_corner_propagates_from_the_level_that_holds_it_only(hm):
    lattices = qx.random_pyramid("L2", seed=13)
    s = qx.spacings(lattices, LO, HI)
    mean = np.array([[0.1, 0.2, 0.3]] * 3, F)
    cov = np.zeros((3, 6), F)
    cov[:, 3] = [(0.25 * s[0]) ** 2, ((s[0] + s[1]) / 4) ** 2, (0.75 * s[1]) ** 2]    # below s_0, between the two, above s_1
    lower = [g.copy() for g in lattices]
    lower[0][:] = np.nan
    got, lvl, g = host_density(hm, lower, 1.0, mean, cov)
    assert lvl.tolist() == [0, 0, 1] and g[0] == 0 and 0 < g[1] < 1 and g[2] == 0
    assert np.isnan(got[0]) and np.isnan(got[1]) and not np.isnan(got[2])
    upper = [g.copy() for g in lattices]
    upper[1][:] = np.nan
    got, _, _ = host_density(hm, upper, 1.0, mean, cov)
    assert not np.isnan(got[0]) and np.isnan(got[1]) and np.isnan(got[2])            # g == 0 at level 0: the upper level is not read
    for lat in (lower, upper):
        assert same_bits(host_density(hm, lat, 1.0, mean, cov)[0], qx.pyramid_f32(lat, LO, HI, 1.0, mean, cov)[0])


@pytest.mark.parametrize("shape", [(2, 2, 2), (5, 7, 9), (33, 33, 33)])
def test_one_level_is_the_single_lattice_lookup_bit_for_bit(hm, hm1, shape):
    lo, hi = (-1.5, -0.7, 0.25), (2.25, 1.3, 4.0)
    lat = px.random_lattice(shape, seed=sum(shape))
    pts = np.concatenate([px.box_points(lo, hi, seed=1), px.nonfinite_points(lo, hi)])
    cov = np.abs(np.random.default_rng(0).normal(size=(len(pts), 6))).astype(F) * F(10)
    got, lvl, g = host_density(hm, [lat], 1.0, pts, cov, lo, hi)
    want = np.full(len(pts), -7.0, F)
    lat32, lo32, hi32, p32 = np.ascontiguousarray(lat, F), np.asarray(lo, F), np.asarray(hi, F), np.ascontiguousarray(pts, F)
    hm1.hm_lattice_trilinear(_p(lat32), shape[2], shape[1], shape[0], _p(lo32), _p(hi32), C.c_longlong(len(pts)), _p(p32), _p(want))
    assert same_bits(got, want) and (lvl == 0).all() and (g == 0).all()


def _rays(seed=0):
    """(t0, t1, o, d, radius): random rays from |o| ~ 0.5 .. 3 with t up to 1e4; means inside the unit ball; a sample whose mean has
    |mean|^2 just above 1; a ray through the origin; radius 0"""
    rng = np.random.default_rng(seed)
    n = 600
    o = rng.normal(size=(n, 3)) * rng.uniform(0.2, 1.5, (n, 1))
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    t0 = 10.0 ** rng.uniform(-2, 4, n)
    t1 = np.minimum(t0 * (1.0 + 10.0 ** rng.uniform(-3, 0.5, n)), 1e4 * 1.0001)
    radius = 10.0 ** rng.uniform(-4, -2, n)
    radius[::7] = 0.0
    # inside the unit ball: short samples near a small origin
    o[:60] *= 0.3
    t0[:60], t1[:60] = rng.uniform(0.0, 0.2, 60), rng.uniform(0.2, 0.4, 60)
    # through the origin
    o[60:70] = -d[60:70] * rng.uniform(0.5, 3.0, (10, 1))
    # |mean|^2 just above 1: a thin sample centred at distance 1 + tiny from the origin along a ray that starts at the origin
    o[70:80] = 0.0
    t0[70:80], t1[70:80] = 1.0, 1.0 + 2.0 ** -20 * np.arange(1, 11)
    return [np.ascontiguousarray(a, F) for a in (t0, t1, o, d, radius)]


@pytest.mark.parametrize("name", list(qx.PYRAMIDS))
def test_the_sample_function_is_the_contracted_gaussian_then_the_rule(hm, name):
    lattices = qx.random_pyramid(name, seed=17)
    t0, t1, o, d, radius = _rays()
    mean, cov = host_gauss(hm, t0, t1, o, d, radius)
    n2 = (mean.astype(np.float64) ** 2).sum(-1)
    world = (o.astype(np.float64) + d * ((t0.astype(np.float64) + t1) / 2)[:, None])
    wn2 = (world ** 2).sum(-1)
    assert (n2 < 4.0).all() and (wn2 < 1.0).any() and ((wn2 > 1.0) & (wn2 < 1.0 + 1e-4)).any() and (wn2 > 1e6).any()
    assert (radius == 0).any() and float(t1.max()) >= 1e4
    for footprint in (1.0, 4.0):
        got = host_density_sample(hm, lattices, footprint, t0, t1, o, d, radius)
        two_step, lvl, _ = host_density(hm, lattices, footprint, mean, cov)
        assert same_bits(got, two_step)
        assert same_bits(got, qx.pyramid_f32(lattices, LO, HI, footprint, mean, cov)[0])
    if len(lattices) == 4:
        assert len(np.unique(lvl)) >= 3                # the rays' own covariances spread over the levels


@pytest.mark.parametrize("name", list(qx.PYRAMIDS))
def test_host_function_against_float64_within_a_derived_bound(hm, name):
    """Bound, with eps = 2^-24; the inputs (mean, cov, lo, hi, the lattices) are float32 in both, so only the arithmetic differs.  Let
    T_l = 3 * 4.01 eps (n_l - 1) S_l + 10 eps A_l be the bound of test_proposal_cpu.py for the trilinear value of level l, D = max - min
    over all lattices (no two values differ by more), A = max |lattice|, s_l the spacings (float32 in both).
      w:  the trace rounds twice and is a sum of non-negative terms (relative error <= 2 eps), sqrtf halves that and rounds once, the
          product with 2 is exact and the one with footprint rounds once: |w_32 - w_64| <= dw = 3.01 eps w.
      value as a function of w: continuous and piecewise linear -- v_l at w = s_l, v_{l+1} at s_{l+1}, constant below s_0 and above s_{L-1}
          -- with slope at most D / min_l (s_{l+1} - s_l), and not constant only for w <= s_{L-1}: moving w by dw moves it by at most
          3.01 eps s_{L-1} D / min_l (s_{l+1} - s_l), whether or not the float32 w falls into the neighbouring segment.
      g:  w - s_l (<= s_{l+1} - s_l in size) and s_{l+1} - s_l round once each and so does the quotient: g carries 3.01 eps more, times D.
      mix: 1 - g rounds once, the two products and the sum once each: <= 3 eps A up to higher-order terms, as one blend step of the lookup;
          a convex combination does not amplify the T_l it is handed.
    bound = max_l T_l + 3.01 eps (s_{L-1} / min_l (s_{l+1} - s_l) + 1) D + 3 eps A (the last two terms only when L > 1)."""
    lattices = qx.random_pyramid(name, seed=19)
    eps = 2.0 ** -24
    s = qx.spacings(lattices, LO, HI).astype(np.float64)
    A = max(float(np.abs(g).max()) for g in lattices)
    D = max(float(g.max()) for g in lattices) - min(float(g.min()) for g in lattices)
    T = max(3 * 4.01 * eps * (max(g.shape) - 1) * (float(g.max()) - float(g.min())) + 10 * eps * float(np.abs(g).max()) for g in lattices)
    bound = T + (3.01 * eps * (s[-1] / np.diff(s).min() + 1.0) * D + 3 * eps * A if len(s) > 1 else 0.0)
    worst = 0.0
    for footprint in FOOTPRINTS:
        mean, cov = _cases(lattices, footprint, seed=23)
        cov[:, [1, 2, 4]] = 0.0
        got = host_density(hm, lattices, footprint, mean, cov)[0].astype(np.float64)
        worst = max(worst, float(np.abs(got - qx.pyramid_f64(lattices, LO, HI, footprint, mean, cov)).max()))
    print(f"pyramid {name}: max |fp32 - fp64| = {worst:.3e}, bound {bound:.3e}")
    assert worst <= bound


# ---- the tenth library: declarations, bindings, exports, argument checks ------------------------------------------------------------
NAMES = ["mipnerf_lattice_density_360", "mipnerf_proposal_360_abi_version", "mipnerf_proposal_360_last_error", "mipnerf_reciprocal_360"]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.PROPOSAL_360_LIB_PATH):
        from mipnerf_pl_amd import build
        build.build(verbose=False)
    return L.proposal_360_lib()


def _header(comments=False):
    text = open(os.path.join(REPO, "include", "mipnerf_proposal_360.h")).read()
    return text if comments else re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return sorted(line.split()[-1] for line in out.splitlines() if line.strip())


def test_header_bindings_and_dynamic_symbols_are_one_set(lib):
    declared = sorted(set(re.findall(r"\b(mipnerf_[a-z0-9_]+)\s*\(", _header())))
    assert declared == sorted(L.PROPOSAL_360_SIGNATURES) == NAMES
    assert _exports(L.PROPOSAL_360_LIB_PATH) == declared
    for name, (_, args) in L.PROPOSAL_360_SIGNATURES.items():
        proto = re.search(r"\b" + name + r"\s*\(([^)]*)\)", _header()).group(1).strip()
        assert (0 if proto in ("", "void") else proto.count(",") + 1) == len(args), (name, proto)
    assert lib.mipnerf_proposal_360_abi_version() == 1 == L.PROPOSAL_360_ABI
    assert int(re.search(r"#define MIPNERF_PROPOSAL_MAX_LEVELS (\d+)", _header()).group(1)) == L.PROPOSAL_MAX_LEVELS == 4
    text = re.sub(r"\s+", " ", re.sub(r"\n \*", "\n", _header(comments=True)))
    for rule in ("Q1 G = the contracted full-covariance Gaussian", "Q2 w = footprint * (2.0f * sqrtf((cov_xx + cov_yy) + cov_zz))",
                 "Q3 (l, g) = mip_level(spacing, L, w)", "only when g > 0: v = (1 - g) * v + g *", "A non-finite mean gives 0 and loads nothing",
                 "spacing[l] = max over the axes of (hi - lo) / float(n_l - 1)", "never allocates and never synchronises"):
        assert rule in text, rule


def test_the_other_libraries_keep_their_tables_and_the_struct_has_the_header_layout(lib):
    assert len(L.SIGNATURES) == 93 and lib.mipnerf_proposal_360_abi_version() == 1
    for table in (L.SIGNATURES, L.DIAG_SIGNATURES, L.PREVIEW_SIGNATURES, L.PREVIEW_MIP_SIGNATURES, L.PREVIEW_SPARSE_SIGNATURES,
                  L.PREVIEW_TUNE_SIGNATURES, L.PREVIEW_360_SIGNATURES, L.PREVIEW_REG_SIGNATURES, L.PREVIEW_TUNE_360_SIGNATURES):
        assert not set(table) & set(L.PROPOSAL_360_SIGNATURES)
    assert not any("_360" in n and "proposal" in n for n in _exports(L.LIB_PATH))
    P = L.ProposalPyramid
    assert (P.levels.offset, P.dims.offset, P.lattice.offset, P.lo.offset, P.hi.offset) == (0, 4, 56, 88, 100) and C.sizeof(P) == 112


def _pyramid(dims=((9, 9, 9), (5, 5, 5)), lo=(-2, -2, -2), hi=(2, 2, 2), lattice=16, levels=None):
    p = L.ProposalPyramid()
    p.levels = len(dims) if levels is None else levels
    for l, d in enumerate(dims):
        for a in range(3):
            p.dims[l][a] = d[a]
        p.lattice[l] = lattice
    for a in range(3):
        p.lo[a], p.hi[a] = lo[a], hi[a]
    return p


def test_lattice_density_360_validates_its_arguments_without_a_gpu(lib):
    err = lambda: (lib.mipnerf_proposal_360_last_error() or b"").decode()  # noqa: E731

    def call(p=None, footprint=1.0, B=4, N=64, t=16, o=16, d=16, r=16, out=16, null_pyramid=False):
        p = _pyramid() if p is None else p
        return lib.mipnerf_lattice_density_360(None if null_pyramid else C.byref(p), footprint, B, N, t, o, d, r, out, None)
    assert call(null_pyramid=True) == L.E_INVALID and "lattice_density_360" in err() and "null" in err()
    for kw in (dict(t=None), dict(o=None), dict(d=None), dict(r=None), dict(out=None)):
        assert call(**kw) == L.E_INVALID and "null" in err(), kw
    assert call(p=_pyramid(lattice=None)) == L.E_INVALID and "null" in err() and "level 0" in err()
    for levels in (0, -1, 5):
        assert call(p=_pyramid(levels=levels)) == L.E_INVALID and "levels" in err(), levels
    for bad in ((1, 9, 9), (9, 1, 9), (9, 9, 1), (0, 9, 9)):
        assert call(p=_pyramid(dims=(bad,))) == L.E_INVALID and "at least 2 points" in err(), bad
        assert call(p=_pyramid(dims=((17, 17, 17), bad))) == L.E_INVALID and "level 1" in err(), bad
    assert call(p=_pyramid(lo=(2, 2, 2), hi=(-2, -2, -2))) == L.E_INVALID and "hi > lo" in err()
    assert call(p=_pyramid(hi=(2, -2, 2))) == L.E_INVALID and "hi > lo" in err()                      # hi == lo on one axis
    assert call(p=_pyramid(hi=(2, float("nan"), 2))) == L.E_INVALID
    assert call(p=_pyramid(dims=((1024, 1024, 512),))) == L.E_INVALID and "2^31" in err()             # 7 nx ny nz >= 2^31
    assert call(p=_pyramid(dims=((675, 675, 674),))) == L.E_INVALID and "2^31" in err()               # 307.1e6 points: just above 2^31 / 7
    assert call(p=_pyramid(dims=((675, 674, 674),)), B=0) == L.OK                                     # 306.6e6: just below
    for dims in (((9, 9, 9), (9, 9, 9)), ((5, 5, 5), (9, 9, 9)), ((9, 9, 9), (5, 5, 5), (5, 5, 5)), ((9, 9, 9), (17, 2, 2), (9, 9, 9))):
        assert call(p=_pyramid(dims=dims)) == L.E_INVALID and "increase strictly" in err(), dims
    assert call(p=_pyramid(dims=((9, 9, 9), (17, 17, 3))), B=0) == L.OK                               # the LARGEST axis spacing counts
    for fp in (-1.0, -0.0001, float("inf"), float("nan")):
        assert call(footprint=fp) == L.E_INVALID and "footprint" in err(), fp
    for n in (0, -1, L.MAX_SAMPLES + 1):
        assert call(N=n) == L.E_INVALID and "num_samples" in err(), n
    assert call(B=-1) == L.E_INVALID and call(B=1 << 31) == L.E_INVALID
    assert call(out=8) == L.E_INVALID and "16-byte" in err()
    # zero rays: nothing to do, whatever the ray pointers; four levels and footprint 0 are fine
    assert call(B=0, t=None, o=None, d=None, r=None, out=None) == L.OK
    assert call(p=_pyramid(dims=((33, 33, 33), (17, 17, 17), (9, 9, 9), (5, 5, 5))), footprint=0.0, B=0) == L.OK


def test_the_build_units_are_compiled_without_contraction_into_a_tenth_library():
    from mipnerf_pl_amd import build as b
    assert [u for u, _ in b.PROPOSAL_360_UNITS] == ["kernels_proposal_360.hip", "proposal_360_capi.hip"]
    assert all("-ffp-contract=off" in flags for _, flags in b.PROPOSAL_360_UNITS)
    assert os.path.basename(b.PROPOSAL_360_LIB) == "libmipnerf_proposal_360.so" == os.path.basename(L.PROPOSAL_360_LIB_PATH)
    assert not any("proposal_360" in u for u, _ in b.UNITS + b.DIAG_UNITS + b.PREVIEW_UNITS + b.PREVIEW_MIP_UNITS + b.PREVIEW_SPARSE_UNITS +
                   b.PREVIEW_TUNE_UNITS + b.PREVIEW_360_UNITS + b.PREVIEW_REG_UNITS + b.PREVIEW_TUNE_360_UNITS)
    src = open(os.path.join(REPO, "mipnerf_pl_amd", "build.py")).read()
    assert '"include", "mipnerf_proposal_360.h"' in src and "os.path.exists(PROPOSAL_360_LIB)" in src
    rules = open(os.path.join(CSRC, "lattice_sample_360.hpp")).read()
    for inc in ('#include "lattice_sample.hpp"', '#include "preview_mip.hpp"', '#include "raymath360.hpp"'):
        assert inc in rules
    code = re.sub(r"//.*", "", rules)
    assert "MIP_HD" in code and "mip_level(" in code and "lattice_trilinear(" in code and "conical_frustum_to_gaussian_full(" in code
    assert not re.search(r"floorf|inv_h\[| / ", code)                         # restates neither the cell nor the level rule; no division
    assert not re.search(r"\.(lattice|box)\[l\]|\.(lattice|box)\[l \+ 1\]", code)      # the descriptors are indexed by the loop counter only
    unit = re.sub(r"//.*", "", open(os.path.join(CSRC, "kernels_proposal_360.hip")).read())
    assert re.search(r"__global__[^;{]*\bk_lattice_density_360\(", unit) and "pyramid_density_sample(" in unit and "make_float4(" in unit
    assert "template <int K" not in unit and "hipFuncSetAttribute" not in unit and "__shared__" not in unit and "atomic" not in unit
    # the bounded proposal path is untouched: its unit does not know the pyramid
    assert "360" not in open(os.path.join(CSRC, "kernels_proposal.hip")).read().replace("mipnerf_hip.h", "")


# ---- Python surface -----------------------------------------------------------------------------------------------------------------
def test_names_signatures_and_defaults():
    from mipnerf_pl_amd import ops
    assert list(inspect.signature(ops.ProposalGrid360.__init__).parameters) == ["self", "lattices", "lo", "hi", "far_radius", "footprint"]
    assert inspect.signature(ops.ProposalGrid360.__init__).parameters["footprint"].default == 1.0
    assert not issubclass(ops.ProposalGrid360, ops.ProposalGrid) and ops.ProposalGrid360.space == "contracted"
    sig = inspect.signature(ops.field_proposal_360)
    assert list(sig.parameters) == ["model_or_system", "grid", "levels", "far_radius", "bound", "cov_scale", "footprint", "precision"]
    assert [sig.parameters[k].default for k in list(sig.parameters)[1:]] == [256, 1, 64.0, 2.0, 1.0, 1.0, None]
    assert list(inspect.signature(ops.lattice_density_360).parameters) == ["grid", "t_samples", "origins", "directions", "radii"]
    assert "choices, not measurements" in re.sub(r"\s+", " ", ops.field_proposal_360.__doc__)
    # the bounded route keeps its pinned signature and its refusal
    sig = inspect.signature(ops.field_proposal)
    assert list(sig.parameters) == ["model_or_system", "grid", "lo", "hi", "cov_scale", "precision"] and sig.parameters["grid"].default == 256
    with pytest.raises(NotImplementedError, match="unbounded=True.*field_proposal_360"):
        ops._refuse_proposal_model(SimpleNamespace(unbounded=True, num_levels=2), "x")
    assert list(inspect.signature(ops._refuse_proposal_model).parameters) == ["model", "name", "grid"]
    assert inspect.signature(ops._refuse_proposal_model).parameters["grid"].default is None
    from mipnerf_pl_amd import evaluate
    sig = inspect.signature(evaluate.scene_proposal)
    assert list(sig.parameters) == ["system", "frames", "grid", "bound", "verbose", "distorted", "space", "far_radius", "levels", "footprint"]
    assert [sig.parameters[k].default for k in ("space", "far_radius", "levels", "footprint")] == [None, None, 1, 1.0]
    assert "choices, not measurements" in re.sub(r"\s+", " ", evaluate.scene_proposal.__doc__)
    with pytest.raises(NotImplementedError, match="unbounded=True.*field_proposal_360"):
        ops.field_proposal(SimpleNamespace(unbounded=True), 64, -1.0, 1.0)


def test_the_ladder_of_field_proposal_360():
    from mipnerf_pl_amd import ops
    want = {4: [4, 2], 5: [5, 3, 2], 16: [16, 8, 4, 2], 256: [256, 128, 64, 32]}
    for grid, full in want.items():
        for levels in range(1, 5):
            if levels <= len(full):
                assert ops.proposal_ladder_360(grid, levels) == full[:levels], (grid, levels)
            else:
                with pytest.raises(ValueError, match="has no level"):
                    ops.proposal_ladder_360(grid, levels)
    assert ops.proposal_ladder_360(257, 4) == [257, 129, 65, 33]             # n - 1 even: every other point of the level below
    for levels in (0, 5):
        with pytest.raises(ValueError, match="levels"):
            ops.proposal_ladder_360(64, levels)
    with pytest.raises(ValueError, match="at least 2"):
        ops.proposal_ladder_360(1, 1)


def test_models_and_grids_that_do_not_fit_are_refused_before_any_device_work():
    from mipnerf_pl_amd import ops
    bounded = SimpleNamespace(mlp=SimpleNamespace(native=None, _cfg_extra={}), unbounded=False)
    with pytest.raises(ValueError, match="unbounded=True"):
        ops.field_proposal_360(bounded, grid=16)
    with pytest.raises(TypeError, match="MipNeRFSystem, MipNerf or MLP"):
        ops.field_proposal_360(SimpleNamespace(unbounded=True), grid=16)
    unbounded = SimpleNamespace(mlp=SimpleNamespace(native=None, _cfg_extra={"unbounded": 1}), unbounded=True)
    with pytest.raises(ValueError, match="has no level"):
        ops.field_proposal_360(unbounded, grid=4, levels=3)
    with pytest.raises(ValueError, match="positive"):
        ops.field_proposal_360(unbounded, grid=16, bound=0.0)
    with pytest.raises(TypeError, match="ProposalGrid360"):
        ops.lattice_density_360(SimpleNamespace(), None, None, None, None)


def _grid360():
    """a ProposalGrid360 without a device: the dispatch reads the type alone"""
    from mipnerf_pl_amd import ops
    return object.__new__(ops.ProposalGrid360)


def test_dispatch_on_the_grid_type_refuses_every_mismatch():
    from mipnerf_pl_amd import evaluate, ops
    g360, g = _grid360(), object.__new__(ops.ProposalGrid)
    ops._refuse_proposal_model(SimpleNamespace(unbounded=True, num_levels=2), "x", g360)           # the one new pair that passes
    ops._refuse_proposal_model(SimpleNamespace(unbounded=False, num_levels=2), "x", g)
    ops._refuse_proposal_model(SimpleNamespace(unbounded=False, num_levels=2), "x")
    with pytest.raises(NotImplementedError, match="bounded"):
        ops._refuse_proposal_model(SimpleNamespace(unbounded=False, num_levels=2), "x", g360)
    with pytest.raises(NotImplementedError, match="unbounded"):
        ops._refuse_proposal_model(SimpleNamespace(unbounded=True, num_levels=2), "x", g)
    for grid in (g, g360, None):
        for unbounded in (False, True):
            with pytest.raises(NotImplementedError, match="two-level|unbounded|bounded"):
                ops._refuse_proposal_model(SimpleNamespace(unbounded=unbounded, num_levels=1), "x", grid)
    with pytest.raises(NotImplementedError, match="two-level"):
        ops._refuse_proposal_model(SimpleNamespace(unbounded=True, num_levels=1), "x", g360)
    # scene_proposal: space=None keeps refusing, a bounded system with space='contracted' and another space are refused
    unb, bnd = SimpleNamespace(mip_nerf=SimpleNamespace(unbounded=True)), SimpleNamespace(mip_nerf=SimpleNamespace(unbounded=False))
    with pytest.raises(NotImplementedError, match="unbounded=True.*space='contracted'"):
        evaluate.scene_proposal(unb, None, 64, 1.0)
    with pytest.raises(ValueError, match="bounded"):
        evaluate.scene_proposal(bnd, None, 64, space="contracted", far_radius=8.0)
    with pytest.raises(ValueError, match="space must be"):
        evaluate.scene_proposal(unb, None, 64, space="world")
    with pytest.raises(ValueError, match="has no level"):
        evaluate.scene_proposal(unb, None, 4, space="contracted", far_radius=8.0, levels=3)
    with pytest.raises(ValueError, match="frames to be rendered or a far_radius"):
        evaluate.scene_proposal(unb, None, 64, space="contracted")


def test_proposal_space_flags_and_their_defaults_on_both_command_lines():
    from mipnerf_pl_amd import eval as eval_cli
    from mipnerf_pl_amd import render_video
    base = ["--out_dir", "o", "--scale", "1"]
    for parser in (eval_cli.build_parser(), render_video.build_parser()):
        a = parser.parse_args(base)
        assert (a.proposal_space, a.proposal_far_radius, a.proposal_levels, a.proposal_footprint, a.proposal_grid) == (None,) * 5
        a = parser.parse_args(base + ["--proposal_grid", "128", "--proposal_space", "contracted", "--proposal_far_radius", "40", "--proposal_levels",
                                      "3", "--proposal_footprint", "0.5", "--cull", "--cull_space", "contracted"])
        assert (a.proposal_grid, a.proposal_space, a.proposal_far_radius, a.proposal_levels, a.proposal_footprint) == (128, "contracted", 40.0, 3, 0.5)
        with pytest.raises(SystemExit):
            parser.parse_args(base + ["--proposal_grid", "--proposal_space", "world"])
        text = re.sub(r"\s+", " ", parser.format_help())
        for flag in ("--proposal_space", "--proposal_far_radius", "--proposal_levels", "--proposal_footprint"):
            assert flag in text
        assert text.count("a choice, not a measurement") >= 2


def test_proposal_space_refusals_come_before_anything_is_loaded_or_written(tmp_path):
    from mipnerf_pl_amd import eval as eval_cli
    from mipnerf_pl_amd import render_video
    missing, out = str(tmp_path / "no_such.ckpt"), str(tmp_path / "o")               # never opened: the refusal comes first
    cases = [(["--proposal_space", "contracted"], "--proposal_space.*--proposal_grid"),
             (["--proposal_grid", "--proposal_levels", "2"], "--proposal_levels belongs to --proposal_space contracted"),
             (["--proposal_grid", "--proposal_footprint", "1"], "--proposal_footprint belongs to --proposal_space contracted"),
             (["--proposal_grid", "--proposal_far_radius", "9"], "--proposal_far_radius belongs to --proposal_space contracted"),
             (["--proposal_grid", "--proposal_space", "contracted", "--proposal_levels", "0"], "1 to 4 levels"),
             (["--proposal_grid", "--proposal_space", "contracted", "--proposal_levels", "5"], "1 to 4 levels"),
             (["--proposal_grid", "--proposal_space", "contracted", "--proposal_footprint", "-0.5"], "finite and >= 0"),
             (["--proposal_grid", "--proposal_space", "contracted", "--proposal_far_radius", "1"], "must exceed 1"),
             (["--proposal_grid", "4", "--proposal_space", "contracted", "--proposal_levels", "3"], "has no level")]
    for extra, msg in cases:
        with pytest.raises(SystemExit, match=msg):
            eval_cli.main(["--ckpt", missing, "--data", str(tmp_path), "--out_dir", out, "--scale", "1"] + extra)
        with pytest.raises(SystemExit, match=msg):
            render_video.main(["--ckpt", missing, "--out_dir", out, "--scale", "1"] + extra)
    assert not os.path.exists(out)
    # after the checkpoint is read: the space and the model must agree
    on = SimpleNamespace(proposal_grid=64, proposal_bound=None, proposal_space="contracted")
    for name in ("llff", "realdata360"):
        unb = SimpleNamespace(hparams={"dataset_name": name}, mip_nerf=SimpleNamespace(unbounded=True))
        render_video.refuse_scene360_proposal(on, unb)
        with pytest.raises(SystemExit, match="--proposal_grid.*captured scene.*" + name + ".*--proposal_space contracted"):
            render_video.refuse_scene360_proposal(SimpleNamespace(proposal_grid=64, proposal_bound=None, proposal_space=None), unb)
    with pytest.raises(SystemExit, match="--proposal_space contracted.*bounded"):
        render_video.refuse_scene360_proposal(on, SimpleNamespace(hparams={"dataset_name": "blender"}, mip_nerf=SimpleNamespace(unbounded=False)))


def test_a_bounded_checkpoint_is_refused_with_proposal_space_by_both_commands_before_rendering(tmp_path):
    from mipnerf_pl_amd import eval as eval_cli
    from mipnerf_pl_amd import render_video
    from mipnerf_pl_amd.system import DEFAULT_HPARAMS, MipNeRFSystem
    hp = dict(DEFAULT_HPARAMS)
    hp.update({"nerf.num_samples": 16, "exp_name": "clib", "dataset_name": "blender"})
    ckpt, out = str(tmp_path / "last.ckpt"), str(tmp_path / "o")
    MipNeRFSystem(hp, precision="fp32").save_checkpoint(ckpt)
    extra = ["--proposal_grid", "16", "--proposal_space", "contracted"]
    with pytest.raises(SystemExit, match="--proposal_space contracted.*bounded"):
        eval_cli.main(["--ckpt", ckpt, "--data", str(tmp_path), "--out_dir", out, "--scale", "1"] + extra)
    with pytest.raises(SystemExit, match="--proposal_space contracted.*bounded"):
        render_video.main(["--ckpt", ckpt, "--data", str(tmp_path), "--out_dir", out, "--scale", "1"] + extra)
    assert not os.path.exists(out)
