"""CPU (no GPU): the preview over a cone-radius pyramid of lattices -- the fourth library's declarations, bindings, exports and argument
checks without a device; the float64 fixture (tests/preview_mip_fixture.py) on its own conditions, against closed forms and against the
host build of csrc/preview_mip.hpp (g++ -O2 -ffp-contract=off from tests/hostmath/preview_mip.cpp); rule P7 byte for byte against the
host build of the plain march; the anti-aliasing scene in float64; `BakedPyramid`; the build units; the command's parser and refusals.

Bounds: the project's fp32 bounds of test_preview_cpu.TOL on the rays the fixture does not call fragile, `steps` equal, lod within
1e-4 L.  The level rule adds one rounding of w = k t and one of g (both ~1e-7 relative) and one fp32 mix per row element to the plain
march's arithmetic, far inside those bounds."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import preview_fixture as pf
import preview_mip_fixture as mf
from mipnerf_pl_amd import _lib as L

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
CSRC = os.path.join(REPO, "mipnerf_pl_amd", "csrc")
F = np.float32
TOL = dict(rgb=5e-5, acc=5e-5, distance=2e-4)          # test_preview_cpu.TOL: the project's fp32 bounds; distance times max(1, far)
WHITE = (1.0, 1.0, 1.0)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.PREVIEW_MIP_LIB_PATH):
        from mipnerf_pl_amd import build
        build.build(verbose=False)
    return L.preview_mip_lib()


def _host(name):
    src, so = os.path.join(HERE, "hostmath", name + ".cpp"), os.path.join(HERE, "hostmath", "_" + name + ".so")
    hdrs = [os.path.join(CSRC, h) for h in ("raymath.hpp", "lattice_sample.hpp", "preview_march.hpp", "preview_mip.hpp")]
    if (not os.path.exists(so)) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in [src] + hdrs):
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", src, "-o", so])
    return C.CDLL(so)


@pytest.fixture(scope="module")
def hm():
    return _host("preview_mip")


@pytest.fixture(scope="module")
def hm_plain():
    return _host("preview")


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def host_march(hm, levels, degree, rays, radii, step_scale, t_min, max_steps, background, occupancy=None, footprint=mf.FOOTPRINT,
               lo=pf.LO, hi=pf.HI):
    o, d, tn, tf = rays
    n = len(levels)
    B = o.shape[0]
    bits = [np.ascontiguousarray(r).view(np.uint16) for r in levels]
    occupancy = [None] * n if occupancy is None else [None if w is None else np.ascontiguousarray(w) for w in occupancy]
    rows_p = (C.c_void_p * n)(*[b.ctypes.data for b in bits])
    occ_p = (C.c_void_p * n)(*[None if w is None else w.ctypes.data for w in occupancy])
    dims = np.array([[r.shape[2], r.shape[1], r.shape[0]] for r in levels], np.int32)
    rgb, acc, dist, steps, lod = np.zeros((B, 3), F), np.zeros(B, F), np.zeros(B, F), np.zeros(B, np.int32), np.zeros(B, F)
    lo, hi, bg = np.array(lo, F), np.array(hi, F), np.array(background, F)
    hm.hm_preview_mip_march(n, rows_p, occ_p, _p(dims), _p(lo), _p(hi), degree, C.c_float(footprint), C.c_float(step_scale), C.c_float(t_min),
                            max_steps, _p(bg), C.c_longlong(B), _p(o), _p(d), _p(np.ascontiguousarray(radii, F)), _p(tn), _p(tf), _p(rgb),
                            _p(acc), _p(dist), _p(steps), _p(lod))
    return rgb, acc, dist, steps, lod


def host_plain(hm_plain, rows, degree, rays, step_scale, t_min, max_steps, background, occupancy=None, lo=pf.LO, hi=pf.HI):
    o, d, tn, tf = rays
    nz, ny, nx, _ = rows.shape
    B = o.shape[0]
    bits = np.ascontiguousarray(rows).view(np.uint16)
    rgb, acc, dist, steps = np.zeros((B, 3), F), np.zeros(B, F), np.zeros(B, F), np.zeros(B, np.int32)
    lo, hi, bg = np.array(lo, F), np.array(hi, F), np.array(background, F)
    hm_plain.hm_preview_march(_p(bits), _p(occupancy), nx, ny, nz, _p(lo), _p(hi), degree, C.c_float(step_scale), C.c_float(t_min), max_steps,
                              _p(bg), C.c_longlong(B), _p(o), _p(d), _p(tn), _p(tf), _p(rgb), _p(acc), _p(dist), _p(steps))
    return rgb, acc, dist, steps


def fixture_march(levels, degree, rays, radii, step_scale=0.5, t_min=0.0, max_steps=4096, background=WHITE, occupancy=None,
                  footprint=mf.FOOTPRINT):
    return mf.march(levels, pf.LO, pf.HI, degree, rays[0], rays[1], radii, rays[2], rays[3], footprint, step_scale, t_min, max_steps,
                    background, occupancy)


# ---- the fourth library: declarations, bindings, exports ---------------------------------------------------------------------------
def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "mipnerf_preview_mip.h")).read(), flags=re.S)


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return sorted(line.split()[-1] for line in out.splitlines() if line.strip())


def test_header_bindings_and_dynamic_symbols_are_one_set(lib):
    declared = sorted(set(re.findall(r"\b(mipnerf_[a-z0-9_]+)\s*\(", _header())))
    assert declared == sorted(L.PREVIEW_MIP_SIGNATURES) == ["mipnerf_preview_mip_abi_version", "mipnerf_preview_mip_last_error",
                                                             "mipnerf_preview_mip_march"]
    assert _exports(L.PREVIEW_MIP_LIB_PATH) == declared
    for name, (_, args) in L.PREVIEW_MIP_SIGNATURES.items():
        proto = re.search(r"\b" + name + r"\s*\(([^)]*)\)", _header()).group(1).strip()
        count = 0 if proto in ("", "void") else proto.count(",") + 1
        assert count == len(args), (name, proto)
    assert lib.mipnerf_preview_mip_abi_version() == 1 == L.PREVIEW_MIP_ABI
    assert '#include "mipnerf_preview.h"' in _header()


def test_the_other_three_libraries_are_untouched(lib):
    assert len(L.SIGNATURES) == 93 and not any("preview" in n for n in L.SIGNATURES)
    assert sorted(L.PREVIEW_SIGNATURES) == ["mipnerf_preview_abi_version", "mipnerf_preview_last_error", "mipnerf_preview_march",
                                            "mipnerf_preview_pack"]
    assert not any(n in L.SIGNATURES or n in L.DIAG_SIGNATURES or n in L.PREVIEW_SIGNATURES for n in L.PREVIEW_MIP_SIGNATURES)
    assert _exports(L.PREVIEW_LIB_PATH) == sorted(L.PREVIEW_SIGNATURES)
    assert _exports(L.LIB_PATH) == sorted(L.SIGNATURES)
    assert _exports(L.DIAG_LIB_PATH) == sorted(L.DIAG_SIGNATURES)
    for hdr in ("mipnerf_hip.h", "mipnerf_preview.h", "mipnerf_diag.h"):
        assert "preview_mip" not in open(os.path.join(REPO, "include", hdr)).read()


def test_struct_layout_matches_the_header():
    assert C.sizeof(L.PreviewPyramid) == 8 + 8 * C.sizeof(L.PreviewField) == 456
    assert L.PreviewPyramid.levels.offset == 0 and L.PreviewPyramid.level.offset == 8
    hdr = _header()
    assert re.search(r"typedef struct \{\s*int32_t levels;\s*mipnerf_preview_field_t level\[8\];\s*\} mipnerf_preview_pyramid_t;", hdr)


def _field(dims=(8, 9, 10), lo=pf.LO, hi=pf.HI, degree=1, rows=0x1000, occ=None):
    return L.PreviewField((C.c_int32 * 3)(*dims), (C.c_float * 3)(*lo), (C.c_float * 3)(*hi), degree, rows, occ)


def _pyramid(fields=None, levels=None):
    fields = [_field(dims=d) for d in mf.LEVEL_DIMS] if fields is None else fields
    p = L.PreviewPyramid()
    p.levels = len(fields) if levels is None else levels
    for i, f in enumerate(fields[:8]):
        p.level[i] = f
    return p


def _params(step_scale=0.5, t_min=0.0, max_steps=64, background=WHITE):
    return L.PreviewParams(step_scale, t_min, max_steps, (C.c_float * 3)(*background))


def test_every_argument_is_validated_before_any_hip_call(lib):
    """No device here: a call that reached the HIP runtime would fail with code 3, not with 1 / 2 and a message naming the entry point."""
    P = 0x1000        # never dereferenced: the checks come first

    def march(pyr, params, footprint=1.0, n=4, ptrs=(P,) * 8):
        return lib.mipnerf_preview_mip_march(C.byref(pyr) if pyr is not None else None, C.byref(params) if params is not None else None,
                                             footprint, n, *ptrs, None, None, None)

    def with_level(i, **kw):
        fields = [_field(dims=d) for d in mf.LEVEL_DIMS]
        fields[i] = _field(**dict(dict(dims=mf.LEVEL_DIMS[i]), **kw))
        return _pyramid(fields)

    one_bit = float(np.nextafter(F(pf.HI[1]), F(2.0)))
    bad = [
        (lambda: march(None, _params()), L.E_INVALID), (lambda: march(_pyramid(), None), L.E_INVALID),
        (lambda: march(_pyramid(levels=0), _params()), L.E_INVALID), (lambda: march(_pyramid(levels=9), _params()), L.E_INVALID),
        (lambda: march(_pyramid(levels=-1), _params()), L.E_INVALID),
        # one box, bit for bit, and one degree
        (lambda: march(with_level(1, hi=(pf.HI[0], one_bit, pf.HI[2])), _params()), L.E_INVALID),
        (lambda: march(with_level(2, lo=(pf.LO[0], pf.LO[1], float(np.nextafter(F(pf.LO[2]), F(0.0))))), _params()), L.E_INVALID),
        (lambda: march(with_level(1, degree=2), _params()), L.E_INVALID), (lambda: march(with_level(2, degree=0), _params()), L.E_INVALID),
        # spacings equal or decreasing
        (lambda: march(_pyramid([_field(), _field()]), _params()), L.E_INVALID),
        (lambda: march(_pyramid([_field(dims=mf.LEVEL_DIMS[1]), _field(dims=mf.LEVEL_DIMS[0])]), _params()), L.E_INVALID),
        (lambda: march(_pyramid([_field(dims=d) for d in (mf.LEVEL_DIMS[0], mf.LEVEL_DIMS[2], mf.LEVEL_DIMS[1])]), _params()), L.E_INVALID),
        (lambda: march(_pyramid([_field(dims=(8, 9, 10)), _field(dims=(8, 9, 5))]), _params()), L.E_INVALID),      # the same smallest spacing
        # a level that mipnerf_preview_march would refuse
        (lambda: march(with_level(1, dims=(1, 5, 6)), _params()), L.E_INVALID), (lambda: march(with_level(2, dims=(3, 3, 1)), _params()), L.E_INVALID),
        (lambda: march(with_level(0, dims=(1024, 1024, 1024)), _params()), L.E_INVALID),
        (lambda: march(with_level(1, rows=None), _params()), L.E_INVALID),
        (lambda: march(_pyramid([_field(hi=(pf.LO[0], 1.0, 2.375))]), _params()), L.E_INVALID),
        (lambda: march(_pyramid([_field(lo=(float("nan"), -0.75, 0.125))]), _params()), L.E_INVALID),
        (lambda: march(_pyramid([_field(hi=(float("inf"), 1.0, 2.375))]), _params()), L.E_INVALID),
        (lambda: march(with_level(0, degree=3), _params()), L.E_UNSUPPORTED), (lambda: march(_pyramid([_field(degree=-1)]), _params()), L.E_UNSUPPORTED),
        (lambda: march(with_level(2, rows=0x1008), _params()), L.E_INVALID),                       # 16-byte alignment of every level's rows
        (lambda: march(_pyramid([_field(degree=0, rows=0x1004)]), _params()), L.E_INVALID),        # 8 for degree 0
        # the footprint and the march parameters
        (lambda: march(_pyramid(), _params(), footprint=-1.0), L.E_INVALID), (lambda: march(_pyramid(), _params(), footprint=float("nan")), L.E_INVALID),
        (lambda: march(_pyramid(), _params(), footprint=float("inf")), L.E_INVALID),
        (lambda: march(_pyramid(), _params(step_scale=0.0)), L.E_INVALID), (lambda: march(_pyramid(), _params(step_scale=float("nan"))), L.E_INVALID),
        (lambda: march(_pyramid(), _params(max_steps=0)), L.E_INVALID),
        (lambda: march(_pyramid(), _params(t_min=1.0)), L.E_INVALID), (lambda: march(_pyramid(), _params(t_min=float("nan"))), L.E_INVALID),
        (lambda: march(_pyramid(), _params(), n=-1), L.E_INVALID),
    ] + [(lambda k=k: march(_pyramid(), _params(), ptrs=tuple(None if j == k else P for j in range(8))), L.E_INVALID) for k in range(8)]
    for i, (call, code) in enumerate(bad):
        assert call() == code, i
        assert b"preview_mip_march" in lib.mipnerf_preview_mip_last_error(), i
    # no rays: fine whatever the ray pointers; footprint 0 and a degree-0 pyramid with 8-byte aligned rows are valid too
    assert march(_pyramid(), _params(), n=0, ptrs=(None,) * 8) == L.OK
    assert march(_pyramid(), _params(), footprint=0.0, n=0, ptrs=(None,) * 8) == L.OK
    assert march(_pyramid([_field(dims=d, degree=0, rows=0x1008) for d in mf.LEVEL_DIMS]), _params(), n=0, ptrs=(None,) * 8) == L.OK
    assert march(_pyramid([_field()]), _params(), n=0, ptrs=(None,) * 8) == L.OK
    with pytest.raises(ValueError, match="x: .*preview_mip_march"):
        L.preview_mip_check(L.E_INVALID, "x")
    with pytest.raises(NotImplementedError):
        L.preview_mip_check(L.E_UNSUPPORTED, "x")


def test_the_build_units_are_compiled_without_contraction_into_a_fourth_library():
    from mipnerf_pl_amd import build as b
    assert [u for u, _ in b.PREVIEW_MIP_UNITS] == ["kernels_preview_mip.hip", "preview_mip_capi.hip"]
    assert all("-ffp-contract=off" in flags for _, flags in b.PREVIEW_MIP_UNITS)
    assert os.path.basename(b.PREVIEW_MIP_LIB) == "libmipnerf_preview_mip.so" == os.path.basename(L.PREVIEW_MIP_LIB_PATH)
    assert not any(u.startswith(("kernels_preview_mip", "preview_mip_capi")) for u, _ in b.UNITS + b.DIAG_UNITS + b.PREVIEW_UNITS)
    src = open(os.path.join(REPO, "mipnerf_pl_amd", "build.py")).read()
    assert '"include", "mipnerf_preview_mip.h"' in src and "os.path.exists(PREVIEW_MIP_LIB)" in src
    rules = open(os.path.join(CSRC, "preview_mip.hpp")).read()
    assert '#include "preview_march.hpp"' in rules
    assert not re.search(r"floorf|inv_h\[|expf|half_bits_to_float", rules)                 # restates neither the index rule nor rule 4
    unit = open(os.path.join(CSRC, "kernels_preview_mip.hip")).read()
    assert '#include "preview_wave_march.hpp"' in unit                     # the march kernel is the shared header's: the unit and it are one text
    kernel = unit + open(os.path.join(CSRC, "preview_wave_march.hpp")).read()
    for f in os.listdir(CSRC):                                             # and the only one: neither entry point has a kernel of its own
        if f.endswith((".hip", ".hpp", ".py")):
            assert not re.search(r"k_preview_march|k_preview_mip_march", open(os.path.join(CSRC, f)).read()), f
    sources = [open(os.path.join(CSRC, f)).read() for f in os.listdir(CSRC) if f.endswith((".hip", ".hpp"))]
    assert sum(len(re.findall(r"__global__[^;{]*k_preview\w*_march\s*\(", t)) for t in sources) == 1      # one march kernel,
    assert sum(len(re.findall(r"float \w*incl_prod_dpp\s*\(float", t)) for t in sources) == 1                # one product scan
    assert '#include "preview_mip.hpp"' in kernel and "lattice_cell(" in kernel and "preview_row<" in kernel and "preview_shade<" in kernel
    assert not re.search(r"atomic\w*\s*\(|\basm\b|__shared__", kernel)
    capi = open(os.path.join(CSRC, "preview_mip_capi.hip")).read()
    assert not re.search(r"hipMalloc|hipFree|Synchronize|hipMemcpy", capi + kernel)          # never allocates, never synchronises


# ---- the fixture on its own ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rays():
    return pf.scene_rays()


@pytest.fixture(scope="module")
def radii():
    return mf.scene_radii()


@pytest.fixture(scope="module")
def reference(rays, radii):
    """the fixture's march of the shared scene, once per (degree, step_scale, max_steps)"""
    cache = {}

    def get(degree, step_scale, max_steps=4096):
        key = (degree, step_scale, max_steps)
        if key not in cache:
            levels = [r for r, _ in mf.scene_levels(degree)]
            cache[key] = (levels, fixture_march(levels, degree, rays, radii, step_scale, 0.0, max_steps))
        return cache[key]
    return get


def test_the_scene_has_the_spacings_few_fragile_rays_and_all_four_regimes(reference, radii):
    assert [mf.spacing(d, pf.LO, pf.HI) for d in mf.LEVEL_DIMS] == [0.21875, 0.4375, 0.75]
    assert radii.shape == (pf.N_RAYS,) and 0.005 <= radii.min() < 0.01 and 0.4 < radii.max() <= 0.6
    for step_scale in (0.5, 0.1):
        _, want = reference(1, step_scale)
        fragile, regimes = want[5], want[6]
        share = regimes / regimes.sum()
        print(f"step {step_scale}: fragile {fragile.mean():.4f}, regimes {np.round(share, 4)}, mean lod {want[4].mean():.4f}")
        assert fragile.mean() <= 0.10
        assert regimes.shape == (5,) and all(share[i] >= 0.05 for i in (0, 1, 3, 4))


def test_fixture_with_one_level_or_zero_radii_is_the_plain_fixture(rays, radii):
    levels = [r for r, _ in mf.scene_levels(1)]
    want = pf.march(levels[0], pf.LO, pf.HI, 1, *rays, 0.5, 1e-3, 4096, WHITE)
    for got in (fixture_march(levels[:1], 1, rays, radii, t_min=1e-3), fixture_march(levels, 1, rays, 0.0 * radii, t_min=1e-3)):
        for a, b in zip(got[:3], want[:3]):
            assert np.abs(a - b).max() < 1e-12
        assert np.array_equal(got[3], want[3]) and np.array_equal(got[5], want[4]) and (got[4] == 0).all()
    # a radius that is negative or not finite is a miss (P2)
    bad = radii.copy()
    bad[:3] = [-1e-3, np.nan, np.inf]
    got = fixture_march(levels, 1, rays, bad)
    assert (got[3][:3] == 0).all() and (got[1][:3] == 0).all() and (got[0][:3] == 1).all() and np.array_equal(got[2][:3], rays[2][:3])


# ---- the host build of the rules against the fixture --------------------------------------------------------------------------------
def compare(got, want, rays, L_levels, what):
    rgb, acc, dist, steps, lod, fragile = want[:6]
    ok = ~fragile
    err = dict(rgb=np.abs(got[0] - rgb)[ok].max(), acc=np.abs(got[1] - acc)[ok].max(),
               distance=(np.abs(got[2] - dist) / np.maximum(1.0, rays[3]))[ok].max())
    lod_err = np.abs(got[4] - lod)[ok].max()
    print(what, "fragile", int(fragile.sum()), "of", fragile.size, " ".join(f"{k}={v:.3e}" for k, v in err.items()), f"lod={lod_err:.3e}")
    assert np.array_equal(got[3][ok], steps[ok]), (what, np.flatnonzero((got[3] != steps) & ok))
    for k, v in err.items():
        assert v <= TOL[k], (what, k, v)
    assert lod_err <= 1e-4 * L_levels, (what, lod_err)


@pytest.mark.parametrize("degree", [0, 1, 2])
def test_host_build_of_the_rules_against_the_fixture(hm, reference, rays, radii, degree):
    for step_scale, max_steps in ((0.5, 4096), (0.1, 4096), (0.1, 70)):
        levels, want = reference(degree, step_scale, max_steps)
        assert want[5].mean() <= 0.10 and want[3].max() == min(max_steps, 33 if step_scale == 0.5 else 166)
        got = host_march(hm, levels, degree, rays, radii, step_scale, 0.0, max_steps, WHITE)
        compare(got, want, rays, 3, f"degree {degree}, step {step_scale}, cap {max_steps}")
        assert 0.3 < want[4][want[1] > 0].mean() < 1.7                      # the levels really are mixed


def test_host_build_with_per_level_occupancy(hm, rays, radii):
    """hollow rows: every level has clear cells of its own, so P5's OR decides samples whose own level is clear and whose next one is not"""
    made = mf.scene_levels(1, hollow=True)
    levels = [r for r, _ in made]
    words = [mf.cell_occupancy(r[..., 0].astype(F), 5.0) for r in levels]
    want = fixture_march(levels, 1, rays, radii, occupancy=words)
    free = fixture_march(levels, 1, rays, radii)
    own = fixture_march(levels, 1, rays, radii, occupancy=[words[0], None, None])      # other grids: other samples are clear
    # a condition on the inputs, not on the code: the grids clear samples on a good share of the rays (about a fifth with these seeds)
    assert (want[3] < free[3]).mean() > 0.15 and not np.array_equal(want[3], own[3])
    got = host_march(hm, levels, 1, rays, radii, 0.5, 0.0, 4096, WHITE, occupancy=words)
    compare(got, want, rays, 3, "occupancy on every level")
    got = host_march(hm, levels, 1, rays, radii, 0.5, 0.0, 4096, WHITE, occupancy=[words[0], None, words[2]])
    compare(got, fixture_march(levels, 1, rays, radii, occupancy=[words[0], None, words[2]]), rays, 3, "occupancy on levels 0 and 2")


@pytest.mark.parametrize("degree", [0, 1, 2])
def test_one_level_and_zero_radii_are_the_plain_march_byte_for_byte(hm, hm_plain, rays, radii, degree):
    """P7 on the host builds: every ray, fragile or not, NaN or not"""
    levels = [r for r, _ in mf.scene_levels(degree, hollow=True)]
    words = mf.cell_occupancy(levels[0][..., 0].astype(F), 5.0)
    for occ in (None, words):
        for step_scale, t_min, cap in ((0.5, 0.0, 4096), (0.1, 1e-3, 70)):
            plain = host_plain(hm_plain, levels[0], degree, rays, step_scale, t_min, cap, (0.0, 0.25, 0.5), occupancy=occ)
            one = host_march(hm, levels[:1], degree, rays, radii, step_scale, t_min, cap, (0.0, 0.25, 0.5), occupancy=None if occ is None else [occ])
            zero = host_march(hm, levels, degree, rays, 0.0 * radii, step_scale, t_min, cap, (0.0, 0.25, 0.5),
                              occupancy=None if occ is None else [occ, None, None])
            nofoot = host_march(hm, levels, degree, rays, radii, step_scale, t_min, cap, (0.0, 0.25, 0.5), footprint=0.0,
                                occupancy=None if occ is None else [occ, None, None])
            for got in (one, zero, nofoot):
                for a, b in zip(got[:4], plain):
                    assert a.tobytes() == b.tobytes()
                assert (got[4] == 0).all()
            assert plain[3].max() > 0


def test_constant_levels_give_the_closed_form_for_any_radii(hm, rays, radii):
    sigma, colour, bg = 0.75, (0.25, 0.5, 0.75), (1.0, 0.5, 0.0)
    levels = []
    for nx, ny, nz in mf.LEVEL_DIMS:
        coef = np.zeros((nz, ny, nx, 1, 3), F)
        coef[..., 0, :] = np.asarray(colour, F) / F(pf.C0)
        levels.append(pf.pack_rows(np.full((nz, ny, nx), sigma, F), coef, 0))
    s = float(F(0.5) * F(0.21875))
    c16 = levels[0][0, 0, 0, 1:4].astype(np.float64) * pf.C0
    for rad in (radii, 0.0 * radii, np.full_like(radii, 10.0)):
        want = fixture_march(levels, 0, rays, rad, background=bg)
        hit = want[3] > 0
        assert hit.sum() > 200
        want_acc = 1.0 - np.exp(-sigma * s * want[3][hit])
        assert np.abs(want[1][hit] - want_acc).max() < 1e-12
        assert np.abs(want[0][hit] - (want_acc[:, None] * c16 + (1 - want_acc)[:, None] * np.array(bg))).max() < 1e-12
        got = host_march(hm, levels, 0, rays, rad, 0.5, 0.0, 4096, bg)
        ok = ~want[5]
        assert np.array_equal(got[3][ok], want[3][ok])
        assert np.abs(got[1][hit & ok] - want_acc[ok[hit]]).max() <= TOL["acc"]
    assert (fixture_march(levels, 0, rays, np.full_like(radii, 10.0))[4][hit] == 2.0).all()       # w >= s_2 everywhere: the top level


def test_a_nan_row_in_level_1_poisons_only_the_rays_that_read_it(hm, rays, radii):
    levels = [r.copy() for r, _ in mf.scene_levels(1)]
    clean = host_march(hm, levels, 1, rays, radii, 0.5, 0.0, 4096, WHITE)
    levels[1][3, 2, 2, 0] = np.nan
    levels[1][1, 3, 3, 5] = np.nan
    want = fixture_march(levels, 1, rays, radii)
    got = host_march(hm, levels, 1, rays, radii, 0.5, 0.0, 4096, WHITE)
    bad = np.isnan(want[1]) | np.isnan(want[0]).any(-1)
    sure = ~want[5]
    assert 0 < bad.sum() < 200
    assert (np.isnan(got[0]).any(-1) == bad)[sure].all() and np.isnan(got[2][np.isnan(want[2]) & sure]).all()
    same = ~bad & sure
    assert np.array_equal(got[0][same], clean[0][same]) and np.array_equal(got[3][sure], clean[3][sure])
    # the same rays with radii 0 never read level 1
    zero = host_march(hm, levels, 1, rays, 0.0 * radii, 0.5, 0.0, 4096, WHITE)
    assert np.isfinite(zero[0]).all() and np.isfinite(zero[1]).all() and np.isfinite(zero[2][np.isfinite(rays[2])]).all()


# ---- the anti-aliasing scene in float64 --------------------------------------------------------------------------------------------
def test_the_pyramid_anti_aliases_the_scene_of_the_issue():
    """33 / 17 / 9 points over [-1, 1]^3, constant density, colour sinusoids of wavelength 3 fine cells, a pinhole camera; the truth is the
    6 x 6 supersampled plain march.  At 12 x 12 a pixel is 1.6 - 2 fine cells wide and the pyramid must at least halve the plain march's
    mean squared error; at 24 x 24 a pixel stays below the finest spacing and the pyramid IS the plain march."""
    plain, mip = mf.aa_reference(12)
    print(f"12 x 12: MSE plain {plain:.3e}, pyramid {mip:.3e}, ratio {mip / plain:.4f}")
    assert mip < 0.5 * plain
    plain, mip = mf.aa_reference(24)
    print(f"24 x 24: MSE plain {plain:.3e}, pyramid {mip:.3e}, ratio {mip / plain:.6f}")
    assert abs(mip - plain) <= 1e-3 * plain
    o, d, rad, tn, tf = mf.aa_rays(24)
    assert float(F(mf.FOOTPRINT) * rad.max()) * 10.0 < mf.spacing(mf.AA_DIMS[0], mf.AA_LO, mf.AA_HI)      # t <= 10 inside the box


# ---- python layer without a device -----------------------------------------------------------------------------------------------
def _baked(rows, dims, degree=1, lo=pf.LO, hi=pf.HI, occ=None):
    from mipnerf_pl_amd import preview
    return preview.BakedField(torch.from_numpy(np.ascontiguousarray(rows)), dims, lo, hi, degree, occ)


def test_baked_pyramid_validates_and_round_trips_through_one_npz(tmp_path):
    from mipnerf_pl_amd import ops, preview
    made = [r for r, _ in mf.scene_levels(1)]
    nx, ny, nz = mf.LEVEL_DIMS[1]
    bits = torch.from_numpy(np.random.default_rng(1).integers(0, 2 ** 4, (nz - 1, ny - 1, 1), dtype=np.int64).astype(np.int32)).view(torch.uint32)
    occ = ops.Occupancy(bits, mf.LEVEL_DIMS[1], pf.LO, pf.HI)
    occ.threshold, occ.dilate = 5.0, 1
    fields = [_baked(made[0], mf.LEVEL_DIMS[0]), _baked(made[1], mf.LEVEL_DIMS[1], occ=occ), _baked(made[2], mf.LEVEL_DIMS[2])]
    pyr = preview.BakedPyramid(fields)
    assert len(pyr) == 3 and pyr.degree == 1 and pyr.lo == fields[0].lo and pyr.hi == fields[0].hi
    assert pyr.spacings == (0.21875, 0.4375, 0.75) and pyr.nbytes == sum(f.nbytes for f in fields)
    path = pyr.save(str(tmp_path / "p.npz"))
    assert preview.BakedPyramid.stored_levels(path) == 3 and preview.BakedField.stored_degree(path) == 1
    again = preview.BakedPyramid.load(path, "cpu")
    assert len(again) == 3
    for a, b in zip(again.levels, fields):
        assert torch.equal(a.rows.view(torch.int16), b.rows.view(torch.int16)) and a.dims == b.dims and a.lo == b.lo and a.hi == b.hi
        assert a.degree == b.degree and (a.occupancy is None) == (b.occupancy is None)
    assert torch.equal(again.levels[1].occupancy.bits.view(torch.int32), bits.view(torch.int32)) and again.levels[1].occupancy.dilate == 1
    # the single lattice's format is what it was, and each loader names the other
    single = fields[0].save(str(tmp_path / "s.npz"))
    assert preview.BakedPyramid.stored_levels(single) is None
    with np.load(single) as z:
        assert sorted(z.files) == ["degree", "dims", "hi", "lo", "rows", "threshold"]
    with pytest.raises(ValueError, match="BakedField.load"):
        preview.BakedPyramid.load(single, "cpu")
    with pytest.raises(ValueError, match="BakedPyramid.load"):
        preview.BakedField.load(path, "cpu")
    # refusals
    one_bit = (pf.HI[0], float(np.nextafter(F(pf.HI[1]), F(2.0))), pf.HI[2])
    with pytest.raises(ValueError, match="one box"):
        preview.BakedPyramid([fields[0], _baked(made[1], mf.LEVEL_DIMS[1], hi=one_bit)])
    with pytest.raises(ValueError, match="degree"):
        preview.BakedPyramid([fields[0], _baked(mf.random_level(mf.LEVEL_DIMS[1], 2, 5)[0], mf.LEVEL_DIMS[1], degree=2)])
    with pytest.raises(ValueError, match="increase strictly"):
        preview.BakedPyramid([fields[1], fields[0]])
    with pytest.raises(ValueError, match="increase strictly"):
        preview.BakedPyramid([fields[0], fields[0]])
    with pytest.raises(ValueError, match="1 .. 8"):
        preview.BakedPyramid([])
    nine = [_baked(np.zeros((n, n, n, 16), np.float16), (n, n, n)) for n in (257, 129, 65, 33, 17, 9, 5, 3, 2)]
    with pytest.raises(ValueError, match="1 .. 8"):
        preview.BakedPyramid(nine)
    assert len(preview.BakedPyramid(nine[1:])) == 8


def test_pyramid_dims_halve_the_points_and_stop_when_the_spacing_stops_growing():
    from mipnerf_pl_amd import preview
    assert preview.pyramid_dims(256, 4, -1.5, 1.5) == [(256,) * 3, (128,) * 3, (64,) * 3, (32,) * 3]
    assert preview.pyramid_dims(24, 3, -1.0, 1.0) == [(24,) * 3, (12,) * 3, (6,) * 3]
    assert preview.pyramid_dims((33, 17, 9), 8, -1.0, 1.0) == [(33, 17, 9), (17, 9, 5), (9, 5, 3), (5, 3, 2), (3, 2, 2), (2, 2, 2)]
    assert preview.pyramid_dims(3, 8, -1.0, 1.0) == [(3, 3, 3), (2, 2, 2)] and preview.pyramid_dims(2, 4, -1.0, 1.0) == [(2, 2, 2)]
    for bad in (0, 9):
        with pytest.raises(ValueError, match="1 .. 8"):
            preview.pyramid_dims(64, bad, -1.0, 1.0)


def test_bake_pyramid_refuses_what_bake_field_refuses():
    from types import SimpleNamespace
    from mipnerf_pl_amd import preview
    with pytest.raises(NotImplementedError, match="unbounded=True.*contracted"):
        preview.bake_pyramid(SimpleNamespace(unbounded=True, num_levels=2), grid=8, lo=-1, hi=1)
    with pytest.raises(NotImplementedError, match="two-level"):
        preview.bake_pyramid(SimpleNamespace(unbounded=False, num_levels=1), grid=8, lo=-1, hi=1)
    ok = SimpleNamespace(unbounded=False, num_levels=2)
    with pytest.raises(NotImplementedError, match="degree"):
        preview.bake_pyramid(ok, grid=8, degree=3, lo=-1, hi=1)
    with pytest.raises(ValueError, match="at least 2 points"):
        preview.bake_pyramid(ok, grid=(8, 1, 8), lo=-1, hi=1)
    with pytest.raises(ValueError, match="box"):
        preview.bake_pyramid(ok, grid=8)
    with pytest.raises(ValueError, match="1 .. 8"):
        preview.bake_pyramid(ok, grid=8, levels=9, lo=-1, hi=1)


# ---- command line ----------------------------------------------------------------------------------------------------------------
def test_parser_mip_and_footprint():
    from mipnerf_pl_amd import preview
    p = preview.build_parser()
    a = p.parse_args(["--out_dir", "o"])
    assert a.mip is None and a.footprint is None
    # the existing defaults are what they were
    assert a.grid == [256] and a.sh_degree is None and a.bound is None and a.threshold == 0.01 and a.dilate == 1
    assert a.step == 0.5 and a.t_min == 1e-3 and a.precision is None and a.n_poses == 120 and a.scale == 1
    assert a.save_baked is False and a.baked is None and a.data is None and a.compare is False
    assert p.parse_args(["--out_dir", "o", "--mip"]).mip == 4 == preview.DEFAULT_MIP_LEVELS
    assert p.parse_args(["--out_dir", "o", "--mip", "--grid", "64"]).mip == 4
    a = p.parse_args(["--out_dir", "o", "--mip", "3", "--footprint", "1.5"])
    assert a.mip == 3 and a.footprint == 1.5
    assert preview.DEFAULT_FOOTPRINT == float(np.sqrt(3.0))
    text = re.sub(r"\s+", " ", p.format_help())
    assert "--mip [L]" in text and "the bare flag means 4 levels (a choice" in text and "--footprint F" in text
    from mipnerf_pl_amd import eval as eval_cli
    from mipnerf_pl_amd import render_video
    for parser in (eval_cli.build_parser(), render_video.build_parser()):
        assert "--mip" not in parser.format_help() and "--footprint" not in parser.format_help()


def test_mip_refusals_come_before_the_checkpoint_is_opened(tmp_path):
    from mipnerf_pl_amd import preview
    missing = str(tmp_path / "no_such.ckpt")               # never opened: the refusal comes first
    out = str(tmp_path / "o")
    base = ["--ckpt", missing, "--out_dir", out]
    for extra, match in ((["--footprint", "1.0"], "--footprint.*give --mip"), (["--mip", "0"], "1 .. 8"), (["--mip", "9"], "1 .. 8"),
                         (["--mip", "--footprint", "-1"], "finite and >= 0"), (["--mip", "--footprint", "nan"], "finite and >= 0")):
        with pytest.raises(SystemExit, match=match):
            preview.main(base + extra)
    made = [r for r, _ in mf.scene_levels(1)]
    fields = [_baked(r, d) for r, d in zip(made, mf.LEVEL_DIMS)]
    pyr = preview.BakedPyramid(fields).save(str(tmp_path / "pyr.npz"))
    single = fields[0].save(str(tmp_path / "single.npz"))
    with pytest.raises(SystemExit, match="pyramid of 3 levels.*--mip 3"):
        preview.main(base + ["--baked", pyr])
    with pytest.raises(SystemExit, match="pyramid of 3 levels, --mip asks for 4"):
        preview.main(base + ["--baked", pyr, "--mip"])
    with pytest.raises(SystemExit, match="single lattice, --mip asks for 3"):
        preview.main(base + ["--baked", single, "--mip", "3"])
    with pytest.raises(SystemExit, match="degree 1.*--sh_degree asks for 2"):
        preview.main(base + ["--baked", pyr, "--mip", "3", "--sh_degree", "2"])
    for ok in (["--baked", pyr, "--mip", "3"], ["--baked", single]):
        with pytest.raises(FileNotFoundError):             # matching counts: on to the (missing) checkpoint
            preview.main(base + ok)
    assert not os.path.exists(out)
