"""CPU (no GPU): the baked-lattice preview renderer -- its third library's declarations, bindings, exports and argument checks without a
device; the spherical-harmonic basis and fit against scipy; the float64 fixture (tests/preview_fixture.py) against closed forms and
against the host build of csrc/preview_march.hpp (g++ -O2 -ffp-contract=off from tests/hostmath/preview.cpp); the build units; the
command's parser and refusals."""
import ctypes as C
import os
import re
import subprocess
import warnings
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import preview_fixture as pf
from mipnerf_pl_amd import _lib as L

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
SRC = os.path.join(HERE, "hostmath", "preview.cpp")
SO = os.path.join(HERE, "hostmath", "_preview.so")
F = np.float32
TOL = dict(rgb=5e-5, acc=5e-5, distance=2e-4)          # the project's fp32 bounds (__graft_entry__.py); distance times max(1, far)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.PREVIEW_LIB_PATH):
        from mipnerf_pl_amd import build
        build.build(verbose=False)
    return L.preview_lib()


@pytest.fixture(scope="module")
def hm():
    hdrs = [os.path.join(REPO, "mipnerf_pl_amd", "csrc", h) for h in ("raymath.hpp", "lattice_sample.hpp", "preview_march.hpp")]
    if (not os.path.exists(SO)) or os.path.getmtime(SO) < max(os.path.getmtime(f) for f in [SRC] + hdrs):
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", SRC, "-o", SO])
    return C.CDLL(SO)


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def host_march(hm, rows, degree, rays, step_scale, t_min, max_steps, background, occupancy=None, lo=pf.LO, hi=pf.HI):
    o, d, tn, tf = rays
    nz, ny, nx, _ = rows.shape
    B = o.shape[0]
    bits = np.ascontiguousarray(rows).view(np.uint16)
    rgb, acc, dist, steps = np.zeros((B, 3), F), np.zeros(B, F), np.zeros(B, F), np.zeros(B, np.int32)
    lo, hi, bg = np.array(lo, F), np.array(hi, F), np.array(background, F)
    hm.hm_preview_march(_p(bits), _p(occupancy), nx, ny, nz, _p(lo), _p(hi), degree, C.c_float(step_scale), C.c_float(t_min), max_steps, _p(bg),
                        C.c_longlong(B), _p(o), _p(d), _p(tn), _p(tf), _p(rgb), _p(acc), _p(dist), _p(steps))
    return rgb, acc, dist, steps


# ---- the third library: declarations, bindings, exports ---------------------------------------------------------------------------
def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "mipnerf_preview.h")).read(), flags=re.S)


def test_header_bindings_and_dynamic_symbols_are_one_set(lib):
    declared = sorted(set(re.findall(r"\b(mipnerf_[a-z0-9_]+)\s*\(", _header())))
    assert declared == sorted(L.PREVIEW_SIGNATURES) == ["mipnerf_preview_abi_version", "mipnerf_preview_last_error", "mipnerf_preview_march",
                                                         "mipnerf_preview_pack"]
    out = subprocess.run(["nm", "-D", "--defined-only", L.PREVIEW_LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert sorted(line.split()[-1] for line in out.splitlines() if line.strip()) == declared
    for name, (_, args) in L.PREVIEW_SIGNATURES.items():
        proto = re.search(r"\b" + name + r"\s*\(([^)]*)\)", _header()).group(1).strip()
        count = 0 if proto in ("", "void") else proto.count(",") + 1
        assert count == len(args), (name, proto)
    assert lib.mipnerf_preview_abi_version() == 1 == L.PREVIEW_ABI


def test_the_drop_in_library_is_untouched():
    assert len(L.SIGNATURES) == 93 and not any("preview" in n for n in L.SIGNATURES)
    assert not any(n in L.SIGNATURES or n in L.DIAG_SIGNATURES for n in L.PREVIEW_SIGNATURES)
    hdr = open(os.path.join(REPO, "include", "mipnerf_hip.h")).read()
    assert "mipnerf_preview" not in hdr


def test_struct_layouts_match_the_header():
    assert C.sizeof(L.PreviewField) == 56 and L.PreviewField.rows.offset == 40 and L.PreviewField.occupancy.offset == 48
    assert L.PreviewField.degree.offset == 36 and C.sizeof(L.PreviewParams) == 24 and L.PreviewParams.background.offset == 12
    hdr = _header()
    for field in ("int32_t dims[3]", "float lo[3], hi[3]", "int32_t degree", "const void* rows", "const uint32_t* occupancy", "float step_scale",
                  "float t_min", "int32_t max_steps", "float background[3]"):
        assert field in hdr, field


def _field(dims=(8, 9, 10), lo=pf.LO, hi=pf.HI, degree=1, rows=0x1000, occ=None):
    return L.PreviewField((C.c_int32 * 3)(*dims), (C.c_float * 3)(*lo), (C.c_float * 3)(*hi), degree, rows, occ)


def _params(step_scale=0.5, t_min=0.0, max_steps=64, background=(1.0, 1.0, 1.0)):
    return L.PreviewParams(step_scale, t_min, max_steps, (C.c_float * 3)(*background))


def test_every_entry_point_validates_before_any_hip_call(lib):
    """No device here: a call that reached the HIP runtime would fail with code 3, not with 1 / 2 and a message naming the entry point."""
    P = 0x1000        # never dereferenced: the checks come first

    def march(field, params, n=4, ptrs=(P,) * 7):
        return lib.mipnerf_preview_march(C.byref(field) if field is not None else None, C.byref(params) if params is not None else None, n,
                                         *ptrs, None, None)

    bad = [
        (lambda: march(None, _params()), L.E_INVALID), (lambda: march(_field(), None), L.E_INVALID),
        (lambda: march(_field(rows=None), _params()), L.E_INVALID),
        (lambda: march(_field(dims=(1, 9, 10)), _params()), L.E_INVALID), (lambda: march(_field(dims=(8, 9, 1)), _params()), L.E_INVALID),
        (lambda: march(_field(dims=(1024, 1024, 1024)), _params()), L.E_INVALID),
        (lambda: march(_field(hi=(pf.LO[0], 1.0, 2.375)), _params()), L.E_INVALID),
        (lambda: march(_field(lo=(float("nan"), -0.75, 0.125)), _params()), L.E_INVALID),
        (lambda: march(_field(hi=(float("inf"), 1.0, 2.375)), _params()), L.E_INVALID),
        (lambda: march(_field(degree=3), _params()), L.E_UNSUPPORTED), (lambda: march(_field(degree=-1), _params()), L.E_UNSUPPORTED),
        (lambda: march(_field(), _params(step_scale=0.0)), L.E_INVALID), (lambda: march(_field(), _params(step_scale=-1.0)), L.E_INVALID),
        (lambda: march(_field(), _params(step_scale=float("nan"))), L.E_INVALID),
        (lambda: march(_field(), _params(max_steps=0)), L.E_INVALID),
        (lambda: march(_field(), _params(t_min=1.0)), L.E_INVALID), (lambda: march(_field(), _params(t_min=-0.1)), L.E_INVALID),
        (lambda: march(_field(), _params(t_min=float("nan"))), L.E_INVALID),
        (lambda: march(_field(), _params(), n=-1), L.E_INVALID),
        (lambda: march(_field(rows=0x1008), _params()), L.E_INVALID),                          # 16-byte alignment of the rows
    ] + [(lambda k=k: march(_field(), _params(), ptrs=tuple(None if j == k else P for j in range(7))), L.E_INVALID) for k in range(7)]
    for call, code in bad:
        assert call() == code
        assert b"preview_march" in lib.mipnerf_preview_last_error()
    # no rays: fine whatever the ray pointers
    assert march(_field(), _params(), n=0, ptrs=(None,) * 7) == L.OK
    dims = (C.c_int32 * 3)(8, 9, 10)
    small = (C.c_int32 * 3)(8, 1, 10)
    for call, code in [(lambda: lib.mipnerf_preview_pack(None, 1, P, P, None, P, None), L.E_INVALID),
                       (lambda: lib.mipnerf_preview_pack(dims, 1, None, P, None, P, None), L.E_INVALID),
                       (lambda: lib.mipnerf_preview_pack(dims, 1, P, None, None, P, None), L.E_INVALID),
                       (lambda: lib.mipnerf_preview_pack(dims, 1, P, P, None, None, None), L.E_INVALID),
                       (lambda: lib.mipnerf_preview_pack(small, 1, P, P, None, P, None), L.E_INVALID),
                       (lambda: lib.mipnerf_preview_pack(dims, 3, P, P, None, P, None), L.E_UNSUPPORTED),
                       (lambda: lib.mipnerf_preview_pack(dims, -1, P, P, None, P, None), L.E_UNSUPPORTED)]:
        assert call() == code
        assert b"preview_pack" in lib.mipnerf_preview_last_error()
    with pytest.raises(ValueError, match="x: .*preview_pack"):
        L.preview_check(L.E_INVALID, "x")
    with pytest.raises(NotImplementedError):
        L.preview_check(L.E_UNSUPPORTED, "x")


def test_the_build_units_are_compiled_without_contraction_into_a_third_library():
    from mipnerf_pl_amd import build as b
    assert [u for u, _ in b.PREVIEW_UNITS] == ["kernels_preview.hip", "preview_capi.hip"]
    assert all("-ffp-contract=off" in flags for _, flags in b.PREVIEW_UNITS)
    assert os.path.basename(b.PREVIEW_LIB) == "libmipnerf_preview.so" == os.path.basename(L.PREVIEW_LIB_PATH)
    assert not any(u.startswith(("kernels_preview", "preview_capi")) for u, _ in b.UNITS + b.DIAG_UNITS)
    src = open(os.path.join(REPO, "mipnerf_pl_amd", "build.py")).read()
    assert '"include", "mipnerf_preview.h"' in src and "os.path.exists(PREVIEW_LIB)" in src
    csrc = os.path.join(REPO, "mipnerf_pl_amd", "csrc")
    rules = open(os.path.join(csrc, "preview_march.hpp")).read()
    assert '#include "lattice_sample.hpp"' in rules and "floorf" not in rules and "inv_h[" not in rules      # the index rule is not restated
    unit = open(os.path.join(csrc, "kernels_preview.hip")).read()
    assert '#include "preview_wave_march.hpp"' in unit                     # the march kernel is the shared header's: the unit and it are one text
    kernel = unit + open(os.path.join(csrc, "preview_wave_march.hpp")).read()
    for f in os.listdir(csrc):                                             # and the only one: neither entry point has a kernel of its own
        if f.endswith((".hip", ".hpp", ".py")):
            assert not re.search(r"k_preview_march|k_preview_mip_march", open(os.path.join(csrc, f)).read()), f
    assert '#include "preview_march.hpp"' in kernel and "lattice_cell(" in kernel and not re.search(r"atomic\w*\s*\(|\basm\b", kernel)
    capi = open(os.path.join(csrc, "preview_capi.hip")).read()
    assert not re.search(r"hipMalloc|hipFree|Synchronize|hipMemcpy", capi + kernel)          # never allocates, never synchronises


# ---- the basis and the fit -------------------------------------------------------------------------------------------------------
def _scipy_real_sh(dirs, degree):
    """The real spherical harmonics from scipy's complex ones, re-expressed in the header's order and signs: Y_lm = sqrt(2) (-1)^m Im / Re
    of Y_l^|m| (Condon-Shortley phase removed), PlenOctrees' basis = (-1)^m times that for l = 1 and as listed for l = 2."""
    from scipy.special import sph_harm
    d = np.asarray(dirs, np.float64)
    theta = np.arctan2(d[:, 1], d[:, 0])                 # azimuth
    phi = np.arccos(np.clip(d[:, 2], -1, 1))             # polar
    def real(l, m):
        with warnings.catch_warnings():                  # scipy 1.15 announces sph_harm_y as its successor
            warnings.simplefilter("ignore", DeprecationWarning)
            y = sph_harm(abs(m), l, theta, phi)
        if m == 0:
            return y.real
        return np.sqrt(2) * (-1) ** m * (y.imag if m < 0 else y.real)
    cols = [real(0, 0)]
    if degree >= 1:
        cols += [-real(1, -1), real(1, 0), -real(1, 1)]                                   # -C1 y, C1 z, -C1 x
    if degree >= 2:
        cols += [real(2, -2), -real(2, -1), real(2, 0), -real(2, 1), real(2, 2)]         # C20 xy, C21 yz (C21 < 0), C22 (..), C23 xz (C23 < 0), C24 (xx - yy)
    return np.stack(cols, -1)


@pytest.mark.parametrize("degree", [0, 1, 2])
def test_sh_basis_and_fixture_basis_against_scipy(degree):
    from mipnerf_pl_amd import preview
    rng = np.random.default_rng(3)
    d = rng.normal(size=(200, 3))
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    want = _scipy_real_sh(d, degree)
    assert want.shape == (200, (degree + 1) ** 2)
    assert np.abs(preview.sh_basis(torch.from_numpy(d), degree).numpy() - want).max() < 1e-14
    assert np.abs(pf.sh_basis(d, degree) - want).max() < 1e-14
    assert preview.sh_basis(torch.from_numpy(d.astype(F)), degree).dtype == torch.float32


@pytest.mark.parametrize("degree", [0, 1, 2])
def test_fit_sh_recovers_random_coefficients_from_32_directions(degree):
    from mipnerf_pl_amd import preview
    dirs = preview.bake_directions(32)
    assert dirs.shape == (32, 3) and dirs.dtype == torch.float64
    assert float((dirs.norm(dim=-1) - 1).abs().max()) < 1e-15 and float(dirs.mean(0).abs().max()) < 0.02       # unit, spread over the sphere
    g = torch.Generator().manual_seed(degree)
    coef = torch.randn(50, (degree + 1) ** 2, 3, generator=g, dtype=torch.float64).float()
    basis = torch.from_numpy(_scipy_real_sh(dirs.numpy(), degree))                       # [K, nb], scipy's
    rgb = torch.einsum("kb,mbc->mkc", basis, coef.double()).float()
    got = preview.fit_sh(rgb, dirs, degree)
    assert got.shape == coef.shape and got.dtype == torch.float32
    assert float((got - coef).abs().max()) < 1e-5
    with pytest.raises(NotImplementedError):
        preview.fit_sh(rgb, dirs, 3)
    with pytest.raises(ValueError):
        preview.fit_sh(rgb[:, :3], dirs[:3], 2)                                            # 3 directions, 9 unknowns


# ---- the fixture against closed forms --------------------------------------------------------------------------------------------
def _constant_rows(degree, sigma, colour):
    nx, ny, nz = pf.DIMS
    s = np.full((nz, ny, nx), sigma, F)
    coef = np.zeros((nz, ny, nx, (degree + 1) ** 2, 3), F)
    coef[..., 0, :] = np.asarray(colour, F) / F(pf.C0)
    return pf.pack_rows(s, coef, degree)


def test_fixture_constant_sigma_gives_the_closed_form():
    rays = pf.scene_rays()
    sigma, colour, bg = 0.75, (0.25, 0.5, 0.75), (1.0, 0.5, 0.0)
    rows = _constant_rows(0, sigma, colour)
    rgb, acc, dist, steps, _ = pf.march(rows, pf.LO, pf.HI, 0, *rays, 0.5, 0.0, 4096, bg)
    h = (np.array(pf.HI, F) - np.array(pf.LO, F)) / (np.array(pf.DIMS) - 1).astype(F)
    s = float(F(0.5) * h.min())
    hit = steps > 0
    assert hit.sum() > 200 and (~hit).sum() >= 9
    want_acc = 1.0 - np.exp(-sigma * s * steps[hit])
    assert np.abs(acc[hit] - want_acc).max() < 1e-12
    c16 = rows[0, 0, 0, 1:4].astype(np.float64) * pf.C0                                  # the colour after its fp16 rounding
    want_rgb = want_acc[:, None] * c16 + (1 - want_acc)[:, None] * np.array(bg)
    assert np.abs(rgb[hit] - want_rgb).max() < 1e-12
    # no sample: the miss outputs
    assert (acc[~hit] == 0).all() and (rgb[~hit] == np.array(bg)).all()
    near, far = rays[2][~hit], rays[3][~hit]
    assert np.array_equal(dist[~hit], np.where(np.isfinite(near), near, np.where(np.isfinite(far), far, 0.0)))
    # the distance of a uniform medium lies inside the ray's interval
    assert (dist[hit] >= rays[2][hit]).all() and (dist[hit] <= rays[3][hit]).all()


def test_fixture_empty_lattice_and_clear_occupancy_give_the_miss_outputs():
    rays = pf.scene_rays()
    bg = (0.0, 0.0, 0.0)
    rows = _constant_rows(1, 0.0, (0.3, 0.3, 0.3))
    rgb, acc, dist, steps, _ = pf.march(rows, pf.LO, pf.HI, 1, *rays, 0.5, 0.0, 4096, bg)
    assert (acc == 0).all() and (rgb == 0).all() and steps.max() > 0                      # samples are evaluated, and weigh nothing
    finite = np.isfinite(rays[2])
    assert np.array_equal(dist[finite], rays[2][finite].astype(np.float64))
    nx, ny, nz = pf.DIMS
    clear = np.zeros((nz - 1, ny - 1, 1), np.uint32)
    rows = _constant_rows(1, 30.0, (0.3, 0.3, 0.3))
    rgb, acc, dist, steps, _ = pf.march(rows, pf.LO, pf.HI, 1, *rays, 0.5, 0.0, 4096, (1.0, 1.0, 1.0), occupancy=clear)
    assert (steps == 0).all() and (acc == 0).all() and (rgb == 1).all()
    # an early stop shortens an opaque march and changes the outputs by at most t_min
    full = pf.march(rows, pf.LO, pf.HI, 1, *rays, 0.5, 0.0, 4096, (1.0, 1.0, 1.0))
    cut = pf.march(rows, pf.LO, pf.HI, 1, *rays, 0.5, 1e-2, 4096, (1.0, 1.0, 1.0))
    assert (cut[3] <= full[3]).all() and (cut[3] < full[3]).mean() > 0.5
    assert np.abs(cut[0] - full[0]).max() <= 1e-2 and np.abs(cut[1] - full[1]).max() <= 1e-2
    # max_steps caps the samples
    capped = pf.march(rows, pf.LO, pf.HI, 1, *rays, 0.5, 0.0, 5, (1.0, 1.0, 1.0))
    assert capped[3].max() == 5


def test_fixture_nan_row_poisons_only_the_rays_through_it():
    rays = pf.scene_rays()
    rows, _ = pf.random_rows(1)
    rows = rows.copy()
    rows[4, 4, 3, 0] = np.nan
    clean = pf.march(pf.random_rows(1)[0], pf.LO, pf.HI, 1, *rays, 0.5, 0.0, 4096, (1.0, 1.0, 1.0))
    got = pf.march(rows, pf.LO, pf.HI, 1, *rays, 0.5, 0.0, 4096, (1.0, 1.0, 1.0))
    bad = np.isnan(got[1])
    assert 0 < bad.sum() < 200 and np.isnan(got[0][bad]).all() and np.isnan(got[2][bad]).all()
    assert np.array_equal(got[0][~bad], clean[0][~bad]) and np.array_equal(got[3], clean[3])


# ---- the shared scene: few fragile rays, and the header's host build inside the fp32 bounds ------------------------------------------
@pytest.mark.parametrize("degree", [0, 1, 2])
def test_host_build_of_the_rules_against_the_fixture(hm, degree):
    rays = pf.scene_rays()
    rows, sigma = pf.random_rows(degree)
    assert rows.shape == (10, 9, 8, pf.ROW_HALVES[degree]) and (sigma == 0).any() and sigma.max() <= 50
    bg = (1.0, 1.0, 1.0)
    want = pf.march(rows, pf.LO, pf.HI, degree, *rays, 0.5, 0.0, 4096, bg)
    fragile = want[4]
    assert fragile.mean() <= 0.10                                     # the condition test_gpu_preview.py relies on, checked without a GPU
    got = host_march(hm, rows, degree, rays, 0.5, 0.0, 4096, bg)
    ok = ~fragile
    assert np.array_equal(got[3][ok], want[3][ok])
    assert np.abs(got[0] - want[0])[ok].max() <= TOL["rgb"] and np.abs(got[1] - want[1])[ok].max() <= TOL["acc"]
    assert (np.abs(got[2] - want[2]) / np.maximum(1.0, rays[3]))[ok].max() <= TOL["distance"]
    # more than one block of 64 samples per ray, and a step cap inside a block
    for step_scale, max_steps in ((0.1, 4096), (0.1, 70)):
        want = pf.march(rows, pf.LO, pf.HI, degree, *rays, step_scale, 0.0, max_steps, bg)
        got = host_march(hm, rows, degree, rays, step_scale, 0.0, max_steps, bg)
        ok = ~want[4]
        assert want[3].max() > 64 and ok.mean() > 0.8
        assert np.array_equal(got[3][ok], want[3][ok]) and np.abs(got[0] - want[0])[ok].max() <= TOL["rgb"]


def test_host_half_conversions_are_numpys(hm):
    rng = np.random.default_rng(0)
    v = np.concatenate([rng.normal(0, 10, 4000), rng.normal(0, 1e-5, 2000), rng.uniform(-7e4, 7e4, 2000),
                        [0.0, -0.0, 65504.0, 65519.9, 65520.0, 1e6, -1e6, np.inf, -np.inf, np.nan, 2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -25,
                         2.0 ** -14, 6.1e-5, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11]]).astype(F)
    out = np.zeros(v.size, np.uint16)
    hm.hm_preview_half_bits(C.c_longlong(v.size), _p(v), 0, _p(out))
    with np.errstate(over="ignore"):
        want = v.astype(np.float16)
    nan = np.isnan(want)
    assert np.array_equal(out[~nan], want.view(np.uint16)[~nan]) and np.isnan(out.view(np.float16)[nan]).all()
    hm.hm_preview_half_bits(C.c_longlong(v.size), _p(v), 1, _p(out))
    with np.errstate(over="ignore"):
        want = np.where(v > 65504.0, F(65504.0), v).astype(np.float16)                   # saturated on the high side, as sigma is
    assert np.array_equal(out[~nan], want.view(np.uint16)[~nan]) and np.isnan(out.view(np.float16)[nan]).all()
    allbits = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    back = np.zeros(65536, F)
    hm.hm_preview_half_to_float(C.c_longlong(65536), _p(allbits), _p(back))
    want = allbits.view(np.float16).astype(F)
    nan = np.isnan(want)
    assert np.array_equal(back[~nan].view(np.uint32), want[~nan].view(np.uint32)) and np.isnan(back[nan]).all()


# ---- python layer without a device -----------------------------------------------------------------------------------------------
def test_models_the_bake_refuses():
    from mipnerf_pl_amd import preview
    for m in (SimpleNamespace(unbounded=True, num_levels=2), SimpleNamespace(mip_nerf=SimpleNamespace(unbounded=True, num_levels=2))):
        with pytest.raises(NotImplementedError, match="unbounded=True.*contracted"):
            preview.bake_field(m, grid=8, lo=-1, hi=1)
    with pytest.raises(NotImplementedError, match="two-level"):
        preview.bake_field(SimpleNamespace(unbounded=False, num_levels=1), grid=8, lo=-1, hi=1)
    ok = SimpleNamespace(unbounded=False, num_levels=2)
    with pytest.raises(NotImplementedError, match="degree"):
        preview.bake_field(ok, grid=8, degree=3, lo=-1, hi=1)
    with pytest.raises(ValueError, match="at least 2 points"):
        preview.bake_field(ok, grid=(8, 1, 8), lo=-1, hi=1)
    with pytest.raises(ValueError, match="2\\^31"):
        preview.bake_field(ok, grid=1024, lo=-1, hi=1)
    with pytest.raises(ValueError, match="box"):
        preview.bake_field(ok, grid=8)


def test_baked_field_round_trips_through_one_npz_on_the_host(tmp_path):
    from mipnerf_pl_amd import ops, preview
    rows, _ = pf.random_rows(2)
    nx, ny, nz = pf.DIMS
    bits = torch.from_numpy(np.random.default_rng(1).integers(0, 2 ** 7, (nz - 1, ny - 1, 1), dtype=np.int64).astype(np.int32)).view(torch.uint32)
    occ = ops.Occupancy(bits, pf.DIMS, pf.LO, pf.HI)
    occ.threshold, occ.dilate = 5.0, 1
    b = preview.BakedField(torch.from_numpy(rows), pf.DIMS, pf.LO, pf.HI, 2, occ, 5.0)
    assert b.nbytes == rows.nbytes + bits.numel() * 4
    path = b.save(str(tmp_path / "b.npz"))
    assert preview.BakedField.stored_degree(path) == 2
    c = preview.BakedField.load(path, "cpu")
    assert torch.equal(c.rows.view(torch.int16), b.rows.view(torch.int16)) and c.dims == b.dims and c.lo == b.lo and c.hi == b.hi
    assert c.degree == 2 and c.threshold == 5.0 and c.occupancy.dilate == 1
    assert torch.equal(c.occupancy.bits.view(torch.int32), bits.view(torch.int32))
    cells = preview.occupied_cells(occ).numpy()
    want = np.array([[[pf.occupancy_bit(bits.view(torch.int32).numpy().view(np.uint32), i, j, k) for i in range(nx - 1)] for j in range(ny - 1)]
                     for k in range(nz - 1)])
    assert np.array_equal(cells, want)
    pts = preview.baked_points(occ).numpy()
    for k in range(nz):
        for j in range(ny):
            for i in range(nx):
                around = want[max(k - 1, 0):k + 1, max(j - 1, 0):j + 1, max(i - 1, 0):i + 1]
                assert pts[k, j, i] == around.any()
    with pytest.raises(ValueError, match="rows"):
        preview.BakedField(torch.from_numpy(rows), pf.DIMS, pf.LO, pf.HI, 1)
    with pytest.raises(ValueError, match="hi > lo"):
        preview.BakedField(torch.from_numpy(rows), pf.DIMS, pf.HI, pf.LO, 2)


# ---- command line ----------------------------------------------------------------------------------------------------------------
def test_parser_and_defaults():
    from mipnerf_pl_amd import preview
    p = preview.build_parser()
    a = p.parse_args(["--out_dir", "o"])
    assert a.grid == [256] and a.sh_degree is None and a.bound is None and a.threshold == 0.01 and a.dilate == 1
    assert a.step == 0.5 and a.t_min == 1e-3 and a.precision is None and a.n_poses == 120 and a.scale == 1
    assert a.save_baked is False and a.baked is None and a.data is None and a.compare is False
    a = p.parse_args(["--out_dir", "o", "--grid", "64", "48", "32", "--sh_degree", "2", "--bound", "1.5", "--step", "1", "--t_min", "0",
                      "--precision", "bf16", "--save_baked", "--data", "d", "--compare"])
    assert a.grid == [64, 48, 32] and a.sh_degree == 2 and a.bound == 1.5 and a.step == 1.0 and a.t_min == 0 and a.compare
    assert preview.refuse_arguments(p.parse_args(["--out_dir", "o", "--ckpt", "c", "--grid", "64", "48", "32"])) == (64, 48, 32)
    assert preview.refuse_arguments(p.parse_args(["--out_dir", "o", "--ckpt", "c"])) == (256, 256, 256)
    text = re.sub(r"\s+", " ", p.format_help())
    assert "a choice" in text and "--sh_degree" in text
    # nothing launches differently without the command: neither existing command line knows these flags
    from mipnerf_pl_amd import eval as eval_cli
    from mipnerf_pl_amd import render_video
    for parser in (eval_cli.build_parser(), render_video.build_parser()):
        assert "--sh_degree" not in parser.format_help() and "--baked" not in parser.format_help()


def test_refusals_come_before_anything_is_opened(tmp_path):
    from mipnerf_pl_amd import preview
    missing = str(tmp_path / "no_such.ckpt")               # never opened: the refusal comes first
    out = str(tmp_path / "o")
    base = ["--ckpt", missing, "--out_dir", out]
    for extra, match in ((["--grid", "1"], "at least 2 points"), (["--grid", "64", "1", "64"], "at least 2 points"),
                         (["--grid", "64", "64"], "one number or NX NY NZ"), (["--grid", "1024"], "2\\^31"),
                         (["--sh_degree", "3"], "0, 1 or 2"), (["--sh_degree", "-1"], "0, 1 or 2"),
                         (["--step", "0"], "must be positive"), (["--step", "-0.5"], "must be positive"),
                         (["--t_min", "1"], "\\[0, 1\\)"), (["--bound", "0"], "must be positive"),
                         (["--compare"], "--compare.*--data")):
        with pytest.raises(SystemExit, match=match):
            preview.main(base + extra)
    # --baked of another degree than --sh_degree: the file's degree is read, the checkpoint is not
    rows, _ = pf.random_rows(1)
    baked = preview.BakedField(torch.from_numpy(rows), pf.DIMS, pf.LO, pf.HI, 1).save(str(tmp_path / "deg1.npz"))
    with pytest.raises(SystemExit, match="degree 1.*--sh_degree asks for 2"):
        preview.main(base + ["--baked", baked, "--sh_degree", "2"])
    with pytest.raises(FileNotFoundError):                 # the same degree: on to the (missing) checkpoint
        preview.main(base + ["--baked", baked, "--sh_degree", "1"])
    assert not os.path.exists(out)


def test_captured_scene_checkpoints_are_refused_before_any_device_work(tmp_path):
    from mipnerf_pl_amd import preview
    from mipnerf_pl_amd.config import SCENE360_PRESET
    from mipnerf_pl_amd.system import DEFAULT_HPARAMS, MipNeRFSystem
    for name in ("llff", "realdata360"):
        with pytest.raises(SystemExit, match="captured scene.*" + name):
            preview.refuse_checkpoint(SimpleNamespace(hparams={"dataset_name": name}, mip_nerf=SimpleNamespace(unbounded=True, num_levels=2)))
    with pytest.raises(SystemExit, match="bounded"):
        preview.refuse_checkpoint(SimpleNamespace(hparams={"dataset_name": "blender"}, mip_nerf=SimpleNamespace(unbounded=True, num_levels=2)))
    with pytest.raises(SystemExit, match="two-level"):
        preview.refuse_checkpoint(SimpleNamespace(hparams={"dataset_name": "blender"}, mip_nerf=SimpleNamespace(unbounded=False, num_levels=1)))
    preview.refuse_checkpoint(SimpleNamespace(hparams={"dataset_name": "blender"}, mip_nerf=SimpleNamespace(unbounded=False, num_levels=2)))
    hp = dict(DEFAULT_HPARAMS)
    hp.update(SCENE360_PRESET)
    hp.update({"nerf.num_samples": 16, "exp_name": "cli360", "dataset_name": "llff"})
    ckpt = str(tmp_path / "last.ckpt")
    MipNeRFSystem(hp, precision="fp32").save_checkpoint(ckpt)
    out = str(tmp_path / "o")
    with pytest.raises(SystemExit, match="captured scene"):
        preview.main(["--ckpt", ckpt, "--out_dir", out, "--grid", "16"])        # no device on this machine: the refusal came before one was needed
    assert not os.path.exists(out)
