"""CPU (no GPU): tuning the baked preview's lattice -- the sixth library's declarations, bindings, exports and argument checks without a
device; the numpy restatement of rules 8 - 10 (tests/preview_tune_fixture.py) against central differences of the float64 march; the clamps;
the rules of csrc/preview_tune.hpp (g++ -O2 -ffp-contract=off from tests/hostmath/preview_tune.cpp) against the fixture; the Adam rule bit
for bit; the command's parser and refusals; the convergence recipe the GPU test repeats.

THE TOLERANCE OF THE GRADIENT.  Scaled error = |got - want| / (A_e + 1e-3 max_e A_e), A_e the sum of the absolute values of the terms of
entry e (the fixture returns it).  Nothing in the project gives a bound for it, so it is measured, on the reference alone: the fixture's own
float32 run against its float64 run on the same inputs (degrees 0 - 2, steps 0.5 and 0.1, every case and both loss sides the tests use) is
what fp32 arithmetic does to these formulas.  Largest values so measured: 9.09e-6 with a given grad_rgb, 3.72e-5 in target mode (G cancels
where rgb comes close to the target); preview_tune_fixture.MEASURED rounds them up and LIMIT is 4 x MEASURED per mode: the margin covers
another summation order (wave scans, atomics) and expf's 2 ulp."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import preview_fixture as pf
import preview_tune_fixture as tf
from mipnerf_pl_amd import _lib as L

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
CSRC = os.path.join(REPO, "mipnerf_pl_amd", "csrc")
F = np.float32
WHITE = (1.0, 1.0, 1.0)
BG = tf.BG
LATE_T_MIN = tf.LATE_T_MIN


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.PREVIEW_TUNE_LIB_PATH):
        from mipnerf_pl_amd import build
        build.build(verbose=False)
    return L.preview_tune_lib()


def host():
    src, so = os.path.join(HERE, "hostmath", "preview_tune.cpp"), os.path.join(HERE, "hostmath", "_preview_tune.so")
    hdrs = [os.path.join(CSRC, h) for h in ("raymath.hpp", "lattice_sample.hpp", "preview_march.hpp", "preview_tune.hpp")]
    if (not os.path.exists(so)) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in [src] + hdrs):
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", src, "-o", so])
    return C.CDLL(so)


@pytest.fixture(scope="module")
def hm():
    return host()


@pytest.fixture(scope="module")
def rays():
    return pf.scene_rays()


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


# ---- the sixth library: declarations, bindings, exports ----------------------------------------------------------------------------
NAMES = ["mipnerf_preview_tune_abi_version", "mipnerf_preview_tune_adam", "mipnerf_preview_tune_grad", "mipnerf_preview_tune_last_error"]


def _header(name="mipnerf_preview_tune.h"):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", name)).read(), flags=re.S)


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return sorted(line.split()[-1] for line in out.splitlines() if line.strip())


def test_header_bindings_and_dynamic_symbols_are_one_set(lib):
    declared = sorted(set(re.findall(r"\b(mipnerf_[a-z0-9_]+)\s*\(", _header())))
    assert declared == sorted(L.PREVIEW_TUNE_SIGNATURES) == NAMES
    assert _exports(L.PREVIEW_TUNE_LIB_PATH) == declared
    for name, (_, args) in L.PREVIEW_TUNE_SIGNATURES.items():
        proto = re.search(r"\b" + name + r"\s*\(([^)]*)\)", _header()).group(1).strip()
        count = 0 if proto in ("", "void") else proto.count(",") + 1
        assert count == len(args), (name, proto)
    assert lib.mipnerf_preview_tune_abi_version() == 1 == L.PREVIEW_TUNE_ABI
    assert '#include "mipnerf_preview.h"' in _header()


def test_the_other_five_libraries_keep_their_tables(lib):
    others = dict(hip=L.SIGNATURES, diag=L.DIAG_SIGNATURES, preview=L.PREVIEW_SIGNATURES, mip=L.PREVIEW_MIP_SIGNATURES,
                  sparse=L.PREVIEW_SPARSE_SIGNATURES)
    assert [len(t) for t in others.values()] == [93, 3, 4, 3, 7]
    for table in others.values():
        assert not set(table) & set(L.PREVIEW_TUNE_SIGNATURES) and not any("tune" in n for n in table)
    for path, table in ((L.PREVIEW_LIB_PATH, L.PREVIEW_SIGNATURES), (L.PREVIEW_MIP_LIB_PATH, L.PREVIEW_MIP_SIGNATURES),
                        (L.PREVIEW_SPARSE_LIB_PATH, L.PREVIEW_SPARSE_SIGNATURES)):
        assert _exports(path) == sorted(table)
    for hdr in ("mipnerf_hip.h", "mipnerf_preview.h", "mipnerf_preview_mip.h", "mipnerf_preview_sparse.h", "mipnerf_diag.h"):
        assert "preview_tune" not in open(os.path.join(REPO, "include", hdr)).read()


def test_the_build_units_are_compiled_without_contraction_into_a_sixth_library():
    from mipnerf_pl_amd import build as b
    assert [u for u, _ in b.PREVIEW_TUNE_UNITS] == ["kernels_preview_tune.hip", "preview_tune_capi.hip"]
    assert all("-ffp-contract=off" in flags for _, flags in b.PREVIEW_TUNE_UNITS)
    assert os.path.basename(b.PREVIEW_TUNE_LIB) == "libmipnerf_preview_tune.so" == os.path.basename(L.PREVIEW_TUNE_LIB_PATH)
    assert not any("tune" in u for u, _ in b.UNITS + b.DIAG_UNITS + b.PREVIEW_UNITS + b.PREVIEW_MIP_UNITS + b.PREVIEW_SPARSE_UNITS)
    src = open(os.path.join(REPO, "mipnerf_pl_amd", "build.py")).read()
    assert '"include", "mipnerf_preview_tune.h"' in src and "os.path.exists(PREVIEW_TUNE_LIB)" in src
    rules = open(os.path.join(CSRC, "preview_tune.hpp")).read()
    assert "MIP_HD" in rules and '#include "preview_march.hpp"' in rules and "preview_half_bits(" in rules
    assert not re.search(r"floorf|inv_h\[|expf|half_bits_to_float\(", rules)           # restates neither the cell index, the blend nor rule 4
    unit = open(os.path.join(CSRC, "kernels_preview_tune.hip")).read()
    assert '#include "preview_wave_march.hpp"' in unit and '#include "preview_tune.hpp"' in unit
    assert "wave_incl_prod_dpp(" in unit and not re.search(r"float \w*incl_prod_dpp\s*\(float", unit)      # the product scan is the march's
    assert re.search(r"__global__[^;{]*\bk_preview_tune_grad\s*\(", unit) and re.search(r"__global__[^;{]*\bk_preview_tune_adam\s*\(", unit)
    assert not re.search(r"__global__[^;{]*k_\w*march\s*\(", unit)                      # no second march kernel
    for call in ("lattice_cell(", "preview_occupied(", "preview_row<", "preview_shade<", "tune_q(", "tune_d_sigma(", "tune_d_colour(",
                 "tune_corner_weight(", "tune_adam_element("):
        assert call in unit, call
    assert "atomicAdd(" in unit and not re.search(r"\basm\b|__shared__", unit)         # plain atomics, no inline assembly, no LDS
    others = [f for f in os.listdir(CSRC) if f.endswith((".hip", ".hpp"))
              and re.search(r"__global__[^;{]*\bk_preview_tune_\w+\s*\(", open(os.path.join(CSRC, f)).read())]
    assert others == ["kernels_preview_tune.hip"]                                       # the kernels live in the new unit only
    capi = open(os.path.join(CSRC, "preview_tune_capi.hip")).read()
    assert "preview_field_check(" in capi and "preview_call_check(" in capi           # the checks of mipnerf_preview_march, by call
    assert not re.search(r"hipMalloc|hipFree|Synchronize|hipMemcpy", capi + unit)


def _field(dims=(8, 9, 10), lo=pf.LO, hi=pf.HI, degree=1, rows=0x1000, occ=0x2000):
    return L.PreviewField((C.c_int32 * 3)(*dims), (C.c_float * 3)(*lo), (C.c_float * 3)(*hi), degree, rows, occ)


def _params(step_scale=0.5, t_min=0.0, max_steps=64, background=WHITE):
    return L.PreviewParams(step_scale, t_min, max_steps, (C.c_float * 3)(*background))


def test_every_entry_point_validates_before_any_hip_call(lib):
    """No device here: a call that reached the HIP runtime would fail with code 3, not with 1 / 2 and a message naming the entry point."""
    P = 0x1000        # never dereferenced: the checks come first

    def grad(field, params, n=4, rays=(P,) * 4, grad_rgb=P, target=None, scale=1.0, grad_acc=None, rgb=P, acc=P, grad_rows=P, counters=None):
        return lib.mipnerf_preview_tune_grad(C.byref(field) if field is not None else None, C.byref(params) if params is not None else None,
                                             n, *rays, grad_rgb, target, scale, grad_acc, rgb, acc, grad_rows, counters, None)

    bad = [
        (lambda: grad(None, _params()), L.E_INVALID), (lambda: grad(_field(), None), L.E_INVALID),
        # everything mipnerf_preview_march checks
        (lambda: grad(_field(rows=None), _params()), L.E_INVALID),
        (lambda: grad(_field(degree=3), _params()), L.E_UNSUPPORTED), (lambda: grad(_field(degree=-1), _params()), L.E_UNSUPPORTED),
        (lambda: grad(_field(dims=(1, 5, 6)), _params()), L.E_INVALID), (lambda: grad(_field(dims=(1024, 1024, 1024)), _params()), L.E_INVALID),
        (lambda: grad(_field(hi=(pf.LO[0], 1.0, 2.375)), _params()), L.E_INVALID),
        (lambda: grad(_field(lo=(float("nan"), -0.75, 0.125)), _params()), L.E_INVALID),
        (lambda: grad(_field(), _params(step_scale=0.0)), L.E_INVALID), (lambda: grad(_field(), _params(step_scale=float("inf"))), L.E_INVALID),
        (lambda: grad(_field(), _params(max_steps=0)), L.E_INVALID), (lambda: grad(_field(), _params(t_min=1.0)), L.E_INVALID),
        (lambda: grad(_field(), _params(t_min=-0.1)), L.E_INVALID), (lambda: grad(_field(), _params(), n=-1), L.E_INVALID),
        (lambda: grad(_field(), _params(), n=2 ** 31), L.E_INVALID),
        (lambda: grad(_field(rows=0x1008), _params()), L.E_INVALID), (lambda: grad(_field(degree=0, rows=0x1004), _params()), L.E_INVALID),
        # exactly one of grad_rgb / target
        (lambda: grad(_field(), _params(), grad_rgb=None, target=None), L.E_INVALID),
        (lambda: grad(_field(), _params(), grad_rgb=P, target=P), L.E_INVALID),
        # a finite loss_scale in target mode
        (lambda: grad(_field(), _params(), grad_rgb=None, target=P, scale=float("nan")), L.E_INVALID),
        (lambda: grad(_field(), _params(), grad_rgb=None, target=P, scale=float("inf")), L.E_INVALID),
        # grad_rows: not NULL, 16-byte aligned
        (lambda: grad(_field(), _params(), grad_rows=None), L.E_INVALID), (lambda: grad(_field(), _params(), grad_rows=0x1008), L.E_INVALID),
        (lambda: grad(_field(), _params(), counters=0x1004), L.E_INVALID),
        # NULL rgb / acc
        (lambda: grad(_field(), _params(), rgb=None), L.E_INVALID), (lambda: grad(_field(), _params(), acc=None), L.E_INVALID),
    ] + [(lambda k=k: grad(_field(), _params(), rays=tuple(None if j == k else P for j in range(4))), L.E_INVALID) for k in range(4)]
    for i, (call, code) in enumerate(bad):
        assert call() == code, i
        assert b"preview_tune_grad" in lib.mipnerf_preview_tune_last_error(), i
    assert grad(_field(), _params(), n=0, rays=(None,) * 4, rgb=None, acc=None) == L.OK
    assert grad(_field(occ=None), _params(), n=0, rays=(None,) * 4, grad_rgb=None, target=P, scale=0.5, rgb=None, acc=None) == L.OK
    assert grad(_field(degree=0, rows=0x1008), _params(), n=0, rays=(None,) * 4, rgb=None, acc=None) == L.OK
    # (a non-finite loss_scale is ignored in grad_rgb mode, and a NULL occupancy / grad_acc is valid: they reach the launch, covered on the GPU)

    def adam(n=4, degree=1, ptrs=(P,) * 5, mask=None, lr_sigma=0.2, lr_colour=0.01, beta1=0.9, beta2=0.999, eps=1e-8, c1=10.0, c2=1000.0):
        return lib.mipnerf_preview_tune_adam(n, degree, *ptrs, mask, lr_sigma, lr_colour, beta1, beta2, eps, c1, c2, None)

    bad = [
        (lambda: adam(degree=3), L.E_UNSUPPORTED), (lambda: adam(degree=-1), L.E_UNSUPPORTED), (lambda: adam(n=-1), L.E_INVALID),
        (lambda: adam(n=2 ** 31), L.E_INVALID),
        (lambda: adam(lr_sigma=float("nan")), L.E_INVALID), (lambda: adam(lr_colour=float("inf")), L.E_INVALID),
        (lambda: adam(beta1=1.0), L.E_INVALID), (lambda: adam(beta2=-0.1), L.E_INVALID), (lambda: adam(eps=-1e-8), L.E_INVALID),
        (lambda: adam(c1=float("inf")), L.E_INVALID), (lambda: adam(c2=float("nan")), L.E_INVALID),
        (lambda: adam(ptrs=(0x1008, P, P, P, P)), L.E_INVALID), (lambda: adam(ptrs=(P, P, P, 0x1004, P)), L.E_INVALID),
        (lambda: adam(ptrs=(P, P, P, P, 0x1004)), L.E_INVALID),
    ] + [(lambda k=k: adam(ptrs=tuple(None if j == k else P for j in range(5))), L.E_INVALID) for k in range(5)]
    for i, (call, code) in enumerate(bad):
        assert call() == code, i
        assert b"preview_tune_adam" in lib.mipnerf_preview_tune_last_error(), i
    assert adam(n=0, ptrs=(None,) * 5) == L.OK
    with pytest.raises(ValueError, match="x: .*preview_tune"):
        L.preview_tune_check(L.E_INVALID, "x")
    with pytest.raises(NotImplementedError):
        L.preview_tune_check(L.E_UNSUPPORTED, "x")


# ---- the fixture against central differences of the float64 march --------------------------------------------------------------------
def _objective(rows64, degree, sub, G, ga):
    rgb, acc = pf.march(rows64, pf.LO, pf.HI, degree, *sub, 0.5, 0.0, 4096, BG)[:2]
    return float((rgb * G).sum() + (acc * ga).sum())


@pytest.mark.parametrize("degree", [0, 1, 2])
def test_fixture_against_central_differences_of_the_float64_march(rays, degree):
    """on the smooth variant (no kink inside a difference step): >= 30 random non-zero entries, |fd - g| <= 1e-5 A_e"""
    rows = tf.smooth_rows(degree)
    assert float(rows[..., 0].min()) >= 0.5
    fragile = pf.march(rows, pf.LO, pf.HI, degree, *rays, 0.5, 0.0, 4096, BG)[4]
    ok = np.flatnonzero(~fragile)[::5]                           # a fifth of the non-fragile rays keeps the differences quick
    sub = tuple(a[ok] for a in rays)
    G, ga, _ = tf.loss_inputs(n=len(ok))
    out = tf.march_grad(rows, pf.LO, pf.HI, degree, *sub, 0.5, 0.0, 4096, BG, grad_rgb=G, grad_acc=ga)
    assert 0.05 <= out["v_range"][0] and out["v_range"][1] <= 0.95
    assert np.abs(out["rgb"] - pf.march(rows, pf.LO, pf.HI, degree, *sub, 0.5, 0.0, 4096, BG)[0]).max() < 1e-12      # the same forward
    rng = np.random.default_rng(7 + degree)
    # a float64 difference quotient of an objective of size ~50 carries a rounding error of ~1e-13 / eps: entries whose every term is
    # smaller than that (corner weights of 1e-10 exist) cannot be checked to 1e-5 A_e by any step, so the draw is among the others
    hit = np.argwhere((out["grad"] != 0) & (out["A"] >= 1e-3 * out["A"].max()))
    assert len(hit) > 200 and (out["count"][..., tf.USED[degree]:] == 0).all() and not out["grad"][..., tf.USED[degree]:].any()
    picks = hit[rng.choice(len(hit), 32, replace=False)]
    picks = np.concatenate([picks, hit[hit[:, 3] == 0][:4]])     # density entries are among them whatever the draw
    rows64 = rows.astype(np.float64)
    worst = 0.0
    for k, j, i, e in picks:
        eps = 1e-3
        up, down = rows64.copy(), rows64.copy()
        up[k, j, i, e] += eps
        down[k, j, i, e] -= eps
        fd = (_objective(up, degree, sub, G, ga) - _objective(down, degree, sub, G, ga)) / (2 * eps)
        err = abs(fd - out["grad"][k, j, i, e]) / out["A"][k, j, i, e]
        worst = max(worst, err)
        assert err <= 1e-5, (degree, (k, j, i, e), fd, out["grad"][k, j, i, e], out["A"][k, j, i, e])
    print(f"degree {degree}: {len(picks)} entries, worst |fd - g| / A_e = {worst:.2e}")


def test_the_clamps_exactly(rays, hm):
    """an entry whose every sample is clamped has gradient exactly 0; a lattice whose blended sigma is negative everywhere has zero density
    gradient (and, all weights being zero, no gradient at all)"""
    G, ga, target = tf.loss_inputs()
    for degree in (0, 1, 2):
        rows = tf.scene_rows(degree)
        bright = rows.copy()
        bright[..., 1:4] = np.float16(2.0 / pf.C0)               # DC alone is 2: with the small coefficients below every colour exceeds 1
        bright[..., 4:] = (bright[..., 4:].astype(F) * F(0.01)).astype(np.float16)
        out = tf.march_grad(bright, pf.LO, pf.HI, degree, *rays, 0.5, 0.0, 4096, WHITE, grad_rgb=G, grad_acc=ga)
        assert out["v_range"][0] > 1.0
        assert not out["grad"][..., 1:].any() and not out["count"][..., 1:].any() and out["grad"][..., 0].any()
        got = host_grad(hm, bright, None, degree, rays, 0.5, 0.0, 4096, WHITE, grad_rgb=G, grad_acc=ga)
        assert not got[0][..., 1:].any() and got[0][..., 0].any()
        dark = rows.copy()
        dark[..., 0] = np.float16(-1.0)
        out = tf.march_grad(dark, pf.LO, pf.HI, degree, *rays, 0.5, 0.0, 4096, WHITE, target=target, loss_scale=0.01)
        assert not out["grad"].any() and not out["count"].any() and (out["acc"] == 0).all()
        got = host_grad(hm, dark, None, degree, rays, 0.5, 0.0, 4096, WHITE, target=target, loss_scale=0.01)
        assert not got[0].any() and (got[2] == 0).all()


# ---- the tolerance, measured on the reference alone ------------------------------------------------------------------------------------
def test_the_measured_fp32_error_of_the_formulas_is_the_constant():
    worst = dict.fromkeys(tf.MODES, 0.0)
    for degree in (0, 1, 2):
        for case in range(len(tf.CASES)):
            for mode in tf.MODES:
                want, got = tf.reference(degree, case, mode), tf.reference(degree, case, mode, F)
                assert got["grad"].dtype == F
                err = float(tf.scaled_error(got["grad"], want["grad"], want["A"]).max())
                print(f"degree {degree} {tf.CASES[case]} {mode}: fp32 fixture against float64 fixture, scaled error {err:.3e}")
                worst[mode] = max(worst[mode], err)
    for mode in tf.MODES:
        assert 0.9 * tf.MEASURED[mode] < worst[mode] <= tf.MEASURED[mode] and tf.LIMIT[mode] == 4 * tf.MEASURED[mode]
    assert [c[:2] for c in tf.CASES[:4]] == [(0.5, 0.0), (0.5, 0.2), (0.1, 0.0), (0.1, 0.2)] and any(c[2] for c in tf.CASES)


# ---- the host build of preview_tune.hpp --------------------------------------------------------------------------------------------------
def host_grad(hm, rows, occupancy, degree, rays, step_scale, t_min, max_steps, background, grad_rgb=None, grad_acc=None, target=None,
              loss_scale=0.0, select=None):
    """(grad_rows, rgb, acc) of the sequential loop over the rules of preview_tune.hpp on the rays `select` (default: all)"""
    o, d, tn, tf_ = [np.ascontiguousarray(a if select is None else a[select]) for a in rays]
    pick = lambda a: None if a is None else np.ascontiguousarray(a if select is None else a[select], F)
    grad_rgb, grad_acc, target = pick(grad_rgb), pick(grad_acc), pick(target)
    nz, ny, nx, W = rows.shape
    B = o.shape[0]
    bits = np.ascontiguousarray(rows).view(np.uint16)
    grad = np.zeros((nz, ny, nx, W), F)
    rgb, acc = np.zeros((B, 3), F), np.zeros(B, F)
    lo, hi, bg = np.array(pf.LO, F), np.array(pf.HI, F), np.array(background, F)
    hm.hm_preview_tune_grad(_p(bits), None if occupancy is None else _p(np.ascontiguousarray(occupancy)), nx, ny, nz, _p(lo), _p(hi), degree,
                            C.c_float(step_scale), C.c_float(t_min), max_steps, _p(bg), C.c_longlong(B), _p(o), _p(d), _p(tn), _p(tf_),
                            _p(grad_rgb), _p(target), C.c_float(loss_scale), _p(grad_acc), _p(rgb), _p(acc), _p(grad))
    return grad, rgb, acc


@pytest.mark.parametrize("degree", [0, 1, 2])
def test_host_build_of_the_rules_is_inside_the_bound(hm, rays, degree):
    for case, (step, t_min, hollow) in enumerate(tf.CASES):
        rows, occ, ok = tf.case_inputs(degree, case)
        for mode in tf.MODES:
            want = tf.reference(degree, case, mode)
            got, rgb, acc = host_grad(hm, rows, occ, degree, rays, step, t_min, 4096, BG, select=ok, **tf.loss_side(mode))
            err = float(tf.scaled_error(got, want["grad"], want["A"]).max())
            print(f"degree {degree} step {step} t_min {t_min} hollow {hollow} {mode}: scaled error {err:.3e}")
            assert err <= tf.LIMIT[mode]
            assert not got[want["count"] == 0].any()
            assert np.abs(rgb - want["rgb"][ok]).max() <= 5e-5 and np.abs(acc - want["acc"][ok]).max() <= 5e-5
            if hollow:
                assert (want["count"].reshape(-1, rows.shape[-1]).sum(1) == 0).any() and want["count"].any()


def test_late_stops_exist_at_the_late_t_min(rays):
    """the GPU test's third t_min: at step 0.1 at least 10 non-fragile rays stop after their 64th sample (in the second or third block
    of 64), at least one of them after its 128th"""
    for degree in (0, 1, 2):
        rows = tf.scene_rows(degree)
        free = pf.march(rows, pf.LO, pf.HI, degree, *rays, 0.1, 0.0, 4096, WHITE)
        late = pf.march(rows, pf.LO, pf.HI, degree, *rays, 0.1, LATE_T_MIN, 4096, WHITE)
        assert late[4].mean() <= 0.10
        stopped = (late[3] < free[3]) & ~late[4]
        assert int((stopped & (late[3] > 64)).sum()) >= 10 and int((stopped & (late[3] > 128)).sum()) >= 1
        assert int((free[3] > 128).sum()) >= 10                      # and without a stop rays run through three blocks


def host_adam(hm, master, m, v, grad, rows, mask, degree, scalars):
    hm.hm_preview_tune_adam(C.c_longlong(master.shape[0]), degree, _p(master), _p(m), _p(v), _p(grad), _p(rows.view(np.uint16)), _p(mask),
                            *[C.c_float(x) for x in scalars])


def adam_inputs(degree, n, seed=3):
    """ragged n, random state, sentinels in the pad entries, a mask, sigma entries that saturate at 65504 and one NaN gradient"""
    rng = np.random.default_rng(seed + degree)
    W = pf.ROW_HALVES[degree]
    master = rng.normal(0.0, 1.0, (n, W)).astype(F)
    master[:, 0] = rng.uniform(0.0, 50.0, n).astype(F)
    master[::7, 0] = F(65503.0)
    m, v = rng.normal(0.0, 0.1, (n, W)).astype(F), rng.uniform(0.0, 0.01, (n, W)).astype(F)
    grad = rng.normal(0.0, 1.0, (n, W)).astype(F)
    grad[::7, 0] = F(-30.0)                                      # pushes the saturating sigma up
    grad[5, 2] = F(np.nan)
    grad[11] = F(0.0)
    rows = master.astype(np.float16)
    for a in (master, m, v, grad):
        a[:, tf.USED[degree]:] = F(777.0)
    rows[:, tf.USED[degree]:] = np.float16(0.5)
    mask = (rng.uniform(size=n) < 0.6).astype(np.uint8)
    return [master, m, v, grad, rows], mask


@pytest.mark.parametrize("degree", [0, 1, 2])
def test_host_adam_is_the_fixtures_float32_adam_bit_for_bit(hm, degree):
    for mask_on in (True, False):
        want, mask = adam_inputs(degree, 723)
        got = [a.copy() for a in want]
        pads = [a[:, tf.USED[degree]:].copy() for a in want]
        for step in (1, 2):
            c1, c2 = tf.bias_corrections(0.9, 0.999, step)
            scalars = (0.2, 0.01, 0.9, 0.999, 1e-8, c1, c2)
            tf.adam(*want, mask if mask_on else None, degree, *scalars)
            host_adam(hm, *got, mask if mask_on else None, degree, scalars)
            for a, b, name in zip(got, want, ("master", "m", "v", "grad", "rows")):
                assert a.tobytes() == b.tobytes(), (degree, mask_on, step, name)
            want[3][...] = got[3][...] = np.random.default_rng(step).normal(size=want[3].shape).astype(F)      # the next gradient (pads too)
            pads[3] = want[3][:, tf.USED[degree]:].copy()
            if step == 1:
                assert (want[4][::7, 0][(mask[::7] != 0) | (not mask_on)] == np.float16(65504.0)).all()         # saturated, not inf
                assert np.isnan(want[0][5, 2]) == bool(mask[5] or not mask_on)
        for a, p in zip(want[:3] + [want[4]], pads[:3] + [pads[4]]):
            assert a[:, tf.USED[degree]:].tobytes() == p.tobytes()                                               # pads never touched
        if mask_on:
            off = mask == 0
            fresh, _ = adam_inputs(degree, 723)
            assert np.array_equal(want[0][off], fresh[0][off]) and np.array_equal(want[4][off], fresh[4][off])  # a masked point keeps its row


# ---- python layer without a device -----------------------------------------------------------------------------------------------------
def test_tuning_targets_are_refused_by_kind():
    from mipnerf_pl_amd import preview
    import test_preview_sparse_cpu as sparse_cpu
    field = sparse_cpu._sparse((8, 9, 10))[0]
    o, d, tn, tf_ = [torch.from_numpy(a) for a in pf.scene_rays()]
    with pytest.raises(NotImplementedError, match="SparseField is not a tuning target"):
        preview.march_grad(field, o, d, tn, tf_, WHITE, grad_rgb=torch.zeros(257, 3))
    with pytest.raises(NotImplementedError, match="SparseField is not a tuning target"):
        preview.TuneState(field)
    pyr = preview.BakedPyramid([field.to_dense()])
    with pytest.raises(NotImplementedError, match="BakedPyramid is not a tuning target"):
        preview.TuneState(pyr)
    with pytest.raises(NotImplementedError, match="BakedPyramid is not a tuning target"):
        preview.tune_field(pyr, lambda k: None, 1)
    dense = field.to_dense()
    with pytest.raises(ValueError, match="exactly one of grad_rgb and target"):
        preview.march_grad(dense, o, d, tn, tf_, WHITE)
    with pytest.raises(ValueError, match="exactly one of grad_rgb and target"):
        preview.march_grad(dense, o, d, tn, tf_, WHITE, grad_rgb=torch.zeros(257, 3), target=torch.zeros(257, 3), loss_scale=1.0)
    with pytest.raises(ValueError, match="target needs loss_scale"):
        preview.march_grad(dense, o, d, tn, tf_, WHITE, target=torch.zeros(257, 3))
    with pytest.raises(ValueError, match="grad_rows must be a contiguous fp32 tensor"):
        preview.march_grad(dense, o, d, tn, tf_, WHITE, grad_rgb=torch.zeros(257, 3), grad_rows=torch.zeros(10, 9, 8, 4))
    with pytest.raises(ValueError, match="at least one step"):
        preview.tune_field(dense, lambda k: None, 0)
    # the state: fp32 masters of the fp16 rows, the mask of the points next to an occupied cell
    state = preview.TuneState(dense)
    assert state.master.dtype == torch.float32 and torch.equal(state.master.to(torch.float16), dense.rows)
    assert torch.equal(state.mask.bool(), preview.baked_points(dense.occupancy)) and state.steps == 0
    assert (state.lr_sigma, state.lr_colour, state.betas, state.eps) == (0.2, 0.01, (0.9, 0.999), 1e-8)
    other = preview.TuneState(dense, lr_sigma=0.5)
    saved = state.state_dict()
    saved["steps"], saved["m"] = 7, torch.ones_like(state.m)
    other.load_state_dict(saved)
    assert other.steps == 7 and other.lr_sigma == 0.2 and bool((other.m == 1).all())
    assert torch.equal(preview.pack_master(torch.tensor([[70000.0, 70000.0, 0.1, -2.0]]), 0),
                       torch.tensor([[65504.0, float("inf"), 0.1, -2.0]]).to(torch.float16))


# ---- command line ------------------------------------------------------------------------------------------------------------------------
def test_parser_tune():
    from mipnerf_pl_amd import preview
    p = preview.build_parser()
    a = p.parse_args(["--out_dir", "o"])
    assert a.tune is None and all(getattr(a, f) is None for f in preview.TUNE_FLAGS)
    a = p.parse_args(["--out_dir", "o", "--tune", "500"])
    assert a.tune == 500 and a.tune_batch is None and a.tune_target is None
    assert (preview.DEFAULT_TUNE_BATCH, preview.DEFAULT_TUNE_LR_SIGMA, preview.DEFAULT_TUNE_LR_COLOUR) == (65536, 0.2, 0.01)
    a = p.parse_args(["--out_dir", "o", "--tune", "3", "--tune_batch", "512", "--tune_lr_sigma", "0.5", "--tune_lr_colour", "0.02",
                      "--tune_target", "mlp", "--tune_seed", "4"])
    assert (a.tune, a.tune_batch, a.tune_lr_sigma, a.tune_lr_colour, a.tune_target, a.tune_seed) == (3, 512, 0.5, 0.02, "mlp", 4)
    with pytest.raises(SystemExit):
        p.parse_args(["--out_dir", "o", "--tune", "3", "--tune_target", "pictures"])
    text = re.sub(r"\s+", " ", p.format_help())
    for flag in ("--tune STEPS", "--tune_batch", "--tune_lr_sigma", "--tune_lr_colour", "--tune_target {photos,mlp}", "--tune_seed"):
        assert flag in text, flag
    assert "ON THE RENDERED POSES" in text and text.count("a choice, not a measurement") >= 2 and "peak memory is the dense bake's" in text
    from mipnerf_pl_amd import eval as eval_cli
    from mipnerf_pl_amd import render_video
    for parser in (eval_cli.build_parser(), render_video.build_parser()):
        assert "--tune" not in parser.format_help()


def test_tune_refusals_come_before_the_checkpoint_is_opened(tmp_path):
    from mipnerf_pl_amd import preview
    import test_preview_sparse_cpu as sparse_cpu
    missing = str(tmp_path / "no_such.ckpt")               # never opened: the refusal comes first
    out = str(tmp_path / "o")
    base = ["--ckpt", missing, "--out_dir", out]
    sparse_file = sparse_cpu._sparse((8, 9, 10))[0].save(str(tmp_path / "s.npz"))
    for extra, why in ((["--tune", "3", "--mip"], "--tune with --mip"), (["--tune", "3", "--mip", "2"], "--tune with --mip"),
                       (["--tune", "3", "--baked", sparse_file, "--sparse"], "--tune with a sparse --baked file"),
                       (["--tune", "3", "--tune_target", "photos"], "--tune_target photos .* give --data"),
                       (["--tune", "0"], "--tune 0: at least one step"), (["--tune", "-2"], "at least one step"),
                       (["--tune", "3", "--tune_batch", "0"], "--tune_batch 0"),
                       (["--tune", "3", "--tune_lr_sigma", "-1"], "--tune_lr_sigma"),
                       (["--tune_batch", "512"], "--tune_batch belongs to --tune"), (["--tune_lr_sigma", "0.1"], "--tune_lr_sigma belongs to --tune"),
                       (["--tune_lr_colour", "0.1"], "belongs to --tune"), (["--tune_target", "mlp"], "belongs to --tune"),
                       (["--tune_seed", "1"], "--tune_seed belongs to --tune")):
        with pytest.raises(SystemExit, match=why):
            preview.main(base + extra)
    for ok in (["--tune", "3"], ["--tune", "3", "--sparse"], ["--tune", "3", "--tune_target", "mlp", "--data", str(tmp_path)],
               ["--tune", "3", "--tune_target", "photos", "--data", str(tmp_path)]):
        with pytest.raises(FileNotFoundError):             # nothing to refuse: on to the (missing) checkpoint
            preview.main(base + ok)
    assert not os.path.exists(out)


# ---- the convergence recipe, on the reference alone ----------------------------------------------------------------------------------------
def test_the_reference_converges_on_the_recipe(rays):
    """degree 1, teacher = the scene, t_min 1e-3, step 0.5, white background, target = the teacher's march; student = `student_rows`; the full
    batch of non-fragile rays, lr_sigma 0.2, lr_colour 0.02, float64 gradients, float32 Adam, rows re-rounded to fp16 every step.  Measured:
    the mean squared error goes from 1.52e-3 to 7.2e-6 in 40 steps (ratio 0.0047).  The GPU test's threshold (0.05) rests on this."""
    teacher = tf.scene_rows(1)
    want = pf.march(teacher, pf.LO, pf.HI, 1, *rays, 0.5, 1e-3, 4096, WHITE)
    ok = np.flatnonzero(~want[4])
    target = want[0].astype(F)
    rows = tf.student_rows(teacher, 1)
    shape = rows.shape
    rows = rows.reshape(-1, 16)
    master = rows.astype(F)
    m, v = np.zeros_like(master), np.zeros_like(master)
    losses = []
    for k in range(41):
        out = tf.march_grad(rows.reshape(shape), pf.LO, pf.HI, 1, *rays, 0.5, 1e-3, 4096, WHITE, target=target, loss_scale=2.0 / (3 * len(ok)),
                            rays=ok)
        losses.append(float(((out["rgb"][ok] - target[ok]) ** 2).mean()))
        if k < 40:
            c1, c2 = tf.bias_corrections(0.9, 0.999, k + 1)
            tf.adam(master, m, v, out["grad"].astype(F).reshape(-1, 16), rows, None, 1, 0.2, 0.02, 0.9, 0.999, 1e-8, c1, c2)
    print(f"loss {losses[0]:.3e} -> {losses[-1]:.3e} (ratio {losses[-1] / losses[0]:.4f})")
    assert losses[-1] <= 0.02 * losses[0]
