"""CPU (no GPU): tuning the contracted preview lattice -- the ninth library's declarations, bindings, exports and argument checks without a
device; the numpy restatement of rules C6 - C8 (tests/preview_tune360_fixture.py) against central differences of the float64 march of
tests/preview360_fixture.py; the rules of csrc/preview_tune_360.hpp (g++ -O2 -ffp-contract=off from tests/hostmath/preview_tune_360.cpp)
against the fixture, per sample bit for bit; six deliberate mistakes that each miss the limit; the module's and the command's refusals;
the convergence recipe the GPU test repeats.

THE TOLERANCE OF THE GRADIENT.  Scaled error = |got - want| / (A_e + 1e-3 max_e A_e), A_e the sum of the absolute values of the terms of
entry e (the fixture returns it).  It is measured on the reference alone: the fixture's own float32 run (float32 tan / arctan and edge
differences included) against its float64 run on the same inputs, degrees 0 - 2, every case and both loss sides, on the non-fragile rays.
Largest values so measured: 5.66e-6 with a given grad_rgb, 9.60e-6 in target mode; preview_tune360_fixture.MEASURED rounds them up and LIMIT
is 4 x MEASURED per mode: the margin covers another summation order (wave scans, atomics) and expf / tanf a few ulp apart."""
import ctypes as C
import os
import re
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import preview360_fixture as pf
import preview_tune360_fixture as tf
from mipnerf_pl_amd import _lib as L

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
CSRC = os.path.join(REPO, "mipnerf_pl_amd", "csrc")
F = np.float32
WHITE = (1.0, 1.0, 1.0)
BG = tf.BG
R = tf.R


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.PREVIEW_TUNE_360_LIB_PATH):
        from mipnerf_pl_amd import build
        build.build(verbose=False)
    return L.preview_tune_360_lib()


def host():
    src, so = os.path.join(HERE, "hostmath", "preview_tune_360.cpp"), os.path.join(HERE, "hostmath", "_preview_tune_360.so")
    hdrs = [os.path.join(CSRC, h) for h in ("raymath.hpp", "lattice_sample.hpp", "preview_march.hpp", "preview_march_360.hpp", "preview_tune.hpp",
                                            "preview_tune_360.hpp")]
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


# ---- the ninth library: declarations, bindings, exports ----------------------------------------------------------------------------
NAMES = ["mipnerf_preview_tune_360_abi_version", "mipnerf_preview_tune_360_grad", "mipnerf_preview_tune_360_last_error"]


def _header(name="mipnerf_preview_tune_360.h", comments=False):
    text = open(os.path.join(REPO, "include", name)).read()
    return text if comments else re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return sorted(line.split()[-1] for line in out.splitlines() if line.strip())


def test_header_bindings_and_dynamic_symbols_are_one_set(lib):
    declared = sorted(set(re.findall(r"\b(mipnerf_[a-z0-9_]+)\s*\(", _header())))
    assert declared == sorted(L.PREVIEW_TUNE_360_SIGNATURES) == NAMES
    assert _exports(L.PREVIEW_TUNE_360_LIB_PATH) == declared
    for name, (_, args) in L.PREVIEW_TUNE_360_SIGNATURES.items():
        proto = re.search(r"\b" + name + r"\s*\(([^)]*)\)", _header()).group(1).strip()
        count = 0 if proto in ("", "void") else proto.count(",") + 1
        assert count == len(args), (name, proto)
    assert lib.mipnerf_preview_tune_360_abi_version() == 1 == L.PREVIEW_TUNE_360_ABI
    text = re.sub(r"\s+\*?\s*", " ", _header(comments=True))
    for rule in ("C6. q_i = sum_c G_c (colour_{i,c} - background_c) + g_a", "C7.", "delta_i (T_{i+1} q_i - S_i)", "C8.", "NOT BITWISE REPRODUCIBLE",
                 "The contributions of ONE ray arrive in a fixed order"):
        assert rule in text, rule


def test_the_other_libraries_keep_their_tables(lib):
    others = dict(hip=L.SIGNATURES, diag=L.DIAG_SIGNATURES, preview=L.PREVIEW_SIGNATURES, mip=L.PREVIEW_MIP_SIGNATURES,
                  sparse=L.PREVIEW_SPARSE_SIGNATURES, tune=L.PREVIEW_TUNE_SIGNATURES, p360=L.PREVIEW_360_SIGNATURES, reg=L.PREVIEW_REG_SIGNATURES)
    assert [len(t) for t in others.values()] == [93, 3, 4, 3, 7, 4, 4, 3]
    for table in others.values():
        assert not set(table) & set(L.PREVIEW_TUNE_360_SIGNATURES) and not any("tune_360" in n for n in table)
    for path, table in ((L.PREVIEW_TUNE_LIB_PATH, L.PREVIEW_TUNE_SIGNATURES), (L.PREVIEW_360_LIB_PATH, L.PREVIEW_360_SIGNATURES),
                        (L.PREVIEW_REG_LIB_PATH, L.PREVIEW_REG_SIGNATURES)):
        assert _exports(path) == sorted(table)


def test_the_build_units_are_compiled_without_contraction_into_a_ninth_library():
    from mipnerf_pl_amd import build as b
    assert [u for u, _ in b.PREVIEW_TUNE_360_UNITS] == ["kernels_preview_tune_360.hip", "preview_tune_360_capi.hip"]
    assert all("-ffp-contract=off" in flags for _, flags in b.PREVIEW_TUNE_360_UNITS)
    assert os.path.basename(b.PREVIEW_TUNE_360_LIB) == "libmipnerf_preview_tune_360.so" == os.path.basename(L.PREVIEW_TUNE_360_LIB_PATH)
    assert not any("tune_360" in u for u, _ in b.UNITS + b.DIAG_UNITS + b.PREVIEW_UNITS + b.PREVIEW_MIP_UNITS + b.PREVIEW_SPARSE_UNITS +
                   b.PREVIEW_TUNE_UNITS + b.PREVIEW_360_UNITS + b.PREVIEW_REG_UNITS)
    src = open(os.path.join(REPO, "mipnerf_pl_amd", "build.py")).read()
    assert '"include", "mipnerf_preview_tune_360.h"' in src and "os.path.exists(PREVIEW_TUNE_360_LIB)" in src
    rules = open(os.path.join(CSRC, "preview_tune_360.hpp")).read()
    assert "MIP_HD" in rules and '#include "preview_march_360.hpp"' in rules and '#include "preview_tune.hpp"' in rules
    assert not re.search(r"floorf|inv_h\[|expf|tanf|atanf|sqrtf", rules)               # restates neither the cell, the warp nor the contraction
    unit = open(os.path.join(CSRC, "kernels_preview_tune_360.hip")).read()
    assert '#include "preview_wave_march.hpp"' in unit and '#include "preview_tune_360.hpp"' in unit
    assert re.search(r"__global__[^;{]*\bk_preview_360_tune_grad\s*\(", unit)
    assert len(re.findall(r"\btune360_block<DEG>\(", unit)) == 2                        # ONE block function, one call per sweep
    for call in ("preview360_sample_w(", "preview360_exists(", "preview360_unwarp(", "preview360_upper_edge(", "tune360_cell(", "tune360_delta(",
                 "preview_occupied(", "preview_row<", "preview_shade<", "wave_incl_prod_dpp(", "tune_q(", "tune360_d_sigma(", "tune_d_colour(",
                 "tune_corner_weight(", "readfirstlane"):
        assert call in unit, call
    assert "atomicAdd(" in unit and not re.search(r"\basm\b|__shared__", unit)         # plain atomics, no inline assembly, no LDS
    capi = open(os.path.join(CSRC, "preview_tune_360_capi.hip")).read()
    assert "preview_field_check(" in capi and "preview_call_check(" in capi
    assert not re.search(r"hipMalloc|hipFree|Synchronize|hipMemcpy", capi + unit)
    entry = open(os.path.join(REPO, "__graft_entry__.py")).read()
    assert entry.count("preview_tune_360_lib()") == 1


def _field(dims=(8, 9, 10), lo=pf.LO, hi=pf.HI, degree=1, rows=0x1000, occ=0x2000):
    return L.PreviewField((C.c_int32 * 3)(*dims), (C.c_float * 3)(*lo), (C.c_float * 3)(*hi), degree, rows, occ)


def _params(step_scale=0.5, t_min=0.0, max_steps=64, background=WHITE):
    return L.PreviewParams(step_scale, t_min, max_steps, (C.c_float * 3)(*background))


def test_the_entry_point_validates_before_any_hip_call(lib):
    """No device here: a call that reached the HIP runtime would fail with code 3, not with 1 / 2 and a message naming the entry point."""
    P = 0x1000        # never dereferenced: the checks come first

    def grad(field, params, radius=8.0, n=4, rays=(P,) * 4, grad_rgb=P, target=None, scale=1.0, grad_acc=None, rgb=P, acc=P, grad_rows=P,
             counters=None):
        return lib.mipnerf_preview_tune_360_grad(C.byref(field) if field is not None else None, radius,
                                                 C.byref(params) if params is not None else None, n, *rays, grad_rgb, target, scale, grad_acc, rgb,
                                                 acc, grad_rows, counters, None)

    bad = [
        (lambda: grad(None, _params()), L.E_INVALID), (lambda: grad(_field(), None), L.E_INVALID),
        # everything mipnerf_preview_360_march checks
        (lambda: grad(_field(rows=None), _params()), L.E_INVALID),
        (lambda: grad(_field(degree=3), _params()), L.E_UNSUPPORTED), (lambda: grad(_field(degree=-1), _params()), L.E_UNSUPPORTED),
        (lambda: grad(_field(dims=(1, 5, 6)), _params()), L.E_INVALID), (lambda: grad(_field(dims=(1024, 1024, 1024)), _params()), L.E_INVALID),
        (lambda: grad(_field(hi=(pf.LO[0], 1.0, 2.375)), _params()), L.E_INVALID),
        (lambda: grad(_field(lo=(float("nan"), -0.75, 0.125)), _params()), L.E_INVALID),
        (lambda: grad(_field(), _params(), radius=1.0), L.E_INVALID), (lambda: grad(_field(), _params(), radius=float("inf")), L.E_INVALID),
        (lambda: grad(_field(), _params(), radius=float("nan")), L.E_INVALID), (lambda: grad(_field(), _params(), radius=-3.0), L.E_INVALID),
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
        assert b"preview_tune_360_grad" in lib.mipnerf_preview_tune_360_last_error(), i
    assert grad(_field(), _params(), n=0, rays=(None,) * 4, rgb=None, acc=None) == L.OK
    assert grad(_field(occ=None), _params(), n=0, rays=(None,) * 4, grad_rgb=None, target=P, scale=0.5, rgb=None, acc=None) == L.OK
    with pytest.raises(ValueError, match="x: .*preview_tune_360"):
        L.preview_tune_360_check(L.E_INVALID, "x")
    with pytest.raises(NotImplementedError):
        L.preview_tune_360_check(L.E_UNSUPPORTED, "x")


# ---- the tolerance, measured on the reference alone ------------------------------------------------------------------------------------
def test_the_measured_fp32_error_of_the_formulas_is_the_constant():
    assert tf.CASES == [(0.5, 0.0, False), (0.5, 0.2, False), (0.05, 0.0, False), (0.05, 0.2, False), (0.1, 0.2, True), (0.05, 0.0, True)]
    assert tf.BG == (0.0, 0.25, 0.5) and tf.LOSS_SCALE == 0.37 and pf.N_RAYS == 270 and pf.DIMS == (9, 10, 11)
    worst = dict.fromkeys(tf.MODES, 0.0)
    for degree in (0, 1, 2):
        for case in range(len(tf.CASES)):
            _, _, ok = tf.case_inputs(degree, case)
            assert len(ok) >= 0.9 * pf.N_RAYS                    # at most 10 % of the rays are fragile and left out
            for mode in tf.MODES:
                want, got = tf.reference(degree, case, mode), tf.reference(degree, case, mode, F)
                assert got["grad"].dtype == F
                # the two runs visit the same cells on every non-fragile ray
                assert all(want["cells"][int(b)] == got["cells"][int(b)] for b in ok), (degree, case)
                err = float(tf.scaled_error(got["grad"], want["grad"], want["A"]).max())
                print(f"degree {degree} {tf.CASES[case]} {mode}: fp32 fixture against float64 fixture, scaled error {err:.3e}, "
                      f"{pf.N_RAYS - len(ok)} fragile rays")
                worst[mode] = max(worst[mode], err)
    for mode in tf.MODES:
        assert 0.9 * tf.MEASURED[mode] < worst[mode] <= tf.MEASURED[mode] and tf.LIMIT[mode] == 4 * tf.MEASURED[mode]


def test_the_cases_cross_block_boundaries_and_stop_late(rays):
    """step 0.05: most rays pass one 64-sample block, tens pass two; with t_min 0.2 some early stops fall behind the 64th counted sample"""
    for degree in (0, 1, 2):
        free = tf.reference(degree, 2, "grad")
        steps = free["steps"][free["steps"] >= 0]
        assert int(steps.max()) > 256 and int((steps > 64).sum()) >= 150 and int((steps > 128).sum()) >= 40
        early = tf.reference(degree, 3, "grad")
        _, _, ok = tf.case_inputs(degree, 3)
        stopped = early["steps"][ok] < free["steps"][ok]
        assert int((stopped & (early["steps"][ok] > 64)).sum()) >= 3, degree
        rows, occ, _ = tf.case_inputs(degree, 5)
        hollow = tf.reference(degree, 5, "grad")
        assert (hollow["count"].reshape(-1, rows.shape[-1]).sum(1) == 0).any() and hollow["count"].any()
        assert not hollow["grad"][..., tf.USED[degree]:].any() and not hollow["count"][..., tf.USED[degree]:].any()


# ---- the fixture against central differences of the float64 march --------------------------------------------------------------------
def _objective(rows64, degree, sub, G, ga):
    rgb, acc = pf.march(rows64, pf.LO, pf.HI, degree, R, *sub, 0.5, 0.0, 4096, BG)[:2]
    return float((rgb * G).sum() + (acc * ga).sum())


@pytest.mark.parametrize("degree", [0, 1, 2])
def test_fixture_against_central_differences_of_the_float64_march(rays, degree):
    """on the smooth variant (no kink inside a difference step): a handful of entries per degree, |fd - g| <= 1e-5 A_e"""
    rows = tf.smooth_rows(degree)
    assert float(rows[..., 0].min()) >= 0.5
    fragile = pf.march(rows, pf.LO, pf.HI, degree, R, *rays, 0.5, 0.0, 4096, BG)[4]
    ok = np.flatnonzero(~fragile)[::5]                           # a fifth of the non-fragile rays keeps the differences quick
    sub = tuple(a[ok] for a in rays)
    G, ga, _ = tf.loss_inputs(n=len(ok))
    out = tf.march_grad(rows, pf.LO, pf.HI, degree, R, *sub, 0.5, 0.0, 4096, BG, grad_rgb=G, grad_acc=ga)
    assert 0.05 < out["v_range"][0] and out["v_range"][1] < 0.95
    assert np.abs(out["rgb"] - pf.march(rows, pf.LO, pf.HI, degree, R, *sub, 0.5, 0.0, 4096, BG)[0]).max() < 1e-12      # the same forward
    rng = np.random.default_rng(7 + degree)
    hit = np.argwhere((out["grad"] != 0) & (out["A"] >= 1e-3 * out["A"].max()))
    assert len(hit) > 100 and (out["count"][..., tf.USED[degree]:] == 0).all() and not out["grad"][..., tf.USED[degree]:].any()
    picks = hit[rng.choice(len(hit), 8, replace=False)]
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


# ---- six deliberate mistakes, each caught by the limit on a named case -----------------------------------------------------------------
MUTATIONS = [("s_for_delta", 1, 0, "grad"), ("t_i_for_t_next", 1, 0, "grad"), ("prefix_for_suffix", 1, 1, "target"),
             ("y_from_contracted_direction", 1, 0, "grad"), ("cell_from_x", 0, 0, "grad"), ("last_remainder_dropped", 1, 0, "grad")]


@pytest.mark.parametrize("name,degree,case,mode", MUTATIONS)
def test_each_mistake_misses_the_limit(rays, name, degree, case, mode):
    step, t_min, _ = tf.CASES[case]
    rows, occ, ok = tf.case_inputs(degree, case)
    want = tf.reference(degree, case, mode)
    got = tf.march_grad(rows, pf.LO, pf.HI, degree, R, *rays, step, t_min, 4096, BG, occ, rays=ok, mutate=name, **tf.loss_side(mode))
    if name != "last_remainder_dropped":                         # the other mistakes sit in the backward alone
        assert np.abs(got["rgb"][ok] - want["rgb"][ok]).max() == 0.0
    err = float(tf.scaled_error(got["grad"], want["grad"], want["A"]).max())
    print(f"{name} on degree {degree} {tf.CASES[case]} {mode}: scaled error {err:.3e} against the limit {tf.LIMIT[mode]:.1e}")
    assert err > 10 * tf.LIMIT[mode]


# ---- the host build of preview_tune_360.hpp ------------------------------------------------------------------------------------------------
def host_grad(hm, rows, occupancy, degree, rays, step_scale, t_min, max_steps, background, grad_rgb=None, grad_acc=None, target=None,
              loss_scale=0.0, select=None):
    """(grad_rows, rgb, acc) of the sequential loop over the rules of preview_tune_360.hpp on the rays `select` (default: all)"""
    o, d, tn, tf_ = [np.ascontiguousarray(a if select is None else a[select]) for a in rays]
    pick = lambda a: None if a is None else np.ascontiguousarray(a if select is None else a[select], F)
    grad_rgb, grad_acc, target = pick(grad_rgb), pick(grad_acc), pick(target)
    nz, ny, nx, W = rows.shape
    B = o.shape[0]
    bits = np.ascontiguousarray(rows).view(np.uint16)
    grad = np.zeros((nz, ny, nx, W), F)
    rgb, acc = np.zeros((B, 3), F), np.zeros(B, F)
    lo, hi, bg = np.array(pf.LO, F), np.array(pf.HI, F), np.array(background, F)
    hm.hm_preview_tune360_grad(_p(bits), None if occupancy is None else _p(np.ascontiguousarray(occupancy)), nx, ny, nz, _p(lo), _p(hi), degree,
                               C.c_float(R), C.c_float(step_scale), C.c_float(t_min), max_steps, _p(bg), C.c_longlong(B), _p(o), _p(d), _p(tn),
                               _p(tf_), _p(grad_rgb), _p(target), C.c_float(loss_scale), _p(grad_acc), _p(rgb), _p(acc), _p(grad))
    return grad, rgb, acc


@pytest.mark.parametrize("degree", [0, 1, 2])
def test_host_build_of_the_rules_is_inside_the_bound(hm, rays, degree):
    for case, (step, t_min, hollow) in enumerate(tf.CASES):
        rows, occ, ok = tf.case_inputs(degree, case)
        for mode in tf.MODES:
            want = tf.reference(degree, case, mode)
            got, rgb, acc = host_grad(hm, rows, occ, degree, rays, step, t_min, 4096, BG, select=ok, **tf.loss_side(mode))
            err = float(tf.scaled_error(got, want["grad"], want["A"]).max())
            print(f"degree {degree} step {step} t_min {t_min} hollow {hollow} {mode}: scaled error {err:.3e} ({err / tf.LIMIT[mode]:.2f} of the limit)")
            assert err <= tf.LIMIT[mode]
            assert not got[want["count"] == 0].any()
            assert np.abs(rgb - want["rgb"][ok]).max() <= 5e-5 and np.abs(acc - want["acc"][ok]).max() <= 5e-5


def test_host_per_sample_functions_are_the_float32_restatement_bit_for_bit(hm):
    rng = np.random.default_rng(11)
    n = 4096
    G, ga, bg = rng.normal(size=3).astype(F), F(rng.normal()), np.array(BG, F)
    e_lo = rng.uniform(0.0, 5.0, n).astype(F)
    e_hi = (e_lo + rng.uniform(-0.1, 1.0, n).astype(F)).astype(F)                      # some edges in the wrong order: delta clamps at 0
    colour = rng.uniform(-0.2, 1.2, (n, 3)).astype(F)
    colour = np.where(colour < 0, F(0), np.where(colour > 1, F(1), colour)).astype(F)
    w, t_next, rest = rng.uniform(0, 1, n).astype(F), rng.uniform(0, 1, n).astype(F), rng.normal(size=n).astype(F)
    row0 = rng.normal(size=n).astype(F)
    row0[::9] = F(0.0)
    fr = rng.uniform(0, 1, (n, 3)).astype(F)
    delta, q, ds = np.zeros(n, F), np.zeros(n, F), np.zeros(n, F)
    dc, corner = np.zeros((n, 3), F), np.zeros((n, 8), F)
    hm.hm_preview_tune360_samples(n, _p(G), C.c_float(ga), _p(bg), _p(e_lo), _p(e_hi), _p(colour), _p(w), _p(t_next), _p(rest), _p(row0), _p(fr),
                                  _p(delta), _p(q), _p(ds), _p(dc), _p(corner))
    want_delta = np.maximum(e_hi - e_lo, F(0.0))
    want_q = ((G[0] * (colour[:, 0] - bg[0]) + G[1] * (colour[:, 1] - bg[1])) + G[2] * (colour[:, 2] - bg[2])) + ga
    want_ds = np.where(row0 > 0, want_delta * (t_next * want_q - rest), F(0.0)).astype(F)
    want_dc = np.where((colour > 0) & (colour < 1), w[:, None] * G[None, :], F(0.0)).astype(F)
    want_corner = np.zeros((n, 8), F)
    for k in range(8):
        a, b, c = k & 1, (k >> 1) & 1, k >> 2
        wx = fr[:, 0] if a else F(1.0) - fr[:, 0]
        wy = fr[:, 1] if b else F(1.0) - fr[:, 1]
        wz = fr[:, 2] if c else F(1.0) - fr[:, 2]
        want_corner[:, k] = (wx * wy) * wz
    for got, want, name in ((delta, want_delta, "delta"), (q, want_q, "q"), (ds, want_ds, "d_sigma"), (dc, want_dc, "d_colour"),
                            (corner, want_corner, "corner")):
        assert want.dtype == F and got.tobytes() == want.tobytes(), name
    assert (delta == 0).any() and (ds == 0).any() and (dc == 0).any()
    # C8: the cell is lattice_cell of z = contract(x), not of x: far out on a ray x lies outside the box and z inside
    o, d = np.array([0.1, -0.2, 0.05], F), np.array([0.6, -0.48, 0.64], F)
    t = np.array([0.0, 0.5, 1.5, 3.0, 7.5, 100.0], F)
    inside, c, frac = np.zeros(6, np.int32), np.zeros((6, 3), np.int32), np.zeros((6, 3), F)
    nx, ny, nz = pf.DIMS
    hm.hm_preview_tune360_cells(nx, ny, nz, _p(np.array(pf.LO, F)), _p(np.array(pf.HI, F)), _p(o), _p(d), 6, _p(t), _p(inside), _p(c), _p(frac))
    x = o[None, :] + t[:, None] * d[None, :]
    n2 = (x[:, 0] * x[:, 0] + x[:, 1] * x[:, 1]) + x[:, 2] * x[:, 2]
    norm = np.sqrt(n2)
    k = np.where(n2 > 1, (F(2.0) - F(1.0) / norm) / norm, F(1.0)).astype(F)
    z = np.where(n2[:, None] > 1, x * k[:, None], x).astype(F)
    lo, hi = np.array(pf.LO, F), np.array(pf.HI, F)
    want_inside = ((z >= lo) & (z <= hi)).all(-1)
    assert inside.astype(bool).tolist() == want_inside.tolist() and want_inside.any() and (np.abs(x) > 2).any()
    inv_h = (np.array(pf.DIMS) - 1).astype(F) / (hi - lo)
    u = np.clip((z - lo) * inv_h, F(0.0), (np.array(pf.DIMS) - 1).astype(F)).astype(F)
    cell = np.minimum(np.floor(u).astype(np.int32), np.array(pf.DIMS) - 2)
    on = want_inside
    assert np.array_equal(c[on], cell[on]) and frac[on].tobytes() == (u - cell.astype(F))[on].astype(F).tobytes()


# ---- python layer without a device -----------------------------------------------------------------------------------------------------
def _cpu_field(degree=1, space="contracted", far_radius=R):
    from mipnerf_pl_amd import preview
    from mipnerf_pl_amd.ops import Occupancy
    rows, sigma = pf.random_rows(degree, hollow=True)
    words = torch.from_numpy(pf.occupancy_words(sigma).view(np.int32)).view(torch.uint32)
    occ = Occupancy(words, pf.DIMS, pf.LO, pf.HI, space=space)
    occ.threshold, occ.dilate = 0.0, 0
    return preview.BakedField(torch.from_numpy(rows), pf.DIMS, pf.LO, pf.HI, degree, occ, 0.0, space=space, far_radius=far_radius)


def test_the_module_refuses_by_kind_and_space_without_a_device():
    from mipnerf_pl_amd import preview, preview_tune360 as pt
    field = _cpu_field()
    world = _cpu_field(space=None, far_radius=None)
    o, d, tn, tf_ = [torch.from_numpy(a) for a in pf.scene_rays()]
    with pytest.raises(ValueError, match=r"world coordinates.*preview\.march_grad"):
        pt.march_grad(world, o, d, tn, tf_, WHITE, grad_rgb=torch.zeros(pf.N_RAYS, 3))
    with pytest.raises(ValueError, match=r"world coordinates.*preview\.TuneState"):
        pt.TuneState360(world)
    with pytest.raises(ValueError, match="world coordinates"):
        pt.tune_field(world, lambda k: None, 1)
    with pytest.raises(ValueError, match="world coordinates"):
        pt.reoccupy(world, 0.5)
    pyr = object.__new__(preview.BakedPyramid)                    # (a contracted pyramid cannot be built: its kind alone is what is refused)
    for call in (lambda: pt.TuneState360(pyr), lambda: pt.march_grad(pyr, o, d, tn, tf_, WHITE, grad_rgb=torch.zeros(pf.N_RAYS, 3))):
        with pytest.raises(NotImplementedError, match="BakedPyramid is not a tuning target"):
            call()
    sparse = object.__new__(preview.SparseField)
    for call in (lambda: pt.TuneState360(sparse), lambda: pt.march_grad(sparse, o, d, tn, tf_, WHITE, grad_rgb=torch.zeros(pf.N_RAYS, 3)),
                 lambda: pt.tune_field(sparse, lambda k: None, 1)):
        with pytest.raises(NotImplementedError, match="SparseField is not a tuning target"):
            call()
    with pytest.raises(TypeError):
        pt.TuneState360(object())
    with pytest.raises(ValueError, match="exactly one of grad_rgb and target"):
        pt.march_grad(field, o, d, tn, tf_, WHITE)
    with pytest.raises(ValueError, match="exactly one of grad_rgb and target"):
        pt.march_grad(field, o, d, tn, tf_, WHITE, grad_rgb=torch.zeros(pf.N_RAYS, 3), target=torch.zeros(pf.N_RAYS, 3), loss_scale=1.0)
    with pytest.raises(ValueError, match="target needs loss_scale"):
        pt.march_grad(field, o, d, tn, tf_, WHITE, target=torch.zeros(pf.N_RAYS, 3))
    with pytest.raises(ValueError, match="grad_rows must be a contiguous fp32 tensor"):
        pt.march_grad(field, o, d, tn, tf_, WHITE, grad_rgb=torch.zeros(pf.N_RAYS, 3), grad_rows=torch.zeros(10, 9, 8, 4))
    with pytest.raises(ValueError, match="at least one step"):
        pt.tune_field(field, lambda k: None, 0)
    with pytest.raises(ValueError, match="finite and >= 0"):
        pt.reoccupy(field, -1.0)
    # the state: TuneState's fields, mask and weights; its optimiser and regulariser are preview's own functions
    state = pt.TuneState360(field, tv_sigma=1e-3)
    assert isinstance(state, preview.TuneState) and state.master.dtype == torch.float32 and torch.equal(state.master.to(torch.float16), field.rows)
    assert torch.equal(state.mask.bool(), preview.baked_points(field.occupancy)) and state.steps == 0 and state.regularised
    assert (state.lr_sigma, state.lr_colour, state.betas, state.eps) == (0.2, 0.01, (0.9, 0.999), 1e-8)
    other = pt.TuneState360(field, lr_sigma=0.5)
    saved = state.state_dict()
    saved["steps"], saved["m"] = 7, torch.ones_like(state.m)
    other.load_state_dict(saved)
    assert other.steps == 7 and other.lr_sigma == 0.2 and other.tv_sigma == 1e-3 and bool((other.m == 1).all())
    assert "tune_adam" not in vars(pt) and "tune_regularise" not in vars(pt)


def test_preview_still_refuses_a_contracted_lattice_and_names_the_new_module(tmp_path):
    from mipnerf_pl_amd import preview
    field = _cpu_field()
    o, d, tn, tf_ = [torch.from_numpy(a) for a in pf.scene_rays()]
    for call in (lambda: preview.march_grad(field, o, d, tn, tf_, WHITE, grad_rgb=torch.zeros(pf.N_RAYS, 3)), lambda: preview.TuneState(field),
                 lambda: preview.tune_field(field, lambda k: None, 1)):
        with pytest.raises(NotImplementedError, match=r"contracted.*mipnerf_pl_amd\.preview_tune360"):
            call()
    with pytest.raises(SystemExit, match=r"--tune.*python -m mipnerf_pl_amd\.preview_tune360"):
        preview.main(["--ckpt", str(tmp_path / "no_such.ckpt"), "--out_dir", str(tmp_path / "o"), "--space", "contracted", "--data", "d",
                      "--tune", "3"])
    assert not os.path.exists(str(tmp_path / "o"))


def test_the_command_refuses_before_any_file_is_opened_and_after_the_keys(tmp_path):
    from mipnerf_pl_amd import preview_tune360 as pt
    missing = str(tmp_path / "no_such.ckpt")               # never opened: the refusal comes first
    out = str(tmp_path / "o")
    base = ["--ckpt", missing, "--out_dir", out, "--data", str(tmp_path)]
    nofile = str(tmp_path / "no_such.npz")
    for extra, why in ((["--steps", "0"], "--steps 0: at least one step"), (["--steps", "-2"], "at least one step"),
                       (["--steps", "3", "--tv_sigma", "-1"], "--tv_sigma"), (["--steps", "3", "--tv_colour", "nan"], "--tv_colour"),
                       (["--steps", "3", "--sh_decay", "inf"], "--sh_decay"), (["--steps", "3", "--lr_sigma", "-0.1"], "--lr_sigma"),
                       (["--steps", "3", "--tv_eps", "0"], "--tv_eps"), (["--steps", "3", "--batch", "0"], "--batch 0"),
                       (["--steps", "3", "--reoccupy", "-0.5"], "--reoccupy"),
                       (["--steps", "3", "--baked", nofile, "--grid", "64"], "--baked .*--grid"),
                       (["--steps", "3", "--baked", nofile, "--threshold", "0.1"], "--baked .*--threshold"),
                       (["--steps", "3", "--baked", nofile, "--far_radius", "9"], "--baked .*--far_radius"),
                       (["--steps", "3", "--far_radius", "1"], "finite and > 1"), (["--steps", "3", "--bound", "3"], "ends at 2"),
                       (["--steps", "3", "--sh_degree", "3"], "--sh_degree 3"), (["--steps", "3", "--grid", "1"], "--grid 1")):
        with pytest.raises(SystemExit, match=why):
            pt.main(base + extra)
    with pytest.raises(SystemExit, match="give --data"):
        pt.main(["--ckpt", missing, "--out_dir", out, "--steps", "3"])
    for ok in (["--steps", "3"], ["--steps", "3", "--target", "mlp", "--tv_sigma", "1e-3", "--reoccupy", "0.5", "--sparse", "--compare"]):
        with pytest.raises(FileNotFoundError):             # nothing to refuse: on to the (missing) checkpoint
            pt.main(base + ok)
    # after the keys are read: a --baked file that is not a contracted dense single lattice
    world = _cpu_field(space=None, far_radius=None).save(str(tmp_path / "world.npz"))
    with pytest.raises(SystemExit, match="world coordinates.*preview --tune"):
        pt.main(base + ["--steps", "3", "--baked", world])
    from mipnerf_pl_amd import preview
    field = _cpu_field()
    with np.load(field.save(str(tmp_path / "dense.npz"))) as z:
        arrays = {k: z[k] for k in z.files}
    arrays["sparse_rows"] = arrays.pop("rows")             # the key a sparse file is told by
    np.savez(str(tmp_path / "sparse.npz"), **arrays)
    assert preview.BakedPyramid.stored_sparse(str(tmp_path / "sparse.npz"))
    with pytest.raises(SystemExit, match="sparse rows are not a tuning target"):
        pt.main(base + ["--steps", "3", "--baked", str(tmp_path / "sparse.npz")])
    with pytest.raises(FileNotFoundError):                 # a contracted dense file passes: on to the (missing) checkpoint
        pt.main(base + ["--steps", "3", "--baked", str(tmp_path / "dense.npz")])
    # and a bounded checkpoint
    system = lambda name, unbounded: SimpleNamespace(hparams={"dataset_name": name}, mip_nerf=SimpleNamespace(unbounded=unbounded, num_levels=2))
    with pytest.raises(SystemExit, match="bounded model.*preview --tune"):
        pt.refuse_checkpoint(system("blender", False))
    with pytest.raises(SystemExit, match="bounded model"):
        pt.refuse_checkpoint(system("llff", False))
    pt.refuse_checkpoint(system("realdata360", True))
    pt.refuse_checkpoint(system("llff", True))
    assert not os.path.exists(out)
    text = re.sub(r"\s+", " ", pt.build_parser().format_help())
    for flag in ("--ckpt", "--data", "--out_dir", "--steps N", "--baked FILE", "--grid", "--sh_degree", "--bound", "--threshold T", "--dilate",
                 "--far_radius R", "--precision", "--batch", "--lr_sigma", "--lr_colour", "--target {photos,mlp}", "--seed", "--tv_sigma X",
                 "--tv_colour X", "--sh_decay X", "--tv_eps X", "--reoccupy T", "--sparse", "--factor", "--compare"):
        assert flag in text, flag


# ---- the convergence recipe, on the reference alone ----------------------------------------------------------------------------------------
def test_the_reference_converges_on_the_recipe(rays):
    """degree 1, teacher = the scene, t_min 1e-3, step 0.5, white background, target = the teacher's march; student = `student_rows`; the full
    batch of non-fragile rays, lr_sigma 0.2, lr_colour 0.02, float64 gradients, float32 Adam, rows re-rounded to fp16 every step.  The
    end / start ratio of the mean squared error after 40 steps is preview_tune360_fixture.CONVERGENCE_RATIO; the GPU test allows 10 x it."""
    teacher = tf.scene_rows(1)
    want = pf.march(teacher, pf.LO, pf.HI, 1, R, *rays, 0.5, 1e-3, 4096, WHITE)
    ok = np.flatnonzero(~want[4])
    target = want[0].astype(F)
    rows = tf.student_rows(teacher, 1)
    shape = rows.shape
    rows = rows.reshape(-1, 16)
    master = rows.astype(F)
    m, v = np.zeros_like(master), np.zeros_like(master)
    losses = []
    for k in range(41):
        out = tf.march_grad(rows.reshape(shape), pf.LO, pf.HI, 1, R, *rays, 0.5, 1e-3, 4096, WHITE, target=target,
                            loss_scale=2.0 / (3 * len(ok)), rays=ok)
        losses.append(float(((out["rgb"][ok] - target[ok]) ** 2).mean()))
        if k < 40:
            c1, c2 = tf.bias_corrections(0.9, 0.999, k + 1)
            tf.adam(master, m, v, out["grad"].astype(F).reshape(-1, 16), rows, None, 1, 0.2, 0.02, 0.9, 0.999, 1e-8, c1, c2)
    ratio = losses[-1] / losses[0]
    print(f"loss {losses[0]:.3e} -> {losses[-1]:.3e} (ratio {ratio:.4f})")
    assert 0.8 * tf.CONVERGENCE_RATIO <= ratio <= tf.CONVERGENCE_RATIO
