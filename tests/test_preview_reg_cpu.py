"""CPU (no GPU): the regulariser of the baked lattice's tuning -- the eighth library's declarations, bindings, exports and argument checks
without a device; the numpy restatement of rules R1 - R4 (tests/preview_reg_fixture.py) against central differences of its own float64
value; the rules of csrc/preview_reg.hpp (g++ -O2 -ffp-contract=off from tests/hostmath/preview_reg.cpp) against the float32 restatement
bit for bit; the Python layer, the command's parser and refusals; the recorded numbers of the end-to-end recipe.

THE TOLERANCE OF THE CENTRAL DIFFERENCES.  The value is a sum of w sqrt(q + eps) with eps = 1e-4 and differences of size 1 - 50; with a
step h = 1e-4 the truncation error of a central difference is h^2 / 6 times the third derivative, at most ~ w h^2 / eps^1.5 / 6 ~ 2e-3 w
where a norm is as small as sqrt(eps) (there are none that small on random rows: the smallest norm is ~ 0.1, which gives 2e-6 w), and the
rounding error of the quotient is ~ 1e-16 x value / h ~ 1e-9.  The bound is 1e-5 x (w_sigma + w_colour + w_view): five times the first."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import preview_fixture as pf
import preview_reg_fixture as rf
import preview_tune_fixture as tf
from mipnerf_pl_amd import _lib as L

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
CSRC = os.path.join(REPO, "mipnerf_pl_amd", "csrc")
F = np.float32


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.PREVIEW_REG_LIB_PATH):
        from mipnerf_pl_amd import build
        build.build(verbose=False)
    return L.preview_reg_lib()


def host():
    src, so = os.path.join(HERE, "hostmath", "preview_reg.cpp"), os.path.join(HERE, "hostmath", "_preview_reg.so")
    hdrs = [os.path.join(CSRC, h) for h in ("raymath.hpp", "lattice_sample.hpp", "preview_march.hpp", "preview_reg.hpp")]
    if (not os.path.exists(so)) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in [src] + hdrs):
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", src, "-o", so])
    return C.CDLL(so)


@pytest.fixture(scope="module")
def hm():
    return host()


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def host_grad(hm, master, mask, dims, degree, scale, grad, w_sigma, w_colour, w_view, eps):
    """`grad` plus the regulariser's gradient by the sequential loop over the rules of preview_reg.hpp, as a new array"""
    out = np.ascontiguousarray(grad, F).copy()
    hm.hm_preview_reg_grad(*dims, degree, _p(np.ascontiguousarray(scale, F)), _p(np.ascontiguousarray(master, F)),
                           _p(None if mask is None else np.ascontiguousarray(mask, np.uint8)), _p(out),
                           *[C.c_float(x) for x in (w_sigma, w_colour, w_view, eps)])
    return out


def same_bits(a, b):
    """equal bit for bit, except that a NaN only has to be a NaN (which sign an operation leaves on one differs between compilers)"""
    nan = np.isnan(b)
    return a.dtype == b.dtype == F and a.shape == b.shape and np.array_equal(np.isnan(a), nan) and \
        np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan])


def masks_of(dims, degree):
    """the masks of the byte-for-byte cases: none, one with holes from `occupancy_of` on the 8 x 9 x 10 lattice (a random one on the
    others, which have no hollow scene), a single point"""
    if tuple(dims) == tuple(pf.DIMS):
        holes = rf.point_mask(tf.occupancy_of(tf.scene_rows(degree, hollow=True)), dims)
        assert 0 < int(holes.sum()) < holes.size
    else:
        holes = rf.random_mask(dims)
    single = np.zeros(holes.shape, np.uint8)
    single[min(1, dims[2] - 1), 1, dims[0] // 2] = 1
    return dict(none=None, holes=holes, single=single)


def grad_before(shape, degree, seed=1):
    """a gradient buffer with random used entries and a sentinel in the pad entries"""
    g = np.random.default_rng(seed).normal(size=shape).astype(F)
    g[..., rf.USED[degree]:] = F(-555.0)
    return g


# ---- the eighth library: declarations, bindings, exports ----------------------------------------------------------------------------
NAMES = ["mipnerf_preview_reg_abi_version", "mipnerf_preview_reg_grad", "mipnerf_preview_reg_last_error"]


def _header(name="mipnerf_preview_reg.h"):
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", name)).read(), flags=re.S)


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return sorted(line.split()[-1] for line in out.splitlines() if line.strip())


def test_header_bindings_and_dynamic_symbols_are_one_set(lib):
    declared = sorted(set(re.findall(r"\b(mipnerf_[a-z0-9_]+)\s*\(", _header())))
    assert declared == sorted(L.PREVIEW_REG_SIGNATURES) == NAMES
    assert _exports(L.PREVIEW_REG_LIB_PATH) == declared
    for name, (_, args) in L.PREVIEW_REG_SIGNATURES.items():
        proto = re.search(r"\b" + name + r"\s*\(([^)]*)\)", _header()).group(1).strip()
        count = 0 if proto in ("", "void") else proto.count(",") + 1
        assert count == len(args), (name, proto)
    assert lib.mipnerf_preview_reg_abi_version() == 1 == L.PREVIEW_REG_ABI


def test_the_other_seven_libraries_keep_their_tables(lib):
    others = dict(hip=L.SIGNATURES, diag=L.DIAG_SIGNATURES, preview=L.PREVIEW_SIGNATURES, mip=L.PREVIEW_MIP_SIGNATURES,
                  sparse=L.PREVIEW_SPARSE_SIGNATURES, tune=L.PREVIEW_TUNE_SIGNATURES, p360=L.PREVIEW_360_SIGNATURES)
    assert [len(t) for t in others.values()] == [93, 3, 4, 3, 7, 4, 4]
    for table in others.values():
        assert not set(table) & set(L.PREVIEW_REG_SIGNATURES) and not any("preview_reg" in n for n in table)
    for path, table in ((L.PREVIEW_LIB_PATH, L.PREVIEW_SIGNATURES), (L.PREVIEW_MIP_LIB_PATH, L.PREVIEW_MIP_SIGNATURES),
                        (L.PREVIEW_SPARSE_LIB_PATH, L.PREVIEW_SPARSE_SIGNATURES), (L.PREVIEW_TUNE_LIB_PATH, L.PREVIEW_TUNE_SIGNATURES),
                        (L.PREVIEW_360_LIB_PATH, L.PREVIEW_360_SIGNATURES)):
        assert _exports(path) == sorted(table)
    assert (L.PREVIEW_ABI, L.PREVIEW_MIP_ABI, L.PREVIEW_SPARSE_ABI, L.PREVIEW_TUNE_ABI, L.PREVIEW_360_ABI) == (1, 1, 1, 1, 1)
    for hdr in sorted(os.listdir(os.path.join(REPO, "include"))):
        if hdr != "mipnerf_preview_reg.h":
            assert "preview_reg" not in open(os.path.join(REPO, "include", hdr)).read(), hdr


def test_the_build_units_are_compiled_without_contraction_into_an_eighth_library():
    from mipnerf_pl_amd import build as b
    assert [u for u, _ in b.PREVIEW_REG_UNITS] == ["kernels_preview_reg.hip", "preview_reg_capi.hip"]
    assert all("-ffp-contract=off" in flags for _, flags in b.PREVIEW_REG_UNITS)
    assert os.path.basename(b.PREVIEW_REG_LIB) == "libmipnerf_preview_reg.so" == os.path.basename(L.PREVIEW_REG_LIB_PATH)
    rest = b.UNITS + b.DIAG_UNITS + b.PREVIEW_UNITS + b.PREVIEW_MIP_UNITS + b.PREVIEW_SPARSE_UNITS + b.PREVIEW_TUNE_UNITS + b.PREVIEW_360_UNITS
    assert not any("preview_reg" in u for u, _ in rest)
    src = open(os.path.join(REPO, "mipnerf_pl_amd", "build.py")).read()
    assert '"include", "mipnerf_preview_reg.h"' in src and "os.path.exists(PREVIEW_REG_LIB)" in src
    rules = open(os.path.join(CSRC, "preview_reg.hpp")).read()
    assert "MIP_HD" in rules and "sqrtf(((dx * dx + dy * dy) + dz * dz) + eps)" in rules and "atomic" not in rules
    unit = open(os.path.join(CSRC, "kernels_preview_reg.hip")).read()
    assert '#include "preview_reg.hpp"' in unit and re.search(r"__global__[^;{]*\bk_preview_reg_grad\s*\(", unit)
    for call in ("reg_stencil(", "reg_touches(", "reg_add("):
        assert call in unit, call
    assert "sqrtf" not in unit                                                           # the rule is not restated in the kernel
    code = re.sub(r"//[^\n]*", "", unit)
    assert not re.search(r"atomic\w*\s*\(|\basm\b|__shared__", code)                     # a gather: no atomics, no inline assembly, no LDS
    others = [f for f in os.listdir(CSRC) if f.endswith((".hip", ".hpp"))
              and re.search(r"__global__[^;{]*\bk_preview_reg_\w+\s*\(", open(os.path.join(CSRC, f)).read())]
    assert others == ["kernels_preview_reg.hip"]
    capi = open(os.path.join(CSRC, "preview_reg_capi.hip")).read()
    assert "preview_dims_ok(" in capi                                                    # the lattice rule of every preview entry point, by call
    assert not re.search(r"hipMalloc|hipFree|Synchronize|hipMemcpy", capi + unit)


def test_the_entry_point_validates_before_any_hip_call(lib):
    """No device here: a call that reached the HIP runtime would fail with code 3, not with 1 / 2 and a message naming the entry point."""
    P = 0x1000        # never dereferenced: the checks come first

    def grad(dims=(8, 9, 10), degree=1, scale=(1.0, 0.5, 0.25), master=P, mask=None, g=P, w=(0.1, 0.2, 0.3), eps=1e-4):
        return lib.mipnerf_preview_reg_grad(None if dims is None else (C.c_int32 * 3)(*dims), degree,
                                            None if scale is None else (C.c_float * 3)(*scale), master, mask, g, *w, eps, None)

    nan, inf = float("nan"), float("inf")
    bad = [
        (lambda: grad(dims=None), L.E_INVALID), (lambda: grad(scale=None), L.E_INVALID),
        (lambda: grad(degree=3), L.E_UNSUPPORTED), (lambda: grad(degree=-1), L.E_UNSUPPORTED),
        (lambda: grad(dims=(1, 5, 6)), L.E_INVALID), (lambda: grad(dims=(1024, 1024, 1024)), L.E_INVALID),
        (lambda: grad(dims=(-1, 0, 6)), L.E_INVALID),
        (lambda: grad(scale=(1.0, 0.0, 1.0)), L.E_INVALID), (lambda: grad(scale=(1.0, nan, 1.0)), L.E_INVALID),
        (lambda: grad(scale=(inf, 1.0, 1.0)), L.E_INVALID), (lambda: grad(scale=(1.0, 1.0, -0.5)), L.E_INVALID),
        (lambda: grad(w=(-0.1, 0.2, 0.3)), L.E_INVALID), (lambda: grad(w=(0.1, nan, 0.3)), L.E_INVALID),
        (lambda: grad(w=(0.1, 0.2, inf)), L.E_INVALID),
        (lambda: grad(eps=0.0), L.E_INVALID), (lambda: grad(eps=-1e-4), L.E_INVALID), (lambda: grad(eps=nan), L.E_INVALID),
        (lambda: grad(eps=inf), L.E_INVALID),
        (lambda: grad(master=None), L.E_INVALID), (lambda: grad(g=None), L.E_INVALID),
        (lambda: grad(master=0x1008), L.E_INVALID), (lambda: grad(g=0x1004), L.E_INVALID),
        (lambda: grad(w=(0.0, 0.0, 0.0), master=None), L.E_INVALID),          # the checks do not depend on the weights
    ]
    for i, (call, code) in enumerate(bad):
        assert call() == code, i
        assert b"preview_reg_grad" in lib.mipnerf_preview_reg_last_error(), i
    assert grad(w=(0.0, 0.0, 0.0)) == L.OK                                  # nothing to add: no launch (there is no device to launch on)
    assert grad(dims=(0, 9, 10), master=None, g=None) == L.OK               # no points: ok whatever the pointers
    assert grad(dims=(8, 9, 0), master=0x1004, g=0x1004) == L.OK
    with pytest.raises(ValueError, match="x: .*preview_reg"):
        L.preview_reg_check(L.E_INVALID, "x")
    with pytest.raises(NotImplementedError):
        L.preview_reg_check(L.E_UNSUPPORTED, "x")


# ---- the fixture against central differences of its own float64 value ------------------------------------------------------------------
@pytest.mark.parametrize("degree", [0, 1, 2])
def test_float64_gradient_against_central_differences_of_the_float64_value(degree):
    dims, lo, hi = rf.LATTICES[0]
    scale = rf.axis_scale(dims, lo, hi)
    assert scale.max() == 1.0 and scale.min() < 0.6                       # the non-cubic box: r_a != 1 on two axes
    master = rf.master_rows(dims, degree).astype(np.float64)
    for name, mask in masks_of(dims, degree).items():
        zero = np.zeros(master.shape)
        g = rf.gradient(master, mask, degree, scale, zero, *rf.WEIGHTS, rf.EPS)
        on = np.ones(master.shape[:3], bool) if mask is None else mask != 0
        assert not g[~on].any() and not g[..., rf.USED[degree]:].any()
        rng = np.random.default_rng(9 + degree)
        points = np.argwhere(on)
        picks = [(tuple(points[rng.integers(len(points))]), int(rng.integers(rf.USED[degree]))) for _ in range(24)]
        picks += [(tuple(points[0]), 0), (tuple(points[-1]), rf.USED[degree] - 1)]
        worst = 0.0
        for (k, j, i), e in picks:
            h = 1e-4
            up, down = master.copy(), master.copy()
            up[k, j, i, e] += h
            down[k, j, i, e] -= h
            fd = (rf.value(up, mask, degree, scale, *rf.WEIGHTS, rf.EPS) - rf.value(down, mask, degree, scale, *rf.WEIGHTS, rf.EPS)) / (2 * h)
            worst = max(worst, abs(fd - g[k, j, i, e]))
            assert abs(fd - g[k, j, i, e]) <= 1e-5 * sum(rf.WEIGHTS), (degree, name, (k, j, i, e), fd, g[k, j, i, e])
        print(f"degree {degree} mask {name}: {len(picks)} entries, worst |fd - g| = {worst:.2e}")
    # an unmasked point moves nothing, as a value or as a neighbour
    mask = masks_of(dims, degree)["holes"]
    off = tuple(np.argwhere(mask == 0)[0])
    moved = master.copy()
    moved[off] += 3.0
    assert rf.value(moved, mask, degree, scale, *rf.WEIGHTS, rf.EPS) == rf.value(master, mask, degree, scale, *rf.WEIGHTS, rf.EPS)


# ---- the host build of preview_reg.hpp ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("degree", [0, 1, 2])
def test_host_build_is_the_float32_restatement_bit_for_bit(hm, degree):
    for dims, lo, hi in rf.LATTICES:
        scale = rf.axis_scale(dims, lo, hi)
        master = rf.master_rows(dims, degree)
        before = grad_before(master.shape, degree)
        for name, mask in masks_of(dims, degree).items():
            for w in (rf.WEIGHTS, (rf.WEIGHTS[0], 0.0, 0.0), (0.0, rf.WEIGHTS[1], 0.0), (0.0, 0.0, rf.WEIGHTS[2])):
                want = rf.gradient(master, mask, degree, scale, before, *w, rf.EPS, F)
                got = host_grad(hm, master, mask, dims, degree, scale, before, *w, rf.EPS)
                assert want.dtype == F and got.tobytes() == want.tobytes(), (degree, dims, name, w)
                on = np.ones(master.shape[:3], bool) if mask is None else mask != 0
                assert got[~on].tobytes() == before[~on].tobytes() and (got[..., rf.USED[degree]:] == F(-555.0)).all()
                touched = np.zeros(rf.USED[degree], bool)
                touched[0], touched[1:] = w[0] != 0, w[1] != 0
                touched[4:] |= w[2] != 0
                assert got[..., :rf.USED[degree]][..., ~touched].tobytes() == before[..., :rf.USED[degree]][..., ~touched].tobytes()
                if mask is None and touched.any():
                    assert (got[..., :rf.USED[degree]][..., touched] != before[..., :rf.USED[degree]][..., touched]).mean() > 0.9
        err = np.abs(rf.gradient(master, None, degree, scale, before, *rf.WEIGHTS, rf.EPS, F).astype(np.float64) -
                     rf.gradient(master, None, degree, scale, before, *rf.WEIGHTS, rf.EPS)).max()
        assert err < 1e-6                                                  # and float32 is float64 to a few ulp of the entries of size ~1


def nan_case(dims, degree, mask):
    """(master with one NaN entry at a present point well inside, the point (x, y, z), the entry)"""
    on = np.ones((dims[2], dims[1], dims[0]), bool) if mask is None else mask != 0
    inner = [p for p in np.argwhere(on) if all(0 < p[2 - a] < dims[a] - 1 for a in range(3))] or list(np.argwhere(on))
    k, j, i = inner[len(inner) // 2]
    e = min(5, rf.USED[degree] - 1)
    master = rf.master_rows(dims, degree)
    master[k, j, i, e] = F(np.nan)
    return master, (int(i), int(j), int(k)), e


@pytest.mark.parametrize("degree", [0, 1, 2])
def test_a_nan_master_entry_spoils_exactly_its_stencils(hm, degree):
    dims, lo, hi = rf.LATTICES[0]
    scale = rf.axis_scale(dims, lo, hi)
    for name, mask in masks_of(dims, degree).items():
        master, q, e = nan_case(dims, degree, mask)
        on = np.ones(master.shape[:3], bool) if mask is None else mask != 0
        zero = np.zeros(master.shape, F)
        got = host_grad(hm, master, mask, dims, degree, scale, zero, *rf.WEIGHTS, rf.EPS)
        assert same_bits(got, rf.gradient(master, mask, degree, scale, zero, *rf.WEIGHTS, rf.EPS, F))
        spoiled = {(int(i), int(j), int(k), int(en)) for k, j, i, en in np.argwhere(np.isnan(got))}
        assert spoiled == {p + (e,) for p in rf.stencil_points(q, dims, on, e >= 4)} and len(spoiled) <= 13, (degree, name)
        if mask is None:
            assert len(spoiled) == 13
        # a term whose weight is 0 is not formed
        w = (0.0, rf.WEIGHTS[1], 0.0) if e == 0 else (rf.WEIGHTS[0], 0.0, 0.0)
        assert not np.isnan(host_grad(hm, master, mask, dims, degree, scale, zero, *w, rf.EPS)).any()


# ---- python layer without a device -----------------------------------------------------------------------------------------------------
def _dense():
    import test_preview_sparse_cpu as sparse_cpu
    return sparse_cpu._sparse((8, 9, 10))[0].to_dense()


def test_tune_state_carries_the_weights_and_zero_weights_never_load_the_library(monkeypatch):
    from mipnerf_pl_amd import preview
    from mipnerf_pl_amd.rays import Rays
    dense = _dense()
    calls = []
    monkeypatch.setattr(preview, "march_grad", lambda baked, *a, **k: calls.append("march_grad") or (k["grad_rows"], torch.zeros(4, 3), None))
    monkeypatch.setattr(preview, "tune_adam", lambda *a, **k: calls.append("tune_adam"))

    def no_library():
        raise AssertionError("libmipnerf_preview_reg.so must not be loaded")
    monkeypatch.setattr(L, "preview_reg_lib", no_library)
    z = torch.zeros(4, 3)
    rays = Rays(z, z, z, z[:, :1], z[:, :1], z[:, :1], z[:, :1])
    state = preview.TuneState(dense)
    assert (state.tv_sigma, state.tv_colour, state.sh_decay, state.tv_eps) == (0.0, 0.0, 0.0, preview.DEFAULT_TUNE_TV_EPS) and not state.regularised
    state.step(rays, z, True)
    assert calls == ["march_grad", "tune_adam"] and state._n_points is None      # (the loader raises here: it was not called)
    # with a weight the regulariser runs between the two, with the masked points counted once
    seen = []
    monkeypatch.setattr(preview, "tune_regularise", lambda *a: calls.append("tune_regularise") or seen.append(a))
    for kw in (dict(tv_sigma=0.5), dict(tv_colour=0.25), dict(sh_decay=0.125)):
        del calls[:], seen[:]
        state = preview.TuneState(dense, tv_eps=1e-3, **kw)
        assert state.regularised
        state.step(rays, z, True)
        state.step(rays, z, True)
        assert calls == ["march_grad", "tune_regularise", "tune_adam"] * 2
        master, mask, dims, lo, hi, degree, grad, tv_sigma, tv_colour, sh_decay, tv_eps, n_points = seen[0]
        assert master is state.master and mask is state.mask and grad is state.grad and (dims, lo, hi, degree) == (dense.dims, dense.lo, dense.hi, 1)
        assert dict(tv_sigma=tv_sigma, tv_colour=tv_colour, sh_decay=sh_decay) == dict(dict(tv_sigma=0.0, tv_colour=0.0, sh_decay=0.0), **kw)
        assert tv_eps == 1e-3 and n_points == int(state.mask.sum()) == state.n_points and 0 < n_points < 720
    for kw in (dict(tv_sigma=-1.0), dict(tv_colour=float("nan")), dict(sh_decay=float("inf")), dict(tv_eps=0.0), dict(tv_eps=-1.0)):
        with pytest.raises(ValueError, match="tv_sigma, tv_colour and sh_decay"):
            preview.TuneState(dense, **kw)
    # kwargs reach the state through tune_field
    state, _ = preview.tune_field(dense, lambda k: (rays, z), 1, tv_colour=0.75)
    assert state.tv_colour == 0.75 and state.steps == 1


def test_state_dict_round_trip_with_and_without_the_new_keys():
    from mipnerf_pl_amd import preview
    dense = _dense()
    state = preview.TuneState(dense, tv_sigma=0.5, tv_colour=0.25, sh_decay=0.125, tv_eps=1e-3)
    saved = state.state_dict()
    assert {k: saved[k] for k in ("tv_sigma", "tv_colour", "sh_decay", "tv_eps")} == dict(tv_sigma=0.5, tv_colour=0.25, sh_decay=0.125, tv_eps=1e-3)
    other = preview.TuneState(dense)
    other.load_state_dict(saved)
    assert (other.tv_sigma, other.tv_colour, other.sh_decay, other.tv_eps) == (0.5, 0.25, 0.125, 1e-3) and other.regularised
    old = {k: v for k, v in saved.items() if k not in ("tv_sigma", "tv_colour", "sh_decay", "tv_eps")}
    assert sorted(old) == sorted(["master", "m", "v", "steps", "lr_sigma", "lr_colour", "betas", "eps"])      # what the state held before
    old["steps"] = 3
    plain = preview.TuneState(dense)
    plain.load_state_dict(old)
    assert plain.steps == 3 and not plain.regularised and plain.tv_eps == preview.DEFAULT_TUNE_TV_EPS
    kept = preview.TuneState(dense, sh_decay=0.5)
    kept.load_state_dict(old)                                              # a dict without the keys says nothing about them
    assert kept.sh_decay == 0.5 and kept.steps == 3


def test_the_binding_checks_its_tensors_before_the_library(monkeypatch):
    from mipnerf_pl_amd import preview
    monkeypatch.setattr(L, "preview_reg_lib", lambda: (_ for _ in ()).throw(AssertionError("not reached")))
    master, grad = torch.zeros(10, 9, 8, 16), torch.zeros(10, 9, 8, 16)
    mask = torch.ones(10, 9, 8, dtype=torch.uint8)
    args = ((8, 9, 10), pf.LO, pf.HI, 1, grad, 0.1, 0.1, 0.1, 1e-4)
    with pytest.raises(ValueError, match="master must be a contiguous fp32 tensor"):
        preview.tune_regularise(master.double(), None, *args)
    with pytest.raises(ValueError, match="grad must be a contiguous fp32 tensor"):
        preview.tune_regularise(master, None, (8, 9, 10), pf.LO, pf.HI, 1, torch.zeros(10, 9, 8, 4), 0.1, 0.1, 0.1, 1e-4)
    with pytest.raises(ValueError, match="one contiguous uint8 mask byte per point"):
        preview.tune_regularise(master, mask.bool(), *args, 5)
    with pytest.raises(ValueError, match="n_points .* must be given"):
        preview.tune_regularise(master, mask, *args)
    with pytest.raises(ValueError, match="weights must be finite"):
        preview.tune_regularise(master, None, (8, 9, 10), pf.LO, pf.HI, 1, grad, -0.1, 0.1, 0.1, 1e-4)
    with pytest.raises(NotImplementedError):
        preview.tune_regularise(master, None, (8, 9, 10), pf.LO, pf.HI, 3, grad, 0.1, 0.1, 0.1, 1e-4)
    assert preview.lattice_axis_scale((8, 9, 10), pf.LO, pf.HI).tobytes() == rf.axis_scale((8, 9, 10), pf.LO, pf.HI).tobytes()
    assert preview.lattice_axis_scale((16, 16, 16), (-1.0,) * 3, (1.0,) * 3).tolist() == [1.0, 1.0, 1.0]      # a cubic lattice


# ---- command line ------------------------------------------------------------------------------------------------------------------------
REG_FLAGS = ("tune_tv_sigma", "tune_tv_colour", "tune_sh_decay", "tune_tv_eps")


def test_parser_defaults_and_help():
    from mipnerf_pl_amd import preview
    p = preview.build_parser()
    a = p.parse_args(["--out_dir", "o", "--tune", "5"])
    assert all(f in preview.TUNE_FLAGS and getattr(a, f) is None for f in REG_FLAGS)
    assert preview.TUNE_FLAGS[:5] == ("tune_batch", "tune_lr_sigma", "tune_lr_colour", "tune_target", "tune_seed")
    a = p.parse_args(["--out_dir", "o", "--tune", "5", "--tune_tv_sigma", "0.5", "--tune_tv_colour", "0.25", "--tune_sh_decay", "0.125",
                      "--tune_tv_eps", "1e-3"])
    assert (a.tune_tv_sigma, a.tune_tv_colour, a.tune_sh_decay, a.tune_tv_eps) == (0.5, 0.25, 0.125, 1e-3)
    text = re.sub(r"\s+", " ", p.format_help())
    for flag in REG_FLAGS:
        assert "--" + flag + " X" in text, flag
    assert text.count("a choice, not a measurement") >= 6 and text.count("default 0: off") == 3
    assert preview.DEFAULT_TUNE_TV_EPS == 1e-4
    from mipnerf_pl_amd import eval as eval_cli
    from mipnerf_pl_amd import render_video
    for parser in (eval_cli.build_parser(), render_video.build_parser()):
        assert "--tune_tv" not in parser.format_help()


def test_refusals_come_before_the_checkpoint_is_opened(tmp_path):
    from mipnerf_pl_amd import preview
    missing = str(tmp_path / "no_such.ckpt")               # never opened: the refusal comes first
    out = str(tmp_path / "o")
    base = ["--ckpt", missing, "--out_dir", out]
    for flag in REG_FLAGS:
        with pytest.raises(SystemExit, match=f"--{flag} belongs to --tune"):
            preview.main(base + ["--" + flag, "0.1"])
    for extra, why in ((["--tune_tv_sigma", "-0.1"], "--tune_tv_sigma -0.1: must be finite and >= 0"),
                       (["--tune_tv_colour", "nan"], "--tune_tv_colour nan"), (["--tune_sh_decay", "inf"], "--tune_sh_decay inf"),
                       (["--tune_tv_eps", "0"], "--tune_tv_eps 0.0: must be finite and > 0"), (["--tune_tv_eps", "-1"], "--tune_tv_eps"),
                       (["--tune_tv_eps", "nan"], "--tune_tv_eps")):
        with pytest.raises(SystemExit, match=why):
            preview.main(base + ["--tune", "3"] + extra)
    for ok in (["--tune", "3", "--tune_tv_sigma", "0"], ["--tune", "3", "--tune_tv_sigma", "0.1", "--tune_tv_colour", "0.1", "--tune_sh_decay",
                                                           "0.01", "--tune_tv_eps", "1e-5", "--sparse"]):
        with pytest.raises(FileNotFoundError):             # nothing to refuse: on to the (missing) checkpoint
            preview.main(base + ok)
    assert not os.path.exists(out)


# ---- the end-to-end recipe, on the fixtures alone ----------------------------------------------------------------------------------------
def test_the_recorded_numbers_of_the_recipe_are_what_the_fixtures_give():
    """The yardstick of test_gpu_preview_reg.py's end-to-end test: 40 steps of the tune tests' student / teacher recipe with and without
    the regulariser (weights 2e-4 / 2e-4 / 5e-5 per point), float64 march gradients, float32 regulariser gradient and Adam.  Measured: the
    batch loss goes 1.518e-3 -> 7.17e-6 without and -> 1.86e-5 with it; the final total variation (sigma, colour) is (4195, 9061) without
    and (703, 4470) with it."""
    for reg in (False, True):
        losses, tv = rf.recipe(reg)
        want = rf.RECORDED[reg]
        print(f"regularised {reg}: loss {losses[0]:.4e} -> {losses[-1]:.4e}, tv sigma {tv[0]:.4e} colour {tv[1]:.4e}")
        assert abs(losses[0] - want["loss0"]) <= 1e-3 * want["loss0"] and abs(losses[-1] - want["loss"]) <= 1e-3 * want["loss"]
        assert all(abs(a - b) <= 1e-3 * b for a, b in zip(tv, want["tv"]))
    assert rf.RECORDED[True]["loss"] < 0.05 * rf.RECORDED[True]["loss0"]                       # the loss still falls
    assert all(a < 0.5 * b for a, b in zip(rf.RECORDED[True]["tv"], rf.RECORDED[False]["tv"]))  # and the total variation is less than half
