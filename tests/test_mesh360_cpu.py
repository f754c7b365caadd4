"""CPU (no GPU): the lattice and mesh of the unbounded-scene model -- the new C entry points' bindings and argument checks, the command
line's --space / --far_radius and default boxes, and the un-contraction math of csrc/raymath360.hpp (the source the gfx950 kernel
inlines, built with g++ -ffp-contract=off) against float64 numpy.

Bounds of the un-contraction (include/mipnerf_hip.h states the fp32 rules), r = 1 / (2 - min(|z|, c)) the world radius:
  positions  |x - x64| <= 1e-6 * max(r, 1) * |x64|: n = |z| carries at most about 3 ulp, dn <= 3.6e-7; 2 - n is exact, so the scale r / n
             has the relative error r * dn plus a few ulp; the bound leaves about 2.5 x on that;
  normals    |n - n64| <= 1e-6 * max(r, 1) + 1e-6 (the tangential part is scaled by 2 r - 1 and inherits the error of u = z / n);
  no result lies beyond far_radius * (1 + 1e-6): r is clamped to far_radius, which matters where c = 2 - 1 / far_radius is rounded up (radii that
             are no power of two: 30) or to 2 (2^25)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostmath", "uncontract.cpp")
SO = os.path.join(HERE, "hostmath", "_uncontract.so")

NEW_ENTRY_POINTS = ("mipnerf_density_grid_360_workspace_bytes", "mipnerf_density_grid_360", "mipnerf_uncontract_vertices")


def uncontract64(z, g, far_radius):
    """float64 numpy: (x, world normals, r).  c is the library's fp32 cap 2 - 1 / far_radius, as a double."""
    z, g = z.astype(np.float64), g.astype(np.float64)
    c = float(np.float32(2) - np.float32(1) / np.float32(far_radius))
    n = np.linalg.norm(z, axis=-1, keepdims=True)
    out = n > 1
    with np.errstate(divide="ignore"):
        r = np.where(out, np.minimum(1.0 / (2.0 - np.minimum(n, c)), float(far_radius)), 1.0)
    nsafe = np.where(out, n, 1.0)
    x = np.where(out, z * (r / nsafe), z)
    u = z / nsafe
    ug = (u * g).sum(-1, keepdims=True)
    w = (2 * r - 1) * (g - ug * u) + ug * u
    wl = np.linalg.norm(w, axis=-1, keepdims=True)
    nw = np.where(out, np.where(wl > 0, w / np.where(wl > 0, wl, 1.0), 0.0), g)
    return x, nw, r[..., 0]


def position_bound(x64, r):
    return 1e-6 * np.maximum(r, 1.0)[:, None] * np.linalg.norm(x64, axis=-1, keepdims=True)


def normal_bound(r):
    return (1e-6 * np.maximum(r, 1.0) + 1e-6)[:, None]


@pytest.fixture(scope="module")
def um():
    hdr = os.path.join(HERE, "..", "mipnerf_pl_amd", "csrc", "raymath360.hpp")
    if (not os.path.exists(SO)) or os.path.getmtime(SO) < max(os.path.getmtime(SRC), os.path.getmtime(hdr)):
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", SRC, "-o", SO])
    return C.CDLL(SO)


def p(a):
    return a.ctypes.data_as(C.c_void_p)


def _norms(rng, far_radius, count):
    """norms over [0, 2.2] plus values within 1e-6 of 1, of c and of 2 (both sides, and the values themselves)"""
    c = float(np.float32(2) - np.float32(1) / np.float32(far_radius))
    near = np.concatenate([v + np.concatenate([[0.0], rng.uniform(-1e-6, 1e-6, 40)]) for v in (1.0, c, 2.0)])
    return np.concatenate([rng.uniform(0.0, 2.2, count), rng.uniform(0.9, 1.1, count // 4), rng.uniform(c - 0.02, 2.0, count // 4), near, [0.0, 1e-20]])


@pytest.mark.parametrize("far_radius", [64.0, 8.0, 4096.0, 30.0, 1000.0, 2.0 ** 25])        # c exact (powers of two), rounded, and rounded to 2
def test_uncontraction_math_against_float64(um, far_radius):
    rng = np.random.default_rng(int(far_radius))
    n = _norms(rng, far_radius, 4000)
    d = rng.normal(size=(n.size, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    z = (d * n[:, None]).astype(np.float32)
    g = rng.normal(size=z.shape)
    g = (g / np.linalg.norm(g, axis=1, keepdims=True)).astype(np.float32)
    g[1::53] = (z[1::53] / np.maximum(np.linalg.norm(z[1::53], axis=1, keepdims=True), 1e-30)).astype(np.float32)     # purely radial
    g[::97] = 0                                                  # (0, 0, 0) stays (0, 0, 0)
    x, nw = np.empty_like(z), np.empty_like(z)
    um.um_uncontract(len(z), C.c_float(far_radius), p(z), p(g), p(x), p(nw))
    x64, n64, r64 = uncontract64(z, g, far_radius)
    zn = np.linalg.norm(z.astype(np.float64), axis=1)
    c = float(np.float32(2) - np.float32(1) / np.float32(far_radius))
    assert (np.abs(zn - 1) < 1e-6).sum() >= 30 and (np.abs(zn - c) < 1e-6).sum() >= 30 and (np.abs(zn - 2) < 1e-6).sum() >= 30
    assert (zn >= c).sum() > 100 and (zn < 1).sum() > 100
    assert np.isfinite(x).all() and np.isfinite(nw).all()
    assert (np.abs(x - x64) <= position_bound(x64, r64)).all(), float((np.abs(x - x64) / np.maximum(position_bound(x64, r64), 1e-300)).max())
    assert (np.abs(nw - n64) <= normal_bound(r64)).all(), float((np.abs(nw - n64) / normal_bound(r64)).max())
    assert np.linalg.norm(x.astype(np.float64), axis=1).max() <= far_radius * (1 + 1e-6)
    assert np.linalg.norm(x.astype(np.float64), axis=1)[zn > c].min() >= far_radius * (1 - 1e-6) - far_radius ** 2 * 2.0 ** -24 or c == 2.0   # the cap is reached (c is off by half an ulp at most)
    # inside the unit ball nothing moves, bit for bit; zero normals stay zero everywhere
    inside = zn <= 1 - 1e-6
    assert np.array_equal(x[inside], z[inside]) and np.array_equal(nw[inside], g[inside])
    assert not nw[::97].any()
    unit = np.linalg.norm(nw.astype(np.float64), axis=1)
    assert (np.abs(unit[g.any(1)] - 1) <= 2e-6).all()
    # and it is the inverse of the contraction the kernels apply (where the cap does not bite): contract(x) = z to fp32 rounding
    back = np.empty_like(z)
    um.um_contract(len(z), p(x), p(back))
    free = zn <= c
    assert np.abs(back[free] - z[free]).max() <= 1e-6


def test_normal_transform_is_the_transposed_jacobian():
    """the well-scaled form of the header against J^T g with J built from finite differences of the contraction, in float64"""
    rng = np.random.default_rng(7)
    z = rng.normal(size=(200, 3))
    z *= (rng.uniform(1.05, 1.9, 200) / np.linalg.norm(z, axis=1))[:, None]
    g = rng.normal(size=z.shape)
    g /= np.linalg.norm(g, axis=1, keepdims=True)
    x, nw, _ = uncontract64(z, g, 64.0)

    def contract(v):
        n = np.linalg.norm(v, axis=-1, keepdims=True)
        return np.where(n > 1, (2 - 1 / n) * v / n, v)
    assert np.abs(contract(x) - z).max() <= 1e-12
    eps = 1e-6
    J = np.stack([(contract(x + eps * e) - contract(x - eps * e)) / (2 * eps) for e in np.eye(3)], -1)      # J[v, i, j] = d z_i / d x_j
    want = np.einsum("vij,vi->vj", J, g)
    want /= np.linalg.norm(want, axis=1, keepdims=True)
    assert np.abs(nw - want).max() <= 1e-7


def test_bindings_and_argument_checks_without_a_gpu():
    import re
    from mipnerf_pl_amd import _lib as L
    for n in NEW_ENTRY_POINTS + ("mipnerf_lattice_ipe_360",):
        assert n in L.SIGNATURES
    header = open(os.path.join(HERE, "..", "include", "mipnerf_hip.h")).read()
    decls = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for n in NEW_ENTRY_POINTS:
        assert re.search(r"\b" + n + r"\s*\(", decls), n
    assert "MIPNERF_SPACE_WORLD = 0" in decls and "MIPNERF_SPACE_CONTRACTED = 1" in decls
    assert (L.SPACE_WORLD, L.SPACE_CONTRACTED) == (0, 1) and L.SPACES == {"world": 0, "contracted": 1}
    if not os.path.exists(L.LIB_PATH):
        from mipnerf_pl_amd import build
        build.build(verbose=False)
    lib = L.lib()
    assert lib.mipnerf_abi_version() == 6                                          # the ABI only grows
    dims, f3 = (C.c_int32 * 3), (C.c_float * 3)
    lo, hi = f3(-2, -2, -2), f3(2, 2, 2)

    def grid(d=(8, 8, 8), lo=lo, hi=hi, cov_scale=1.0, space=L.SPACE_CONTRACTED, far_radius=64.0, precision=L.PREC_FP32):
        # every scalar argument is checked before the context is looked at: no device needed
        rc = lib.mipnerf_density_grid_360(None, dims(*d), lo, hi, cov_scale, space, far_radius, precision, None, None, 0, None)
        return rc, lib.mipnerf_last_error()

    for space in (-1, 2, 7):
        rc, msg = grid(space=space)
        assert rc == L.E_INVALID and b"space" in msg
    for far in (1.0, 0.5, 0.0, -3.0, float("inf"), float("nan")):
        rc, msg = grid(far_radius=far)
        assert rc == L.E_INVALID and b"far_radius" in msg, far
    for cs in (-1.0, float("inf"), float("nan")):
        rc, msg = grid(cov_scale=cs)
        assert rc == L.E_INVALID and b"cov_scale" in msg, cs
    for d in ((1, 8, 8), (8, 8, 0), (675, 675, 675)):
        rc, msg = grid(d=d)
        assert rc == L.E_INVALID and (b"2^31" in msg or b"at least 2 points" in msg), d
    rc, msg = grid(hi=f3(2, float("inf"), 2))
    assert rc == L.E_INVALID and b"not finite" in msg
    rc, msg = grid(precision=5)
    assert rc == L.E_INVALID and b"precision" in msg
    rc, msg = grid()                                                               # all scalars good: now the null context is what is wrong
    assert rc == L.E_INVALID and b"null" in msg
    assert lib.mipnerf_density_grid_360_workspace_bytes(None, 1024, L.PREC_FP32) == 0
    # the encoder alone and the un-contraction check theirs as well
    enc = lambda **kw: lib.mipnerf_lattice_ipe_360(dims(8, 8, 8), lo, hi, kw.get("first", 0), kw.get("count", 512), kw.get("cov_scale", 1.0),
                                                   kw.get("space", 1), 0, kw.get("max_deg", 16), None, kw.get("dtype", L.PREC_FP32), None)
    assert enc(space=3) == L.E_INVALID and enc(cov_scale=-1.0) == L.E_INVALID and enc(count=513) == L.E_INVALID and enc(first=-1) == L.E_INVALID
    assert enc(max_deg=5) == L.E_INVALID and enc(dtype=9) == L.E_INVALID and enc() == L.E_INVALID            # the last one: a null buffer
    for far in (1.0, float("nan"), float("inf")):
        assert lib.mipnerf_uncontract_vertices(4, far, None, None, None, None, None) == L.E_INVALID
        assert b"far_radius" in lib.mipnerf_last_error()
    assert lib.mipnerf_uncontract_vertices(4, 64.0, None, None, None, None, None) == L.E_INVALID               # null points
    assert lib.mipnerf_uncontract_vertices(0, 64.0, None, None, None, None, None) == L.OK                      # nothing to do
    # mipnerf_density_grid itself keeps its contract: a null context is its first complaint
    assert lib.mipnerf_density_grid(None, dims(8, 8, 8), lo, hi, 1.0, L.PREC_FP32, None, None, 0, None) == L.E_INVALID


def test_command_line_space_flags_and_default_boxes():
    from mipnerf_pl_amd import extract_mesh as cli
    from mipnerf_pl_amd.mesh import Mesh, default_box
    p_ = cli.build_parser()
    a = p_.parse_args(["--ckpt", "x.ckpt", "--out_dir", "out"])
    assert (a.space, a.far_radius, a.bound) == (None, 64.0, 1.5)
    assert cli.lattice_of(a) == ((256,) * 3, (-1.5,) * 3, (1.5,) * 3)
    a = p_.parse_args(["--ckpt", "x", "--out_dir", "o", "--space", "contracted", "--grid", "64"])
    assert (a.space, a.far_radius) == ("contracted", 64.0)
    assert cli.lattice_of(a) == ((64,) * 3, (-2.0,) * 3, (2.0,) * 3)                 # the whole contracted space
    a = p_.parse_args(["--ckpt", "x", "--out_dir", "o", "--space", "world", "--far_radius", "30"])
    assert (a.space, a.far_radius) == ("world", 30.0)
    assert cli.lattice_of(a) == ((256,) * 3, (-1.5,) * 3, (1.5,) * 3)
    a = p_.parse_args(["--ckpt", "x", "--out_dir", "o", "--space", "contracted", "--bound", "1.5"])
    assert cli.lattice_of(a) == ((256,) * 3, (-1.5,) * 3, (1.5,) * 3)                # a typed --bound is kept, also when it equals the default
    a = p_.parse_args(["--ckpt", "x", "--out_dir", "o", "--space", "contracted", "--aabb", "-1", "0", "0.5", "1", "2", "1.5"])
    assert cli.lattice_of(a) == ((256,) * 3, (-1.0, 0.0, 0.5), (1.0, 2.0, 1.5))
    with pytest.raises(SystemExit):
        p_.parse_args(["--ckpt", "x", "--out_dir", "o", "--space", "somewhere"])
    assert default_box(None) == default_box("world") == ((-1.5,) * 3, (1.5,) * 3) and default_box("contracted") == ((-2.0,) * 3, (2.0,) * 3)
    assert Mesh._fields[-1] == "vertices_contracted" and Mesh._field_defaults["vertices_contracted"] is None


def test_ops_refusals_without_a_gpu():
    import torch
    from mipnerf_pl_amd import MipNerf, ops
    from mipnerf_pl_amd.mesh import extract_mesh
    unb, bnd = MipNerf(num_samples=8, unbounded=True), MipNerf(num_samples=8)
    box = ((8, 8, 8), (-1,) * 3, (1,) * 3)
    with pytest.raises(NotImplementedError):                                        # as before: an unbounded model and no space
        ops.density_grid(unb, *box)
    with pytest.raises(NotImplementedError):
        extract_mesh(unb, grid=8)
    with pytest.raises(NotImplementedError):
        ops.field_at(unb, torch.zeros(1, 3), torch.zeros(1), torch.zeros(1, 3))
    for space in ("world", "contracted"):                                          # a bounded model and a space
        with pytest.raises(ValueError, match="unbounded=True"):
            ops.density_grid(bnd, *box, space=space)
        with pytest.raises(ValueError, match="unbounded=True"):
            ops.field_at(bnd, torch.zeros(1, 3), torch.zeros(1), torch.zeros(1, 3), space=space)
        with pytest.raises(ValueError, match="unbounded=True"):
            extract_mesh(bnd, grid=8, space=space)
        with pytest.raises(RuntimeError, match="no CPU fallback"):                 # on the host: past the checks, and no further
            ops.density_grid(unb, *box, space=space)
    with pytest.raises(ValueError, match="space must be"):
        ops.density_grid(unb, *box, space="disparity")
    with pytest.raises(RuntimeError):
        ops.uncontract(torch.zeros(4, 3))
