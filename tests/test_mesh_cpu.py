"""CPU (no GPU): the comparator of the isosurface kernels (tests/isosurface_fixture.py) against analytic fields and first principles,
the PLY writer / reader, the extract_mesh command line's parser, and the new C entry points' bindings and argument checks."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

import isosurface_fixture as fx

BOX = ([-1.5] * 3, [1.5] * 3)


# (field, V, F, Euler characteristic, volume relative to the analytic one - 1) on 64^3 over [-1.5, 1.5]^3 at threshold 0
TABLE = [("sphere", fx.sphere_field, fx.SPHERE_VOLUME, 20072, 40140, 2, -0.00210),
         ("torus", fx.torus_field, fx.TORUS_VOLUME, 18760, 37520, 0, -0.00826)]


@pytest.mark.parametrize("name,field,volume,V,F,chi,vol_err", TABLE, ids=[t[0] for t in TABLE])
def test_fixture_on_analytic_fields(name, field, volume, V, F, chi, vol_err):
    m = fx.marching_tets(field(64), 0.0, *BOX)
    v, f = m["vertices"], m["faces"]
    assert (len(v), len(f)) == (V, F)
    assert fx.is_closed(f) and fx.is_oriented(f) and fx.zero_area_faces(v, f) == 0
    assert fx.euler_characteristic(len(v), f) == chi
    assert abs(fx.enclosed_volume(v, f) / volume - 1 - vol_err) <= 1e-4          # the margin covers the summation order, nothing else
    # vertices sorted by (smaller end, larger end); edges are (inside, outside)
    e = m["edges"]
    key = e.min(1) * field(64).size + e.max(1)
    assert (np.diff(key) > 0).all()
    fl = field(64).reshape(-1)
    assert (fl[e[:, 0]] > 0).all() and not (fl[e[:, 1]] > 0).any()


def test_fixture_volume_error_falls_fourfold_per_doubling():
    errs = []
    for n in (16, 32, 64):
        m = fx.marching_tets(fx.sphere_field(n), 0.0, *BOX)
        errs.append(fx.enclosed_volume(m["vertices"], m["faces"]) / fx.SPHERE_VOLUME - 1)
    for got, want in zip(errs, (-0.0368, -0.0086, -0.0021)):
        assert abs(got - want) <= 1e-4
    assert 3.5 < errs[0] / errs[1] < 4.5 and 3.5 < errs[1] / errs[2] < 4.5


def test_fixture_sphere_normals_are_radial():
    """central differences are exact for a quadratic"""
    m = fx.marching_tets(fx.sphere_field(32), 0.0, *BOX)
    r = m["vertices"] - fx.CENTRE
    cos = (r / np.linalg.norm(r, axis=1)[:, None] * m["normals"]).sum(1)
    assert cos.min() >= 1 - 1e-6 and not m["weak"].any()      # the field is float32: 1 - 1e-7 would be its rounding


def test_all_sign_cases_of_all_six_tetrahedra():
    """Every one of the 256 sign patterns of a 2 x 2 x 2 lattice (all 16 cases of each of the six tetrahedra, in every combination):
    the fixture's faces against first principles.  Face count: one triangle per tetrahedron with 1 or 3 corners inside, two with 2.
    Winding: inside a tetrahedron the field's linear interpolant has a constant gradient, and every face's geometric normal must point
    down that gradient.  No directed edge twice."""
    rng = np.random.default_rng(0)
    mag = rng.uniform(0.5, 2.0, 8)
    pos, _ = fx.lattice_positions((2, 2, 2), [0, 0, 0], [1, 1, 1])
    tets = []
    for p in fx.PERMUTATIONS:
        c1 = 1 << p[0]
        tets.append((0, c1, c1 | (1 << p[1]), 7))
    cases = set()
    for pattern in range(256):
        inside = np.array([(pattern >> c) & 1 for c in range(8)], bool)
        f = np.where(inside, mag, -mag).astype(np.float32).reshape(2, 2, 2)        # flat index = corner code dx + 2 dy + 4 dz
        m = fx.marching_tets(f, 0.0, [0, 0, 0], [1, 1, 1])
        want = 0
        for t, tet in enumerate(tets):
            k = int(inside[list(tet)].sum())
            want += (0, 1, 2, 1, 0)[k]
            cases.add((t, sum(int(inside[c]) << i for i, c in enumerate(tet))))
        assert len(m["faces"]) == want, pattern
        assert fx.directed_edges_unique(m["faces"]), pattern
        fl = f.reshape(-1).astype(np.float64)
        for face in m["faces"]:
            corners = sorted(set(m["edges"][face].reshape(-1)))
            assert len(corners) == 4 and tuple(corners) in tets, (pattern, corners)
            A = pos[corners[1:]] - pos[corners[0]]
            g = np.linalg.solve(A, fl[corners[1:]] - fl[corners[0]])
            v = m["vertices"][face]
            n = np.cross(v[1] - v[0], v[2] - v[0])
            assert np.linalg.norm(n) > 0 and n @ g < 0, (pattern, face)
            # ... and the three vertices lie on the zero set of that interpolant
            assert np.abs(fl[corners[0]] + (v - pos[corners[0]]) @ g).max() < 1e-12
    assert len(cases) == 6 * 16


def test_fixture_keeps_collapsed_triangles_and_handles_non_finite_values():
    rng = np.random.default_rng(1)
    f = rng.integers(-2, 3, size=(9, 8, 7)).astype(np.float32)                    # ties with the threshold 0 everywhere
    m = fx.marching_tets(f, 0.0, [-1, -1, -1], [1, 1, 1])
    assert fx.directed_edges_unique(m["faces"]) and fx.zero_area_faces(m["vertices"], m["faces"]) > 0
    g = rng.normal(size=(7, 9, 8)).astype(np.float32)
    g.reshape(-1)[rng.choice(g.size, 60, replace=False)] = np.array([np.nan, np.inf, -np.inf] * 20, np.float32)
    m = fx.marching_tets(g, 0.25, [-1, -1, -1], [1, 1, 1])
    assert np.isfinite(m["vertices"]).all() and np.isfinite(m["normals"]).all() and fx.directed_edges_unique(m["faces"])
    fl = g.reshape(-1)
    assert (fl[m["edges"][:, 0]] > 0.25).all() and not (fl[m["edges"][:, 1]] > 0.25).any()     # NaN is outside
    for const in (-1.0, 1.0):
        m = fx.marching_tets(np.full((4, 5, 6), const, np.float32), 0.0, [-1] * 3, [1] * 3)
        assert len(m["vertices"]) == 0 and len(m["faces"]) == 0


def test_ply_round_trip_and_header(tmp_path):
    from mipnerf_pl_amd.mesh import read_ply, write_ply
    rng = np.random.default_rng(2)
    v = rng.normal(size=(11, 3)).astype(np.float32)
    n = rng.normal(size=(11, 3)).astype(np.float32)
    f = rng.integers(0, 11, size=(7, 3)).astype(np.int32)
    c = rng.integers(0, 256, size=(11, 3)).astype(np.uint8)
    path = write_ply(str(tmp_path / "a.ply"), v, n, f, c)
    head = (b"ply\nformat binary_little_endian 1.0\ncomment mipnerf_pl_amd.mesh\nelement vertex 11\n"
            b"property float x\nproperty float y\nproperty float z\nproperty float nx\nproperty float ny\nproperty float nz\n"
            b"property uchar red\nproperty uchar green\nproperty uchar blue\n"
            b"element face 7\nproperty list uchar int vertex_indices\nend_header\n")
    data = open(path, "rb").read()
    assert data[:len(head)] == head and len(data) == len(head) + 11 * 27 + 7 * 13
    assert data[len(head):len(head) + 12] == v[0].astype("<f4").tobytes() and data[len(head) + 24:len(head) + 27] == c[0].tobytes()
    assert data[len(head) + 11 * 27:len(head) + 11 * 27 + 13] == b"\x03" + f[0].astype("<i4").tobytes()
    rv, rn, rf, rc = read_ply(path)
    assert np.array_equal(rv, v) and np.array_equal(rn, n) and np.array_equal(rf, f) and np.array_equal(rc, c)
    assert rf.dtype == np.int32 and rv.dtype == np.float32 and rc.dtype == np.uint8
    # no colours: the three properties are gone; an empty mesh is a valid file
    path = write_ply(str(tmp_path / "b.ply"), v, n, f)
    assert b"red" not in open(path, "rb").read()[:400] and os.path.getsize(path) == len(head) - len(b"property uchar red\nproperty uchar green\nproperty uchar blue\n") + 11 * 24 + 7 * 13
    rv, rn, rf, rc = read_ply(path)
    assert np.array_equal(rv, v) and np.array_equal(rn, n) and np.array_equal(rf, f) and rc is None
    rv, rn, rf, rc = read_ply(write_ply(str(tmp_path / "c.ply"), np.zeros((0, 3)), np.zeros((0, 3)), np.zeros((0, 3), int), np.zeros((0, 3))))
    assert rv.shape == (0, 3) and rf.shape == (0, 3) and rc.shape == (0, 3)
    with pytest.raises(ValueError):
        write_ply(str(tmp_path / "d.ply"), v, n[:5], f)


def test_command_line_parser():
    from mipnerf_pl_amd import extract_mesh as cli
    from mipnerf_pl_amd.mesh import DEFAULT_THRESHOLD
    p = cli.build_parser()
    a = p.parse_args(["--ckpt", "x.ckpt", "--out_dir", "out"])
    assert (a.grid, a.bound, a.aabb, a.threshold, a.cov_scale, a.precision, a.color, a.save_density) == \
        ([256], 1.5, None, DEFAULT_THRESHOLD, 1.0, None, True, False)
    assert DEFAULT_THRESHOLD == 10.0
    assert cli.lattice_of(a) == ((256, 256, 256), (-1.5,) * 3, (1.5,) * 3)
    a = p.parse_args(["--ckpt", "x", "--out_dir", "o", "--grid", "64", "48", "32", "--bound", "2", "--no_color", "--save_density",
                      "--precision", "bf16", "--threshold", "3.5", "--cov_scale", "0"])
    assert cli.lattice_of(a) == ((64, 48, 32), (-2.0,) * 3, (2.0,) * 3)
    assert (a.color, a.save_density, a.precision, a.threshold, a.cov_scale) == (False, True, "bf16", 3.5, 0.0)
    b = p.parse_args(["--ckpt", "x", "--out_dir", "o", "--grid", "64", "48", "32", "--aabb", "-2", "-2", "-2", "2", "2", "2"])
    assert cli.lattice_of(b) == cli.lattice_of(a)                                   # --bound B is --aabb -B -B -B B B B
    c = p.parse_args(["--ckpt", "x", "--out_dir", "o", "--bound", "9", "--aabb", "-1", "0", "0.5", "1", "2", "3"])
    assert cli.lattice_of(c) == ((256,) * 3, (-1.0, 0.0, 0.5), (1.0, 2.0, 3.0))     # --aabb wins
    with pytest.raises(SystemExit):
        cli.lattice_of(p.parse_args(["--ckpt", "x", "--out_dir", "o", "--grid", "64", "48"]))
    assert "scene dependent" in p.format_help()


def test_lattice_variance_is_the_stated_float32_formula():
    from mipnerf_pl_amd.mesh import lattice_variance
    v = lattice_variance((17, 24, 40), (-1.0, -0.5, 0.25), (1.5, 1.0, 2.0), 1.0)
    assert v.dtype == np.float32
    h = (np.array([1.5, 1.0, 2.0], np.float32) - np.array([-1.0, -0.5, 0.25], np.float32)) / np.array([16, 23, 39], np.float32)
    assert np.array_equal(v, np.float32(1.0) * h * h / np.float32(12))
    assert np.array_equal(lattice_variance((4, 4, 4), (0,) * 3, (1,) * 3, 0.0), np.zeros(3, np.float32))


NEW_ENTRY_POINTS = ("mipnerf_density_grid_workspace_bytes", "mipnerf_density_grid", "mipnerf_isosurface_workspace_bytes",
                    "mipnerf_isosurface_count", "mipnerf_isosurface_emit")


def test_bindings_name_the_new_entry_points_and_arguments_are_checked_without_a_gpu():
    from mipnerf_pl_amd import _lib as L
    for n in NEW_ENTRY_POINTS:
        assert n in L.SIGNATURES
    if not os.path.exists(L.LIB_PATH):
        from mipnerf_pl_amd import build
        build.build(verbose=False)
    lib = L.lib()
    assert lib.mipnerf_abi_version() == 6                                          # the ABI only grows
    dims = (C.c_int32 * 3)
    nv, nf = C.c_int64(-1), C.c_int64(-1)
    # 7 nx ny nz >= 2^31 is refused on the arguments: no such lattice needs allocating
    for d in ((675, 675, 675), (2048, 2048, 128), (1 << 20, 2, 147)):
        assert 7 * d[0] * d[1] * d[2] >= 2 ** 31
        assert lib.mipnerf_isosurface_count(dims(*d), None, 0.0, None, 0, C.byref(nv), C.byref(nf), None) == L.E_INVALID
        assert b"2^31" in lib.mipnerf_last_error()
        assert lib.mipnerf_isosurface_workspace_bytes(*d) == 0
    assert lib.mipnerf_isosurface_count(dims(1, 8, 8), None, 0.0, None, 0, C.byref(nv), C.byref(nf), None) == L.E_INVALID
    assert lib.mipnerf_isosurface_count(dims(8, 8, 8), None, 0.0, None, 0, C.byref(nv), C.byref(nf), None) == L.E_INVALID     # null lattice
    # 512^3 must work: mask + per-point base + block tables
    n = 512 ** 3
    need = lib.mipnerf_isosurface_workspace_bytes(512, 512, 512)
    assert 5 * n < need < 5.1 * n
    assert lib.mipnerf_density_grid_workspace_bytes(None, 1024, L.PREC_FP32) == 0
    f3 = (C.c_float * 3)
    assert lib.mipnerf_density_grid(None, dims(8, 8, 8), f3(-1, -1, -1), f3(1, 1, 1), 1.0, L.PREC_FP32, None, None, 0, None) == L.E_INVALID
    assert lib.mipnerf_isosurface_emit(dims(8, 8, 1), f3(-1, -1, -1), f3(1, 1, 1), None, 0.0, None, 0, None, None, None, None, None) == L.E_INVALID


def test_ops_refuse_what_they_cannot_do():
    import torch
    from mipnerf_pl_amd import MipNerf, ops
    with pytest.raises(NotImplementedError):
        ops.density_grid(MipNerf(num_samples=8, unbounded=True), (8, 8, 8), (-1,) * 3, (1,) * 3)
    with pytest.raises(RuntimeError):
        ops.density_grid(MipNerf(num_samples=8), (8, 8, 8), (-1,) * 3, (1,) * 3)      # on the host: there is no CPU fallback
    with pytest.raises(RuntimeError):
        ops.isosurface(torch.zeros(4, 4, 4), 0.0, (-1,) * 3, (1,) * 3)
    assert len(list(itertools.permutations(range(3)))) == len(fx.PERMUTATIONS)
