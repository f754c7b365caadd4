"""CPU (no GPU): the sparse row table of the baked preview -- the fifth library's declarations, bindings, exports and argument checks
without a device; the storage rule of csrc/preview_sparse.hpp (g++ -O2 -ffp-contract=off from tests/hostmath/preview_sparse.cpp) against
the numpy restatement of tests/preview_sparse_fixture.py; the host sparse march against the host dense marches byte for byte;
`SparseField` and `BakedPyramid`; the file formats; the command's parser and refusals.

No tolerance anywhere: the table is integers and the sparse march reads the rows the dense march reads."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import preview_fixture as pf
import preview_mip_fixture as mf
import preview_sparse_fixture as sf
from mipnerf_pl_amd import _lib as L

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
CSRC = os.path.join(REPO, "mipnerf_pl_amd", "csrc")
F = np.float32
BG = (0.0, 0.25, 0.5)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.PREVIEW_SPARSE_LIB_PATH):
        from mipnerf_pl_amd import build
        build.build(verbose=False)
    return L.preview_sparse_lib()


def _host(name):
    src, so = os.path.join(HERE, "hostmath", name + ".cpp"), os.path.join(HERE, "hostmath", "_" + name + ".so")
    hdrs = [os.path.join(CSRC, h) for h in ("raymath.hpp", "lattice_sample.hpp", "preview_march.hpp", "preview_mip.hpp", "preview_sparse.hpp")]
    if (not os.path.exists(so)) or os.path.getmtime(so) < max(os.path.getmtime(f) for f in [src] + hdrs):
        subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", src, "-o", so])
    return C.CDLL(so)


@pytest.fixture(scope="module")
def hs():
    h = _host("preview_sparse")
    h.hm_sparse_table.restype = C.c_longlong
    h.hm_sparse_slot.restype = C.c_longlong
    return h


@pytest.fixture(scope="module")
def hm_mip():
    return _host("preview_mip")


@pytest.fixture(scope="module")
def hm_plain():
    return _host("preview")


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


# ---- the fifth library: declarations, bindings, exports ----------------------------------------------------------------------------
NAMES = ["mipnerf_preview_sparse_abi_version", "mipnerf_preview_sparse_gather", "mipnerf_preview_sparse_index",
         "mipnerf_preview_sparse_last_error", "mipnerf_preview_sparse_march", "mipnerf_preview_sparse_pack",
         "mipnerf_preview_sparse_scratch_bytes"]


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "mipnerf_preview_sparse.h")).read(), flags=re.S)


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return sorted(line.split()[-1] for line in out.splitlines() if line.strip())


def test_header_bindings_and_dynamic_symbols_are_one_set(lib):
    declared = sorted(set(re.findall(r"\b(mipnerf_[a-z0-9_]+)\s*\(", _header())))
    assert declared == sorted(L.PREVIEW_SPARSE_SIGNATURES) == NAMES
    assert _exports(L.PREVIEW_SPARSE_LIB_PATH) == declared
    for name, (_, args) in L.PREVIEW_SPARSE_SIGNATURES.items():
        proto = re.search(r"\b" + name + r"\s*\(([^)]*)\)", _header()).group(1).strip()
        count = 0 if proto in ("", "void") else proto.count(",") + 1
        assert count == len(args), (name, proto)
    assert lib.mipnerf_preview_sparse_abi_version() == 1 == L.PREVIEW_SPARSE_ABI
    assert '#include "mipnerf_preview.h"' in _header()
    assert not any(n in L.SIGNATURES or n in L.DIAG_SIGNATURES or n in L.PREVIEW_SIGNATURES or n in L.PREVIEW_MIP_SIGNATURES
                   for n in L.PREVIEW_SPARSE_SIGNATURES)
    for hdr in ("mipnerf_hip.h", "mipnerf_preview.h", "mipnerf_preview_mip.h", "mipnerf_diag.h"):
        assert "preview_sparse" not in open(os.path.join(REPO, "include", hdr)).read()


def test_struct_layouts_match_the_header():
    assert C.sizeof(L.PreviewSparseField) == C.sizeof(L.PreviewField) + 16 == 72
    assert L.PreviewSparseField.field.offset == 0 and L.PreviewSparseField.table.offset == 56 and L.PreviewSparseField.n_rows.offset == 64
    assert C.sizeof(L.PreviewSparsePyramid) == 8 + 8 * 72 and L.PreviewSparsePyramid.level.offset == 8
    hdr = _header()
    assert re.search(r"typedef struct \{\s*mipnerf_preview_field_t field;\s*const uint32_t\* table;\s*int64_t n_rows;\s*\} "
                     r"mipnerf_preview_sparse_field_t;", hdr)
    assert re.search(r"typedef struct \{\s*int32_t levels;\s*mipnerf_preview_sparse_field_t level\[8\];\s*\} mipnerf_preview_sparse_pyramid_t;", hdr)


def test_the_build_units_are_compiled_without_contraction_into_a_fifth_library():
    from mipnerf_pl_amd import build as b
    assert [u for u, _ in b.PREVIEW_SPARSE_UNITS] == ["kernels_preview_sparse.hip", "preview_sparse_capi.hip"]
    assert all("-ffp-contract=off" in flags for _, flags in b.PREVIEW_SPARSE_UNITS)
    assert os.path.basename(b.PREVIEW_SPARSE_LIB) == "libmipnerf_preview_sparse.so" == os.path.basename(L.PREVIEW_SPARSE_LIB_PATH)
    assert not any("sparse" in u for u, _ in b.UNITS + b.DIAG_UNITS + b.PREVIEW_UNITS + b.PREVIEW_MIP_UNITS)
    src = open(os.path.join(REPO, "mipnerf_pl_amd", "build.py")).read()
    assert '"include", "mipnerf_preview_sparse.h"' in src and "os.path.exists(PREVIEW_SPARSE_LIB)" in src
    rules = open(os.path.join(CSRC, "preview_sparse.hpp")).read()
    assert "MIP_HD" in rules and "preview_blend<" in rules
    assert not re.search(r"floorf|inv_h\[|expf|half_bits_to_float\(", rules)           # restates neither the index rule nor the blend
    unit = open(os.path.join(CSRC, "kernels_preview_sparse.hip")).read()
    assert '#include "preview_wave_march.hpp"' in unit and "preview_pack_row(" in unit and "__global__" in unit
    assert not re.search(r"k_\w*march\s*\(", unit)                                      # the march is the shared header's kernel
    assert not re.search(r"atomic\w*\s*\(|\basm\b", unit)
    capi = open(os.path.join(CSRC, "preview_sparse_capi.hip")).read()
    assert not re.search(r"hipMalloc|hipFree|Synchronize|hipMemcpy", capi + unit)
    dense = open(os.path.join(CSRC, "kernels_preview.hip")).read()
    assert "preview_pack_row(" in dense                                                 # one rounding rule for both packs


def _field(dims=(8, 9, 10), lo=pf.LO, hi=pf.HI, degree=1, rows=0x1000, occ=0x2000):
    return L.PreviewField((C.c_int32 * 3)(*dims), (C.c_float * 3)(*lo), (C.c_float * 3)(*hi), degree, rows, occ)


def _level(table=0x3000, n_rows=5, **kw):
    return L.PreviewSparseField(_field(**kw), table, n_rows)


def _pyramid(levels=None, count=None):
    levels = [_level(dims=d) for d in mf.LEVEL_DIMS] if levels is None else levels
    p = L.PreviewSparsePyramid()
    p.levels = len(levels) if count is None else count
    for i, f in enumerate(levels[:8]):
        p.level[i] = f
    return p


def _params(step_scale=0.5, t_min=0.0, max_steps=64, background=(1.0, 1.0, 1.0)):
    return L.PreviewParams(step_scale, t_min, max_steps, (C.c_float * 3)(*background))


def test_every_entry_point_validates_before_any_hip_call(lib):
    """No device here: a call that reached the HIP runtime would fail with code 3, not with 1 / 2 and a message naming the entry point."""
    P = 0x1000        # never dereferenced: the checks come first

    def march(pyr, params, footprint=1.0, n=4, ptrs=(P,) * 8):
        return lib.mipnerf_preview_sparse_march(C.byref(pyr) if pyr is not None else None, C.byref(params) if params is not None else None,
                                                footprint, n, *ptrs, None, None, None)

    def with_level(i, **kw):
        levels = [_level(dims=d) for d in mf.LEVEL_DIMS]
        levels[i] = _level(**dict(dict(dims=mf.LEVEL_DIMS[i]), **kw))
        return _pyramid(levels)

    one_bit = float(np.nextafter(F(pf.HI[1]), F(2.0)))
    bad = [
        (lambda: march(None, _params()), L.E_INVALID), (lambda: march(_pyramid(), None), L.E_INVALID),
        (lambda: march(_pyramid(count=0), _params()), L.E_INVALID), (lambda: march(_pyramid(count=9), _params()), L.E_INVALID),
        (lambda: march(with_level(1, hi=(pf.HI[0], one_bit, pf.HI[2])), _params()), L.E_INVALID),
        (lambda: march(with_level(1, degree=2), _params()), L.E_INVALID),
        (lambda: march(_pyramid([_level(), _level()]), _params()), L.E_INVALID),
        (lambda: march(_pyramid([_level(dims=mf.LEVEL_DIMS[1]), _level(dims=mf.LEVEL_DIMS[0])]), _params()), L.E_INVALID),
        (lambda: march(with_level(1, dims=(1, 5, 6)), _params()), L.E_INVALID),
        (lambda: march(with_level(0, dims=(1024, 1024, 1024)), _params()), L.E_INVALID),
        (lambda: march(with_level(1, rows=None), _params()), L.E_INVALID),               # NULL rows with n_rows > 0
        (lambda: march(with_level(1, occ=None), _params()), L.E_INVALID),                # a sparse level needs its occupancy
        (lambda: march(with_level(2, table=None), _params()), L.E_INVALID),              # and its table
        (lambda: march(with_level(0, n_rows=-1), _params()), L.E_INVALID),
        (lambda: march(with_level(2, n_rows=3 * 3 * 4 + 1), _params()), L.E_INVALID),
        (lambda: march(_pyramid([_level(hi=(pf.LO[0], 1.0, 2.375))]), _params()), L.E_INVALID),
        (lambda: march(_pyramid([_level(lo=(float("nan"), -0.75, 0.125))]), _params()), L.E_INVALID),
        (lambda: march(with_level(0, degree=3), _params()), L.E_UNSUPPORTED), (lambda: march(_pyramid([_level(degree=-1)]), _params()), L.E_UNSUPPORTED),
        (lambda: march(with_level(2, rows=0x1008), _params()), L.E_INVALID),
        (lambda: march(_pyramid([_level(degree=0, rows=0x1004)]), _params()), L.E_INVALID),
        (lambda: march(with_level(1, table=0x3004), _params()), L.E_INVALID),
        (lambda: march(_pyramid(), _params(), footprint=-1.0), L.E_INVALID), (lambda: march(_pyramid(), _params(), footprint=float("nan")), L.E_INVALID),
        (lambda: march(_pyramid(), _params(step_scale=0.0)), L.E_INVALID), (lambda: march(_pyramid(), _params(max_steps=0)), L.E_INVALID),
        (lambda: march(_pyramid(), _params(t_min=1.0)), L.E_INVALID), (lambda: march(_pyramid(), _params(), n=-1), L.E_INVALID),
    ] + [(lambda k=k: march(_pyramid(), _params(), ptrs=tuple(None if j == k else P for j in range(8))), L.E_INVALID) for k in range(8) if k != 2]
    for i, (call, code) in enumerate(bad):
        assert call() == code, i
        assert b"preview_sparse_march" in lib.mipnerf_preview_sparse_last_error(), i
    assert march(_pyramid(), _params(), n=0, ptrs=(None,) * 8) == L.OK
    assert march(_pyramid([_level()]), _params(), footprint=0.0, n=0, ptrs=(None,) * 8) == L.OK
    assert march(_pyramid([_level(rows=None, n_rows=0)]), _params(), n=0, ptrs=(None,) * 8) == L.OK          # nothing stored, no rows
    assert march(_pyramid([_level(dims=d, degree=0, rows=0x1008) for d in mf.LEVEL_DIMS]), _params(), n=0, ptrs=(None,) * 8) == L.OK
    # (NULL radii are valid -- every radius is 0 -- and reach the launch: covered on the GPU)

    dims, small = (C.c_int32 * 3)(8, 9, 10), (C.c_int32 * 3)(8, 1, 10)
    calls = {
        "preview_sparse_index": [
            (lambda: lib.mipnerf_preview_sparse_index(None, P, P, P, P, None), L.E_INVALID),
            (lambda: lib.mipnerf_preview_sparse_index(dims, None, P, P, P, None), L.E_INVALID),         # NULL occupancy: stays dense
            (lambda: lib.mipnerf_preview_sparse_index(dims, P, None, P, P, None), L.E_INVALID),
            (lambda: lib.mipnerf_preview_sparse_index(dims, P, P, None, P, None), L.E_INVALID),
            (lambda: lib.mipnerf_preview_sparse_index(dims, P, P, P, None, None), L.E_INVALID),
            (lambda: lib.mipnerf_preview_sparse_index(small, P, P, P, P, None), L.E_INVALID),
            (lambda: lib.mipnerf_preview_sparse_index(dims, P, 0x1004, P, P, None), L.E_INVALID)],
        "preview_sparse_gather": [
            (lambda: lib.mipnerf_preview_sparse_gather(None, 1, P, P, P, None), L.E_INVALID),
            (lambda: lib.mipnerf_preview_sparse_gather(dims, 1, None, P, P, None), L.E_INVALID),
            (lambda: lib.mipnerf_preview_sparse_gather(dims, 1, P, None, P, None), L.E_INVALID),
            (lambda: lib.mipnerf_preview_sparse_gather(dims, 1, P, P, None, None), L.E_INVALID),
            (lambda: lib.mipnerf_preview_sparse_gather(small, 1, P, P, P, None), L.E_INVALID),
            (lambda: lib.mipnerf_preview_sparse_gather(dims, 3, P, P, P, None), L.E_UNSUPPORTED),
            (lambda: lib.mipnerf_preview_sparse_gather(dims, 1, P, 0x1008, P, None), L.E_INVALID),
            (lambda: lib.mipnerf_preview_sparse_gather(dims, 2, P, P, 0x1008, None), L.E_INVALID)],
        "preview_sparse_pack": [
            (lambda: lib.mipnerf_preview_sparse_pack(-1, 1, P, P, P, None), L.E_INVALID),
            (lambda: lib.mipnerf_preview_sparse_pack(4, 3, P, P, P, None), L.E_UNSUPPORTED),
            (lambda: lib.mipnerf_preview_sparse_pack(4, -1, P, P, P, None), L.E_UNSUPPORTED),
            (lambda: lib.mipnerf_preview_sparse_pack(4, 1, None, P, P, None), L.E_INVALID),
            (lambda: lib.mipnerf_preview_sparse_pack(4, 1, P, None, P, None), L.E_INVALID),
            (lambda: lib.mipnerf_preview_sparse_pack(4, 1, P, P, None, None), L.E_INVALID)],
    }
    for who, cases in calls.items():
        for i, (call, code) in enumerate(cases):
            assert call() == code, (who, i)
            assert who.encode() in lib.mipnerf_preview_sparse_last_error(), (who, i)
    assert lib.mipnerf_preview_sparse_pack(0, 1, None, None, None, None) == L.OK
    # the scratch: one uint32 per block of 256 table words
    assert lib.mipnerf_preview_sparse_scratch_bytes(dims) == 4 * ((10 * 9 * 1 + 255) // 256)
    assert lib.mipnerf_preview_sparse_scratch_bytes((C.c_int32 * 3)(65, 40, 30)) == 4 * ((30 * 40 * 3 + 255) // 256)
    assert lib.mipnerf_preview_sparse_scratch_bytes(small) == 0 and b"preview_sparse_scratch_bytes" in lib.mipnerf_preview_sparse_last_error()
    assert lib.mipnerf_preview_sparse_scratch_bytes(None) == 0
    with pytest.raises(ValueError, match="x: .*preview_sparse"):
        L.preview_sparse_check(L.E_INVALID, "x")
    with pytest.raises(NotImplementedError):
        L.preview_sparse_check(L.E_UNSUPPORTED, "x")


# ---- the storage rule ------------------------------------------------------------------------------------------------------------
def host_table(hs, words, dims):
    nx, ny, nz = dims
    table = np.full((nz, ny, sf.words_p(nx), 2), 0xdeadbeef, np.uint32)
    total = hs.hm_sparse_table(_p(np.ascontiguousarray(words)), nx, ny, nz, _p(table))
    return table, int(total)


@pytest.mark.parametrize("dims", sf.LATTICES)
@pytest.mark.parametrize("kind", sf.OCCUPANCIES)
def test_host_build_of_the_table_against_numpy(hs, dims, kind):
    nx, ny, nz = dims
    assert hs.hm_sparse_words_p(nx) == sf.words_p(nx)
    words = sf.occupancy_words(kind, dims)
    want, m, pts = sf.numpy_table(words, dims)
    got, total = host_table(hs, words, dims)
    assert total == m == int(pts.sum()) and got.tobytes() == want.tobytes()
    if kind == "clear":
        assert m == 0 and not got.any()
    if kind == "set":
        assert m == nx * ny * nz
    if kind in ("x31", "last"):
        assert m == 8
    # the lookup: every stored point's slot is its position among the stored points; in an occupied cell the next corner is the next slot
    flat = np.cumsum(pts.reshape(-1)) - 1
    cells = sf.words_to_cells(words, dims)
    for k, j, i in np.argwhere(pts)[:: max(1, m // 200)]:
        assert hs.hm_sparse_slot(_p(got), nx, ny, int(i), int(j), int(k)) == flat[(k * ny + j) * nx + i]
    for k, j, i in np.argwhere(cells)[:: max(1, int(cells.sum()) // 100)]:
        for dk in (0, 1):
            for dj in (0, 1):
                a = hs.hm_sparse_slot(_p(got), nx, ny, int(i), int(j + dj), int(k + dk))
                assert a >= 0 and hs.hm_sparse_slot(_p(got), nx, ny, int(i) + 1, int(j + dj), int(k + dk)) == a + 1
    if not pts.all():
        k, j, i = np.argwhere(~pts)[0]
        assert hs.hm_sparse_slot(_p(got), nx, ny, int(i), int(j), int(k)) == -1


def test_garbage_bits_past_the_last_cell_store_nothing(hs):
    """the occupancy words' bits at cells >= nx - 1 are not cells: `preview.occupied_cells` slices them off and so does the rule"""
    for dims in ((8, 9, 10), (34, 3, 3), (40, 3, 3), (96, 2, 2)):          # lattices whose last cell word has bits to spare
        words = sf.occupancy_words("hollow", dims)
        dirty = words.copy()
        nx = dims[0]
        valid = (nx - 1) - 32 * (dirty.shape[-1] - 1)
        assert 0 < valid < 32
        dirty[..., -1] |= np.uint32((0xffffffff << valid) & 0xffffffff)
        assert not np.array_equal(dirty, words)
        assert host_table(hs, dirty, dims)[0].tobytes() == host_table(hs, words, dims)[0].tobytes()


def test_torch_restatement_is_the_numpy_table():
    from mipnerf_pl_amd import preview
    for dims in sf.LATTICES:
        for kind in sf.OCCUPANCIES:
            want, m, pts = sf.numpy_table(sf.occupancy_words(kind, dims), dims)
            got, total = preview.table_of_points(torch.from_numpy(pts))
            assert total == m and got.numpy().view(np.uint32).tobytes() == want.tobytes()
            assert preview.table_words(dims[0]) == sf.words_p(dims[0])


# ---- the host sparse march against the host dense marches --------------------------------------------------------------------------
def host_sparse(hs, levels, degree, rays, radii, step_scale, t_min, max_steps, footprint=mf.FOOTPRINT):
    """levels: [(compact rows, occupancy words, table, dims)]"""
    o, d, tn, tf = rays
    n, B = len(levels), o.shape[0]
    bits = [np.ascontiguousarray(r).view(np.uint16) for r, _, _, _ in levels]
    keep = [np.ascontiguousarray(w) for _, w, _, _ in levels], [np.ascontiguousarray(t) for _, _, t, _ in levels]
    rows_p = (C.c_void_p * n)(*[b.ctypes.data if b.size else None for b in bits])
    occ_p = (C.c_void_p * n)(*[w.ctypes.data for w in keep[0]])
    tab_p = (C.c_void_p * n)(*[t.ctypes.data for t in keep[1]])
    dims = np.array([d3 for _, _, _, d3 in levels], np.int32)
    rgb, acc, dist, steps, lod = np.zeros((B, 3), F), np.zeros(B, F), np.zeros(B, F), np.zeros(B, np.int32), np.zeros(B, F)
    lo, hi, bg = np.array(pf.LO, F), np.array(pf.HI, F), np.array(BG, F)
    hs.hm_preview_sparse_march(n, rows_p, occ_p, tab_p, _p(dims), _p(lo), _p(hi), degree, C.c_float(footprint), C.c_float(step_scale),
                               C.c_float(t_min), max_steps, _p(bg), C.c_longlong(B), _p(o), _p(d),
                               None if radii is None else _p(np.ascontiguousarray(radii, F)), _p(tn), _p(tf), _p(rgb), _p(acc), _p(dist),
                               _p(steps), _p(lod))
    return rgb, acc, dist, steps, lod


def host_dense_plain(hm_plain, rows, words, degree, rays, step_scale, t_min, max_steps):
    o, d, tn, tf = rays
    nz, ny, nx, _ = rows.shape
    B = o.shape[0]
    bits = np.ascontiguousarray(rows).view(np.uint16)
    rgb, acc, dist, steps = np.zeros((B, 3), F), np.zeros(B, F), np.zeros(B, F), np.zeros(B, np.int32)
    lo, hi, bg = np.array(pf.LO, F), np.array(pf.HI, F), np.array(BG, F)
    hm_plain.hm_preview_march(_p(bits), _p(np.ascontiguousarray(words)), nx, ny, nz, _p(lo), _p(hi), degree, C.c_float(step_scale),
                              C.c_float(t_min), max_steps, _p(bg), C.c_longlong(B), _p(o), _p(d), _p(tn), _p(tf), _p(rgb), _p(acc), _p(dist),
                              _p(steps))
    return rgb, acc, dist, steps


def host_dense_mip(hm_mip, levels, occupancy, dims, degree, rays, radii, step_scale, t_min, max_steps, footprint):
    o, d, tn, tf = rays
    n, B = len(levels), o.shape[0]
    bits = [np.ascontiguousarray(r).view(np.uint16) for r in levels]
    occupancy = [np.ascontiguousarray(w) for w in occupancy]
    rows_p = (C.c_void_p * n)(*[b.ctypes.data for b in bits])
    occ_p = (C.c_void_p * n)(*[w.ctypes.data for w in occupancy])
    dims = np.array(dims, np.int32)
    rgb, acc, dist, steps, lod = np.zeros((B, 3), F), np.zeros(B, F), np.zeros(B, F), np.zeros(B, np.int32), np.zeros(B, F)
    lo, hi, bg = np.array(pf.LO, F), np.array(pf.HI, F), np.array(BG, F)
    hm_mip.hm_preview_mip_march(n, rows_p, occ_p, _p(dims), _p(lo), _p(hi), degree, C.c_float(footprint), C.c_float(step_scale),
                                C.c_float(t_min), max_steps, _p(bg), C.c_longlong(B), _p(o), _p(d), _p(np.ascontiguousarray(radii, F)), _p(tn),
                                _p(tf), _p(rgb), _p(acc), _p(dist), _p(steps), _p(lod))
    return rgb, acc, dist, steps, lod


def sparse_level(rows, words, dims, stored=None):
    """`stored`: the words of the cells whose corners are kept (default: the occupied cells)"""
    table, m, pts = sf.numpy_table(words if stored is None else stored, dims)
    compact = sf.compact(rows, pts)
    assert compact.shape[0] == m
    return compact, words, table, dims


@pytest.fixture(scope="module")
def rays():
    return pf.scene_rays()


@pytest.mark.parametrize("degree", [0, 1, 2])
@pytest.mark.parametrize("dims", sf.LATTICES)
def test_host_sparse_march_is_the_host_dense_march_byte_for_byte(hs, hm_plain, rays, dims, degree):
    rows, words = sf.lattice_rows(dims, degree)
    level = sparse_level(rows, words, dims)
    assert 0 < level[0].shape[0] < rows.shape[0] * rows.shape[1] * rows.shape[2]            # really sparse, really something
    hit = 0
    for step_scale, t_min, cap in ((0.5, 0.0, 4096), (0.1, 1e-3, 70)):
        want = host_dense_plain(hm_plain, rows, words, degree, rays, step_scale, t_min, cap)
        got = host_sparse(hs, [level], degree, rays, None, step_scale, t_min, cap, footprint=0.0)
        for a, b in zip(got[:4], want):
            assert a.tobytes() == b.tobytes()
        assert (got[4] == 0).all()
        hit += int(want[3].max())
    assert hit > 0
    # an all-clear occupancy: M = 0, no rows at all, every ray a miss or a march through empty cells
    clear = sf.occupancy_words("clear", dims)
    want = host_dense_plain(hm_plain, rows, clear, degree, rays, 0.5, 0.0, 4096)
    got = host_sparse(hs, [sparse_level(rows, clear, dims)], degree, rays, None, 0.5, 0.0, 4096, footprint=0.0)
    for a, b in zip(got[:4], want):
        assert a.tobytes() == b.tobytes()
    assert (got[3] == 0).all() and (got[1] == 0).all()


@pytest.mark.parametrize("degree", [0, 1, 2])
def test_host_sparse_pyramid_is_the_host_dense_pyramid_byte_for_byte(hs, hm_mip, rays, degree):
    made = [r for r, _ in mf.scene_levels(degree, hollow=True)]
    words = [mf.cell_occupancy(r[..., 0].astype(F), sf.THRESHOLD) for r in made]
    # a sample between two levels reads both when either's bit is set (P5), so a level keeps more than its own occupied cells
    stored = sf.pyramid_storage_words(words, mf.LEVEL_DIMS)
    assert all(not (w & ~k).any() for w, k in zip(words, stored)) and any((k & ~w).any() for w, k in zip(words, stored))
    levels = [sparse_level(r, w, d, k) for r, w, d, k in zip(made, words, mf.LEVEL_DIMS, stored)]
    assert all(lv[0].shape[0] < r.shape[0] * r.shape[1] * r.shape[2] for lv, r in zip(levels[:1], made))       # level 0 is still sparse
    radii = mf.scene_radii()
    for footprint in (mf.FOOTPRINT, 0.0):
        for step_scale, t_min, cap in ((0.5, 0.0, 4096), (0.1, 1e-3, 70)):
            want = host_dense_mip(hm_mip, made, words, mf.LEVEL_DIMS, degree, rays, radii, step_scale, t_min, cap, footprint)
            got = host_sparse(hs, levels, degree, rays, radii, step_scale, t_min, cap, footprint)
            for a, b in zip(got, want):
                assert a.tobytes() == b.tobytes()
    assert want[3].max() > 0 and 0.3 < host_dense_mip(hm_mip, made, words, mf.LEVEL_DIMS, degree, rays, radii, 0.5, 0.0, 4096,
                                                      mf.FOOTPRINT)[4].max()


# ---- python layer without a device -----------------------------------------------------------------------------------------------
def _occupancy(words, dims):
    from mipnerf_pl_amd import ops
    occ = ops.Occupancy(torch.from_numpy(np.ascontiguousarray(words).view(np.int32)).view(torch.uint32), dims, pf.LO, pf.HI)
    occ.threshold, occ.dilate = sf.THRESHOLD, 0
    return occ


def _sparse(dims, degree=1, table=None, rows=None, stored=None):
    from mipnerf_pl_amd import preview
    dense, words = sf.lattice_rows(dims, degree)
    want, m, pts = sf.numpy_table(words if stored is None else stored, dims)
    rows = sf.compact(dense, pts) if rows is None else rows
    table = want if table is None else table
    return preview.SparseField(torch.from_numpy(rows), torch.from_numpy(table.view(np.int32)), dims, pf.LO, pf.HI, degree,
                               _occupancy(words, dims), sf.THRESHOLD, stored=None if stored is None else _occupancy(stored, dims)), dense, words, pts


def _sparse_levels():
    """the three levels of the shared scene, each keeping the cells of the numpy `pyramid_storage_words`"""
    words = [sf.lattice_rows(d, 1)[1] for d in mf.LEVEL_DIMS]
    return [_sparse(d, stored=k) for d, k in zip(mf.LEVEL_DIMS, sf.pyramid_storage_words(words, mf.LEVEL_DIMS))]


def test_pyramid_storage_is_the_numpy_restatement():
    from mipnerf_pl_amd import preview
    assert preview.STORAGE_EPS == sf.STORAGE_EPS
    for dims in (mf.LEVEL_DIMS, ((33, 5, 4), (17, 3, 3)), ((65, 4, 3), (33, 3, 2), (17, 2, 2))):
        words = [sf.occupancy_words("hollow", d, seed=9) for d in dims]
        want = sf.pyramid_storage_words(words, dims)
        got = preview.pyramid_storage([_occupancy(w, d) for w, d in zip(words, dims)])
        for g, w, own in zip(got, want, words):
            assert g.bits.view(torch.int32).numpy().view(np.uint32).tobytes() == w.tobytes()
            assert not (own & ~w).any()
    # a lone occupied cell of the coarse level makes the fine level keep every cell it overlaps: 2 x 2 x 2 of them plus the cells touching
    # its faces where the lattices are aligned (8 -> 4 points: 7 cells against 3, not aligned; 9 -> 5 points: aligned)
    coarse = np.zeros((4, 4, 4), bool)
    coarse[1, 2, 1] = True
    got = preview.pyramid_storage([_occupancy(sf.cells_to_words(np.zeros((8, 8, 8), bool)), (9, 9, 9)),
                                   _occupancy(sf.cells_to_words(coarse), (5, 5, 5))])
    fine = sf.words_to_cells(got[0].bits.view(torch.int32).numpy().view(np.uint32), (9, 9, 9))
    want = np.zeros((8, 8, 8), bool)
    want[1:5, 3:7, 1:5] = True                     # cells 2 .. 3 (4 .. 5 on y) and one touching neighbour on each side
    assert np.array_equal(fine, want)
    one = _occupancy(sf.occupancy_words("hollow", (8, 9, 10)), (8, 9, 10))
    assert preview.pyramid_storage([one])[0] is one


def test_sparse_field_counts_checks_its_table_and_round_trips(tmp_path):
    from mipnerf_pl_amd import preview
    dims = (33, 5, 4)
    field, dense, words, pts = _sparse(dims)
    m = int(pts.sum())
    assert field.n_rows == m and field.stored_share() == m / (33 * 5 * 4)
    assert field.nbytes == m * 32 + 4 * 5 * 2 * 2 * 4 + words.size * 4 and field.dense_nbytes == 33 * 5 * 4 * 32 + words.size * 4
    assert torch.equal(field.stored_points(), torch.from_numpy(pts))
    # to_dense: the stored rows at their points, zeros elsewhere (NOT the dense bake's bytes there: that keeps sigma)
    back = field.to_dense()
    assert isinstance(back, preview.BakedField) and back.occupancy is field.occupancy
    got = back.rows.numpy().view(np.uint16)
    assert np.array_equal(got[pts], dense.view(np.uint16)[pts]) and not got[~pts].any() and dense[~pts].any()
    # a foreign table is recomputed from the occupancy and a mismatch refused
    want = sf.numpy_table(words, dims)[0]
    for wrong in (want ^ np.uint32(1), np.roll(want, 1, axis=2)):
        with pytest.raises(ValueError, match="not the one of the stored cells"):
            _sparse(dims, table=np.ascontiguousarray(wrong))
    with pytest.raises(ValueError, match=f"have {m} corner points, rows holds {m - 1}"):
        _sparse(dims, rows=sf.compact(dense, pts)[:-1])
    rows_t, table_t = field.rows, field.table
    with pytest.raises(ValueError, match="needs its occupancy"):
        preview.SparseField(rows_t, table_t, dims, pf.LO, pf.HI, 1, None)
    with pytest.raises(ValueError, match="table must be contiguous int32"):
        preview.SparseField(rows_t, table_t[:, :, :1], dims, pf.LO, pf.HI, 1, field.occupancy)
    with pytest.raises(ValueError, match="rows must be contiguous fp16"):
        preview.SparseField(rows_t.float(), table_t, dims, pf.LO, pf.HI, 1, field.occupancy)
    with pytest.raises(ValueError, match="rows must be contiguous fp16"):
        preview.SparseField(rows_t, table_t, dims, pf.LO, pf.HI, 2, field.occupancy)
    with pytest.raises(ValueError, match="occupancy grid must lie"):
        preview.SparseField(rows_t, table_t, dims, pf.LO, pf.HI, 1, _occupancy(sf.occupancy_words("set", (8, 9, 10)), (8, 9, 10)))
    with pytest.raises(NotImplementedError, match="degree"):
        preview.SparseField(rows_t, table_t, dims, pf.LO, pf.HI, 3, field.occupancy)
    # a dense lattice without an occupancy stays dense
    with pytest.raises(ValueError, match="stays dense"):
        preview.BakedField(torch.from_numpy(dense), dims, pf.LO, pf.HI, 1).to_sparse()
    # the file: keys of its own, and every loader names the right one
    path = field.save(str(tmp_path / "s.npz"))
    with np.load(path) as z:
        assert sorted(z.files) == ["degree", "dilate", "dims", "hi", "lo", "occupancy", "sparse_rows", "table", "threshold"]
        assert z["table"].dtype == np.uint32 and z["table"].tobytes() == want.tobytes()
    again = preview.SparseField.load(path, "cpu")
    assert torch.equal(again.rows.view(torch.int16), field.rows.view(torch.int16)) and torch.equal(again.table, field.table)
    assert again.dims == dims and again.lo == field.lo and again.hi == field.hi and again.degree == 1 and again.threshold == sf.THRESHOLD
    assert torch.equal(again.occupancy.bits.view(torch.int32), field.occupancy.bits.view(torch.int32)) and again.occupancy.dilate == 0
    assert preview.BakedPyramid.stored_sparse(path) and preview.BakedPyramid.stored_levels(path) is None
    assert preview.BakedField.stored_degree(path) == 1
    with pytest.raises(ValueError, match="SparseField.load"):
        preview.BakedField.load(path, "cpu")
    with pytest.raises(ValueError, match="SparseField.load"):
        preview.BakedPyramid.load(path, "cpu")
    dense_path = back.save(str(tmp_path / "d.npz"))
    assert not preview.BakedPyramid.stored_sparse(dense_path)
    with pytest.raises(ValueError, match="BakedField.load"):
        preview.SparseField.load(dense_path, "cpu")


def test_pyramid_of_sparse_levels_refuses_a_mix_and_round_trips(tmp_path):
    from mipnerf_pl_amd import preview
    fields = [m[0] for m in _sparse_levels()]
    pyr = preview.BakedPyramid(fields)
    # levels that keep their own occupied cells only do not hold every row a sample between two levels reads
    with pytest.raises(ValueError, match="does not store the rows"):
        preview.BakedPyramid([_sparse(d)[0] for d in mf.LEVEL_DIMS])
    assert len(preview.BakedPyramid([_sparse(mf.LEVEL_DIMS[0])[0]])) == 1          # one level reads nothing else
    with pytest.raises(ValueError, match="occupied cell is not among the stored"):
        _sparse((8, 9, 10), stored=sf.occupancy_words("clear", (8, 9, 10)))
    assert pyr.sparse and len(pyr) == 3 and pyr.nbytes == sum(f.nbytes for f in fields) < pyr.dense_nbytes == sum(f.dense_nbytes for f in fields)
    assert pyr.stored_share() == sum(f.n_rows for f in fields) / float(sum(np.prod(d) for d in mf.LEVEL_DIMS))
    dense = [f.to_dense() for f in fields]
    plain = preview.BakedPyramid(dense)
    assert not plain.sparse and plain.stored_share() == 1.0 and plain.dense_nbytes == plain.nbytes == pyr.dense_nbytes
    with pytest.raises(ValueError, match="not a mix"):
        preview.BakedPyramid([fields[0], dense[1], fields[2]])
    with pytest.raises(ValueError, match="not a mix"):
        preview.BakedPyramid([dense[0], fields[1]])
    with pytest.raises(ValueError, match="increase strictly"):
        preview.BakedPyramid([fields[1], fields[0]])
    path = pyr.save(str(tmp_path / "p.npz"))
    assert preview.BakedPyramid.stored_levels(path) == 3 and preview.BakedPyramid.stored_sparse(path)
    with np.load(path) as z:
        assert int(z["sparse"]) == 1 and "l0_sparse_rows" in z.files and "l2_table" in z.files and "l0_rows" not in z.files
        assert "l1_stored" in z.files
    again = preview.BakedPyramid.load(path, "cpu")
    assert again.sparse and len(again) == 3
    for a, b in zip(again.levels, fields):
        assert torch.equal(a.rows.view(torch.int16), b.rows.view(torch.int16)) and torch.equal(a.table, b.table) and a.dims == b.dims
        assert torch.equal(a.stored.bits.view(torch.int32), b.stored.bits.view(torch.int32))
    with pytest.raises(ValueError, match="BakedPyramid.load"):
        preview.SparseField.load(path, "cpu")
    # the dense pyramid's file is what it was
    dense_path = plain.save(str(tmp_path / "d.npz"))
    with np.load(dense_path) as z:
        assert "sparse" not in z.files
    assert not preview.BakedPyramid.stored_sparse(dense_path) and not preview.BakedPyramid.load(dense_path, "cpu").sparse


def test_marching_a_sparse_lattice_without_its_occupancy_is_refused():
    from mipnerf_pl_amd import preview
    field = _sparse((8, 9, 10))[0]
    o, d, tn, tf = [torch.from_numpy(a) for a in pf.scene_rays()]
    with pytest.raises(ValueError, match="without its occupancy"):
        preview.march(field, o, d, tn, tf, BG, use_occupancy=False)


def test_bake_field_sparse_refuses_what_bake_field_refuses():
    from types import SimpleNamespace
    from mipnerf_pl_amd import preview
    with pytest.raises(NotImplementedError, match="unbounded=True.*contracted"):
        preview.bake_field(SimpleNamespace(unbounded=True, num_levels=2), grid=8, lo=-1, hi=1, sparse=True)
    with pytest.raises(ValueError, match="box"):
        preview.bake_pyramid(SimpleNamespace(unbounded=False, num_levels=2), grid=8, sparse=True)
    import inspect
    assert inspect.signature(preview.bake_field).parameters["sparse"].default is False


# ---- command line ----------------------------------------------------------------------------------------------------------------
def test_parser_sparse():
    from mipnerf_pl_amd import preview
    p = preview.build_parser()
    assert p.parse_args(["--out_dir", "o"]).sparse is False
    assert p.parse_args(["--out_dir", "o", "--sparse"]).sparse is True
    a = p.parse_args(["--out_dir", "o", "--sparse", "--mip", "--save_baked"])
    assert a.sparse is True and a.mip == 4 and a.save_baked is True
    assert "--sparse" in p.format_help()
    from mipnerf_pl_amd import eval as eval_cli
    from mipnerf_pl_amd import render_video
    for parser in (eval_cli.build_parser(), render_video.build_parser()):
        assert "--sparse" not in parser.format_help()


def test_kind_mismatch_is_refused_before_the_checkpoint_is_opened(tmp_path):
    from mipnerf_pl_amd import preview
    missing = str(tmp_path / "no_such.ckpt")               # never opened: the refusal comes first
    out = str(tmp_path / "o")
    base = ["--ckpt", missing, "--out_dir", out]
    fields = [m[0] for m in _sparse_levels()]
    sparse_single = fields[0].save(str(tmp_path / "ss.npz"))
    dense_single = fields[0].to_dense().save(str(tmp_path / "ds.npz"))
    sparse_pyr = preview.BakedPyramid(fields).save(str(tmp_path / "sp.npz"))
    dense_pyr = preview.BakedPyramid([f.to_dense() for f in fields]).save(str(tmp_path / "dp.npz"))
    for extra in (["--baked", sparse_single], ["--baked", sparse_pyr, "--mip", "3"]):
        with pytest.raises(SystemExit, match="holds sparse rows: give --sparse"):
            preview.main(base + extra)
    for extra in (["--baked", dense_single, "--sparse"], ["--baked", dense_pyr, "--mip", "3", "--sparse"]):
        with pytest.raises(SystemExit, match="holds dense rows, --sparse asks for sparse ones"):
            preview.main(base + extra)
    with pytest.raises(SystemExit, match="single lattice, --mip asks for 3"):          # the level check still comes first
        preview.main(base + ["--baked", sparse_single, "--mip", "3", "--sparse"])
    for ok in (["--baked", sparse_single, "--sparse"], ["--baked", sparse_pyr, "--mip", "3", "--sparse"], ["--baked", dense_single],
               ["--baked", dense_pyr, "--mip", "3"]):
        with pytest.raises(FileNotFoundError):             # matching kinds: on to the (missing) checkpoint
            preview.main(base + ok)
    assert not os.path.exists(out)
