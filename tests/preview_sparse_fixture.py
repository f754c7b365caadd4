"""TEST INFRASTRUCTURE for the sparse row table (include/mipnerf_preview_sparse.h), shared by tests/test_preview_sparse_cpu.py and
tests/test_gpu_preview_sparse.py: a numpy restatement of the storage rule that shares no code with csrc/preview_sparse.hpp (points from
cells by slicing, as `preview.baked_points`; ranks as the exclusive cumsum of the popcounts), the lattices and the occupancies of the
issue, and rows compacted by a boolean mask.

The lattices: (8, 9, 10) is the shared scene's; nx = 33, 65, 97 are 32 m + 1, where the table has one word per line more than the
occupancy grid; nx = 34 puts two points into the second word; (97, 2, 2) has one cell line only."""
import numpy as np

import preview_fixture as pf
import preview_mip_fixture as mf

LATTICES = ((8, 9, 10), (33, 5, 4), (34, 3, 3), (65, 4, 3), (97, 2, 2))
OCCUPANCIES = ("hollow", "clear", "set", "x31", "last")
THRESHOLD = 5.0


def words_p(nx):
    return (nx + 31) // 32


def cells_to_words(cells):
    nzc, nyc, nxc = cells.shape
    words = np.zeros((nzc, nyc, (nxc + 31) // 32), np.uint32)
    for i in range(nxc):
        words[:, :, i >> 5] |= cells[:, :, i].astype(np.uint32) << np.uint32(i & 31)
    return words


def words_to_cells(words, dims):
    nx, ny, nz = dims
    bits = (words[..., None] >> np.arange(32, dtype=np.uint32)) & np.uint32(1)
    return bits.reshape(nz - 1, ny - 1, -1)[..., :nx - 1].astype(bool)


def occupancy_words(kind, dims, seed=5):
    """uint32 [nz - 1, ny - 1, ceil((nx - 1) / 32)] of one of OCCUPANCIES; 'hollow': random cells in the high-x half only"""
    nx, ny, nz = dims
    cells = np.zeros((nz - 1, ny - 1, nx - 1), bool)
    if kind == "hollow":
        rng = np.random.default_rng(seed + nx)
        cells = rng.uniform(size=cells.shape) < 0.4
        cells[:, :, :(nx - 1) // 2] = False
    elif kind == "set":
        cells[:] = True
    elif kind == "x31":
        cells[(nz - 1) // 2, (ny - 1) // 2, min(31, nx - 2)] = True          # the last bit of the first cell word where the line has one
    elif kind == "last":
        cells[-1, -1, -1] = True
    elif kind != "clear":
        raise ValueError(kind)
    return cells_to_words(cells)


def stored_points(words, dims):
    """bool [nz, ny, nx]: the points next to a set cell"""
    nx, ny, nz = dims
    cells = words_to_cells(words, dims)
    pts = np.zeros((nz, ny, nx), bool)
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                pts[dz:dz + nz - 1, dy:dy + ny - 1, dx:dx + nx - 1] |= cells
    return pts


def numpy_table(words, dims):
    """(table uint32 [nz, ny, words_p, 2], M, stored bool [nz, ny, nx])"""
    nx, ny, nz = dims
    pts = stored_points(words, dims)
    wp = words_p(nx)
    padded = np.zeros((nz, ny, wp * 32), np.uint64)
    padded[..., :nx] = pts
    padded = padded.reshape(nz, ny, wp, 32)
    mask = (padded << np.arange(32, dtype=np.uint64)).sum(-1)
    count = padded.sum(-1).reshape(-1)
    rank = np.cumsum(count) - count
    table = np.stack([mask.astype(np.uint32), rank.reshape(nz, ny, wp).astype(np.uint32)], -1)
    return np.ascontiguousarray(table), int(count.sum()), pts


def lattice_rows(dims, degree, hollow=True):
    """(rows fp16 [nz, ny, nx, W], occupancy words of sigma > THRESHOLD) with content of its own per lattice"""
    rows, _ = pf.random_rows(degree, hollow=hollow) if tuple(dims) == pf.DIMS else mf.random_level(dims, degree, 31 + dims[0], hollow=hollow)
    return rows, mf.cell_occupancy(rows[..., 0].astype(np.float32), THRESHOLD)


def compact(rows, stored):
    """rows [M, W] of the stored points, in flat order"""
    return np.ascontiguousarray(rows.reshape(-1, rows.shape[-1])[stored.reshape(-1)])


STORAGE_EPS = 1e-5          # preview.STORAGE_EPS: the share of a box edge by which two cells count as touching


def axis_share(n_to, n_from):
    """bool [n_to - 1, n_from - 1]: the closed intervals of cell a (n_to points) and cell b (n_from points) on the unit edge come within
    STORAGE_EPS of each other; plain loops in float64"""
    out = np.zeros((n_to - 1, n_from - 1), bool)
    for a in range(n_to - 1):
        for b in range(n_from - 1):
            left, right = max(a / (n_to - 1), b / (n_from - 1)), min((a + 1) / (n_to - 1), (b + 1) / (n_from - 1))
            out[a, b] = left < right + STORAGE_EPS
    return out


def pyramid_storage_words(words, dims):
    """per level: its occupied cells plus every cell that shares a point with an occupied cell of the level below or above -- a sample
    between two levels reads both when either's bit is set (P5)"""
    cells = [words_to_cells(w, d) for w, d in zip(words, dims)]
    out = []
    for i, d in enumerate(dims):
        keep = cells[i].copy()
        for j in (i - 1, i + 1):
            if 0 <= j < len(dims):
                sx, sy, sz = (axis_share(d[a], dims[j][a]).astype(np.int64) for a in range(3))
                keep |= np.einsum("kji,ai,bj,ck->cba", cells[j].astype(np.int64), sx, sy, sz) > 0
        out.append(cells_to_words(keep))
    return out
