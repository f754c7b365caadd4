"""numpy brute force of the occupancy rules of include/mipnerf_hip.h (mipnerf_occupancy_build, mipnerf_ray_occupancy, mipnerf_compact_rays,
mipnerf_scatter_frame).  Nothing here is fast or clever: the bits come from explicit loops over corners and offsets, the ray classes from
float64 bounding boxes and a summed-volume table."""
import numpy as np


# ---- bits ---------------------------------------------------------------------------------------------------------------
def raw_occupied(lattice, threshold):
    """bool [nz - 1, ny - 1, nx - 1]: any of the 8 corner values is > threshold or is NaN"""
    f = np.asarray(lattice, np.float32)
    hot = ~(f <= np.float32(threshold))                     # > threshold or NaN
    nz, ny, nx = f.shape
    out = np.zeros((nz - 1, ny - 1, nx - 1), bool)
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                out |= hot[dz:dz + nz - 1, dy:dy + ny - 1, dx:dx + nx - 1]
    return out


def dilate(occ, d):
    """a cell is occupied iff a raw-occupied cell lies within Chebyshev distance d: OR over all (2d + 1)^3 offsets, clipped at the grid"""
    occ = np.asarray(occ, bool)
    cz, cy, cx = occ.shape
    out = np.zeros_like(occ)
    for oz in range(-d, d + 1):
        for oy in range(-d, d + 1):
            for ox in range(-d, d + 1):
                if abs(oz) >= cz or abs(oy) >= cy or abs(ox) >= cx:
                    continue                                 # the offset leaves the grid from every cell
                src = occ[max(0, oz):cz + min(0, oz), max(0, oy):cy + min(0, oy), max(0, ox):cx + min(0, ox)]
                out[max(0, -oz):cz + min(0, -oz), max(0, -oy):cy + min(0, -oy), max(0, -ox):cx + min(0, -ox)] |= src
    return out


def pack(occ):
    """uint32 [cz, cy, ceil(cx / 32)]: cell i is bit i & 31 of word i >> 5, padding bits 0"""
    occ = np.asarray(occ, bool)
    cz, cy, cx = occ.shape
    wx = (cx + 31) // 32
    words = np.zeros((cz, cy, wx), np.uint32)
    for i in range(cx):
        words[:, :, i >> 5] |= occ[:, :, i].astype(np.uint32) << np.uint32(i & 31)
    return words


def unpack(words, cx):
    words = np.asarray(words).view(np.uint32)
    out = np.zeros(words.shape[:2] + (cx,), bool)
    for i in range(cx):
        out[:, :, i] = (words[:, :, i >> 5] >> np.uint32(i & 31)) & np.uint32(1)
    return out


def occupancy_words(lattice, threshold, d):
    return pack(dilate(raw_occupied(lattice, threshold), d))


# ---- rays ---------------------------------------------------------------------------------------------------------------
def fence_posts(near, far, num_samples, disparity=False):
    """float64 [n, N + 1]: near + (far - near) * i / N, or linear in disparity"""
    lin = np.arange(num_samples + 1, dtype=np.float64) / num_samples
    near, far = np.asarray(near, np.float64).reshape(-1, 1), np.asarray(far, np.float64).reshape(-1, 1)
    if disparity:
        return 1.0 / (1.0 / near * (1.0 - lin) + 1.0 / far * lin)
    return near + (far - near) * lin


def _volume_table(occ):
    s = np.zeros(tuple(n + 1 for n in occ.shape), np.int64)
    s[1:, 1:, 1:] = occ.astype(np.int64).cumsum(0).cumsum(1).cumsum(2)
    return s


def _box_count(s, z0, z1, y0, y1, x0, x1):
    """occupied cells of the inclusive index boxes"""
    z1, y1, x1 = z1 + 1, y1 + 1, x1 + 1
    return (s[z1, y1, x1] - s[z0, y1, x1] - s[z1, y0, x1] - s[z1, y1, x0] + s[z0, y0, x1] + s[z0, y1, x0] + s[z1, y0, x0] - s[z0, y0, x0])


def classify(occ, dims, lo, hi, origins, directions, radii, near, far, num_samples, margin=0.0, disparity=False, outside_occupied=True,
             cone_scale=1.0):
    """bool [n]: a ray is live iff some coarse frustum's cell range holds an occupied cell of `occ` (bool [cz, cy, cx]).  Everything in
    float64; every bounding interval is grown by margin * h on both sides (negative: shrunk; an interval shrunk to nothing touches no cell)."""
    occ = np.asarray(occ, bool)
    dims = np.asarray(dims)
    lo64, hi64 = np.asarray(lo, np.float32).astype(np.float64), np.asarray(hi, np.float32).astype(np.float64)
    h = (hi64 - lo64) / (dims - 1)
    cells = dims - 1
    o, d = np.asarray(origins, np.float64), np.asarray(directions, np.float64)
    t = fence_posts(near, far, num_samples, disparity)
    rho = cone_scale * np.asarray(radii, np.float64).reshape(-1, 1) * t[:, 1:]                  # [n, N]
    table = _volume_table(occ)
    n = o.shape[0]
    c0, c1 = np.empty((3, n, num_samples), np.int64), np.empty((3, n, num_samples), np.int64)
    outside = np.zeros((n, num_samples), bool)
    empty = np.zeros((n, num_samples), bool)                 # nothing of the range is inside the grid
    inverted = np.zeros((n, num_samples), bool)              # an interval shrunk to nothing
    for a in range(3):
        p0 = o[:, a:a + 1] + t[:, :-1] * d[:, a:a + 1]
        p1 = o[:, a:a + 1] + t[:, 1:] * d[:, a:a + 1]
        xlo = np.minimum(p0, p1) - rho - margin * h[a]
        xhi = np.maximum(p0, p1) + rho + margin * h[a]
        inverted |= xlo > xhi
        a0, a1 = np.floor((xlo - lo64[a]) / h[a]).astype(np.int64), np.floor((xhi - lo64[a]) / h[a]).astype(np.int64)
        outside |= (a0 < 0) | (a1 > cells[a] - 1)
        a0, a1 = np.maximum(a0, 0), np.minimum(a1, cells[a] - 1)
        empty |= a0 > a1
        c0[a], c1[a] = np.minimum(a0, cells[a] - 1), np.maximum(a1, 0)                           # clamped only to index the table
    count = _box_count(table, c0[2], c1[2], c0[1], c1[1], c0[0], c1[0])
    hit = (count > 0) & ~empty
    if outside_occupied:
        hit |= outside
    return (hit & ~inverted).any(axis=1)


# ---- compaction and scatter ----------------------------------------------------------------------------------------------
def compact(live, rays):
    idx = np.flatnonzero(np.asarray(live))
    return idx, [np.asarray(r)[idx] for r in rays]


def scatter(index, compact_outputs, n, live, near, white_bkgd):
    """per level (rgb [n, 3], distance [n], acc [n]): live pixels take their compact slot, dead pixels rgb = 1 / 0, acc = 0, distance = near"""
    live = np.asarray(live).astype(bool)
    out = []
    for rgb, dist, acc in compact_outputs:
        f_rgb = np.full((n, 3), 1.0 if white_bkgd else 0.0, np.float32)
        f_dist = np.asarray(near, np.float32).reshape(n).copy()
        f_acc = np.zeros(n, np.float32)
        f_rgb[index], f_dist[index], f_acc[index] = rgb[:len(index)], dist[:len(index)], acc[:len(index)]
        assert not (~live[index]).any()
        out.append((f_rgb, f_dist, f_acc))
    return out
