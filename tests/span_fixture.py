"""numpy brute force of the span rules of include/mipnerf_hip.h (mipnerf_ray_span), on top of occupancy_fixture: the per-frustum hit
matrix in float64 with the margin argument -- the body of `occupancy_fixture.classify` before its `.any(axis=1)` -- and from it the first
and the last hitting frustum of every ray."""
import numpy as np

import occupancy_fixture as fx


def hit_matrix(occ, dims, lo, hi, origins, directions, radii, near, far, num_samples, margin=0.0, disparity=False, outside_occupied=True,
               cone_scale=1.0):
    """bool [n, N]: coarse frustum i of ray b holds an occupied cell of `occ` (bool [cz, cy, cx]) in its cell range.  Everything in
    float64; every bounding interval is grown by margin * h on both sides (negative: shrunk; an interval shrunk to nothing hits nothing)."""
    occ = np.asarray(occ, bool)
    dims = np.asarray(dims)
    lo64, hi64 = np.asarray(lo, np.float32).astype(np.float64), np.asarray(hi, np.float32).astype(np.float64)
    h = (hi64 - lo64) / (dims - 1)
    cells = dims - 1
    o, d = np.asarray(origins, np.float64), np.asarray(directions, np.float64)
    t = fx.fence_posts(near, far, num_samples, disparity)
    rho = cone_scale * np.asarray(radii, np.float64).reshape(-1, 1) * t[:, 1:]                  # [n, N]
    table = fx._volume_table(occ)
    n = o.shape[0]
    c0, c1 = np.empty((3, n, num_samples), np.int64), np.empty((3, n, num_samples), np.int64)
    outside = np.zeros((n, num_samples), bool)
    empty = np.zeros((n, num_samples), bool)
    inverted = np.zeros((n, num_samples), bool)
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
        c0[a], c1[a] = np.minimum(a0, cells[a] - 1), np.maximum(a1, 0)
    count = fx._box_count(table, c0[2], c1[2], c0[1], c1[1], c0[0], c1[0])
    hit = (count > 0) & ~empty
    if outside_occupied:
        hit |= outside
    return hit & ~inverted


def span_of(hit):
    """(live bool [n], first int [n], last int [n]) of a hit matrix [n, N]: the smallest and the largest hitting frustum; a dead ray has
    first = N, last = -1"""
    hit = np.asarray(hit, bool)
    n, N = hit.shape
    live = hit.any(axis=1)
    first = np.where(live, hit.argmax(axis=1), N)
    last = np.where(live, N - 1 - hit[:, ::-1].argmax(axis=1), -1)
    return live, first.astype(np.int64), last.astype(np.int64)


def span(*args, **kw):
    return span_of(hit_matrix(*args, **kw))


def span_share(first, last, num_samples):
    """mean of (last - first + 1) / N over the live rays"""
    live = last >= first
    return float(np.mean((last[live] - first[live] + 1) / float(num_samples))) if live.any() else float("nan")
