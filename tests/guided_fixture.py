"""The rule of error-guided batch sampling (include/mipnerf_hip.h, mipnerf_guided_*) restated in numpy: pure integer / float32 / float64,
no torch.  What the device kernels and `train_guided` are compared with byte for byte.

Cells: every image (h, w) of `sizes` is cut into tiles of T x T pixels (smaller at the right and bottom edges), numbered image by image,
row-major inside an image.  The table is int64 [n_images + 1][4]: (first cell, first pixel, W, H) per image, last row (n_cells, N, 0, 0).
"""
import numpy as np

TWO24, TWO20, TWO30 = float(1 << 24), float(1 << 20), float(1 << 30)


def table(sizes, T):
    rows, cell, pix = [], 0, 0
    for h, w in sizes:
        rows.append((cell, pix, w, h))
        cell += ((w + T - 1) // T) * ((h + T - 1) // T)
        pix += h * w
    rows.append((cell, pix, 0, 0))
    return np.asarray(rows, np.int64)


def cells(tab, T):
    """Per cell: dict of int64 arrays img, x0, y0, w, h, n (pixels), W, pix0."""
    out = {k: [] for k in ("img", "x0", "y0", "w", "h", "W", "pix0")}
    for i, (c0, p0, W, H) in enumerate(tab[:-1]):
        for y0 in range(0, H, T):
            for x0 in range(0, W, T):
                for k, v in zip(out, (i, x0, y0, min(T, W - x0), min(T, H - y0), W, p0)):
                    out[k].append(v)
    out = {k: np.asarray(v, np.int64) for k, v in out.items()}
    out["n"] = out["w"] * out["h"]
    assert len(out["n"]) == tab[-1, 0] and out["n"].sum() == tab[-1, 1]
    return out


def draw_error(rgb, gt):
    """(fx uint64, counted bool) per ray: se = ((d0 d0) + d1 d1) + d2 d2 in float32, fx = floor((double) se 2^24 + 0.5)."""
    d = rgb.astype(np.float32) - gt.astype(np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        se = ((d[:, 0] * d[:, 0]) + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        ok = np.isfinite(se) & (se >= 0)
        fx = np.floor(np.where(ok, se, 0).astype(np.float64) * TWO24 + 0.5).astype(np.uint64)
    return fx, ok


def slots(b, B, ring, n_order):
    """(ray indices i that are touched, their ring slots) of batch b."""
    i = np.arange(B, dtype=np.int64)
    j = b * B + i
    keep = (j < n_order) if b >= 0 else np.zeros(B, bool)
    return i[keep], (j[keep] % ring)


def accumulate(s, cnt, ring_cell, b, B, n_order, rgb, gt):
    """sum / cnt (uint64 / uint32, changed in place) after batch b."""
    i, sl = slots(b, B, len(ring_cell), n_order)
    fx, ok = draw_error(rgb, gt)
    c = ring_cell[sl].astype(np.int64)
    ok = ok[i] & (c >= 0) & (c < len(s))
    np.add.at(s, c[ok], fx[i][ok])
    np.add.at(cnt, c[ok], np.uint32(1))


def fold(err, s, cnt, rate):
    """New err (float32); a cell with cnt = 0 keeps its value."""
    err = err.astype(np.float32).copy()
    v = cnt > 0
    mean = ((s[v].astype(np.float64) / cnt[v].astype(np.float64)) * (1.0 / TWO24)).astype(np.float32)
    err[v] = err[v] + np.float32(rate) * (mean - err[v])
    return err


def mass(err, n, mix):
    """(q uint64, cdf uint64, Q, A) of a map."""
    N = int(n.sum())
    ef = np.floor(err.astype(np.float64) * TWO20 + 0.5).astype(np.uint64)
    a = n.astype(np.uint64) * ef
    A = int(a.sum())
    share = n.astype(np.float64) / float(N)
    prop = a.astype(np.float64) / float(A) if A > 0 else share
    p = (1.0 - mix) * share + mix * prop
    q = np.maximum(1, np.floor(p * TWO30).astype(np.uint64)).astype(np.uint64)
    cdf = np.cumsum(q, dtype=np.uint64)
    return q, cdf, int(cdf[-1]), A


def draw(tab, T, cdf, r0, r1):
    """(order int64, weight float32, cell int32) of the draws (r0[j], r1[j]), both in [0, 2^32)."""
    g = cells(tab, T)
    N, Q = int(tab[-1, 1]), int(cdf[-1])
    r0, r1 = np.asarray(r0, np.uint64), np.asarray(r1, np.uint64)
    t = (r0 * np.uint64(Q)) >> np.uint64(32)
    c = np.searchsorted(cdf, t, side="right")                 # the first cell with cdf[c] > t
    n = g["n"][c].astype(np.uint64)
    k = ((r1 * n) >> np.uint64(32)).astype(np.int64)
    x, y = g["x0"][c] + k % g["w"][c], g["y0"][c] + k // g["w"][c]
    order = g["pix0"][c] + y * g["W"][c] + x
    q = np.diff(np.concatenate([[0], cdf.astype(np.int64)]))[c]
    share = g["n"][c].astype(np.float64) / float(N)
    weight = (share / (q.astype(np.float64) / float(Q))).astype(np.float32)
    return order.astype(np.int64), weight, c.astype(np.int32)


def cell_probabilities(cdf):
    """P_c counted exactly from the 2^32 values of r0: the number of r0 with cdf[c - 1] <= (r0 Q) >> 32 < cdf[c], over 2^32.
    (r0 Q) >> 32 >= m  <=>  r0 >= ceil(m 2^32 / Q)."""
    Q = int(cdf[-1])
    edge = [0] + [min(1 << 32, -((-int(m) << 32) // Q)) for m in cdf]
    return np.asarray([(edge[i + 1] - edge[i]) / float(1 << 32) for i in range(len(cdf))], np.float64)


def boundary_r0(cdf):
    """The two r0 on each side of every cdf boundary (the last r0 of a cell and the first of the next), plus 0 and 2^32 - 1."""
    Q = int(cdf[-1])
    out = {0, (1 << 32) - 1}
    for m in cdf[:-1]:
        first = -((-int(m) << 32) // Q)
        out.update(v for v in (first - 2, first - 1, first, first + 1) if 0 <= v < (1 << 32))
    return np.asarray(sorted(out), np.uint64)
