"""The rule of adaptive sample counts and the padded stable partition, restated in numpy (no package code): what
mipnerf_bucket_rays / ops.bucket_rays / model.CulledFrame(adaptive=True) are compared against.

    need   = ((last - first + 1) * N + S - 1) // S          1 <= need <= N for a live ray
    bucket = the smallest b with c_b >= need                 -1 for a dead ray
    base_0 = 0, base_{b+1} = round_up(base_b + count_b, 64)
    slot   = base_bucket + the ray's rank among the rays of its bucket, in the original order; -1 for a dead ray
"""
import numpy as np

ALIGN = 64


def default_ladder(N):
    """the distinct values of ceil(N * k / 4), k = 1..4"""
    return tuple(sorted({-(-N * k // 4) for k in range(1, 5)}))


def need(first, last, S, N):
    first, last = np.asarray(first, np.int64), np.asarray(last, np.int64)
    return ((last - first + 1) * N + S - 1) // S


def bucket(live, first, last, S, ladder):
    """int64 [n]: the bucket of every ray, -1 for a dead one"""
    ladder = np.asarray(ladder, np.int64)
    nd = need(first, last, S, int(ladder[-1]))
    b = np.searchsorted(ladder, nd, side="left")            # the smallest b with ladder[b] >= need
    return np.where(np.asarray(live).astype(bool), b, -1)


def bases(counts):
    out = [0]
    for c in counts:
        out.append((out[-1] + int(c) + ALIGN - 1) // ALIGN * ALIGN)
    return out


def partition(live, first, last, S, ladder):
    """(counts [B], bases [B + 1], slot [n] int64)"""
    b = bucket(live, first, last, S, ladder)
    B = len(ladder)
    counts = [int((b == k).sum()) for k in range(B)]
    base = bases(counts)
    slot = np.full(b.shape, -1, np.int64)
    for k in range(B):
        idx = np.nonzero(b == k)[0]                         # ascending: the original order
        slot[idx] = base[k] + np.arange(len(idx))
    return counts, base, slot


def sample_share(live, first, last, S, ladder):
    """the mean of c_bucket / N over the live rays; NaN when none is live"""
    b = bucket(live, first, last, S, ladder)
    lv = b >= 0
    if not lv.any():
        return float("nan")
    return float(np.asarray(ladder, np.float64)[b[lv]].mean() / float(ladder[-1]))
