"""numpy float64 restatement of the contracted-space bounding rule of include/mipnerf_hip.h (mipnerf_ray_occupancy_360 /
mipnerf_ray_span_360; csrc/raymath360.hpp contracted_frustum_box) and, on top of occupancy_fixture / span_fixture, the ray classes and
spans it gives on a bit grid laid out in contracted coordinates.  Nothing here is fast or clever."""
import numpy as np

import occupancy_fixture as fx
import span_fixture as sx


def contract(x):
    """x inside the unit ball, (2 - 1 / |x|) x / |x| outside; float64 [..., 3]"""
    x = np.asarray(x, np.float64)
    n = np.linalg.norm(x, axis=-1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(n > 1.0, (2.0 - 1.0 / n) * x / n, x)


def fence_posts(near, far, num_samples):
    """float64 [n, N + 1]: 1 / (fi s + (1 - s) ni), s = i / N, ni = 1 / near, fi = 1 / far"""
    s = np.arange(num_samples + 1, dtype=np.float64) / num_samples
    ni, fi = 1.0 / np.asarray(near, np.float64).reshape(-1, 1), 1.0 / np.asarray(far, np.float64).reshape(-1, 1)
    return 1.0 / (fi * s + (1.0 - s) * ni)


def frustum_box(t0, t1, origins, directions, radii, cone_scale=1.0, branch=None):
    """(lo [n, N, 3], hi [n, N, 3], rmin [n, N]) of the frusta [t0, t1] ([n, N] each) of rays (origins, directions [n, 3], radii [n]): the
    rule, term by term as the header states it.  `branch` None: each frustum takes the case its own rmin picks; 'outside' / 'mixed':
    every frustum is put through that case (what a test needs for a frustum whose rmin lies within rounding of 1)."""
    t0, t1 = np.asarray(t0, np.float64)[..., None], np.asarray(t1, np.float64)[..., None]
    o, d = np.asarray(origins, np.float64)[:, None, :], np.asarray(directions, np.float64)[:, None, :]
    rr = cone_scale * np.asarray(radii, np.float64).reshape(-1, 1, 1)
    rho = rr * t1
    p0, p1 = o + t0 * d, o + t1 * d
    with np.errstate(divide="ignore", invalid="ignore"):
        tc = np.fmin(np.fmax(-(o * d).sum(-1, keepdims=True) / (d * d).sum(-1, keepdims=True), t0), t1)
    rc = np.linalg.norm(o + tc * d, axis=-1, keepdims=True)
    n0, n1 = np.linalg.norm(p0, axis=-1, keepdims=True), np.linalg.norm(p1, axis=-1, keepdims=True)
    rmin, rmax = rc - rho, np.maximum(n0, n1) + rho
    with np.errstate(divide="ignore", invalid="ignore"):
        # the frustum lies wholly outside the unit ball
        u0, u1 = p0 / n0, p1 / n1
        sag = 1.0 - np.sqrt(np.maximum(0.0, (1.0 + (u0 * u1).sum(-1, keepdims=True)) / 2.0))
        e = sag + rho / rmin
        ulo, uhi = np.maximum(np.minimum(u0, u1) - e, -1.0), np.minimum(np.maximum(u0, u1) + e, 1.0)
        flo, fhi = 2.0 - 1.0 / rmin, 2.0 - 1.0 / rmax
        lo_out, hi_out = np.where(ulo < 0, ulo * fhi, ulo * flo), np.where(uhi > 0, uhi * fhi, uhi * flo)
        # otherwise
        xlo, xhi = np.minimum(p0, p1) - rho, np.maximum(p0, p1) + rho
        slo = np.where(rmax > 1, (2.0 - 1.0 / rmax) / rmax, 1.0)
        F = np.where(rmax > 1, 2.0 - 1.0 / rmax, rmax)
        lo_mix = np.clip(np.where(xlo < 0, xlo, xlo * slo), -F, F)
        hi_mix = np.clip(np.where(xhi > 0, xhi, xhi * slo), -F, F)
    pick = (rmin >= 1.0) if branch is None else np.full(rmin.shape, branch == "outside")
    lo, hi = np.where(pick, lo_out, lo_mix), np.where(pick, hi_out, hi_mix)
    bad = ~np.isfinite((n0 + n1) + (rc + rho))
    lo, hi = np.where(bad, np.nan, lo), np.where(bad, np.nan, hi)
    return lo, hi, rmin[..., 0]


def hit_matrix(occ, dims, lo, hi, origins, directions, radii, near, far, num_samples, margin=0.0, outside_occupied=True, cone_scale=1.0):
    """bool [n, N]: coarse frustum i of ray b holds an occupied cell of `occ` (bool [cz, cy, cx], a grid over lo .. hi in CONTRACTED
    coordinates) in the cell range of its box.  Everything in float64; every interval is grown by margin * h on both sides (negative:
    shrunk; an interval shrunk to nothing hits nothing).  The cell rule is that of span_fixture.hit_matrix."""
    occ = np.asarray(occ, bool)
    dims = np.asarray(dims)
    lo64, hi64 = np.asarray(lo, np.float32).astype(np.float64) * np.ones(3), np.asarray(hi, np.float32).astype(np.float64) * np.ones(3)
    h = (hi64 - lo64) / (dims - 1)
    cells = dims - 1
    t = fence_posts(near, far, num_samples)
    blo, bhi, _ = frustum_box(t[:, :-1], t[:, 1:], origins, directions, radii, cone_scale)
    table = fx._volume_table(occ)
    n = t.shape[0]
    c0, c1 = np.empty((3, n, num_samples), np.int64), np.empty((3, n, num_samples), np.int64)
    outside = np.zeros((n, num_samples), bool)
    empty = np.zeros((n, num_samples), bool)
    inverted = np.zeros((n, num_samples), bool)
    for a in range(3):
        xlo, xhi = blo[..., a] - margin * h[a], bhi[..., a] + margin * h[a]
        nan = ~(np.isfinite(xlo) & np.isfinite(xhi))
        inverted |= (xlo > xhi) & ~nan
        with np.errstate(invalid="ignore"):
            a0 = np.floor((np.where(nan, lo64[a] - h[a], xlo) - lo64[a]) / h[a]).astype(np.int64)      # a NaN interval is outside at both ends
            a1 = np.floor((np.where(nan, hi64[a] + h[a], xhi) - lo64[a]) / h[a]).astype(np.int64)
        outside |= (a0 < 0) | (a1 > cells[a] - 1)
        a0, a1 = np.maximum(a0, 0), np.minimum(a1, cells[a] - 1)
        empty |= (a0 > a1) | nan                             # ... and holds no cell of the grid
        c0[a], c1[a] = np.minimum(a0, cells[a] - 1), np.maximum(a1, 0)
    count = fx._box_count(table, c0[2], c1[2], c0[1], c1[1], c0[0], c1[0])
    hit = (count > 0) & ~empty
    if outside_occupied:
        hit |= outside
    return hit & ~inverted


def classify(*args, **kw):
    """bool [n]: a ray is live iff some coarse frustum hits (the arguments of `hit_matrix`)"""
    return hit_matrix(*args, **kw).any(axis=1)


def span(*args, **kw):
    """(live, first, last) as span_fixture.span_of"""
    return sx.span_of(hit_matrix(*args, **kw))


# ---- the ray sets the rule was checked on ------------------------------------------------------------------------------------------
def adversarial_rays(n=600, seed=5):
    """origins 0.01 .. 3 from the centre, every sixth ray aimed through the centre, unit directions, near 0.05, far 1e4, the golden
    captures' pixel radius: (origins, directions, radii, near, far) float32"""
    rng = np.random.default_rng(seed)
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    o = u * np.geomspace(0.01, 3.0, n)[rng.permutation(n)][:, None]
    d = rng.normal(size=(n, 3))
    d[::6] = -o[::6]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    one = np.ones((n, 1))
    return tuple(np.ascontiguousarray(a, np.float32) for a in (o, d, 0.027 * one, 0.05 * one, 1e4 * one))


def sample_frusta(t0, t1, origins, directions, radii, cone_scale, count, rng):
    """float64 [n, N, count, 3]: points x = o + t d + delta of every frustum, delta perpendicular to d with |delta| <= cone_scale radii t;
    a quarter of them on the end caps and a quarter on the mantle"""
    o, d = np.asarray(origins, np.float64)[:, None, None, :], np.asarray(directions, np.float64)[:, None, None, :]
    t0, t1 = np.asarray(t0, np.float64)[..., None], np.asarray(t1, np.float64)[..., None]
    shape = t0.shape[:2] + (count,)
    w = rng.uniform(size=shape)
    w[..., : count // 8] = 0.0
    w[..., count // 8: count // 4] = 1.0
    t = t0 + (t1 - t0) * w
    # an orthonormal pair perpendicular to d
    dn = d / np.linalg.norm(d, axis=-1, keepdims=True)
    helper = np.where(np.abs(dn[..., :1]) < 0.9, np.array([1.0, 0.0, 0.0]), np.array([0.0, 1.0, 0.0]))
    e1 = np.cross(dn, helper)
    e1 /= np.linalg.norm(e1, axis=-1, keepdims=True)
    e2 = np.cross(dn, e1)
    ang = rng.uniform(0.0, 2.0 * np.pi, shape)[..., None]
    frac = np.sqrt(rng.uniform(size=shape))
    frac[..., count // 4: count // 2] = 1.0
    rad = (cone_scale * np.asarray(radii, np.float64).reshape(-1, 1, 1) * t * frac)[..., None]
    return o + t[..., None] * d + rad * (np.cos(ang) * e1 + np.sin(ang) * e2)
