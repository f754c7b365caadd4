"""Rules Q2 - Q4 of csrc/lattice_sample_360.hpp restated in numpy, for test_proposal360_cpu.py and test_gpu_proposal360.py: the footprint,
`mip_level` of csrc/preview_mip.hpp, the trilinear value (tests/proposal_fixture.py) and the mix of two levels.  `pyramid_f32` repeats
the header op for op in float32 (every numpy operation on float32 arrays rounds once, as the header's do under -ffp-contract=off),
`pyramid_f64` is the same function of the same float32 inputs in float64."""
import numpy as np

import proposal_fixture as px

F = np.float32
PYRAMIDS = {                       # name -> lattice shapes [nz, ny, nx], finest first
    "L1": [(2, 2, 2)],
    "L2": [(5, 7, 9), (3, 4, 5)],
    "L4": [(33, 33, 33), (17, 17, 17), (9, 9, 9), (5, 5, 5)],
}
LO, HI = (-2.0, -2.0, -2.0), (2.0, 2.0, 2.0)      # the usual box of the contracted space


def random_pyramid(name, seed):
    return [px.random_lattice(shape, seed=seed + 7 * l) for l, shape in enumerate(PYRAMIDS[name])]


def spacings(lattices, lo, hi):
    """spacing[l] = max over the axes of (hi - lo) / float(n_l - 1) in float32, as the library's host code forms it"""
    lo, hi = np.asarray(lo, F), np.asarray(hi, F)
    out = []
    for lat in lattices:
        nz, ny, nx = np.asarray(lat).shape
        out.append(((hi - lo) / (np.asarray((nx, ny, nz), np.int64) - 1).astype(F)).max())
    return np.asarray(out, F)


def footprint_f32(footprint, cov):
    """Q2: cov [..., 6] float32 (xx, xy, xz, yy, yz, zz) -> w float32"""
    cov = np.asarray(cov, F)
    with np.errstate(invalid="ignore", over="ignore"):
        w = F(footprint) * (F(2) * np.sqrt((cov[..., 0] + cov[..., 3]) + cov[..., 5]))
    assert w.dtype == F
    return w


def mip_level_f32(spacing, w):
    """Q3 = P4 of csrc/preview_mip.hpp, float32: (l int, g float32) per entry of w"""
    spacing, w = np.asarray(spacing, F), np.asarray(w, F)
    L = len(spacing)
    l, g = np.zeros(w.shape, np.int64), np.zeros(w.shape, F)
    if L == 1:
        return l, g
    with np.errstate(invalid="ignore"):
        above = w > spacing[0]                     # False for a NaN
        top = above & (w >= spacing[L - 1])
        mid = above & ~top
        lv, sl, sn = np.zeros(w.shape, np.int64), np.full(w.shape, spacing[0], F), np.full(w.shape, spacing[1], F)
        for k in range(1, L - 1):
            m = spacing[k] <= w
            lv[m], sl[m], sn[m] = k, spacing[k], spacing[k + 1]
        gm = (w - sl) / (sn - sl)
    assert gm.dtype == F
    l[top] = L - 1
    l[mid], g[mid] = lv[mid], gm[mid]
    return l, g


def pyramid_f32(lattices, lo, hi, footprint, mean, cov):
    """Q2 - Q4: lattices = list of [nz, ny, nx] float32 (finest first), mean [..., 3], cov [..., 6] float32 -> (value, l, g)"""
    mean, cov = np.asarray(mean, F), np.asarray(cov, F)
    shape = mean.shape[:-1]
    mean, cov = mean.reshape(-1, 3), cov.reshape(-1, 6)
    finite = np.isfinite(mean).all(-1)
    l, g = mip_level_f32(spacings(lattices, lo, hi), footprint_f32(footprint, cov))
    two = g > 0
    v, upper = np.zeros(len(mean), F), np.zeros(len(mean), F)
    for lv, lat in enumerate(lattices):
        own, nxt = finite & (l == lv), finite & two & (l + 1 == lv)
        if own.any():
            v[own] = px.trilinear_f32(lat, lo, hi, mean[own])
        if nxt.any():
            upper[nxt] = px.trilinear_f32(lat, lo, hi, mean[nxt])
    with np.errstate(invalid="ignore"):
        mixed = (F(1) - g) * v + g * upper
    assert mixed.dtype == F
    out = np.where(finite, np.where(two, mixed, v), F(0)).astype(F)
    return out.reshape(shape), l.reshape(shape), g.reshape(shape)


def pyramid_f64(lattices, lo, hi, footprint, mean, cov):
    """the same function of the same float32 inputs, every operation in float64 (finite means, finite covariances with a non-negative
    trace); the level is found from the float64 footprint against the float32 spacings"""
    mean, cov = np.asarray(mean, F).astype(np.float64).reshape(-1, 3), np.asarray(cov, F).astype(np.float64).reshape(-1, 6)
    s = spacings(lattices, lo, hi).astype(np.float64)
    L = len(s)
    w = float(F(footprint)) * 2.0 * np.sqrt(cov[:, 0] + cov[:, 3] + cov[:, 5])
    values = [px.trilinear_f64(lat, lo, hi, mean.astype(F)) for lat in lattices]
    out = values[0].copy()
    if L > 1:
        out = np.where(w >= s[L - 1], values[L - 1], out)
        for k in range(L - 1):
            m = (w > s[k]) & (w < s[k + 1]) if k == 0 else (w >= s[k]) & (w < s[k + 1])
            gk = (w - s[k]) / (s[k + 1] - s[k])
            out = np.where(m, (1.0 - gk) * values[k] + gk * values[k + 1], out)
    return out


def covariances_for(spacing, footprint, seed, per_case=40):
    """diagonal-dominant covariances [P, 6] float32 whose footprint w = footprint * 2 sqrt(trace) hits: below spacing[0], exactly each
    spacing (where float32 can), between each pair, above the last; the trace is split unevenly over the axes and the off-diagonal
    entries are random (the rule must not read them)"""
    rng = np.random.default_rng(seed)
    spacing = np.asarray(spacing, np.float64)
    targets = [0.0, 0.3 * spacing[0], float(np.nextafter(F(spacing[0]), F(0)))]
    for k, s in enumerate(spacing):
        targets += [float(s), float(np.nextafter(F(s), F(np.inf)))]
        if k + 1 < len(spacing):
            targets += list(s + (spacing[k + 1] - s) * np.array([0.01, 0.25, 0.5, 0.99]))
    targets += [1.5 * spacing[-1], 100.0 * spacing[-1]]
    cov = []
    for w in targets:
        trace = (w / (2.0 * max(float(footprint), 1e-30))) ** 2 if footprint > 0 else w * w
        split = rng.dirichlet((1.0, 1.0, 1.0), per_case)
        off = rng.normal(size=(per_case, 3)) * trace
        cov.append(np.stack([trace * split[:, 0], off[:, 0], off[:, 1], trace * split[:, 1], off[:, 2], trace * split[:, 2]], -1))
    return np.concatenate(cov).astype(F)
