"""The trilinear lattice lookup of csrc/lattice_sample.hpp restated in numpy, for test_proposal_cpu.py and test_gpu_proposal.py:
`trilinear_f32` repeats the header op for op in float32 (every numpy operation on float32 arrays rounds once, as the header's do under
-ffp-contract=off), `trilinear_f64` is the same function of the same float32 inputs in float64."""
import numpy as np

F = np.float32


def inv_h(dims, lo, hi):
    """float(n - 1) / (hi - lo) per axis in float32, as the library's host code forms it; dims = (nx, ny, nz)"""
    lo, hi = np.asarray(lo, F), np.asarray(hi, F)
    return (np.asarray(dims, np.int64) - 1).astype(F) / (hi - lo)


def trilinear_f32(lattice, lo, hi, xyz):
    """lattice [nz, ny, nx] float32, lo / hi [3] in (x, y, z) order, xyz [..., 3] float32 -> [...] float32"""
    lat = np.ascontiguousarray(lattice, F)
    nz, ny, nx = lat.shape
    dims = (nx, ny, nz)
    lo32, ih = np.asarray(lo, F), inv_h(dims, lo, hi)
    p = np.asarray(xyz, F).reshape(-1, 3)
    finite = np.isfinite(p).all(-1)
    p = np.where(finite[:, None], p, F(0))
    c, f = [], []
    with np.errstate(over="ignore", invalid="ignore"):
        for a in range(3):
            u = (p[:, a] - lo32[a]) * ih[a]
            u = np.minimum(np.maximum(u, F(0)), F(dims[a] - 1))
            i = np.floor(u).astype(np.int64)
            c.append(np.minimum(i, dims[a] - 2))
            f.append(u - c[a].astype(F))
        flat = lat.reshape(-1)
        q = (c[2] * ny + c[1]) * nx + c[0]
        sy, sz = nx, nx * ny
        v000, v100, v010, v110 = flat[q], flat[q + 1], flat[q + sy], flat[q + sy + 1]
        v001, v101, v011, v111 = flat[q + sz], flat[q + sz + 1], flat[q + sz + sy], flat[q + sz + sy + 1]
        gx, gy, gz = F(1) - f[0], F(1) - f[1], F(1) - f[2]
        v00 = gx * v000 + f[0] * v100
        v10 = gx * v010 + f[0] * v110
        v01 = gx * v001 + f[0] * v101
        v11 = gx * v011 + f[0] * v111
        v0 = gy * v00 + f[1] * v10
        v1 = gy * v01 + f[1] * v11
        out = gz * v0 + f[2] * v1
    assert out.dtype == F
    return np.where(finite, out, F(0)).reshape(np.asarray(xyz).shape[:-1])


def trilinear_f64(lattice, lo, hi, xyz):
    """the same function of the same float32 inputs, every operation in float64 (finite coordinates only)"""
    lat = np.asarray(lattice, np.float64)
    nz, ny, nx = lat.shape
    dims = (nx, ny, nz)
    lo64, hi64 = np.asarray(lo, F).astype(np.float64), np.asarray(hi, F).astype(np.float64)
    p = np.asarray(xyz, F).astype(np.float64).reshape(-1, 3)
    c, f = [], []
    for a in range(3):
        u = (p[:, a] - lo64[a]) * ((dims[a] - 1) / (hi64[a] - lo64[a]))
        u = np.clip(u, 0.0, dims[a] - 1.0)
        c.append(np.minimum(np.floor(u).astype(np.int64), dims[a] - 2))
        f.append(u - c[a])
    v = lambda dx, dy, dz: lat[c[2] + dz, c[1] + dy, c[0] + dx]  # noqa: E731
    lerp = lambda a_, b_, w: (1.0 - w) * a_ + w * b_  # noqa: E731
    v0 = lerp(lerp(v(0, 0, 0), v(1, 0, 0), f[0]), lerp(v(0, 1, 0), v(1, 1, 0), f[0]), f[1])
    v1 = lerp(lerp(v(0, 0, 1), v(1, 0, 1), f[0]), lerp(v(0, 1, 1), v(1, 1, 1), f[0]), f[1])
    return lerp(v0, v1, f[2]).reshape(np.asarray(xyz).shape[:-1])


def random_lattice(shape, seed, scale=40.0):
    """a non-negative density-like lattice [nz, ny, nx]: mostly small values, some large"""
    rng = np.random.default_rng(seed)
    return (rng.random(shape) ** 4 * scale).astype(F)


def box_points(lo, hi, seed, n_random=2000):
    """float32 points [P, 3]: random ones inside the box, every face / edge / corner combination (27 per-axis choices of lo, middle,
    hi, plus the float32 neighbours of lo and hi on either side), points outside the box, and non-finite coordinates"""
    rng = np.random.default_rng(seed)
    lo, hi = np.asarray(lo, F), np.asarray(hi, F)
    inside = (lo + (hi - lo) * rng.random((n_random, 3)).astype(F)).astype(F)
    per_axis = []
    for a in range(3):
        mid = F(lo[a] + (hi[a] - lo[a]) * F(0.37))
        per_axis.append([lo[a], hi[a], mid, np.nextafter(lo[a], F(np.inf)), np.nextafter(lo[a], F(-np.inf)),
                         np.nextafter(hi[a], F(np.inf)), np.nextafter(hi[a], F(-np.inf))])
    combos = np.array([[x, y, z] for x in per_axis[0] for y in per_axis[1] for z in per_axis[2]], F)
    outside = (lo + (hi - lo) * (rng.random((400, 3)).astype(F) * F(3) - F(1))).astype(F)
    far = np.array([[3e38, 0, 0], [0, -3e38, 0], [1e30, -1e30, 1e30]], F)
    return np.concatenate([inside, combos, outside, far]).astype(F)


def nonfinite_points(lo, hi):
    mid = (np.asarray(lo, F) + np.asarray(hi, F)) / F(2)
    pts = []
    for bad in (np.nan, np.inf, -np.inf):
        for a in range(3):
            q = mid.copy()
            q[a] = bad
            pts.append(q)
    pts.append(np.array([np.nan, np.inf, -np.inf], F))
    return np.array(pts, F)
