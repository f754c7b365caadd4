"""Numpy statements of the rules of include/mipnerf_fuse.h, written from the rules and not from csrc/fuse_rules.hpp -- the comparators of
tests/test_fuse_cpu.py and tests/test_gpu_fuse.py:

  - `integrate_f32` / `finalise_f32`: rules T1 - T6 and F in float32, one rounding per operation, vectorised over the lattice points;
  - `quantile_f64`: rule D with float64 prefixes; `quantile_f32seq`: the same with sequential float32 prefixes (an emulation of a cheaper
    kernel); `quantile_bracket`: the test that bounds what prefix rounding can move;
  - `pixel_point_f64`: the reference's pixel-to-direction formula (datasets.py:226-228 / 125-131) in float64;
  - the cameras, the depth maps and the sphere scene the tests share.
"""
import numpy as np

import isosurface_fixture as ix

F = np.float32
INF = F(np.inf)


# ---- cameras -----------------------------------------------------------------------------------------------------------------------
def look_at(eye, target, up=(0.0, 0.0, 1.0)):
    """c2w [3, 4] float64 of a camera at `eye` that looks along its -z axis at `target` (x right, y up)"""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    back = eye - target
    back /= np.linalg.norm(back)
    right = np.cross(np.asarray(up, np.float64), back)
    if np.linalg.norm(right) < 1e-6:
        right = np.cross(np.array([0.0, 1.0, 0.0]), back)
    right /= np.linalg.norm(right)
    true_up = np.cross(back, right)
    return np.concatenate([np.stack([right, true_up, back], 1), eye[:, None]], 1)


def camera_row(c2w, W, H, near, far, focal=None, pix2cam=None):
    """the 32 floats of a camera record (include/mipnerf_hip.h), float32: mode 0 with `focal`, mode 1 with `pix2cam`"""
    rec = np.zeros(32, F)
    rec[:12] = np.asarray(c2w, np.float64).reshape(-1)
    rec[21:25] = (W, H, near, far)
    rec[25] = 1.0
    if pix2cam is not None:
        rec[12:21] = np.asarray(pix2cam, np.float64).reshape(-1)
        rec[26] = 1.0
    else:
        rec[27] = focal
    return rec


def pix2cam_of(fx, fy, cx, cy, skew=0.0):
    """K^-1 with rows 1 and 2 negated (last row (0, 0, -1)), as datasets.load_realdata360 builds it"""
    K = np.array([[fx, skew, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])
    return np.diag([1.0, -1.0, -1.0]) @ np.linalg.inv(K)


def pixel_direction_f64(rec, x, y):
    """the direction of pixel (x, y) of a mode-0 / mode-1 record in float64 (datasets.py:226-228 / 125-131); the third camera component is -1"""
    rec = np.asarray(rec, np.float64)
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    if rec[26] == 0:
        c = np.stack([(x - rec[21] * 0.5 + 0.5) / rec[27], -(y - rec[22] * 0.5 + 0.5) / rec[27], -np.ones_like(x)], -1)
    else:
        c = np.stack([x + 0.5, y + 0.5, np.ones_like(x)], -1) @ rec[12:21].reshape(3, 3).T
    return c @ rec[:12].reshape(3, 4)[:, :3].T


def pixel_point_f64(rec, x, y, t):
    """o + t d of pixel (x, y)"""
    return np.asarray(rec, np.float64)[:12].reshape(3, 4)[:, 3] + np.asarray(t, np.float64)[..., None] * pixel_direction_f64(rec, x, y)


# ---- rules T and F in float32 ----------------------------------------------------------------------------------------------------------
def lattice_points_f32(dims, lo, hi):
    """(x, y, z) float32 arrays [nz, ny, nx]: p = lo + float32(i) * h, h = (hi - lo) / float32(n - 1)  (T1)"""
    lo, hi = np.asarray(lo, F), np.asarray(hi, F)
    axes = []
    for a in range(3):
        h = (hi[a] - lo[a]) / F(dims[a] - 1)
        axes.append(lo[a] + np.arange(dims[a]).astype(F) * h)
    z, y, x = np.meshgrid(axes[2], axes[1], axes[0], indexing="ij")
    return x, y, z


def integrate_f32(dims, lo, hi, trunc, carve, frames, offsets, depth, sum_, count):
    """rules T1 - T6 for the frames in order; returns new (sum, count) [nz, ny, nx] float32"""
    x, y, z = lattice_points_f32(dims, lo, hi)
    s, c = np.array(sum_, F), np.array(count, F)
    depth, trunc = np.asarray(depth, F).reshape(-1), F(trunc)
    with np.errstate(all="ignore"):
        for P, off in zip(np.asarray(frames, F).reshape(-1, 16), np.asarray(offsets, np.int64)):
            a = (P[0] * x + P[1] * y) + (P[2] * z + P[3])
            b = (P[4] * x + P[5] * y) + (P[6] * z + P[7])
            t = (P[8] * x + P[9] * y) + (P[10] * z + P[11])
            W, H, near, far = P[12:16]
            u, v = np.floor(a / t), np.floor(b / t)
            ok = (near < t) & (t <= far) & (F(0) <= u) & (u < W) & (F(0) <= v) & (v < H)                     # T2
            at = np.where(ok, off + np.where(ok, v, 0).astype(np.int64) * np.int64(W) + np.where(ok, u, 0).astype(np.int64), 0)
            D = depth[at]                                                                                    # T3
            ok &= D > 0
            free = ok & (D == INF)                                                                           # T4
            sd = D - t                                                                                       # T5
            surf = ok & ~free & ~(sd < -trunc)
            d = np.where(free, F(1), np.minimum(F(1), sd / trunc)).astype(F)
            upd = surf | (free if carve else np.zeros_like(free))
            s = np.where(upd, s + d, s).astype(F)                                                            # T6
            c = np.where(upd, c + F(1), c).astype(F)
    return s, c


def finalise_f32(sum_, count, unseen="inside"):
    with np.errstate(all="ignore"):
        return np.where(count > 0, -(np.asarray(sum_, F) / np.asarray(count, F)), F(1 if unseen == "inside" else -1)).astype(F)


# ---- rule D ------------------------------------------------------------------------------------------------------------------------
def _first_crossing(P, q):
    """per ray the first i with P_{i-1} < q <= P_i (P_{-1} = 0), or -1"""
    prev = np.concatenate([np.zeros_like(P[:, :1]), P[:, :-1]], 1)
    hit = (prev < q) & (q <= P)
    return np.where(hit.any(1), hit.argmax(1), -1), prev


def quantile_f64(w, t, q):
    """rule D with float64 prefixes of the float32 weights; q a float64 scalar or [B].  q <= 0 gives t_0 (the lower end of every bracket)"""
    w, t = np.asarray(w, np.float64), np.asarray(t, np.float64)
    wp = np.where(w > 0, w, 0.0)
    P = np.cumsum(wp, 1)
    q = np.broadcast_to(np.asarray(q, np.float64), (w.shape[0],))[:, None]
    i, prev = _first_crossing(P, q)
    r = np.arange(w.shape[0])
    ic = np.maximum(i, 0)
    with np.errstate(all="ignore"):
        f = np.clip((q[:, 0] - prev[r, ic]) / wp[r, ic], 0.0, 1.0)
    d = t[r, ic] + f * (t[r, ic + 1] - t[r, ic])
    return np.where(i < 0, np.where(q[:, 0] <= 0, t[:, 0], np.inf), d)


def quantile_f32seq(w, t, q):
    """an emulation with sequential FLOAT32 prefixes and float32 interpolation: what a cheaper kernel would compute"""
    w, t = np.asarray(w, F), np.asarray(t, F)
    wp = np.where(w > 0, w, F(0)).astype(F)
    P = np.cumsum(wp, 1, dtype=F)
    i, prev = _first_crossing(P, F(q))
    r = np.arange(w.shape[0])
    ic = np.maximum(i, 0)
    with np.errstate(all="ignore"):
        f = np.clip((F(q) - prev[r, ic]) / wp[r, ic], F(0), F(1)).astype(F)
    d = (t[r, ic] + f * (t[r, ic + 1] - t[r, ic])).astype(F)
    return np.where(i < 0, INF, d).astype(F)


def quantile_bracket(w, t, q, d):
    """Per ray: is d inside [D64(q - eps) - slack, D64(q + eps) + slack], eps = 2 N 2^-24 max(1, acc), slack = 4 * 2^-24 * t_N, with
    d = +inf allowed exactly when D64(q + eps) is +inf?  D(q) is non-decreasing in q, so the bracket holds every depth whose prefixes are off
    by less than eps.  Returns a bool [B]."""
    w64 = np.asarray(w, np.float64)
    N = w64.shape[1]
    acc = np.where(w64 > 0, w64, 0.0).sum(1)
    eps = 2.0 * N * 2.0 ** -24 * np.maximum(1.0, acc)
    slack = 4.0 * 2.0 ** -24 * np.asarray(t, np.float64)[:, -1]
    lo, hi = quantile_f64(w, t, np.float64(q) - eps), quantile_f64(w, t, np.float64(q) + eps)
    d = np.asarray(d, np.float64)
    ok = (lo - slack <= d) & (d <= hi + slack)
    return np.where(np.isinf(d), np.isinf(hi) & (d > 0), ok)


QUANTILE_NS = (1, 5, 64, 65, 129, 300, 513, 1024)
QUANTILE_CLASSES = ("empty", "soft", "opaque", "surface", "zero", "edge")
QUANTILES = (0.05, 0.5, 0.95)


def quantile_rays(N, cls, B, seed, q=0.5):
    """(weights [B, N], t [B, N + 1]) float32 of ray class `cls`:
    empty: weights that sum to < 0.04; soft: a broad bump of total 0.3 .. 1, with a NaN and a negative weight thrown in; opaque: one sample
    holds (nearly) everything; surface: a narrow bump of total ~1; zero: all-zero; edge: a soft ray scaled so that a float32 prefix lands
    on q (the float32 value of `q`) as nearly as float32 weights allow."""
    rng = np.random.default_rng(seed)
    t = np.sort(rng.uniform(2.0, 6.0, (B, N + 1)), 1).astype(F)
    i = np.arange(N)[None, :]
    centre = rng.uniform(0, N, (B, 1))
    if cls == "zero":
        w = np.zeros((B, N))
    elif cls == "empty":
        w = rng.random((B, N))
        w *= rng.uniform(0.0, 0.04, (B, 1)) / w.sum(1, keepdims=True)
    elif cls == "opaque":
        w = rng.random((B, N)) * 1e-6 / N
        w[np.arange(B), rng.integers(0, N, B)] = rng.uniform(0.96, 1.0, B)
    else:
        width = (0.5 + 0.02 * N) if cls == "surface" else (1.0 + 0.3 * N)
        w = np.exp(-0.5 * ((i - centre) / width) ** 2) + 1e-12
        w *= (rng.uniform(0.97, 1.0, (B, 1)) if cls == "surface" else rng.uniform(0.3, 1.0, (B, 1))) / w.sum(1, keepdims=True)
    w = w.astype(F)
    if cls == "edge":
        k = rng.integers(0, N, B)
        P = np.cumsum(w.astype(np.float64), 1)[np.arange(B), k]
        w = (w.astype(np.float64) * (np.float64(F(q)) / P)[:, None]).astype(F)
    if cls == "soft" and N >= 5:
        w[:, 1] = np.nan
        w[:, 3] = -0.25
    return w, t


# ---- depth maps and lattices of the integration tests --------------------------------------------------------------------------------
LATTICES = (((67, 9, 5), (-1.2, -0.9, -0.6), (1.3, 0.8, 0.7)), ((5, 6, 7), (-1.0, -1.0, -1.0), (1.0, 1.1, 1.2)))
IMAGES = ((14, 9), (6, 5))


def frame_cameras(n, seed=0):
    """n camera rows looking at the box from radius ~3, alternating mode 0 / mode 1 and the two image sizes; near 0.5, far 3.4 (points
    of the box lie beyond far), some points lie behind a camera that stands inside the box (the last one) or outside its image"""
    rng = np.random.default_rng(seed)
    rows = []
    for f in range(n):
        W, H = IMAGES[f % 2]
        d = rng.normal(size=3)
        d /= np.linalg.norm(d)
        eye = d * (0.3 if f == n - 1 and n > 1 else 3.0)
        c2w = look_at(eye, rng.uniform(-0.3, 0.3, 3))
        focal = 1.1 * W
        if f % 4 < 2:
            rows.append(camera_row(c2w, W, H, 0.5, 3.4, focal=focal))
        else:
            rows.append(camera_row(c2w, W, H, 0.5, 3.4, pix2cam=pix2cam_of(focal, 0.93 * focal, 0.5 * W + 0.4, 0.5 * H - 0.3, skew=0.02)))
    return np.stack(rows)


def frame_depths(cams, seed=1):
    """(depth flat float32, offsets int64): per frame a finite surface around t = 3 (a tilted plane, so D - t takes both signs over the
    box), with +inf, NaN, 0, a negative value and -inf pixels"""
    rng = np.random.default_rng(seed)
    maps, offsets, at = [], [], 0
    for rec in cams:
        W, H = int(rec[21]), int(rec[22])
        yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        D = (3.0 + 0.05 * (xx - W / 2) - 0.04 * (yy - H / 2) + 0.1 * rng.normal(size=(H, W))).astype(F)
        special = rng.random((H, W))
        D[special < 0.15] = np.inf
        D[(special >= 0.15) & (special < 0.20)] = np.nan
        D[(special >= 0.20) & (special < 0.24)] = 0.0
        D[(special >= 0.24) & (special < 0.28)] = -1.5
        D[(special >= 0.28) & (special < 0.30)] = -np.inf
        maps.append(D.reshape(-1))
        offsets.append(at)
        at += W * H
    return np.concatenate(maps), np.asarray(offsets, np.int64)


# ---- the sphere scene ------------------------------------------------------------------------------------------------------------------
SPHERE_GRID, SPHERE_BOUND, SPHERE_TRUNC_CELLS = 33, 1.5, 3.0
SPHERE_VIEWS, SPHERE_PIXELS, SPHERE_FOV, SPHERE_NEAR, SPHERE_FAR, SPHERE_RADIUS = 12, 64, 50.0, 0.5, 8.0, 4.0


SPHERE_MAX_OBLIQUITY = 65.0      # degrees


def sphere_view_directions(seed):
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(8, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return np.concatenate([d, -d[:4]])


def view_obliquity(directions, n=4000):
    """the largest angle (degrees) between a surface normal of the sphere and the nearest view direction, over a Fibonacci lattice"""
    k = np.arange(n) + 0.5
    z, phi = 1.0 - 2.0 * k / n, np.pi * (1.0 + 5.0 ** 0.5) * k
    p = np.stack([np.sqrt(1.0 - z * z) * np.cos(phi), np.sqrt(1.0 - z * z) * np.sin(phi), z], 1)
    return float(np.degrees(np.arccos(np.clip((p @ np.asarray(directions).T).max(1), -1.0, 1.0))).max())


def sphere_cameras(seed=None):
    """12 look-at views of the fixture's sphere from radius 4: 8 seeded random directions and the negatives of the first 4; 64 x 64
    pixels, 50 degrees field of view (mode 0).  From radius 4 a view sees the cap within acos(0.9 / 4) = 77 degrees of its direction, the
    rim at grazing incidence, where a nearest-pixel depth says little.  The statement about unseen='outside' (a second, inner shell) is one
    about a sphere whose whole surface is observed, so the seed is the first whose views see every surface point within
    SPHERE_MAX_OBLIQUITY degrees of a view direction: a coverage condition on the cameras alone."""
    if seed is None:
        seed = next(s for s in range(100) if view_obliquity(sphere_view_directions(s)) <= SPHERE_MAX_OBLIQUITY)
    d = sphere_view_directions(seed)
    focal = 0.5 * SPHERE_PIXELS / np.tan(np.radians(SPHERE_FOV) / 2)
    return np.stack([camera_row(look_at(ix.CENTRE + SPHERE_RADIUS * v, ix.CENTRE), SPHERE_PIXELS, SPHERE_PIXELS, SPHERE_NEAR, SPHERE_FAR,
                                focal=focal) for v in d])


def sphere_depths(cams):
    """(depth flat float32, offsets): the ray parameter of each pixel centre's first hit of the sphere, +inf where it misses"""
    maps, offsets, at = [], [], 0
    for rec in cams:
        W, H = int(rec[21]), int(rec[22])
        yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        d = pixel_direction_f64(rec, xx.reshape(-1), yy.reshape(-1))
        oc = np.asarray(rec, np.float64)[:12].reshape(3, 4)[:, 3] - ix.CENTRE
        A, Bh, Cc = (d * d).sum(1), (d * oc).sum(1), (oc * oc).sum() - ix.SPHERE_R ** 2
        disc = Bh * Bh - A * Cc
        with np.errstate(all="ignore"):
            t = (-Bh - np.sqrt(disc)) / A
        maps.append(np.where((disc > 0) & (t > 0), t, np.inf).astype(F))
        offsets.append(at)
        at += W * H
    return np.concatenate(maps), np.asarray(offsets, np.int64)


def sphere_lattice():
    n, b = SPHERE_GRID, SPHERE_BOUND
    h = 2 * b / (n - 1)
    return (n,) * 3, (-b,) * 3, (b,) * 3, h, SPHERE_TRUNC_CELLS * h


def check_sphere_mesh(vertices, faces):
    """the conditions of the sphere test on any (vertices, faces); returns the figures it judged"""
    v, f = np.asarray(vertices, np.float64), np.asarray(faces, np.int64)
    h = sphere_lattice()[3]
    radius_error = float(np.abs(np.linalg.norm(v - ix.CENTRE, axis=1) - ix.SPHERE_R).max())
    volume = ix.enclosed_volume(v, f)
    figures = dict(vertices=len(v), faces=len(f), euler=ix.euler_characteristic(len(v), f), radius_error=radius_error, h=h,
                   volume_error=volume / ix.SPHERE_VOLUME - 1.0)
    print("fused sphere:", figures)
    assert ix.is_closed(f) and ix.is_oriented(f)
    assert figures["euler"] == 2
    assert radius_error <= h
    assert abs(figures["volume_error"]) <= 0.06
    return figures
