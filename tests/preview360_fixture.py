"""Rules C1 - C5 of include/mipnerf_preview_360.h (with rules 5 - 7 of include/mipnerf_preview.h) restated in numpy float64, for
test_preview360_cpu.py and test_gpu_preview360.py.  The fixture is given the fp16 rows as they are and marches one ray after the other:
it knows nothing of wavefronts or blocks.  It also says which rays are FRAGILE -- rays on which fp32 arithmetic may legitimately land a
sample in another cell, on the other side of a box face, or gain / lose a sample:
    - some sample's z lies within 1e-4 of a cell of a cell face or a box face, or
    - the last sample, or the first missing one, lies within 1e-4 s of wb (or w_0 does: the ray is about half a step long)."""
import numpy as np

from preview_fixture import ROW_HALVES, miss_distance, occupancy_bit, pack_rows, sh_basis       # noqa: F401  (re-exported)

FRAGILE = 1e-4
TINY_P = 2.0 ** -20


def contract(x):
    x = np.asarray(x, np.float64)
    n = np.linalg.norm(x, axis=-1, keepdims=True)
    safe = np.maximum(n, 1e-300)
    return np.where(n <= 1.0, x, (2.0 - 1.0 / safe) * x / safe)


class Ray:
    """C2 - C3 of one ray in float64; `hit` False: a miss."""

    def __init__(self, o, d, near, far, R):
        o, d = np.asarray(o, np.float64), np.asarray(d, np.float64)
        near, far = float(near), float(far)
        self.o, self.d, self.hit = o, d, False
        with np.errstate(all="ignore"):
            if not (np.isfinite(o).all() and np.isfinite(d).all() and np.isfinite(near) and np.isfinite(far) and far > near):
                return
            length = float(np.sqrt((d * d).sum()))
            if not length > 0.0 or not np.isfinite(np.float32(length)):
                return
            self.len, self.u = length, d / length
            self.tc = -float(o @ self.u)
            m = o + self.tc * self.u
            self.p2 = float(m @ m)
            if not self.p2 < R * R:
                return
            half = np.sqrt(R * R - self.p2)
            self.la, self.lb = max(near * length, self.tc - half), min(far * length, self.tc + half)
            if not self.la < self.lb:
                return
        self.p = np.sqrt(self.p2)
        self.c = np.sqrt(4.0 * self.p2 + 1.0)
        self.ts = np.sqrt(max(self.c - self.p2, 0.0))
        self.hit = True
        self.wa, self.wb = float(self.W(self.la - self.tc)), float(self.W(self.lb - self.tc))

    def W(self, tau):
        tau = np.asarray(tau, np.float64)
        a = np.abs(tau)
        g = np.maximum(a - self.ts, 0.0) / np.maximum(self.p2 + a * self.ts, 1e-300)
        beyond = self.ts + (self.c * g if self.p < TINY_P else (self.c / self.p) * np.arctan(self.p * g))
        return np.where(a <= self.ts, tau, np.sign(tau) * beyond)

    def V(self, w):
        w = np.asarray(w, np.float64)
        a = np.abs(w)
        D = np.maximum(a - self.ts, 0.0)
        with np.errstate(all="ignore"):
            q = D / self.c if self.p < TINY_P else np.tan(self.p * D / self.c) / self.p
            den = 1.0 - q * self.ts
            v = np.sign(w) * (self.ts + q * self.p2) / den
        lo, hi = self.la - self.tc, self.lb - self.tc
        v = np.where(den > 0.0, v, np.where(w < 0.0, lo, hi))
        return np.clip(np.where(a <= self.ts, w, v), lo, hi)

    def samples(self, s, max_steps):
        """C4: dict of the existing samples' w, tau, t, x, z, delta and the edges e_0 .. e_n."""
        n = int(min(max_steps, max(0, np.ceil((self.wb - self.wa) / s) + 2)))
        i = np.arange(n)
        w = self.wa + (i + 0.5) * s
        w = w[w < self.wb]
        if w.shape[0] == 0 and max_steps >= 1:
            w = np.array([0.5 * (self.wa + self.wb)])          # a hit ray shorter than half a step has this one sample
        n = w.shape[0]
        tau = self.V(w)
        t = (self.tc + tau) / self.len
        x = self.o + t[:, None] * self.d
        we = np.minimum(self.wa + np.arange(n + 1) * s, self.wb)
        if n and not self.wa + (n + 0.5) * s < self.wb:
            we[n] = self.wb                       # the last sample by w takes the remainder of less than half a step
        edges = self.V(we)
        return dict(w=w, tau=tau, t=t, x=x, z=contract(x), edges=edges, delta=np.maximum(np.diff(edges), 0.0))


def lattice_step(dims, lo, hi, step_scale):
    """C1 with the library's fp32 h (the lattice is DEFINED by float32 lo, hi): the step is a float32 number."""
    n = np.asarray(dims)
    h32 = (np.asarray(hi, np.float32) - np.asarray(lo, np.float32)) / (n - 1).astype(np.float32)
    return float(np.float32(step_scale) * h32.min())


def march(rows, lo, hi, degree, far_radius, origins, directions, near, far, step_scale, t_min, max_steps, background, occupancy=None):
    """(rgb [B, 3], acc [B], distance [B], steps [B] int32, fragile [B] bool).  rows: fp16 [nz, ny, nx, W] over the contracted box lo .. hi
    (the float32 values the library is given); occupancy: uint32 words or None."""
    rows64 = np.asarray(rows).astype(np.float64)
    nz, ny, nx, _ = rows64.shape
    n = np.array([nx, ny, nz])
    s = lattice_step(n, lo, hi, step_scale)
    lo = np.asarray(lo, np.float32).astype(np.float64)
    hi = np.asarray(hi, np.float32).astype(np.float64)
    h = (hi - lo) / (n - 1)
    bg = np.asarray(background, np.float64)
    o_all, d_all = np.asarray(origins, np.float64), np.asarray(directions, np.float64)
    B = o_all.shape[0]
    nb = (degree + 1) ** 2
    rgb, acc, dist = np.zeros((B, 3)), np.zeros(B), np.zeros(B)
    steps, fragile = np.zeros(B, np.int32), np.zeros(B, bool)
    for b in range(B):
        tn, tf = float(near[b]), float(far[b])
        ray = Ray(o_all[b], d_all[b], tn, tf, float(far_radius))
        if not ray.hit:
            rgb[b], acc[b], dist[b] = bg, 0.0, miss_distance(tn, tf)
            continue
        sm = ray.samples(s, max_steps)
        count = sm["w"].shape[0]
        if count and (ray.wb - sm["w"][-1]) / s < FRAGILE:
            fragile[b] = True
        if abs(ray.wa + 0.5 * s - ray.wb) / s < FRAGILE:
            fragile[b] = True
        if count < max_steps and (ray.wa + (count + 0.5) * s - ray.wb) / s < FRAGILE:
            fragile[b] = True
        u = (sm["z"] - lo) / h
        near_box = ((u > -FRAGILE) & (u < n - 1.0 + FRAGILE)).all(-1)
        if (near_box & (np.abs(u - np.round(u)) < FRAGILE).any(-1)).any():
            fragile[b] = True
        inside = ((sm["z"] >= lo) & (sm["z"] <= hi)).all(-1)
        idx = np.nonzero(inside)[0]
        uu = np.clip(u[idx], 0.0, n - 1.0)
        c = np.minimum(np.floor(uu).astype(np.int64), n - 2)
        f = uu - c
        if occupancy is not None and idx.size:
            keep = np.array([occupancy_bit(occupancy, int(a), int(bb), int(cc)) for a, bb, cc in c], bool)
            idx, c, f = idx[keep], c[keep], f[keep]
        Y = sh_basis(ray.u, degree)
        with np.errstate(invalid="ignore", over="ignore"):
            row = np.zeros((idx.size, rows64.shape[-1]))
            for dz in (0, 1):
                for dy in (0, 1):
                    for dx in (0, 1):
                        wgt = (f[:, 2] if dz else 1 - f[:, 2]) * (f[:, 1] if dy else 1 - f[:, 1]) * (f[:, 0] if dx else 1 - f[:, 0])
                        row += wgt[:, None] * rows64[c[:, 2] + dz, c[:, 1] + dy, c[:, 0] + dx]
            sigma = np.where(row[:, 0] < 0.0, 0.0, row[:, 0])                                    # a NaN stays a NaN
            colour = (row[:, 1:1 + 3 * nb].reshape(-1, nb, 3) * Y[None, :, None]).sum(1)
            colour = np.where(colour < 0.0, 0.0, np.where(colour > 1.0, 1.0, colour))
            alpha = 1.0 - np.exp(-sigma * sm["delta"][idx])
            after = np.cumprod(1.0 - alpha)
            stop = np.nonzero(after < t_min)[0]
            m = idx.size if stop.size == 0 else int(stop[0]) + 1
            before = np.concatenate([[1.0], after[:-1]])[:m] if idx.size else np.zeros(0)
            wgt = before * alpha[:m]
            a_sum, d_sum = wgt.sum(), (wgt * sm["t"][idx[:m]]).sum()
            rgb[b] = (wgt[:, None] * colour[:m]).sum(0) + (1.0 - a_sum) * bg
            acc[b] = a_sum
            if a_sum == 0.0:
                dist[b] = tn
            else:
                v = d_sum / a_sum
                dist[b] = v if np.isnan(v) else min(max(v, tn), tf)
        steps[b] = m
    return rgb, acc, dist, steps, fragile


# ---- the shared test scene: the smallest shapes at which the kernel can still go wrong ---------------------------------------------
DIMS = (9, 10, 11)                                  # (nx, ny, nz): all different, so an axis swap shows
LO = (-2.0, -1.9, -2.0)
HI = (2.0, 2.0, 1.8)                                # a non-cubic box of the contracted space with non-cubic cells; parts of |z| <= 2 lie outside
FAR_RADIUS = 8.0
N_SEEDED = 257
SEED = 5
P_FLAT = float(np.sqrt(2.0 + np.sqrt(5.0)))         # 2.058...: from this distance of the centre on, ts = 0 (c <= p2)


UNIT_E = np.array([0.6, -0.48, 0.64])                # a unit vector, and one perpendicular to it: a ray m + t e with m = p q has |m| = p
UNIT_Q = np.array([0.8, 0.6, -0.3]) / np.sqrt(1.09)


def random_rows(degree, seed=SEED, hollow=False):
    """random fp16 rows [nz, ny, nx, W]: sigma in [0, 4] with exact zeros (`hollow`: every point with x < 0 is zero as well, so an
    occupancy grid has clear cells), coefficients that put the colours on both sides of 0 and 1.  Returns (rows, the fp32 sigma)."""
    rng = np.random.default_rng(seed + 100 * degree)
    nx, ny, nz = DIMS
    sigma = rng.uniform(0.0, 4.0, (nz, ny, nx)).astype(np.float32)
    sigma[rng.uniform(size=sigma.shape) < 0.3] = 0.0
    if hollow:
        sigma[:, :, :nx // 2] = 0.0
    coef = rng.normal(0.0, 0.6, (nz, ny, nx, (degree + 1) ** 2, 3)).astype(np.float32)
    coef[..., 0, :] += np.float32(0.5 / 0.28209479177387814)
    return pack_rows(sigma, coef, degree), sigma


def fog_rows(degree, sigma=0.3, colour=(0.25, 0.5, 0.75)):
    """every row: the same density and a constant colour (the DC coefficient alone)"""
    nx, ny, nz = DIMS
    coef = np.zeros((nz, ny, nx, (degree + 1) ** 2, 3), np.float32)
    coef[..., 0, :] = np.asarray(colour, np.float32) / np.float32(0.28209479177387814)
    return pack_rows(np.full((nz, ny, nx), sigma, np.float32), coef, degree)


def occupancy_words(sigma, threshold=0.0):
    """the words of `ops.occupancy_grid` without dilation: a cell is occupied when one of its 8 corners exceeds the threshold"""
    nz, ny, nx = sigma.shape
    big = sigma > threshold
    cells = np.zeros((nz - 1, ny - 1, nx - 1), bool)
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                cells |= big[dz:dz + nz - 1, dy:dy + ny - 1, dx:dx + nx - 1]
    words = np.zeros((nz - 1, ny - 1, (nx - 1 + 31) // 32), np.uint32)
    for i in range(nx - 1):
        words[:, :, i >> 5] |= cells[:, :, i].astype(np.uint32) << np.uint32(i & 31)
    return words


def scene_rays(seed=SEED):
    """(origins, directions, near, far) float32.  257 seeded rays: origins at radii around 0.3, 0.9, 1, 3 and 6, a third aimed near the
    centre, |d| of 0.5, 1 and 2, far of 2, 30 and 1e3; then 13 hand-made rays: through the exact centre (p = 0), p just below and just
    above P_FLAT, p >= far_radius, near beyond the ball, and eight misses (a NaN origin, |d| = 0, a non-finite near, far <= near, a
    non-finite direction, a non-finite far, pointing away from outside the ball, far before the ball).  Directions are not normalised."""
    rng = np.random.default_rng(seed)
    o, d, tn, tf = [], [], [], []
    for k in range(N_SEEDED):
        sc = [0.3, 0.9, 1.0, 3.0, 6.0][k % 5]
        org = rng.normal(size=3)
        org *= sc / np.linalg.norm(org) * rng.uniform(0.5, 1.0)
        u = rng.normal(size=3)
        if k % 3 == 0:
            u = -org / np.linalg.norm(org) + 0.2 * rng.normal(size=3)
        u *= [0.5, 1.0, 2.0][(k // 3) % 3] / np.linalg.norm(u)
        o.append(org); d.append(u); tn.append(0.05); tf.append([2.0, 30.0, 1e3][k % 3])
    e, q = UNIT_E, UNIT_Q
    hand = [
        (-3.0 * e, 1.5 * e, 0.0, 1e3),                      # through the exact centre: p = 0
        ((P_FLAT - 1e-3) * q - 5.0 * e, e, 0.0, 1e3),       # ts barely positive
        ((P_FLAT + 1e-3) * q - 5.0 * e, e, 0.0, 1e3),       # ts = 0
        (8.5 * q - 5.0 * e, e, 0.0, 1e3),                   # p >= far_radius: a miss
        (-3.0 * e, e, 12.0, 1e3),                           # near beyond the ball: a miss
        ((np.nan, 0.2, 1.3), (0.9, -0.3, 0.45), 0.0, 9.0),
        ((0.1, 0.2, 1.3), (0.0, 0.0, 0.0), 0.0, 9.0),
        ((0.1, 0.2, 1.3), (0.9, -0.3, 0.45), np.inf, 9.0),
        ((0.1, 0.2, 1.3), (0.9, -0.3, 0.45), 2.0, 2.0),
        ((0.1, 0.2, 1.3), (0.9, np.inf, 0.45), 0.0, 9.0),
        ((0.1, 0.2, 1.3), (0.9, -0.3, 0.45), 0.0, np.inf),
        (9.0 * e, e, 0.0, 1e3),                             # outside the ball, pointing away
        (-12.0 * e, e, 0.0, 3.0),                           # outside the ball, far before it
    ]
    for a, b, c, f in hand:
        o.append(np.array(a, np.float64)); d.append(np.array(b, np.float64)); tn.append(c); tf.append(f)
    return (np.array(o, np.float32), np.array(d, np.float32), np.array(tn, np.float32), np.array(tf, np.float32))


N_RAYS = N_SEEDED + 13                              # ragged: 67 blocks of 4 rays and one of 2
