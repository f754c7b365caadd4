"""Rules P1 - P7 of include/mipnerf_preview_mip.h restated in numpy float64, for test_preview_mip_cpu.py and test_gpu_preview_mip.py.
The fixture is given every level's fp16 rows as they are.  It marches all rays together, one sample index after the other (so that the
6 x 6 supersampled picture of the anti-aliasing scene costs a second, not a minute); it knows nothing of wavefronts, blocks or level
walks.  The packing, the basis, the occupancy bit and the rays are preview_fixture's.

FRAGILE rays are those on which fp32 arithmetic may legitimately differ: preview_fixture's two conditions -- a lattice coordinate within
1e-4 of an integer, on every level the sample actually reads, and a last sample at the interval's end -- and one more:
    - |w - s_l| < 1e-4 s_l for some level l: there the test g > 0 flips, and with it the levels a sample reads and P5's OR.

REGIMES: `march` counts the samples that exist (occupied or not, before the early stop ends the ray) by regime 2 l + (g > 0): for three
levels 0 = `w <= s_0`, 1 = a blend of levels 0 / 1, 2 = level 1 alone (w == s_1 exactly), 3 = a blend of levels 1 / 2, 4 = `w >= s_2`."""
import functools

import numpy as np

import preview_fixture as pf

FRAGILE = pf.FRAGILE
F = np.float32


def spacing(dims, lo, hi):
    """s_l of P1 as the float32 number the library forms: min over the axes of the fp32 (hi - lo) / float(n - 1)"""
    return float(((np.asarray(hi, F) - np.asarray(lo, F)) / (np.asarray(dims) - 1).astype(F)).min())


def select_level(w, s):
    """P4 on arrays: (l, g) of footprints w for the spacings s"""
    L = len(s)
    l = np.zeros(w.shape, np.int64)
    g = np.zeros(w.shape)
    if L == 1:
        return l, g
    top = w >= s[-1]
    inner = (w > s[0]) & ~top
    l[top] = L - 1
    for j in range(L - 1):
        l[inner & (s[j] <= w)] = j
    sl, sn = np.asarray(s)[l], np.asarray(s)[np.minimum(l + 1, L - 1)]
    g[inner] = ((w - sl) / np.where(inner, sn - sl, 1.0))[inner]
    return l, g


def _gather(rows64, n, lo, h, x, words):
    """the cell rule, the occupancy bit and the trilinear row of points x [M, 3] on one level: (row [M, W], bit [M], near_face [M])"""
    u = np.clip((x - lo) / h, 0.0, n - 1.0)
    near_face = (np.abs(u - np.round(u)) < FRAGILE).any(-1)
    c = np.minimum(np.floor(u).astype(np.int64), n - 2)
    f = u - c
    if words is None:
        bit = np.ones(len(x), bool)
    else:
        bit = ((words[c[:, 2], c[:, 1], c[:, 0] >> 5].astype(np.int64) >> (c[:, 0] & 31)) & 1).astype(bool)
    row = np.zeros((len(x), rows64.shape[-1]))
    with np.errstate(invalid="ignore"):
        for dz in (0, 1):
            for dy in (0, 1):
                for dx in (0, 1):
                    wgt = (f[:, 2] if dz else 1 - f[:, 2]) * (f[:, 1] if dy else 1 - f[:, 1]) * (f[:, 0] if dx else 1 - f[:, 0])
                    row += wgt[:, None] * rows64[c[:, 2] + dz, c[:, 1] + dy, c[:, 0] + dx]
    return row, bit, near_face


def march(levels, lo, hi, degree, origins, directions, radii, near, far, footprint, step_scale, t_min, max_steps, background,
          occupancy=None):
    """P1 - P6 in float64: (rgb [B, 3], acc [B], distance [B], steps [B] int32, lod [B], fragile [B] bool, regimes [2 L - 1] int64).
    levels: the fp16 rows [nz, ny, nx, W] of every level, finest first; lo / hi: the box as the float32 values the library is given;
    occupancy: None, or one entry per level (uint32 words or None); footprint: rounded to float32, as the C argument is."""
    L = len(levels)
    rows64 = [np.asarray(r).astype(np.float64) for r in levels]
    dims = [np.array([r.shape[2], r.shape[1], r.shape[0]]) for r in rows64]
    occupancy = [None] * L if occupancy is None else list(occupancy)
    s_l = [spacing(n, lo, hi) for n in dims]
    assert all(a < b for a, b in zip(s_l, s_l[1:])), s_l
    lo = np.asarray(lo, F).astype(np.float64)
    hi = np.asarray(hi, F).astype(np.float64)
    h_l = [(hi - lo) / (n - 1) for n in dims]
    s = float(F(step_scale) * F(s_l[0]))                    # P2: the step is a float32 number
    bg = np.asarray(background, np.float64)
    o, d = np.asarray(origins, np.float64), np.asarray(directions, np.float64)
    tn, tf, rad = np.asarray(near, np.float64), np.asarray(far, np.float64), np.asarray(radii, np.float64)
    B = o.shape[0]
    nb = (degree + 1) ** 2
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        ok = np.isfinite(o).all(-1) & np.isfinite(d).all(-1) & np.isfinite(tn) & np.isfinite(tf) & (tf > tn) & np.isfinite(rad) & ~(rad < 0)
        ta, tb = tn.copy(), tf.copy()
        for a in range(3):
            zero = d[:, a] == 0.0
            ok &= ~zero | ((lo[a] <= o[:, a]) & (o[:, a] <= hi[a]))
            t0, t1 = (lo[a] - o[:, a]) / d[:, a], (hi[a] - o[:, a]) / d[:, a]
            ta = np.where(zero, ta, np.maximum(ta, np.minimum(t0, t1)))
            tb = np.where(zero, tb, np.minimum(tb, np.maximum(t0, t1)))
        length = np.sqrt((d * d).sum(-1))
        ok &= (length > 0.0) & (ta < tb)
        ok &= np.isfinite(length)
        dt = s / length
        Y = pf.sh_basis(d / length[:, None], degree)
        k = float(F(footprint)) * rad
        q = (tb - ta) / dt - 0.5
        fragile = ok & (np.abs(q - np.round(q)) < FRAGILE)
    T, c_sum, a_sum, d_sum, l_sum = np.ones(B), np.zeros((B, 3)), np.zeros(B), np.zeros(B), np.zeros(B)
    steps = np.zeros(B, np.int32)
    regimes = np.zeros(2 * L - 1, np.int64)
    alive = ok.copy()
    for i in range(max_steps):
        with np.errstate(invalid="ignore"):
            t_all = ta + (i + 0.5) * dt
            alive &= t_all < tb
        idx = np.flatnonzero(alive)
        if idx.size == 0:
            break
        t = t_all[idx]
        x = o[idx] + t[:, None] * d[idx]
        w = k[idx] * t
        l, g = select_level(w, s_l)
        if L > 1:
            fragile[idx] |= (np.abs(w[:, None] - np.array(s_l)) < FRAGILE * np.array(s_l)).any(-1)
        np.add.at(regimes, 2 * l + (g > 0), 1)
        bit = np.zeros(idx.size, bool)
        row = np.zeros((idx.size, rows64[0].shape[-1]))
        for lv in range(L):                                   # ascending: a sample's own level before the one mixed in
            lower, upper = l == lv, (g > 0) & (l + 1 == lv)
            m = lower | upper
            if not m.any():
                continue
            got, b, near_face = _gather(rows64[lv], dims[lv], lo, h_l[lv], x[m], occupancy[lv])
            fragile[idx[m]] |= near_face
            bit[m] |= b
            with np.errstate(invalid="ignore"):
                gm = g[m][:, None]
                row[m] = np.where(lower[m][:, None], got, (1.0 - gm) * row[m] + gm * got)
        n_occ = int(bit.sum())
        if n_occ:
            j, r = idx[bit], row[bit]
            with np.errstate(invalid="ignore"):
                sigma = np.where(r[:, 0] < 0.0, 0.0, r[:, 0])                                # a NaN stays a NaN
                colour = (r[:, 1:1 + 3 * nb].reshape(-1, nb, 3) * Y[j][:, :, None]).sum(1)
                colour = np.where(colour < 0.0, 0.0, np.where(colour > 1.0, 1.0, colour))
                alpha = 1.0 - np.exp(-sigma * s)
                wt = T[j] * alpha
                c_sum[j] += wt[:, None] * colour
                a_sum[j] += wt
                d_sum[j] += wt * t[bit]
                l_sum[j] += wt * (l[bit] + g[bit])
                T[j] = T[j] * (1.0 - alpha)
                steps[j] += 1
                alive[j[T[j] < t_min]] = False
    with np.errstate(invalid="ignore", divide="ignore"):
        rgb = c_sum + (1.0 - a_sum)[:, None] * bg
        v = d_sum / a_sum
        dist = np.where(a_sum == 0.0, tn, np.where(np.isnan(v), v, np.minimum(np.maximum(v, tn), tf)))
        lod = np.where(a_sum == 0.0, 0.0, l_sum / a_sum)
    miss = ~ok
    rgb[miss], dist[miss] = bg, [pf.miss_distance(a, b) for a, b in zip(tn[miss], tf[miss])]
    return rgb, a_sum, dist, steps, lod, fragile, regimes


# ---- the shared test scene: the smallest shapes at which the kernel can still go wrong ---------------------------------------------
LEVEL_DIMS = ((8, 9, 10), (5, 5, 6), (3, 3, 4))          # s_l = 0.21875, 0.4375, 0.75 over pf.LO .. pf.HI
FOOTPRINT = float(np.sqrt(3.0))
SEED = 23


def random_level(dims, degree, seed, opaque=False, hollow=False):
    """preview_fixture.random_rows at other dims: every level has its OWN content (not a filtered copy), so a level mix-up shows"""
    rng = np.random.default_rng(seed + 100 * degree)
    nx, ny, nz = dims
    sigma = rng.uniform(20.0 if opaque else 0.0, 50.0, (nz, ny, nx)).astype(F)
    if not opaque:
        sigma[rng.uniform(size=sigma.shape) < 0.3] = 0.0
    if hollow:
        sigma[:, :, :nx // 2] = 0.0
    coef = rng.normal(0.0, 0.6, (nz, ny, nx, (degree + 1) ** 2, 3)).astype(F)
    coef[..., 0, :] += F(0.5 / pf.C0)
    return pf.pack_rows(sigma, coef, degree), sigma


def scene_levels(degree, **kw):
    """[(rows, sigma)] of the three levels; level 0 is preview_fixture.random_rows itself"""
    return [pf.random_rows(degree, **kw)] + [random_level(dims, degree, SEED + 7 * i, **kw) for i, dims in enumerate(LEVEL_DIMS[1:], 1)]


def scene_radii(seed=SEED):
    """seeded log-uniform radii over [0.005, 0.6] for the 257 rays of preview_fixture.scene_rays: with footprint sqrt(3) and t of 1 .. 8
    the footprints w = footprint * radius * t spread over all four regimes of the three spacings"""
    rng = np.random.default_rng(seed)
    return np.exp(rng.uniform(np.log(0.005), np.log(0.6), pf.N_RAYS)).astype(F)


def cell_occupancy(sigma, threshold):
    """uint32 words [nz - 1, ny - 1, ceil((nx - 1) / 32)]: a cell is occupied when one of its 8 corners exceeds the threshold"""
    nz, ny, nx = sigma.shape
    above = sigma > threshold
    cells = np.zeros((nz - 1, ny - 1, nx - 1), bool)
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                cells |= above[dz:dz + nz - 1, dy:dy + ny - 1, dx:dx + nx - 1]
    words = np.zeros((nz - 1, ny - 1, (nx - 1 + 31) // 32), np.uint32)
    for i in range(nx - 1):
        words[:, :, i >> 5] |= cells[:, :, i].astype(np.uint32) << np.uint32(i & 31)
    return words


# ---- the anti-aliasing scene ---------------------------------------------------------------------------------------------------------
AA_DIMS = ((33, 33, 33), (17, 17, 17), (9, 9, 9))
AA_LO, AA_HI = (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)
AA_SIGMA = 3.0
AA_WAVELENGTH = 3.0 * 2.0 / 32.0                       # 3 cells of the finest lattice
AA_EYE_Z = 9.0
AA_WIDTH = 0.148                                         # 2 tan(fov / 2): 24 pixels of 0.148 / 24 * 10 = 0.0617 < s_0 = 0.0625 at the far face


def aa_levels():
    """degree-0 rows of the three lattices: constant density, red a plane-wave sinusoid of wavelength 3 fine cells along (1, 1, 0) /
    sqrt(2) and green one along (1, -1, 0) / sqrt(2), EACH LEVEL PRE-FILTERED BY ITS OWN LATTICE GAUSSIAN (variance h^2 / 12 per axis),
    which is what `bake_field` does through the integrated encoding: a sinusoid of wavelength lam keeps exp(-2 pi^2 (h^2 / 12) / lam^2)
    of its amplitude.  The waves run along the image diagonals, so their wavelength PER LATTICE AXIS is 3 sqrt(2) = 4.24 fine cells =
    2.12 cells of level 1: level 1 still samples them above its own Nyquist rate.  (Along an axis the same wave would have 1.5 cells of
    level 1 per period and the h^2 / 12 filter leaves 48 % of it: level 1 would hold an alias, not a pre-filtered wave.  The wider
    pre-filter that cures that is not part of the pyramid, see the README's "Not done".)"""
    out = []
    for n in AA_DIMS:
        nx = n[0]
        h = 2.0 / (nx - 1)
        keep = np.exp(-2.0 * np.pi ** 2 * (h * h / 12.0) / AA_WAVELENGTH ** 2)
        p = -1.0 + h * np.arange(nx)
        x, y = p[None, None, :], p[None, :, None]
        coef = np.zeros((nx, nx, nx, 1, 3), F)
        coef[..., 0, 0] = (0.5 + 0.4 * keep * np.sin(2.0 * np.pi * (x + y) / np.sqrt(2.0) / AA_WAVELENGTH)) / pf.C0
        coef[..., 0, 1] = (0.5 + 0.4 * keep * np.sin(2.0 * np.pi * (x - y) / np.sqrt(2.0) / AA_WAVELENGTH)) / pf.C0
        coef[..., 0, 2] = 0.5 / pf.C0
        out.append(pf.pack_rows(np.full((nx, nx, nx), AA_SIGMA, F), coef, 0))
    return out


def aa_rays(res, sub=1):
    """a pinhole camera on the z axis looking down -z at the box: res x res pixels, each split into sub x sub rays (pixel-major); radii =
    the PIXEL's dx / sqrt(3) whatever `sub`, so footprint sqrt(3) makes w one pixel's width.  (origins, directions, radii, near, far) float32"""
    m = res * sub
    c = ((np.arange(m) + 0.5) / m - 0.5) * AA_WIDTH
    py, px = np.meshgrid(c, c, indexing="ij")
    pix = lambda a: a.reshape(res, sub, res, sub).transpose(0, 2, 1, 3).reshape(-1)
    d = np.stack([pix(px), pix(py), -np.ones(m * m)], -1).astype(F)
    o = np.broadcast_to(np.array([0.0, 0.0, AA_EYE_Z], F), d.shape).copy()
    n = d.shape[0]
    return o, d, np.full(n, AA_WIDTH / res / np.sqrt(3.0), F), np.full(n, 0.5, F), np.full(n, 20.0, F)


def aa_march(res, sub=1, mip=True, step_scale=0.5):
    """the float64 picture [res * res, 3] of the scene: the pyramid, or the plain march of level 0 (L = 1); `sub` > 1: the mean over each
    pixel's sub x sub rays"""
    o, d, rad, tn, tf = aa_rays(res, sub)
    levels = aa_levels()
    rgb = march(levels if mip else levels[:1], AA_LO, AA_HI, 0, o, d, rad, tn, tf, FOOTPRINT, step_scale, 0.0, 4096, (1.0, 1.0, 1.0))[0]
    return rgb.reshape(res * res, sub * sub, 3).mean(1)


@functools.lru_cache(maxsize=None)
def aa_truth(res):
    """the 6 x 6 supersampled plain march, computed once per resolution and shared"""
    out = aa_march(res, sub=6, mip=False)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def aa_reference(res):
    """(MSE of the plain march, MSE of the pyramid) against the truth, in float64"""
    truth = aa_truth(res)
    return tuple(float(((aa_march(res, mip=m) - truth) ** 2).mean()) for m in (False, True))
