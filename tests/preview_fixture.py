"""The row layout and the marching rules of include/mipnerf_preview.h restated in numpy float64, for test_preview_cpu.py and
test_gpu_preview.py.  The fixture is given the fp16 rows as they are and marches one ray after the other, one sample after the other:
it knows nothing of wavefronts or blocks.  It also says which rays are FRAGILE -- rays on which fp32 arithmetic may legitimately land a
sample in another cell or gain / lose a sample:
    - some sample lies within 1e-4 h of a cell face on some axis, or
    - (tb - ta) / dt - 0.5 lies within 1e-4 of an integer (the last sample sits at the interval's end)."""
import numpy as np

C0 = 0.28209479177387814
C1 = 0.4886025119029199
C2 = (1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396)
ROW_HALVES = {0: 4, 1: 16, 2: 32}
FRAGILE = 1e-4


def sh_basis(dirs, degree):
    """[..., (degree + 1)^2] float64 of unit directions [..., 3], PlenOctrees' order and signs"""
    d = np.asarray(dirs, np.float64)
    x, y, z = d[..., 0], d[..., 1], d[..., 2]
    out = [np.full(x.shape, C0)]
    if degree >= 1:
        out += [-C1 * y, C1 * z, -C1 * x]
    if degree >= 2:
        out += [C2[0] * x * y, C2[1] * y * z, C2[2] * (2 * z * z - x * x - y * y), C2[3] * x * z, C2[4] * (x * x - y * y)]
    return np.stack(out, -1)


def pack_rows(sigma, coef, degree, mask=None):
    """fp16 rows [nz, ny, nx, W] of sigma [nz, ny, nx] and coef [nz, ny, nx, (degree + 1)^2, 3] (float32): numpy's round-to-nearest-even
    cast, sigma saturated at the fp16 maximum, the coefficients of masked-out points zero"""
    sigma = np.asarray(sigma, np.float32)
    coef = np.asarray(coef, np.float32).reshape(sigma.shape + (-1,))
    rows = np.zeros(sigma.shape + (ROW_HALVES[degree],), np.float16)
    with np.errstate(over="ignore", invalid="ignore"):
        rows[..., 0] = np.where(sigma > 65504.0, np.float32(65504.0), sigma).astype(np.float16)
        c = coef.astype(np.float16)
    if mask is not None:
        c = np.where(np.asarray(mask).astype(bool)[..., None], c, np.float16(0))
    rows[..., 1:1 + c.shape[-1]] = c
    return rows


def occupancy_bit(words, cx, cy, cz):
    """bit of cell (cx, cy, cz) in the word layout of ops.Occupancy: [nz - 1, ny - 1, ceil((nx - 1) / 32)]"""
    return bool((int(words[cz, cy, cx >> 5]) >> (cx & 31)) & 1)


def miss_distance(near, far):
    return near if np.isfinite(near) else (far if np.isfinite(far) else 0.0)


def march(rows, lo, hi, degree, origins, directions, near, far, step_scale, t_min, max_steps, background, occupancy=None):
    """rules 1 - 6 in float64: (rgb [B, 3], acc [B], distance [B], steps [B] int32, fragile [B] bool).  rows: fp16 [nz, ny, nx, W];
    lo / hi: the box as the float32 values the library is given; occupancy: uint32 words or None."""
    rows64 = np.asarray(rows).astype(np.float64)
    nz, ny, nx, _ = rows64.shape
    n = np.array([nx, ny, nz])
    lo = np.asarray(lo, np.float32).astype(np.float64)
    hi = np.asarray(hi, np.float32).astype(np.float64)
    # rule 1 with the library's fp32 h (the lattice is DEFINED by float32 lo, hi): the step is a float32 number
    h32 = (np.asarray(hi, np.float32) - np.asarray(lo, np.float32)) / (n - 1).astype(np.float32)
    s = float(np.float32(step_scale) * h32.min())
    h = (hi - lo) / (n - 1)
    bg = np.asarray(background, np.float64)
    o_all, d_all = np.asarray(origins, np.float64), np.asarray(directions, np.float64)
    B = o_all.shape[0]
    nb = (degree + 1) ** 2
    rgb, acc, dist = np.zeros((B, 3)), np.zeros(B), np.zeros(B)
    steps, fragile = np.zeros(B, np.int32), np.zeros(B, bool)
    for b in range(B):
        o, d, tn, tf = o_all[b], d_all[b], float(near[b]), float(far[b])
        miss = not (np.isfinite(o).all() and np.isfinite(d).all() and np.isfinite(tn) and np.isfinite(tf) and tf > tn)
        ta, tb = tn, tf
        if not miss:
            for a in range(3):
                if d[a] == 0.0:
                    miss = miss or not (lo[a] <= o[a] <= hi[a])
                else:
                    t0, t1 = (lo[a] - o[a]) / d[a], (hi[a] - o[a]) / d[a]
                    ta, tb = max(ta, min(t0, t1)), min(tb, max(t0, t1))
            length = float(np.sqrt((d * d).sum()))
            miss = miss or not length > 0.0 or not ta < tb
        if miss:
            rgb[b], acc[b], dist[b] = bg, 0.0, miss_distance(tn, tf)
            continue          # (a ray that only just hits has no sample either: t_0 = ta + dt / 2 lies beyond tb, and the outputs are the same)
        dt = s / length
        Y = sh_basis(d / length, degree)
        q = (tb - ta) / dt - 0.5
        if abs(q - round(q)) < FRAGILE:
            fragile[b] = True
        T, c_sum, a_sum, d_sum, count = 1.0, np.zeros(3), 0.0, 0.0, 0
        i = 0
        while i < max_steps:
            t = ta + (i + 0.5) * dt
            if not t < tb:
                break
            u = np.clip((o + t * d - lo) / h, 0.0, n - 1.0)
            if (np.abs(u - np.round(u)) < FRAGILE).any():
                fragile[b] = True
            c = np.minimum(np.floor(u).astype(np.int64), n - 2)
            f = u - c
            i += 1
            if occupancy is not None and not occupancy_bit(occupancy, int(c[0]), int(c[1]), int(c[2])):
                continue
            cell = rows64[c[2]:c[2] + 2, c[1]:c[1] + 2, c[0]:c[0] + 2]                     # [z, y, x, W]
            wz, wy, wx = np.array([1 - f[2], f[2]]), np.array([1 - f[1], f[1]]), np.array([1 - f[0], f[0]])
            with np.errstate(invalid="ignore"):
                row = np.einsum("zyxw,z,y,x->w", cell, wz, wy, wx)
                sigma = row[0] if not row[0] < 0.0 else 0.0
                colour = (row[1:1 + 3 * nb].reshape(nb, 3) * Y[:, None]).sum(0)
                colour = np.where(colour < 0.0, 0.0, np.where(colour > 1.0, 1.0, colour))        # a NaN stays a NaN
                alpha = 1.0 - np.exp(-sigma * s)
                w = T * alpha
                c_sum, a_sum, d_sum = c_sum + w * colour, a_sum + w, d_sum + w * t
                T = T * (1.0 - alpha)
            count += 1
            if T < t_min:
                break
        with np.errstate(invalid="ignore"):
            rgb[b] = c_sum + (1.0 - a_sum) * bg
            acc[b] = a_sum
            if a_sum == 0.0:
                dist[b] = tn
            else:
                v = d_sum / a_sum
                dist[b] = v if np.isnan(v) else min(max(v, tn), tf)
        steps[b] = count
    return rgb, acc, dist, steps, fragile


# ---- the shared test scene: the smallest shapes at which the kernel can still go wrong ---------------------------------------------
DIMS = (8, 9, 10)                                   # (nx, ny, nz): all different, so an axis swap shows
LO = (-1.25, -0.75, 0.125)
HI = (1.5, 1.0, 2.375)                              # a non-cubic box with non-cubic cells
N_RAYS = 257                                        # ragged: 64 blocks of 4 rays and one of 1
SEED = 11


def random_rows(degree, seed=SEED, opaque=False, hollow=False):
    """random fp16 rows [nz, ny, nx, W]: sigma in [0, 50] with exact zeros (`opaque`: in [20, 50], none zero; `hollow`: the low-x half of
    the box is all zeros as well, so an occupancy grid has clear cells), coefficients that put the colours on both sides of 0 and 1.
    Returns (rows, the fp32 sigma lattice before its fp16 rounding)."""
    rng = np.random.default_rng(seed + 100 * degree)
    nx, ny, nz = DIMS
    sigma = rng.uniform(20.0 if opaque else 0.0, 50.0, (nz, ny, nx)).astype(np.float32)
    if not opaque:
        sigma[rng.uniform(size=sigma.shape) < 0.3] = 0.0
    if hollow:
        sigma[:, :, :nx // 2] = 0.0
    coef = rng.normal(0.0, 0.6, (nz, ny, nx, (degree + 1) ** 2, 3)).astype(np.float32)
    coef[..., 0, :] += np.float32(0.5 / C0)
    return pack_rows(sigma, coef, degree), sigma


def scene_rays(seed=SEED):
    """(origins [257, 3], directions [257, 3], near [257], far [257]) float32: two cameras outside the box, one inside, and hand-made
    rays (the last 17): axis-parallel with zero components, grazing a face, starting inside, near beyond the box, far before it, a NaN
    origin, |d| = 0, a non-finite near, far <= near.  Directions are not normalised."""
    rng = np.random.default_rng(seed)
    lo, hi = np.array(LO), np.array(HI)
    mid = 0.5 * (lo + hi)
    o, d, tn, tf = [], [], [], []
    for eye, count in ((mid + np.array([4.0, 2.5, 3.0]), 100), (mid + np.array([-3.0, 3.5, -2.0]), 100), (mid + np.array([0.31, -0.17, 0.23]), 40)):
        target = rng.uniform(lo - 0.3, hi + 0.3, (count, 3))
        v = target - eye
        v *= rng.uniform(0.4, 1.6, (count, 1)) / np.linalg.norm(v, axis=-1, keepdims=True)
        o += [eye] * count
        d += list(v)
        tn += [0.05] * count
        tf += [25.0] * count
    hand = [
        ((lo[0] - 1.0, 0.173, 1.211), (1.0, 0.0, 0.0), 0.0, 9.0),            # axis-parallel, two zero components
        ((0.411, hi[1] + 2.0, 0.877), (0.0, -2.0, 0.0), 0.0, 9.0),
        ((-0.613, 0.291, lo[2] - 0.5), (0.0, 0.0, 0.5), 0.1, 30.0),
        ((0.377, 0.119, 1.003), (0.0, 0.7, -0.4), 0.0, 9.0),                 # one zero component, starts inside
        ((lo[0] - 1.0, 0.173, hi[2]), (1.0, 0.0, 0.0), 0.0, 9.0),            # grazing: in the plane of the z = hi face
        ((lo[0], lo[1] - 1.0, 1.0), (0.0, 1.0, 0.0), 0.0, 9.0),              # grazing: in the plane of the x = lo face
        ((lo[0] - 1.0, 0.173, hi[2] + 1e-3), (1.0, 0.0, 0.0), 0.0, 9.0),     # parallel to a face, just outside: a miss
        ((0.1, 0.2, 1.3), (0.9, -0.3, 0.45), 0.0, 9.0),                      # starts inside
        ((0.1, 0.2, 1.3), (0.9, -0.3, 0.45), 0.2, 0.9),                      # starts and ends inside
        ((mid[0] + 4.0, mid[1] + 2.5, mid[2] + 3.0), (-4.0, -2.5, -3.0), 3.0, 9.0),      # near beyond the box
        ((mid[0] + 4.0, mid[1] + 2.5, mid[2] + 3.0), (-4.0, -2.5, -3.0), 0.0, 0.2),      # far before it
        ((mid[0] + 4.0, mid[1] + 2.5, mid[2] + 3.0), (4.0, 2.5, 3.0), 0.0, 9.0),         # pointing away
        ((np.nan, 0.2, 1.3), (0.9, -0.3, 0.45), 0.0, 9.0),                   # a NaN origin
        ((0.1, 0.2, 1.3), (0.0, 0.0, 0.0), 0.0, 9.0),                        # |d| = 0
        ((0.1, 0.2, 1.3), (0.9, -0.3, 0.45), np.inf, 9.0),                   # a non-finite near
        ((0.1, 0.2, 1.3), (0.9, -0.3, 0.45), 2.0, 2.0),                      # far <= near
        ((0.1, 0.2, 1.3), (0.9, np.inf, 0.45), 0.0, 9.0),                    # a non-finite direction
    ]
    for a, b, c, e in hand:
        o.append(np.array(a)); d.append(np.array(b)); tn.append(c); tf.append(e)
    out = (np.array(o, np.float32), np.array(d, np.float32), np.array(tn, np.float32), np.array(tf, np.float32))
    assert out[0].shape == (N_RAYS, 3)
    return out
