"""Rules 8 - 10 of include/mipnerf_preview_tune.h (the gradient of the baked preview's march with respect to its rows) and the Adam rule,
restated in numpy on top of preview_fixture, for test_preview_tune_cpu.py and test_gpu_preview_tune.py.  One ray after the other; the
samples of a ray as arrays; S_i accumulated in reverse.  The fixture knows nothing of wavefronts, blocks, lanes or atomics.

`march_grad(..., dtype=np.float64)` is the reference.  The same function with dtype=np.float32 is WHAT FP32 ARITHMETIC DOES TO THESE
FORMULAS, independent of the code under test: the gradient tolerance of both test files is measured as the scaled distance of the two.
It runs on the rays it is given (the tests give it the non-fragile ones: on a fragile ray a sample may legitimately land in another
cell)."""
import numpy as np

import preview_fixture as pf

USED = {0: 4, 1: 13, 2: 28}              # 1 + 3 (degree + 1)^2: the entries of a row that are not padding
SIGMA_SCALE = 0.2                        # random_rows' sigma times this: rays are not all opaque after three samples


def scene_rows(degree, hollow=False, seed=pf.SEED):
    """`preview_fixture.random_rows` with sigma multiplied by SIGMA_SCALE (fp16 [nz, ny, nx, W])"""
    rows, _ = pf.random_rows(degree, seed=seed, hollow=hollow)
    rows = rows.copy()
    rows[..., 0] = (rows[..., 0].astype(np.float32) * np.float32(SIGMA_SCALE)).astype(np.float16)
    return rows


def smooth_rows(degree, seed=pf.SEED):
    """A variant without kinks inside a finite-difference step: sigma in [0.5, 10], and coefficients so small around a DC term of colour
    0.5 that every colour before its clamp stays inside [0.05, 0.95] for every direction (the tests assert it)."""
    rng = np.random.default_rng(seed + 1000 * (degree + 1))
    nx, ny, nz = pf.DIMS
    nb = (degree + 1) ** 2
    sigma = rng.uniform(0.5, 10.0, (nz, ny, nx)).astype(np.float32)
    coef = rng.uniform(-0.02, 0.02, (nz, ny, nx, nb, 3)).astype(np.float32)
    coef[..., 0, :] = (0.5 + rng.uniform(-0.2, 0.2, (nz, ny, nx, 3))).astype(np.float32) / np.float32(pf.C0)
    return pf.pack_rows(sigma, coef, degree)


def cell_words(cells):
    """occupancy words [nz - 1, ny - 1, ceil((nx - 1) / 32)] of bool cells [nz - 1, ny - 1, nx - 1]"""
    cz, cy, cx = cells.shape
    words = np.zeros((cz, cy, (cx + 31) // 32), np.uint32)
    for i in range(cx):
        words[..., i >> 5] |= cells[..., i].astype(np.uint32) << np.uint32(i & 31)
    return words


def occupancy_of(rows, threshold=0.0):
    """a cell is occupied when one of its 8 corners has sigma > threshold"""
    s = rows[..., 0].astype(np.float32) > threshold
    cells = np.zeros((s.shape[0] - 1, s.shape[1] - 1, s.shape[2] - 1), bool)
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                cells |= s[dz:dz + cells.shape[0], dy:dy + cells.shape[1], dx:dx + cells.shape[2]]
    return cell_words(cells)


def basis(u, degree, D):
    """`preview_fixture.sh_basis` of one unit direction with every operation in dtype D"""
    x, y, z = (D(v) for v in u)
    out = [D(pf.C0)]
    if degree >= 1:
        out += [-D(pf.C1) * y, D(pf.C1) * z, -D(pf.C1) * x]
    if degree >= 2:
        out += [D(pf.C2[0]) * x * y, D(pf.C2[1]) * y * z, D(pf.C2[2]) * (D(2.0) * z * z - x * x - y * y), D(pf.C2[3]) * x * z,
                D(pf.C2[4]) * (x * x - y * y)]
    return np.array(out, D)


def march_grad(rows, lo, hi, degree, origins, directions, near, far, step_scale, t_min, max_steps, background, occupancy=None,
               grad_rgb=None, grad_acc=None, target=None, loss_scale=None, rays=None, dtype=np.float64):
    """Forward (rules 1 - 5) and backward (rules 8 - 10) of the rays with indices `rays` (default: all), every operation in `dtype`.
    Exactly one of grad_rgb [B, 3] and (target [B, 3], loss_scale).  Returns a dict:
        grad   [nz, ny, nx, W] dtype    the gradient
        A      [nz, ny, nx, W] dtype    per entry, the sum of the absolute values of every term that enters it; for the density entry of a
                                        sample, s (|T_{i+1} q_i| + sum_j |w_j q_j|) over the whole ray, times the corner weight
        count  [nz, ny, nx, W] int64    the number of terms with a non-zero absolute value
        rgb [B, 3], acc [B], steps [B]  the march's outputs (NaN / -1 for rays not in `rays`)
        cells  per ray the list of flat cell indices of its counted samples, in order (for run counting)
        v_range  (min, max) of the colours before their clamp over all counted samples"""
    D = dtype
    assert (grad_rgb is None) != (target is None)
    rows_d = np.asarray(rows).astype(D)
    nz, ny, nx, W = rows_d.shape
    n = np.array([nx, ny, nz])
    lo32, hi32 = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
    h32 = (hi32 - lo32) / (n - 1).astype(np.float32)
    s = D(np.float32(step_scale) * h32.min())                    # the library's float32 step
    lo_d, hi_d = lo32.astype(D), hi32.astype(D)
    h = (hi_d - lo_d) / (n - 1).astype(D)
    top = (n - 1).astype(D)
    bg = np.asarray(background, D)
    nb = (degree + 1) ** 2
    B = origins.shape[0]
    grad, A = np.zeros(rows_d.shape, D), np.zeros(rows_d.shape, D)
    count = np.zeros(rows_d.shape, np.int64)
    rgb, acc, steps = np.full((B, 3), np.nan, D), np.full(B, np.nan, D), np.full(B, -1, np.int64)
    cells_of = {}
    v_lo, v_hi = np.inf, -np.inf
    one, zero, half = D(1.0), D(0.0), D(0.5)
    for b in (range(B) if rays is None else rays):
        b = int(b)
        o, d, tn, tf = np.asarray(origins[b], D), np.asarray(directions[b], D), D(near[b]), D(far[b])
        miss = not (np.isfinite(o).all() and np.isfinite(d).all() and np.isfinite(tn) and np.isfinite(tf) and tf > tn)
        ta, tb = tn, tf
        if not miss:
            for a in range(3):
                if d[a] == 0.0:
                    miss = miss or not (lo_d[a] <= o[a] <= hi_d[a])
                else:
                    t0, t1 = (lo_d[a] - o[a]) / d[a], (hi_d[a] - o[a]) / d[a]
                    ta, tb = max(ta, min(t0, t1)), min(tb, max(t0, t1))
            length = np.sqrt((d * d).sum(dtype=D))
            miss = miss or not length > 0.0 or not ta < tb
        if miss:
            rgb[b], acc[b], steps[b] = bg, 0.0, 0
            cells_of[b] = []
            continue
        dt = s / length
        Y = basis(d / length, degree, D)
        imax = int(min(max_steps, np.ceil(float(tb - ta) / float(dt)) + 2))
        t = ta + (np.arange(imax).astype(D) + half) * dt
        t = t[t < tb]
        u = np.clip((o[None, :] + t[:, None] * d[None, :] - lo_d) / h, zero, top)
        c = np.minimum(np.floor(u).astype(np.int64), n - 2)
        f = u - c.astype(D)
        if occupancy is not None:
            bits = (occupancy[c[:, 2], c[:, 1], c[:, 0] >> 5].astype(np.int64) >> (c[:, 0] & 31)) & 1
            c, f = c[bits == 1], f[bits == 1]
        m = c.shape[0]
        with np.errstate(invalid="ignore", over="ignore"):
            corner = np.stack([np.stack([np.stack([rows_d[c[:, 2] + dz, c[:, 1] + dy, c[:, 0] + dx] for dx in (0, 1)], 1) for dy in (0, 1)], 1)
                               for dz in (0, 1)], 1)                                          # [m, z, y, x, W]
            wx, wy, wz = np.stack([one - f[:, 0], f[:, 0]], 1), np.stack([one - f[:, 1], f[:, 1]], 1), np.stack([one - f[:, 2], f[:, 2]], 1)
            wts = (wz[:, :, None, None] * wy[:, None, :, None] * wx[:, None, None, :]).astype(D)      # [m, z, y, x]
            row = (corner * wts[..., None]).sum((1, 2, 3), dtype=D)
            sigma = np.where(row[:, 0] < 0.0, zero, row[:, 0])
            alpha = one - np.exp(-sigma * s)
            v = (row[:, 1:1 + 3 * nb].reshape(m, nb, 3) * Y[None, :, None]).sum(1, dtype=D)
            colour = np.where(v < 0.0, zero, np.where(v > 1.0, one, v))                      # a NaN stays a NaN
            t_next = np.cumprod(one - alpha, dtype=D)
            below = np.nonzero(t_next < D(t_min))[0]
            if below.size:                                       # the stopping sample is the last one that counts
                m = int(below[0]) + 1
                c, f, wts, row, alpha, v, colour, t_next = c[:m], f[:m], wts[:m], row[:m], alpha[:m], v[:m], colour[:m], t_next[:m]
            if m:
                v_lo, v_hi = min(v_lo, float(np.nanmin(v))), max(v_hi, float(np.nanmax(v)))
            T = np.concatenate([[one], t_next[:-1]]).astype(D)
            w = T * alpha
            a_sum = w.sum(dtype=D)
            rgb[b] = (w[:, None] * colour).sum(0, dtype=D) + (one - a_sum) * bg
            acc[b], steps[b] = a_sum, m
            cells_of[b] = list(((c[:, 2] * ny + c[:, 1]) * nx + c[:, 0]).tolist())
            G = np.asarray(grad_rgb[b], D) if grad_rgb is not None else D(loss_scale) * (rgb[b] - np.asarray(target[b], D))
            ga = zero if grad_acc is None else D(grad_acc[b])
            if m == 0 or not (np.isfinite(rgb[b]).all() and np.isfinite(acc[b]) and np.isfinite(G).all() and np.isfinite(ga)):
                continue
            q = ((colour - bg) * G[None, :]).sum(1, dtype=D) + ga
            wq = w * q
            behind = np.concatenate([np.cumsum(wq[::-1], dtype=D)[::-1][1:], [zero]]).astype(D)      # S_i, accumulated in reverse
            live = row[:, 0] > 0.0
            drow, arow = np.zeros((m, W), D), np.zeros((m, W), D)
            drow[:, 0] = np.where(live, s * (t_next * q - behind), zero)
            arow[:, 0] = np.where(live, s * (np.abs(t_next * q) + np.abs(wq).sum(dtype=D)), zero)
            inside = (v > 0.0) & (v < 1.0)
            dcol = np.where(inside, w[:, None] * G[None, :], zero)                            # [m, 3]
            drow[:, 1:1 + 3 * nb] = (Y[None, :, None] * dcol[:, None, :]).reshape(m, 3 * nb)
            arow[:, 1:1 + 3 * nb] = np.abs(drow[:, 1:1 + 3 * nb])
            for dz in (0, 1):
                for dy in (0, 1):
                    for dx in (0, 1):
                        at = (c[:, 2] + dz, c[:, 1] + dy, c[:, 0] + dx)
                        wt = wts[:, dz, dy, dx, None]
                        np.add.at(grad, at, wt * drow)
                        np.add.at(A, at, np.abs(wt) * arow)
                        np.add.at(count, at, (np.abs(wt) * arow > 0).astype(np.int64))
    return dict(grad=grad, A=A, count=count, rgb=rgb, acc=acc, steps=steps, cells=cells_of, v_range=(v_lo, v_hi))


def loss_inputs(seed=5, n=pf.N_RAYS):
    """(grad_rgb [n, 3], grad_acc [n], target [n, 3]) float32: the loss sides both test files use"""
    rng = np.random.default_rng(seed)
    return (rng.normal(size=(n, 3)).astype(np.float32), rng.normal(size=n).astype(np.float32),
            rng.uniform(0.0, 1.0, (n, 3)).astype(np.float32))


def scaled_error(got, want, A):
    """|got - want| / (A_e + 1e-3 max_e A_e), the quantity both test files bound"""
    A = np.asarray(A, np.float64)
    return np.abs(np.asarray(got, np.float64) - np.asarray(want, np.float64)) / (A + 1e-3 * A.max())


def runs(cells_of):
    """(samples, flushes) over the rays of a `cells` result: a flush per run of consecutive samples of a ray in one cell"""
    samples = flushes = 0
    for cells in cells_of.values():
        samples += len(cells)
        flushes += sum(1 for i, c in enumerate(cells) if i == 0 or c != cells[i - 1])
    return samples, flushes


# ---- the Adam rule in float32 ------------------------------------------------------------------------------------------------------
def bias_corrections(beta1, beta2, step):
    """(c1, c2) of step `step` >= 1 as the host forms them: Python floats, rounded to float32 when they are passed on"""
    return 1.0 / (1.0 - beta1 ** step), 1.0 / (1.0 - beta2 ** step)


def adam(master, m, v, grad, rows, mask, degree, lr_sigma, lr_colour, beta1, beta2, eps, c1, c2):
    """One step on float32 [N, W] arrays and fp16 rows [N, W], IN PLACE; every operation rounds once to float32.  mask: [N] or None."""
    F = np.float32
    used = USED[degree]
    on = np.ones(master.shape[0], bool) if mask is None else np.asarray(mask).astype(bool)
    b1, b2, e, k1, k2 = F(beta1), F(beta2), F(eps), F(c1), F(c2)
    lr = np.full(used, F(lr_colour), F)
    lr[0] = F(lr_sigma)
    g = grad[on, :used]
    mn = b1 * m[on, :used] + (F(1.0) - b1) * g
    vn = b2 * v[on, :used] + (F(1.0) - b2) * (g * g)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        p = master[on, :used] - lr[None, :] * ((mn * k1) / (np.sqrt(vn * k2) + e))
        half = p.astype(np.float16)
        half[:, 0] = np.where(p[:, 0] > F(65504.0), F(65504.0), p[:, 0]).astype(np.float16)
    assert mn.dtype == F and vn.dtype == F and p.dtype == F
    m[on, :used], v[on, :used], master[on, :used] = mn, vn, p
    rows[on, :used] = half
    grad[:, :used] = 0.0


# ---- the convergence recipe --------------------------------------------------------------------------------------------------------
def student_rows(teacher, degree, seed=23):
    """the teacher with sigma x U(0.5, 1.5) per point and N(0, 0.2) added to the used coefficients"""
    rng = np.random.default_rng(seed)
    rows = teacher.astype(np.float32)
    rows[..., 0] *= rng.uniform(0.5, 1.5, rows.shape[:3]).astype(np.float32)
    rows[..., 1:USED[degree]] += rng.normal(0.0, 0.2, rows.shape[:3] + (USED[degree] - 1,)).astype(np.float32)
    return rows.astype(np.float16)


# ---- the shared cases of both test files: computed once per process ------------------------------------------------------------------
BG = (0.0, 0.25, 0.5)
LATE_T_MIN = 1e-4            # at step 0.1: rays stop after their 64th sample, some after their 128th (test_preview_tune_cpu.py asserts it)
# (step_scale, t_min, hollow occupancy): step 0.1 takes three 64-sample blocks per ray, so carries and runs cross block boundaries
CASES = [(0.5, 0.0, False), (0.5, 0.2, False), (0.1, 0.0, False), (0.1, 0.2, False), (0.1, LATE_T_MIN, False), (0.5, 0.0, True), (0.1, 0.2, True)]
MODES = ("grad", "target")   # random grad_rgb with grad_acc; target mode with loss_scale 0.37
LOSS_SCALE = 0.37
# THE TOLERANCE OF THE GRADIENT, measured on the reference alone (test_preview_tune_cpu.py repeats the measurement and asserts these
# constants): the largest scaled error of this file's float32 run against its float64 run over degrees 0 - 2 and all CASES, per mode.
# Target mode is worse conditioned: G = loss_scale * (rgb - target) cancels where a ray's rgb comes close to its target, and A_e knows
# nothing of that.  The limit of the code under test is 4 x the measured value: the margin covers another summation order (wave scans,
# atomics) and expf's 2 ulp.
MEASURED = {"grad": 9.5e-6, "target": 3.8e-5}        # measured 9.09e-6 (degree 2, step 0.1, t_min 0.2) and 3.72e-5 (degree 1, step 0.1, t_min 0.2)
LIMIT = {mode: 4 * v for mode, v in MEASURED.items()}
_cache = {}


def loss_side(mode):
    G, ga, target = loss_inputs()
    return dict(grad_rgb=G, grad_acc=ga) if mode == "grad" else dict(target=target, loss_scale=LOSS_SCALE)


def case_inputs(degree, case):
    """(rows, occupancy words or None, indices of the non-fragile rays) of CASES[case]; at most 10 % of the rays may be fragile"""
    key = ("in", degree, case)
    if key not in _cache:
        step, t_min, hollow = CASES[case]
        rows = scene_rows(degree, hollow=hollow)
        occ = occupancy_of(rows) if hollow else None
        fragile = pf.march(rows, pf.LO, pf.HI, degree, *pf.scene_rays(), step, t_min, 4096, BG, occ)[4]
        assert fragile.mean() <= 0.10
        _cache[key] = (rows, occ, np.flatnonzero(~fragile))
    return _cache[key]


def reference(degree, case, mode, dtype=np.float64):
    """`march_grad` of CASES[case] on its non-fragile rays, background BG"""
    key = ("ref", degree, case, mode, np.dtype(dtype).name)
    if key not in _cache:
        step, t_min, _ = CASES[case]
        rows, occ, ok = case_inputs(degree, case)
        _cache[key] = march_grad(rows, pf.LO, pf.HI, degree, *pf.scene_rays(), step, t_min, 4096, BG, occ, rays=ok, dtype=dtype, **loss_side(mode))
    return _cache[key]
