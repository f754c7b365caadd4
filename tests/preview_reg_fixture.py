"""Rules R1 - R4 of csrc/preview_reg.hpp (the total-variation term and the SH decay on the master rows of a baked lattice, value and
gradient) restated in numpy, for test_preview_reg_cpu.py and test_gpu_preview_reg.py.  Whole-array slices; the fixture knows nothing of
threads, chunks or stencils of 13 values.

`gradient(..., dtype=np.float64)` is the reference; with dtype=np.float32 every operation rounds once to float32 IN THE ORDER THE HEADER
WRITES DOWN, so the host build of the header (tests/hostmath/preview_reg.cpp) and the kernel must give its bytes."""
import numpy as np

import preview_fixture as pf
import preview_tune_fixture as tf

USED = tf.USED
F = np.float32
# the lattices of the GPU test: the 8 x 9 x 10 lattice over the non-cubic box of the other preview tests, and two whose x-lines are shorter
# than a wave / straddle waves and whose smallest spacing sits on another axis each
LATTICES = [(pf.DIMS, pf.LO, pf.HI), ((2, 3, 65), pf.LO, pf.HI), ((67, 3, 2), pf.LO, pf.HI)]
WEIGHTS = (0.03, 0.011, 0.007)           # w_sigma, w_colour, w_view of the byte-for-byte cases: arbitrary, all different
EPS = 1e-4


def axis_scale(dims, lo, hi):
    """r_a = hmin / h_a in float32, h_a = (hi_a - lo_a) / float(n_a - 1) as the preview libraries form the spacings -> float32 [3]"""
    h = (np.asarray(hi, F) - np.asarray(lo, F)) / (np.asarray(dims) - 1).astype(F)
    return (h.min() / h).astype(F)


def point_mask(words, dims):
    """uint8 [nz, ny, nx]: 1 at the points next to an occupied cell of the occupancy words (`preview.baked_points`)"""
    nx, ny, nz = dims
    cells = np.zeros((nz - 1, ny - 1, nx - 1), bool)
    for i in range(nx - 1):
        cells[..., i] = (words[..., i >> 5] >> np.uint32(i & 31)) & 1
    mask = np.zeros((nz, ny, nx), bool)
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                mask[dz:dz + nz - 1, dy:dy + ny - 1, dx:dx + nx - 1] |= cells
    return mask.astype(np.uint8)


def master_rows(dims, degree, seed=41, sentinel=777.0):
    """fp32 [nz, ny, nx, W] master rows: sigma in [0, 50], coefficients N(0, 1); the pad entries hold `sentinel`"""
    rng = np.random.default_rng(seed + 10 * degree + dims[0])
    nx, ny, nz = dims
    rows = rng.normal(0.0, 1.0, (nz, ny, nx, pf.ROW_HALVES[degree])).astype(F)
    rows[..., 0] = rng.uniform(0.0, 50.0, (nz, ny, nx)).astype(F)
    rows[..., USED[degree]:] = F(sentinel)
    return rows


def random_mask(dims, seed=43, keep=0.7):
    rng = np.random.default_rng(seed + dims[0])
    nx, ny, nz = dims
    return (rng.uniform(size=(nz, ny, nx)) < keep).astype(np.uint8)


def _shift(a, axis, by, fill):
    """a[p + by e_axis], `fill` where that leaves the lattice; axis 0 / 1 / 2 = x / y / z of arrays [nz, ny, nx, ...]"""
    ax = 2 - axis
    out = np.full_like(a, fill)
    src = [slice(None)] * a.ndim
    dst = [slice(None)] * a.ndim
    if by > 0:
        src[ax], dst[ax] = slice(by, None), slice(None, -by)
    else:
        src[ax], dst[ax] = slice(None, by), slice(-by, None)
    out[tuple(dst)] = a[tuple(src)]
    return out


def _differences(v, on, r, eps, D):
    """(d [3][nz, ny, nx, U], n [nz, ny, nx, U]) of rules R1 and R2 at every anchor; meaningless where the anchor is not present"""
    d = []
    for a in range(3):
        there = _shift(v, a, 1, 0)
        both = (on & _shift(on, a, 1, False))[..., None]
        with np.errstate(invalid="ignore", over="ignore"):
            d.append(np.where(both, r[a] * (there - v), D(0.0)))
    with np.errstate(invalid="ignore", over="ignore"):
        n = np.sqrt(((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]) + D(F(eps)))
    return d, n


def _prepare(master, mask, degree, scale, dtype):
    D = dtype
    used = USED[degree]
    v = np.asarray(master)[..., :used].astype(D)
    on = np.ones(v.shape[:3], bool) if mask is None else np.asarray(mask).reshape(v.shape[:3]) != 0
    return D, used, v, on, [D(x) for x in np.asarray(scale, F)]


def value(master, mask, degree, scale, w_sigma, w_colour, w_view, eps, dtype=np.float64):
    """The regulariser's value: sum_p w n(p) over the present p and the used e, plus 0.5 w_view v^2 over the entries e >= 4.  n(p) in
    `dtype`, the sums in float64 (no library forms them)."""
    D, used, v, on, r = _prepare(master, mask, degree, scale, dtype)
    _, n = _differences(v, on, r, eps, D)
    w = np.full(used, float(F(w_colour)))
    w[0] = float(F(w_sigma))
    tv = (n[on].astype(np.float64) * w).sum()
    return float(tv + 0.5 * float(F(w_view)) * (v[on][:, 4:].astype(np.float64) ** 2).sum())


def total_variation(master, mask, degree, scale, eps):
    """(sum_p n(p) of the density entry, the same of the colour entries) in float64: the figures the end-to-end test compares"""
    D, used, v, on, r = _prepare(master, mask, degree, scale, np.float64)
    _, n = _differences(v, on, r, eps, D)
    return float(n[on][:, 0].sum()), float(n[on][:, 1:].sum())


def gradient(master, mask, degree, scale, grad, w_sigma, w_colour, w_view, eps, dtype=np.float64):
    """`grad` [nz, ny, nx, W] plus the gradient of `value`, as a new array of `dtype`: rules R3 and R4, operation by operation.  Entries of
    points that are not present, and pad entries, are `grad`'s."""
    D, used, v, on, r = _prepare(master, mask, degree, scale, dtype)
    d, n = _differences(v, on, r, eps, D)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        t = -(((r[0] * d[0] + r[1] * d[1]) + r[2] * d[2]) / n)
        for a in range(3):
            back = (r[a] * _shift(d[a], a, -1, 0)) / _shift(n, a, -1, 1)
            t = np.where(_shift(on, a, -1, False)[..., None], t + back, t)
        out = np.asarray(grad).astype(D).copy()
        g = out[..., :used].copy()
        w = np.full(used, D(F(w_colour)), D)
        w[0] = D(F(w_sigma))
        g = np.where(w != 0, g + w * t, g)
        if D(F(w_view)) != 0 and used > 4:
            g[..., 4:] = g[..., 4:] + D(F(w_view)) * v[..., 4:]
    assert t.dtype == D and g.dtype == D
    out[..., :used] = np.where(on[..., None], g, out[..., :used])
    return out


def stencil_points(q, dims, on, decays):
    """the present points p whose gradient reads entry e of the present point q = (x, y, z), by the header's closing paragraph: q - e_a (q
    is its forward neighbour), q + e_a (q is its backward anchor), q + e_a - e_b, b != a (q is the neighbour along b of its backward anchor
    q - e_b, which must be present itself), and q itself when one of its six axis neighbours is present or the entry decays (`decays`:
    e >= 4 with w_view != 0) -- a point without present neighbours has only zero differences, which do not read its own value"""
    e = np.eye(3, dtype=int)
    q = np.array(q)
    here = lambda c: bool(all(0 <= x < m for x, m in zip(c, dims)) and on[c[2], c[1], c[0]])
    cand = [q - e[a] for a in range(3)] + [q + e[a] for a in range(3)]
    cand += [q] if decays or any(here(c) for c in cand) else []
    cand += [q + e[a] - e[b] for a in range(3) for b in range(3) if a != b and here(q - e[b])]
    return {tuple(int(x) for x in c) for c in cand if here(c)}


# ---- the end-to-end recipe: the tune tests' student / teacher, with and without the regulariser -----------------------------------------
RECIPE = dict(tv_sigma=2e-4, tv_colour=2e-4, sh_decay=5e-5, tv_eps=EPS, steps=40, lr_sigma=0.2, lr_colour=0.02)


def recipe(regularised, steps=None):
    """The recipe of test_preview_tune_cpu.test_the_reference_converges_on_the_recipe, on the fixtures alone: float64 gradients of the march
    (preview_tune_fixture), this file's float32 gradient of the regulariser added with the weights of RECIPE divided by the number of
    points (no mask: all of them), float32 Adam, rows re-rounded to fp16 every step.  Returns (losses [steps + 1], (tv_sigma, tv_colour) of
    the final master rows)."""
    rays = pf.scene_rays()
    steps = RECIPE["steps"] if steps is None else steps
    teacher = tf.scene_rows(1)
    want = pf.march(teacher, pf.LO, pf.HI, 1, *rays, 0.5, 1e-3, 4096, (1.0, 1.0, 1.0))
    ok = np.flatnonzero(~want[4])
    target = want[0].astype(F)
    rows = tf.student_rows(teacher, 1)
    shape = rows.shape
    rows = rows.reshape(-1, 16)
    master = rows.astype(F)
    m, v = np.zeros_like(master), np.zeros_like(master)
    scale = axis_scale(pf.DIMS, pf.LO, pf.HI)
    n_points = master.shape[0]
    losses = []
    for k in range(steps + 1):
        out = tf.march_grad(rows.reshape(shape), pf.LO, pf.HI, 1, *rays, 0.5, 1e-3, 4096, (1.0, 1.0, 1.0), target=target,
                            loss_scale=2.0 / (3 * len(ok)), rays=ok)
        losses.append(float(((out["rgb"][ok] - target[ok]) ** 2).mean()))
        if k < steps:
            grad = out["grad"].astype(F)
            if regularised:
                grad = gradient(master.reshape(shape), None, 1, scale, grad, RECIPE["tv_sigma"] / n_points, RECIPE["tv_colour"] / n_points,
                                RECIPE["sh_decay"] / n_points, RECIPE["tv_eps"], F)
            c1, c2 = tf.bias_corrections(0.9, 0.999, k + 1)
            tf.adam(master, m, v, grad.reshape(-1, 16), rows, None, 1, RECIPE["lr_sigma"], RECIPE["lr_colour"], 0.9, 0.999, 1e-8, c1, c2)
    return np.array(losses), total_variation(master.reshape(shape), None, 1, scale, RECIPE["tv_eps"])


# What `recipe` gives (python tests/preview_reg_fixture.py prints them): the yardstick of the end-to-end GPU test, measured on the
# fixtures alone.  Batch loss before step 0 and before step 40, and the final (sigma, colour) total variation.
# The weights are small because Adam rescales whatever it is given: they decide only how the regulariser's pull compares with the
# photometric one at the points the rays reach (at 2e-3 / 2e-3 / 5e-4 the same run stops at a loss of 2.9e-4, at 2e-2 the loss rises).
RECORDED = {
    False: dict(loss0=1.5179e-3, loss=7.1657e-6, tv=(4.1948e3, 9.0612e3)),
    True: dict(loss0=1.5179e-3, loss=1.8586e-5, tv=(7.0259e2, 4.4696e3)),
}


if __name__ == "__main__":
    for reg in (False, True):
        losses, tv = recipe(reg)
        print(f"regularised {reg}: loss {losses[0]:.4e} -> {losses[-1]:.4e}, tv sigma {tv[0]:.4e} colour {tv[1]:.4e}")
