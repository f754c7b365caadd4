"""Fixture of the distortion loss (numpy only, no kernel runs here): classes of weights and fence posts, the float64 truth of the per-ray
value and of every d_w / d_t entry, a budget per entry, and an fp32 numpy emulation of distloss_ray (csrc/raywave.hpp) from which the
budgets' constants are taken.  Nothing is normalised by a batch's largest gradient.

    m_i = fl32(0.5 (t_{i+1} + t_i))     iv_i = fl32(t_{i+1} - t_i)          as the kernel and the reference form them, restated bit for bit
    value  = sum_i iv_i w_i^2 / 3 + sum_ij w_i w_j |m_i - m_j|                the O(N^2) definition (mip.py:8-20), float64 from here on
    d_w_i  = g (2/3 iv_i w_i + 2 sum_j w_j |m_i - m_j|)
    d_t[i] = (A_{i-1} - A_i) + (C_{i-1} + C_i) / 2,    A_i = g w_i^2 / 3,    C_i = 2 g w_i sum_j w_j sign(m_i - m_j)

Budgets, u = 2^-24, e = 2^-53 (the scans are float64: at most K = 16 sequential and 6 shuffled additions each, four scans and eight more
operations in an entry, so 128 e of the magnitudes that cancel):
    value   C_V u |truth| + 128 e sum_i w_i m_i sum_j w_j
    d_w     C_W u |g| (2/3 iv_i w_i + 2 sum_j w_j |m_i - m_j|) + 128 e |g| 2 (m_i sum_j w_j + sum_j w_j m_j)
    d_t     C_T u (|A_{i-1}| + |A_i| + |C_{i-1}| / 2 + |C_i| / 2) + 128 e |g| (w_{i-1} + w_i) sum_j w_j
each plus 2^-120 for the subnormal weights behind a surface (their squares underflow in fp32).
At exactly tied midpoints the reference's autograd takes sign(0) = 0 where the O(N) form orders the tie by index: both are subgradients.
Value and d_w do not depend on the rule; d_t is compared only at fence posts that touch no tied sample (`checked`)."""
import numpy as np

import ray_jacobian as rj

F = np.float32
F8 = np.float64
U = 2.0 ** -24
E64 = 2.0 ** -53
FLOOR = 2.0 ** -120
# The constants of the budgets.  With C = 1 the emulation below (emulate(): double scans, the kernel's fp32 expressions in its order)
# measures over every class and N at B = 18 (test_distloss_cpu.py prints them) a worst |emulation - truth| / budget of
#     value 1.88    d_w 1.87    d_t 2.80
# The constants are twice those.  They come from the emulation, never from the kernel under test.
C_VALUE, C_DW, C_DT = 3.8, 3.8, 5.6

CLASSES = ("soft", "empty", "onehot", "surface", "farfield", "coincident")
SIZES = rj.SIZES + (1024,)
RAYS = 18
G_PATTERN = (1.0, 0.0, -1.0, 1.0e3, -2.5e-3, 0.37, -40.0)
MAX_UNCHECKED = 5


def case_seed(cls, N):
    return 7000 + 1000 * CLASSES.index(cls) + N


def _composite(x):
    """weights of compositing optical depths x [B,N]: w_i = (1 - e^-x_i) exp(-sum_{j<i} x_j), so sum w <= 1"""
    cum = np.concatenate([np.zeros_like(x[:, :1]), np.cumsum(x, -1)[:, :-1]], -1)
    return (-np.expm1(-x) * np.exp(-cum)).astype(F)


def make(cls, B, N, rng):
    """weights [B,N], t [B,N+1], g_ray [B] (fp32) and a dict of what names the class"""
    assert cls in CLASSES
    while True:
        t = np.sort(rng.uniform(2.0, 6.0, (B, N + 1)), axis=-1).astype(F)
        if np.all(np.diff(t, axis=-1) > 0):
            break
    x = np.exp(rng.normal(-2.0, 2.0, (B, N)))
    info = {}
    if cls in ("soft", "farfield", "coincident"):
        w = _composite(x)
    if cls == "empty":
        w = np.zeros((B, N), F)
    if cls == "onehot":
        cand = [min(max(i, 0), N - 1) for i in (0, N // 2, N - 1, 63, 64, rj.lane_bucket(N) - 1, rj.lane_bucket(N))]
        k = np.array([cand[b % len(cand)] for b in range(B)])
        w = np.zeros((B, N), F)
        w[np.arange(B), k] = 1
        info.update(k=k)
    if cls == "surface":
        h = rng.integers(0, N, (B, 1))
        i = np.arange(N)[None, :]
        w = _composite(np.where(i < h, 1e-9 * x, np.minimum(1e-3 * 8.0 ** np.minimum(i - h, 20), 50.0)))
    if cls == "farfield":
        start = rng.uniform(1e2, 9e2, (B, 1)).astype(F)
        steps = np.floor(2.0 ** rng.uniform(1.0, 14.0, (B, N))).astype(np.int64)          # intervals of 2 to 16384 ulp of t
        bits = start.view(np.int32).astype(np.int64) + np.concatenate([np.zeros((B, 1), np.int64), np.cumsum(steps, -1)], -1)
        t = bits.astype(np.int32).view(F)
    if cls == "coincident" and N >= 5:
        j = np.minimum(w[:, :-1], w[:, 1:]).argmax(-1)                                     # t_j = t_{j+1} = t_{j+2} where both tied samples weigh most
        for b in range(B):
            t[b, j[b] + 1] = t[b, j[b]]
            t[b, j[b] + 2] = t[b, j[b]]
        info.update(j=j)
    g = np.array([G_PATTERN[b % len(G_PATTERN)] for b in range(B)]) * np.where(np.arange(B) < len(G_PATTERN), 1.0, rng.uniform(0.5, 2.0, B))
    w, t, g = np.ascontiguousarray(w, F), np.ascontiguousarray(t, F), np.ascontiguousarray(g, F)
    assert np.isfinite(w).all() and np.isfinite(t).all() and np.all(np.diff(t, axis=-1) >= 0) and np.all(w >= 0)
    assert np.all(w.astype(F8).sum(-1) <= 1.0 + 1e-6)
    return w, t, g, info


def mid_interval(t):
    """(m, iv) in fp32, bit for bit as the kernel: (t1 + t0) * 0.5f and t1 - t0"""
    t0, t1 = t[:, :-1], t[:, 1:]
    m, iv = (t1 + t0) * F(0.5), t1 - t0
    assert m.dtype == F and iv.dtype == F
    return m, iv


def tied(t):
    """[B,N] mask of the samples whose midpoint equals another sample's (midpoints are non-decreasing: a neighbour's)"""
    m, _ = mid_interval(t)
    eq = m[:, 1:] == m[:, :-1]
    out = np.zeros(m.shape, bool)
    out[:, 1:] |= eq
    out[:, :-1] |= eq
    return out


def checked_posts(t):
    """[B,N+1] mask of the fence posts that touch no tied sample"""
    td = tied(t)
    out = np.ones(t.shape, bool)
    out[:, :-1] &= ~td
    out[:, 1:] &= ~td
    return out


def _fence(lo, hi):
    z = np.zeros((lo.shape[0], 1))
    return np.concatenate([z, lo], -1), np.concatenate([hi, z], -1)


def truth(w, t, g, c=(C_VALUE, C_DW, C_DT)):
    """dict of float64 value [B], d_w [B,N], d_t [B,N+1] and their budgets, O(N^2) per ray"""
    m32, iv32 = mid_interval(t)
    w8, m, iv, g8 = w.astype(F8), m32.astype(F8), iv32.astype(F8), g.astype(F8)
    B, N = w.shape
    value, sabs, ssgn = np.zeros(B), np.zeros((B, N)), np.zeros((B, N))
    for b in range(B):
        diff = m[b][:, None] - m[b][None, :]
        sabs[b] = np.abs(diff) @ w8[b]
        ssgn[b] = np.sign(diff) @ w8[b]
        value[b] = (iv[b] * w8[b] ** 2).sum() / 3.0 + w8[b] @ sabs[b]
    W, WM = w8.sum(-1, keepdims=True), (w8 * m).sum(-1, keepdims=True)
    dw_mag = (2.0 / 3.0) * iv * w8 + 2.0 * sabs
    d_w = g8[:, None] * dw_mag
    A, C = g8[:, None] * w8 ** 2 / 3.0, 2.0 * g8[:, None] * w8 * ssgn
    (Ap, An), (Cp, Cn) = _fence(A, A), _fence(C, C)                                       # at post i: the values of samples i - 1 and i
    d_t = (Ap - An) + 0.5 * (Cp + Cn)
    wp, wn = _fence(w8, w8)
    return dict(value=value, d_w=d_w, d_t=d_t,
                budget_value=c[0] * U * np.abs(value) + 128 * E64 * (WM * W)[:, 0] + FLOOR,
                budget_w=c[1] * U * np.abs(g8)[:, None] * dw_mag + 128 * E64 * np.abs(g8)[:, None] * 2.0 * (m * W + WM) + FLOOR,
                budget_t=c[2] * U * (np.abs(Ap) + np.abs(An) + 0.5 * np.abs(Cp) + 0.5 * np.abs(Cn))
                + 128 * E64 * np.abs(g8)[:, None] * (wp + wn) * W + FLOOR)


def _ratio(got, want, budget, mask=None):
    """worst |got - want| / budget; an entry with budget 0 must be exact"""
    err = np.abs(got.astype(F8) - want)
    r = np.where(budget > 0, err / np.where(budget > 0, budget, 1.0), np.where(err == 0, 0.0, np.inf))
    if mask is not None:
        r = r[mask]
    return float(r.max()) if r.size else 0.0


def ratios(tr, value=None, d_w=None, d_t=None, checked=None):
    out = {}
    if value is not None:
        out["value"] = _ratio(value, tr["value"], tr["budget_value"])
    if d_w is not None:
        out["d_w"] = _ratio(d_w, tr["d_w"], tr["budget_w"])
    if d_t is not None:
        out["d_t"] = _ratio(d_t, tr["d_t"], tr["budget_t"], checked)
    return out


def emulate(w, t, g, mutation=None):
    """distloss_ray in numpy: its fp32 expressions in its order, its scans in double (their association differs from the wavefront's,
    which moves a double sum by 1e-16).  Returns value [B], d_w [B,N], d_t [B,N+1] in fp32.  mutation: None, "fp32_scan" (the prefix
    sums kept in fp32), "no_self" (the w_i^2 term of d_w dropped), "sign" (the midpoint term of d_t with the wrong sign)."""
    m, iv = mid_interval(t)
    w8, m8 = w.astype(F8), m.astype(F8)
    ex = lambda v: np.concatenate([np.zeros_like(v[:, :1]), np.cumsum(v, -1)[:, :-1]], -1)
    if mutation == "fp32_scan":
        P, Q = ex(w).astype(F8), ex(w * m).astype(F8)
        totP, totQ = w.sum(-1, keepdims=True, dtype=F).astype(F8), (w * m).sum(-1, keepdims=True, dtype=F).astype(F8)
    else:
        P, Q = ex(w8), ex(w8 * m8)
        totP, totQ = w8.sum(-1, keepdims=True), (w8 * m8).sum(-1, keepdims=True)
    uni = (iv * w * w).astype(F8).sum(-1)
    bi = (w8 * (m8 * P - Q)).sum(-1)
    value = (uni / 3.0 + 2.0 * bi).astype(F)
    sj = m8 * P - Q + (totQ - Q - w8 * m8) - m8 * (totP - P - w8)
    self_term = 0.0 if mutation == "no_self" else (2.0 / 3.0) * iv.astype(F8) * w8
    d_w = g[:, None] * (self_term + 2.0 * sj).astype(F)
    A = g[:, None] * (w8 * w8 / 3.0).astype(F)
    C = g[:, None] * (2.0 * w8 * (2.0 * P + w8 - totP)).astype(F)
    if mutation == "sign":
        C = -C
    z = np.zeros((w.shape[0], 1), F)
    d_t = (np.concatenate([z, A], -1) - np.concatenate([A, z], -1)) + F(0.5) * (np.concatenate([z, C], -1) + np.concatenate([C, z], -1))
    assert value.dtype == F and d_w.dtype == F and d_t.dtype == F
    return value, d_w, d_t
