"""Fixture of the forward compositing checks (numpy only, no kernel runs here): the ray classes of tests/ray_jacobian.py plus a group of
degenerate rays, the float64 truth of every output of composite_ray (csrc/raywave.hpp, behind k_volumetric_rendering,
k_composite_resample and k_composite_train) from the kernel's own fp32 operands, a running-error budget per entry, and an fp32
emulation of composite_ray from which the budgets' one constant is taken and on which the wrong variants ("mutants") are switches.

Every entry is compared on its own: nothing is normalised by a batch's largest value, so a weight of 1e-7 behind a surface counts like
any other, and no entry is left out (the masks of compared() are all-true).

    delta_i = (t_{i+1} - t_i) |d|     x_i = sigma_i delta_i     cum_i = sum_{j<i} x_j     T_i = exp(-cum_i)
    w_i     = -expm1(-x_i) T_i
    acc     = sum_i w_i
    rgb_c   = sum_i w_i c_ic + [white] (1 - acc)
    distance = clip(sum_i w_i tmid_i, t_0, t_N),   tmid_i = (t_i + t_{i+1}) / 2

Budgets (units of u = 2^-24; bounds on the rounding the kernel's fp32 evaluation order can accumulate, not tolerances):
    growth_i = 2 + cum_i                       the kernel rounds cum_i to fp32 before expf: T_i carries cum_i u, expf its own ulps
    werr_i   = w_i (growth_i + x_i) + T_i      alpha = 1 - expf(-x) carries an ABSOLUTE rounding of one ulp of 1 (the reference's own form,
                                               kept for parity), which enters w_i as T_i -- the same term as in ray_jacobian.py
    S        = K + 6                           the fp32 additions on the longest path of one of the kernel's five sums: K in the lane
                                               (sr += w * c, K times) and the six DPP steps of wave_incl_scan_dpp (row_shr 1, 2, 4, 8,
                                               row_bcast 15, 31), read off raywave.hpp
    budget_w     = C u werr_i + 2^-120
    budget_acc   = C u (sum werr + S sum w) + 2^-120
    budget_rgb_c = C u (sum werr |c| + S sum w |c|) + [white] (budget_acc + C u (1 + |rgb_c|)) + 2^-120
    budget_dist  = C u (sum werr tmid + S sum w tmid + t_N) + 2^-120
clip is 1-Lipschitz, so a ray whose distance sits on or near a clamp bound is compared like any other.  The 2^-120 floor covers
subnormal transmittances.

The constant.  With C = 1 the fp32 emulation below (emulate(): the kernel's expressions one by one, its exclusive scan in double, its
five sums in the kernel's lane-then-wave order, numpy's expf) measures over every class, both white flags and every N of SIZES at B = 18,
and over the degenerate group at DEGENERATE_SIZES (test_composite_forward_cpu.py prints them):
    worst |emulation - truth| / budget:   weights 2.32 (opaque, N = 513)    acc 1.39    rgb 1.39    distance 0.20
C = 4.64 = the worst ratio (2.32, the weights; one constant serves all four outputs), times 2 for the 1-2 ulp by which the device's expf
may differ from numpy's.  It comes from the emulation, never from the kernel under test.  (The worst entry is a weight of 2.5e-15 at
cum_i = 32: the fp32 |d| of its ray is 1.4 u short, which enters EVERY x_j of the ray with one sign, the products' roundings bring the
double sum to 1.9 u cum_i and its rounding to fp32 to 2.7 u cum_i, where growth_i counts 1 u cum_i.)"""
import numpy as np

import ray_jacobian as rj
from ray_jacobian import CLASSES, FLOOR, RAYS, U, F, case_seed, lane_bucket, make, Ray   # noqa: F401  (re-exported to the tests)

C_BUDGET = 4.64
SIZES = rj.SIZES + (1024,)                     # 1024: the full last lane of K = 16
DEGENERATE_SIZES = (5, 65, 1024)
DEGENERATE_KINDS = ("zero_ray", "zero_samples", "zero_width", "flat", "zero_dir", "opaque_last")
OUTPUTS = ("weights", "acc", "rgb", "distance")
MUTANTS = ("inclusive", "no_dnorm", "no_wave_offset", "unclamped", "last_post_zero")


def scan_depth(N):
    """S: the fp32 additions on the longest path of a sum of composite_ray<K>"""
    return lane_bucket(N) + 6


def edge_samples(N):
    """both ends of lane 0's share, the lane boundary (K - 1 | K) and the last sample"""
    K = lane_bucket(N)
    return sorted({min(max(i, 0), N - 1) for i in (0, K - 1, K, N - 1)})


def degenerate_rays(B=RAYS):
    """kind -> the rays of the batch that carry it (two each, in different workgroups); every other ray is soft"""
    assert B >= 13
    return {kind: (k, k + 7) for k, kind in enumerate(DEGENERATE_KINDS)}


def make_degenerate(N, B=RAYS):
    """rgb_sigma [B,N,4], t [B,N+1], dirs [B,3] (finite fp32) of the degenerate group and the exact facts that hold for them:
    zero_w [B,N] (weight == 0), empty [B] (weights 0, acc 0, rgb == white flag, distance == t_0), at_near [B] (distance == t_0)"""
    rng = np.random.default_rng(7000 + N)
    rs, t, d = make("soft", B, N, rng)
    rays = degenerate_rays(B)
    edges = edge_samples(N)
    zero_w = np.zeros((B, N), bool)
    empty, at_near = np.zeros(B, bool), np.zeros(B, bool)
    for b in rays["zero_ray"]:
        rs[b, :, 3] = 0
        zero_w[b] = empty[b] = at_near[b] = True
    for b in rays["zero_samples"]:
        rs[b, edges, 3] = 0
        zero_w[b, edges] = True
    for b in rays["zero_width"]:
        for i in edges:                        # increasing: neighbouring edges give a run of equal fence posts
            t[b, i + 1] = t[b, i]
        zero_w[b, edges] = True
    for b in rays["flat"]:
        t[b, :] = t[b, 0]
        zero_w[b] = at_near[b] = True
    for b in rays["zero_dir"]:
        d[b] = 0
        zero_w[b] = empty[b] = at_near[b] = True
    for b in rays["opaque_last"]:
        rs[b, N - 1, 3] = 1e6
    assert rs.dtype == F and t.dtype == F and d.dtype == F
    assert np.isfinite(rs).all() and np.isfinite(t).all() and np.isfinite(d).all() and np.all(np.diff(t, axis=-1) >= 0)
    return rs, t, d, dict(zero_w=zero_w, empty=empty, at_near=at_near)


# ---- float64 truth and budgets --------------------------------------------------------------------------------------------------------
def truth(ray, white, c_budget=C_BUDGET):
    """the four outputs and their budgets in float64 from a ray_jacobian.Ray; `sum_dist` is the distance before the clamp"""
    B, N = ray.x.shape
    S = float(scan_depth(N))
    cu = c_budget * U
    w = ray.w
    acc = w.sum(-1)
    rgb = (w[..., None] * ray.c).sum(-2) + ((1.0 - acc)[:, None] if white else 0.0)
    sum_dist = (w * ray.tmid).sum(-1)
    distance = np.clip(sum_dist, ray.t0, ray.tN)
    werr = w * (ray.growth + ray.x) + ray.T
    cabs = np.abs(ray.c)
    budget_w = cu * werr + FLOOR
    budget_acc = cu * (werr.sum(-1) + S * w.sum(-1)) + FLOOR
    budget_rgb = cu * ((werr[..., None] * cabs).sum(-2) + S * (w[..., None] * cabs).sum(-2)) + FLOOR
    if white:
        budget_rgb = budget_rgb + (budget_acc[:, None] + cu * (1.0 + np.abs(rgb)))
    budget_dist = cu * ((werr * ray.tmid).sum(-1) + S * (w * ray.tmid).sum(-1) + ray.tN) + FLOOR
    return dict(weights=w, acc=acc, rgb=rgb, distance=distance, sum_dist=sum_dist,
                budget_weights=budget_w, budget_acc=budget_acc, budget_rgb=budget_rgb, budget_distance=budget_dist)


def compared(tr):
    """the entries of each output that ratios() compares: all of them"""
    return {k: np.ones(tr[k].shape, bool) for k in OUTPUTS}


def ratios(got, tr):
    """worst |got - truth| / budget per output; got = (rgb [B,3], distance [B], acc [B], weights [B,N]), the order of the entry point.
    A non-finite entry gives a non-finite ratio, which no `<= 1` accepts."""
    mask = compared(tr)
    out = {}
    for k, g in zip(("rgb", "distance", "acc", "weights"), got):
        g = np.asarray(g)
        assert g.shape == tr[k].shape, (k, g.shape, tr[k].shape)
        with np.errstate(invalid="ignore"):
            e = np.abs(g.astype(np.float64) - tr[k]) / tr["budget_" + k]
        e = e[mask[k]]
        out[k] = float("nan") if np.isnan(e).any() else float(e.max())
    return {k: out[k] for k in OUTPUTS}


# ---- fp32 emulation of composite_ray ---------------------------------------------------------------------------------------------------
def _wave_sum32(v):
    """lane 63 of wave_incl_scan_dpp on [B,64] fp32: row_shr 1, 2, 4, 8 inside each row of 16, then row_bcast 15 (lane 15 of rows 0 / 2
    into rows 1 / 3) and row_bcast 31 (lane 31 into rows 2 and 3)"""
    assert v.dtype == F and v.shape[-1] == 64
    r = np.arange(64) % 16
    for n in (1, 2, 4, 8):
        sh = np.zeros_like(v)
        sh[:, n:] = v[:, :-n]
        sh[:, r < n] = 0
        v = v + sh
    add = np.zeros_like(v)
    add[:, 16:32] = v[:, 15:16]
    add[:, 48:64] = v[:, 47:48]
    v = v + add
    add = np.zeros_like(v)
    add[:, 32:64] = v[:, 31:32]
    v = v + add
    assert v.dtype == F
    return v[:, 63]


def _lane_then_wave(term, K):
    """sum of term [B,N] fp32 as the kernel forms it: each lane adds its K samples in order (samples past N add 0), then the wave"""
    B, N = term.shape
    pad = np.zeros((B, 64 * K), F)
    pad[:, :N] = term
    pad = pad.reshape(B, 64, K)
    s = np.zeros((B, 64), F)
    for k in range(K):
        s = s + pad[:, :, k]
    return _wave_sum32(s)


def emulate(rgb_sigma, t, dirs, white, mutant=None, mutant_lane=1):
    """composite_ray's arithmetic in numpy fp32, expression by expression, with its exclusive scan in double (the association of the
    wavefront's double scan differs, which moves a double sum by 1e-16) and its five sums in the kernel's lane-then-wave order.
    mutant: one of MUTANTS --
      inclusive       transmittance from the inclusive sum
      no_dnorm        delta without |d|
      no_wave_offset  the share of lane `mutant_lane` without the wave's offset (its transmittances restart at 1)
      unclamped       distance left unclamped
      last_post_zero  tv[K] of a lane read as 0 where i0 + K == N (the guard `i0 + k < N` in place of `<=`)
    Returns rgb [B,3], distance [B], acc [B], weights [B,N] in fp32."""
    assert mutant is None or mutant in MUTANTS
    f8 = np.float64
    B, N = rgb_sigma.shape[:2]
    K = lane_bucket(N)
    c, sig = rgb_sigma[..., :3], rgb_sigma[..., 3]
    dx_, dy_, dz_ = dirs[:, 0], dirs[:, 1], dirs[:, 2]
    dn = np.sqrt(dx_ * dx_ + dy_ * dy_ + dz_ * dz_)[:, None]
    t0, t1 = t[:, :-1], t[:, 1:].copy()
    if mutant == "last_post_zero" and N % K == 0:
        t1[:, N - 1] = 0
    delta = (t1 - t0) if mutant == "no_dnorm" else (t1 - t0) * dn
    dd = sig * delta
    incl = np.cumsum(dd.astype(f8), axis=-1)
    cum = incl if mutant == "inclusive" else incl - dd.astype(f8)
    if mutant == "no_wave_offset":
        i0 = mutant_lane * K
        if i0 < N:
            cum = cum.copy()
            cum[:, i0:i0 + K] -= cum[:, i0:i0 + 1].copy()
    with np.errstate(over="ignore"):           # last_post_zero makes dd negative
        alpha = F(1) - np.exp(-dd)
    trans = np.exp(-cum.astype(F))
    w = alpha * trans
    tmid = F(0.5) * (t0 + t1)
    sr, sg, sb = (_lane_then_wave(w * c[..., k], K) for k in range(3))
    sa = _lane_then_wave(w, K)
    sd = _lane_then_wave(w * tmid, K)
    dist = np.nan_to_num(sd)
    if mutant != "unclamped":
        dist = np.minimum(np.maximum(dist, t[:, 0]), t[:, -1])
    rgb = np.stack([sr, sg, sb], -1)
    if white:
        rgb = rgb + (F(1) - sa)[:, None]
    assert rgb.dtype == F and dist.dtype == F and sa.dtype == F and w.dtype == F
    return rgb, dist, sa, w
