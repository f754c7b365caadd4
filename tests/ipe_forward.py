"""Fixture of the forward Gaussians and encodings (numpy only, no kernel runs here): the six classes of rays of ipe_jacobian.make, a
hand-made table of (mean, cov) rows, view directions, the float64 truth of every mean, covariance and feature, a budget per entry,
numpy emulations of the fp32 and of the bf16 ("fast pair") arithmetic, and the mutations a subtly wrong kernel could carry.

Nothing is normalised by a batch maximum and no entry is left out: every entry is held to its own budget.

    mu = (t0 + t1) / 2   hw = (t1 - t0) / 2   den = 3 mu^2 + hw^2          c4 = fl32(4/15), c5 = fl32(5/12): the header's fp32 constants
    t_mean = mu + 2 mu hw^2 / den      t_var = hw^2 / 3 - c4 hw^4 (12 mu^2 - hw^2) / den^2      r_var = r^2 (mu^2 / 4 + c5 hw^2 - c4 hw^4 / den)
    mean_a = d_a t_mean + o_a          cov_a = t_var d_a^2 + r_var (1 - d_a^2 / dn)             dn = |d|^2 + fl32(1e-10)
    feature(half, l, a) = exp(-yv / 2) sin(x)      y = mean_a 2^l, yv = cov_a 4^l (exact scalings)      x = y  |  x = fl32(y + kHalfPiF)
    view(half, l, a)    = sin(x)                   xb = v_a 2^l                                          x = xb |  x = fl32(xb + kHalfPiF)

Truth: these in float64 at the fp32 operands -- t, o, d, radius for the Gaussians; the fp32 (mean, cov) the forward made for the
features.  The fp32 add of the "cos" phase belongs to the reference's definition (mip.py:349-350), so fl32(y + kHalfPiF) is an operand.

Budgets, u = 2^-24, plus a floor of 2^-126 on every entry (a flushed denormal passes):
    mean      C_M u (|d_a| |t_mean| + |o_a|)
    cov       C_V u (|t_var| d_a^2 + |r_var| (1 + d_a^2 / dn))          the header's last expression, every term absolute
    feature   C_F u |truth|                                             fp32 rows (libm sinf / expf) and the view encoding
    bf16 row  2^(e-8) + E,   e = floor(log2(|truth| + E)),   E = damp (2^-16 + 4 pi |x| 2^-53),   damp = exp(-yv / 2)
2^(e-8) is half a bf16 ulp at the truth.  The second term of E is derived: the fp64 reduction of sin_fast resolves 2 |x| 2^-53 turns.
The first is a REQUIREMENT on the fast pair, not a measurement: the error of v_sin_f32 / v_exp_f32 behind sin_fast / exp_fast has to
stay 1/128 of bf16's half ulp at full scale (about 80 times what is derivable: pi u from rounding the reduced phase to fp32 and
|arg| u from __expf's fp32 product).  The emulation below (fp64 reduction, fp32 reduced phase, exact sine, exp2 of the fp32 product,
RNE) reaches 0.996 of this budget; truncation in place of RNE reaches 1.99.

C_M, C_V and C_F are twice the worst ratio (at C = 1) of the HOST build of csrc/raymath.hpp (tests/hostmath: g++ -O2
-ffp-contract=off, glibc sinf / expf) over every class, shape and configuration of this fixture, the hand-made table and the view
directions included; test_ipe_forward_cpu.py measures and prints them.  Measured there: 2.90 (mean, `far` 2x64), 4.99 (covariance,
`wide` 1x513), 2.75 (feature, `far` 1x513, degrees 3-19) and 1.04 for the view encoding alone (B = 257, deg = 4).  They are never
taken from a kernel.  No C_F above C_F_CEILING = 15 would be accepted: (3 + 4 + 1/2) ulp, OpenCL's limits for exp and sin, to which
the device library is built, and the product's rounding.  On the MI355X the fp32 rows reach 0.60 of their budget (3.4 u), the bf16
rows 0.996, where the emulation is (DESIGN.md has the per-class figures)."""
import numpy as np

import ipe_jacobian as ij
from mipnerf_pl_amd.mlp_plan import bf16_round

F = np.float32
F8 = np.float64
U = 2.0 ** -24
FLOOR = 2.0 ** -126
HALF_PI_F = ij.HALF_PI_F
C4 = float(F(4.0 / 15.0))
C5 = float(F(5.0 / 12.0))
EPS_DN = float(F(1e-10))
INV_2PI = 0.15915494309189535                       # sin_fast's constant
LOG2E_F = F(1.4426950408889634)

C_M = 5.8
C_V = 10.0
C_F = 5.6
C_F_CEILING = 15.0

CLASSES = ij.CLASSES
CONFIGS = ((0, 16, False), (0, 16, True), (3, 19, False), (3, 19, True), (15, 31, False), (15, 31, True))
SHAPES = ((7, 1), (5, 5), (3, 43), (2, 64), (1, 513))          # 129 samples: one past a workgroup; 128: exactly one; 513
L = 16
CANARY = 64
config_id = ij.config_id


def case_seed(cls, B, N):
    return 777000 + 1000 * CLASSES.index(cls) + 7 * N + B


def make(cls, B, N):
    """t [B,N+1], o [B,3], d [B,3], r [B] fp32 and the class's info (ipe_jacobian.make)"""
    return ij.make(cls, B, N, np.random.default_rng(case_seed(cls, B, N)))


def table():
    """hand-made (mean, cov) rows [35,3] fp32: every pair of mean in {+0, -0, a denormal, 1e-20, +1, -1, 1e6} and cov in {0, a
    denormal, 1e-12, 1, 1e30} on every axis.  For degrees (0, 16): y stays finite, yv = 1e30 4^15 overflows to inf in fp32."""
    means = np.array([0.0, -0.0, 3e-42, 1e-20, 1.0, -1.0, 1e6], F)
    covs = np.array([0.0, 5e-43, 1e-12, 1.0, 1e30], F)
    pair = (np.arange(35)[:, None] + 12 * np.arange(3)[None, :]) % 35
    mean, cov = means[pair % 7], covs[pair // 7]
    assert all(len({(m.tobytes(), c.tobytes()) for m, c in zip(mean[:, a], cov[:, a])}) == 35 for a in range(3))
    return np.ascontiguousarray(mean), np.ascontiguousarray(cov)


def view_dirs(B):
    """[B,3] fp32: unit vectors, then (from the end) axis-aligned rows with exact 0 and +-1 and one row with a denormal component"""
    v = np.random.default_rng(4242 + B).standard_normal((B, 3))
    v = (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(F)
    special = np.array([[1e-40, 0.6, -0.8], [1, 0, 0], [0, -1, 0], [0, 0, 1], [-1, 0, 0], [0, 1, 0], [0, 0, -1]], F)
    k = min(B, len(special))
    v[B - k:] = special[:k]
    return np.ascontiguousarray(v)


# ---- host build of raymath.hpp --------------------------------------------------------------------------------------------------------
host_gaussians = ij.host_gaussians


def _host():
    if ij._HOST is None:
        z = np.ones((1, 2), F)
        ij.host_gaussians(z, np.zeros((1, 3), F), np.ones((1, 3), F), np.ones(1, F))
    return ij._HOST


def _p(a):
    import ctypes
    return a.ctypes.data_as(ctypes.c_void_p)


def host_features(mean, cov, cfg):
    """fp32 rows [..., 6L] of ipe_feature (hm_ipe: glibc sinf / expf); disable_integration is a zeroed covariance, as in k_cast_ipe"""
    min_deg, max_deg, noint = cfg
    m = np.ascontiguousarray(mean, F).reshape(-1, 3)
    c = np.zeros_like(m) if noint else np.ascontiguousarray(cov, F).reshape(-1, 3)
    out = np.empty((m.shape[0], 6 * (max_deg - min_deg)), F)
    _host().hm_ipe(m.shape[0], _p(m), _p(c), min_deg, max_deg - min_deg, _p(out))
    return out.reshape(mean.shape[:-1] + (out.shape[1],))


def host_view(v, deg):
    v = np.ascontiguousarray(v, F)
    out = np.empty((v.shape[0], 3 + 6 * deg), F)
    _host().hm_view(v.shape[0], _p(v), deg, _p(out))
    return out


# ---- float64 truth and budgets --------------------------------------------------------------------------------------------------------
def worst(got, truth, budget):
    """largest |got - truth| / budget over every entry; a NaN or an inf in `got` counts as inf"""
    got = np.asarray(got, F8)
    if not np.isfinite(got).all():
        return float("inf")
    return float((np.abs(got - truth) / budget).max()) if got.size else 0.0


def gaussian_truth(t, o, d, r):
    """dict of float64 arrays: mean, cov [B,N,3], their magnitudes mag_mean, mag_cov (budget = C u mag + FLOOR), t_mean, t_var, r_var"""
    t8, o8, d8 = t.astype(F8), o.astype(F8), d.astype(F8)
    t0, t1 = t8[:, :-1], t8[:, 1:]
    mu, hw = (t0 + t1) / 2, (t1 - t0) / 2
    mu2, hw2 = mu * mu, hw * hw
    hw4 = hw2 * hw2
    den = 3 * mu2 + hw2
    t_mean = mu + (2 * mu * hw2) / den
    t_var = hw2 / 3 - C4 * ((hw4 * (12 * mu2 - hw2)) / (den * den))
    r_var = (r.astype(F8) ** 2)[:, None] * (mu2 / 4 + C5 * hw2 - C4 * hw4 / den)
    dd = d8 * d8
    dn = dd.sum(-1, keepdims=True) + EPS_DN
    mean = d8[:, None, :] * t_mean[..., None] + o8[:, None, :]
    cov = t_var[..., None] * dd[:, None, :] + r_var[..., None] * (1 - dd / dn)[:, None, :]
    mag_mean = np.abs(d8)[:, None, :] * np.abs(t_mean)[..., None] + np.abs(o8)[:, None, :]
    mag_cov = np.abs(t_var)[..., None] * dd[:, None, :] + np.abs(r_var)[..., None] * (1 + dd / dn)[:, None, :]
    return dict(mean=mean, cov=cov, mag_mean=mag_mean, mag_cov=mag_cov, t_mean=t_mean, t_var=t_var, r_var=r_var)


def gaussian_ratios(mean, cov, tr, c_m=C_M, c_v=C_V):
    return (worst(mean, tr["mean"], c_m * U * tr["mag_mean"] + FLOOR), worst(cov, tr["cov"], c_v * U * tr["mag_cov"] + FLOOR))


def _flat(a, b):
    """[..., L, 3] sin half and "cos" half -> [..., 6L], index = half 3L + l 3 + axis"""
    lead = a.shape[:-2]
    return np.concatenate([a.reshape(lead + (-1,)), b.reshape(lead + (-1,))], -1)


def feature_truth(mean, cov, cfg):
    """dict of float64 [..., 6L]: truth, damp, x (the phase of each feature), budgets f32(c_f) and bf16"""
    min_deg, max_deg, noint = cfg
    scale = 2.0 ** np.arange(min_deg, max_deg)
    y = mean.astype(F8)[..., None, :] * scale[:, None]
    yv = cov.astype(F8)[..., None, :] * (scale * scale)[:, None]              # float64 keeps what overflows fp32: exp gives 0 either way
    y32 = y.astype(F)
    assert np.array_equal(y32.astype(F8), y), "y = mean 2^l is exact in fp32"
    if noint:
        yv = np.zeros_like(yv)
    x = _flat(y, (y32 + F(HALF_PI_F)).astype(F8))
    damp = np.exp(-0.5 * yv)
    damp = _flat(damp, damp)
    truth = damp * np.sin(x)
    E = damp * (2.0 ** -16 + 4 * np.pi * np.abs(x) * 2.0 ** -53)
    with np.errstate(divide="ignore"):
        e = np.floor(np.log2(np.abs(truth) + E))
    return dict(truth=truth, damp=damp, x=x, E=E, bf16=2.0 ** (e - 8) + E + FLOOR)


def f32_budget(truth, c_f=C_F):
    return c_f * U * np.abs(truth) + FLOOR


def view_truth(v, deg):
    """float64 [B, 3 + 6 deg] and the mask of the columns that must be exact (the identity)"""
    v8 = v.astype(F8)
    scale = 2.0 ** np.arange(deg)
    xb = v8[:, None, :] * scale[:, None]
    assert np.array_equal(xb.astype(F).astype(F8), xb)
    xc = (xb.astype(F) + F(HALF_PI_F)).astype(F8)
    truth = np.concatenate([v8, np.sin(_flat(xb, xc))], -1)
    exact = np.arange(3 + 6 * deg) < 3
    return truth, exact


# ---- numpy emulations and their mutations ---------------------------------------------------------------------------------------------
GAUSS_MUTATIONS = ("unstable_t_var", "fma_mean")
FEATURE_MUTATIONS = ("true_cos", "exp2_product", "fp32_reduction", "degree_off_by_one", "swap_halves", "scale_not_squared",
                     "swap_threads", "double_half_pi")
BF16_MUTATIONS = ("fp32_reduction", "truncate")


def emulate_gaussians(t, o, d, r, mutation=None):
    """conical_frustum_to_gaussian restated in numpy fp32, operation by operation in the header's order: (mean, cov) [B,N,3] fp32.
    unstable_t_var: t_var = 3/5 (t1^5 - t0^5) / (t1^3 - t0^3) - t_mean^2 with the t_mean of that branch (mip.py:74-77).
    fma_mean: d t_mean + o with one rounding."""
    assert mutation is None or mutation in GAUSS_MUTATIONS
    assert all(a.dtype == F for a in (t, o, d, r))
    t0, t1 = t[:, :-1], t[:, 1:]
    mu, hw = (t0 + t1) / F(2), (t1 - t0) / F(2)
    mu2, hw2 = mu * mu, hw * hw
    hw4 = hw2 * hw2
    den = F(3) * mu2 + hw2
    t_mean = mu + (F(2) * mu * hw2) / den
    t_var = hw2 / F(3) - F(C4) * ((hw4 * (F(12) * mu2 - hw2)) / (den * den))
    if mutation == "unstable_t_var":
        with np.errstate(invalid="ignore", divide="ignore"):
            p3 = t1 ** 3 - t0 ** 3
            tm = (F(3) * (t1 ** 4 - t0 ** 4)) / (F(4) * p3)
            t_var = F(3.0 / 5.0) * (t1 ** 5 - t0 ** 5) / p3 - tm ** 2
    r2 = (r * r)[:, None]
    r_var = r2 * (mu2 / F(4) + F(C5) * hw2 - F(C4) * hw4 / den)
    dd = d * d
    dn = ((dd[:, 0] + dd[:, 1]) + dd[:, 2] + F(1e-10))[:, None]
    if mutation == "fma_mean":
        mean = (d.astype(F8)[:, None, :] * t_mean.astype(F8)[..., None] + o.astype(F8)[:, None, :]).astype(F)
    else:
        mean = d[:, None, :] * t_mean[..., None] + o[:, None, :]
    null = F(1) - dd / dn
    cov = t_var[..., None] * dd[:, None, :] + r_var[..., None] * null[:, None, :]
    assert mean.dtype == F and cov.dtype == F
    return mean, cov


def _round_sin(x):
    return np.sin(x.astype(F8)).astype(F)                 # a correctly rounded fp32 sine


def _sin_fp32_reduction(x):
    r = x * F(INV_2PI)
    r = r - np.rint(r)
    return np.sin(2 * np.pi * r.astype(F8)).astype(F)


def _scaled(mean, cov, cfg, mutation):
    min_deg, max_deg, noint = cfg
    scale = (2.0 ** np.arange(min_deg, max_deg)).astype(F)
    if mutation == "degree_off_by_one":
        scale = scale * F(2)
    if mutation == "swap_threads":
        scale = np.roll(scale, L // 2)                     # thread q writes the degrees of thread 1 - q
    vs = scale if mutation == "scale_not_squared" else scale * scale
    with np.errstate(over="ignore"):
        y = mean.astype(F)[..., None, :] * scale[:, None]
        yv = cov.astype(F)[..., None, :] * vs[:, None]
    if noint:
        yv = np.zeros_like(yv)
    return y, yv


def emulate_features(mean, cov, cfg, mutation=None):
    """the fp32 row [..., 6L] restated in numpy: fp32 scalings, fp32 phase add, correctly rounded fp32 exp and sin, fp32 product"""
    assert mutation is None or mutation in FEATURE_MUTATIONS
    y, yv = _scaled(mean, cov, cfg, mutation)
    arg = F(-0.5) * yv
    if mutation == "exp2_product":
        damp = np.exp2((arg * LOG2E_F).astype(F8)).astype(F)
    else:
        damp = np.exp(arg.astype(F8)).astype(F)
    xc = y + F(HALF_PI_F)
    if mutation == "double_half_pi":
        xc = (y.astype(F8) + 0.5 * np.pi).astype(F)
    sin = _sin_fp32_reduction if mutation == "fp32_reduction" else _round_sin
    fs = damp * sin(y)
    fc = damp * (np.cos(y.astype(F8)).astype(F) if mutation == "true_cos" else sin(xc))
    if mutation == "swap_halves":
        fs, fc = fc, fs
    out = _flat(fs, fc)
    assert out.dtype == F
    return out


def emulate_bf16(mean, cov, cfg, mutation=None):
    """the bf16 row (as fp32 values) of the fast pair: sin_fast = fp64 reduction to turns, fp32 reduced phase, exact sine of it rounded
    to fp32; exp_fast = exp2 of the fp32 product arg log2(e); fp32 product; RNE to bf16 (mlp_plan.bf16_round)"""
    assert mutation is None or mutation in BF16_MUTATIONS
    y, yv = _scaled(mean, cov, cfg, None)

    def sin_fast(x):
        if mutation == "fp32_reduction":
            return _sin_fp32_reduction(x)
        r = x.astype(F8) * INV_2PI
        r = (r - np.rint(r)).astype(F)
        return np.sin(2 * np.pi * r.astype(F8)).astype(F)

    damp = np.exp2(((F(-0.5) * yv) * LOG2E_F).astype(F8)).astype(F)
    out = _flat(damp * sin_fast(y), damp * sin_fast(y + F(HALF_PI_F)))
    assert out.dtype == F
    if mutation == "truncate":
        return (out.view(np.uint32) & np.uint32(0xFFFF0000)).view(F)
    return bf16_round(out)
