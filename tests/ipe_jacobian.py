"""Fixture of the IPE backward's Jacobian probes (numpy only, no kernel runs here): classes of rays and fence posts, upstream-gradient
probes, the float64 truth of every d_t entry, a budget per entry, and a numpy emulation of k_cast_ipe_bwd (csrc/kernels_resample_grad.hip)
from which the budget's one constant is taken.

The kernel is linear in d_enc, so a probe drives it with a few features at a time.  Every d_t entry is compared on its own: nothing is
normalised by a batch's largest gradient, so a fence post that only the r_var path reaches counts like any other.

    mu = (t0 + t1) / 2   hw = (t1 - t0) / 2   D = 3 mu^2 + hw^2
    t_mean = mu + 2 mu hw^2 / D      t_var = hw^2 / 3 - 4/15 hw^4 (12 mu^2 - hw^2) / D^2      r_var = r^2 (mu^2 / 4 + 5/12 hw^2 - 4/15 hw^4 / D)
    mean_a = o_a + d_a t_mean        cov_a = t_var d_a^2 + r_var (1 - d_a^2 / (|d|^2 + 1e-10))
    feature(half, l, a) = exp(-cov_a 4^l / 2) sin(mean_a 2^l + half pi / 2)

Truth: d feature / d mean_a and d feature / d cov_a in float64 at the fp32 (mean, cov) the forward made (the device's own on the GPU, the
host build of raymath.hpp here; y = mean 2^l and yv = cov 4^l are exact scalings, pi / 2 is float64's), times the float64 derivatives of
(t_mean, t_var, r_var) with respect to (t0, t1) at the fp32 t, o, d, radius.  Fence post i collects the t0 derivative of sample i and the t1
derivative of sample i - 1, on top of what d_t held.

Budget of a d_t entry, u = 2^-24:
    C u M + |fl32(pi/2) - pi/2| Mphi + 2^-120
    M    = |prefill| + the same adjoint with every term absolute: |g_f| |feature derivative| |geometry factor| (|d/dmu| + |d/dhw|) / 2, summed
           over features, axes, the three paths t_mean / t_var / r_var and the one or two samples at the post
    Mphi = M of the "cos" half alone with each feature derivative replaced by its derivative in the phase (the kernel adds fl32(pi/2),
           4.4e-8 above pi / 2, to the phase: |cos| small next to |sin| makes that term larger than any multiple of u |cos|)
The kernel works in float64; C covers the fp32 rounding of the two contributions and of the two atomic adds in either order."""
import ctypes
import os
import subprocess

import numpy as np

F = np.float32
F8 = np.float64
U = 2.0 ** -24
FLOOR = 2.0 ** -120
HALF_PI_F = float(F(0.5) * F(np.pi))              # raymath.hpp kHalfPiF
DPHI = abs(HALF_PI_F - 0.5 * np.pi)               # 4.37e-8
# The constant of the budget.  With C = 1 the emulation below (emulate(): float64 arithmetic, the kernel's expressions and constants, fp32
# rounding of each contribution, both orders of the two adds) measures over every class, configuration, shape and probe
# (test_ipe_jacobian_cpu.py prints them) a worst |emulation - truth| / budget of 1.68 (`coarse_pixel`, degrees 3-11, a single-degree
# probe): up to u on each of the two contributions and on each of the two adds bounds it by 3.  C = 3.4 = twice the measured figure.  It
# comes from the emulation, never from the kernel under test.  (The one-hot probes reach 0.99 at any C: there the kernel's phase offset
# fl32(pi/2) - pi/2 is the whole error and the Mphi term the whole budget.)
C_BUDGET = 3.4

CLASSES = ("scene", "thin", "wide", "axis", "coarse_pixel", "far")
CONFIGS = ((0, 16, False), (0, 16, True), (3, 11, False), (0, 31, False))        # (min_deg, max_deg, disable_integration)
SHAPES = ((7, 1), (5, 5), (5, 64), (3, 171))                                      # 3 x 171 = 513: one thread past two workgroups
FINEST_RADIUS = 5.2e-4
AXIS_NORMS = (0.3, 1.0, 2.5)
CANARY = 64


def case_seed(cls, cfg, B, N):
    return 100000 * CLASSES.index(cls) + 1000 * CONFIGS.index(tuple(cfg)) + 7 * N + B


def config_id(cfg):
    return f"deg{cfg[0]}-{cfg[1]}{'-noint' if cfg[2] else ''}"


# ---- operands -------------------------------------------------------------------------------------------------------------------------
def _sorted_posts(rng, lo, hi, B, n):
    while True:                                 # fp32 rounding can merge two sorted draws: draw again
        t = np.sort(rng.uniform(lo, hi, (B, n)), axis=-1).astype(F)
        if n == 1 or np.all(np.diff(t, axis=-1) > 0):
            return t


def make(cls, B, N, rng):
    """t [B,N+1], origins [B,3], dirs [B,3], radii [B] (fp32) and a dict of what names the class (masks the CPU test asserts on)"""
    from oracle import mipnerf_oracle as orc
    assert cls in CLASSES
    rays = orc.synthetic_rays(B, seed=int(rng.integers(1 << 30)), multiscale=True)
    o, d, r = np.array(rays.origins, F), np.array(rays.directions, F), np.array(rays.radii, F).reshape(B)
    info = {}
    if cls in ("scene", "axis", "coarse_pixel"):
        t = _sorted_posts(rng, 2.0, 6.0, B, N + 1)
    if cls == "coarse_pixel":
        r = (F(FINEST_RADIUS) * np.where(np.arange(B) % 2 == 0, F(8), F(64))).astype(F)
    if cls == "axis":
        k = np.arange(B) % 3
        in_plane = (np.arange(B) + N) % 2 == 1
        norm = np.array(AXIS_NORMS)[(np.arange(B) + np.arange(B) // 3) % 3]
        th = rng.uniform(0.3, 1.2, B)
        d = np.zeros((B, 3))
        rows = np.arange(B)
        d[rows, k] = np.where(in_plane, 0.0, norm)
        d[rows, (k + 1) % 3] = np.where(in_plane, norm * np.cos(th), 0.0)
        d[rows, (k + 2) % 3] = np.where(in_plane, norm * np.sin(th), 0.0)
        d = d.astype(F)
        info.update(norm=norm, in_plane=in_plane)
    if cls == "thin":
        rel = 10.0 ** rng.uniform(-6.0, -3.0, (B, N))                     # hw / mu of each sample
        t = rng.uniform(2.0, 5.0, (B, 1)) * np.concatenate([np.ones((B, 1)), np.cumprod((1 + rel) / (1 - rel), -1)], -1)
        t = t.astype(F)
        rep = rng.integers(0, N, B)                                        # sample `rep` of a ray gets t0 == t1
        if N == 1:
            rep = np.where(np.arange(B) % 2 == 0, 0, -1)                   # a one-sample ray is either repeated or thin: alternate
        for b in range(B):
            if rep[b] >= 0:
                t[b, rep[b] + 1] = t[b, rep[b]]
        info.update(repeated=rep)
    if cls == "wide":
        nw = min(N, 3)
        rel = np.concatenate([np.linspace(0.3, 0.97, B)[:, None], rng.uniform(0.3, 0.6, (B, 2))], -1)[:, :nw]
        t = 0.05 * rng.uniform(1.0, 2.0, (B, 1)) * np.concatenate([np.ones((B, 1)), np.cumprod((1 + rel) / (1 - rel), -1)], -1)
        if N > nw:
            rest = np.sort(rng.uniform(0.0, 4.0, (B, N - nw)), -1) + 0.01 * (1 + np.arange(N - nw))
            t = np.concatenate([t, t[:, -1:] + rest], -1)
        t = t.astype(F)
        info.update(n_wide=nw)
    if cls == "far":
        t = _sorted_posts(rng, 2.0, 100.0, B, N + 1)
        t[:, -1] = F(100.0)
    assert t.shape == (B, N + 1) and np.all(np.diff(t, axis=-1) >= 0) and np.isfinite(t).all() and t.min() > 0
    return np.ascontiguousarray(t), np.ascontiguousarray(o), np.ascontiguousarray(d), np.ascontiguousarray(r), info


def hw_over_mu(t):
    t = t.astype(F8)
    return (t[:, 1:] - t[:, :-1]) / (t[:, 1:] + t[:, :-1])


_HOST = None


def host_gaussians(t, o, d, r):
    """(mean, cov) [B,N,3] fp32 of conical_frustum_to_gaussian from the host build of csrc/raymath.hpp (tests/hostmath/hostmath.cpp,
    g++ -O2 -ffp-contract=off: the build test_hostmath_cpu.py uses)"""
    global _HOST
    here = os.path.dirname(os.path.abspath(__file__))
    src, so = os.path.join(here, "hostmath", "hostmath.cpp"), os.path.join(here, "hostmath", "_hostmath.so")
    if _HOST is None:
        hdrs = [os.path.join(here, "..", "mipnerf_pl_amd", "csrc", h) for h in ("raymath.hpp", "raymath360.hpp")]
        if (not os.path.exists(so)) or os.path.getmtime(so) < max(os.path.getmtime(p) for p in [src] + hdrs):
            subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", src, "-o", so])
        _HOST = ctypes.CDLL(so)
    B, N = t.shape[0], t.shape[1] - 1
    t0, t1 = np.ascontiguousarray(t[:, :-1]).ravel(), np.ascontiguousarray(t[:, 1:]).ravel()
    dd, oo, rr = np.repeat(d, N, axis=0).astype(F), np.repeat(o, N, axis=0).astype(F), np.repeat(r, N).astype(F)
    mean, cov = np.empty((B * N, 3), F), np.empty((B * N, 3), F)
    p = [a.ctypes.data_as(ctypes.c_void_p) for a in (t0, t1, dd, oo, rr, mean, cov)]
    _HOST.hm_cast(B * N, *p)
    return mean.reshape(B, N, 3), cov.reshape(B, N, 3)


def ulp_distance(a, b):
    """largest distance in units of the last place between two fp32 arrays of the same sign pattern"""
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    return int(np.abs(ia - ib).max())


# ---- float64 truth --------------------------------------------------------------------------------------------------------------------
def _frustum_derivatives(t, r):
    """d (t_mean, t_var, r_var) / d (mu, hw) in float64 at the fp32 t and radius: dict of [B,N] arrays"""
    t = t.astype(F8)
    t0, t1 = t[:, :-1], t[:, 1:]
    mu, hw = 0.5 * (t0 + t1), 0.5 * (t1 - t0)
    r2 = (r.astype(F8) ** 2)[:, None]
    D, D_mu, D_hw = 3 * mu ** 2 + hw ** 2, 6 * mu, 2 * hw
    P, P_mu, P_hw = 2 * mu * hw ** 2, 2 * hw ** 2, 4 * mu * hw                            # t_mean = mu + P / D
    Q = hw ** 4 * (12 * mu ** 2 - hw ** 2)                                                # t_var = hw^2 / 3 - 4/15 Q / D^2
    Q_mu, Q_hw = 24 * mu * hw ** 4, 48 * mu ** 2 * hw ** 3 - 6 * hw ** 5
    R, R_hw = hw ** 4, 4 * hw ** 3                                                        # r_var = r^2 (mu^2/4 + 5/12 hw^2 - 4/15 R / D)
    return dict(tm_mu=1 + P_mu / D - P * D_mu / D ** 2, tm_hw=P_hw / D - P * D_hw / D ** 2,
                tv_mu=-(4 / 15) * (Q_mu / D ** 2 - 2 * Q * D_mu / D ** 3),
                tv_hw=2 * hw / 3 - (4 / 15) * (Q_hw / D ** 2 - 2 * Q * D_hw / D ** 3),
                rv_mu=r2 * (mu / 2 + (4 / 15) * R * D_mu / D ** 2),
                rv_hw=r2 * (5 * hw / 6 - (4 / 15) * (R_hw / D - R * D_hw / D ** 2)))


TERMS = ("tm_mu", "tm_hw", "tv_mu", "tv_hw", "rv_mu", "rv_hw")


class Jacobian:
    """The six terms of d feature / d (mu, hw) per sample and feature, float64 [B,N,6L] each, their absolute sums, and the phase terms
    of the "cos" half.  mean, cov: the forward's fp32 Gaussians [B,N,3]."""

    def __init__(self, t, o, d, r, mean, cov, cfg):
        min_deg, max_deg, noint = cfg
        B, N = t.shape[0], t.shape[1] - 1
        L = max_deg - min_deg
        self.B, self.N, self.L, self.cfg = B, N, L, tuple(cfg)
        scale = 2.0 ** np.arange(min_deg, max_deg)                                        # [L]
        y = mean.astype(F8)[:, :, None, :] * scale[:, None]                               # [B,N,L,3]: exact
        yv = cov.astype(F8)[:, :, None, :] * (scale * scale)[:, None]
        assert np.array_equal(y.astype(F).astype(F8), y) and np.array_equal(yv.astype(F).astype(F8), yv), "fp32 scalings are exact"
        if noint:
            yv = np.zeros_like(yv)
        e = np.exp(-0.5 * yv)
        self.damp, self.phase_max = e, float(np.abs(y).max())
        sc = np.broadcast_to(scale[:, None], y.shape)
        d8 = d.astype(F8)
        dd = d8 * d8
        null = 1.0 - dd / (dd.sum(-1, keepdims=True) + 1e-10)
        fd = _frustum_derivatives(t, r)
        geo = dict(tm=d8[:, None, None, :], tv=dd[:, None, None, :], rv=null[:, None, None, :])
        self.terms, absmu, abshw, phimu, phihw = {}, 0.0, 0.0, 0.0, 0.0
        halves = []
        for half in (0, 1):
            ph = y + half * (0.5 * np.pi)
            s, c = np.sin(ph), np.cos(ph)
            f_mean, f_cov = sc * e * c, (0.0 if noint else -0.5) * sc * sc * e * s
            p_mean, p_cov = sc * e * np.abs(s), (0.0 if noint else 0.5) * sc * sc * e * np.abs(c)       # |d / d phase| of the two
            halves.append((f_mean, f_cov, p_mean, p_cov))
        flat = lambda a, b: np.concatenate([a.reshape(B, N, 3 * L), b.reshape(B, N, 3 * L)], -1)        # index = half 3L + l 3 + axis
        for k in TERMS:
            path, var = k.split("_")
            which = 0 if path == "tm" else 1
            fac = fd[k][:, :, None, None] * geo[path]
            self.terms[k] = flat(halves[0][which] * fac, halves[1][which] * fac)
            phi = flat(np.zeros_like(y), halves[1][2 + which] * np.abs(fac))
            if var == "mu":
                absmu, phimu = absmu + np.abs(self.terms[k]), phimu + phi
            else:
                abshw, phihw = abshw + np.abs(self.terms[k]), phihw + phi
        self.jmu = self.terms["tm_mu"] + self.terms["tv_mu"] + self.terms["rv_mu"]
        self.jhw = self.terms["tm_hw"] + self.terms["tv_hw"] + self.terms["rv_hw"]
        self.jabs = 0.5 * (absmu + abshw)
        self.jphi = 0.5 * (phimu + phihw)

    def truth(self, g, prefill=None, only=None, c_budget=C_BUDGET):
        """dict(d_t, budget, M) [B,N+1] in float64 for d_enc = g [B,N,6L]; only: a tuple of TERMS to keep (the rest detached)"""
        g8 = g.astype(F8)
        if only is None:
            jmu, jhw = self.jmu, self.jhw
        else:
            jmu = sum(self.terms[k] for k in only if k.endswith("mu")) + 0.0 * self.jmu
            jhw = sum(self.terms[k] for k in only if k.endswith("hw")) + 0.0 * self.jhw
        gmu, ghw = (jmu * g8).sum(-1), (jhw * g8).sum(-1)
        z = np.zeros((self.B, 1))
        fence = lambda lo, hi: np.concatenate([lo, z], -1) + np.concatenate([z, hi], -1)
        pre = np.zeros((self.B, self.N + 1)) if prefill is None else prefill.astype(F8)
        d_t = pre + fence(0.5 * (gmu - ghw), 0.5 * (gmu + ghw))
        m = (self.jabs * np.abs(g8)).sum(-1)
        M = np.abs(pre) + fence(m, m)
        mphi = (self.jphi * np.abs(g8)).sum(-1)
        return dict(d_t=d_t, M=M, budget=c_budget * U * M + DPHI * fence(mphi, mphi) + FLOOR)


def ratio(got, tr):
    return float((np.abs(got.astype(F8) - tr["d_t"]) / tr["budget"]).max())


# ---- probes ---------------------------------------------------------------------------------------------------------------------------
def onehot_rounds(B, N, L):
    return -(-6 * L // (B * N))


def onehot_probe(B, N, L, rnd, parity):
    """d_enc with one feature (value 1) on every sample of the given parity, feature index cycling with the flat sample index so that the
    rounds together hit all 6 L features; mask [B,N+1] of the fence posts that touch a driven sample (each touches exactly one)"""
    g = np.zeros((B, N, 6 * L), F)
    s = np.arange(B * N).reshape(B, N)
    drive = (np.arange(N)[None, :] % 2 == parity) & np.ones((B, 1), bool)
    feat = (s + rnd * B * N) % (6 * L)
    bb, ii = np.nonzero(drive)
    g[bb, ii, feat[bb, ii]] = 1
    touched = np.zeros((B, N + 1), bool)
    touched[:, :-1] |= drive
    touched[:, 1:] |= drive
    return g, touched, feat, drive


def probes(B, N, L, rng):
    """yields (kind, name, d_enc [B,N,6L] fp32, prefill [B,N+1] fp32 or None); kind `onehot` carries (round, parity) in its name"""
    for rnd in range(onehot_rounds(B, N, L)):
        for parity in ((0,) if N == 1 else (0, 1)):
            yield "onehot", f"onehot{rnd}_{parity}", onehot_probe(B, N, L, rnd, parity)[0], None
    dense = rng.standard_normal((B, N, 6 * L)).astype(F)
    deg = np.tile(np.repeat(np.arange(L), 3), 2)
    for l in range(L):
        yield "degree", f"degree_{l}", (dense * (deg == l)).astype(F), None
    half = np.arange(6 * L) >= 3 * L
    yield "sin_half", "sin_half", (dense * ~half).astype(F), None
    yield "cos_half", "cos_half", (dense * half).astype(F), None
    yield "dense", "dense", dense, None
    pre = (rng.standard_normal((B, N + 1)) * 10.0 ** rng.uniform(-3, 3, (B, N + 1))).astype(F)
    yield "accumulate", "accumulate", rng.standard_normal((B, N, 6 * L)).astype(F), pre
    yield "zero", "zero", np.zeros((B, N, 6 * L), F), pre


KINDS = ("onehot", "degree", "sin_half", "cos_half", "dense", "accumulate", "zero")


# ---- numpy emulation of k_cast_ipe_bwd ------------------------------------------------------------------------------------------------
MUTATIONS = tuple(f"{m}_{k}" for k in TERMS for m in ("drop", "halve")) + ("drop_r_var", "degree_off_by_one", "swap_halves", "assign")


def emulate(t, o, d, r, mean, cov, cfg, g, prefill=None, mutation=None, fp32_phase_add=False):
    """The kernel's arithmetic in float64, expression by expression with its constants, each contribution rounded to fp32, and the two
    adds of a fence post in both orders (fp32 each): returns (d_t with the t0 contribution added first, with the t1 contribution first).
    fp32_phase_add: the "cos" phase formed as fl32(y + fl32(pi/2)), which the kernel did before this fixture.  mutation: one of MUTATIONS."""
    min_deg, max_deg, noint = cfg
    B, N = t.shape[0], t.shape[1] - 1
    L = max_deg - min_deg
    assert mutation is None or mutation in MUTATIONS
    ge = g.astype(F8)
    gs, gc = ge[..., :3 * L].reshape(B, N, L, 3), ge[..., 3 * L:].reshape(B, N, L, 3)
    if mutation == "swap_halves":
        gs, gc = gc, gs
    scale = (2.0 ** np.arange(min_deg, max_deg))[:, None]
    y = (mean[:, :, None, :] * scale.astype(F)).astype(F)
    yv = np.zeros_like(y) if noint else (cov[:, :, None, :] * (scale * scale).astype(F)).astype(F)
    e = np.exp(-0.5 * yv.astype(F8))
    ys = y.astype(F8)
    yc = (y + F(HALF_PI_F)).astype(F8) if fp32_phase_add else ys + HALF_PI_F
    ss, cs, sc, cc = np.sin(ys), np.cos(ys), np.sin(yc), np.cos(yc)
    dscale = scale * (2.0 if mutation == "degree_off_by_one" else 1.0)
    dmean = (dscale * e * (gs * cs + gc * cc)).sum(2)                                     # [B,N,3]
    dcov = (-0.5 * dscale * dscale * e * (gs * ss + gc * sc)).sum(2)
    d8 = d.astype(F8)
    dd = d8 * d8
    dn = dd.sum(-1, keepdims=True) + 1e-10
    g_tmean = (dmean * d8[:, None, :]).sum(-1)
    g_tvar = np.zeros((B, N)) if noint else (dcov * dd[:, None, :]).sum(-1)
    g_rvar = np.zeros((B, N)) if noint or mutation == "drop_r_var" else (dcov * (1.0 - dd / dn)[:, None, :]).sum(-1)
    t8 = t.astype(F8)
    t0, t1 = t8[:, :-1], t8[:, 1:]
    mu, hw = 0.5 * (t0 + t1), 0.5 * (t1 - t0)
    mu2, hw2 = mu * mu, hw * hw
    hw3, hw4 = hw2 * hw, hw2 * hw2
    hw5 = hw4 * hw
    D = 3.0 * mu2 + hw2
    D2 = D * D
    D3 = D2 * D
    Nn = hw4 * (12.0 * mu2 - hw2)
    r2 = (r.astype(F8) * r.astype(F8))[:, None]
    v = dict(tm_mu=1.0 + 2.0 * hw2 / D - 12.0 * mu2 * hw2 / D2,
             tm_hw=4.0 * mu * hw / D - 4.0 * mu * hw3 / D2,
             tv_mu=-(4.0 / 15.0) * (24.0 * mu * hw4 / D2 - 12.0 * mu * Nn / D3),
             tv_hw=2.0 * hw / 3.0 - (4.0 / 15.0) * ((48.0 * mu2 * hw3 - 6.0 * hw5) / D2 - 4.0 * hw * Nn / D3),
             rv_mu=r2 * (0.5 * mu + (8.0 / 5.0) * mu * hw4 / D2),
             rv_hw=r2 * (5.0 * hw / 6.0 - (4.0 / 15.0) * (4.0 * hw3 / D - 2.0 * hw5 / D2)))
    if mutation is not None and mutation.split("_", 1)[-1] in TERMS:
        how, k = mutation.split("_", 1)
        v[k] = v[k] * (0.0 if how == "drop" else 0.5)
    g_mu = g_tmean * v["tm_mu"] + g_tvar * v["tv_mu"] + g_rvar * v["rv_mu"]
    g_hw = g_tmean * v["tm_hw"] + g_tvar * v["tv_hw"] + g_rvar * v["rv_hw"]
    lo, hi = (0.5 * g_mu - 0.5 * g_hw).astype(F), (0.5 * g_mu + 0.5 * g_hw).astype(F)
    z = np.zeros((B, 1), F)
    lo, hi = np.concatenate([lo, z], -1), np.concatenate([z, hi], -1)
    pre = np.zeros((B, N + 1), F) if prefill is None else prefill
    if mutation == "assign":                                                              # `=` in place of `+=`: the last store stays
        first = np.concatenate([lo[:, :-1], hi[:, -1:]], -1)
        second = np.concatenate([lo[:, :1], hi[:, 1:]], -1)
        return first, second
    a, b = (pre + lo) + hi, (pre + hi) + lo
    assert a.dtype == F and b.dtype == F
    return a, b
