"""Fixture of the unbounded-scene forward path (numpy only, no kernel runs here): csrc/raymath360.hpp and csrc/kernels_360.hip held to
float64 entry by entry -- seven classes of rays, five ragged shapes, five ranges of degrees, a hand-made table of Gaussians, a small
lattice, the float64 truth of every fence post, mean, covariance and feature, a budget per entry, numpy emulations of the fp32 and of
the bf16 arithmetic, and the mutations a subtly wrong kernel could carry.  Conventions of tests/ipe_forward.py: u = 2^-24, a floor of
2^-126 on every budget (a flushed denormal passes), nothing normalised by a batch maximum, no entry left out.

Truth: the header's expression in float64 at the fp32 operands the stage receives, with the header's fp32 constants.
    1 fence posts   ni = 1 / near, fi = 1 / far, s = torch_linspace_at(0, 1, N + 1, k) (fp32, an operand)
                    post_k = fi s + (1 - s) ni;  jitter: lo = (post_k + post_k-1) / 2 (post_0 at k = 0), up likewise,  t_inv = lo + (up - lo) t_rand
                    t = 1 / t_inv from the route's OWN fp32 t_inv: one correctly rounded division, held to 1 u relative
    2 frustum       mu, hw, den, t_mean, t_var, r_var as in ipe_forward;  mean_a = d_a t_mean + o_a
                    cov_ab = t_var d_a d_b + r_var (delta_ab - d_a d_b / dn),  dn = |d|^2 + fl32(1e-10)
    3 fused         from the fp32 UNCONTRACTED mean m (contracted = 0 returns it: the same expression, the same bits) and the float64 t_var,
                    r_var, d, dn:  n2 = |m|^2, n = sqrt(n2), u = m / n, a = (2 n - 1) / n2, b = 1 / n2, v = a d + ((b - a) (u . d)) u
                    mean' = m (2 - 1 / n) / n,   cov'_ij = t_var v_i v_j + r_var (delta_ij a^2 + (b^2 - a^2) u_i u_j - v_i v_j / dn)
                    n2 <= 1 (decided in float64; no frustum sample of the fixture has |n2 - 1| < 2^-18): the Gaussian of stage 2, bit for bit
    4 generic       mean' as above, cov' = J C J^T with J = a (I - u u^T) + b u u^T at the given fp32 (mean, cov)
    5 features      from the fp32 (mean, cov) the per-direction route returns: y = p . mean, var = p^T cov p, x = 2^l y,
                    damp = exp(-0.5 4^l var);  fp32 rows: damp sin(x) | damp sin(fl32(x + kHalfPiF));  bf16 rows: damp sin(x) | damp cos(x)

Budgets, first-order propagation through those expressions with EVERY term absolute (for a difference the sum of the magnitudes):
    fence post      C_T u (fi s + (1 - s) ni)                  jittered: C_T u (lo + (up + lo) t_rand)
    mean            C_M u (|d_a| |t_mean| + |o_a|)
    cov             C_V u (T |d_a d_b| + R (delta_ab + |d_a d_b| / dn))
                    T = hw^2 / 3 + c4 hw^4 (12 mu^2 + hw^2) / den^2,  R = r^2 (mu^2 / 4 + c5 hw^2 + c4 hw^4 / den): t_var and r_var, absolute
    mean'           C_MC u |m_a| (2 + 1 / n) / n
    fused cov'      C_VF u (T |vv| + |t_var| Mvv + R (|jj| + |vv| / dn) + |r_var| (Mjj + Mvv / dn)),  vv = v_i v_j, |jj| = delta a^2 + |b^2 - a^2| |u_i u_j|
                    Ma = (2 n + 1) / n2, Mv_i = Ma |d_i| + (b + Ma) (sum |u_a d_a|) |u_i|, Mvv = Mv_i |v_j| + |v_i| Mv_j + |vv|,
                    Mjj = delta 2 |a| Ma + (2 b^2 + 2 |a| Ma + 2 |b^2 - a^2|) |u_i u_j|
    generic cov'    C_VG u sum_k (MT_ik |J_jk| + |T_ik| MJ_jk),  MJ_ij = Ma (delta_ij + |u_i u_j|) + b |u_i u_j|,  T = J C,  MT_ij = sum_k MJ_ik |C_kj|
    fp32 feature    C_F u |truth|  +  damp_hi 2^l dy  +  (damp_hi - damp_lo)            C_F = ipe_forward.C_F (libm; ceiling 15)
                    dy = C_P u sum_a |m_a p_a|,  dvar = C_P u sum_ab |cov_ab p_a p_b|,  damp_hi / damp_lo = damp at max(var - dvar, 0) / var + dvar:
                    an interval, not a derivative (0.5 4^l dvar need not be small)
    bf16 feature    2^(e-8) + E + the same phase and damping terms,  E = damp (2^-16 + 2 pi 2^-24),  e = floor(log2(|truth| + E + those terms))
                    2 pi 2^-24: the two-float reduction's bound in turns (kernels_360.hip, Ipe360Math<__bf16>); 2^-16: the requirement on the
                    hardware pair stated in ipe_forward.py
Each constant is twice the worst ratio at C = 1 of the HOST build of raymath360.hpp (tests/hostmath: g++ -O2 -ffp-contract=off) over the
whole fixture; test_ipe360_forward_cpu.py measures and prints them with the class and shape where they occur.  Never from a kernel.
MEASURED (host build, worst |got - truth| / budget at C = 1):
    fence post 2.31 (`far` 2x129) -> C_T = 4.7      mean 2.84 (`perpendicular` 2x129) -> C_M = 5.7      cov 5.47 (`typical` 3x21) -> C_V = 11.0
    mean' 2.40 (`far` 2x129) -> C_MC = 4.8           fused cov' 2.54 (`far` 3x21) -> C_VF = 5.1          generic cov' 2.67 (`far` 2x129) -> C_VG = 5.4
    fp32 feature 3.24 (`near` 2x129, degrees 3-19, a "cos" entry: the truth rounds x + kHalfPiF from the float64 x, the kernel from its fp32 x) -> C_P = 6.5
The bf16 emulation below reaches 0.993 of its budget, truncation in place of RNE 1.98.  On the MI355X every entry stays within 0.52 of
its budget (fp32 rows, Gaussians, fence posts) and 0.994 (bf16 rows), where the host build and the emulation are (DESIGN.md has the
per-class figures).

Two things the float64 budget cannot see, because they are smaller than the rounding it must grant y = p . mean (C_P u 2^l sum |m_a p_a| >=
6.5 u |x|): fp32 rows with the true cosine (at most u |x| of phase) and the bf16 reduction without its `lo` term (0.68 u |x|).
projection_truth below is the sharper, CPU-only criterion that sees both: truth at the fp32 projection the host build forms.
"""
import ctypes

import numpy as np

import ipe_forward as fw
from mipnerf_pl_amd.mlp_plan import bf16_round

F = np.float32
F8 = np.float64
U = fw.U
FLOOR = fw.FLOOR
HALF_PI_F = fw.HALF_PI_F
C4, C5, EPS_DN = fw.C4, fw.C5, fw.EPS_DN
C_F = fw.C_F
K_HI, K_LO = F(0.15915494), F(6.4206382e-09)         # Ipe360Math<__bf16>: 1 / 2 pi = hi + lo
EXP2_K = F(-0.72134752)                              # -0.5 log2(e)
MARGIN_N2 = 2.0 ** -18

C_T = 4.7
C_M = 5.7
C_V = 11.0
C_MC = 4.8
C_VF = 5.1
C_VG = 5.4
C_P = 6.5

# the 21 fp32 basis rows of raymath360.hpp (test_ipe360_forward_cpu.py compares them with the header's text)
BASIS = np.array([
    [0.8506508, 0., 0.5257311], [0.809017, 0.5, 0.309017], [0.5257311, 0.8506508, 0.], [1., 0., 0.],
    [0.809017, 0.5, -0.309017], [0.8506508, 0., -0.5257311], [0.309017, 0.809017, -0.5],
    [0., 0.5257311, -0.8506508], [0.5, 0.309017, -0.809017], [0., 1., 0.], [-0.5257311, 0.8506508, 0.],
    [-0.309017, 0.809017, -0.5], [0., 0.5257311, 0.8506508], [-0.309017, 0.809017, 0.5],
    [0.309017, 0.809017, 0.5], [0.5, 0.309017, 0.809017], [0.5, -0.309017, 0.809017], [0., 0., 1.],
    [-0.5, 0.309017, 0.809017], [-0.809017, 0.5, 0.309017], [-0.809017, 0.5, -0.309017]], F)
NB = 21

CLASSES = ("typical", "near", "straddle", "radial", "perpendicular", "unnormalised", "far")
SHAPES = ((1, 1), (3, 21), (1, 64), (5, 13), (2, 129))      # 63: one short of a workgroup tile; 64; 65; 258: one past a fragment tile
DEGREES = ((0, 16), (3, 19), (15, 31), (0, 8), (0, 6))      # shipped; shifted; scale 2^30; 21 vectors per half; only the per-direction kernel
CANARY = 64
LATTICE = dict(dims=(5, 4, 3), lo=(-1.7, -1.1, -0.6), hi=(1.9, 1.3, 1.25), first=7, count=47, cov_scale=1.5)


def deg_id(deg):
    return f"deg{deg[0]}-{deg[1]}"


def tiled(deg):
    """whether mipnerf_cast_ipe_360 takes the tiled kernel for an encoding-only call"""
    return (NB * (deg[1] - deg[0])) % 8 == 0


def case_seed(cls, B, N):
    return 360000 + 1000 * CLASSES.index(cls) + 7 * N + B


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def make(cls, B, N):
    """dict of fp32 operands: near, far [B], t_rand [B,N+1] (holds 0 and nextafter(1, 0)), o, d [B,3], r [B]"""
    assert cls in CLASSES
    rng = np.random.default_rng(case_seed(cls, B, N))
    o = rng.uniform(-0.5, 0.5, (B, 3))
    d = _unit(rng.standard_normal((B, 3))) * rng.uniform(0.8, 1.2, (B, 1))
    r = rng.uniform(5e-4, 4e-3, B)
    near, far = np.full(B, 0.2), rng.uniform(30.0, 1000.0, B)
    if cls == "near":                      # short, thin frusta well inside |x| < 1.5: the top degrees stay alive and their phase budgets small
        o = rng.uniform(-0.15, 0.15, (B, 3))
        d = _unit(d)
        near = rng.uniform(0.05, 0.3, B)
        far = near * (1.0 + 10.0 ** rng.uniform(-5.0, -3.5, B))
        r = 10.0 ** rng.uniform(-6.0, -5.0, B)
    if cls == "straddle":
        o = rng.uniform(-0.3, 0.3, (B, 3))
        near, far = np.full(B, 0.3), rng.uniform(2.0, 6.0, B)
    if cls == "radial":                    # d parallel to o: u is parallel to d
        axis = _unit(rng.standard_normal((B, 3)))
        o, d = axis * rng.uniform(0.1, 0.5, (B, 1)), axis * rng.uniform(0.8, 1.2, (B, 1))
    if cls == "perpendicular":             # d orthogonal to one basis direction
        p = BASIS[(5 * np.arange(B) + N) % NB].astype(F8)
        g = rng.standard_normal((B, 3))
        d = _unit(g - (g * p).sum(-1, keepdims=True) * p / (p * p).sum(-1, keepdims=True))
    if cls == "unnormalised":
        d = _unit(d) * rng.uniform(0.5, 2.0, (B, 1))
    if cls == "far":
        near, far = rng.uniform(50.0, 300.0, B), rng.uniform(500.0, 1000.0, B)
    t_rand = rng.uniform(0.0, 1.0, (B, N + 1)).astype(F)
    t_rand[0, 0], t_rand[-1, -1] = F(0), np.nextafter(F(1), F(0))
    c = lambda a: np.ascontiguousarray(a, F)
    return dict(near=c(near), far=c(far), t_rand=c(t_rand), o=c(o), d=c(d), r=c(r))


def sampler_operands(c):
    """(near, far, t_rand) of make()'s rays for the sampler, with one more ray whose near equals its far"""
    near, far = np.append(c["near"], F(2.5)), np.append(c["far"], F(2.5))
    return np.ascontiguousarray(near, F), np.ascontiguousarray(far, F), np.ascontiguousarray(np.vstack([c["t_rand"], c["t_rand"][:1]]), F)


def table():
    """hand-made Gaussians for mipnerf_gauss_360: means [M,3] x covs [M,3,3] fp32 -- |mean| in { inside, exactly 1, nextafter above 1, 2,
    30, 400 } on the directions (1,0,0) and (0.6,0.8,0) and on a generic one, times the scales { 1, 1 + 2^-3 } outside; covs { 0, a
    denormal, 1e-12, 1, anisotropic 1e-6 : 1 }.  Returns also the mask of the rows that must come back bit for bit (|mean|^2 <= 1)."""
    dirs = np.array([[1, 0, 0], [0.6, 0.8, 0], [0.36, -0.48, 0.8]], F8)
    means = []
    for u in dirs:
        for n in (0.25, 1.0, 2.0, 30.0, 400.0):
            for s in ((1.0,) if n <= 1 else (1.0, 1.125)):
                means.append((u * n * s).astype(F))
    for m in (np.array([1, 0, 0], F), np.array([0.6, 0.8, 0], F)):                                    # one component at nextafter above: must come back contracted
        for a in np.nonzero(m)[0]:
            q = m.copy()
            q[a] = np.nextafter(q[a], F(2))
            means.append(q)
    means = np.array(means, F)
    rot = np.array([[0.36, 0.48, -0.8], [-0.8, 0.6, 0.0], [0.48, 0.64, 0.6]], F8)
    covs = [np.zeros((3, 3)), np.eye(3) * 5e-43, np.eye(3) * 1e-12, np.eye(3), rot @ np.diag([1e-6, 1.0, 1.0]) @ rot.T,
            rot @ np.diag([1.0, 1e-6, 1e-6]) @ rot.T]
    covs = np.array([0.5 * (c + c.T) for c in covs]).astype(F)
    covs = np.maximum(covs, covs.transpose(0, 2, 1))   # symmetric bit for bit
    mm = np.repeat(means, len(covs), axis=0)
    cc = np.tile(covs, (len(means), 1, 1))
    return np.ascontiguousarray(mm), np.ascontiguousarray(cc)


# ---- host build of raymath360.hpp -----------------------------------------------------------------------------------------------------
def _host():
    return fw._host()


_p = fw._p


def host_sample(near, far, t_rand, N):
    """(t_inv, t) [B,N+1] fp32 of hm_sample_360; t_rand may be None"""
    B = near.shape[0]
    t_inv, t = np.empty((B, N + 1), F), np.empty((B, N + 1), F)
    _host().hm_sample_360(B, N, _p(near), _p(far), None if t_rand is None else _p(np.ascontiguousarray(t_rand, F)), _p(t_inv), _p(t))
    return t_inv, t


def host_cast(t, o, d, r, contracted, deg):
    """(mean [B,N,3], cov [B,N,3,3], rows [B,N,42L]) fp32 of hm_cast_ipe_360 (fused contraction when `contracted`)"""
    B, N = t.shape[0], t.shape[1] - 1
    L = deg[1] - deg[0]
    t0, t1 = np.ascontiguousarray(t[:, :-1]).ravel(), np.ascontiguousarray(t[:, 1:]).ravel()
    dd, oo, rr = np.repeat(d, N, axis=0), np.repeat(o, N, axis=0), np.repeat(r, N)
    mean, cov, enc = np.empty((B * N, 3), F), np.empty((B * N, 9), F), np.empty((B * N, 2 * NB * L), F)
    _host().hm_cast_ipe_360(B * N, _p(t0), _p(t1), _p(dd), _p(oo), _p(rr), int(bool(contracted)), deg[0], L, _p(mean), _p(cov), _p(enc))
    return mean.reshape(B, N, 3), cov.reshape(B, N, 3, 3), enc.reshape(B, N, -1)


def host_gauss(means, covs, contracted, deg):
    """(mean [M,3], cov [M,3,3], rows [M,42L]) fp32 of hm_gauss_360 (generic contraction when `contracted`)"""
    m, c = np.ascontiguousarray(means, F).reshape(-1, 3), np.ascontiguousarray(covs, F).reshape(-1, 9)
    L = deg[1] - deg[0]
    mo, co, enc = np.empty_like(m), np.empty_like(c), np.empty((m.shape[0], 2 * NB * L), F)
    _host().hm_gauss_360(m.shape[0], _p(m), _p(c), int(bool(contracted)), deg[0], L, _p(mo), _p(co), _p(enc))
    lead = np.shape(means)[:-1]
    return mo.reshape(lead + (3,)), co.reshape(lead + (3, 3)), enc.reshape(lead + (-1,))


def host_lattice(dims, lo, hi, first, count, cov_scale):
    """fp32 Gaussians (mean [count,3], cov [count,3,3]) of lattice points first .. first + count - 1 (hm_lattice_gauss_360)"""
    h = _host()
    h.hm_lattice_gauss_360.argtypes = [ctypes.c_void_p] * 3 + [ctypes.c_int, ctypes.c_int, ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p]
    mean, cov = np.empty((count, 3), F), np.empty((count, 9), F)
    h.hm_lattice_gauss_360(_p(np.array(dims, np.int32)), _p(np.array(lo, F)), _p(np.array(hi, F)), first, count, cov_scale, _p(mean), _p(cov))
    return mean, cov.reshape(count, 3, 3)


def host_linspace(N):
    h = _host()
    h.hm_linspace.argtypes = [ctypes.c_float, ctypes.c_float, ctypes.c_int, ctypes.c_void_p]
    out = np.empty(N + 1, F)
    h.hm_linspace(0.0, 1.0, N + 1, _p(out))
    return out


# ---- float64 truths and budgets -------------------------------------------------------------------------------------------------------
worst = fw.worst


def where_worst(got, truth, budget):
    """(ratio, flat index) of the worst entry"""
    r = np.abs(np.asarray(got, F8) - truth) / budget
    r = np.where(np.isfinite(np.asarray(got, F8)), r, np.inf)
    k = int(np.argmax(r))
    return float(r.ravel()[k]), k


def linspace_weights(N):
    """s_k = torch_linspace_at(0, 1, N + 1, k) in fp32: fma(step, k, 0) below the middle, fma(-step, N - k, 1) from it on"""
    steps = N + 1
    step = F8(F(1) / F(steps - 1))
    k = np.arange(steps)
    return np.where(k < steps // 2, (step * k).astype(F), (1.0 - step * (steps - 1 - k)).astype(F)).astype(F)


def posts_truth(near, far, t_rand, N):
    """dict(t_inv, mag) [B,N+1] float64; budget = C_T u mag + FLOOR"""
    s = linspace_weights(N).astype(F8)[None, :]
    ni, fi = 1.0 / near.astype(F8)[:, None], 1.0 / far.astype(F8)[:, None]
    post = fi * s + (1.0 - s) * ni
    if t_rand is None:
        return dict(t_inv=post, mag=post.copy())
    mid = 0.5 * (post[:, 1:] + post[:, :-1])
    lo, up = post.copy(), post.copy()
    lo[:, 1:], up[:, :-1] = mid, mid
    rr = t_rand.astype(F8)
    return dict(t_inv=lo + (up - lo) * rr, mag=lo + (up + lo) * rr)


def posts_budget(tr, c_t=None):
    return (C_T if c_t is None else c_t) * U * tr["mag"] + FLOOR


def reciprocal_ratio(t, t_inv):
    """worst |t - 1 / t_inv| / (u / t_inv + FLOOR): 1 / t_inv in float64 from the fp32 t_inv"""
    w = 1.0 / t_inv.astype(F8)
    return worst(t, w, U * np.abs(w) + FLOOR)


def _outer(a, b=None):
    b = a if b is None else b
    return a[..., :, None] * b[..., None, :]


EYE = np.eye(3)


def frustum_truth(t, o, d, r):
    """stage 2: dict of float64 arrays -- mean, mag_mean [B,N,3], cov, mag_cov [B,N,3,3], t_var, r_var, T, R [B,N], dn [B]"""
    t8, o8, d8 = t.astype(F8), o.astype(F8), d.astype(F8)
    t0, t1 = t8[:, :-1], t8[:, 1:]
    mu, hw = (t0 + t1) / 2, (t1 - t0) / 2
    mu2, hw2 = mu * mu, hw * hw
    hw4 = hw2 * hw2
    den = 3 * mu2 + hw2
    t_mean = mu + (2 * mu * hw2) / den
    t_var = hw2 / 3 - C4 * ((hw4 * (12 * mu2 - hw2)) / (den * den))
    T = hw2 / 3 + C4 * ((hw4 * (12 * mu2 + hw2)) / (den * den))
    r2 = (r.astype(F8) ** 2)[:, None]
    r_var = r2 * (mu2 / 4 + C5 * hw2 - C4 * hw4 / den)
    R = r2 * (mu2 / 4 + C5 * hw2 + C4 * hw4 / den)
    dn = (d8 * d8).sum(-1) + EPS_DN
    dd = _outer(d8)[:, None]                                       # [B,1,3,3]
    dnb = dn[:, None, None, None]
    e = lambda a: a[..., None, None]
    mean = d8[:, None, :] * t_mean[..., None] + o8[:, None, :]
    mag_mean = np.abs(d8)[:, None, :] * np.abs(t_mean)[..., None] + np.abs(o8)[:, None, :]
    cov = e(t_var) * dd + e(r_var) * (EYE - dd / dnb)
    mag_cov = e(T) * np.abs(dd) + e(R) * (EYE + np.abs(dd) / dnb)
    return dict(mean=mean, mag_mean=mag_mean, cov=cov, mag_cov=mag_cov, t_var=t_var, r_var=r_var, T=T, R=R, dn=dn, d=d8)


def _jacobian(m):
    """contract_jacobian in float64 at m [...,3]: dict(n2, n, u, a, b, Ma, ms, Mms)"""
    n2 = (m * m).sum(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        n = np.sqrt(n2)
        return dict(n2=n2, n=n, u=m / n[..., None], a=(2 * n - 1) / n2, b=1 / n2, Ma=(2 * n + 1) / n2, ms=(2 - 1 / n) / n, Mms=(2 + 1 / n) / n)


def fused_truth(m32, fr, margin=MARGIN_N2):
    """stage 3 from the fp32 uncontracted means m32 [B,N,3] and frustum_truth's dict: mean, mag_mean, cov, mag_cov and `out` (n2 > 1 in
    float64).  Rows with n2 <= 1: stage 2's truth and magnitudes (kind `cov`); the caller asserts their bits."""
    m = m32.astype(F8)
    j = _jacobian(m)
    assert np.abs(j["n2"] - 1.0).min() >= margin, "a frustum sample within 2^-18 of the unit sphere"
    out = j["n2"] > 1.0
    d = fr["d"][:, None, :]
    u, a, b, Ma = j["u"], j["a"][..., None], j["b"][..., None], j["Ma"][..., None]
    ud, Mud = (u * d).sum(-1, keepdims=True), np.abs(u * d).sum(-1, keepdims=True)
    v = a * d + ((b - a) * ud) * u
    Mv = Ma * np.abs(d) + ((b + Ma) * Mud) * np.abs(u)
    vv, uu = _outer(v), _outer(u)
    Mvv = _outer(Mv, np.abs(v)) + _outer(np.abs(v), Mv) + np.abs(vv)
    e = lambda x: x[..., None, None]
    a2, b2a2 = e(j["a"] ** 2), e(j["b"] ** 2 - j["a"] ** 2)
    Ma2 = e(2 * np.abs(j["a"]) * j["Ma"])
    jj, ajj = EYE * a2 + b2a2 * uu, EYE * a2 + np.abs(b2a2 * uu)
    Mjj = EYE * Ma2 + (2 * e(j["b"] ** 2) + Ma2 + 2 * np.abs(b2a2)) * np.abs(uu)
    dn = fr["dn"][:, None, None, None]
    tv, rv, T, R = e(fr["t_var"]), e(fr["r_var"]), e(fr["T"]), e(fr["R"])
    cov = tv * vv + rv * (jj - vv / dn)
    mag = T * np.abs(vv) + np.abs(tv) * Mvv + R * (ajj + np.abs(vv) / dn) + np.abs(rv) * (Mjj + Mvv / dn)
    o3, o33 = out[..., None], e(out)
    return dict(out=out, mean=np.where(o3, m * j["ms"][..., None], m), mag_mean=np.where(o3, np.abs(m) * j["Mms"][..., None], 0.0),
                cov=np.where(o33, cov, fr["cov"]), mag_cov=np.where(o33, mag, fr["mag_cov"]))


def generic_truth(mean32, cov32):
    """stage 4 at the given fp32 (mean [M,3], cov [M,3,3], symmetric): mean, mag_mean, cov, mag_cov, out"""
    m, C = mean32.astype(F8), cov32.astype(F8)
    j = _jacobian(m)
    out = n2_fp32(mean32) > F(1)
    safe = np.where(out[..., None], j["u"], 0.0)
    e = lambda x: np.where(out, x, 1.0)[..., None, None]
    uu = _outer(safe)
    a, b, Ma = e(j["a"]), e(j["b"]), e(j["Ma"])
    J = a * (EYE - uu) + b * uu
    MJ = Ma * (EYE + np.abs(uu)) + b * np.abs(uu)
    Tm = J @ C
    MT = MJ @ np.abs(C)
    cov = Tm @ J.swapaxes(-1, -2)
    mag = MT @ np.abs(J).swapaxes(-1, -2) + np.abs(Tm) @ MJ.swapaxes(-1, -2)
    o3, o33 = out[..., None], out[..., None, None]
    ms, Mms = np.where(out, j["ms"], 1.0)[..., None], np.where(out, j["Mms"], 0.0)[..., None]
    return dict(out=out, mean=np.where(o3, m * ms, m), mag_mean=np.abs(m) * Mms, cov=np.where(o33, cov, C), mag_cov=np.where(o33, mag, 0.0))


def n2_fp32(mean32):
    """the header's fp32 (mx mx + my my) + mz mz: what decides the branch of contract_gaussian"""
    m = np.ascontiguousarray(mean32, F)
    return (m[..., 0] * m[..., 0] + m[..., 1] * m[..., 1]) + m[..., 2] * m[..., 2]


def gauss_ratios(mean, cov, tr, c_mean, c_cov):
    return (worst(mean, tr["mean"], c_mean * U * tr["mag_mean"] + FLOOR), worst(cov, tr["cov"], c_cov * U * tr["mag_cov"] + FLOOR))


def _rows(a, b):
    """[..., L, 21] sin half and "cos" half -> [..., 42 L], index = half 21 L + l 21 + j"""
    lead = a.shape[:-2]
    return np.concatenate([a.reshape(lead + (-1,)), b.reshape(lead + (-1,))], -1)


def feature_truth(mean32, cov32, deg, c_p=None):
    """stage 5 at the fp32 (mean [...,3], cov [...,3,3]): dict of float64 [..., 42 L] -- f32, bf16 (truths), bud_f32, bud_bf16, damp, and the
    parts libm, phase, interval of the fp32 budget"""
    c_p = C_P if c_p is None else c_p
    m, C, P = mean32.astype(F8), cov32.astype(F8), BASIS.astype(F8)
    y, My = m @ P.T, np.abs(m) @ np.abs(P).T                                          # [...,21]
    var = np.einsum("...ab,ja,jb->...j", C, P, P)
    Mvar = np.einsum("...ab,ja,jb->...j", np.abs(C), np.abs(P), np.abs(P))
    scale = (2.0 ** np.arange(deg[0], deg[1]))[:, None]                                # [L,1]
    k = 0.5 * scale * scale
    x = y[..., None, :] * scale
    dy, dvar = c_p * U * My[..., None, :], c_p * U * Mvar[..., None, :]
    v = var[..., None, :]
    damp, hi, lo = np.exp(-k * v), np.exp(-k * np.minimum(v, np.maximum(v - dvar, 0.0))), np.exp(-k * (v + dvar))
    xc = (x + HALF_PI_F).astype(F).astype(F8)
    f32 = _rows(damp * np.sin(x), damp * np.sin(xc))
    b16 = _rows(damp * np.sin(x), damp * np.cos(x))
    phase = _rows(hi * scale * dy, hi * scale * dy)
    interval = _rows(hi - lo, hi - lo)
    damp2 = _rows(damp, damp)
    libm = C_F * U * np.abs(f32)
    E = damp2 * (2.0 ** -16 + 2 * np.pi * 2.0 ** -24)
    rest = E + phase + interval
    with np.errstate(divide="ignore"):
        e = np.floor(np.log2(np.abs(b16) + rest))
    return dict(f32=f32, bf16=b16, damp=damp2, libm=libm, phase=phase, interval=interval, bud_f32=libm + phase + interval + FLOOR,
                bud_bf16=2.0 ** (e - 8) + rest + FLOOR)


def informative(truth, budget):
    return budget <= np.maximum(np.abs(truth) / 4, 2.0 ** -12)


def lattice_truth(dims, lo, hi, first, count, cov_scale):
    """(lo + i h, diag(cov_scale h^2 / 12)) in float64 from the fp32 lo, hi, cov_scale: mean, mag_mean [count,3], var [count,3]"""
    lo8, hi8, cs = np.array(lo, F).astype(F8), np.array(hi, F).astype(F8), float(F(cov_scale))
    p = first + np.arange(count)
    row = p // dims[0]
    idx = np.stack([p - row * dims[0], row % dims[1], row // dims[1]], -1)
    h = (hi8 - lo8) / (np.array(dims) - 1)
    return dict(mean=lo8 + idx * h, mag_mean=np.abs(lo8) + idx * (np.abs(hi8) + np.abs(lo8)) / (np.array(dims) - 1),
                var=np.broadcast_to(cs * h * h / 12, (count, 3)))


def frag_index(s, f, width):
    """enc360_index of kernels_360.hip: where feature f of sample s lies in a fragment buffer of `width` features per sample"""
    return ((s >> 5) * (width >> 4) + (f >> 4)) * 512 + ((f >> 3) & 1) * 256 + (s & 31) * 8 + (f & 7)


def rows_of_fragments(flat, M, width):
    """[ceil(M / 256) * 256, width] rows read back from a flat fragment buffer"""
    Mp = -(-M // 256) * 256
    s, f = np.meshgrid(np.arange(Mp), np.arange(width), indexing="ij")
    idx = frag_index(s, f, width)
    assert np.array_equal(np.sort(idx.ravel()), np.arange(Mp * width)), "the fragment layout is a permutation of the buffer"
    return flat[idx]


# ---- numpy emulations (fp32 operation by operation in the header's order) and their mutations -------------------------------------------
SAMPLE_MUTATIONS = ("t_unjittered",)
GAUSS_MUTATIONS = ("t_var_perp", "swap_ab", "mean_scale", "dn", "xy_to_xz")
GENERIC_MUTATIONS = ("jacobian_only", "swap_ab", "mean_scale")
FEATURE_MUTATIONS = ("basis_negated", "wrap_direction", "damp_2l", "cos_next_degree", "true_cos")
BF16_MUTATIONS = ("no_lo", "truncate")


def emulate_sample(near, far, t_rand, N, mutation=None):
    assert mutation is None or mutation in SAMPLE_MUTATIONS
    s = linspace_weights(N)[None, :]
    ni, fi = (F(1) / near)[:, None], (F(1) / far)[:, None]
    post = fi * s + (F(1) - s) * ni
    ti = post
    if t_rand is not None:
        lo, up = post.copy(), post.copy()
        lo[:, 1:] = F(0.5) * (post[:, 1:] + post[:, :-1])
        up[:, :-1] = F(0.5) * (post[:, 1:] + post[:, :-1])
        ti = lo + (up - lo) * t_rand
    t = F(1) / (post if mutation == "t_unjittered" else ti)
    assert ti.dtype == F and t.dtype == F
    return ti, t


def _sym(upper):
    """dict {(i,j): [...]} of the upper triangle -> [...,3,3]"""
    return np.stack([np.stack([upper[(min(i, j), max(i, j))] for j in range(3)], -1) for i in range(3)], -2)


def _emu_jacobian(m, n2, mutation):
    n = np.sqrt(n2)
    u = m / n[..., None]
    a, b = (F(2) * n - F(1)) / n2, F(1) / n2
    ms = (F(2) - F(1) / n) if mutation == "mean_scale" else (F(2) - F(1) / n) / n
    if mutation == "swap_ab":
        a, b = b, a
    return u, a, b, ms


def emulate_cast(t, o, d, r, contracted, mutation=None):
    """conical_frustum_to_gaussian_full: (mean [B,N,3], cov [B,N,3,3]) fp32"""
    assert mutation is None or mutation in GAUSS_MUTATIONS
    t0, t1 = t[:, :-1], t[:, 1:]
    mu, hw = (t0 + t1) / F(2), (t1 - t0) / F(2)
    mu2, hw2 = mu * mu, hw * hw
    hw4 = hw2 * hw2
    den = F(3) * mu2 + hw2
    t_mean = mu + (F(2) * mu * hw2) / den
    t_var = hw2 / F(3) - F(C4) * ((hw4 * (F(12) * mu2 - hw2)) / (den * den))
    r_var = (r * r)[:, None] * (mu2 / F(4) + F(C5) * hw2 - F(C4) * hw4 / den)
    p_var = t_var if mutation == "t_var_perp" else r_var
    dd = d * d
    dn = ((dd[:, 0] + dd[:, 1]) + dd[:, 2]) + F(1e-10)
    if mutation == "dn":
        dn = np.full_like(dn, F(1) + F(1e-10))
    dn = dn[:, None]
    db = np.broadcast_to(d[:, None, :], (t0.shape[0], t0.shape[1], 3))
    mean = db * t_mean[..., None] + o[:, None, :]
    n2 = (mean[..., 0] * mean[..., 0] + mean[..., 1] * mean[..., 1]) + mean[..., 2] * mean[..., 2]
    plain, fused = {}, {}
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        u, a, b, ms = _emu_jacobian(mean, n2, mutation)
        ud = (u[..., 0] * db[..., 0] + u[..., 1] * db[..., 1]) + u[..., 2] * db[..., 2]
        v = a[..., None] * db + ((b - a) * ud)[..., None] * u
        a2 = a * a
        b2a2 = b * b - a2
        for i in range(3):
            for j in range(i, 3):
                dij = db[..., i] * db[..., j]
                plain[(i, j)] = t_var * dij + p_var * ((F(1) if i == j else F(0)) - dij / dn)
                vv = v[..., i] * v[..., j]
                jj = (a2 if i == j else F(0)) + b2a2 * (u[..., i] * u[..., j])
                fused[(i, j)] = t_var * vv + p_var * (jj - vv / dn)
        if mutation == "xy_to_xz":
            for c in (plain, fused):
                c[(0, 2)] = c[(0, 1)]
        plain, fused = _sym(plain), _sym(fused)
        if not contracted:
            return mean, plain
        out = n2 > F(1)
        mean_c = np.where(out[..., None], mean * ms[..., None], mean)
        cov_c = np.where(out[..., None, None], fused, plain)
    assert mean_c.dtype == F and cov_c.dtype == F
    return mean_c, cov_c


def emulate_generic(mean, cov, mutation=None):
    """contract_gaussian on (mean [M,3], cov [M,3,3]) fp32"""
    assert mutation is None or mutation in GENERIC_MUTATIONS
    n2 = (mean[..., 0] * mean[..., 0] + mean[..., 1] * mean[..., 1]) + mean[..., 2] * mean[..., 2]
    out = n2 > F(1)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        u, a, b, ms = _emu_jacobian(mean, n2, mutation)
        J = [[None] * 3 for _ in range(3)]
        for i in range(3):
            for j in range(3):
                uu = u[..., i] * u[..., j]
                J[i][j] = a * ((F(1) if i == j else F(0)) - uu) + b * uu
        C = [[cov[..., min(i, j), max(i, j)] for j in range(3)] for i in range(3)]
        T = [[(J[i][0] * C[0][j] + J[i][1] * C[1][j]) + J[i][2] * C[2][j] for j in range(3)] for i in range(3)]
        up = {(i, j): (T[i][0] * J[j][0] + T[i][1] * J[j][1]) + T[i][2] * J[j][2] for i in range(3) for j in range(i, 3)}
        if mutation == "jacobian_only":
            up = {(i, j): J[i][j] for i in range(3) for j in range(i, 3)}
        cov_c = np.where(out[..., None, None], _sym(up), _sym({(i, j): C[i][j] for i in range(3) for j in range(i, 3)}))
        mean_c = np.where(out[..., None], mean * ms[..., None], mean)
    assert mean_c.dtype == F and cov_c.dtype == F
    return mean_c, cov_c


def emulate_project(mean, cov, basis=BASIS):
    """project_360 for the 21 directions: (y, var) [...,21] fp32"""
    px, py, pz = basis[:, 0], basis[:, 1], basis[:, 2]
    m, c = mean[..., None, :], cov[..., None, :, :]
    y = (m[..., 0] * px + m[..., 1] * py) + m[..., 2] * pz
    cx = (c[..., 0, 0] * px + c[..., 0, 1] * py) + c[..., 0, 2] * pz
    cy = (c[..., 0, 1] * px + c[..., 1, 1] * py) + c[..., 1, 2] * pz
    cz = (c[..., 0, 2] * px + c[..., 1, 2] * py) + c[..., 2, 2] * pz
    var = (cx * px + cy * py) + cz * pz
    assert y.dtype == F and var.dtype == F
    return y, var


def _projected(mean, cov, deg, mutation):
    basis = BASIS.copy()
    if mutation == "basis_negated":
        basis[7] = -basis[7]
    y, var = emulate_project(mean, cov, basis)
    L = deg[1] - deg[0]
    scale = (2.0 ** np.arange(deg[0], deg[1])).astype(F)[:, None]
    with np.errstate(over="ignore", invalid="ignore"):
        ys = y[..., None, :] * scale
        vs = var[..., None, :] * (scale if mutation == "damp_2l" else scale * scale)
    if mutation == "wrap_direction":
        # the tiled kernel's vector of eight features (l0, j0 ..): past direction 20 the next degree starts -- with direction j0 + i - 20
        f = np.arange(L * NB)
        wrapped = (f // 8 * 8) % NB + f % 8 >= NB
        l, j = f // NB, f % NB
        jm = np.where(wrapped, (j + 1) % NB, j)
        ys = (y[..., jm] * scale[l, 0]).reshape(ys.shape)
        with np.errstate(over="ignore"):
            vs = (var[..., jm] * (scale[l, 0] * scale[l, 0])).reshape(vs.shape)
    return ys, vs


def projection_truth(mean, cov, deg):
    """The sharper, CPU-only criterion: truth and budgets at the fp32 projection (ys, vs) the host build forms (emulate_project restates it
    bit for bit with -ffp-contract=off; a device compiler may contract it, so the GPU test does not use this).  With the phase an exact
    operand the budgets are those of ipe_forward: C_F u |truth| for the fp32 rows, 2^(e-8) + E for the bf16 rows.  It sees what the
    float64 budget cannot: an error of the order of u |x|, which is below the conditioning of y = p . mean."""
    ys, vs = _projected(mean, cov, deg, None)
    x, k = ys.astype(F8), vs.astype(F8)
    damp = np.exp(-0.5 * k)
    f32 = _rows(damp * np.sin(x), damp * np.sin((ys + F(HALF_PI_F)).astype(F8)))
    b16 = _rows(damp * np.sin(x), damp * np.cos(x))
    E = _rows(damp, damp) * (2.0 ** -16 + 2 * np.pi * 2.0 ** -24)
    with np.errstate(divide="ignore"):
        e = np.floor(np.log2(np.abs(b16) + E))
    return dict(f32=f32, bf16=b16, bud_f32=C_F * U * np.abs(f32) + FLOOR, bud_bf16=2.0 ** (e - 8) + E + FLOOR)


def emulate_features(mean, cov, deg, mutation=None):
    """the fp32 rows [..., 42 L]: fp32 projection and scalings, fp32 phase add, correctly rounded fp32 exp and sin, fp32 product"""
    assert mutation is None or mutation in FEATURE_MUTATIONS
    ys, vs = _projected(mean, cov, deg, mutation)
    with np.errstate(over="ignore", invalid="ignore"):
        damp = np.exp((F(-0.5) * vs).astype(F8)).astype(F)
        yc = ys * F(2) if mutation == "cos_next_degree" else ys
        cs = np.cos(yc.astype(F8)).astype(F) if mutation == "true_cos" else np.sin((yc + F(HALF_PI_F)).astype(F8)).astype(F)
        out = _rows(damp * np.sin(ys.astype(F8)).astype(F), damp * cs)
    assert out.dtype == F
    return out


def emulate_bf16(mean, cov, deg, mutation=None):
    """the bf16 rows (as fp32 values): the two-float reduction with its fma, exact sine of the reduced phase and exact exp2 (each rounded
    to fp32), fp32 product, RNE to bf16"""
    assert mutation is None or mutation in BF16_MUTATIONS
    ys, vs = _projected(mean, cov, deg, None)
    with np.errstate(over="ignore", invalid="ignore"):
        x8 = ys.astype(F8)
        p = ys * K_HI
        e = (x8 * F8(K_HI) - p.astype(F8)).astype(F)            # fma(x, hi, -p): exact
        t = e if mutation == "no_lo" else (x8 * F8(K_LO) + e.astype(F8)).astype(F)
        rf = (p - np.rint(p)) + t
        sn = np.sin(2 * np.pi * rf.astype(F8)).astype(F)
        cs = np.sin(2 * np.pi * (rf + F(0.25)).astype(F8)).astype(F)
        damp = np.exp2((vs * EXP2_K).astype(F8)).astype(F)
        out = _rows(damp * sn, damp * cs)
    assert out.dtype == F
    if mutation == "truncate":
        return (out.view(np.uint32) & np.uint32(0xFFFF0000)).view(F)
    return bf16_round(out)
