"""Fixture of the compositing backward's Jacobian probes (numpy only, no kernel runs here): ray classes, upstream-gradient probes, the
float64 truth of every d_raw / d_t entry from the kernel's own fp32 operands, a running-error budget per entry, and an fp32 emulation of
k_volumetric_rendering_bwd (csrc/kernels_train.hip) from which the budget's one constant is taken.

The backward is linear in the upstream gradients (g_rgb, g_dist, g_acc, g_w), so a probe drives it with one kind at a time.  Every entry
is compared on its own: nothing is normalised by the largest gradient of a batch, so the samples of empty space, behind a surface and
of saturated colour count like any other.

    delta_i = (t_{i+1} - t_i) |d|     x_i = sigma_i delta_i     cum_i = sum_{j<i} x_j     T_i = exp(-cum_i)
    alpha_i = -expm1(-x_i)            w_i = alpha_i T_i         T1_i = exp(-(cum_i + x_i))
    G_i  = sum_c g_rgb_c c_ic - [white] sum_c g_rgb_c + g_acc + gd tmid_i + g_w_i        (gd = g_dist iff t_0 < distance < t_N)
    dx_i = G_i T1_i - sum_{k>i} G_k w_k
    d_raw.w_i = delta_i dx_i (-expm1(-sigma_i))
    d_raw.c_i = w_i g_rgb_c (1 + 2p) s (1 - s),   s = (c + p) / (1 + 2p),   p = fl32(0.001)
    d_t[i]    = |d| (a_{i-1} - a_i) + (h_{i-1} + h_i) + [i = 0] gd_lo + [i = N] gd_hi,   a_i = sigma_i dx_i,   h_i = gd w_i / 2

Budget (units of u = 2^-24; a bound on the rounding the kernel's fp32 evaluation order can accumulate, not a tolerance):
    Gabs_i   = sum of the absolute values of the terms of G_i
    growth_i = 2 + cum_i                       the kernel rounds cum_i to fp32 before expf: T_i carries cum_i u, expf its own ulps
    dxmag_i  = Gabs_i T1_i (growth_i + x_i) + sum_{k>i} Gabs_k (w_k growth_k + T_k)
               alpha = 1 - expf(-x) carries an ABSOLUTE rounding of one ulp of 1, which enters w_k as T_k
    mag_i    = delta_i fac_i dxmag_i,          fac_i = -expm1(-sigma_i)
    budget_w = C u (4 |truth| + mag_i) + 2^-120
    budget_c = C u |truth| (growth_i + 1 / alpha_i + 1 / min(s, 1 - s)) + 2^-120
    budget_t = C u (4 (sum of the absolute values of the terms of d_t[i]) + |d| (sigma dxmag)_{i-1, i} + |gd| / 2 (w growth + T)_{i-1, i}) + 2^-120
The 2^-120 floor covers subnormal transmittances."""
import numpy as np

F = np.float32
U = 2.0 ** -24
FLOOR = 2.0 ** -120
PAD = F(0.001)                     # rgb_padding of the shipped config
# The constant of the budgets.  With C = 1 the fp32 emulation below (emulate(), double scans, the kernel's operation order, numpy's expf /
# expm1f) measures over every class, probe and N of SIZES at B = 18 (test_ray_jacobian_cpu.py prints them):
#     worst |emulation - truth| / budget:   d_raw.w 2.06    d_raw.c 2.19    d_t 2.08
# C = 4 = that worst ratio of about 2, times 2 for the 1-2 ulp by which the device's expf / expm1f may differ from numpy's.  It comes
# from the emulation, never from the kernel under test.
C_BUDGET = 4.0

CLASSES = ("empty", "soft", "opaque", "surface", "saturated")
SIZES = (1, 5, 64, 65, 129, 300, 513)          # lane buckets K = 1, 1, 1, 2, 4, 8, 16
RAYS = 18                                      # not a multiple of the 4 rays of a workgroup
CLAMP_MARGIN = 1e-5


def lane_bucket(N):
    """csrc/lane_buckets.hpp: the smallest K in 1, 2, 4, ... with 64 K >= N"""
    K = 1
    while 64 * K < N:
        K *= 2
    return K


def sigmoid32(r):
    r = np.asarray(r, F)
    return F(1) / (F(1) + np.exp(-r))


def softplus32(x):
    """torch.nn.Softplus(beta=1, threshold=20) in fp32, as raymath.hpp density_activation"""
    x = np.asarray(x, F)
    return np.where(x > F(20), x, np.log1p(np.exp(np.minimum(x, F(20))))).astype(F)


def rgb_activation32(r):
    return (sigmoid32(r) * (F(1) + F(2) * PAD) - PAD).astype(F)


def make(cls, B, N, rng):
    """rgb_sigma [B,N,4], t [B,N+1], dirs [B,3] (fp32) of one ray class: activated values the activations can really produce"""
    assert cls in CLASSES
    while True:                                 # fp32 rounding can merge two of N + 1 sorted draws: draw again
        t = np.sort(rng.uniform(2.0, 6.0, (B, N + 1)), axis=-1).astype(F)
        if np.all(np.diff(t, axis=-1) > 0):
            break
    d = rng.standard_normal((B, 3))
    d *= rng.uniform(0.8, 1.3, (B, 1)) / np.linalg.norm(d, axis=-1, keepdims=True)
    dirs = d.astype(F)
    r = rng.normal(0.0, 2.5, (B, N, 3))
    i = np.arange(N)[None, :]
    h = rng.integers(0, N, (B, 1))
    x_empty = rng.uniform(-20.0, -8.0, (B, N))
    if cls == "empty":
        x = x_empty
    elif cls in ("soft", "saturated"):
        x = rng.normal(0.0, 2.5, (B, N))
        if cls == "saturated":
            r = rng.choice([9.0, -9.0, 14.0, -14.0], (B, N, 3)) + rng.normal(0.0, 0.5, (B, N, 3))
    elif cls == "opaque":
        x = np.where(i < h, x_empty, rng.uniform(50.0, 500.0, (B, N)))
    else:
        x = np.where(i < h, x_empty, np.minimum(-6.0 + 3.0 * (i - h), 200.0))
    rgb_sigma = np.concatenate([rgb_activation32(r.astype(F)), softplus32(x.astype(F))[..., None]], axis=-1).astype(F)
    check_inputs(rgb_sigma, t, dirs)
    return np.ascontiguousarray(rgb_sigma), np.ascontiguousarray(t), np.ascontiguousarray(dirs)


def check_inputs(rgb_sigma, t, dirs):
    """the conditions every case of this fixture meets: finite operands, strictly increasing t in [2, 6], |d| in [0.8, 1.3], densities > 0,
    colours strictly inside the sigmoid's range"""
    assert rgb_sigma.dtype == F and t.dtype == F and dirs.dtype == F
    assert np.isfinite(rgb_sigma).all() and np.isfinite(t).all() and np.isfinite(dirs).all()
    assert np.all(np.diff(t, axis=-1) > 0) and t.min() >= 2.0 and t.max() <= 6.0
    dn = np.linalg.norm(dirs.astype(np.float64), axis=-1)
    assert np.all(dn >= 0.8) and np.all(dn <= 1.3)
    assert np.all(rgb_sigma[..., 3] > 0)
    s = _s_of(rgb_sigma[..., :3].astype(np.float64))
    assert np.all(s > 0) and np.all(s < 1)


def _s_of(c):
    p = float(PAD)
    return (c + p) / (1.0 + 2.0 * p)


def _excl_prefix(v):
    return np.concatenate([np.zeros_like(v[:, :1]), np.cumsum(v, axis=-1)[:, :-1]], axis=-1)


def _excl_suffix(v):
    return _excl_prefix(v[:, ::-1])[:, ::-1]


# ---- probes ---------------------------------------------------------------------------------------------------------------------------
def onehot_indices(B, N):
    """one index per ray, cycling through both ends of lane 0's share, the middle and the last sample"""
    K = lane_bucket(N)
    cand = [min(max(i, 0), N - 1) for i in (0, K - 1, K, N // 2, N - 1)]
    return np.array([cand[b % len(cand)] for b in range(B)])


def probes(B, N, rng):
    """[(name, white_bkgd, dict(g_rgb [B,3], g_dist [B], g_acc [B], g_w [B,N]; None = not driven))]"""
    idx = onehot_indices(B, N)
    g_w = np.zeros((B, N), F)
    g_w[np.arange(B), idx] = 1
    unit = np.zeros((B, 3), F)
    unit[np.arange(B), np.arange(B) % 3] = 1
    none = dict(g_rgb=None, g_dist=None, g_acc=None, g_w=None)
    mixed = dict(g_rgb=rng.standard_normal((B, 3)).astype(F), g_dist=rng.standard_normal(B).astype(F),
                 g_acc=rng.standard_normal(B).astype(F), g_w=rng.standard_normal((B, N)).astype(F))
    return [("onehot", 0, dict(none, g_w=g_w)),
            ("acc", 0, dict(none, g_acc=np.ones(B, F))),
            ("rgb", 0, dict(none, g_rgb=unit)),
            ("rgb", 1, dict(none, g_rgb=unit)),
            ("dist", 0, dict(none, g_dist=np.ones(B, F))),
            ("mixed", 0, mixed),
            ("mixed", 1, mixed)]


def zero_filled(g, B, N):
    """the same probe with zero tensors in place of the pointers that are not driven"""
    shapes = dict(g_rgb=(B, 3), g_dist=(B,), g_acc=(B,), g_w=(B, N))
    return {k: np.zeros(shapes[k], F) if v is None else v for k, v in g.items()}


# ---- float64 truth and budgets --------------------------------------------------------------------------------------------------------
class Ray:
    """float64 quantities of the forward, from the fp32 operands widened to double"""

    def __init__(self, rgb_sigma, t, dirs):
        f8 = np.float64
        self.c, self.sigma = rgb_sigma[..., :3].astype(f8), rgb_sigma[..., 3].astype(f8)
        t = t.astype(f8)
        self.t0, self.tN = t[:, 0], t[:, -1]
        self.dn = np.sqrt((dirs.astype(f8) ** 2).sum(-1))
        self.delta = (t[:, 1:] - t[:, :-1]) * self.dn[:, None]
        self.x = self.sigma * self.delta
        self.cum = _excl_prefix(self.x)
        self.T = np.exp(-self.cum)
        self.alpha = -np.expm1(-self.x)
        self.w = self.alpha * self.T
        self.T1 = np.exp(-(self.cum + self.x))
        self.tmid = 0.5 * (t[:, 1:] + t[:, :-1])
        self.fac = -np.expm1(-self.sigma)
        self.s = _s_of(self.c)
        self.growth = 2.0 + self.cum
        self.distance = (self.w * self.tmid).sum(-1)
        self.inside = (self.distance > self.t0) & (self.distance < self.tN)
        self.below = self.distance < self.t0
        self.above = self.distance > self.tN

    def clamp_margin(self):
        """the smallest relative gap between a ray's distance and a clamp bound"""
        return float(np.minimum(np.abs(self.distance - self.t0) / self.t0, np.abs(self.distance - self.tN) / self.tN).min())


def truth(ray, white, g_rgb=None, g_dist=None, g_acc=None, g_w=None, c_budget=C_BUDGET):
    """dict(d_raw [B,N,4], d_t [B,N+1], budget_raw [B,N,4], budget_t [B,N+1], absterms [B,N]) in float64"""
    f8 = np.float64
    B, N = ray.x.shape
    if g_dist is not None:
        assert ray.clamp_margin() > CLAMP_MARGIN, "a ray's distance sits on a clamp bound: the gradient's support is ill-defined"
    gr = np.zeros((B, 3)) if g_rgb is None else g_rgb.astype(f8)
    ga = np.zeros(B) if g_acc is None else g_acc.astype(f8)
    gdist = np.zeros(B) if g_dist is None else g_dist.astype(f8)
    gw = np.zeros((B, N)) if g_w is None else g_w.astype(f8)
    gd = np.where(ray.inside, gdist, 0.0)
    gd_lo, gd_hi = np.where(ray.below, gdist, 0.0), np.where(ray.above, gdist, 0.0)
    terms = [gr[:, None, c] * ray.c[..., c] for c in range(3)]
    if white:
        terms += [-gr[:, None, c] * np.ones((1, N)) for c in range(3)]
    terms += [ga[:, None] * np.ones((1, N)), gd[:, None] * ray.tmid, gw]
    G = sum(terms)
    Gabs = sum(np.abs(v) for v in terms)
    dx = G * ray.T1 - _excl_suffix(G * ray.w)
    d_w = ray.delta * dx * ray.fac
    p = float(PAD)
    d_c = ray.w[..., None] * gr[:, None, :] * (1.0 + 2.0 * p) * ray.s * (1.0 - ray.s)
    werr = ray.w * ray.growth + ray.T                         # rounding of w_k in units of u
    dxmag = Gabs * ray.T1 * (ray.growth + ray.x) + _excl_suffix(Gabs * werr)
    mag = ray.delta * ray.fac * dxmag
    cu = c_budget * U
    budget_w = cu * (4.0 * np.abs(d_w) + mag) + FLOOR
    cond_c = ray.growth + 1.0 / ray.alpha
    budget_c = cu * np.abs(d_c) * (cond_c[..., None] + 1.0 / np.minimum(ray.s, 1.0 - ray.s)) + FLOOR
    # the terms of dx_i without their cancellation: the scale of an independent float64 evaluation's own rounding
    absterms = ray.delta * ray.fac * (Gabs * ray.T1 + _excl_suffix(Gabs * ray.w))

    def fence(v):                                             # v_{i-1} + v_i on the N + 1 fence posts
        z = np.zeros((B, 1))
        return np.concatenate([z, v], -1) + np.concatenate([v, z], -1)
    a = ray.sigma * dx * ray.dn[:, None]
    h = 0.5 * gd[:, None] * ray.w
    z = np.zeros((B, 1))
    d_t = (np.concatenate([z, a], -1) - np.concatenate([a, z], -1)) + fence(h)
    d_t[:, 0] += gd_lo
    d_t[:, N] += gd_hi
    t_abs = fence(np.abs(a) + np.abs(h))
    t_abs[:, 0] += np.abs(gd_lo)
    t_abs[:, N] += np.abs(gd_hi)
    t_mag = fence(ray.dn[:, None] * ray.sigma * dxmag + 0.5 * np.abs(gd)[:, None] * werr)
    budget_t = cu * (4.0 * t_abs + t_mag) + FLOOR
    absterms_t = fence(ray.dn[:, None] * ray.sigma * (Gabs * ray.T1 + _excl_suffix(Gabs * ray.w)) + np.abs(h))
    return dict(d_raw=np.concatenate([d_c, d_w[..., None]], -1), d_t=d_t, budget_raw=np.concatenate([budget_c, budget_w[..., None]], -1),
                budget_t=budget_t, absterms=absterms, absterms_t=absterms_t, gd=gd)


def ratios(d_raw, d_t, tr):
    """worst |got - truth| / budget of the density entries, the colour entries and the fence posts (d_t may be None)"""
    e = np.abs(d_raw.astype(np.float64) - tr["d_raw"]) / tr["budget_raw"]
    out = dict(w=float(e[..., 3].max()), c=float(e[..., :3].max()))
    if d_t is not None:
        out["t"] = float((np.abs(d_t.astype(np.float64) - tr["d_t"]) / tr["budget_t"]).max())
    return out


# ---- fp32 emulation of k_volumetric_rendering_bwd ----------------------------------------------------------------------------------
def emulate(rgb_sigma, t, dirs, white, g_rgb=None, g_dist=None, g_acc=None, g_w=None, cancelling_factor=False):
    """The kernel's arithmetic in numpy fp32, expression by expression, with its scans in double (their association differs from the
    wavefront's, which moves a double sum by 1e-16).  cancelling_factor: d softplus as 1 - expf(-sigma), the form this kernel had before
    density_activation_grad.  Returns d_raw [B,N,4], d_t [B,N+1] in fp32."""
    f8 = np.float64
    B, N = rgb_sigma.shape[:2]
    c, sig = rgb_sigma[..., :3], rgb_sigma[..., 3]
    dx_, dy_, dz_ = dirs[:, 0], dirs[:, 1], dirs[:, 2]
    dn = np.sqrt(dx_ * dx_ + dy_ * dy_ + dz_ * dz_)[:, None]
    t0, t1 = t[:, :-1], t[:, 1:]
    delta = (t1 - t0) * dn
    xx = sig * delta
    cum = _excl_prefix(xx.astype(f8))
    ex = np.exp(-xx)
    trans = np.exp(-cum.astype(F))
    w = (F(1) - ex) * trans
    T1 = trans * ex
    tmid = F(0.5) * (t0 + t1)
    zB = np.zeros(B, F)
    gr = np.zeros((B, 3), F) if g_rgb is None else g_rgb
    ga = zB if g_acc is None else g_acc
    gw = np.zeros((B, N), F) if g_w is None else g_w
    gd = gd_lo = gd_hi = zB
    if g_dist is not None:
        dsum = (w * tmid).astype(f8).sum(-1).astype(F)
        tn, tf = t[:, 0], t[:, -1]
        gd = np.where((dsum >= tn) & (dsum <= tf), g_dist, F(0))
        gd_lo, gd_hi = np.where(dsum < tn, g_dist, F(0)), np.where(dsum > tf, g_dist, F(0))
    bg = (gr[:, 0] + gr[:, 1]) + gr[:, 2] if white else zB
    G = gr[:, None, 0] * c[..., 0] + gr[:, None, 1] * c[..., 1] + gr[:, None, 2] * c[..., 2] - bg[:, None] + ga[:, None] \
        + gd[:, None] * tmid + gw
    suf = _excl_suffix((G * w).astype(f8))
    dxk = G * T1 - suf.astype(F)
    dsig = delta * dxk
    sc = F(1) + F(2) * PAD
    s = (c + PAD) / sc
    o_c = w[..., None] * gr[:, None, :] * sc * s * (F(1) - s)
    fac = (F(1) - np.exp(-sig)) if cancelling_factor else -np.expm1(-sig)
    o_w = dsig * fac
    a = sig * dxk * dn
    h = F(0.5) * gd[:, None] * w
    z = np.zeros((B, 1), F)
    d_t = (np.concatenate([z, a], -1) - np.concatenate([a, z], -1)) + (np.concatenate([z, h], -1) + np.concatenate([h, z], -1))
    d_t[:, 0] += gd_lo
    d_t[:, N] += gd_hi
    d_raw = np.concatenate([o_c, o_w[..., None]], -1)
    assert d_raw.dtype == F and d_t.dtype == F
    return d_raw, d_t


# ---- one sample per ray, from the raw density on ---------------------------------------------------------------------------------------
FROM_RAW_RAYS = 512
FROM_RAW_BIAS = -1.0
# acc = 1 - exp(-softplus(x) delta), so with g_acc = 1 the density entry is delta exp(-softplus(x) delta) sigmoid(x): the reference's own
# derivative in x = fl32(raw + bias), not only the kernel's reading of its sigma.  The sample widths are those of a fine level (1/256 to
# 1/64 of a unit), so that sigma delta stays below 0.6 and the entry keeps its conditioning over the whole grid: sigma's rounding
# (expf, log1pf) then moves exp(-sigma delta) and the factor by at most its own relative size.
FROM_RAW_BOUND = 16 * U


def from_raw_case():
    """raw [B,1,4] with raw_density on a grid over [-30, 30], t [B,2], dirs [B,3] (fp32) and the float64 d_raw.w for g_acc = 1"""
    B = FROM_RAW_RAYS
    rng = np.random.default_rng(7)
    raw = np.zeros((B, 1, 4), F)
    raw[:, 0, :3] = rng.normal(0.0, 2.5, (B, 3))
    raw[:, 0, 3] = np.linspace(-30.0, 30.0, B)
    _, _, dirs = make("soft", B, 1, rng)
    t0 = rng.uniform(2.0, 5.9, B)
    t = np.stack([t0, t0 + rng.uniform(1.0 / 256, 1.0 / 64, B)], -1).astype(F)
    x = (raw[:, 0, 3] + F(FROM_RAW_BIAS)).astype(np.float64)              # raymath.hpp density_activation: fl32(raw + bias)
    delta = (t[:, 1] - t[:, 0]).astype(np.float64) * np.sqrt((dirs.astype(np.float64) ** 2).sum(-1))
    want = delta * np.exp(-np.logaddexp(0.0, x) * delta) / (1.0 + np.exp(-x))
    assert np.all(np.logaddexp(0.0, x) * delta < 0.6)
    return raw, t, dirs, want


def case_seed(cls, N):
    return 1000 * CLASSES.index(cls) + N
