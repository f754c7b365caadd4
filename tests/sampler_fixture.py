"""Fixture of the inverse-CDF sampler's per-entry probes (numpy only, no kernel runs here): weight classes, bins, draws, the float64 truth
of every resampled t and of every d_weights entry from the kernel's own fp32 operands, a running-error budget per entry, and an fp32
emulation of pdf_ray (csrc/raywave.hpp) and k_resample_bwd (csrc/kernels_resample_grad.hip) from which the budgets' two constants are taken.

    v_i   = (max(w_{i-1}, w_i) + max(w_i, w_{i+1})) / 2 + padding     (blur route; w_{-1} = w_0, w_N = w_{N-1}; no-blur route: v = w)
    pad   = max(0, 1e-5 - sum v)     v_i += pad / N     S = sum v + pad     pdf_i = v_i / S
    cs_i  = sum_{m<i} pdf_m          cdf = [0, min(1, cs_1), ..., min(1, cs_{N-1}), 1]
    i(j)  = searchsorted(cdf, u_j, right=True) - 1         the LAST interval whose lower entry is <= u_j
    den   = c1 - c0,  den < 1e-5 -> 1                       t'_j = b0 + (u_j - c0) / den (b1 - b0)
The truth evaluates this chain in float64 from the fp32 weights, bins, padding, fl32(1e-5) and the fp32 draws u.  The backward truth is
the closed-form adjoint of the same chain (g0 / g1 per interval -> d cs, half at cs == 1 -> exclusive suffix sums -> d v through S, or
through the constant S = 1e-5 when pad > 0 -> the blur pool's shares, a half to each side at a tie), cross-checked against torch float64
autograd in test_sampler_cpu.py.

Draws.  Deterministic: torch.linspace(0, 1 - eps, n)[j] with the kernel's single-rounded fma.  Randomized: fl(fl(j u_step) + fl(r_j
u_jitter)) clipped to 1 - eps, (u_step, u_jitter) of draw_step in csrc/lane_buckets.hpp.  Every u row of this fixture is non-decreasing
(asserted in make_draws): the backward's bisection assumes that, and rows that are not non-decreasing are not covered here.

Fragile draws.  cdf32 differs from cdf64 by at most about 3.5 x 2^-24 cdf (two rounded divisions and a rounded sum per pdf entry, the
double prefix sum rounded once).  A draw whose u lies within BAND cdf_i = 2^-20 cdf_i (that bound times about 4.5) of an interior entry i
without being equal to it is *fragile*: the kernel may put it on the other side of the entry.  A draw equal to an entry (u == cdf64_i, so the
entry is an fp32 number: the engineered ties of `uniform_ties` and u = 0 behind leading zero-weight bins) is not fragile.
    forward   continuous across an entry whose two bins both have mass >= 1e-5: a fragile draw is compared like any other, with the
              larger of the two bins' terms in its budget.  Next to a bin of mass < 1e-5 the forward jumps (den -> 1): only those
              fragile draws are left out.
    backward  not continuous.  Dense probes carry g_j = 0 on fragile draws; a one-hot probe on a fragile draw must match, within
              budget, the truth of one of the two memberships.
At most 1 % of a case's draws may be fragile (test_sampler_cpu.py asserts it of these inputs), except in the *aligned* cases
(aligned_case), whose deterministic draws sit on cdf entries by construction:
    `empty`, `uniform_ties`   u_j = (1 - eps) j / N under cdf_j = j / N: every interior draw is fragile, the dense probes are zero on all of them
    `onehot`, N = 65 and 300  one weight 1 and padding 0.01 give cdf_i = 0.01 i / (0.01 N + 2) beside the hot bin: i / 265 meets j / 65 at
                              every 13th draw, i / 500 meets j / 300 at every third (22.6 % of the draws); the dense probes keep the others
The aligned cases run EITHER_OR = 4 further one-hot either-or probes: with each ray's fragile draws in a list of length L, probe k
takes entry round(k (L - 1) / 3), k = 0 .. 3 -- evenly placed from the first fragile draw to the last (in `empty` and `uniform_ties`
draw 1 + round(k (N - 2) / 3)), N >= 4, every one on a fragile draw and non-zero (asserted).  No draw is left out for any other reason.

Inputs where the classes leave a choice.  `tiny` runs with padding 0 only (with 0.01 it is `empty` again) and is rescaled, where needed, to a
blurred sum of 5e-6, so that the pad > 0 branch runs at every N (1024 weights of up to 1e-7 would pass 1e-5).  `empty` runs with padding 0.01 and
0.  `soft` and `sliver` keep every mass 2e-6 away from the 1e-5 rule (a weight that close is halved), since den32 < 1e-5 and den64 < 1e-5
must agree.  The hot bin of `onehot` cycles over both ends, the middle and both sides of three lane boundaries (onehot_bins).

Mutations (test_sampler_cpu.py; arithmetic only).  Forward: "left" searchsorted left; "blur_zero_left" the clamped left term of the pooled
row taken as 0, v_0 = max(w_0, w_1) / 2 + padding (a 0 in place of w_0 in the PADDED WEIGHTS would be the identity on non-negative
weights: max(0, w_0) = w_0); "pad_inside" 0.5 (max + max + padding); "pad_not_div" the 1e-5 pad not divided by N.  Backward: "tie_one"
share 1 at a tie; "no_self" the two self-neighbour terms at c = 0 and c = N - 1 dropped; "no_dot" the dot term dropped; "pad_formula" the
pad == 0 formula when pad > 0; "left" left membership.

Budgets (units of u = 2^-24; bounds on the rounding the kernel's evaluation order can accumulate, not tolerances):
    forward   budget_j = C_F u (slope_j c1_j + |t'_j| + |b1 - b0|),    slope_j = |b1 - b0| / den
              slope c1: the CDF's relative rounding moved through the interpolation; the other two: the final roundings
    backward  per draw of interval i:  a0_j = |g_j db (u - c1)| / den^2,  a1_j = |g_j db (u - c0)| / den^2,  amp_j = |g_j db| / den^2
              (den < 1e-5: a0_j = |g_j db|, a1_j = amp_j = 0).  amp_j is the amplification of the CDF's rounding: u - c carries the
              ABSOLUTE error of c.
              M0_i = sum_j (a0_j + amp_j)   M1_i = sum_j (a1_j + amp_j)   Mcs_i = M0_i + M1_{i-1}   Mpdf_m = sum_{i>m} Mcs_i
              Mv_i = (Mpdf_i + sum_m Mpdf_m pdf_m) / S        (pad > 0: (Mpdf_i + sum_m Mpdf_m / N) / S)
              Mw   = the blur pool's shares applied to Mv
              budget = C_B u Mw + 2^-120
    No floor but the 2^-120 for subnormals, and nothing is normalised by a ray's or a batch's largest entry."""
import numpy as np

F = np.float32
D = np.float64
U = 2.0 ** -24
FLOOR = 2.0 ** -120
EPS32 = F(1.1920928955078125e-07)
UMAX = F(1) - EPS32
E5 = F(1e-5)                        # the kernel's 1e-5f, an fp32 operand of the truth
BAND = 2.0 ** -20                   # guard band of a fragile draw, relative to the cdf entry
CDF_BOUND = 3.5 * U                 # the derived bound on |cdf32 - cdf64| / cdf64 (asserted of the emulation in test_sampler_cpu.py)
SLIVER_GUARD = 1e-6                 # no bin's mass lies within this of 1e-5: den32 < 1e-5 and den64 < 1e-5 then agree
# The constants of the budgets: the worst |emulation - truth| / budget(C = 1) of emulate_forward / emulate_backward below over every
# class, size, route, padding and probe of this fixture (test_sampler_cpu.py prints them and asserts emulation / budget <= 0.5), times 2
# for evaluation order the emulation does not reproduce (the sampler calls no math library).  Measured worst ratios at C = 1:
#     forward   blur route 1.833 (tiny, padding 0)    no-blur route 1.463 (soft)
#     backward  1.859 (soft, N = 300, the one-hot probe on the last draw)
# They come from the emulation, never from the kernel under test.
C_F = 3.7
C_B = 3.75

RAYS = 18                           # a ragged last workgroup of the 4-rays-per-block forward
SIZES = (1, 5, 64, 65, 129, 300, 513, 1024)          # lane buckets K = 1, 1, 1, 2, 4, 8, 16, 16
TIE_SIZES = (1, 4, 64, 1024)        # uniform_ties: the powers of two among SIZES, plus 4
NOBLUR_SIZES = (5, 64, 129, 1024)
BLUR_CLASSES = ("soft", "empty", "onehot", "surface", "plateau", "tiny", "uniform_ties")
NOBLUR_CLASSES = ("soft", "empty", "onehot", "surface", "sliver")
ALL_CLASSES = BLUR_CLASSES + ("sliver",)
EITHER_OR = 4
ALIGNED_ONEHOT = (("onehot", 65), ("onehot", 300))
FORWARD_MUTATIONS = ("left", "blur_zero_left", "pad_inside", "pad_not_div")
BACKWARD_MUTATIONS = ("tie_one", "no_self", "no_dot", "pad_formula", "left")


def lane_bucket(N):
    """csrc/lane_buckets.hpp: the smallest K in 1, 2, 4, ... with 64 K >= N"""
    K = 1
    while 64 * K < N:
        K *= 2
    return K


def sizes_of(cls):
    return TIE_SIZES if cls == "uniform_ties" else SIZES


def paddings_of(cls):
    """resample_padding 0.01 (the shipped value), and 0.0 as well where it reaches the pad > 0 branch"""
    return (0.01, 0.0) if cls == "empty" else ((0.0,) if cls == "tiny" else (0.01,))


def noblur_draw_counts(N):
    """num_draws of the no-blur entry point: 1, 2, N + 1, a full trip of the search 64 (K + 1) and one draw into the next"""
    K = lane_bucket(N)
    return (1, 2, N + 1, 64 * (K + 1), 64 * (K + 1) + 1)


# ---- draws ------------------------------------------------------------------------------------------------------------------------------
def draw_step(n):
    """csrc/lane_buckets.hpp draw_step: double arithmetic rounded once"""
    s = 1.0 / float(n)
    return F(s), F(s - float(EPS32))


def linspace_u(n):
    """torch_linspace_at(0, 1 - eps, n, j) of csrc/raymath.hpp for j = 0 .. n - 1: step * j below the midpoint, end - step * (n - 1 - j) above,
    each a fused multiply-add (the double expression is exact, so one rounding)"""
    if n == 1:
        return np.zeros(1, F)
    step = D(UMAX / F(n - 1))
    j = np.arange(n)
    lo = (step * j).astype(F)
    hi = (D(UMAX) - step * (n - 1 - j)).astype(F)
    return np.where(j < n // 2, lo, hi).astype(F)


def u_of(r, n):
    """the kernel's randomized draw from u_rand r [B, n]"""
    step, jit = draw_step(n)
    j = np.arange(n, dtype=F)[None, :]
    return np.minimum(j * step + r.astype(F) * jit, UMAX).astype(F)


def engineered_ties(N):
    """u_rand row [N + 1] whose draws j = 1 .. N - 1 equal j / N exactly (N a power of two), and the mask of the j for which the search
    succeeded.  The search starts from the float64 solution of j u_step + r u_jitter = j / N (about j / N) and tries its fp32 neighbours."""
    n = N + 1
    step, jit = draw_step(n)
    r = np.zeros(n, F)
    ok = np.ones(n, bool)
    r[N] = F(0.5)
    if N < 2:
        return r, ok
    j = np.arange(1, N)
    target = (j / N).astype(F)
    assert np.all(target.astype(D) == j / N)
    js = j.astype(F) * step
    est = ((target.astype(D) - js.astype(D)) / D(jit)).astype(F)
    k = np.arange(-64, 65)
    k = k[np.argsort(np.abs(k), kind="stable")]
    cand = (est.view(np.int32)[:, None] + k[None, :]).astype(np.int32).view(F)
    hit = (js[:, None] + cand * jit == target[:, None]) & (cand >= 0) & (cand < 1)
    first = hit.argmax(-1)
    ok[1:N] = hit.any(-1)
    r[1:N] = cand[np.arange(N - 1), first]
    return r, ok


def make_draws(n, randomized, rng, B=RAYS, ties_N=None):
    """(u_rand [B, n] or None, u [B, n]) in fp32; ties_N: the engineered row of uniform_ties (n == ties_N + 1)"""
    if not randomized:
        r, u = None, np.tile(linspace_u(n), (B, 1))
    else:
        r = rng.random((B, n), dtype=F)
        if ties_N is not None:
            assert n == ties_N + 1
            row, ok = engineered_ties(ties_N)
            assert ok.all()
            r = np.tile(row, (B, 1))
        u = u_of(r, n)
    assert u.dtype == F and np.all(np.diff(u, axis=-1) >= 0) and u.min() >= 0 and u.max() <= UMAX
    return r, np.ascontiguousarray(u)


# ---- bins and weights -------------------------------------------------------------------------------------------------------------------
def make_bins(N, rng, B=RAYS, decreasing=False):
    """strictly increasing fp32 fence posts in [2, 6]; decreasing: strictly decreasing inverse depths in (0, 5]"""
    while True:
        if decreasing:
            b = np.sort(rng.uniform(0.01, 5.0, (B, N + 1)), axis=-1)[:, ::-1].astype(F)
            good = np.all(np.diff(b, axis=-1) < 0) and b.min() > 0 and b.max() <= 5
        else:
            b = np.sort(rng.uniform(2.0, 6.0, (B, N + 1)), axis=-1).astype(F)
            good = np.all(np.diff(b, axis=-1) > 0) and b.min() >= 2 and b.max() <= 6
        if good:
            return np.ascontiguousarray(b)


def onehot_bins(B, N):
    """the hot bin of each ray: both ends, the middle, both sides of the boundary between lane 0 and lane 1 (K - 1, K), of the DPP rows
    (16 K) and of the half wave 64 K' (K' = K / 2, the next smaller bucket's size), clipped to the ray"""
    K = lane_bucket(N)
    cand = []
    for i in (0, N - 1, N // 2, K - 1, K, 32 * K - 1, 32 * K, 16 * K - 1, 16 * K):
        i = min(max(i, 0), N - 1)
        if i not in cand:
            cand.append(i)
    return np.array([cand[b % len(cand)] for b in range(B)])


def _blur(w, padding, T):
    wl = np.concatenate([w[:, :1], w[:, :-1]], -1)
    wr = np.concatenate([w[:, 1:], w[:, -1:]], -1)
    return T(0.5) * (np.maximum(wl, w) + np.maximum(w, wr)) + T(F(padding))


def make_weights(cls, N, rng, B=RAYS, n_draws=None):
    """fp32 weights [B, N] the compositing can produce: non-negative, sum at most 1.  n_draws: the deterministic draw count under
    which `sliver` places its bin (default N + 1)."""
    i = np.arange(N)[None, :]
    if cls == "soft":
        w = rng.uniform(0.0, 1.0, (B, N)) ** 6
        w *= rng.uniform(0.3, 0.999, (B, 1)) / w.sum(-1, keepdims=True)
    elif cls == "empty":
        w = np.zeros((B, N))
    elif cls == "onehot":
        w = (i == onehot_bins(B, N)[:, None]).astype(D)
    elif cls == "surface":
        ramp = np.array([0.04, 0.12, 0.3, 0.45])[-min(4, N):]
        h = rng.integers(0, N - len(ramp) + 1, B)
        h[0], h[1 % B] = 0, N - len(ramp)                 # a surface at each end of the ray as well
        k = i - h[:, None]
        w = np.where((k >= 0) & (k < len(ramp)), ramp[np.clip(k, 0, len(ramp) - 1)], 0.0) * rng.uniform(0.5, 1.0, (B, 1))
    elif cls == "plateau":
        w = np.zeros((B, N))
        for b in range(B):
            pos = 0
            while pos < N:                                # runs of 2 .. 5 equal weights (the first and the last touch the ends)
                run = int(rng.integers(2, 6))
                w[b, pos:pos + run] = 0.0 if rng.random() < 0.2 else rng.uniform(0.1, 1.0)
                pos += run
            if N >= 2:
                w[b, -2] = w[b, -1]
            if np.all(w[b] == w[b, 0]):                   # one run only: that is `uniform_ties`; two runs, or a single bin of weight 1
                w[b] = 1.0
                w[b, :N // 2] = 0.37 if N >= 4 else 1.0
        w = (w.astype(F) * F(0.9) / w.astype(F).sum(-1, keepdims=True).astype(F)).astype(D)      # one fp32 factor per ray: ties survive
    elif cls == "tiny":
        w = np.exp(rng.uniform(np.log(1e-9), np.log(1e-7), (B, N)))
        s = _blur(w.astype(F), 0.0, F).astype(D).sum(-1, keepdims=True)
        w = w * np.minimum(1.0, 5e-6 / s)                 # the blurred sum stays below 1e-5 at every N: the pad > 0 branch
    elif cls == "uniform_ties":
        assert N & (N - 1) == 0
        w = np.full((B, N), 1.0 / N)
    elif cls == "sliver":
        # [zeros] A [zeros] sliver [zeros] rest [zeros]: cdf reaches u_j - 2.5e-6 in front of a sliver of mass 5e-6, so the deterministic
        # draw j sits in its middle (the band of a fragile draw is 2^-20 cdf < 1e-6 on each side)
        assert N >= 5
        n = N + 1 if n_draws is None else n_draws
        u = linspace_u(n).astype(D)
        w = np.zeros((B, N))
        for b in range(B):
            a = float(u[1 + (3 * b) % (n - 2)]) - 2.5e-6 if n >= 3 else 0.4
            if a < 0.02 or a > 0.95:
                a = 0.4 + 0.01 * b if n < 3 else float(u[np.argmin(np.abs(u - 0.5))]) - 2.5e-6
            lead = 1 if N >= 7 else 0
            pa = lead + (int(rng.integers(0, N - 6)) if N > 6 else 0)
            ps = pa + 2
            pr = ps + 2 if N < 8 else int(rng.integers(ps + 2, N - 1))
            w[b, pa], w[b, ps], w[b, pr] = a, 5e-6, 1.0 - a - 5e-6
    else:
        raise ValueError(cls)
    w = np.ascontiguousarray(w.astype(F))
    if cls in ("soft", "sliver"):                         # no mass within SLIVER_GUARD of the 1e-5 rule (no-blur route: pdf = w / sum)
        for _ in range(8):
            pdf = w.astype(D) / np.maximum(w.astype(D).sum(-1, keepdims=True), 1e-30)
            near = np.abs(pdf - D(E5)) <= 2 * SLIVER_GUARD
            if not near.any():
                break
            w[near] *= F(0.5)
    assert w.dtype == F and np.all(w >= 0) and np.all(w.astype(D).sum(-1) <= 1.0 + 1e-6)
    return w


def blur_case(cls, N, padding, randomized, decreasing=False):
    """one case of the blur route (N + 1 draws): dict(bins, w, r, u, rng); r = None: deterministic draws"""
    rng = np.random.default_rng([1, ALL_CLASSES.index(cls), N, int(randomized), int(decreasing), int(padding == 0)])
    bins = make_bins(N, rng, decreasing=decreasing)
    w = make_weights(cls, N, rng)
    r, u = make_draws(N + 1, randomized, rng, ties_N=N if cls == "uniform_ties" and randomized else None)
    return dict(bins=bins, w=w, r=r, u=u, rng=rng)


def noblur_case(cls, N, n_draws, randomized):
    """one case of the no-blur entry point with n_draws draws"""
    rng = np.random.default_rng([2, ALL_CLASSES.index(cls), N, int(randomized), n_draws])
    bins = make_bins(N, rng)
    w = make_weights(cls, N, rng, n_draws=n_draws)
    r, u = make_draws(n_draws, randomized, rng)
    return dict(bins=bins, w=w, r=r, u=u, rng=rng)


# ---- the chain, in float64 (truth) or in the kernel's fp32 order (emulation) -----------------------------------------------------------
def _excl_prefix(v):
    return np.concatenate([np.zeros_like(v[:, :1]), np.cumsum(v, axis=-1)[:, :-1]], axis=-1)


def _take(a, idx):
    return np.take_along_axis(a, idx, axis=-1)


def _chain(bins, w, u, blur, padding, f32, mut=None):
    T = F if f32 else D
    B, N = w.shape
    bins, w, u = bins.astype(T), w.astype(T), u.astype(T)
    if blur:
        wl = np.concatenate([w[:, :1], w[:, :-1]], -1)
        wr = np.concatenate([w[:, 1:], w[:, -1:]], -1)
        ml, mr = np.maximum(wl, w), np.maximum(w, wr)
        if mut == "blur_zero_left":                       # the clamped left term of the pooled row taken as 0 instead of max(w_0, w_0)
            ml[:, 0] = 0
        v = T(0.5) * (ml + mr + T(F(padding))) if mut == "pad_inside" else T(0.5) * (ml + mr) + T(F(padding))
    else:
        v = w
    wsum = v.astype(D).sum(-1).astype(T)                  # a double sum rounded once
    pad = np.maximum(T(0), T(E5) - wsum)
    padn = pad if mut == "pad_not_div" else pad / T(N)
    wsum = wsum + pad
    pdf = (v + padn[:, None]) / wsum[:, None]
    cs = _excl_prefix(pdf.astype(D)).astype(T)
    cdf = np.concatenate([np.zeros((B, 1), T), np.minimum(T(1), cs[:, 1:]), np.ones((B, 1), T)], -1)
    side = "left" if mut == "left" else "right"
    idx = np.stack([np.searchsorted(cdf[b], u[b], side=side) for b in range(B)])
    below, above = np.maximum(idx - 1, 0), np.minimum(idx, N)
    c0, c1, b0, b1 = _take(cdf, below), _take(cdf, above), _take(bins, below), _take(bins, above)
    den = c1 - c0
    den = np.where(den < T(E5), T(1), den)
    t = b0 + (u - c0) / den * (b1 - b0)
    assert t.dtype == T and pdf.dtype == T and cdf.dtype == T
    return dict(B=B, N=N, T=T, bins=bins, w=w, u=u, v=v, pad=pad, wsum=wsum, pdf=pdf, cs=cs, cdf=cdf, idx=idx, bin=below, t=t, blur=blur)


def emulate_forward(bins, w, u, blur, padding, mut=None):
    """pdf_ray in numpy fp32, expression by expression, its prefix sums in double rounded once; the whole state (t [B, n] under "t")"""
    return _chain(bins, w, u, blur, padding, True, mut)


def forward_truth(bins, w, u, blur, padding, c_f=C_F):
    """the float64 chain, plus per draw: fragile, alt (the bin on the other side of the entry a fragile draw is near), left_out (fragile
    next to a bin of mass < 1e-5) and the forward budget"""
    tr = _chain(bins, w, u, blur, padding, False)
    N, cdf, pdf, k, uu = tr["N"], tr["cdf"], tr["pdf"], tr["bin"], tr["u"]
    assert np.all(np.abs(pdf - D(E5)) > SLIVER_GUARD), "a bin's mass sits on the 1e-5 rule"
    assert np.all(np.abs(tr["wsum"] - tr["pad"] - D(E5)) > SLIVER_GUARD), "a ray's sum sits on the 1e-5 padding rule"
    assert np.all(tr["cs"] < 1.0 - BAND) or not blur, "cs reaches 1 on the blur route"
    c0, c1 = _take(cdf, k), _take(cdf, k + 1)
    d_lo, d_hi = uu - c0, c1 - uu
    frag_lo = (k >= 1) & (d_lo > 0) & (d_lo <= BAND * c0)
    frag_hi = (k <= N - 2) & (d_hi <= BAND * c1)
    alt = np.where(frag_lo, k - 1, np.where(frag_hi, k + 1, k))
    small = pdf < D(E5)
    lo_n, hi_n = np.clip(k - 1, 0, N - 1), np.clip(k + 1, 0, N - 1)
    left_out = (frag_lo & (_take(small, lo_n) | _take(small, k))) | (frag_hi & (_take(small, hi_n) | _take(small, k)))
    db = np.abs(np.diff(tr["bins"], axis=-1))
    den = np.diff(cdf, axis=-1)
    slope_c = db / np.where(den < D(E5), 1.0, den) * cdf[:, 1:]
    budget = c_f * U * (np.maximum(_take(slope_c, k), _take(slope_c, alt)) + np.abs(tr["t"]) + np.maximum(_take(db, k), _take(db, alt)))
    tr.update(fragile=frag_lo | frag_hi, alt=alt, left_out=left_out, budget=budget)
    return tr


def forward_ratio(t, tr):
    """worst |t - truth| / budget over the draws that are compared"""
    e = np.abs(t.astype(D) - tr["t"]) / tr["budget"]
    return float(np.where(tr["left_out"], 0.0, e).max())


def _segment_sum(term, key, size, f32):
    """sum of term over equal keys (non-decreasing flat keys); fp32: in j order, one rounded add per draw, as the kernel's loop"""
    term, key = term.ravel(), key.ravel()
    if not f32:
        out = np.zeros(size, D)
        np.add.at(out, key, term)
        return out
    assert np.all(np.diff(key) >= 0)
    cnt = np.bincount(key, minlength=size)
    start = np.cumsum(cnt) - cnt
    acc = np.zeros(size, F)
    live = np.nonzero(cnt > 0)[0]
    k = 0
    while live.size:
        acc[live] = acc[live] + term[start[live] + k]
        k += 1
        live = live[cnt[live] > k]
    return acc


def _share(a, b, T, tie):
    return np.where(a > b, T(1), np.where(a == b, T(tie), T(0)))


def _blur_adjoint(w, dv, T, tie=0.5, no_self=False):
    """d_weights from d v in the kernel's gather order"""
    B, N = w.shape
    half = T(0.5)
    wl = np.concatenate([w[:, :1], w[:, :-1]], -1)
    wr = np.concatenate([w[:, 1:], w[:, -1:]], -1)
    g = half * dv * (_share(w, wl, T, tie) + _share(w, wr, T, tie))
    if not no_self:
        g[:, 0] = g[:, 0] + half * dv[:, 0] * _share(wl[:, 0], w[:, 0], T, tie)
        g[:, -1] = g[:, -1] + half * dv[:, -1] * _share(wr[:, -1], w[:, -1], T, tie)
    if N > 1:
        g[:, :-1] = g[:, :-1] + half * dv[:, 1:] * _share(w[:, :-1], w[:, 1:], T, tie)
        g[:, 1:] = g[:, 1:] + half * dv[:, :-1] * _share(w[:, 1:], w[:, :-1], T, tie)
    return g


def _backward(st, g, f32, bins_of=None, mut=None, magnitudes=False):
    """d_weights [B, N] of the upstream g [B, N + 1] from the state of _chain (same precision).  bins_of: the interval of every draw
    (default: the state's own).  magnitudes: the abs-sum Mw of the budget in place of the gradient (float64 state only)."""
    T = st["T"]
    B, N, cdf, u, pdf = st["B"], st["N"], st["cdf"], st["u"], st["pdf"]
    k = st["bin"] if bins_of is None else bins_of
    g = g.astype(T)
    c0, c1 = _take(cdf, k), _take(cdf, k + 1)
    db = _take(st["bins"], k + 1) - _take(st["bins"], k)
    den = c1 - c0
    small = den < T(E5)
    dtt = g * db
    with np.errstate(divide="ignore", invalid="ignore"):
        inv2 = T(1) / (den * den)
        if magnitudes:
            amp = np.where(small, 0.0, np.abs(dtt) * inv2)
            t0 = np.where(small, np.abs(dtt), np.abs(dtt * (u - c1)) * inv2) + amp
            t1 = np.where(small, 0.0, np.abs(dtt * (u - c0)) * inv2) + amp
        else:
            t0 = np.where(small, -dtt, dtt * (u - c1) * inv2)
            t1 = np.where(small, T(0), -dtt * (u - c0) * inv2)
    key = k + N * np.arange(B)[:, None]
    g0 = _segment_sum(t0, key, B * N, f32).reshape(B, N).astype(D)
    g1 = _segment_sum(t1, key, B * N, f32).reshape(B, N).astype(D)
    cs = st["cs"]
    through = np.where(cs < T(1), 1.0, np.where(cs == T(1), 0.5, 0.0))
    dcs = np.zeros((B, N))
    dcs[:, 1:] = (g0[:, 1:] + g1[:, :-1]) * through[:, 1:]
    dpdf = _excl_prefix(dcs[:, ::-1])[:, ::-1]
    p = pdf.astype(D)
    S = st["wsum"].astype(D)[:, None]
    padded = (st["pad"] > 0)[:, None]
    sign = 1.0 if magnitudes else -1.0
    dot = (dpdf * p).sum(-1, keepdims=True)
    sumd = dpdf.sum(-1, keepdims=True)
    if mut == "no_dot":
        dot = 0.0 * dot
    if mut == "pad_formula":
        padded = np.zeros_like(padded)
    dv = (np.where(padded, (dpdf + sign * sumd / N) / S, (dpdf + sign * dot) / S)).astype(T)
    if not st["blur"]:
        return dv
    return _blur_adjoint(st["w"], dv, T, tie=1.0 if mut == "tie_one" else 0.5, no_self=mut == "no_self")


def backward_truth(tr, g, bins_of=None, c_b=C_B):
    """(d_weights, budget) in float64 from forward_truth's state"""
    d_w = _backward(tr, g, False, bins_of)
    return d_w, c_b * U * _backward(tr, g, False, bins_of, magnitudes=True) + FLOOR


def emulate_backward(em, g, mut=None):
    """k_resample_bwd in numpy fp32 from emulate_forward's state: fp32 g0 / g1 sums in j order, the double sums between them, fp32 s_dv and
    the blur shares in the kernel's order.  mut == "left": the state must come from emulate_forward(mut="left")."""
    d_w = _backward(em, g, True, mut=mut)
    assert d_w.dtype == F
    return d_w


# ---- probes of the backward ---------------------------------------------------------------------------------------------------------
def aligned_case(cls, N, randomized):
    """the deterministic cases whose draws sit on cdf entries by construction (the module's docstring): they may exceed the 1 % of
    fragile draws and run the EITHER_OR further probes"""
    return not randomized and (cls in ("empty", "uniform_ties") or (cls, N) in ALIGNED_ONEHOT)


def probes(tr, rng, cls, randomized):
    return _probes(tr, rng, aligned_case(cls, tr["N"], randomized))


def _probes(tr, rng, aligned):
    """[(name, g [B, N + 1] fp32, either_or)] for a blur-route case with N + 1 draws.  One-hot probes: the first draw, the last, one in
    the middle of the bin with the most draws, one fragile draw where a ray has one (g = 0 on the other rays); dense probes (random, all
    ones) are zero on fragile draws.  either_or: a one-hot probe that may match the truth of either membership where its draw is fragile."""
    B, N, frag, k = tr["B"], tr["N"], tr["fragile"], tr["bin"]
    n = N + 1
    rows = np.arange(B)

    def onehot(j, live=None):
        g = np.zeros((B, n), F)
        g[rows, j] = 1 if live is None else live.astype(F)
        return g
    cnt = np.stack([np.bincount(k[b], minlength=N) for b in range(B)])
    big = cnt.argmax(-1)
    first_in_big = np.stack([np.searchsorted(k[b], big[b], side="left") for b in range(B)])
    out = [("first", onehot(np.zeros(B, int)), True), ("last", onehot(np.full(B, N)), True),
           ("most", onehot(first_in_big + cnt[rows, big] // 2), True),
           ("fragile", onehot(frag.argmax(-1), frag.any(-1)), True)]
    if aligned and N >= 4:
        has = frag.any(-1)
        assert has.any()
        for e in range(EITHER_OR):                        # the e-th of EITHER_OR evenly placed entries of each ray's list of fragile draws
            j = np.array([np.nonzero(f)[0][int(round(e * (f.sum() - 1) / (EITHER_OR - 1)))] if f.any() else 1 for f in frag])
            assert np.all((j >= 1) & (j <= N - 1))
            out.append((f"either{e}", onehot(j, has), True))
    keep = (~frag).astype(F)
    out.append(("dense", (rng.standard_normal((B, n)).astype(F) * keep).astype(F), False))
    out.append(("ones", keep.copy(), False))
    return out


def backward_ratio(d_w, tr, g, either_or):
    """worst |d_w - truth| / budget per ray [B]; either_or: per ray the better of the two memberships of its fragile draws"""
    want, budget = backward_truth(tr, g)
    r = (np.abs(d_w.astype(D) - want) / budget).max(-1)
    if either_or:
        hot = (g != 0) & tr["fragile"]
        if hot.any():
            want2, budget2 = backward_truth(tr, g, np.where(hot, tr["alt"], tr["bin"]))
            r = np.minimum(r, (np.abs(d_w.astype(D) - want2) / budget2).max(-1))
    return r
