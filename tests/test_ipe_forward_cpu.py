"""CPU: the fixture of the forward Gaussians and encodings (tests/ipe_forward.py) checked on its own, before test_gpu_ipe_forward.py
holds k_cast_rays, k_integrated_pos_enc, k_cast_ipe and k_pos_enc to it: the host build of csrc/raymath.hpp within half of every
budget (the three constants are twice its worst ratios, measured and printed here), the float64 Gaussian truth against mpmath (or
exact rationals), the numpy emulations against the budgets, the hand-made table's exact zeros, and the power of the criteria to see
each mutation a subtly wrong kernel could carry, with the factor by which it misses."""
import functools

import numpy as np
import pytest

import ipe_forward as fw


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _case(cls, B, N):
    t, o, d, r, info = fw.make(cls, B, N)
    mean, cov = fw.host_gaussians(t, o, d, r)
    return (t, o, d, r), (mean, cov), fw.gaussian_truth(t, o, d, r), info


@functools.lru_cache(maxsize=None)
def _truth(cls, B, N, cfg):
    _, (mean, cov), _, _ = _case(cls, B, N)
    return fw.feature_truth(mean, cov, cfg)


def _host_constants():
    """worst ratio at C = 1 of the host build, with the case that gives it: mean, cov, feature, view"""
    wm = wv = wf = ww = (-1.0, "")
    for cls in fw.CLASSES:
        for B, N in fw.SHAPES:
            _, (mean, cov), tr, _ = _case(cls, B, N)
            a, b = fw.gaussian_ratios(mean, cov, tr, 1.0, 1.0)
            wm, wv = max(wm, (a, f"{cls} {B}x{N}")), max(wv, (b, f"{cls} {B}x{N}"))
            for cfg in fw.CONFIGS:
                ft = _truth(cls, B, N, cfg)
                f = fw.worst(fw.host_features(mean, cov, cfg), ft["truth"], fw.f32_budget(ft["truth"], 1.0))
                wf = max(wf, (f, f"{cls} {B}x{N} {fw.config_id(cfg)}"))
    mean, cov = fw.table()
    ft = fw.feature_truth(mean, cov, fw.CONFIGS[0])
    wf = max(wf, (fw.worst(fw.host_features(mean, cov, fw.CONFIGS[0]), ft["truth"], fw.f32_budget(ft["truth"], 1.0)), "table"))
    for B in (1, 7, 257):
        for deg in (0, 4):
            v = fw.view_dirs(B)
            tr, _ = fw.view_truth(v, deg)
            ww = max(ww, (fw.worst(fw.host_view(v, deg), tr, fw.f32_budget(tr, 1.0)), f"B={B} deg={deg}"))
    return wm, wv, wf, ww


def test_constants_are_twice_the_host_build():
    """C_M, C_V, C_F = twice the host build's worst ratio (rounded up to two digits), so the host build sits within half of every
    budget; none above its ceiling (16 for the Gaussians: a larger one means a wrong magnitude; 15 for the features)"""
    wm, wv, wf, ww = _host_constants()
    print(f"ipe_forward host build, worst |got - truth| / (u magnitude + floor): mean {wm[0]:.3f} ({wm[1]}), cov {wv[0]:.3f} ({wv[1]}), "
          f"feature {wf[0]:.3f} ({wf[1]}), view {ww[0]:.3f} ({ww[1]})")
    print(f"ipe_forward constants: C_M = {fw.C_M} C_V = {fw.C_V} C_F = {fw.C_F}")
    for c, w in ((fw.C_M, wm[0]), (fw.C_V, wv[0]), (fw.C_F, max(wf[0], ww[0]))):
        assert w <= c / 2 <= 1.05 * w, (c, w)
    assert fw.C_M <= 16 and fw.C_V <= 16 and fw.C_F <= fw.C_F_CEILING


@pytest.mark.parametrize("cls", fw.CLASSES)
def test_host_build_within_half_of_every_budget(cls):
    """and the numpy restatements: the Gaussians bit for bit the host build (IEEE operations in the same order), the fp32 features
    (correctly rounded exp and sin) within the budget"""
    worst = {}
    for B, N in fw.SHAPES:
        (t, o, d, r), (mean, cov), tr, _ = _case(cls, B, N)
        assert mean.shape == (B, N, 3) and mean.dtype == np.float32 and np.isfinite(mean).all() and np.isfinite(cov).all()
        a, b = fw.gaussian_ratios(mean, cov, tr)
        em, ec = fw.emulate_gaussians(t, o, d, r)
        assert np.array_equal(_bits(em), _bits(mean)) and np.array_equal(_bits(ec), _bits(cov)), (cls, B, N)
        worst["mean"], worst["cov"] = max(worst.get("mean", 0), a), max(worst.get("cov", 0), b)
        for cfg in fw.CONFIGS:
            ft = _truth(cls, B, N, cfg)
            bud = fw.f32_budget(ft["truth"])
            h = fw.worst(fw.host_features(mean, cov, cfg), ft["truth"], bud)
            e = fw.worst(fw.emulate_features(mean, cov, cfg), ft["truth"], bud)
            k = fw.config_id(cfg)
            worst[k], worst[k + " emu"] = max(worst.get(k, 0), h), max(worst.get(k + " emu", 0), e)
    print(f"ipe_forward host {cls}: worst got/budget " + " ".join(f"{k}={v:.3f}" for k, v in worst.items()))
    assert all(v <= 0.5 for k, v in worst.items() if not k.endswith("emu")), worst
    assert all(v <= 1.0 for v in worst.values()), worst


def test_class_extremes():
    """what the configurations are there for: phases near 1e11 rad that nothing damps, and damping that underflows"""
    ft = _truth("far", 1, 513, (15, 31, True))
    assert np.abs(ft["x"]).max() > 5e10 and np.all(ft["damp"] == 1.0)
    ft = _truth("far", 1, 513, (0, 16, False))
    assert 1e6 <= np.abs(ft["x"]).max() <= 4e6 and np.any(ft["damp"] == 0) and np.any(ft["damp"] > 0.5)
    small = (np.abs(ft["truth"]) < 1e-6) & (np.abs(ft["truth"]) > 2.0 ** -100)
    assert small.mean() > 0.01                     # strongly damped degrees a 2e-6 absolute criterion cannot see
    assert [B * N for B, N in fw.SHAPES] == [7, 25, 129, 128, 513]
    (t, _, _, _), _, tr, info = _case("thin", 3, 43)
    assert np.all(info["repeated"] >= 0) and (tr["t_var"] == 0).sum() == 3


def _exact(cls_samples):
    """the Gaussian of a few samples in 60-digit mpmath arithmetic, or in exact rationals where mpmath is missing"""
    try:
        import mpmath
        mpmath.mp.dps = 60
        num, back = mpmath.mpf, float
    except ImportError:
        from fractions import Fraction
        num, back = Fraction, float
    out = []
    for t0, t1, o, d, r in cls_samples:
        t0, t1, r = num(float(t0)), num(float(t1)), num(float(r))
        o, d = [num(float(v)) for v in o], [num(float(v)) for v in d]
        c4, c5, eps = num(fw.C4), num(fw.C5), num(fw.EPS_DN)
        mu, hw = (t0 + t1) / 2, (t1 - t0) / 2
        den = 3 * mu ** 2 + hw ** 2
        # written from mip.py:68-72 with the powers as powers, not from the fixture's expression tree
        t_mean = mu + 2 * mu * hw ** 2 / den
        t_var = hw ** 2 / 3 - c4 * hw ** 4 * (12 * mu ** 2 - hw ** 2) / den ** 2
        r_var = r ** 2 * (mu ** 2 / 4 + c5 * hw ** 2 - c4 * hw ** 4 / den)
        dn = sum(v * v for v in d) + eps
        out.append(([back(d[a] * t_mean + o[a]) for a in range(3)],
                    [back(t_var * d[a] ** 2 + r_var * (1 - d[a] ** 2 / dn)) for a in range(3)]))
    return out


@pytest.mark.parametrize("cls", fw.CLASSES)
def test_gaussian_truth_against_an_independent_form(cls):
    """float64 is 2^-29 of the fp32 unit: the truth must sit within 1e-6 of a budget's unit (u magnitude) of the exact value"""
    (t, o, d, r), _, tr, _ = _case(cls, 5, 5)
    picks = [(0, 0), (1, 4), (2, 2), (3, 1), (4, 3)]
    exact = _exact([(t[b, i], t[b, i + 1], o[b], d[b], r[b]) for b, i in picks])
    for (b, i), (m, c) in zip(picks, exact):
        assert np.all(np.abs(tr["mean"][b, i] - m) <= 1e-6 * fw.U * tr["mag_mean"][b, i] + 1e-300), (cls, b, i)
        assert np.all(np.abs(tr["cov"][b, i] - c) <= 1e-6 * fw.U * tr["mag_cov"][b, i] + 1e-300), (cls, b, i)


# ---- mutations ------------------------------------------------------------------------------------------------------------------------
def _feature_miss(emulate, key, mutation, cls, cfg):
    w = 0.0
    for B, N in fw.SHAPES:
        _, (mean, cov), _, _ = _case(cls, B, N)
        ft = _truth(cls, B, N, cfg)
        bud = fw.f32_budget(ft["truth"]) if key == "f32" else ft["bf16"]
        w = max(w, fw.worst(emulate(mean, cov, cfg, mutation), ft["truth"], bud))
    return w


def test_mutation_unstable_t_var():
    """1: t_var by the reference's unstable branch (mip.py:74-77), on `thin`: NaN on the repeated post, 1e10 budgets elsewhere"""
    for B, N in fw.SHAPES:
        (t, o, d, r), _, tr, info = _case("thin", B, N)
        mean, cov = fw.emulate_gaussians(t, o, d, r, "unstable_t_var")
        rep = np.array([(t[b, 1:] == t[b, :-1]) for b in range(B)])
        assert np.array_equal(np.isnan(cov).all(-1), rep) and rep.sum() >= 1                # the repeated post: 0 / 0
        ratio = np.abs(cov.astype(np.float64) - tr["cov"]) / (fw.C_V * fw.U * tr["mag_cov"] + fw.FLOOR)
        miss = float(ratio[~rep].max()) if (~rep).any() else float("inf")
        print(f"ipe_forward mutation unstable_t_var thin {B}x{N}: cov misses by {miss:.3g}, {int(rep.sum())} NaN rows")
        assert miss > 1e3 and fw.gaussian_ratios(mean, cov, tr)[1] == float("inf")
        assert fw.gaussian_ratios(mean, np.where(np.isnan(cov), 0, cov), tr)[0] <= 0.5          # the mean is untouched


def test_mutation_fma_mean_needs_bit_equality():
    """2: d t_mean + o with one rounding stays within the float64 budget everywhere (it is the more accurate mean); only the
    bit-for-bit comparison with the host build sees it"""
    for cls in fw.CLASSES:
        differ = total = 0
        w = 0.0
        for B, N in fw.SHAPES:
            (t, o, d, r), (hmean, hcov), tr, _ = _case(cls, B, N)
            mean, cov = fw.emulate_gaussians(t, o, d, r, "fma_mean")
            w = max(w, max(fw.gaussian_ratios(mean, cov, tr)))
            differ, total = differ + int((_bits(mean) != _bits(hmean)).sum()), total + mean.size
            assert np.array_equal(_bits(cov), _bits(hcov))
        print(f"ipe_forward mutation fma_mean {cls}: worst got/budget {w:.3f} (passes), {differ} of {total} means differ in their bits")
        assert w <= 1.0 and differ >= total // 20


# (mutation, emulation, budget, class, configuration): the named case on which the mutation must miss
_NAMED = [("true_cos", "f32", "far", (0, 16, False)),                  # 3
          ("exp2_product", "f32", "coarse_pixel", (0, 16, False)),     # 4
          ("fp32_reduction", "f32", "far", (15, 31, True)),            # 5, fp32 path
          ("fp32_reduction", "bf16", "far", (15, 31, True)),           # 5, bf16 path
          ("degree_off_by_one", "f32", "scene", (3, 19, False)),       # 6
          ("swap_halves", "f32", "scene", (0, 16, False)),             # 7
          ("scale_not_squared", "f32", "coarse_pixel", (3, 19, False)),    # 8
          ("swap_threads", "f32", "axis", (0, 16, True)),              # 9
          ("truncate", "bf16", "scene", (0, 16, False)),               # 10
          ("double_half_pi", "f32", "scene", (0, 16, True))]           # 11


@pytest.mark.parametrize("mutation,key,cls,cfg", _NAMED, ids=[f"{m}-{k}" for m, k, _, _ in _NAMED])
def test_budget_sees_the_mutation(mutation, key, cls, cfg):
    emulate = fw.emulate_features if key == "f32" else fw.emulate_bf16
    base = _feature_miss(emulate, key, None, cls, cfg)
    miss = _feature_miss(emulate, key, mutation, cls, cfg)
    everywhere = {c: max(_feature_miss(emulate, key, mutation, c, g) for g in fw.CONFIGS) for c in fw.CLASSES}
    print(f"ipe_forward mutation {mutation} ({key}) on {cls} {fw.config_id(cfg)}: got/budget {miss:.3g} (unmutated {base:.3g}); "
          "worst per class " + " ".join(f"{c}={v:.3g}" for c, v in everywhere.items()))
    assert base <= 1.0 < miss
    if mutation == "truncate":
        assert miss > 1.9                                # half an ulp allowed, nearly a whole one taken
    elif mutation not in ("exp2_product",):
        assert miss > 100.0


def test_mutation_scale_needs_integration():
    """8 and 4 touch the damping alone: with integration disabled they change nothing, which is why both forms are in CONFIGS"""
    for mutation in ("scale_not_squared", "exp2_product"):
        assert _feature_miss(fw.emulate_features, "f32", mutation, "scene", (0, 16, True)) <= 1.0


# ---- bf16 emulation and the table -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cls", fw.CLASSES)
def test_bf16_emulation_within_its_budget(cls):
    res = {}
    for cfg in fw.CONFIGS:
        res[fw.config_id(cfg)] = _feature_miss(fw.emulate_bf16, "bf16", None, cls, cfg)
    print(f"ipe_forward bf16 emulation {cls}: worst got/budget " + " ".join(f"{k}={v:.3f}" for k, v in res.items()))
    assert max(res.values()) <= 1.0


def test_table_rows_and_exact_zeros():
    """the hand-made rows: host build within half the budget, both emulations within theirs; wherever -yv / 2 <= -150 (yv = inf
    included) every form gives exactly +-0, and nothing is NaN"""
    mean, cov = fw.table()
    cfg = fw.CONFIGS[0]
    ft = fw.feature_truth(mean, cov, cfg)
    with np.errstate(over="ignore"):
        yv = cov[:, None, :] * (4.0 ** np.arange(16)).astype(np.float32)[:, None]
    assert np.isinf(yv).any() and np.isfinite(mean[:, None, :] * np.float32(2 ** 15)).all()
    dead = fw._flat(yv, yv) >= 300
    assert dead.any() and np.all(np.abs(ft["truth"][dead]) < 2.0 ** -150)       # below half of fp32's smallest denormal
    rows = dict(host=fw.host_features(mean, cov, cfg), emu=fw.emulate_features(mean, cov, cfg), bf16=fw.emulate_bf16(mean, cov, cfg))
    for name, got in rows.items():
        assert np.isfinite(got).all() and np.all(got[dead] == 0), name
        w = fw.worst(got, ft["truth"], ft["bf16"] if name == "bf16" else fw.f32_budget(ft["truth"]))
        print(f"ipe_forward table {name}: worst got/budget {w:.3f}")
        assert w <= (0.5 if name == "host" else 1.0)
    # sin(+-0) keeps its sign, a denormal mean comes back as itself (or flushed: the floor)
    sin0 = rows["host"][:, :3]
    assert np.array_equal(np.signbit(sin0[mean == 0]), np.signbit(mean[mean == 0]))


def test_view_fixture():
    for B in (1, 7, 257):
        v = fw.view_dirs(B)
        assert v.shape == (B, 3) and np.isfinite(v).all()
        if B >= 7:
            assert np.any((v != 0) & (np.abs(v) < 2.0 ** -126)) and np.any(np.all((v == 0) | (np.abs(v) == 1), -1))
            norm = np.linalg.norm(v.astype(np.float64), axis=-1)
            assert np.all(np.abs(norm - 1) <= 2e-7)
        for deg in (0, 4):
            tr, exact = fw.view_truth(v, deg)
            got = fw.host_view(v, deg)
            assert got.shape == (B, 3 + 6 * deg) and np.array_equal(_bits(got[:, exact]), _bits(v))
            assert fw.worst(got, tr, fw.f32_budget(tr)) <= 0.5
