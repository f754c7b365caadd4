"""CPU: the fixture of the unbounded-scene forward path (tests/ipe360_forward.py) checked on its own, before test_gpu_ipe360_forward.py
holds k_sample_along_rays_360, k_cast_ipe_360, k_cast_ipe_360_tile, k_gauss_360 and k_lattice_ipe_360_tile to it: the host build of
csrc/raymath360.hpp against every float64 truth (the seven constants are twice its worst ratios at C = 1, measured and printed here
with the class and shape where they occur), the numpy restatements bit for bit the host build, the conditions the fixture promises
(no sample within 2^-18 of the unit sphere, enough live and informative entries at every shipped degree), the hand-made table's exact
boundary rows, the bf16 emulation inside its budget with RNE and outside it with truncation, and the power of the criteria to see each
mutation a subtly wrong kernel could carry, with the class and degree that catches it and the factor by which it misses."""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import ipe360_forward as f3

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "mipnerf_pl_amd", "csrc")
F = np.float32


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _case(cls, B, N):
    """operands, the host build's jittered fence posts, its Gaussians for both values of `contracted`, and the float64 truths"""
    c = f3.make(cls, B, N)
    t_inv, t = f3.host_sample(c["near"], c["far"], c["t_rand"], N)
    fr = f3.frustum_truth(t, c["o"], c["d"], c["r"])
    g0 = f3.host_cast(t, c["o"], c["d"], c["r"], 0, (0, 1))[:2]
    g1 = f3.host_cast(t, c["o"], c["d"], c["r"], 1, (0, 1))[:2]
    return dict(c=c, t=t, t_inv=t_inv, fr=fr, g=(g0, g1), fu=f3.fused_truth(g0[0], fr))


def _rows(cls, B, N, contracted, deg):
    k = _case(cls, B, N)
    c = k["c"]
    mean, cov = k["g"][contracted]
    return mean, cov, f3.host_cast(k["t"], c["o"], c["d"], c["r"], contracted, deg)[2]


def _all_cases():
    return [(cls, B, N) for cls in f3.CLASSES for B, N in f3.SHAPES]


def test_restated_constants_are_the_sources():
    """the basis rows, the two-float 1 / 2 pi, the exp2 factor and the fragment index rule restated in the fixture are the sources' own"""
    hdr = open(os.path.join(CSRC, "raymath360.hpp")).read()
    body = hdr[hdr.index("kBasis360[kBasis360N][3] = {"):hdr.index("// Jacobian of contract()")]
    rows = re.findall(r"\{\s*(-?[\d.]+)f,\s*(-?[\d.]+)f,\s*(-?[\d.]+)f\}", body)
    assert len(rows) == 21 and np.array_equal(np.array(rows, np.float64).astype(F), f3.BASIS)
    ker = open(os.path.join(CSRC, "kernels_360.hip")).read()
    assert f"kHi = {f3.K_HI:.8f}f, kLo = 6.4206382e-09f" in ker and F(6.4206382e-09) == f3.K_LO and "vs * -0.72134752f" in ker
    assert "((s >> 5) * (F >> 4) + (f >> 4)) * 512 + ((f >> 3) & 1) * 256 + (s & 31) * 8 + (f & 7)" in ker
    for N in sorted({N for _, N in f3.SHAPES}):
        assert np.array_equal(_bits(f3.linspace_weights(N)), _bits(f3.host_linspace(N))), N
    # (0, 8): 21 vectors per half, so the "cos" half starts on the odd lane half of a fragment; (0, 6) never reaches the tiled kernel
    assert (f3.NB * 8 // 8) % 2 == 1 and f3.tiled((0, 8)) and not f3.tiled((0, 6)) and all(f3.tiled(d) for d in f3.DEGREES[:3])
    assert [B * N for B, N in f3.SHAPES] == [1, 63, 64, 65, 258]
    f3.rows_of_fragments(np.arange(256 * 336), 65, 336)            # asserts that the rule is a permutation


def _host_constants():
    """worst ratio at C = 1 of the host build per output kind, with the case that gives it"""
    W = {}

    def upd(kind, v, tag):
        if v > W.get(kind, (-1.0, ""))[0]:
            W[kind] = (v, tag)
    for cls, B, N in _all_cases():
        k, tag = _case(cls, B, N), f"{cls} {B}x{N}"
        c = k["c"]
        near, far, t_rand = f3.sampler_operands(c)
        for tr in (None, t_rand):
            t_inv, t = f3.host_sample(near, far, tr, N)
            pt = f3.posts_truth(near, far, tr, N)
            upd("post", f3.worst(t_inv, pt["t_inv"], f3.posts_budget(pt, 1.0)), tag + (" jittered" if tr is not None else ""))
            assert f3.reciprocal_ratio(t, t_inv) <= 1.0
        (m0, c0), (m1, c1) = k["g"]
        a, b = f3.gauss_ratios(m0, c0, k["fr"], 1.0, 1.0)
        upd("mean", a, tag), upd("cov", b, tag)
        out = k["fu"]["out"]
        if out.any():
            fu = {n: v[out] for n, v in k["fu"].items()}
            a, b = f3.gauss_ratios(m1[out], c1[out], fu, 1.0, 1.0)
            upd("mean'", a, tag), upd("fused cov'", b, tag)
        gm, gc, _ = f3.host_gauss(m0, c0, 1, (0, 1))                   # the generic form on the same Gaussians
        a, b = f3.gauss_ratios(gm, gc, f3.generic_truth(m0, c0), 1.0, 1.0)
        upd("mean'", a, tag + " generic"), upd("generic cov'", b, tag)
        for contracted in (0, 1):
            for deg in f3.DEGREES:
                mean, cov, rows = _rows(cls, B, N, contracted, deg)
                ft = f3.feature_truth(mean, cov, deg, 1.0)
                upd("feature", f3.worst(rows, ft["f32"], ft["bud_f32"]), f"{tag} contracted={contracted} {f3.deg_id(deg)}")
    mm, cc = f3.table()
    gm, gc, rows = f3.host_gauss(mm, cc, 1, (0, 16))
    a, b = f3.gauss_ratios(gm, gc, f3.generic_truth(mm, cc), 1.0, 1.0)
    upd("mean'", a, "table"), upd("generic cov'", b, "table")
    ft = f3.feature_truth(gm, gc, (0, 16), 1.0)
    upd("feature", f3.worst(rows, ft["f32"], ft["bud_f32"]), "table")
    la = f3.LATTICE
    lm, lc = f3.host_lattice(**la)
    lt = f3.lattice_truth(**la)
    upd("mean", f3.worst(lm, lt["mean"], f3.U * lt["mag_mean"] + f3.FLOOR), "lattice")
    upd("cov", f3.worst(np.diagonal(lc, axis1=1, axis2=2), lt["var"], f3.U * lt["var"] + f3.FLOOR), "lattice")
    gm, gc, _ = f3.host_gauss(lm, lc, 1, (0, 16))
    a, b = f3.gauss_ratios(gm, gc, f3.generic_truth(lm, lc), 1.0, 1.0)
    upd("mean'", a, "lattice"), upd("generic cov'", b, "lattice")
    return W


def test_constants_are_twice_the_host_build():
    """each constant = twice the host build's worst ratio at C = 1 (rounded up to two digits); a ratio above 16 would mean that the
    budget's form lacks a term"""
    W = _host_constants()
    consts = {"post": f3.C_T, "mean": f3.C_M, "cov": f3.C_V, "mean'": f3.C_MC, "fused cov'": f3.C_VF, "generic cov'": f3.C_VG, "feature": f3.C_P}
    for kind, c in consts.items():
        w, tag = W[kind]
        print(f"ipe360_forward host build, {kind}: worst |got - truth| / budget at C = 1 = {w:.3f} ({tag}); constant {c}")
        assert w <= 16.0, (kind, w)
        assert w <= c / 2 <= 1.05 * w, (kind, c, w)
    assert f3.C_F == f3.fw.C_F <= f3.fw.C_F_CEILING


@pytest.mark.parametrize("cls", f3.CLASSES)
def test_host_build_and_restatements(cls):
    """per class: the numpy restatements bit for bit the host build (sampler, both Gaussians, the generic contraction), the host build
    within half of every Gaussian budget and within the feature budget, covariances symmetric bit for bit, contracted = 1 inside the
    unit ball the bits of contracted = 0, and the class's promise"""
    worst = {}

    def upd(k, v):
        worst[k] = max(worst.get(k, 0.0), v)
    for B, N in f3.SHAPES:
        k = _case(cls, B, N)
        c, t = k["c"], k["t"]
        near, far, t_rand = f3.sampler_operands(c)
        assert near[-1] == far[-1] and t_rand.min() == 0 and t_rand.max() == np.nextafter(F(1), F(0))
        for tr in (None, t_rand):
            t_inv, tt = f3.host_sample(near, far, tr, N)
            e_inv, et = f3.emulate_sample(near, far, tr, N)
            assert np.array_equal(_bits(t_inv), _bits(e_inv)) and np.array_equal(_bits(tt), _bits(et))
            pt = f3.posts_truth(near, far, tr, N)
            upd("post", f3.worst(t_inv, pt["t_inv"], f3.posts_budget(pt)))
        assert np.all(np.diff(t, axis=-1) >= 0) and np.isfinite(t).all() and t.min() > 0
        (m0, c0), (m1, c1) = k["g"]
        for contracted, (m, cv) in enumerate(k["g"]):
            em, ec = f3.emulate_cast(t, c["o"], c["d"], c["r"], contracted)
            assert np.array_equal(_bits(em), _bits(m)) and np.array_equal(_bits(ec), _bits(cv)), (cls, B, N, contracted)
            assert np.array_equal(_bits(cv), _bits(cv.swapaxes(-1, -2))) and np.isfinite(m).all() and np.isfinite(cv).all()
        out = k["fu"]["out"]
        assert np.array_equal(_bits(m1[~out]), _bits(m0[~out])) and np.array_equal(_bits(c1[~out]), _bits(c0[~out]))
        a, b = f3.gauss_ratios(m0, c0, k["fr"], f3.C_M, f3.C_V)
        upd("mean", a), upd("cov", b)
        fu = k["fu"]
        upd("mean'", f3.worst(m1[out], fu["mean"][out], f3.C_MC * f3.U * fu["mag_mean"][out] + f3.FLOOR))
        upd("fused cov'", f3.worst(c1[out], fu["cov"][out], f3.C_VF * f3.U * fu["mag_cov"][out] + f3.FLOOR))
        gm, gc, _ = f3.host_gauss(m0, c0, 1, (0, 1))
        eg = f3.emulate_generic(m0, c0)
        assert np.array_equal(_bits(eg[0]), _bits(gm)) and np.array_equal(_bits(eg[1]), _bits(gc))
        a, b = f3.gauss_ratios(gm, gc, f3.generic_truth(m0, c0), f3.C_MC, f3.C_VG)
        upd("mean'", a), upd("generic cov'", b)
        for contracted in (0, 1):
            for deg in f3.DEGREES:
                mean, cov, rows = _rows(cls, B, N, contracted, deg)
                ft = f3.feature_truth(mean, cov, deg)
                upd("feature", f3.worst(rows, ft["f32"], ft["bud_f32"]))
                upd("feature emu", f3.worst(f3.emulate_features(mean, cov, deg), ft["f32"], ft["bud_f32"]))
        # what the class is there for
        n = np.linalg.norm(m0.astype(np.float64), axis=-1)
        if cls == "near":
            assert n.max() < 1.5 and c["r"].max() <= 1e-5
        if cls == "straddle" and N > 1:
            assert (n < 1).any() and (n > 1).any()
        if cls == "radial":
            cosang = np.abs((c["o"].astype(np.float64) * c["d"]).sum(-1)) / np.linalg.norm(c["o"].astype(np.float64), axis=-1) / np.linalg.norm(c["d"].astype(np.float64), axis=-1)
            assert np.all(1 - cosang < 1e-6)
        if cls == "perpendicular":
            assert np.abs(c["d"].astype(np.float64) @ f3.BASIS.astype(np.float64).T).min(-1).max() < 1e-6
        if cls == "unnormalised":
            dn = np.linalg.norm(c["d"].astype(np.float64), axis=-1)
            assert dn.min() >= 0.49 and dn.max() <= 2.01
        if cls == "far" and N > 1:
            assert 300 < n.max() < 1300
    print(f"ipe360_forward host {cls}: worst got/budget " + " ".join(f"{k}={v:.3f}" for k, v in worst.items()))
    assert all(v <= 0.5 for k, v in worst.items() if not k.startswith("feature")), worst
    # the libm part of the feature budget does not scale with C_P, so twice the ratio at C_P = 1 leaves the host build slightly above half
    assert worst["feature"] <= 0.6 and worst["feature emu"] <= 1.0, worst


def test_live_and_informative_shares():
    """with contracted = 1, at every degree of (0, 16): at least 5 % of the fixture's feature entries have |truth| > 2^-10, and of those at
    least 99 % are informative (budget <= max(|truth| / 4, 2^-12)); the same shares for contracted = 0, reported without a cap"""
    deg, L = (0, 16), 16
    for contracted in (1, 0):
        live, inf, tot = np.zeros(L), np.zeros(L), 0
        for cls, B, N in _all_cases():
            mean, cov = _case(cls, B, N)["g"][contracted]
            ft = f3.feature_truth(mean, cov, deg)
            tr, bd = ft["f32"].reshape(-1, 2, L, f3.NB), ft["bud_f32"].reshape(-1, 2, L, f3.NB)
            lv = np.abs(tr) > 2.0 ** -10
            live += lv.sum((0, 1, 3))
            inf += (lv & f3.informative(tr, bd)).sum((0, 1, 3))
            tot += tr.shape[0] * 2 * f3.NB
        print(f"ipe360_forward contracted={contracted}: live share per degree " + " ".join(f"{v:.3f}" for v in live / tot))
        print(f"ipe360_forward contracted={contracted}: informative share of the live " + " ".join(f"{v:.4f}" for v in inf / np.maximum(live, 1)))
        if contracted:
            assert np.all(live / tot >= 0.05) and np.all(inf / live >= 0.99)


def test_table_boundary_rows_and_lattice():
    """mipnerf_gauss_360's table: the exact-boundary means (1,0,0) and (0.6,0.8,0) (fp32 n2 = 1 exactly) come back bit for bit with their
    covariances, one component at nextafter above comes back contracted; the lattice straddles |z| = 1 and its range is ragged"""
    mm, cc = f3.table()
    n2 = f3.n2_fp32(mm)
    gm, gc, _ = f3.host_gauss(mm, cc, 1, (0, 16))
    keep = n2 <= 1
    for m in ([1, 0, 0], [0.6, 0.8, 0]):
        rows = np.all(mm == np.array(m, F), -1)
        assert rows.sum() == 6 and np.all(n2[rows] == 1) and np.array_equal(_bits(gm[rows]), _bits(mm[rows])) and np.array_equal(_bits(gc[rows]), _bits(cc[rows]))
    assert np.array_equal(_bits(gm[keep]), _bits(mm[keep])) and np.array_equal(_bits(gc[keep]), _bits(cc[keep]))
    above = (n2 > 1) & (n2 < 1 + 2.0 ** -20)
    # contracted: at n = 1 + 2^-23 the mean's factor (2 - 1/n) / n rounds to 1, so the covariance shows the branch (b^2 = 1 - 2^-21 radially)
    unit = above & np.all(cc == np.eye(3, dtype=F), (1, 2))
    assert above.sum() == 3 * 6 and unit.sum() == 3 and np.all(np.any(_bits(gc[unit]) != _bits(cc[unit]), (1, 2)))
    eg = f3.emulate_generic(mm, cc)
    assert np.array_equal(_bits(eg[0]), _bits(gm)) and np.array_equal(_bits(eg[1]), _bits(gc))
    assert (cc == 0).all((1, 2)).any() and ((cc != 0) & (np.abs(cc) < 2.0 ** -126)).any() and np.linalg.norm(mm, axis=-1).max() > 400
    la = f3.LATTICE
    lm, _ = f3.host_lattice(**la)
    nz = np.linalg.norm(lm.astype(np.float64), axis=-1)
    assert (nz < 1).any() and (nz > 1).any() and la["count"] % 64 != 0 and la["first"] % 32 != 0
    assert la["first"] + la["count"] <= int(np.prod(la["dims"]))


# ---- bf16 ------------------------------------------------------------------------------------------------------------------------------
def test_bf16_emulation_and_truncation():
    """the numpy emulation of the bf16 rows (two-float reduction with its fma, exact sine and exp2, RNE) stays inside the budget on the
    whole fixture, the share it reaches is printed; truncation in place of RNE exceeds it"""
    reach, trunc = {}, {}
    for deg in f3.DEGREES[:4]:
        for cls, B, N in _all_cases():
            mean, cov = _case(cls, B, N)["g"][1]
            ft = f3.feature_truth(mean, cov, deg)
            reach[deg] = max(reach.get(deg, 0.0), f3.worst(f3.emulate_bf16(mean, cov, deg), ft["bf16"], ft["bud_bf16"]))
            trunc[deg] = max(trunc.get(deg, 0.0), f3.worst(f3.emulate_bf16(mean, cov, deg, "truncate"), ft["bf16"], ft["bud_bf16"]))
    print("ipe360_forward bf16 emulation, share of the budget reached: " + " ".join(f"{f3.deg_id(d)}={v:.3f}" for d, v in reach.items()))
    print("ipe360_forward bf16 truncation: " + " ".join(f"{f3.deg_id(d)}={v:.3f}" for d, v in trunc.items()))
    assert max(reach.values()) <= 1.0 and min(trunc.values()) > 1.5 and trunc[(0, 16)] > 1.9      # (15, 31): the phase term is part of every budget


# ---- mutations -------------------------------------------------------------------------------------------------------------------------
def _gauss_miss(mutation, cls, contracted, kind):
    """worst got/budget of the mutated Gaussian emulation over the class's shapes: (mean, cov)"""
    wm = wc = 0.0
    for B, N in f3.SHAPES:
        k = _case(cls, B, N)
        c = k["c"]
        m, cv = f3.emulate_cast(k["t"], c["o"], c["d"], c["r"], contracted, mutation)
        if contracted:
            fu, out = k["fu"], k["fu"]["out"]
            if not out.any():
                continue
            a = f3.worst(m[out], fu["mean"][out], f3.C_MC * f3.U * fu["mag_mean"][out] + f3.FLOOR)
            b = f3.worst(cv[out], fu["cov"][out], f3.C_VF * f3.U * fu["mag_cov"][out] + f3.FLOOR)
        else:
            a, b = f3.gauss_ratios(m, cv, k["fr"], f3.C_M, f3.C_V)
        wm, wc = max(wm, a), max(wc, b)
    return wm if kind == "mean" else wc


# (mutation, contracted, output, class): the named case on which the mutated Gaussian must miss
_GAUSS = [("t_var_perp", 0, "cov", "typical"),          # 1  t_var in place of r_var in the perpendicular term
          ("t_var_perp", 1, "cov", "straddle"),
          ("swap_ab", 1, "cov", "far"),                 # 3  a and b swapped
          ("mean_scale", 1, "mean", "typical"),         # 4  (2 - 1/n) without the second / n
          ("dn", 0, "cov", "unnormalised"),             # 5  dn without |d|^2
          ("dn", 1, "cov", "unnormalised"),
          ("xy_to_xz", 0, "cov", "typical"),            # 6  cov entry xy written to xz
          ("xy_to_xz", 1, "cov", "far")]


@pytest.mark.parametrize("mutation,contracted,kind,cls", _GAUSS, ids=[f"{m}-c{c}" for m, c, _, _ in _GAUSS])
def test_budget_sees_the_gaussian_mutation(mutation, contracted, kind, cls):
    base, miss = _gauss_miss(None, cls, contracted, kind), _gauss_miss(mutation, cls, contracted, kind)
    print(f"ipe360_forward mutation {mutation} (contracted={contracted}, {kind}) on {cls}: got/budget {miss:.3g} (unmutated {base:.3g})")
    assert base <= 0.5 and miss > 100.0
    if mutation == "dn":                                 # a normalised d hides it: that is why `unnormalised` exists
        assert _gauss_miss(mutation, "near", contracted, kind) <= 1.0


def test_budget_sees_the_generic_mutations():
    """2 (J in place of J C J^T), 3 and 4 on contract_gaussian: `far` and the hand-made table"""
    for mutation, kind in (("jacobian_only", 1), ("swap_ab", 1), ("mean_scale", 0)):
        res = {}
        for name, (mm, cc) in (("far 2x129", _case("far", 2, 129)["g"][0]), ("table", f3.table())):
            tr = f3.generic_truth(mm, cc)
            base = f3.gauss_ratios(*f3.emulate_generic(mm, cc), tr, f3.C_MC, f3.C_VG)[kind]
            res[name] = f3.gauss_ratios(*f3.emulate_generic(mm, cc, mutation), tr, f3.C_MC, f3.C_VG)[kind]
            assert base <= 0.5
        print(f"ipe360_forward mutation {mutation} (generic): got/budget " + " ".join(f"{k}={v:.3g}" for k, v in res.items()))
        assert min(res.values()) > 100.0


def _feature_miss(emulate, key, mutation, cls, deg, contracted=1):
    w = 0.0
    for B, N in f3.SHAPES:
        mean, cov = _case(cls, B, N)["g"][contracted]
        ft = f3.feature_truth(mean, cov, deg)
        w = max(w, f3.worst(emulate(mean, cov, deg, mutation), ft[key], ft["bud_" + key]))
    return w


# (mutation, class, degrees): the named case on which the mutated fp32 rows must miss the float64 budget
_FEATURE = [("basis_negated", "typical", (0, 16)),       # 7  a basis row negated: the sine half of that direction changes its sign
            ("wrap_direction", "straddle", (0, 16)),     # 8  direction index off by one at the 21-to-next-degree wrap of a vector
            ("wrap_direction", "near", (0, 8)),
            ("damp_2l", "typical", (3, 19)),             # 9  4^l replaced by 2^l in the damping
            ("cos_next_degree", "near", (0, 16))]        # 10 the "cos" half taken from degree l + 1


@pytest.mark.parametrize("mutation,cls,deg", _FEATURE, ids=[f"{m}-{f3.deg_id(d)}" for m, _, d in _FEATURE])
def test_budget_sees_the_feature_mutation(mutation, cls, deg):
    base = _feature_miss(f3.emulate_features, "f32", None, cls, deg)
    miss = _feature_miss(f3.emulate_features, "f32", mutation, cls, deg)
    print(f"ipe360_forward mutation {mutation} on {cls} {f3.deg_id(deg)}: got/budget {miss:.3g} (unmutated {base:.3g})")
    assert base <= 1.0 and miss > 100.0


def test_mutations_below_the_conditioning_need_the_projection_criterion():
    """11 (fp32 rows using the true cosine) and 12 (the bf16 reduction without its `lo` term) change the phase by at most u |x| and
    0.68 u |x|.  The float64 budget starts from the fp32 (mean, cov) and has to grant the projection y = p . mean its rounding,
    C_P u 2^l sum |m_a p_a| >= 6.5 u |x|: no budget derived from (mean, cov) can see either, whatever the class or degree (measured
    below: both stay inside it everywhere).  They are seen one step later, where the phase is an exact operand: against the truth at the
    fp32 projection the host build forms (ipe360_forward.projection_truth, ipe_forward's budgets), where the host build and the
    unmutated emulations pass.  `near`, degrees (3, 19) and (15, 31), catches both."""
    inside = {}
    for mutation, emulate, key in (("true_cos", f3.emulate_features, "f32"), ("no_lo", f3.emulate_bf16, "bf16")):
        inside[mutation] = max(_feature_miss(emulate, key, mutation, cls, deg) for cls in f3.CLASSES for deg in f3.DEGREES[:3])
    print("ipe360_forward mutations inside the float64 budget everywhere: " + " ".join(f"{k}={v:.3f}" for k, v in inside.items()))
    assert max(inside.values()) <= 1.0
    for deg in ((3, 19), (15, 31)):
        res = {}
        for B, N in f3.SHAPES:
            mean, cov, rows = _rows("near", B, N, 1, deg)
            pt = f3.projection_truth(mean, cov, deg)
            for name, got, key in (("host", rows, "f32"), ("f32", f3.emulate_features(mean, cov, deg), "f32"),
                                   ("true_cos", f3.emulate_features(mean, cov, deg, "true_cos"), "f32"),
                                   ("bf16", f3.emulate_bf16(mean, cov, deg), "bf16"), ("no_lo", f3.emulate_bf16(mean, cov, deg, "no_lo"), "bf16"),
                                   ("truncate", f3.emulate_bf16(mean, cov, deg, "truncate"), "bf16")):
                res[name] = max(res.get(name, 0.0), f3.worst(got, pt[key], pt["bud_" + key]))
        print(f"ipe360_forward projection criterion, near {f3.deg_id(deg)}: got/budget " + " ".join(f"{k}={v:.3g}" for k, v in res.items()))
        assert res["host"] <= 0.5 and res["f32"] <= 0.5 and res["bf16"] <= 1.0
        assert res["true_cos"] > 100.0 and res["no_lo"] > 100.0 and res["truncate"] > 1.9


def test_mutation_t_from_the_unjittered_post():
    """13: t = 1 / t_inv taken from the fence post before the jitter -- every class with t_rand sees it in the 1 u criterion on t"""
    for cls in f3.CLASSES:
        c = f3.make(cls, 5, 13)
        t_inv, t = f3.emulate_sample(c["near"], c["far"], c["t_rand"], 13)
        m_inv, mt = f3.emulate_sample(c["near"], c["far"], c["t_rand"], 13, "t_unjittered")
        assert np.array_equal(t_inv, m_inv)
        base, miss = f3.reciprocal_ratio(t, t_inv), f3.reciprocal_ratio(mt, m_inv)
        print(f"ipe360_forward mutation t_unjittered on {cls}: got/budget {miss:.3g} (unmutated {base:.3g})")
        assert base <= 1.0 and miss > 10.0                   # `near`: the rays are thin, the jitter moves t by 55 u only
        assert f3.reciprocal_ratio(*f3.emulate_sample(c["near"], c["far"], None, 13, "t_unjittered")[::-1]) <= 1.0     # nothing to see without jitter


def test_hostmath_stand_alone_program():
    """the stand-alone program over the new hostmath entry points (its own main; the build to run under -fsanitize=address,undefined)"""
    exe = os.path.join(HERE, "hostmath", "_ipe360_selftest")
    src = os.path.join(HERE, "hostmath", "ipe360_selftest.cpp")
    subprocess.check_call(["g++", "-O1", "-g", "-ffp-contract=off", src, "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    sys.stdout.write(out.stdout)
    assert out.returncode == 0 and "ok" in out.stdout, out.stderr
