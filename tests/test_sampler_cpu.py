"""CPU: the fixture of the inverse-CDF sampler's per-entry probes (tests/sampler_fixture.py) checked on its own, before
test_gpu_sampler.py holds pdf_ray and k_resample_bwd to it: the engineered ties, the closed-form backward truth against torch float64
autograd, the conditions on the inputs (fragile shares), the shipped budgets against the fp32 emulation of both kernels (the worst
ratios are the figures next to C_F and C_B), and the budgets' power to see nine mutations of the arithmetic, beside what the earlier
criteria (forward: batch maximum <= 1e-4; backward: error over the batch's largest gradient <= 2e-3) make of each."""
import numpy as np
import pytest
import torch

import sampler_fixture as sf

D = np.float64


def _blur_cases(classes=sf.BLUR_CLASSES, sizes=None, decreasing=True):
    for cls in classes:
        for N in sf.sizes_of(cls):
            if sizes is not None and N not in sizes:
                continue
            for padding in sf.paddings_of(cls):
                for rnd in (False, True):
                    for dec in ((False, True) if decreasing and not rnd else (False,)):
                        yield cls, N, padding, rnd, dec, sf.blur_case(cls, N, padding, rnd, dec)


def _noblur_cases(classes=sf.NOBLUR_CLASSES, sizes=sf.NOBLUR_SIZES):
    for cls in classes:
        for N in sizes:
            for n in sf.noblur_draw_counts(N):
                for rnd in (False, True):
                    yield cls, N, n, rnd, sf.noblur_case(cls, N, n, rnd)


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------
def test_engineered_ties_exist_for_every_draw():
    """the search of engineered_ties succeeds for every j, and the kernel's expression then gives j / N exactly"""
    for N in sf.TIE_SIZES:
        r, ok = sf.engineered_ties(N)
        assert ok.all(), (N, np.nonzero(~ok)[0])
        assert r.dtype == np.float32 and np.all(r >= 0) and np.all(r < 1)
        u = sf.u_of(r[None, :], N + 1)[0]
        j = np.arange(1, N)
        assert np.array_equal(u[1:N].astype(D), j / N) and u[0] == 0
        # and both routes put such a draw at the lower edge of interval j, to the bit
        c = sf.blur_case("uniform_ties", N, 0.01, True)
        tr = sf.forward_truth(c["bins"], c["w"], c["u"], True, 0.01)
        em = sf.emulate_forward(c["bins"], c["w"], c["u"], True, 0.01)
        assert np.array_equal(tr["cdf"], np.tile(np.arange(N + 1) / N, (sf.RAYS, 1))) and np.array_equal(em["cdf"].astype(D), tr["cdf"])
        assert np.array_equal(em["t"][:, 1:N], c["bins"][:, 1:N]) and not tr["fragile"][:, :N].any()


def test_draws_and_input_conditions():
    assert [sf.lane_bucket(N) for N in sf.SIZES] == [1, 1, 1, 2, 4, 8, 16, 16]
    for n in (1, 2, 6, 65, 128, 1025, 1089):
        want = torch.linspace(0.0, float(sf.UMAX), n, dtype=torch.float32).numpy()
        assert np.array_equal(sf.linspace_u(n), want), n                     # ATen's linspace, bit for bit
    for cls, N, padding, rnd, dec, c in _blur_cases():
        assert c["w"].shape == (sf.RAYS, N) and c["bins"].shape == (sf.RAYS, N + 1) and c["u"].shape == (sf.RAYS, N + 1)
        assert np.all(np.diff(c["u"], axis=-1) >= 0)
        d = np.diff(c["bins"], axis=-1)
        assert np.all(d < 0) if dec else np.all(d > 0)
        assert np.all(c["w"] >= 0) and np.all(c["w"].astype(D).sum(-1) <= 1 + 1e-6)
        if cls == "tiny":                                                    # the pad > 0 branch, with weights that differ
            st = sf.emulate_forward(c["bins"], c["w"], c["u"], True, padding)
            assert padding == 0.0 and np.all(st["pad"] > 0) and np.all(c["w"] > 0)
            assert N == 1 or np.all(c["w"].max(-1) > 1.5 * c["w"].min(-1))
        if cls == "plateau" and N >= 4:
            assert np.all(c["w"][:, 0] == c["w"][:, 1]) and np.all(c["w"][:, -1] == c["w"][:, -2])
        if cls == "onehot":
            assert np.all((c["w"] == 1).sum(-1) == 1) and np.all((c["w"] == 0).sum(-1) == N - 1)
    hot = set(sf.onehot_bins(sf.RAYS, 300).tolist())
    assert {0, 299, 150, 7, 8, 255, 256, 127, 128} == hot                    # K = 8: lanes 0 | 1, DPP rows, the half wave


def test_fragile_shares():
    """at most 1 % of a case's draws are fragile, except in the deterministic cases whose draws sit on cdf entries by construction; on
    the no-blur route the draws left out (fragile next to a bin of mass < 1e-5) are the only ones not compared"""
    share = {}
    for cls, N, padding, rnd, dec, c in _blur_cases():
        tr = sf.forward_truth(c["bins"], c["w"], c["u"], True, padding)
        assert not tr["left_out"].any(), (cls, N)                            # the blur route has no bin of mass < 1e-5
        f = float(tr["fragile"].mean())
        key = (cls, "aligned" if sf.aligned_case(cls, N, rnd) else "other")
        share[key] = max(share.get(key, 0.0), f)
        if sf.aligned_case(cls, N, rnd):
            if cls != "onehot" and N >= 2:
                assert tr["fragile"][:, 1:N].all(), (cls, N)                 # every interior draw
        else:
            assert f <= 0.01, (cls, N, padding, rnd, dec, f)
    for (cls, kind), f in sorted(share.items()):
        print(f"sampler fragile share, blur route, {cls} ({kind}): worst case {100 * f:.3f} %")
    for cls, N, n, rnd, c in _noblur_cases():
        tr = sf.forward_truth(c["bins"], c["w"], c["u"], False, 0.0)
        assert np.all(tr["fragile"] | ~tr["left_out"])
        if cls == "sliver" and not rnd and n >= 3:                           # the draw placed in the sliver is compared
            small = np.take_along_axis(tr["pdf"], tr["bin"], -1) < 1e-5
            in_sliver = small & (np.take_along_axis(tr["pdf"], tr["bin"], -1) > 0) & ~tr["left_out"]
            assert in_sliver.any(-1).all(), (N, n)


# ---- truth ------------------------------------------------------------------------------------------------------------------------------
def _autograd(c, padding, k, g):
    """torch float64 autograd of sum(t' g) w.r.t. the weights, given the interval k of every draw"""
    f8 = torch.float64
    w = torch.from_numpy(c["w"].astype(D)).requires_grad_(True)
    bins, u = torch.from_numpy(c["bins"].astype(D)), torch.from_numpy(c["u"].astype(D))
    N = w.shape[-1]
    wp = torch.cat([w[:, :1], w, w[:, -1:]], -1)
    mx = torch.maximum(wp[:, :-1], wp[:, 1:])
    v = 0.5 * (mx[:, :-1] + mx[:, 1:]) + float(np.float32(padding))
    s = v.sum(-1, keepdim=True)
    pad = torch.clamp(float(sf.E5) - s, min=0)
    v, s = v + pad / N, s + pad
    pdf = v / s
    one = torch.ones_like(pdf[:, :1])
    cdf = torch.cat([0 * one, torch.minimum(one, torch.cumsum(pdf[:, :-1], -1)), one], -1)
    k = torch.from_numpy(k)
    c0, c1, b0, b1 = (torch.gather(a, 1, i) for a, i in ((cdf, k), (cdf, k + 1), (bins, k), (bins, k + 1)))
    den = c1 - c0
    den = torch.where(den < float(sf.E5), torch.ones_like(den), den)
    t = b0 + (u - c0) / den * (b1 - b0)
    (t * torch.from_numpy(g.astype(D)).to(f8)).sum().backward()
    return t.detach().numpy(), w.grad.numpy()


@pytest.mark.parametrize("cls,N,padding,rnd", [("soft", 5, 0.01, False), ("soft", 65, 0.01, True), ("plateau", 65, 0.01, False),
                                               ("tiny", 5, 0.0, False), ("tiny", 65, 0.0, True), ("empty", 5, 0.0, True),
                                               ("empty", 5, 0.01, False), ("onehot", 65, 0.01, False), ("surface", 5, 0.01, True),
                                               ("uniform_ties", 4, 0.01, True), ("soft", 1, 0.01, False)])
def test_closed_form_matches_float64_autograd(cls, N, padding, rnd):
    """the adjoint with its explicit half shares against torch.maximum / torch.minimum / torch.clamp under autograd, given the same
    memberships: 1e-9 of the entry's abs-sum (the budget's Mw), for a dense g, for every one-hot probe and for the other membership
    of the fragile draws"""
    c = sf.blur_case(cls, N, padding, rnd)
    tr = sf.forward_truth(c["bins"], c["w"], c["u"], True, padding)
    gs = [(g, tr["bin"]) for _, g, _ in sf._probes(tr, c["rng"], True if N >= 4 and tr["fragile"].any(-1).all() else False)]
    gs.append((np.random.default_rng(N).standard_normal(c["u"].shape).astype(np.float32), tr["bin"]))
    gs.append((gs[-1][0], tr["alt"]))
    for g, k in gs:
        t, want = _autograd(c, padding, k, g)
        if k is tr["bin"]:
            assert np.abs(t - tr["t"]).max() <= 1e-13
        got, budget = sf.backward_truth(tr, g, k, c_b=1.0)
        mw = (budget - sf.FLOOR) / sf.U
        assert np.all(np.abs(got - want) <= 1e-9 * mw + 1e-300), (cls, N, float((np.abs(got - want) / np.maximum(mw, 1e-300)).max()))
        assert np.all(np.abs(want) <= mw * (1 + 1e-9) + 1e-300)             # the abs-sum bounds the entry


# ---- emulation against the shipped budgets --------------------------------------------------------------------------------------
def _backward_worst(tr, em, probes):
    worst = {}
    for name, g, either in probes:
        worst[name] = float(sf.backward_ratio(sf.emulate_backward(em, g), tr, g, either).max())
    return worst


def test_emulation_meets_half_the_shipped_budgets():
    """every draw and every d_weights entry of every class, size, padding, route and probe: emulation / budget <= 0.5.  The printed
    worst ratios at C = 1 are the figures next to C_F and C_B.  Also the derived bound on |cdf32 - cdf64| behind the guard band."""
    wf, wn, wb, cdf_err = {}, {}, {}, 0.0
    for cls, N, padding, rnd, dec, c in _blur_cases():
        tr = sf.forward_truth(c["bins"], c["w"], c["u"], True, padding)
        em = sf.emulate_forward(c["bins"], c["w"], c["u"], True, padding)
        cdf_err = max(cdf_err, float((np.abs(em["cdf"].astype(D) - tr["cdf"]) / np.maximum(tr["cdf"], 1e-300)).max()))
        r = sf.forward_ratio(em["t"], tr)
        assert r <= 0.5, (cls, N, padding, rnd, dec, r)
        wf[cls] = max(wf.get(cls, 0.0), r * sf.C_F)
        # the exact structure the GPU test asserts holds in the emulation as well
        d = np.diff(em["t"], axis=-1)
        assert np.all(d <= 0) if dec else np.all(d >= 0)
        assert em["t"].min() >= c["bins"].min(-1).min() and np.all(em["t"] <= c["bins"].max(-1, keepdims=True))
        if dec:
            continue
        probes = sf.probes(tr, c["rng"], cls, rnd)
        if sf.aligned_case(cls, N, rnd) and N >= 4:
            either = [g for name, g, _ in probes if name.startswith("either")]
            assert len(either) == sf.EITHER_OR                                # none of them empty: one fragile draw on every ray that has one
            assert all(np.array_equal(np.abs(g).sum(-1) == 1, tr["fragile"].any(-1)) and np.all(tr["fragile"][g != 0]) for g in either)
            assert tr["fragile"].any(-1).all() or cls == "onehot"
        for name, r in _backward_worst(tr, em, probes).items():
            assert r <= 0.5, (cls, N, padding, rnd, name, r)
            wb[cls] = max(wb.get(cls, 0.0), r * sf.C_B)
    for cls, N, n, rnd, c in _noblur_cases():
        tr = sf.forward_truth(c["bins"], c["w"], c["u"], False, 0.0)
        em = sf.emulate_forward(c["bins"], c["w"], c["u"], False, 0.0)
        r = sf.forward_ratio(em["t"], tr)
        assert r <= 0.5, (cls, N, n, rnd, r)
        wn[cls] = max(wn.get(cls, 0.0), r * sf.C_F)
        assert np.all(np.diff(em["t"], axis=-1) >= 0)
        assert np.all(em["t"] >= c["bins"].min(-1, keepdims=True)) and np.all(em["t"] <= c["bins"].max(-1, keepdims=True))
        mass = np.take_along_axis(tr["pdf"], tr["bin"], -1)
        inside = (mass > 0) & (mass < 1e-5) & ~tr["fragile"]
        b0, b1 = (np.take_along_axis(c["bins"], tr["bin"] + o, -1).astype(D) for o in (0, 1))
        assert np.all(((em["t"] >= b0) & (em["t"] <= b0 + 1e-5 * (b1 - b0)))[inside])
        lead = (np.cumsum(c["w"], -1) == 0).sum(-1)                           # leading zero-weight bins: draw 0 at the first bin with mass
        if not rnd:
            first = np.take_along_axis(c["bins"], np.minimum(lead, N - 1)[:, None], -1)[:, 0]
            assert np.array_equal(em["t"][:, 0], np.where(lead < N, first, c["bins"][:, 0]))
    for tag, d in (("forward, blur route", wf), ("forward, no-blur route", wn), ("backward", wb)):
        print(f"sampler emulation / budget at C = 1, {tag}: worst {max(d.values()):.3f}  (" + " ".join(f"{k}={v:.3f}" for k, v in d.items()) + ")")
    print(f"sampler emulation: worst |cdf32 - cdf64| / cdf64 = {cdf_err / sf.U:.2f} x 2^-24 (bound {sf.CDF_BOUND / sf.U}, band {sf.BAND / sf.U})")
    assert cdf_err <= sf.CDF_BOUND
    # the constants are twice the measured worst ratios, no more
    assert max(wf.values()) <= 0.5 * sf.C_F and max(wn.values()) <= 0.5 * sf.C_F and max(wb.values()) <= 0.5 * sf.C_B
    assert max(max(wf.values()), max(wn.values())) >= 0.45 * sf.C_F and max(wb.values()) >= 0.45 * sf.C_B


# ---- mutations --------------------------------------------------------------------------------------------------------------------------
MUT_SIZES = (1, 4, 5, 64, 65, 129)


def _old_forward(t_mut, tr):
    """the earlier criterion: the largest absolute difference of the batch <= 1e-4"""
    return float(np.abs(t_mut.astype(D) - tr["t"]).max()) > 1e-4


def _old_backward(d_mut, want):
    """the earlier criterion: the largest error over the batch's largest gradient <= 2e-3"""
    return float(np.abs(d_mut.astype(D) - want).max()) > 2e-3 * max(float(np.abs(want).max()), 1e-30)


@pytest.mark.parametrize("mut", sf.FORWARD_MUTATIONS)
def test_forward_budget_sees_mutation(mut):
    """the mutated emulation exceeds some draw's budget by 4 x or more.  Old criterion: on `soft` weights with N + 1 draws (the kind of
    input the earlier tests use) and on any case of this fixture."""
    worst, old_soft, old_any, where = 0.0, set(), False, None
    for cls, N, padding, rnd, dec, c in _blur_cases(sizes=MUT_SIZES, decreasing=False):
        tr = sf.forward_truth(c["bins"], c["w"], c["u"], True, padding)
        t = sf.emulate_forward(c["bins"], c["w"], c["u"], True, padding, mut=mut)["t"]
        r = sf.forward_ratio(t, tr)
        if r > worst:
            worst, where = r, ("blur", cls, N, padding, rnd)
        old = _old_forward(t, tr)
        old_any |= old
        if old and cls == "soft":
            old_soft.add(N)
    for cls, N, n, rnd, c in _noblur_cases(sizes=(5, 64, 129)):
        tr = sf.forward_truth(c["bins"], c["w"], c["u"], False, 0.0)
        t = sf.emulate_forward(c["bins"], c["w"], c["u"], False, 0.0, mut=mut)["t"]
        r = sf.forward_ratio(t, tr)
        if r > worst:
            worst, where = r, ("no-blur", cls, N, n, rnd)
        old = _old_forward(t, tr)
        old_any |= old
        if old and cls == "soft" and n == N + 1:
            old_soft.add(N)
    print(f"sampler mutation forward {mut}: worst got / budget {worst:.3g} at {where}; old criterion notices it on soft inputs at N in "
          f"{sorted(old_soft)} of {MUT_SIZES}, on any case of this fixture: {old_any}")
    assert worst >= 4.0


@pytest.mark.parametrize("mut", sf.BACKWARD_MUTATIONS)
def test_backward_budget_sees_mutation(mut):
    worst, old_soft, old_any, where = 0.0, set(), False, None
    for cls, N, padding, rnd, dec, c in _blur_cases(sizes=MUT_SIZES, decreasing=False):
        tr = sf.forward_truth(c["bins"], c["w"], c["u"], True, padding)
        em = sf.emulate_forward(c["bins"], c["w"], c["u"], True, padding, mut="left" if mut == "left" else None)
        for name, g, either in sf.probes(tr, c["rng"], cls, rnd):
            d_w = sf.emulate_backward(em, g, mut=mut)
            r = float(sf.backward_ratio(d_w, tr, g, either).max())
            if r > worst:
                worst, where = r, (cls, N, padding, rnd, name)
            if name == "dense":
                old = _old_backward(d_w, sf.backward_truth(tr, g)[0])
                old_any |= old
                if old and cls == "soft":
                    old_soft.add(N)
    print(f"sampler mutation backward {mut}: worst got / budget {worst:.3g} at {where}; old criterion (dense g) notices it on soft "
          f"inputs at N in {sorted(old_soft)} of {MUT_SIZES}, on any case of this fixture: {old_any}")
    assert worst >= 4.0
