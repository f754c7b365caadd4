"""CPU: the fixture of the IPE backward's Jacobian probes (tests/ipe_jacobian.py) checked on its own, before test_gpu_ipe_jacobian.py
holds k_cast_ipe_bwd to it: the closed-form adjoint against float64 autograd, the property that names each class, the numpy emulation
of the kernel against the shipped budget (the worst ratios at C = 1 are the figures next to C_BUDGET), and the budget's power to see
each of the mutations a subtly wrong kernel could carry.  The Gaussians come from the host build of csrc/raymath.hpp."""
import functools

import numpy as np
import pytest
import torch

import ipe_jacobian as ij


@functools.lru_cache(maxsize=None)
def _case(cls, cfg, B, N):
    rng = np.random.default_rng(ij.case_seed(cls, cfg, B, N))
    t, o, d, r, info = ij.make(cls, B, N, rng)
    mean, cov = ij.host_gaussians(t, o, d, r)
    return (t, o, d, r, mean, cov), info, ij.Jacobian(t, o, d, r, mean, cov, cfg)


def _probes(cls, cfg, B, N):
    return ij.probes(B, N, cfg[1] - cfg[0], np.random.default_rng(ij.case_seed(cls, cfg, B, N) + 1))


def _autograd(ops, cfg, g):
    """d_t of sum(features * g) by float64 torch autograd: the chain of t_cast_ipe (test_gpu_resample_grad.py) with pi / 2 in float64,
    shifted by constants so that the features are taken at the forward's fp32 (mean, cov)"""
    t, o, d, r, mean, cov = (torch.from_numpy(a).double() for a in ops)
    min_deg, max_deg, noint = cfg
    t.requires_grad_(True)
    t0, t1 = t[:, :-1], t[:, 1:]
    mu, hw = (t0 + t1) / 2, (t1 - t0) / 2
    den = 3 * mu ** 2 + hw ** 2
    t_mean = mu + 2 * mu * hw ** 2 / den
    t_var = hw ** 2 / 3 - (4 / 15) * (hw ** 4 * (12 * mu ** 2 - hw ** 2)) / den ** 2
    r_var = r[:, None] ** 2 * (mu ** 2 / 4 + (5 / 12) * hw ** 2 - (4 / 15) * hw ** 4 / den)
    m = d[:, None, :] * t_mean[..., None] + o[:, None, :]
    d2 = d ** 2
    null = 1 - d2 / (d2.sum(-1, keepdim=True) + 1e-10)
    c = t_var[..., None] * d2[:, None, :] + r_var[..., None] * null[:, None, :]
    m, c = m + (mean - m).detach(), c + (cov - c).detach()
    scales = torch.tensor([2.0 ** i for i in range(min_deg, max_deg)], dtype=torch.float64)
    y = (m[..., None, :] * scales[:, None]).flatten(-2)
    yv = (c[..., None, :] * scales[:, None] ** 2).flatten(-2)
    if noint:
        yv = torch.zeros_like(yv)
    enc = torch.exp(-0.5 * torch.cat([yv, yv], -1)) * torch.sin(torch.cat([y, y + 0.5 * np.pi], -1))
    (enc * torch.from_numpy(g).double()).sum().backward()
    return t.grad.numpy()


@pytest.mark.parametrize("cfg", ij.CONFIGS, ids=ij.config_id)
@pytest.mark.parametrize("cls", ij.CLASSES)
def test_adjoint_matches_float64_autograd(cls, cfg):
    """1e-10 of each entry's sum of absolute terms, at (5, 5) and (3, 171), for a one-hot, a dense and a pre-filled probe"""
    for B, N in ((5, 5), (3, 171)):
        ops, _, jac = _case(cls, cfg, B, N)
        for kind, name, g, pre in _probes(cls, cfg, B, N):
            if name not in ("onehot0_0", "onehot0_1", "dense", "accumulate"):
                continue
            tr = jac.truth(g, pre)
            want = _autograd(ops, cfg, g) + (0.0 if pre is None else pre.astype(np.float64))
            assert np.all(np.abs(want - tr["d_t"]) <= 1e-10 * tr["M"] + 1e-300), (cls, cfg, B, N, name)


@pytest.mark.parametrize("cls", ij.CLASSES)
def test_class_properties(cls):
    cfg = ij.CONFIGS[0]
    for B, N in ij.SHAPES:
        (t, o, d, r, mean, cov), info, jac = _case(cls, cfg, B, N)
        assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in (t, o, d, r, mean, cov))
        assert t.shape == (B, N + 1) and o.shape == (B, 3) and d.shape == (B, 3) and r.shape == (B,) and np.all(np.diff(t, axis=-1) >= 0)
        q = ij.hw_over_mu(t)
        if cls in ("scene", "coarse_pixel", "axis"):
            assert t.min() >= 2.0 and t.max() <= 6.0 and np.all(q > 0)
        if cls == "scene":
            assert set(np.round(r / np.float32(ij.FINEST_RADIUS)).astype(int)) <= {1, 2, 4, 8}
        if cls == "thin":
            rep = info["repeated"]
            assert np.all(rep >= 0) if N > 1 else (np.any(rep >= 0) and np.any(rep < 0))
            for b in range(B):
                zero = q[b] == 0
                assert zero.sum() == (rep[b] >= 0) and (rep[b] < 0 or zero[rep[b]])          # exactly the repeated post has hw == 0
                assert np.all(q[b][~zero] >= 0.9e-6) and np.all(q[b][~zero] <= 2.1e-3)
            if N >= 64:
                assert q[q > 0].min() < 3e-6 and q.max() > 3e-4
        if cls == "wide":
            nw = info["n_wide"]
            assert nw == min(N, 3) and np.all(q[:, :nw] >= 0.3 - 1e-6) and np.all(q[:, :nw] <= 0.98)
            assert q[:, 0].max() >= 0.96                                                      # one sample from near to far: hw^4 matters
        if cls == "axis":
            zero_axes = d == 0
            assert np.all(zero_axes.sum(-1) == np.where(info["in_plane"], 1, 2))
            assert np.allclose(np.linalg.norm(d.astype(np.float64), axis=-1), info["norm"], rtol=1e-6)
            if B >= 5:
                assert info["in_plane"].any() and (~info["in_plane"]).any() and set(info["norm"]) == set(ij.AXIS_NORMS)
            # a feature on a zero-direction axis depends on t through r_var alone: the t_mean and t_var terms are exactly 0, and the
            # r_var terms are not wherever the damping has not underflowed
            L = jac.L
            ax = np.tile(np.arange(3), 2 * L)
            on_zero = zero_axes[:, None, ax] & np.ones((1, N, 1), bool)
            for k in ("tm_mu", "tm_hw", "tv_mu", "tv_hw"):
                assert np.all(jac.terms[k][on_zero] == 0)
            alive = on_zero & (np.concatenate([jac.damp.reshape(B, N, 3 * L)] * 2, -1) > 1e-300)
            assert alive.sum() >= on_zero.sum() // 4
            assert np.all(jac.terms["rv_mu"][alive] != 0)
            g = (rng_like(B, N, L) * on_zero).astype(np.float32)
            full, rv = jac.truth(g), jac.truth(g, only=("rv_mu", "rv_hw"))
            assert np.array_equal(full["d_t"], rv["d_t"]) and np.all(full["d_t"] != 0)
        if cls == "coarse_pixel":
            assert set(np.round(r / np.float32(ij.FINEST_RADIUS)).astype(int)) == {8, 64}
            damp8 = jac.damp[:, :, 8, :].min(-1).max(-1)                                      # degree 2^8, the axis r_var damps most
            assert np.all(damp8[r > 0.02] < 1e-6) and np.all(jac.damp[:, :, 0, :] > 0.1)
        if cls == "far":
            assert t.max() == 100.0 and 1e6 <= jac.phase_max <= 4e6
            assert np.any(jac.damp == 0) and np.any(jac.damp > 0.5)
    # with (0, 31) every class has damping factors that underflow to exactly 0
    _, _, jac = _case(cls, ij.CONFIGS[3], 5, 5)
    assert np.any(jac.damp == 0)


def rng_like(B, N, L):
    return np.random.default_rng(B * 1000 + N).standard_normal((B, N, 6 * L))


def _worst(ops, jac, cfg, probes, c_budget=ij.C_BUDGET, **kw):
    worst = {}
    for kind, name, g, pre in probes:
        tr = jac.truth(g, pre, c_budget=c_budget)
        a, b = ij.emulate(*ops, cfg, g, pre, **kw)
        worst[kind] = max(worst.get(kind, 0.0), ij.ratio(a, tr), ij.ratio(b, tr))
    return worst


@pytest.mark.parametrize("cfg", ij.CONFIGS, ids=ij.config_id)
@pytest.mark.parametrize("cls", ij.CLASSES)
def test_emulation_meets_the_shipped_budget(cls, cfg):
    """every entry of every probe at every shape, both add orders; prints the worst ratios at C = 1"""
    worst1 = {}
    for B, N in ij.SHAPES:
        ops, _, jac = _case(cls, cfg, B, N)
        L = jac.L
        for k, v in _worst(ops, jac, cfg, _probes(cls, cfg, B, N), c_budget=1.0).items():
            worst1[k] = max(worst1.get(k, 0.0), v)
        assert max(_worst(ops, jac, cfg, _probes(cls, cfg, B, N)).values()) <= 1.0, (cls, cfg, B, N)
        # exact structure the GPU test asserts: posts that touch no driven sample are 0, underflowed damping gives 0, zero d_enc keeps the bits
        for rnd in range(ij.onehot_rounds(B, N, L)):
            for parity in ((0,) if N == 1 else (0, 1)):
                g, touched, feat, drive = ij.onehot_probe(B, N, L, rnd, parity)
                a, b = ij.emulate(*ops, cfg, g)
                assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and np.all(a[~touched] == 0)
                dead = drive & (np.concatenate([jac.damp.reshape(B, N, 3 * L)] * 2, -1)[np.arange(B)[:, None], np.arange(N)[None, :], feat] == 0)
                assert np.all(a[:, :-1][dead] == 0) and np.all(a[:, 1:][dead] == 0)
        pre = np.random.default_rng(3).standard_normal((B, N + 1)).astype(np.float32)
        a, b = ij.emulate(*ops, cfg, np.zeros((B, N, 6 * L), np.float32), pre)
        assert np.array_equal(a.view(np.uint32), pre.view(np.uint32)) and np.array_equal(b.view(np.uint32), pre.view(np.uint32))
    print(f"ipe_jacobian emulation {cls} {ij.config_id(cfg)}: worst / budget at C = 1: " + " ".join(f"{k}={v:.2f}" for k, v in worst1.items()))
    assert max(worst1.values()) <= ij.C_BUDGET / 2


def test_fp32_phase_add_misses_the_budget():
    """the "cos" phase as fl32(y + fl32(pi/2)) -- the kernel before this fixture -- is off by up to half an ulp of y in the phase:
    the cos_half and one-hot probes miss the budget in every class with integration on or off"""
    for cls in ij.CLASSES:
        for cfg in ij.CONFIGS[:2]:
            ops, _, jac = _case(cls, cfg, 5, 64)
            w = _worst(ops, jac, cfg, _probes(cls, cfg, 5, 64), fp32_phase_add=True)
            print(f"ipe_jacobian fp32 phase add {cls} {ij.config_id(cfg)}: " + " ".join(f"{k}={v:.3g}" for k, v in w.items()))
            assert w["cos_half"] > 1.0 and w["onehot"] > 1.0 and w["sin_half"] <= 1.0


@pytest.mark.parametrize("mutation", ij.MUTATIONS)
def test_budget_sees_the_mutation(mutation):
    """each mutation of the emulation's arithmetic pushes the worst got / budget above 1 in at least one class"""
    seen = {}
    for cls in ij.CLASSES:
        cfg, (B, N) = ij.CONFIGS[0], (5, 64)
        ops, _, jac = _case(cls, cfg, B, N)
        seen[cls] = max(_worst(ops, jac, cfg, _probes(cls, cfg, B, N), mutation=mutation).values())
    print(f"ipe_jacobian mutation {mutation}: " + " ".join(f"{k}={v:.3g}" for k, v in seen.items()))
    assert max(seen.values()) > 1.0


@pytest.mark.parametrize("L", [8, 16, 31])
def test_onehot_rounds_hit_every_feature_once_per_post(L):
    for B, N in ij.SHAPES:
        hit = set()
        for rnd in range(ij.onehot_rounds(B, N, L)):
            for parity in ((0,) if N == 1 else (0, 1)):
                g, touched, feat, drive = ij.onehot_probe(B, N, L, rnd, parity)
                assert np.array_equal(g.sum(-1) == 1, drive) and np.all((g == 0) | (g == 1))
                per_post = np.zeros((B, N + 1), int)
                per_post[:, :-1] += drive
                per_post[:, 1:] += drive
                assert per_post.max() == 1 and np.array_equal(per_post == 1, touched)      # one contribution per touched fence post
                hit |= set(feat[drive].tolist())
        assert hit == set(range(6 * L)), (B, N, L)
