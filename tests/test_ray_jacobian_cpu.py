"""CPU: the fixture of the compositing backward's Jacobian probes (tests/ray_jacobian.py) checked on its own, before
test_gpu_ray_jacobian.py holds k_volumetric_rendering_bwd to it: the closed-form truth against float64 autograd, the shipped budgets
against the fp32 emulation of the kernel, the budgets' power to see the cancelling density factor this kernel used to have, and the
conditions on the inputs."""
import numpy as np
import pytest
import torch

import ray_jacobian as rj
from test_gpu_train import torch_volumetric_rendering


def _case(cls, N):
    rng = np.random.default_rng(rj.case_seed(cls, N))
    rs, t, d = rj.make(cls, rj.RAYS, N, rng)
    return rs, t, d, rj.Ray(rs, t, d), rj.probes(rj.RAYS, N, rng)


def _autograd(rs, t, d, white, g, stable_alpha):
    """float64 autograd of sum(outputs * upstream) w.r.t. the pre-activations that give exactly the fp32 operands, and w.r.t. t.
    stable_alpha: alpha = -expm1(-x) in place of the restatement's 1 - exp(-x)"""
    f8 = torch.float64
    p = float(rj.PAD)
    c, sigma = torch.from_numpy(rs[..., :3]).to(f8), torch.from_numpy(rs[..., 3:]).to(f8)
    s = (c + p) / (1.0 + 2.0 * p)
    raw_c = (torch.log(s) - torch.log1p(-s)).requires_grad_(True)                 # logit
    raw_d = (sigma + torch.log(-torch.expm1(-sigma))).requires_grad_(True)        # softplus^-1
    rgb = torch.sigmoid(raw_c) * (1.0 + 2.0 * p) - p
    den = -torch.nn.functional.logsigmoid(-raw_d)                                 # softplus, with sigmoid as its derivative everywhere
    assert float((den.detach() - sigma).abs().div(sigma).max()) < 1e-13 and float((rgb.detach() - c).abs().max()) < 1e-15
    tt = torch.from_numpy(t).to(f8).requires_grad_(True)
    dirs = torch.from_numpy(d).to(f8)
    if stable_alpha:
        tm = 0.5 * (tt[:, :-1] + tt[:, 1:])
        x = den[..., 0] * (tt[:, 1:] - tt[:, :-1]) * torch.linalg.norm(dirs, dim=-1, keepdim=True)
        cum = torch.cat([torch.zeros_like(x[:, :1]), torch.cumsum(x[:, :-1], -1)], -1)
        # (torch differentiates expm1 as result + 1, which is 0 once e^-x < 2^-53: 1 - exp above x = 1, where nothing cancels)
        w = torch.where(x < 1.0, -torch.expm1(-x), 1.0 - torch.exp(-x)) * torch.exp(-cum)
        acc = w.sum(-1)
        comp = (w[..., None] * rgb).sum(-2) + ((1.0 - acc[:, None]) if white else 0.0)
        out = comp, torch.clamp((w * tm).sum(-1), tt[:, 0], tt[:, -1]), acc, w
    else:
        out = torch_volumetric_rendering(rgb, den, tt, dirs, bool(white))
    loss = 0.0
    for o, k in zip(out, ("g_rgb", "g_dist", "g_acc", "g_w")):
        if g[k] is not None:
            loss = loss + (o * torch.from_numpy(g[k]).to(f8)).sum()
    loss.backward()
    grads = [torch.zeros_like(v) if v.grad is None else v.grad for v in (raw_c, raw_d, tt)]       # None: not reached by this probe
    return torch.cat(grads[:2], -1).numpy(), grads[2].numpy()


@pytest.mark.parametrize("N", [5, 65])
@pytest.mark.parametrize("cls", rj.CLASSES)
def test_closed_forms_match_float64_autograd(cls, N):
    """1e-10 relative.  Against test_gpu_train's restatement per ray and kind of entry, relative to the ray's largest: its
    alpha = 1 - exp(-x) cancels in double too (x down to 1e-15 on empty samples), and its autograd carries that alpha into every
    sample in front.  Against the same graph with alpha = -expm1(-x), per entry: 1e-10 of the entry, plus float64's own rounding of
    the terms that cancel in dx_i (1e-12 of their absolute sum; in the per-ray comparison the ray's largest such sum: with g_acc on an
    opaque ray every dx_i cancels to ~0).  The colour entries in both comparisons also get float64's rounding
    of 1 - s in the sigmoid's derivative (4 x 2^-53 / min(s, 1 - s) of the entry) and, against the restatement, of its alpha (2^-53
    absolute, times the upstream gradient).  1e-300 absolute: a subnormal double has no relative precision."""
    rs, t, d, ray, probes = _case(cls, N)
    for name, white, g in probes:
        tr = rj.truth(ray, white, **g)
        want = tr["d_raw"]
        round_c = np.abs(want[..., :3]) * 4 * 2.0 ** -53 / np.minimum(ray.s, 1 - ray.s)
        gmax = 0.0 if g["g_rgb"] is None else float(np.abs(g["g_rgb"]).max())
        d_raw, d_t = _autograd(rs, t, d, white, g, stable_alpha=False)
        for got, ref, extra in ((d_raw[..., :3], want[..., :3], round_c.reshape(rj.RAYS, -1).max(-1) + 2.0 ** -53 * gmax),
                                (d_raw[..., 3], want[..., 3], 1e-12 * tr["absterms"].max(-1)),
                                (d_t, tr["d_t"], 1e-12 * tr["absterms_t"].max(-1))):
            got, ref = got.reshape(rj.RAYS, -1), ref.reshape(rj.RAYS, -1)
            scale = np.abs(ref).max(-1)
            err = np.abs(got - ref).max(-1)
            assert np.all(err <= 1e-10 * scale + extra), (cls, N, name, white, float((err / np.maximum(scale, 1e-300)).max()))
        d_raw, d_t = _autograd(rs, t, d, white, g, stable_alpha=True)
        tol_w = 1e-10 * np.abs(want[..., 3]) + 1e-12 * tr["absterms"] + 1e-300
        assert np.all(np.abs(d_raw[..., 3] - want[..., 3]) <= tol_w), (cls, N, name, white)
        assert np.all(np.abs(d_raw[..., :3] - want[..., :3]) <= 1e-10 * np.abs(want[..., :3]) + round_c + 1e-300), (cls, N, name, white)


@pytest.mark.parametrize("cls", rj.CLASSES)
def test_emulation_with_expm1_meets_the_shipped_budgets(cls):
    """every entry of every probe at every size, d_t included; the worst ratios at C = 1 are the figures next to C_BUDGET"""
    worst1 = dict(w=0.0, c=0.0, t=0.0)
    for N in rj.SIZES:
        rs, t, d, ray, probes = _case(cls, N)
        for name, white, g in probes:
            d_raw, d_t = rj.emulate(rs, t, d, white, **g)
            r = rj.ratios(d_raw, d_t, rj.truth(ray, white, **g))
            assert max(r.values()) <= 1.0, (cls, N, name, white, r)
            for k, v in r.items():
                worst1[k] = max(worst1[k], v * rj.C_BUDGET)
            # the exact structure the GPU test asserts holds in the emulation as well
            if name == "onehot":
                idx = rj.onehot_indices(rj.RAYS, N)
                assert np.all(d_raw[..., :3] == 0) and np.all(d_raw[..., 3][np.arange(N)[None, :] > idx[:, None]] == 0)
            if name == "dist":
                assert np.all(d_raw[~ray.inside] == 0)
    print(f"{cls}: worst emulation / budget at C = 1: " + " ".join(f"{k}={v:.2f}" for k, v in worst1.items()))


@pytest.mark.parametrize("cls", ["empty", "opaque", "surface"])
def test_budget_sees_the_cancelling_density_factor(cls):
    """d softplus as 1 - expf(-sigma) -- what the kernel computed before density_activation_grad -- exceeds budget_w by at least 1e3 x
    under the one-hot and the colour probe (white off) wherever the class has empty samples: every N of `empty`; N >= 5 of `opaque` and
    `surface`, whose only sample at N = 1 is the surface itself"""
    for N in rj.SIZES:
        if N == 1 and cls != "empty":
            continue
        rs, t, d, ray, probes = _case(cls, N)
        for name, white, g in probes:
            if (name, white) not in (("onehot", 0), ("rgb", 0)):
                continue
            r = rj.ratios(*rj.emulate(rs, t, d, white, cancelling_factor=True, **g), rj.truth(ray, white, **g))
            print(f"{cls} N={N} {name}: 1 - expf(-sigma) misses budget_w by {r['w']:.3g} x")
            assert r["w"] >= 1e3, (cls, N, name, r)
            assert r["c"] <= 1.0                 # the colour entries do not use the factor


def test_from_raw_case_in_emulation():
    """the one-sample case from the raw density on: the emulation with expm1f is within the bound and has no dead entry; with
    1 - expf(-sigma) a quarter of the grid (raw - 1 < -16.6) is dead"""
    raw, t, d, want = rj.from_raw_case()
    rs = np.concatenate([rj.rgb_activation32(raw[..., :3]), rj.softplus32(raw[..., 3:] + np.float32(rj.FROM_RAW_BIAS))], -1)
    rj.check_inputs(rs, t, d)
    g = dict(g_acc=np.ones(raw.shape[0], np.float32))
    got = rj.emulate(rs, t, d, 0, **g)[0][:, 0, 3].astype(np.float64)
    rel = np.abs(got - want) / want
    print(f"from raw, emulation: worst relative error {rel.max() * 2.0 ** 24:.2f} x 2^-24")
    assert np.all(got != 0) and rel.max() <= rj.FROM_RAW_BOUND / 2          # half: the device's libm may differ by an ulp or two
    dead = rj.emulate(rs, t, d, 0, cancelling_factor=True, **g)[0][:, 0, 3] == 0
    assert dead.sum() >= raw.shape[0] // 5 and np.all(raw[dead, 0, 3] + rj.FROM_RAW_BIAS < -16.0)


@pytest.mark.parametrize("cls", rj.CLASSES)
def test_fixture_input_conditions(cls):
    for N in rj.SIZES:
        rs, t, d, ray, probes = _case(cls, N)
        rj.check_inputs(rs, t, d)                                            # sorted t, finite operands, |d|, colours inside (0, 1)
        assert rs.shape == (rj.RAYS, N, 4) and t.shape == (rj.RAYS, N + 1) and d.shape == (rj.RAYS, 3)
        assert ray.clamp_margin() > rj.CLAMP_MARGIN
        assert not ray.above.any()
        if cls == "empty":
            assert ray.below.all()                                           # sum w tmid < t_0: every empty ray is clamped
        if cls == "opaque" and N >= 64:
            assert np.any(ray.T[:, -1] < 2.0 ** -149)                        # the fp32 transmittance underflows to 0
        for name, white, g in probes:
            for v in g.values():
                assert v is None or (v.dtype == np.float32 and np.isfinite(v).all())
        idx = rj.onehot_indices(rj.RAYS, N)
        K = rj.lane_bucket(N)
        assert set(idx.tolist()) == {min(max(i, 0), N - 1) for i in (0, K - 1, K, N // 2, N - 1)}
    assert [rj.lane_bucket(N) for N in rj.SIZES] == [1, 1, 1, 2, 4, 8, 16]
