"""CPU: the fixture of the distortion loss (tests/distloss_fixture.py) checked on its own, before test_gpu_distloss.py holds
distloss_ray to it: the O(N^2) truth against float64 autograd, the property that names each class, the rule at tied midpoints, the fp32
emulation of the kernel against the shipped budgets (the worst ratios at C = 1 are the figures next to the constants), and the budgets'
power to see a wrong kernel."""
import numpy as np
import pytest
import torch

import distloss_fixture as dl
from test_gpu_resample_grad import t_distloss_rays


def _case(cls, N):
    return dl.make(cls, dl.RAYS, N, np.random.default_rng(dl.case_seed(cls, N)))


def _autograd(w, t, g, restated):
    """value, d_w, d_t by float64 autograd.  restated: the chain of t_distloss_rays shifted by constants so that the midpoints and
    intervals are the fp32 ones of the truth; otherwise t_distloss_rays itself"""
    w8, t8 = torch.from_numpy(w).double().requires_grad_(True), torch.from_numpy(t).double().requires_grad_(True)
    if restated:
        m32, iv32 = (torch.from_numpy(a).double() for a in dl.mid_interval(t))
        iv, m = t8[:, 1:] - t8[:, :-1], 0.5 * (t8[:, 1:] + t8[:, :-1])
        iv, m = iv + (iv32 - iv).detach(), m + (m32 - m).detach()
        val = (iv * w8 * w8).sum(-1) / 3.0 + (w8[:, :, None] * w8[:, None, :] * (m[:, :, None] - m[:, None, :]).abs()).sum((-1, -2))
    else:
        val = t_distloss_rays(w8, t8)
    (val * torch.from_numpy(g).double()).sum().backward()
    return val.detach().numpy(), w8.grad.numpy(), t8.grad.numpy()


@pytest.mark.parametrize("N", [1, 5, 65, 300])
@pytest.mark.parametrize("cls", dl.CLASSES)
def test_truth_matches_float64_autograd(cls, N):
    """1e-10 of each entry's sum of absolute terms (the budget's own magnitude over C u); tied midpoints included: sign(0) = 0 in both"""
    w, t, g, _ = _case(cls, N)
    tr = dl.truth(w, t, g, c=(1.0, 1.0, 1.0))
    val, d_w, d_t = _autograd(w, t, g, restated=True)
    scale = 1e-10 / dl.U
    assert np.all(np.abs(val - tr["value"]) <= scale * tr["budget_value"])
    assert np.all(np.abs(d_w - tr["d_w"]) <= scale * tr["budget_w"])
    assert np.all(np.abs(d_t - tr["d_t"]) <= scale * tr["budget_t"])


def test_truth_matches_t_distloss_rays_on_a_dyadic_grid():
    """fence posts on multiples of 2^-12 in [2, 6]: midpoints and intervals are exact in fp32, so t_distloss_rays' own float64 autograd
    is the truth to 1e-10"""
    rng = np.random.default_rng(5)
    B, N = dl.RAYS, 129
    w, _, g, _ = dl.make("soft", B, N, rng)
    t = np.stack([np.sort(rng.choice(np.arange(2 << 12, 6 << 12), N + 1, replace=False)) for _ in range(B)]).astype(np.float32) / 4096
    m, iv = dl.mid_interval(t)
    assert np.array_equal(m.astype(np.float64), 0.5 * (t[:, 1:].astype(np.float64) + t[:, :-1])) and not dl.tied(t).any()
    tr = dl.truth(w, t, g, c=(1.0, 1.0, 1.0))
    val, d_w, d_t = _autograd(w, t, g, restated=False)
    scale = 1e-10 / dl.U
    assert np.all(np.abs(val - tr["value"]) <= scale * tr["budget_value"])
    assert np.all(np.abs(d_w - tr["d_w"]) <= scale * tr["budget_w"]) and np.all(np.abs(d_t - tr["d_t"]) <= scale * tr["budget_t"])


@pytest.mark.parametrize("cls", dl.CLASSES)
def test_class_properties(cls):
    for N in dl.SIZES:
        w, t, g, info = _case(cls, N)
        B = dl.RAYS
        assert w.shape == (B, N) and t.shape == (B, N + 1) and g.shape == (B,)
        assert np.all(w.astype(np.float64).sum(-1) <= 1.0 + 1e-6)                      # weights a compositing can make
        assert np.any(g == 0) and np.any(g < 0) and np.abs(g).max() >= 1e3
        m, iv = dl.mid_interval(t)
        td, checked = dl.tied(t), dl.checked_posts(t)
        tr = dl.truth(w, t, g)
        if cls == "coincident" and N >= 5:
            j = info["j"]
            for b in range(B):
                assert t[b, j[b]] == t[b, j[b] + 1] == t[b, j[b] + 2] and np.array_equal(np.nonzero(td[b])[0], [j[b], j[b] + 1])
                assert np.all(w[b, j[b]:j[b] + 2] > 0)                                  # the tie carries weight: the rules do differ
            assert np.all((~checked).sum(-1) == 3) and 3 <= dl.MAX_UNCHECKED
        else:
            assert not td.any() and checked.all() and np.all(np.diff(m, axis=-1) > 0)   # no tie: nothing is left out
        if cls == "empty":
            assert np.all(w == 0) and np.all(tr["value"] == 0) and np.all(tr["d_w"] == 0) and np.all(tr["d_t"] == 0)
        if cls == "onehot":
            k = info["k"]
            rows = np.arange(B)
            assert np.all(w.sum(-1) == 1) and np.all(w[rows, k] == 1)
            assert np.array_equal(tr["value"], iv[rows, k].astype(np.float64) / 3.0)
            others = np.ones((B, N), bool)
            others[rows, k] = False
            want = 2.0 * g.astype(np.float64)[:, None] * np.abs(m.astype(np.float64) - m[rows, k].astype(np.float64)[:, None])
            assert np.allclose(tr["d_w"][others], want[others], rtol=1e-14, atol=0)
            assert np.all(tr["d_w"][others & (g != 0)[:, None]] != 0)
            if N >= 129:
                assert {63, 64} <= set(k.tolist())
        if cls == "surface" and N >= 64:
            assert np.median((w > 1e-3).sum(-1)) <= 6 and np.any(w == 0) and np.median(w.sum(-1)) > 0.5
        if cls == "farfield":
            assert t.min() >= 1e2 and t.max() <= 1e3
            ulps = np.diff(t.view(np.int32).astype(np.int64), axis=-1)
            assert ulps.min() >= 2 and (N < 64 or ulps.min() <= 4) and ulps.max() < 1 << 14


@pytest.mark.parametrize("cls", dl.CLASSES)
def test_emulation_meets_the_shipped_budgets(cls):
    """value, every d_w entry and every checked d_t entry at every N; prints the worst ratios at C = 1"""
    worst1 = dict(value=0.0, d_w=0.0, d_t=0.0)
    for N in dl.SIZES:
        w, t, g, _ = _case(cls, N)
        value, d_w, d_t = dl.emulate(w, t, g)
        checked = dl.checked_posts(t)
        r = dl.ratios(dl.truth(w, t, g), value, d_w, d_t, checked)
        assert max(r.values()) <= 1.0, (cls, N, r)
        for k, v in dl.ratios(dl.truth(w, t, g, c=(1.0, 1.0, 1.0)), value, d_w, d_t, checked).items():
            worst1[k] = max(worst1[k], v)
        if cls == "empty":
            assert np.all(value == 0) and np.all(d_w == 0) and np.all(d_t == 0)
    print(f"distloss emulation {cls}: worst / budget at C = 1: " + " ".join(f"{k}={v:.2f}" for k, v in worst1.items()))
    assert worst1["value"] <= dl.C_VALUE / 2 and worst1["d_w"] <= dl.C_DW / 2 and worst1["d_t"] <= dl.C_DT / 2


def test_index_order_at_a_tie_is_outside_the_budget_only_at_the_tied_posts():
    """the O(N) form orders tied midpoints by index: on `coincident` it differs from the truth (sign(0) = 0) by more than 10 budgets
    at the posts left out, and nowhere else"""
    for N in (5, 65, 1024):
        w, t, g, _ = _case("coincident", N)
        tr = dl.truth(w, t, g)
        _, _, d_t = dl.emulate(w, t, g)
        r = np.abs(d_t.astype(np.float64) - tr["d_t"]) / np.maximum(tr["budget_t"], 1e-300)
        checked = dl.checked_posts(t)
        live = (g != 0)
        assert np.all(r[checked] <= 1.0) and np.all(r[~checked].reshape(dl.RAYS, 3)[live].max(-1) > 10.0)


@pytest.mark.parametrize("mutation", ["fp32_scan", "no_self", "sign"])
def test_budget_sees_the_mutation(mutation):
    seen = {}
    for cls in dl.CLASSES:
        worst = 0.0
        for N in (5, 300, 1024):
            w, t, g, _ = _case(cls, N)
            worst = max(worst, *dl.ratios(dl.truth(w, t, g), *dl.emulate(w, t, g, mutation=mutation), dl.checked_posts(t)).values())
        seen[cls] = worst
    print(f"distloss mutation {mutation}: " + " ".join(f"{k}={v:.3g}" for k, v in seen.items()))
    assert max(seen.values()) > 1.0 and seen["empty"] == 0.0
