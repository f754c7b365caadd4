"""CPU: the fixture of the forward compositing checks (tests/composite_forward.py) checked on its own, before
test_gpu_composite_forward.py holds composite_ray to it on all three routes: the fp32 emulation of the kernel against the float64 truth
(the figures the budgets' constant is taken from), the truth against the numpy oracle, the budgets' power to see five wrong variants of
the kernel, and that no entry is left out of a comparison."""
import numpy as np
import pytest

import composite_forward as cf
from oracle import mipnerf_oracle as orc


def _case(cls, N):
    rs, t, d = cf.make(cls, cf.RAYS, N, np.random.default_rng(cf.case_seed(cls, N)))
    return rs, t, d, cf.Ray(rs, t, d)


def _cases():
    """(tag, N, rgb_sigma, t, dirs, Ray, facts or None) of every class and size and of the degenerate group"""
    for cls in cf.CLASSES:
        for N in cf.SIZES:
            yield (cls, N) + _case(cls, N) + (None,)
    for N in cf.DEGENERATE_SIZES:
        rs, t, d, facts = cf.make_degenerate(N)
        yield "degenerate", N, rs, t, d, cf.Ray(rs, t, d), facts


def _same(a, b):
    return np.array_equal(np.asarray(a, np.float32), np.asarray(b, np.float32))


def _exact_facts(got, t, white, facts, who):
    """the facts of the degenerate group that hold without a tolerance (the ones test_gpu_composite_forward.py asserts of the kernel)"""
    rgb, dist, acc, w = got
    e = facts["empty"]
    assert np.all(w[facts["zero_w"]] == 0), who
    assert np.all(w[e] == 0) and np.all(acc[e] == 0) and np.all(rgb[e] == (1.0 if white else 0.0)), who
    assert _same(dist[facts["at_near"]], t[facts["at_near"], 0]), who


def test_emulation_against_truth_gives_the_constant():
    """every class, size and white flag plus the degenerate group: the worst |emulation - truth| / budget at C = 1 per output are the
    figures next to C_BUDGET, and C_BUDGET is twice the worst of them"""
    worst = dict.fromkeys(cf.OUTPUTS, 0.0)
    per_tag = {}
    for tag, N, rs, t, d, ray, facts in _cases():
        for white in (0, 1):
            got = cf.emulate(rs, t, d, white)
            assert all(np.isfinite(g).all() for g in got) and np.all(got[3] >= 0), (tag, N, white)
            r = cf.ratios(got, cf.truth(ray, white, c_budget=1.0))
            mine = per_tag.setdefault(tag, dict.fromkeys(cf.OUTPUTS, 0.0))
            for k, v in r.items():
                worst[k] = max(worst[k], v)
                mine[k] = max(mine[k], v)
            if facts is not None:
                _exact_facts(got, t, white, facts, ("emulation", N, white))
    for tag, r in per_tag.items():
        print(f"composite_forward {tag}: worst emulation / budget at C = 1: " + " ".join(f"{k}={v:.2f}" for k, v in r.items()))
    print("composite_forward all cases: worst emulation / budget at C = 1: " + " ".join(f"{k}={v:.2f}" for k, v in worst.items()))
    assert 2.0 * max(worst.values()) <= cf.C_BUDGET <= 2.02 * max(worst.values())              # the rule: twice the worst, no more


def test_truth_against_the_oracle():
    """orc.volumetric_rendering (the reference's fp32 arithmetic in numpy, its own summation order) is within the shipped budget of the
    truth on every entry, and the exact facts of the degenerate group hold for it too"""
    worst = dict.fromkeys(cf.OUTPUTS, 0.0)
    for tag, N, rs, t, d, ray, facts in _cases():
        for white in (0, 1):
            got = orc.volumetric_rendering(rs[..., :3], rs[..., 3:], t, d, bool(white))
            r = cf.ratios(got, cf.truth(ray, white))
            assert max(r.values()) <= 1.0, (tag, N, white, r)
            worst = {k: max(worst[k], v) for k, v in r.items()}
            if facts is not None:
                _exact_facts(got, t, white, facts, ("oracle", N, white))
    print("composite_forward oracle / budget: " + " ".join(f"{k}={v:.3f}" for k, v in worst.items()))


@pytest.mark.parametrize("mutant", cf.MUTANTS)
def test_budget_sees_the_mutant(mutant):
    """each wrong variant of the kernel, as a switch on the emulation, exceeds ratio 1 at the shipped constant on at least one class and
    size for at least one output"""
    seen = []
    for tag, N, rs, t, d, ray, facts in _cases():
        for white in (0, 1):
            with np.errstate(all="ignore"):
                r = cf.ratios(cf.emulate(rs, t, d, white, mutant=mutant), cf.truth(ray, white))
            seen += [(v, tag, N, white, k) for k, v in r.items() if not v <= 1.0]
    assert seen, f"{mutant}: within budget everywhere"
    finite = [s for s in seen if np.isfinite(s[0])]
    v, tag, N, white, k = max(finite) if finite else seen[0]
    cases = sorted({(s[1], s[2]) for s in seen})
    print(f"composite_forward mutant {mutant}: over budget in {len(cases)} of {len(cf.CLASSES) * len(cf.SIZES) + len(cf.DEGENERATE_SIZES)} "
          f"cases; worst {v:.3g} x budget ({tag} N={N} white={white} {k}); first cases {cases[:6]}")


def test_no_hidden_exclusions():
    """the comparison covers every entry of every output, the degenerate group included; the group holds each kind on two rays of
    different workgroups with soft rays left over, its inputs are finite fp32, and its degenerate samples sit on both ends of lane 0's
    share, on the lane boundary and on the last sample"""
    for tag, N, rs, t, d, ray, facts in _cases():
        tr = cf.truth(ray, 1)
        mask = cf.compared(tr)
        assert sorted(mask) == sorted(cf.OUTPUTS)
        assert mask["weights"].shape == (cf.RAYS, N) and mask["rgb"].shape == (cf.RAYS, 3)
        assert mask["acc"].shape == mask["distance"].shape == (cf.RAYS,)
        assert all(m.dtype == bool and m.all() for m in mask.values())
        assert all(np.isfinite(tr[k]).all() and np.isfinite(tr["budget_" + k]).all() and np.all(tr["budget_" + k] > 0) for k in cf.OUTPUTS)
        if tag == "empty":
            assert np.all(tr["sum_dist"] < ray.t0)                       # the truth's sum lies below t_0: every empty ray is clamped
    assert [cf.scan_depth(N) for N in cf.SIZES] == [7, 7, 7, 8, 10, 14, 22, 22]
    rays = cf.degenerate_rays()
    used = sorted(b for v in rays.values() for b in v)
    assert len(used) == 2 * len(cf.DEGENERATE_KINDS) == len(set(used)) and len(used) < cf.RAYS
    assert all(a // 4 != b // 4 for a, b in rays.values())
    for N in cf.DEGENERATE_SIZES:
        K = cf.lane_bucket(N)
        assert set(cf.edge_samples(N)) == {0, K - 1, min(K, N - 1), N - 1}
        rs, t, d, facts = cf.make_degenerate(N)
        assert rs.dtype == t.dtype == d.dtype == np.float32
        for b in rays["zero_samples"]:
            assert np.flatnonzero(rs[b, :, 3] == 0).tolist() == cf.edge_samples(N)
        for b in rays["zero_width"]:
            assert set(cf.edge_samples(N)) <= set(np.flatnonzero(np.diff(t[b]) == 0).tolist())
        for b in rays["flat"]:
            assert np.all(t[b] == t[b, 0])
        for b in rays["zero_dir"]:
            assert np.all(d[b] == 0)
        for b in rays["opaque_last"]:
            assert rs[b, N - 1, 3] == np.float32(1e6)
        for b in rays["zero_ray"]:
            assert np.all(rs[b, :, 3] == 0)
        soft = [b for b in range(cf.RAYS) if b not in used]
        assert np.all(rs[soft][..., 3] > 0) and np.all(np.diff(t[soft], axis=-1) > 0)
