"""GPU: the forward compositing (composite_ray of csrc/raywave.hpp) entry by entry against float64 on all three of its routes --
mipnerf_volumetric_rendering (k_volumetric_rendering), mipnerf_composite_resample (k_composite_resample, every inference forward) and
mipnerf_composite_train (k_composite_train, every training step) -- on empty, soft, opaque, surface and saturated rays and on a group of
degenerate ones (zero density, zero-width intervals, equal fence posts, a zero direction, one sample of density 1e6).

tests/composite_forward.py has the float64 truth from the kernel's own fp32 operands and the running-error budget of every entry;
tests/test_composite_forward_cpu.py checks that fixture without a GPU.  Nothing here is normalised by a batch's largest value and no entry
is left out: the budget is the only slack, and the facts that hold exactly are asserted without one.  The fused routes must give the
bits of the stand-alone entry points (the compositing outputs, the resampled fence posts, the distortion loss and its gradient), at
B = 18 (4 rays per workgroup: a ragged last one), on the first ray alone (B = 1: three waves of the workgroup shadow it and must store
nothing) and with the rays permuted (the LDS rows are per wave).  Every output buffer is a workgroup's worth of rows longer than needed
and NaN-filled: the tail stays NaN.  N over every lane bucket K = 1, 2, 4, 8, 16 at its first size, two ragged K = 1 sizes and the full
last lane (1024); a case is a few dozen launches of at most 18 x 1024 samples."""
import numpy as np
import pytest
import torch

import composite_forward as cf

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PADDING = 0.01
SPARE = 4                                  # rays of a workgroup
G_CONST = float(np.float32(0.01 / cf.RAYS))


@pytest.fixture(scope="module")
def G():
    import gpu_util
    assert torch.cuda.is_available()
    return gpu_util


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _nan(B, *shape):
    return torch.full((B + SPARE,) + shape, float("nan"), device=DEV)


def _bits(x):
    return x.contiguous().view(torch.int32)


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _finish(B, outs, who):
    """the canary rows of every buffer are still NaN; returns the first B rows"""
    for k, v in outs.items():
        assert bool(torch.isnan(v[B:]).all()), (who, k, "rows past B were written")
    return {k: v[:B] for k, v in outs.items()}


def _composite_bufs(B, N):
    return dict(rgb=_nan(B, 3), distance=_nan(B), acc=_nan(B), weights=_nan(B, N))


def _ptrs(bufs, *names):
    return [bufs[n].data_ptr() for n in names]


def _standalone(rs, t, d, white, u):
    """mipnerf_volumetric_rendering, then mipnerf_resample_along_rays (u = None and u) and mipnerf_distloss (g_ray filled with G_CONST)
    on its weights"""
    from mipnerf_pl_amd import _lib as L
    from mipnerf_pl_amd import ops
    lib, st = L.lib(), ops._stream()
    B, N = rs.shape[:2]
    o = _composite_bufs(B, N)
    L.check(lib.mipnerf_volumetric_rendering(B, N, rs.data_ptr(), t.data_ptr(), d.data_ptr(), white,
                                             *_ptrs(o, "rgb", "distance", "acc", "weights"), st), "volumetric_rendering")
    o.update(t_new=_nan(B, N + 1), t_new_u=_nan(B, N + 1), ray_loss=_nan(B), d_w=_nan(B, N))
    w = o["weights"]
    L.check(lib.mipnerf_resample_along_rays(B, N, t.data_ptr(), w.data_ptr(), None, PADDING, o["t_new"].data_ptr(), st), "resample")
    L.check(lib.mipnerf_resample_along_rays(B, N, t.data_ptr(), w.data_ptr(), u.data_ptr(), PADDING, o["t_new_u"].data_ptr(), st), "resample")
    g = torch.full((B,), G_CONST, device=DEV)
    L.check(lib.mipnerf_distloss(B, N, w.data_ptr(), t.data_ptr(), o["ray_loss"].data_ptr(), g.data_ptr(), o["d_w"].data_ptr(), st),
            "distloss")
    return _finish(B, o, "stand-alone")


def _fused_resample(rs, t, d, white, u):
    from mipnerf_pl_amd import _lib as L
    from mipnerf_pl_amd import ops
    B, N = rs.shape[:2]
    o = _composite_bufs(B, N)
    o["t_new"] = _nan(B, N + 1)
    L.check(L.lib().mipnerf_composite_resample(B, N, rs.data_ptr(), t.data_ptr(), d.data_ptr(), white,
                                               *_ptrs(o, "rgb", "distance", "acc", "weights"), t.data_ptr(),
                                               None if u is None else u.data_ptr(), PADDING, o["t_new"].data_ptr(), ops._stream()),
            "composite_resample")
    return _finish(B, o, "composite_resample")


def _fused_train(rs, t, d, white, u, last_level=False, bins=True):
    from mipnerf_pl_amd import _lib as L
    from mipnerf_pl_amd import ops
    B, N = rs.shape[:2]
    o = _composite_bufs(B, N)
    o.update(ray_loss=_nan(B), d_w=_nan(B, N))
    if not last_level:
        o["t_new"] = _nan(B, N + 1)
    L.check(L.lib().mipnerf_composite_train(B, N, rs.data_ptr(), t.data_ptr(), d.data_ptr(), white,
                                            *_ptrs(o, "rgb", "distance", "acc", "weights", "ray_loss"), G_CONST, o["d_w"].data_ptr(),
                                            None if u is None else u.data_ptr(), PADDING, None if last_level else o["t_new"].data_ptr(),
                                            t.data_ptr() if bins else None, ops._stream()), "composite_train")
    return _finish(B, o, "composite_train")


COMPOSITE = ("rgb", "distance", "acc", "weights")


def _routes(rs, t, d, white, u, who):
    """every route on one batch; asserts that the fused routes give the stand-alone bits; returns the stand-alone outputs"""
    ref = _standalone(rs, t, d, white, u)
    for uu, tn in ((None, "t_new"), (u, "t_new_u")):
        fr = _fused_resample(rs, t, d, white, uu)
        ft = _fused_train(rs, t, d, white, uu)
        for k in COMPOSITE:
            assert _same(fr[k], ref[k]), (who, "composite_resample", uu is not None, k)
            assert _same(ft[k], ref[k]), (who, "composite_train", uu is not None, k)
        assert _same(fr["t_new"], ref[tn]) and _same(ft["t_new"], ref[tn]), (who, tn)
        assert _same(ft["ray_loss"], ref["ray_loss"]) and _same(ft["d_w"], ref["d_w"]), (who, "distloss", uu is not None)
    for ft in (_fused_train(rs, t, d, white, None, last_level=True), _fused_train(rs, t, d, white, u, bins=False)):
        for k in COMPOSITE + ("ray_loss", "d_w"):
            assert _same(ft[k], ref[k]), (who, "composite_train, last level / bins = NULL", k)
        assert "t_new" not in ft or _same(ft["t_new"], ref["t_new_u"]), (who, "bins = NULL")
    return ref


def _check_case(G, tag, N, rs, t, d, facts):
    B = cf.RAYS
    ray = cf.Ray(rs, t, d)
    rng = np.random.default_rng(N + 31)
    u = rng.random((B, N + 1), dtype=np.float32)
    perm = rng.permutation(B)
    rs_d, t_d, d_d, u_d, perm_d = T(rs), T(t), T(d), T(u), T(perm)
    worst, fails = {}, []
    for white in (0, 1):
        who = (tag, N, white)
        tr = cf.truth(ray, white)
        ref = _routes(rs_d, t_d, d_d, white, u_d, who)
        # the first ray alone: three shadow waves; row 0 of the batch bit for bit on every route
        one = _routes(rs_d[:1], t_d[:1], d_d[:1], white, u_d[:1], who + ("B=1",))
        for k, v in one.items():
            assert _same(v, ref[k][:1]), (who, "B=1", k)
        # the rays permuted: each ray's outputs keep their bits on all three routes
        mixed = _routes(rs_d[perm_d].contiguous(), t_d[perm_d].contiguous(), d_d[perm_d].contiguous(), white, u_d[perm_d].contiguous(),
                        who + ("permuted",))
        for k, v in mixed.items():
            assert _same(v, ref[k][perm_d]), (who, "permuted", k)
        # per entry against float64
        got = tuple(ref[k].cpu().numpy() for k in COMPOSITE)
        rgb, dist, acc, w = got
        assert all(np.isfinite(g).all() for g in got), who
        assert np.all(w >= 0), who
        r = cf.ratios(got, tr)
        print(f"composite_forward {tag} N={N} white={white}: worst got/budget " + " ".join(f"{k}={v:.3g}" for k, v in r.items()))
        for k, v in r.items():
            worst[f"{k}{'_white' if white else ''}"] = v
            if not v <= 1.0:
                fails.append((white, k, v))
        # exact facts
        if tag == "empty":
            assert np.all(tr["sum_dist"] < ray.t0)
            assert np.array_equal(dist, t[:, 0]), who
        if facts is not None:
            e = facts["empty"]
            assert np.all(w[facts["zero_w"]] == 0), who
            assert np.all(w[e] == 0) and np.all(acc[e] == 0) and np.all(rgb[e] == (1.0 if white else 0.0)), who
            assert np.array_equal(dist[facts["at_near"]], t[facts["at_near"], 0]), who
    G.record(f"composite_forward {tag} N={N}", **worst)
    assert not fails, fails


@pytest.mark.parametrize("N", cf.SIZES)
@pytest.mark.parametrize("cls", cf.CLASSES)
def test_every_forward_entry_within_its_budget_on_every_route(G, cls, N):
    rs, t, d = cf.make(cls, cf.RAYS, N, np.random.default_rng(cf.case_seed(cls, N)))
    _check_case(G, cls, N, rs, t, d, None)


@pytest.mark.parametrize("N", cf.DEGENERATE_SIZES)
def test_degenerate_rays_on_every_route(G, N):
    rs, t, d, facts = cf.make_degenerate(N)
    _check_case(G, "degenerate", N, rs, t, d, facts)
