"""GPU: the inverse-CDF sampler (pdf_ray behind mipnerf_resample_along_rays and mipnerf_sorted_piecewise_constant_pdf) draw by draw, and
its backward (k_resample_bwd behind mipnerf_resample_along_rays_bwd) entry by entry, against float64.

tests/sampler_fixture.py has the weight classes, bins and draws, the float64 truth from the kernels' own fp32 operands, the fragile draws
and the running-error budget of every draw and every d_weights entry; tests/test_sampler_cpu.py checks that fixture without a GPU.
Nothing here is normalised by a batch's or a ray's largest value, and no draw or entry is left out except as the fixture's docstring
states (a fragile draw next to a bin of mass < 1e-5, forward only): the budget is the only slack.  B = 18 rays (4 per workgroup of the
forward: a ragged last one), N over every lane bucket; every launch is at most 18 x 1089 values.  The fused routes (k_composite_resample,
k_composite_train, the unbounded-scene route) are held to these kernels' bytes by test_gpu_stages / test_gpu_train / test_gpu_unbounded;
the decreasing bins here are that last route's inverse depths."""
import numpy as np
import pytest
import torch

import sampler_fixture as sf

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
D = np.float64


@pytest.fixture(scope="module")
def G():
    import gpu_util
    assert torch.cuda.is_available()
    return gpu_util


def T(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _forward(c, blur, padding, n_draws):
    """t' [B, n_draws] through the ops entry points; the weights tensor must come back with the bits it went in with"""
    from mipnerf_pl_amd import ops
    bins, w, r = T(c["bins"]), T(c["w"]), T(c["r"])
    if blur:
        t = ops.resample_t(bins, w, r is not None, padding, r)
    else:
        t = ops.sorted_piecewise_constant_pdf(bins, w, n_draws, r is not None, r)
    assert np.array_equal(_bits(w.cpu().numpy()), _bits(c["w"])) and np.array_equal(_bits(bins.cpu().numpy()), _bits(c["bins"]))
    t = t.cpu().numpy()
    assert t.shape == (c["w"].shape[0], n_draws) and t.dtype == np.float32
    return t


def _structure(t, c, decreasing=False):
    assert np.isfinite(t).all()
    d = np.diff(t, axis=-1)
    assert np.all(d <= 0) if decreasing else np.all(d >= 0)
    assert np.all(t >= c["bins"].min(-1, keepdims=True)) and np.all(t <= c["bins"].max(-1, keepdims=True))


@pytest.mark.parametrize("cls,N", [(cls, N) for cls in sf.BLUR_CLASSES for N in sf.sizes_of(cls)])
def test_every_resampled_t_within_its_budget(G, cls, N):
    """mipnerf_resample_along_rays: deterministic and randomized draws, increasing fence posts and decreasing inverse depths"""
    worst, differ, fails = {}, 0, []
    for padding in sf.paddings_of(cls):
        for rnd, dec in ((False, False), (True, False), (False, True)):
            c = sf.blur_case(cls, N, padding, rnd, dec)
            tr = sf.forward_truth(c["bins"], c["w"], c["u"], True, padding)
            assert not tr["left_out"].any()
            t = _forward(c, True, padding, N + 1)
            _structure(t, c, dec)
            if cls == "uniform_ties" and rnd and N >= 2:          # a draw on a cdf entry belongs to the interval above it: its lower edge
                assert np.array_equal(_bits(t[:, 1:N]), _bits(c["bins"][:, 1:N]))
            differ += int((_bits(t) != _bits(sf.emulate_forward(c["bins"], c["w"], c["u"], True, padding)["t"])).sum())
            r = sf.forward_ratio(t, tr)
            tag = f"pad{padding}_{'rand' if rnd else 'det'}{'_dec' if dec else ''}"
            print(f"sampler forward blur {cls} N={N} {tag}: worst got/budget {r:.3g}")
            worst[tag] = r
            if not r <= 1.0:
                fails.append((tag, r))
    G.record(f"sampler forward blur {cls} N={N}", differ_from_emulation=differ, **worst)
    assert not fails, fails


@pytest.mark.parametrize("cls,N", [(cls, N) for cls in sf.NOBLUR_CLASSES for N in sf.NOBLUR_SIZES])
def test_every_piecewise_constant_draw_within_its_budget(G, cls, N):
    """mipnerf_sorted_piecewise_constant_pdf with num_draws of 1, 2, N + 1, a full trip of the search and one draw into the next"""
    worst, differ, left_out, fails = {}, 0, 0, []
    for n in sf.noblur_draw_counts(N):
        for rnd in (False, True):
            c = sf.noblur_case(cls, N, n, rnd)
            tr = sf.forward_truth(c["bins"], c["w"], c["u"], False, 0.0)
            t = _forward(c, False, 0.0, n)
            _structure(t, c)
            if not rnd:
                # u = 0 behind leading zero-weight bins: the lower edge of the first bin with mass, to the bit
                lead = (np.cumsum(c["w"], -1) == 0).sum(-1)
                first = np.take_along_axis(c["bins"], np.minimum(lead, N - 1)[:, None], -1)[:, 0]
                assert np.array_equal(_bits(t[:, 0]), _bits(np.where(lead < N, first, c["bins"][:, 0])))
                if cls in ("onehot", "surface", "sliver") and N >= 64:
                    assert (lead > 0).sum() >= sf.RAYS // 2
            # a draw inside a bin of mass < 1e-5 (den -> 1) stays in the first 1e-5 of the bin
            mass = np.take_along_axis(tr["pdf"], tr["bin"], -1)
            inside = (mass > 0) & (mass < 1e-5) & ~tr["fragile"]
            b0 = np.take_along_axis(c["bins"], tr["bin"], -1).astype(D)
            b1 = np.take_along_axis(c["bins"], tr["bin"] + 1, -1).astype(D)
            assert np.all(((t >= b0) & (t <= b0 + 1e-5 * (b1 - b0)))[inside])
            if cls == "sliver" and not rnd and n >= 3:
                assert inside.any(-1).all()
            differ += int((_bits(t) != _bits(sf.emulate_forward(c["bins"], c["w"], c["u"], False, 0.0)["t"])).sum())
            left_out += int(tr["left_out"].sum())
            r = sf.forward_ratio(t, tr)
            tag = f"n{n}_{'rand' if rnd else 'det'}"
            print(f"sampler forward no-blur {cls} N={N} {tag}: worst got/budget {r:.3g}")
            worst[tag] = r
            if not r <= 1.0:
                fails.append((tag, r))
    G.record(f"sampler forward noblur {cls} N={N}", differ_from_emulation=differ, left_out=left_out, **worst)
    assert not fails, fails


def _backward(bins, w, r, padding, g, fill=float("nan")):
    """d_weights [B, N] of one probe through the C entry point, as autograd._ResampleT.backward calls it"""
    from mipnerf_pl_amd import _lib as L
    from mipnerf_pl_amd import ops
    B, N = w.shape
    g = T(g)
    d_w = torch.full((B, N), fill, device=DEV, dtype=torch.float32)
    L.check(L.lib().mipnerf_resample_along_rays_bwd(B, N, bins.data_ptr(), w.data_ptr(), None if r is None else r.data_ptr(), float(padding),
                                                    g.data_ptr(), d_w.data_ptr(), ops._stream()), "resample_along_rays_bwd")
    return d_w.cpu().numpy()


@pytest.mark.parametrize("cls,N", [(cls, N) for cls in sf.BLUR_CLASSES for N in sf.sizes_of(cls)])
def test_every_weight_gradient_within_its_budget(G, cls, N):
    """mipnerf_resample_along_rays_bwd under one-hot, dense and all-ones upstream gradients (sampler_fixture.probes)"""
    worst, fails = {}, []
    for padding in sf.paddings_of(cls):
        for rnd in (False, True):
            c = sf.blur_case(cls, N, padding, rnd)
            tr = sf.forward_truth(c["bins"], c["w"], c["u"], True, padding)
            bins, w, r = T(c["bins"]), T(c["w"]), T(c["r"])
            probes = sf.probes(tr, c["rng"], cls, rnd)
            assert any(np.any(g != 0) for _, g, _ in probes)
            for name, g, either in probes:
                d_w = _backward(bins, w, r, padding, g)
                assert np.isfinite(d_w).all(), (name, padding, rnd)                       # the NaN it was filled with is overwritten everywhere
                ratio = float(sf.backward_ratio(d_w, tr, g, either).max())
                tag = f"pad{padding}_{'rand' if rnd else 'det'}_{name}"
                print(f"sampler backward {cls} N={N} {tag}: worst got/budget {ratio:.3g}")
                worst[tag] = ratio
                if not ratio <= 1.0:
                    fails.append((tag, ratio))
                if name == "dense":                                                        # exact structure: linear in g
                    assert np.array_equal(_bits(_backward(bins, w, r, padding, 2 * g)), _bits(2 * d_w))
                    zero = _backward(bins, w, r, padding, 0 * g)
                    assert np.all(zero == 0)
            assert np.array_equal(_bits(w.cpu().numpy()), _bits(c["w"]))
    G.record(f"sampler backward {cls} N={N}", **worst)
    assert not fails, fails
