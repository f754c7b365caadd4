"""GPU: the Jacobian of the IPE backward (k_cast_ipe_bwd behind mipnerf_cast_ipe_bwd and autograd._CastIPE) entry by entry against
float64, on six classes of rays and fence posts, four configurations of degrees and four ragged shapes.

tests/ipe_jacobian.py has the classes, the probes (a few features of d_enc at a time), the float64 truth from the device's own fp32
Gaussians (ops.cast_rays on the same inputs) and the budget of every d_t entry; tests/test_ipe_jacobian_cpu.py checks that fixture
without a GPU.  Nothing here is normalised by a batch's largest gradient and no entry is left out: the budget is the only slack.  A
case is a few dozen launches of at most 3 x 171 = 513 samples (one thread past two workgroups)."""
import numpy as np
import pytest
import torch

import ipe_jacobian as ij

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CANARY_VALUE = -7.25


@pytest.fixture(scope="module")
def G():
    import gpu_util
    assert torch.cuda.is_available()
    return gpu_util


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _same_bits(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _backward(dev, cfg, g, prefill):
    """d_t [B,N+1] of one probe through the C entry point, accumulated into `prefill` (zeros if None); a canary behind d_t stays"""
    from mipnerf_pl_amd import _lib as L
    from mipnerf_pl_amd import ops
    t, o, d, r = dev
    B, N = t.shape[0], t.shape[1] - 1
    n = B * (N + 1)
    buf = torch.full((n + ij.CANARY,), CANARY_VALUE, device=DEV)
    buf[:n] = 0.0 if prefill is None else T(prefill).reshape(-1)
    g_d = T(g)
    L.check(L.lib().mipnerf_cast_ipe_bwd(B, N, cfg[0], cfg[1], int(cfg[2]), t.data_ptr(), o.data_ptr(), d.data_ptr(), r.data_ptr(),
                                         g_d.data_ptr(), buf.data_ptr(), ops._stream()), "cast_ipe_bwd")
    out = buf.cpu().numpy()
    assert np.all(out[n:] == np.float32(CANARY_VALUE)), "k_cast_ipe_bwd wrote behind d_t"
    return out[:n].reshape(B, N + 1)


def _through_autograd(dev, cfg, g):
    from mipnerf_pl_amd.autograd import _CastIPE
    t, o, d, r = dev
    tt = t.clone().requires_grad_(True)
    _CastIPE.apply(tt, o, d, r, cfg[0], cfg[1], cfg[2]).backward(T(g))
    return tt.grad.cpu().numpy()


@pytest.mark.parametrize("shape", ij.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("cfg", ij.CONFIGS, ids=ij.config_id)
@pytest.mark.parametrize("cls", ij.CLASSES)
def test_every_fence_post_within_its_budget(G, cls, cfg, shape):
    from mipnerf_pl_amd import ops
    B, N = shape
    L = cfg[1] - cfg[0]
    seed = ij.case_seed(cls, cfg, B, N)
    t, o, d, r, _ = ij.make(cls, B, N, np.random.default_rng(seed))
    dev = (T(t), T(o), T(d), T(r))
    # the operands of the truth are the device's own Gaussians; the host build of raymath.hpp gives the same means and nearly the same covs
    mean, cov = (a.cpu().numpy() for a in ops.cast_rays(dev[0], dev[1], dev[2], dev[3].reshape(B, 1)))
    hmean, hcov = ij.host_gaussians(t, o, d, r)
    assert _same_bits(mean, hmean)
    cov_ulps = ij.ulp_distance(cov, hcov)
    jac = ij.Jacobian(t, o, d, r, mean, cov, cfg)
    damp = np.concatenate([jac.damp.reshape(B, N, 3 * L)] * 2, -1)
    worst, fails = {"cov_ulps": float(cov_ulps)}, []
    span16 = L == 16                                         # the forward behind _CastIPE is generated for 16 degrees
    for kind, name, g, pre in ij.probes(B, N, L, np.random.default_rng(seed + 1)):
        got = _backward(dev, cfg, g, pre)
        assert np.isfinite(got).all(), name
        tr = jac.truth(g, pre)
        if kind == "onehot":
            rnd, parity = (int(v) for v in name[len("onehot"):].split("_"))
            _, touched, feat, drive = ij.onehot_probe(B, N, L, rnd, parity)
            assert np.all(got[~touched] == 0), name                               # a post that touches no driven sample: exactly 0
            dead = drive & (damp[np.arange(B)[:, None], np.arange(N)[None, :], feat] == 0)
            assert np.all(got[:, :-1][dead] == 0) and np.all(got[:, 1:][dead] == 0), name    # an underflowed damping factor: exactly 0
            if span16 and rnd == 0 and parity == 0:                              # one contribution per post: autograd gives the same bits
                assert _same_bits(got, _through_autograd(dev, cfg, g)), name
        if kind == "zero":
            assert _same_bits(got, pre), name                                     # a zero d_enc leaves a pre-filled d_t as it is
        if kind == "dense" and span16:
            v = ij.ratio(_through_autograd(dev, cfg, g), tr)
            worst["autograd"] = v
            if not v <= 1.0:
                fails.append(("autograd", v))
        v = ij.ratio(got, tr)
        worst[kind] = max(worst.get(kind, 0.0), v)
        if not v <= 1.0:
            fails.append((name, v))
    print(f"ipe_jacobian {cls} {ij.config_id(cfg)} {B}x{N}: worst got/budget " + " ".join(f"{k}={v:.3g}" for k, v in worst.items()))
    G.record(f"ipe_jacobian {cls} {ij.config_id(cfg)} {B}x{N}", **worst)
    assert not fails, fails
