"""GPU: the distortion loss (distloss_ray behind mipnerf_distloss and mipnerf_distloss_bwd) against float64: the per-ray value and every
d_w / d_t entry on its own, on soft, empty, one-hot, surface, far-field and coincident rays at every lane bucket.

tests/distloss_fixture.py has the classes, the O(N^2) float64 truth from the kernel's own fp32 midpoints and intervals, and the budget of
every entry; tests/test_distloss_cpu.py checks that fixture without a GPU.  Nothing here is normalised by a batch's largest gradient;
only the fence posts at exactly tied midpoints (three per `coincident` ray, none elsewhere) are left out of d_t, where the O(N) form and
the reference's autograd pick different subgradients.  B = 18 rays (4 per workgroup: a ragged last one); a case is three launches."""
import numpy as np
import pytest
import torch

import distloss_fixture as dl

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def G():
    import gpu_util
    assert torch.cuda.is_available()
    return gpu_util


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _same_bits(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _nan(*shape):
    return torch.full(shape, float("nan"), device=DEV)


@pytest.mark.parametrize("N", dl.SIZES)
@pytest.mark.parametrize("cls", dl.CLASSES)
def test_value_and_every_gradient_entry_within_its_budget(G, cls, N):
    from mipnerf_pl_amd import _lib as L
    from mipnerf_pl_amd import ops
    B = dl.RAYS
    w, t, g, info = dl.make(cls, B, N, np.random.default_rng(dl.case_seed(cls, N)))
    w_d, t_d, g_d = T(w), T(t), T(g)
    lib, st = L.lib(), ops._stream()
    # value only
    val = _nan(B)
    L.check(lib.mipnerf_distloss(B, N, w_d.data_ptr(), t_d.data_ptr(), val.data_ptr(), None, None, st), "distloss")
    # value and d_w given g_ray, through the same entry point
    val2, dw_fwd = _nan(B), _nan(B, N)
    L.check(lib.mipnerf_distloss(B, N, w_d.data_ptr(), t_d.data_ptr(), val2.data_ptr(), g_d.data_ptr(), dw_fwd.data_ptr(), st), "distloss")
    # d_w and d_t
    dw_bwd, d_t = _nan(B, N), _nan(B, N + 1)
    L.check(lib.mipnerf_distloss_bwd(B, N, w_d.data_ptr(), t_d.data_ptr(), g_d.data_ptr(), dw_bwd.data_ptr(), d_t.data_ptr(), st),
            "distloss_bwd")
    val, val2, dw_fwd, dw_bwd, d_t = (a.cpu().numpy() for a in (val, val2, dw_fwd, dw_bwd, d_t))
    assert all(np.isfinite(a).all() for a in (val, val2, dw_fwd, dw_bwd, d_t))            # NaN-filled outputs come back finite
    assert _same_bits(val, val2) and _same_bits(dw_fwd, dw_bwd)                            # the same bits through both entry points
    assert _same_bits(w_d.cpu().numpy(), w) and _same_bits(t_d.cpu().numpy(), t)          # the inputs are not written
    tr = dl.truth(w, t, g)
    checked = dl.checked_posts(t)
    if cls == "coincident" and N >= 5:
        assert np.all((~checked).sum(-1) <= dl.MAX_UNCHECKED) and (~checked).any()
    else:
        assert checked.all()                                                               # no tie: nothing is left out
    if cls == "empty":
        assert np.all(val == 0) and np.all(dw_bwd == 0) and np.all(d_t == 0)
    if cls == "onehot":
        others = np.ones((B, N), bool)
        others[np.arange(B), info["k"]] = False
        assert np.all(dw_bwd[others & (g != 0)[:, None]] != 0)                             # 2 g |m_i - m_k|: no dead entry
    r = dl.ratios(tr, val, dw_bwd, d_t, checked)
    print(f"distloss {cls} N={N}: worst got/budget " + " ".join(f"{k}={v:.3g}" for k, v in r.items()))
    G.record(f"distloss_fixture {cls} N={N}", **r)
    assert max(r.values()) <= 1.0, r
