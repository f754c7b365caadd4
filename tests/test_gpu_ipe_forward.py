"""GPU: the forward Gaussians and encodings entry by entry against float64 -- k_cast_rays, k_integrated_pos_enc and k_cast_ipe (fp32 and
bf16) and k_pos_enc behind ops.cast_rays, ops.integrated_pos_enc, ops.cast_ipe and ops.pos_enc -- on six classes of rays, five ragged
shapes (7 to 513 samples: below, at, one past and four times a workgroup's 128) and six configurations of degrees.

tests/ipe_forward.py has the operands, the float64 truths, the budget of every entry and the constants, which come from the host build
of csrc/raymath.hpp and never from a kernel; tests/test_ipe_forward_cpu.py checks that fixture without a GPU.  Nothing here is
normalised by a batch maximum and no entry is left out.  Every result is taken twice: through the ops function, and through the same
C entry point into a buffer with a canary tail, which must come back untouched and with the same bits in front of it.

k_ray_prologue and k_lattice_ipe (and the rows the generated MLP kernels form in registers) have no entry point that returns their
rows: the existing bit-equality tests (test_fused_ipe_equals_separate_kernel and its kin) tie them to k_cast_ipe, which is pinned
here."""
import numpy as np
import pytest
import torch

import ipe_forward as fw

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CANARY_VALUE = -7.25           # exact in bf16


@pytest.fixture(scope="module")
def G():
    import gpu_util
    assert torch.cuda.is_available()
    return gpu_util


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _np(t):
    """fp32 numpy of an fp32 or bf16 device tensor (the widening is exact)"""
    return t.float().cpu().numpy()


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


def _prec(bf16):
    from mipnerf_pl_amd import _lib as L
    return L.PREC_BF16 if bf16 else L.PREC_FP32


def _guarded(shape, bf16, launch, what):
    """run launch(ptr) on a buffer of `shape` followed by a canary tail; returns the fp32 numpy of the front"""
    from mipnerf_pl_amd import _lib as L
    n = int(np.prod(shape))
    buf = torch.full((n + fw.CANARY,), CANARY_VALUE, device=DEV, dtype=torch.bfloat16 if bf16 else torch.float32)
    L.check(launch(buf.data_ptr()), what)
    out = _np(buf)
    assert np.all(out[n:] == np.float32(CANARY_VALUE)), f"{what} wrote behind its output"
    return out[:n].reshape(shape)


def cast_rays(dev, B, N):
    from mipnerf_pl_amd import _lib as L
    from mipnerf_pl_amd import ops
    t, o, d, r = dev
    mean, cov = (_np(a) for a in ops.cast_rays(t, o, d, r.reshape(B, 1)))
    scratch = torch.empty(B * N * 3, device=DEV)                  # one output at a time behind the canary, the other one here
    gm = _guarded((B, N, 3), False, lambda p: L.lib().mipnerf_cast_rays(B, N, t.data_ptr(), o.data_ptr(), d.data_ptr(), r.data_ptr(), p,
                                                                         scratch.data_ptr(), ops._stream()), "cast_rays means")
    gc = _guarded((B, N, 3), False, lambda p: L.lib().mipnerf_cast_rays(B, N, t.data_ptr(), o.data_ptr(), d.data_ptr(), r.data_ptr(),
                                                                         scratch.data_ptr(), p, ops._stream()), "cast_rays covs")
    assert _same_bits(mean, gm) and _same_bits(cov, gc)
    return mean, cov


def ipe(mean_d, cov_d, cfg, bf16):
    from mipnerf_pl_amd import _lib as L
    from mipnerf_pl_amd import ops
    M = mean_d.numel() // 3
    got = _np(ops.integrated_pos_enc((mean_d, cov_d), cfg[0], cfg[1], precision=_prec(bf16)))
    g = _guarded(got.shape, bf16, lambda p: L.lib().mipnerf_integrated_pos_enc(M, cfg[0], cfg[1], mean_d.data_ptr(), cov_d.data_ptr(), p,
                                                                               _prec(bf16), ops._stream()), "integrated_pos_enc")
    assert _same_bits(got, g)
    return got


def cast_ipe(dev, B, N, cfg, bf16):
    from mipnerf_pl_amd import _lib as L
    from mipnerf_pl_amd import ops
    t, o, d, r = dev
    got = _np(ops.cast_ipe(t, o, d, r.reshape(B, 1), cfg[0], cfg[1], disable_integration=cfg[2], precision=_prec(bf16)))
    g = _guarded(got.shape, bf16, lambda p: L.lib().mipnerf_cast_ipe(B, N, cfg[0], cfg[1], int(cfg[2]), t.data_ptr(), o.data_ptr(),
                                                                     d.data_ptr(), r.data_ptr(), p, _prec(bf16), ops._stream()), "cast_ipe")
    assert _same_bits(got, g)
    return got


def _check(worst, fails, key, got, truth, budget):
    v = fw.worst(got, truth, budget)
    worst[key] = max(worst.get(key, 0.0), v)
    if not v <= 1.0:
        fails.append((key, v))


@pytest.mark.parametrize("shape", fw.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("cls", fw.CLASSES)
def test_gaussians_and_rows_within_their_budgets(G, cls, shape):
    B, N = shape
    t, o, d, r, _ = fw.make(cls, B, N)
    dev = (T(t), T(o), T(d), T(r))
    worst, fails = {}, []
    # the Gaussians: the host build's bits, and as a backstop the float64 budgets
    mean, cov = cast_rays(dev, B, N)
    hmean, hcov = fw.host_gaussians(t, o, d, r)
    tr = fw.gaussian_truth(t, o, d, r)
    worst["mean"], worst["cov"] = fw.gaussian_ratios(mean, cov, tr)
    print(f"ipe_forward {cls} {B}x{N}: mean got/budget {worst['mean']:.3g}, cov {worst['cov']:.3g}; bits that differ from the host build: "
          f"{int((mean.view(np.uint32) != hmean.view(np.uint32)).sum())} means, {int((cov.view(np.uint32) != hcov.view(np.uint32)).sum())} covs")
    assert _same_bits(mean, hmean), "means differ from the host build of raymath.hpp"
    assert _same_bits(cov, hcov), "covariances differ from the host build of raymath.hpp"
    assert worst["mean"] <= 1.0 and worst["cov"] <= 1.0
    mean_d, cov_d, zero_d = T(mean), T(cov), torch.zeros(B, N, 3, device=DEV)
    for cfg in fw.CONFIGS:
        k, noint = fw.config_id(cfg), cfg[2]
        ft = fw.feature_truth(mean, cov, cfg)
        rows = {}
        for bf16 in (False, True):
            p = "bf16" if bf16 else "f32"
            got = ipe(mean_d, zero_d if noint else cov_d, (cfg[0], cfg[1], False), bf16)
            rows[p] = got
            _check(worst, fails, f"{p} {k}", got, ft["truth"], ft["bf16"] if bf16 else fw.f32_budget(ft["truth"]))
            # the fused kernel: the same bits as the two launches; disable_integration is the same call on zeroed covariances
            assert _same_bits(cast_ipe(dev, B, N, cfg, bf16), got), (p, k)
        dead = ft["damp"] == 0
        assert np.all(rows["f32"][dead] == 0) and np.all(rows["bf16"][dead] == 0), k          # float64's exp underflowed: exactly +-0
    print(f"ipe_forward {cls} {B}x{N}: worst got/budget " + " ".join(f"{k}={v:.3g}" for k, v in worst.items()))
    G.record(f"ipe_forward {cls} {B}x{N}", **worst)
    assert not fails, fails


def test_hand_made_table(G):
    """mean in {+0, -0, a denormal, 1e-20, +-1, 1e6} x cov in {0, a denormal, 1e-12, 1, 1e30}, degrees (0, 16)"""
    mean, cov = fw.table()
    cfg = fw.CONFIGS[0]
    ft = fw.feature_truth(mean, cov, cfg)
    with np.errstate(over="ignore"):
        yv = cov[:, None, :] * (4.0 ** np.arange(16)).astype(np.float32)[:, None]
    dead = fw._flat(yv, yv) >= 300                         # exp(-150) and below, yv = inf included
    assert np.isinf(yv).any()
    worst, fails = {}, []
    for bf16 in (False, True):
        p = "bf16" if bf16 else "f32"
        got = ipe(T(mean), T(cov), cfg, bf16)
        assert not np.isnan(got).any(), p
        assert np.all(got[dead] == 0), p                   # exactly +-0, not NaN and not a denormal
        _check(worst, fails, p, got, ft["truth"], ft["bf16"] if bf16 else fw.f32_budget(ft["truth"]))
    print("ipe_forward table: worst got/budget " + " ".join(f"{k}={v:.3g}" for k, v in worst.items()))
    G.record("ipe_forward table", **worst)
    assert not fails, fails


@pytest.mark.parametrize("B", [1, 7, 257])
@pytest.mark.parametrize("deg", [0, 4])
def test_view_encoding(G, deg, B):
    from mipnerf_pl_amd import _lib as L
    from mipnerf_pl_amd import ops
    from mipnerf_pl_amd.mlp_plan import bf16_round
    v = fw.view_dirs(B)
    v_d = T(v)
    truth, exact = fw.view_truth(v, deg)
    width = 3 + 6 * deg
    worst, fails = {}, []
    for ld in (width, -(-width // 8) * 8):
        rows = {}
        for bf16 in (False, True):
            got = _np(ops.pos_enc(v_d, 0, deg, True, precision=_prec(bf16), ld=ld))
            g = _guarded((B, ld), bf16, lambda p: L.lib().mipnerf_pos_enc(B, deg, v_d.data_ptr(), p, ld, _prec(bf16), ops._stream()), "pos_enc")
            assert _same_bits(got, g)
            rows[bf16] = got
        f32 = rows[False]
        assert np.all(f32[:, width:] == 0) and np.all(rows[True][:, width:] == 0)                 # pad columns
        assert _same_bits(f32[:, :3], v)                                                          # identity columns, the denormal included
        assert _same_bits(rows[True], bf16_round(f32))
        _check(worst, fails, f"ld{ld}", f32[:, :width], truth, fw.f32_budget(truth))
    print(f"ipe_forward view deg={deg} B={B}: worst got/budget " + " ".join(f"{k}={v:.3g}" for k, v in worst.items()))
    G.record(f"ipe_forward view deg{deg} B{B}", **worst)
    assert not fails, fails
