"""GPU: the Jacobian of the compositing backward (k_volumetric_rendering_bwd behind mipnerf_volumetric_rendering_bwd and
mipnerf_volumetric_rendering_bwd_t) entry by entry against float64, on empty, soft, opaque, surface and saturated rays.

tests/ray_jacobian.py has the ray classes, the probes (one kind of upstream gradient at a time), the float64 truth from the kernel's own
fp32 operands and the running-error budget of every entry; tests/test_ray_jacobian_cpu.py checks that fixture without a GPU.  Nothing
here is normalised by a batch's largest gradient and no entry is left out: the budget is the only slack.  B = 18 rays (4 per workgroup:
a ragged last one), N over every lane bucket K = 1, 2, 4, 8, 16 at its first size plus two ragged K = 1 sizes; a case is a few dozen
launches of at most 18 x 513 samples."""
import numpy as np
import pytest
import torch

import ray_jacobian as rj

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def G():
    import gpu_util
    assert torch.cuda.is_available()
    return gpu_util


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _backward(rs, t, d, white, g, with_t):
    """d_raw [B,N,4] (and d_t [B,N+1]) of one probe through the C entry points, as autograd._RenderFromRaw.backward calls them"""
    from mipnerf_pl_amd import _lib as L
    from mipnerf_pl_amd import ops
    B, N = rs.shape[:2]
    keep = [None if g[k] is None else T(g[k]) for k in ("g_rgb", "g_dist", "g_acc", "g_w")]
    ptrs = [None if k is None else k.data_ptr() for k in keep]
    d_raw = torch.full((B, N, 4), float("nan"), device=DEV)
    if with_t:
        d_t = torch.full((B, N + 1), float("nan"), device=DEV)
        L.check(L.lib().mipnerf_volumetric_rendering_bwd_t(B, N, rs.data_ptr(), t.data_ptr(), d.data_ptr(), int(white), *ptrs,
                                                            float(rj.PAD), d_raw.data_ptr(), d_t.data_ptr(), ops._stream()),
                "volumetric_rendering_bwd_t")
        return d_raw.cpu().numpy(), d_t.cpu().numpy()
    L.check(L.lib().mipnerf_volumetric_rendering_bwd(B, N, rs.data_ptr(), t.data_ptr(), d.data_ptr(), int(white), *ptrs, float(rj.PAD),
                                                      d_raw.data_ptr(), ops._stream()), "volumetric_rendering_bwd")
    return d_raw.cpu().numpy(), None


def _same_bits(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("N", rj.SIZES)
@pytest.mark.parametrize("cls", rj.CLASSES)
def test_every_jacobian_entry_within_its_budget(G, cls, N):
    B = rj.RAYS
    rng = np.random.default_rng(rj.case_seed(cls, N))
    rs, t, d = rj.make(cls, B, N, rng)
    ray = rj.Ray(rs, t, d)
    rs_d, t_d, d_d = T(rs), T(t), T(d)
    idx = rj.onehot_indices(B, N)
    behind = np.arange(N)[None, :] > idx[:, None]
    worst, fails = {}, []
    for name, white, g in rj.probes(B, N, rng):
        tr = rj.truth(ray, white, **g)
        d_raw, _ = _backward(rs_d, t_d, d_d, white, g, False)
        d_raw_t, d_t = _backward(rs_d, t_d, d_d, white, g, True)
        assert np.isfinite(d_raw).all() and np.isfinite(d_t).all(), (name, white)
        # the entry point that also writes d_t gives the same d_raw, and a pointer that is not driven equals a tensor of zeros: same bits
        assert _same_bits(d_raw, d_raw_t), (name, white)
        z_raw, z_t = _backward(rs_d, t_d, d_d, white, rj.zero_filled(g, B, N), True)
        assert _same_bits(d_raw, z_raw) and _same_bits(d_t, z_t), (name, white)
        assert _same_bits(d_raw, _backward(rs_d, t_d, d_d, white, rj.zero_filled(g, B, N), False)[0]), (name, white)
        # exact structure
        if name == "onehot":
            assert np.all(d_raw[..., :3] == 0) and np.all(d_raw[..., 3][behind] == 0)
        if name == "dist":
            assert np.all(d_raw[~ray.inside] == 0)
            if cls == "empty":
                assert not ray.inside.any()
        r = rj.ratios(d_raw, d_t, tr)
        tag = f"{name}{'_white' if white else ''}"
        print(f"ray_jacobian {cls} N={N} {tag}: worst got/budget " + " ".join(f"{k}={v:.3g}" for k, v in r.items()))
        for k, v in r.items():
            worst[f"{tag}_{k}"] = v
            if not v <= 1.0:
                fails.append((tag, k, v))
    G.record(f"ray_jacobian {cls} N={N}", **worst)
    assert not fails, fails


def test_density_gradient_from_raw_is_the_sigmoid(G):
    """One sample per ray from the raw density on: mipnerf_activate (density_bias -1), then the backward with g_acc = 1.
    acc = 1 - exp(-softplus(x) delta), so d_raw.w = delta exp(-softplus(x) delta) sigmoid(x), x = raw - 1: the reference's own
    derivative, not only the kernel's reading of its sigma (ray_jacobian.from_raw_case).  float64 from the fp32 x, 16 x 2^-24
    relative, and no entry is 0."""
    from mipnerf_pl_amd import _lib as L
    from mipnerf_pl_amd import ops
    raw, t, d, want = rj.from_raw_case()
    B = raw.shape[0]
    raw_d, t_d, d_d = T(raw), T(t), T(d)
    rs = torch.empty_like(raw_d)
    L.check(L.lib().mipnerf_activate(B, raw_d.data_ptr(), float(rj.PAD), rj.FROM_RAW_BIAS, None, 0.0, rs.data_ptr(), ops._stream()),
            "activate")
    rj.check_inputs(rs.cpu().numpy(), t, d)
    g = dict(g_rgb=None, g_dist=None, g_acc=np.ones(B, np.float32), g_w=None)
    d_raw, _ = _backward(rs, t_d, d_d, 0, g, False)
    got = d_raw[:, 0, 3].astype(np.float64)
    rel = np.abs(got - want) / want
    worst = int(rel.argmax())
    print(f"ray_jacobian from raw: worst relative error {rel.max():.3g} = {rel.max() * 2.0 ** 24:.2f} x 2^-24 at raw density "
          f"{raw[worst, 0, 3]:.3f}; {int((got == 0).sum())} dead entries")
    G.record("ray_jacobian from_raw", rel=rel.max(), ulps=rel.max() * 2.0 ** 24, dead=float((got == 0).sum()))
    assert np.all(got != 0)
    assert rel.max() <= rj.FROM_RAW_BOUND
    assert np.all(d_raw[..., :3] == 0)
