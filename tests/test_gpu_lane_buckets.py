"""GPU: every per-ray kernel at the EDGES of the samples-per-lane buckets (csrc/lane_buckets.hpp: K = 1, 2, 4, 8, 16 for N <= 64, 128, 256,
512, 1024).  All launchers take their bucket from one rule, so at N = 64 | 65, 128 | 129, 256 | 257, 512 | 513 and 1024
  (a) the fused launches equal the per-stage ones bit for bit (mipnerf_forward, mipnerf_train_step),
  (b) every stand-alone entry point stays within the bound its own test module sets at interior N,
  (c) both ray classifiers agree with the fixtures and with each other, for a world grid and a contracted one,
  (d) and N = 1025 is refused by every per-ray entry point before anything is launched.
B = 5 rays: one full workgroup of four rays and a ragged one.  The references and the bounds are those of test_gpu_stages.py,
test_gpu_train.py, test_gpu_resample_grad.py, test_gpu_span.py and test_gpu_cull360.py: the oracle where it has the function, and for the
backward passes (the oracle has none) the float64 autograd restatements those modules define."""
import ctypes as C

import numpy as np
import pytest
import torch

import cull360_fixture as cx
import gpu_util as G
import test_gpu_cull360 as cull360
import test_gpu_resample_grad as rgrad
import test_gpu_span as span
import test_gpu_train as train
from oracle import mipnerf_oracle as orc

pytestmark = pytest.mark.gpu
DEV = G.DEV
B = 5
EDGES = [64, 65, 128, 129, 256, 257, 512, 513, 1024]


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---- (a) fused against per-stage routes --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", EDGES)
def test_forward_fused_route_equals_per_stage_route_fp32(N):
    """test_gpu_forward.test_fused_small_kernels_equal_per_stage_kernels at the bucket edges: all five outputs of both levels, same bytes"""
    rays = G.to_dev(orc.synthetic_rays(B, seed=5, multiscale=True))
    model = G.make_model(orc.make_params(seed=2, density_gain=30.0), N, "fp32")
    rng = np.random.default_rng(N)
    tr, ur = (T(rng.uniform(0, 1, (B, N + 1)).astype(np.float32)) for _ in range(2))
    for randomized in (False, True):
        outs = []
        for fuse in (1, 0):
            model.mlp.native(torch.device(DEV)).set_option(4, fuse)
            with torch.no_grad():
                kw = dict(t_rand=tr, u_rand=ur) if randomized else {}
                outs.append([tuple(x.clone() for x in lv) for lv in model(rays, randomized, True, **kw)])
        for lvl in range(2):
            assert len(outs[0][lvl]) == len(G.NAMES)
            for nm, a, b in zip(G.NAMES, outs[0][lvl], outs[1][lvl]):
                assert torch.equal(a, b), (randomized, lvl, nm)


@pytest.mark.parametrize("N", EDGES)
def test_train_step_fused_route_equals_per_stage_route(N):
    """the criteria of test_gpu_train.test_native_train_step_fused_tail_equals_per_stage_kernels (loss scalars, every gradient and the
    returned outputs bit-identical), which runs interior N"""
    train.test_native_train_step_fused_tail_equals_per_stage_kernels(G, B, N, True)


# ---- (b) stand-alone entry points -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", EDGES)
def test_volumetric_rendering(N):
    """mipnerf_volumetric_rendering against the oracle: inputs and bounds of test_gpu_stages.test_volumetric_rendering"""
    from mipnerf_pl_amd import ops
    rng = np.random.default_rng(N)
    dirs = orc.synthetic_rays(B, seed=3).directions
    t = np.sort(rng.uniform(2, 6, (B, N + 1)).astype(np.float32), axis=-1)
    rgb = rng.uniform(0, 1, (B, N, 3)).astype(np.float32)
    dens = (rng.uniform(0, 1, (B, N, 1)) ** 8 * 60).astype(np.float32)
    dens[0] = 0                # empty ray
    dens[1] = 0
    dens[1, N - 1] = 1e6       # single opaque bin: the last sample of the last lane that holds one
    for white in (True, False):
        out = ops.volumetric_rendering(T(rgb), T(dens), T(t), T(dirs), white)
        ref = orc.volumetric_rendering(rgb, dens, t, dirs, white)
        errs = [G.maxdiff(a, b) for a, b in zip(out, ref)]
        print(f"volumetric_rendering N={N} white={white} rgb/distance/acc/weights errors {errs}")
        assert errs[0] <= 1e-5 and errs[1] <= 5e-5 and errs[2] <= 1e-5 and errs[3] <= 1e-5
        assert float(out[2][0]) == 0.0 and float(out[1][0]) == float(t[0, 0])           # zero density: acc 0, distance = near
        assert torch.all(out[0][0] == (1.0 if white else 0.0))


@pytest.mark.parametrize("N", EDGES)
def test_resample_along_rays(N):
    """mipnerf_resample_along_rays against the oracle: inputs and bound of test_gpu_stages.test_resample_along_rays (weights ~ U^6, where a
    1e-7 relative change of the weight sum moves t by 4e-5: 1e-4)"""
    from mipnerf_pl_amd import ops
    rng = np.random.default_rng(N + 7)
    rays = orc.synthetic_rays(B, seed=5)
    R = G.to_dev(rays)
    t = np.sort(rng.uniform(2, 6, (B, N + 1)).astype(np.float32), axis=-1)
    w = (rng.uniform(0, 1, (B, N)) ** 6).astype(np.float32)
    w[0] = 0
    w[1] = 0
    w[1, 7] = 1.0
    for randomized in (False, True):
        u = rng.random((B, N + 1), dtype=np.float32) if randomized else None
        tn, _ = ops.resample_along_rays(R.origins, R.directions, R.radii, T(t), T(w), randomized, "cone", True, 0.01,
                                        u_rand=T(u) if randomized else None)
        to, _ = orc.resample_along_rays(rays.origins, rays.directions, rays.radii, t, w, randomized, u_rand=u)
        e = G.maxdiff(tn, to)
        print(f"resample N={N} rand={randomized} error {e}")
        assert e <= 1e-4
        tn_np = tn.cpu().numpy()
        assert np.all(np.diff(tn_np, axis=-1) >= 0)
        assert np.all(tn_np >= t[:, :1] - 1e-6) and np.all(tn_np <= t[:, -1:] + 1e-6)


@pytest.mark.parametrize("N", EDGES)
def test_distloss_and_its_backward(N):
    """mipnerf_distloss (value and d_w) as test_gpu_train.test_distloss_forward_backward: against float64 autograd (2e-6) and the oracle's
    value (2e-5)"""
    from mipnerf_pl_amd.autograd import distloss
    rng = np.random.default_rng(N + 1)
    t = torch.from_numpy(np.sort(rng.uniform(2, 6, (B, N + 1)), axis=-1).astype(np.float32))
    w = torch.from_numpy((rng.uniform(0, 1, (B, N)) ** 3).astype(np.float32))
    w64 = w.double().requires_grad_(True)
    ref = rgrad.t_distloss_rays(w64, t.double()).mean()
    ref.backward()
    wg = w.to(DEV).requires_grad_(True)
    val = distloss(wg, t.to(DEV))
    val.backward()
    ev = abs(float(val.detach()) - float(ref.detach())) / abs(float(ref.detach()))
    eg = G.maxdiff(wg.grad, w64.grad.float())
    print(f"distloss N={N} rel value {ev} grad {eg} scale {float(w64.grad.abs().max())}")
    assert ev <= 2e-6 and eg <= 2e-6 * max(1.0, float(w64.grad.abs().max()))
    np.testing.assert_allclose(float(val.detach()), float(orc.distloss(w.numpy(), t.numpy())), rtol=2e-5)


@pytest.mark.parametrize("N", EDGES)
@pytest.mark.parametrize("white", [True, False])
def test_volumetric_rendering_backward(N, white):
    """mipnerf_volumetric_rendering_bwd as test_gpu_train.test_render_backward_matches_autograd: float64 autograd, 2e-5"""
    from mipnerf_pl_amd.autograd import render_from_raw
    rng = np.random.default_rng(N)
    t = torch.from_numpy(np.sort(rng.uniform(2, 6, (B, N + 1)), axis=-1).astype(np.float32))
    raw = torch.from_numpy(rng.normal(0, 2.5, (B, N, 4)).astype(np.float32))
    dirs = torch.from_numpy(orc.synthetic_rays(B, seed=2).directions)
    coef = [torch.from_numpy(rng.normal(0, 1, s).astype(np.float32)) for s in ((B, 3), (B,), (B,), (B, N))]
    r64 = raw.double().requires_grad_(True)
    rgb = torch.sigmoid(r64[..., :3]) * 1.002 - 0.001
    den = torch.nn.functional.softplus(r64[..., 3:] - 1.0)
    out = train.torch_volumetric_rendering(rgb, den, t.double(), dirs.double(), white)
    sum((o * c).sum() for o, c in zip(out, coef)).backward()
    rg = raw.to(DEV).requires_grad_(True)
    o = render_from_raw(rg, t.to(DEV), dirs.to(DEV), white)
    sum((x * c.to(DEV)).sum() for x, c in zip(o, coef)).backward()
    for a, b in zip(o, out):
        assert G.maxdiff(a, b.float()) <= 2e-5
    e, scale = G.maxdiff(rg.grad, r64.grad.float()), float(r64.grad.abs().max())
    print(f"render_bwd N={N} white={white} error {e} scale {scale}")
    assert e <= 2e-5 * max(1.0, scale)


@pytest.mark.parametrize("N", EDGES)
def test_gradients_with_respect_to_the_fence_posts(N):
    """mipnerf_distloss_bwd and mipnerf_volumetric_rendering_bwd_t: test_gpu_resample_grad's own case and bounds at B = 5"""
    rgrad.test_distloss_and_compositing_gradient_wrt_t(B, N)


@pytest.mark.parametrize("N", EDGES)
@pytest.mark.parametrize("randomized", [False, True])
def test_resample_backward(N, randomized):
    """mipnerf_resample_along_rays_bwd: test_gpu_resample_grad's own case and bounds at B = 5 (the same draws as the forward: the one
    draw step of lane_buckets.hpp)"""
    rgrad.test_resample_backward(B, N, randomized, 0.01)


# ---- (c) the classifiers ----------------------------------------------------------------------------------------------------------------
def _five(candidates, top):
    """B frustum indices: the candidates in [0, top], repeated from the start"""
    ok = sorted({f for f in candidates if 0 <= f <= top})
    return [ok[i % len(ok)] for i in range(B)]


@pytest.mark.parametrize("N", EDGES)
def test_classifiers_on_a_world_grid(N):
    """test_gpu_span's engineered grids (one or two occupied cells, each met by one frustum alone) with five rays: first / last against
    span_fixture, `live` of ray_span byte for byte that of ray_occupancy, near' / far' the sampler's fence posts (all asserted by
    _check_engineered).  The hit frusta sit at both ends of the first lane's and the last lane's share: 0, 63, 64, N - 2, N - 1."""
    firsts = _five((0, 63, 64, N - 2, N - 1), N - 1)
    for outside in (False, True):
        want = span._check_engineered(N, 34, [32], firsts, outside_occupied=outside)
        assert want[0].all()
        if not outside:
            assert want[1].tolist() == firsts and want[2].tolist() == firsts
    if N > 64:                                                        # a second cell 64 frusta on: first and last in different buckets
        firsts = _five((0, 1, 62, 63, N - 65), N - 65)
        want = span._check_engineered(N, 2 * 64 + 36, [32, 32 + 2 * 64], firsts, outside_occupied=False)
        assert want[1].tolist() == firsts and want[2].tolist() == [f + 64 for f in firsts]


@pytest.mark.parametrize("N", EDGES)
def test_classifiers_on_a_contracted_grid(N):
    """the first five edge rays of test_gpu_cull360 (a NaN origin, from inside the unit ball, through the centre, two of the fan) against
    its sphere grid: between cull360_fixture's must and may sets, `live` of both calls the same bytes, near' / far' the fence posts"""
    from mipnerf_pl_amd import ops
    g, _ = cull360._edge_rays()
    g = {k: np.ascontiguousarray(v[:B]) for k, v in g.items()}
    rays = G.to_dev(G.rays_of(g))
    occ, occ_bool = cull360.sphere_occupancy("s64")
    live, first, last, near, far = ops.ray_span(occ, rays, N)
    assert torch.equal(live, ops.ray_occupancy(occ, rays, N))
    lv = live.cpu().numpy().astype(bool)
    args = cull360._fixture_args(occ_bool, cull360.LATTICES["s64"][0], g, N)
    (must, f_must, l_must), (may, f_may, l_may) = (cx.span(*args, margin=m) for m in (-cull360.MARGIN, cull360.MARGIN))
    assert not (must & ~lv).any() and not (lv & ~may).any()
    fi, la = first.cpu().numpy().astype(np.int64), last.cpu().numpy().astype(np.int64)
    assert ((f_may <= fi) & (fi <= f_must)).all() and ((l_must <= la) & (la <= l_may)).all()
    assert lv[0] and fi[0] == 0 and la[0] == N - 1 and lv[1] and fi[1] == 0 and lv[2]
    _, t = ops.sample_t_360(N, rays.near, rays.far, False)
    ok = torch.from_numpy(lv).to(DEV)
    ok[0] = False                                                     # NaN fence posts do not compare
    assert torch.equal(near[ok], t.gather(1, first.long().clamp(0, N)[:, None])[ok])
    assert torch.equal(far[ok], t.gather(1, (last.long() + 1).clamp(0, N)[:, None])[ok])
    dead = ~torch.from_numpy(lv).to(DEV)
    assert (first[dead] == N).all() and (last[dead] == -1).all()


# ---- (d) refusal without a launch --------------------------------------------------------------------------------------------------------
def test_one_sample_too_many_is_refused_before_any_launch():
    """N = 1025 has no bucket: MIPNERF_E_INVALID from every per-ray entry point, and the buffer every pointer argument names -- large enough
    for N = 1025, so that nothing here depends on the refusal -- keeps its bytes"""
    from mipnerf_pl_amd import _lib as L
    lib = L.lib()
    N = L.MAX_SAMPLES + 1
    buf = torch.full((B * (N + 1) * 4,), 7.0, device=DEV)
    p = buf.data_ptr()
    dims, lo, hi = (C.c_int32 * 3)(8, 8, 8), (C.c_float * 3)(-2, -2, -2), (C.c_float * 3)(2, 2, 2)
    rp = L.RaysPtrs(*[p] * 7)
    calls = {
        "mipnerf_volumetric_rendering": (B, N, p, p, p, 1, p, p, p, p, None),
        "mipnerf_composite_resample": (B, N, p, p, p, 1, p, p, p, p, p, p, 0.01, p, None),
        "mipnerf_composite_train": (B, N, p, p, p, 1, p, p, p, p, p, 0.5, p, p, 0.01, p, p, None),
        "mipnerf_resample_along_rays": (B, N, p, p, p, 0.01, p, None),
        "mipnerf_sorted_piecewise_constant_pdf": (B, N, p, p, N + 1, p, p, None),
        "mipnerf_volumetric_rendering_bwd": (B, N, p, p, p, 1, p, p, p, p, 0.001, p, None),
        "mipnerf_volumetric_rendering_bwd_t": (B, N, p, p, p, 1, p, p, p, p, 0.001, p, p, None),
        "mipnerf_distloss": (B, N, p, p, p, p, p, None),
        "mipnerf_distloss_bwd": (B, N, p, p, p, p, p, None),
        "mipnerf_resample_along_rays_bwd": (B, N, p, p, p, 0.01, p, p, None),
        "mipnerf_ray_occupancy": (dims, lo, hi, p, B, N, C.byref(rp), 0, 1, 1.0, p, None),
        "mipnerf_ray_span": (dims, lo, hi, p, B, N, C.byref(rp), 0, 1, 1.0, p, p, p, p, p, None),
        "mipnerf_ray_occupancy_360": (dims, lo, hi, p, B, N, C.byref(rp), 1, 1.0, p, None),
        "mipnerf_ray_span_360": (dims, lo, hi, p, B, N, C.byref(rp), 1, 1.0, p, p, p, p, p, None),
    }
    for name, args in calls.items():
        assert len(args) == len(L.SIGNATURES[name][1]), name
        assert getattr(lib, name)(*args) == L.E_INVALID, name
        assert name[len("mipnerf_"):] in L.last_error(), (name, L.last_error())
    torch.cuda.synchronize()
    assert bool((buf == 7.0).all())
