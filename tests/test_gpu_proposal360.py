"""GPU: the proposal density of the unbounded-scene model (csrc/kernels_proposal_360.hip, libmipnerf_proposal_360.so,
ops.ProposalGrid360 / field_proposal_360 / lattice_density_360).

  - ops.lattice_density_360 torch.equal to the float32 restatement (tests/proposal360_fixture.py) evaluated at the means and covariances
    ops.cast_rays_360(contracted=True) returns on the device: the three pyramids of the CPU test with random lattices, ragged and
    multi-block sizes, scene rays and hand-made ones (an origin inside the unit ball, a ray through the origin, far = 1e4, radius 0, a NaN
    origin between two good rays); every level of the four-level pyramid is selected and every pair of neighbours is mixed, asserted on the
    restatement, so the comparison cannot pass by reading level 0 alone;
  - ops.field_proposal_360 of the trained field: each level is the ops.density_grid(space='contracted') call at its own spacing, byte for
    byte, and the lookup on it is the restatement again;
  - what the constructor and the stage refuse."""
import os

import numpy as np
import pytest
import torch

import gpu_util as G
import proposal360_fixture as qx
import proposal_fixture as px
import test_gpu_cull360 as C3

pytestmark = pytest.mark.gpu
DEV = G.DEV
LO, HI = qx.LO, qx.HI
SIZES = [(1, 1), (3, 85), (1, 257), (37, 64), (5, 1024)]
FOOTPRINTS = (1.0, 8.0)          # 8: the scene's contracted frusta are 0.015 .. 0.15 wide, the coarse test pyramids start at 0.125 and 1
NAN_RAY = 2


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


def _hand_made_rays():
    """an origin inside the unit ball looking outwards; a ray through the origin; a NaN origin; far = 1e4; radius 0"""
    o = np.array([[0.2, 0.1, -0.3], [-2.0, -1.0, 0.5], [np.nan, 0.0, 3.0], [0.0, 0.0, 3.0], [3.0, -1.0, 1.0]])
    d = np.array([_unit([0.6, 0.64, 0.48]), _unit([2.0, 1.0, -0.5]), _unit([0.3, 0.5, -0.6]), _unit([0.8, 0.0, -0.6]), _unit([-1.0, 0.2, -0.1])])
    radii = np.array([0.01, 0.02, 0.01, 0.005, 0.0])[:, None]
    near, far = np.array([0.05, 0.1, 0.5, 1.0, 0.9])[:, None], np.array([20.0, 30.0, 50.0, 1e4, 17.0])[:, None]
    f = [np.ascontiguousarray(a, np.float32) for a in (o, d, d, radii, np.ones((5, 1)), near, far)]
    return G.to_dev(f)


def _six(covs):
    """[B, N, 3, 3] -> [B, N, 6] in the order xx, xy, xz, yy, yz, zz"""
    return torch.stack([covs[..., 0, 0], covs[..., 0, 1], covs[..., 0, 2], covs[..., 1, 1], covs[..., 1, 2], covs[..., 2, 2]], -1)


def _stage(grid, lattices, rays, N):
    """(device result [B, N], restatement (value, l, g) at the device's own Gaussians)"""
    from mipnerf_pl_amd import ops
    _, t = ops.sample_t_360(N, rays.near, rays.far, False)
    got = ops.lattice_density_360(grid, t, rays.origins, rays.directions, rays.radii)
    means, covs = ops.cast_rays_360(t, rays.origins, rays.directions, rays.radii, contracted=True)
    want = qx.pyramid_f32(lattices, LO, HI, grid.footprint, means.cpu().numpy(), _six(covs).cpu().numpy())
    assert torch.equal(ops.lattice_density_360(grid, t, rays.origins, rays.directions, rays.radii), got)      # two runs, the same bytes
    return got.cpu(), want, means.cpu().numpy()


# ---- 1. the stage, bit for bit ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("footprint", FOOTPRINTS)
@pytest.mark.parametrize("name", list(qx.PYRAMIDS))
def test_lattice_density_360_equals_the_float32_restatement_at_the_cast_rays_360_gaussians(name, footprint):
    from mipnerf_pl_amd import Rays, ops
    lattices = qx.random_pyramid(name, seed=31)
    grid = ops.ProposalGrid360([torch.from_numpy(g).to(DEV) for g in lattices], LO, HI, far_radius=64.0, footprint=footprint)
    assert len(grid) == len(lattices) and grid.dims == [(s[2], s[1], s[0]) for s in qx.PYRAMIDS[name]] and grid.space == "contracted"
    assert np.array_equal(np.asarray(grid.spacing, np.float32), qx.spacings(lattices, LO, HI))
    _, scene = C3.ray_set("scene360_rays/6")
    hand = _hand_made_rays()
    levels, mixed = np.zeros(len(lattices), np.int64), np.zeros(len(lattices), np.int64)
    for B, N in SIZES:
        for rays in (Rays(*[t[:B].contiguous() for t in scene]), hand):
            got, (want, l, g), means = _stage(grid, lattices, rays, N)
            assert got.shape == (rays.origins.shape[0], N)
            assert torch.equal(got, torch.from_numpy(want)), (B, N, G.maxdiff(got, torch.from_numpy(want)))
            assert bool((got >= 0).all())
            finite = np.isfinite(means).all(-1)
            assert (np.linalg.norm(means[finite].astype(np.float64), axis=-1) < 2.0).all()           # contracted: inside the usual box
            levels += np.bincount(l[finite], minlength=len(lattices))
            mixed += np.bincount(l[finite & (g > 0)], minlength=len(lattices))
            if rays is hand:
                assert not finite[NAN_RAY].any() and bool((got[NAN_RAY] == 0).all())                # the NaN ray: 0 ...
                assert finite[NAN_RAY - 1].all() and finite[NAN_RAY + 1].all()                       # ... and its neighbours unaffected
                assert (np.linalg.norm(means[0, 0].astype(np.float64)) < 1.0) or N == 1              # the first sample lies inside the unit ball
    print(f"pyramid {name}, footprint {footprint}: samples per level {levels.tolist()}, mixed with the next level {mixed.tolist()}")
    if footprint == FOOTPRINTS[-1] and len(lattices) > 1:
        assert (levels > 0).all() and (mixed[:-1] > 0).all()       # every level is read, every pair of neighbours mixed
    else:
        assert levels[0] > 0


# ---- 2. the trained field's own pyramid ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_field_proposal_360_is_density_grid_per_level_and_the_lookup_is_the_restatement(precision):
    from mipnerf_pl_amd import Rays, ops
    model = C3.model360(precision)
    far_radius = C3.frame_far_radius()
    grid = ops.field_proposal_360(model, grid=16, levels=3, far_radius=far_radius)
    assert grid.dims == [(16,) * 3, (8,) * 3, (4,) * 3] and grid.footprint == 1.0 and grid.far_radius == far_radius
    assert (grid.lo, grid.hi) == ((-2.0,) * 3, (2.0,) * 3)
    for n, lat in zip((16, 8, 4), grid.lattices):
        assert torch.equal(lat, ops.density_grid(model, n, -2.0, 2.0, space="contracted", far_radius=far_radius))
        assert bool((lat >= 0).all()) and bool((lat > 0).any())
    one = ops.field_proposal_360(model, grid=16, far_radius=far_radius)
    assert len(one) == 1 and torch.equal(one.lattices[0], grid.lattices[0])
    _, all_rays = C3.ray_set(C3.FRAME_SET)
    rays = Rays(*[t[:130].contiguous() for t in all_rays])
    lattices = [g.cpu().numpy() for g in grid.lattices]
    got, (want, l, g), _ = _stage(grid, lattices, rays, 96)
    assert torch.equal(got, torch.from_numpy(want)) and bool((got > 0).any())
    # one level: the plain trilinear value at the contracted mean
    _, t = ops.sample_t_360(96, rays.near, rays.far, False)
    means, _ = ops.cast_rays_360(t, rays.origins, rays.directions, rays.radii, contracted=True)
    plain = px.trilinear_f32(lattices[0], LO, HI, means.cpu().numpy())
    assert torch.equal(ops.lattice_density_360(one, t, rays.origins, rays.directions, rays.radii).cpu(), torch.from_numpy(plain))


# ---- 3. refusals ---------------------------------------------------------------------------------------------------------------------
def test_what_the_constructor_and_the_stage_refuse():
    from mipnerf_pl_amd import ops
    z = lambda n: torch.zeros(n, n, n, device=DEV)  # noqa: E731
    with pytest.raises(ValueError, match="1 .. 4 levels"):
        ops.ProposalGrid360([z(33), z(17), z(9), z(5), z(3)], -2.0, 2.0, 64.0)
    with pytest.raises(ValueError, match="1 .. 4 levels"):
        ops.ProposalGrid360([], -2.0, 2.0, 64.0)
    with pytest.raises(ValueError, match="increase strictly"):
        ops.ProposalGrid360([z(9), z(9)], -2.0, 2.0, 64.0)
    with pytest.raises(ValueError, match="at least 2 points"):
        ops.ProposalGrid360([torch.zeros(4, 1, 4, device=DEV)], -2.0, 2.0, 64.0)
    with pytest.raises(ValueError, match="hi > lo"):
        ops.ProposalGrid360([z(4)], 2.0, -2.0, 64.0)
    with pytest.raises(ValueError, match="far_radius"):
        ops.ProposalGrid360([z(4)], -2.0, 2.0, 1.0)
    for fp in (-1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="footprint"):
            ops.ProposalGrid360([z(4)], -2.0, 2.0, 64.0, footprint=fp)
    with pytest.raises(RuntimeError, match="HIP device"):
        ops.ProposalGrid360([torch.zeros(4, 4, 4)], -2.0, 2.0, 64.0)
    bounded = ops.ProposalGrid(z(4), -2.0, 2.0)
    t = torch.linspace(1.0, 2.0, 9, device=DEV)[None]
    o = torch.zeros(1, 3, device=DEV)
    with pytest.raises(TypeError, match="ProposalGrid360"):
        ops.lattice_density_360(bounded, t, o, o, torch.zeros(1, device=DEV))
    with pytest.raises(ValueError, match="unbounded=True"):
        ops.field_proposal_360(C3._bounded_model(), grid=8)
    with pytest.raises(NotImplementedError, match="unbounded=True"):
        ops.field_proposal(C3.model360("fp32"), grid=8, lo=-2.0, hi=2.0)                    # the bounded route keeps refusing
    # a single tensor is a one-level pyramid; zero rays launch nothing
    grid = ops.ProposalGrid360(z(4), -2.0, 2.0, 64.0)
    out = ops.lattice_density_360(grid, torch.zeros(0, 9, device=DEV), torch.zeros(0, 3, device=DEV), torch.zeros(0, 3, device=DEV),
                                  torch.zeros(0, device=DEV))
    assert out.shape == (0, 8)


# ---- 4. where the pyramid puts the fine samples: recorded, not presumed --------------------------------------------------------------
# PSNR of the fine level's colour against the golden file's own fine colour (the 360 oracle's two-level forward, not the code under test)
# on the 1000 rays of full360_1000x96, measured on MI355X (profiles/proposal360_rate.json).  Both levels are composed here through the
# stage entry points, as MipNerf._forward_native(proposal=ProposalGrid360) composes them; the same composition with the MLP as the
# coarse level is held torch.equal to the native two-level forward first.
TWO_LEVEL_MEASURED = {"fp32": 125.61, "bf16": 70.21}          # recorded beside them: the 1e-6 level in fp32, bf16's own error in bf16
QUALITY_MEASURED = {
    ("fp32", 64, 1): 62.66, ("bf16", 64, 1): 61.87,
    ("fp32", 64, 3): 62.34, ("bf16", 64, 3): 61.59,
    ("fp32", 128, 1): 59.80, ("bf16", 128, 1): 59.51,
    ("fp32", 128, 3): 62.42, ("bf16", 128, 3): 61.72,
}


def _margin(grid, levels):
    """the larger of test_gpu_span's QUALITY_MARGIN (0.05 dB) and five times the fp32 - bf16 difference measured on these rays"""
    import test_gpu_span as SP
    return max(SP.QUALITY_MARGIN, 5.0 * abs(QUALITY_MEASURED[("fp32", grid, levels)] - QUALITY_MEASURED[("bf16", grid, levels)]))


def _psnr(a, b):
    mse = float(((a.double() - b.double()) ** 2).mean())
    return float("inf") if mse == 0.0 else -10.0 * float(np.log10(mse))


def _compose(model, rays, coarse):
    """both levels through the stage entry points; coarse(t0) -> [B, N, 4] (colour, density) of level 0; 1 / t_inv is a torch op here"""
    from mipnerf_pl_amd import ops
    N = model.num_samples
    t_inv0, t0 = ops.sample_t_360(N, rays.near, rays.far, False)
    w0 = ops.volumetric_rendering_packed(coarse(t0), t0, rays.directions, True)[3]
    t1 = torch.reciprocal(ops.resample_t(t_inv0, w0, False, model.resample_padding))
    enc = ops.cast_ipe_360(t1, rays.origins, rays.directions, rays.radii, model.min_deg_point, model.max_deg_point, precision=model.precision)
    _, _, act = model.mlp(enc, ops.pos_enc(rays.viewdirs, 0, model.deg_view), return_activated=True)
    return ops.volumetric_rendering_packed(act, t1, rays.directions, True)[0], t1


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_quality_of_the_fine_level_behind_a_pyramid_of_the_trained_field(precision):
    """Each configuration is held at its measured PSNR minus the margin; that three levels beat one at 128^3 and that a finer single
    lattice scores LOWER (64^3 above 128^3) is recorded, not asserted."""
    from mipnerf_pl_amd import ops
    model = C3.model360(precision)
    _, rays = C3.ray_set(C3.FRAME_SET)
    golden = torch.from_numpy(G.load_golden(C3.FRAME_SET)["l1_rgb"]).to(DEV)

    def coarse_mlp(t0):
        enc = ops.cast_ipe_360(t0, rays.origins, rays.directions, rays.radii, model.min_deg_point, model.max_deg_point, precision=model.precision)
        return model.mlp(enc, ops.pos_enc(rays.viewdirs, 0, model.deg_view), return_activated=True)[2]
    with torch.no_grad():
        two = model._forward_native(rays, False, True)
        rgb, t1 = _compose(model, rays, coarse_mlp)
        assert torch.equal(rgb, two[1][0]) and torch.equal(t1, two[1][4])                   # the composition is the forward
        figures = {"two_level": _psnr(two[1][0], golden)}
        for grid, levels in ((64, 1), (64, 3), (128, 1), (128, 3)):
            pyramid = ops.field_proposal_360(model, grid=grid, levels=levels, far_radius=C3.frame_far_radius())

            def coarse_lattice(t0):
                sigma = ops.lattice_density_360(pyramid, t0, rays.origins, rays.directions, rays.radii)
                return torch.cat([torch.zeros(*sigma.shape, 3, device=sigma.device), sigma[..., None]], dim=-1).contiguous()
            figures[(grid, levels)] = _psnr(_compose(model, rays, coarse_lattice)[0], golden)
            del pyramid
    print(f"proposal pyramid quality {precision}: {figures}")
    G.record(f"full360 proposal pyramid {precision}", **{str(k): v for k, v in figures.items()})
    # the existing parity: no entry off by more than the suite's own bound for this precision gives at least -20 log10(bound) dB
    assert figures["two_level"] >= -20.0 * np.log10(G.tol_for(precision, "full360")["rgb"]), figures
    for grid, levels in ((64, 1), (64, 3), (128, 1), (128, 3)):
        assert abs(figures[(grid, levels)] - QUALITY_MEASURED[(precision, grid, levels)]) <= _margin(grid, levels), (grid, levels, figures)


# ---- 5. the chunk forward: _forward_native(proposal=ProposalGrid360) = the per-stage composition ---------------------------------------
_CACHE = {}


def _pyramid(kind, precision="fp32"):
    """'trained1' / 'trained3': the trained field's own pyramid at grid 16 with 1 / 3 levels; 'zero': all zero; 'slab': density 40 at the
    points with 0.8 <= |x| <= 1.2 of every level (16 / 8 / 4 points per axis), 0 elsewhere"""
    from mipnerf_pl_amd import ops
    key = (kind, precision)
    if key not in _CACHE:
        if kind.startswith("trained"):
            _CACHE[key] = ops.field_proposal_360(C3.model360(precision), grid=16, levels=int(kind[-1]), far_radius=C3.frame_far_radius())
        elif kind == "zero":
            _CACHE[key] = ops.ProposalGrid360([torch.zeros(16, 16, 16, device=DEV), torch.zeros(8, 8, 8, device=DEV)], LO, HI, 64.0)
        else:
            levels = []
            for n in (16, 8, 4):
                x = torch.linspace(-2.0, 2.0, n, device=DEV).abs()
                levels.append((40.0 * ((x >= 0.8) & (x <= 1.2)).float())[None, None, :].expand(n, n, n).contiguous())
            _CACHE[key] = ops.ProposalGrid360(levels, LO, HI, 64.0)
    return _CACHE[key]


def _composition(model, grid, rays, white, t_rand=None, u_rand=None):
    """the two levels through the per-stage entry points"""
    from mipnerf_pl_amd import ops
    N, rnd = model.num_samples, t_rand is not None
    t_inv0, t0 = ops.sample_t_360(N, rays.near, rays.far, rnd, t_rand)
    sigma = ops.lattice_density_360(grid, t0, rays.origins, rays.directions, rays.radii)
    packed = torch.cat([torch.zeros(*sigma.shape, 3, device=sigma.device), sigma[..., None]], dim=-1).contiguous()
    rgb0, dist0, acc0, w0 = ops.volumetric_rendering_packed(packed, t0, rays.directions, white)
    t_inv1 = ops.resample_t(t_inv0, w0, rnd, model.resample_padding, u_rand)
    t1 = ops.reciprocal_360(t_inv1)
    assert torch.equal(t1, torch.reciprocal(t_inv1))
    enc = ops.cast_ipe_360(t1, rays.origins, rays.directions, rays.radii, model.min_deg_point, model.max_deg_point, precision=model.precision)
    _, _, act = model.mlp(enc, ops.pos_enc(rays.viewdirs, 0, model.deg_view), return_activated=True)
    rgb1, dist1, acc1, w1 = ops.volumetric_rendering(act[..., :3], act[..., 3:4], t1, rays.directions, white)
    return [(rgb0, dist0, acc0, w0, t0), (rgb1, dist1, acc1, w1, t1)]


@pytest.mark.parametrize("kind", ["trained1", "trained3", "zero", "slab"])
@pytest.mark.parametrize("B,N", [(67, 64), (130, 128)])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_forward_with_a_pyramid_is_the_per_stage_composition(precision, B, N, kind):
    from mipnerf_pl_amd import Rays
    _, all_rays = C3.ray_set(C3.FRAME_SET)
    rays = Rays(*[t[200:200 + B].contiguous() for t in all_rays])
    model = C3.model360(precision, N)
    grid = _pyramid(kind, precision)
    ctx = model.mlp.native(torch.device(DEV))
    try:
        for white in (True, False):
            with torch.no_grad():
                want = _composition(model, grid, rays, white)
            bg = 1.0 if white else 0.0
            assert torch.equal(want[0][0], (bg * (1.0 - want[0][2]))[:, None].expand(-1, 3))       # level 0: the pyramid's silhouette
            if kind == "zero":
                assert bool((want[0][2] == 0).all()) and bool((want[0][3] == 0).all())
            else:
                assert bool((want[0][2] > 0).any())
            for fuse_small in (1, 0):                      # the small-launch fusion of the native forward: this route does not depend on it
                ctx.set_option(4, fuse_small)
                with torch.no_grad():
                    got = model._forward_native(rays, False, white, proposal=grid)
                for lvl in range(2):
                    for name, a, b in zip(G.NAMES, got[lvl], want[lvl]):
                        assert torch.equal(a, b), (white, fuse_small, lvl, name, G.maxdiff(a, b))
    finally:
        ctx.set_option(4, 1)
    with torch.no_grad():
        two = model._forward_native(rays, False, True)
    if kind != "trained1":
        assert not torch.equal(two[1][4], got[1][4])                                           # not the two-level forward
    assert torch.equal(two[0][4], got[0][4])                                                   # the coarse fence posts are the same
    if kind == "slab" and (B, N) == (67, 64):                                                   # randomized once, with given draws
        gen = torch.Generator(device=DEV).manual_seed(5)
        t_rand, u_rand = (torch.rand(B, N + 1, device=DEV, generator=gen) for _ in range(2))
        with torch.no_grad():
            want = _composition(model, grid, rays, True, t_rand, u_rand)
            got = model._forward_native(rays, True, True, t_rand=t_rand, u_rand=u_rand, proposal=grid)
        for lvl in range(2):
            for name, a, b in zip(G.NAMES, got[lvl], want[lvl]):
                assert torch.equal(a, b), ("randomized", lvl, name, G.maxdiff(a, b))


# ---- 6. frames -------------------------------------------------------------------------------------------------------------------------
def _chunked(model, rays, chunk, white, proposal=None):
    from mipnerf_pl_amd import Rays
    parts = []
    for lo in range(0, rays.origins.shape[0], chunk):
        with torch.no_grad():
            kw = {} if proposal is None else {"proposal": proposal}
            parts.append(model._forward_native(Rays(*[t[lo:lo + chunk].contiguous() for t in rays]), False, white, **kw))
    return [torch.cat([p[lvl][k] for p in parts]) for lvl in range(2) for k in range(3)]


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_frames_with_a_pyramid_eager_chunked_and_culled(precision):
    """the 1000 golden rays in 300-ray chunks (a ragged tail)"""
    from mipnerf_pl_amd import ops
    from mipnerf_pl_amd.model import CulledFrame, GraphedFrame
    _, rays = C3.ray_set(C3.FRAME_SET)
    n, chunk, dev = 1000, 300, torch.device(DEV)
    model = C3.model360(precision)
    grid, other = _pyramid("trained3", precision), _pyramid("slab", precision)
    with pytest.warns(UserWarning, match="not captured"):
        asked = GraphedFrame(model, n, chunk, True, dev, proposal=grid)                  # capture asked for: such a frame never captures
    eager = GraphedFrame(model, n, chunk, True, dev, capture=False, proposal=grid)
    with torch.no_grad():
        asked(rays)
        eager(rays)
    assert asked.graph is False and eager.graph is False
    want = _chunked(model, rays, chunk, True, grid)
    for a, b, c in zip(C3._outputs(asked), C3._outputs(eager), want):
        assert torch.equal(a, c) and torch.equal(b, c)
    assert torch.equal(eager.rgb[0], (1.0 - eager.acc[0])[:, None].expand(-1, 3))
    # another grid object: the frame follows
    asked.proposal = other
    with torch.no_grad():
        asked(rays)
    assert all(torch.equal(a, b) for a, b in zip(C3._outputs(asked), _chunked(model, rays, chunk, True, other)))
    # without the keyword: the route of before, _forward_native without `proposal`
    plain = GraphedFrame(model, n, chunk, True, dev, capture=False)
    with torch.no_grad():
        plain(rays)
    assert all(torch.equal(a, b) for a, b in zip(C3._outputs(plain), _chunked(model, rays, chunk, True)))
    assert not torch.equal(plain.rgb[-1], eager.rgb[-1])
    # culled, with the contracted occupancy: live pixels are GraphedFrame(proposal=)'s on the same (tightened) rays
    occ = C3.frame_occupancy(C3.FRAME_THRESHOLD)
    culled = CulledFrame(model, n, chunk, True, dev, occ, proposal=grid)
    with torch.no_grad():
        culled(rays)
    live = culled.live.bool()
    assert 0 < culled.live_count < n
    for a, b in zip(C3._outputs(culled), want):
        assert torch.equal(a[live], b[live])
    _, _, _, near, far = ops.ray_span(occ, rays, model.num_samples)
    tight = CulledFrame(model, n, chunk, True, dev, occ, tighten=True, proposal=grid)
    with torch.no_grad():
        eager(rays._replace(near=near, far=far))
        want_tight = C3._outputs(eager)
        tight(rays)
    for a, b in zip(C3._outputs(tight), want_tight):
        assert torch.equal(a[live], b[live])
    # the setter dispatches too
    culled.proposal = other
    with pytest.raises(NotImplementedError, match="unbounded"):
        culled.proposal = ops.ProposalGrid(torch.zeros(4, 4, 4, device=DEV), -2.0, 2.0)


# ---- 7. refusals of the routes ---------------------------------------------------------------------------------------------------------
def test_mismatched_models_and_grids_are_refused_by_every_route():
    from mipnerf_pl_amd import MipNerf, Rays, ops
    from mipnerf_pl_amd.model import CulledFrame, GraphedFrame
    _, all_rays = C3.ray_set(C3.FRAME_SET)
    rays = Rays(*[t[:8].contiguous() for t in all_rays])
    dev = torch.device(DEV)
    g360 = _pyramid("zero")
    bounded = C3._bounded_model()
    occ_world = ops.field_occupancy(bounded, grid=8, lo=-2.0, hi=2.0, threshold=0.5, dilate=0)
    with pytest.raises(NotImplementedError, match="bounded"):
        bounded._forward_native(rays, False, True, proposal=g360)
    with pytest.raises(NotImplementedError, match="bounded"):
        GraphedFrame(bounded, 8, 8, True, dev, proposal=g360)
    with pytest.raises(NotImplementedError, match="bounded"):
        CulledFrame(bounded, 8, 8, True, dev, occ_world, proposal=g360)
    one_level = MipNerf(num_samples=16, num_levels=1, unbounded=True, precision="fp32").to(DEV).eval()
    with pytest.raises(NotImplementedError, match="two-level"):
        one_level._forward_native(rays, False, True, proposal=g360)
    unb = C3.model360("fp32")
    world = ops.ProposalGrid(torch.zeros(4, 4, 4, device=DEV), -2.0, 2.0)
    with pytest.raises(NotImplementedError, match="unbounded"):
        unb._forward_native(rays, False, True, proposal=world)
    with pytest.raises(NotImplementedError, match="unbounded"):
        GraphedFrame(unb, 8, 8, True, dev, proposal=world)


# ---- 8. both command lines -------------------------------------------------------------------------------------------------------------
def test_eval_and_render_video_with_proposal_space_contracted(tmp_path, capsys):
    from dataset_fixture import write_blender
    from mipnerf_pl_amd import eval as eval_cli
    from mipnerf_pl_amd import render_video
    data = write_blender(str(tmp_path / "data"), seed=6, counts=(("test", 2),), w=16, h=16)
    ckpt = str(tmp_path / "last.ckpt")
    C3._system360().save_checkpoint(ckpt)
    prop = ["--proposal_grid", "16", "--proposal_space", "contracted", "--proposal_levels", "2"]
    cull = ["--cull", "--cull_space", "contracted", "--cull_grid", "24"]
    line = "proposal: 16^3 x 2 levels contracted density lattice over +-2.0000, far radius "
    ev = ["--ckpt", ckpt, "--data", data, "--scale", "1", "--save_image", "--chunk_size", "100", "--precision", "fp32", "--base_size", "16", "16"]
    rv = ["--ckpt", ckpt, "--scale", "1", "--n_poses", "2", "--chunk_size", "100", "--precision", "fp32", "--base_size", "16", "16"]
    for main, common, tag in ((eval_cli.main, ev, "eval"), (render_video.main, rv, "video")):
        plain, with_prop, with_cull = (str(tmp_path / f"{tag}_{k}") for k in ("plain", "prop", "cull"))
        main(common + ["--out_dir", plain])
        assert "proposal:" not in capsys.readouterr().out
        main(common + ["--out_dir", with_prop] + prop)
        text = capsys.readouterr().out
        assert text.count("proposal:") == 1 and text.count(line) == 1 and "built in" in text
        fp, fq = C3._files(plain), C3._files(with_prop)
        assert fp.keys() == fq.keys() and sum(k.endswith("_rgb.png") for k in fq) >= 2
        assert any(fp[k] != fq[k] for k in fp)                                          # not the two-level frames
        main(common + ["--out_dir", with_cull] + prop + cull + ["--proposal_far_radius", "40", "--proposal_footprint", "0.5"])
        text = capsys.readouterr().out
        assert text.count("proposal:") == 1 and "far radius 40.0000" in text and "cull: occupied share" in text
        assert C3._files(with_cull).keys() == fp.keys()
        with pytest.raises(SystemExit, match="--proposal_grid.*captured scene.*blender.*--proposal_space contracted"):
            main(common + ["--out_dir", str(tmp_path / f"{tag}_refused"), "--proposal_grid", "16"])
        assert not os.path.exists(str(tmp_path / f"{tag}_refused"))
