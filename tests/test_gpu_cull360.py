"""GPU: empty-space skipping for the unbounded-scene model in the contracted space (csrc/kernels_occupancy.hip k_ray_occupancy_360 /
k_ray_span_360, ops.ray_occupancy / ops.ray_span on an `Occupancy(space='contracted')`, model.CulledFrame on MipNerf(unbounded=True), and
--cull --cull_space contracted on both command lines).

  - every ray's class between the float64 fixture's must-live and may-live sets (tests/cull360_fixture.py, every box shrunk / grown by a
    margin of h), the rays the margin leaves undecided capped at 0.5 % of the set; two runs give the same bytes;
  - the span: liveness byte for byte that of ops.ray_occupancy, near' / far' torch.equal to the sampler's own inverse-depth fence posts,
    first / last equal to the fixture wherever its must and may spans agree (at least 99 % of the rays);
  - edge rays: N = 1, 63, 64, 65, 1024, a NaN origin, a ray from inside the unit ball to far = 1e4, a ray through the centre, zero rays,
    a box smaller than [-2, 2]^3 with outside_occupied on and off;
  - an analytic sphere from first principles in the contracted space;
  - frames of the trained field: live rays torch.equal to the un-culled renderer, dead rays background, all-occupied = the full frame,
    nothing-occupied = background, a tightened frame torch.equal to the renderer on the tightened rays;
  - both command lines on a 16 x 16 unbounded checkpoint.

Margin.  The device evaluates the rule in fp32: tests/test_cull360_cpu.py holds the same source to 16 fp32 ulps of 2 = 3.8e-6 on every
bound (measured up to 6.2), which is 6e-5 h on the 64^3 grid over +-2 (h = 0.0635) and 1.3e-4 h on the finest axis used here (70 points).
MARGIN = 1e-3 h is eight times that."""
import os

import numpy as np
import pytest
import torch

import cull360_fixture as cx
import gpu_util as G
import occupancy_fixture as fx

pytestmark = pytest.mark.gpu
DEV = G.DEV
LO, HI = (-2.0,) * 3, (2.0,) * 3
MARGIN = 1e-3
UNDECIDED_CAP = 0.005
SPAN_SKIPPED_CAP = 0.01
# (dims, centre, R, dilate): spheres in contracted coordinates, lattice value R - |z - centre|, threshold 0
LATTICES = {
    "s64": ((64, 64, 64), (0.3, -0.2, 0.25), 0.6, 0),
    "s64-dilate1": ((64, 64, 64), (0.3, -0.2, 0.25), 0.6, 1),
    "s45x23x70": ((45, 23, 70), (1.2, 0.4, -0.9), 0.5, 0),
}
RAY_SETS = ("scene360_rays/6", "full360_1000x96")
CONFIGS = [(rs, lat, N) for rs in RAY_SETS for lat in LATTICES for N in (64, 128)]
_CACHE = {}


def _ids(c):
    return f"{c[0]}-{c[1]}-N{c[2]}"


def ray_set(name):
    """(numpy dict in the golden files' layout, device Rays)"""
    if name not in _CACHE:
        if name == "scene360_rays/6":
            g = G.load_golden("scene360_rays")
            g = {k: np.ascontiguousarray(g[k][::6]) for k in g if k.startswith("rays_")}
            assert len(g["rays_origins"]) == 9035
        else:
            g = G.load_golden(name)
            g = {k: g[k] for k in g if k.startswith("rays_")}
        _CACHE[name] = (g, G.to_dev(G.rays_of(g)))
    return _CACHE[name]


def sphere_lattice(dims, centre, R):
    """fp32 [nz, ny, nx]: R - |z - centre| on the lattice points lo + float32(i) * h of the header"""
    ax = [np.float32(LO[a]) + np.arange(dims[a]).astype(np.float32) * ((np.float32(HI[a]) - np.float32(LO[a])) / np.float32(dims[a] - 1))
          for a in range(3)]
    z, y, x = np.meshgrid(ax[2].astype(np.float64), ax[1].astype(np.float64), ax[0].astype(np.float64), indexing="ij")
    return (R - np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2)).astype(np.float32)


def sphere_occupancy(tag):
    from mipnerf_pl_amd import ops
    if ("occ", tag) not in _CACHE:
        dims, centre, R, dilate = LATTICES[tag]
        occ = ops.occupancy_grid(torch.from_numpy(sphere_lattice(dims, centre, R)).to(DEV), 0.0, LO, HI, dilate=dilate)
        occ = ops.Occupancy(occ.bits, occ.dims, occ.lo, occ.hi, space="contracted")
        _CACHE[("occ", tag)] = (occ, fx.unpack(occ.bits.cpu().numpy(), dims[0] - 1))
    return _CACHE[("occ", tag)]


def _fixture_args(occ_bool, dims, g, N):
    return (occ_bool, dims, LO, HI, g["rays_origins"], g["rays_directions"], g["rays_radii"], g["rays_near"], g["rays_far"], N)


def evaluated(cfg):
    """device results and fixture spans of one configuration, computed once and shared by the tests below"""
    if cfg not in _CACHE:
        from mipnerf_pl_amd import ops
        rs, tag, N = cfg
        occ, occ_bool = sphere_occupancy(tag)
        g, rays = ray_set(rs)
        live = ops.ray_occupancy(occ, rays, N)
        span = ops.ray_span(occ, rays, N)
        args = _fixture_args(occ_bool, LATTICES[tag][0], g, N)
        must, may = (cx.span(*args, margin=m) for m in (-MARGIN, MARGIN))
        _CACHE[cfg] = dict(occ=occ, rays=rays, g=g, N=N, live=live, span=span, must=must, may=may)
    return _CACHE[cfg]


# ---- 1. classification between must-live and may-live -------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", CONFIGS, ids=_ids)
def test_every_ray_lies_between_the_must_live_and_may_live_sets(cfg):
    from mipnerf_pl_amd import ops
    r = evaluated(cfg)
    live = r["live"].cpu().numpy().astype(bool)
    must, may = r["must"][0], r["may"][0]
    n = len(live)
    assert r["live"].dtype == torch.uint8 and live.shape == must.shape == (n,)
    undecided = int((may & ~must).sum())
    print(f"cull360 classes {_ids(cfg)}: live {live.mean():.4f}, must {must.mean():.4f}, may {may.mean():.4f}, undecided {undecided} of {n}")
    G.record(f"cull360 classes {_ids(cfg)}", live_share=float(live.mean()), undecided=undecided, rays=n)
    assert not (must & ~may).any()
    assert undecided <= UNDECIDED_CAP * n, "the inputs leave too many rays undecided for the bracket to mean much"
    assert not (must & ~live).any(), int((must & ~live).sum())
    assert not (live & ~may).any(), int((live & ~may).sum())
    assert 0 < int(live.sum()) < n                                                      # both classes are there
    again = ops.ray_occupancy(r["occ"], r["rays"], r["N"], out=torch.full_like(r["live"], 7))
    assert torch.equal(again, r["live"])                                               # two runs, the same bytes
    # a grid in the contracted space takes no disparity flag
    with pytest.raises(ValueError, match="disparity"):
        ops.ray_occupancy(r["occ"], r["rays"], r["N"], disparity=True)


# ---- 2. the span ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", CONFIGS, ids=_ids)
def test_span_against_the_sampler_and_the_fixture(cfg):
    from mipnerf_pl_amd import ops
    r = evaluated(cfg)
    rays, N = r["rays"], r["N"]
    live, first, last, near, far = r["span"]
    assert live.dtype == torch.uint8 and torch.equal(live, r["live"])                  # byte for byte ops.ray_occupancy
    assert first.dtype == last.dtype == torch.int32 and near.shape == rays.near.shape and far.shape == rays.far.shape
    lv = live.bool()
    # the fence posts themselves
    _, t = ops.sample_t_360(N, rays.near, rays.far, False)
    assert torch.equal(near[lv], t.gather(1, first.long().clamp(0, N)[:, None])[lv])
    assert torch.equal(far[lv], t.gather(1, (last.long() + 1).clamp(0, N)[:, None])[lv])
    assert (near[lv] < far[lv]).all()
    # a dead ray
    assert (first[~lv] == N).all() and (last[~lv] == -1).all()
    assert torch.equal(near[~lv], rays.near[~lv]) and torch.equal(far[~lv], rays.far[~lv])
    # first / last are the fixture's wherever its must and may spans agree
    (_, first_must, last_must), (_, first_may, last_may) = r["must"], r["may"]
    fi, la = first.cpu().numpy().astype(np.int64), last.cpu().numpy().astype(np.int64)
    agree = (first_must == first_may) & (last_must == last_may)
    skipped = float(1.0 - agree.mean())
    print(f"cull360 span {_ids(cfg)}: {int((~agree).sum())} of {len(agree)} rays skipped ({skipped:.4%})")
    G.record(f"cull360 span {_ids(cfg)}", skipped_share=skipped)
    assert skipped <= SPAN_SKIPPED_CAP
    assert np.array_equal(fi[agree], first_must[agree]) and np.array_equal(la[agree], last_must[agree])
    # and between them everywhere
    assert ((first_may <= fi) & (fi <= first_must)).all() and ((last_must <= la) & (la <= last_may)).all()
    # the skipped outputs change nothing, and two runs give the same bytes
    only = ops.ray_span(r["occ"], rays, N, out=(torch.empty_like(live), None, None, None, None))
    assert torch.equal(only[0], live) and only[1:] == (None, None, None, None)
    again = ops.ray_span(r["occ"], rays, N)
    assert all(torch.equal(a, b) for a, b in zip(again, r["span"]))


# ---- 3. edge rays --------------------------------------------------------------------------------------------------------------------
def _edge_rays():
    """0: a NaN origin; 1: from inside the unit ball outwards; 2: through the centre from outside; 3 .. : a fan from (0, -3, 0.5) across and
    past the s64 sphere; every ray with near 0.05 and far 1e4 except the fan (near 0.5, far 30).  numpy dict and device Rays."""
    fan = 9
    o = np.array([[np.nan, 0.2, 0.1], [0.2, -0.1, 0.1], [2.0, 1.0, -1.5]] + [[0.0, -3.0, 0.5]] * fan, np.float64)
    d = np.array([[0.0, 0.6, 0.8], [0.48, 0.6, 0.64], [-2.0, -1.0, 1.5]] + [[x, 1.0, -0.1] for x in np.linspace(-0.9, 0.9, fan)], np.float64)
    d[2] /= np.linalg.norm(d[2])
    n = len(o)
    near = np.array([0.05] * 3 + [0.5] * fan)[:, None]
    far = np.array([1e4] * 3 + [30.0] * fan)[:, None]
    one = np.ones((n, 1))
    g = {"rays_" + k: np.ascontiguousarray(v, np.float32) for k, v in zip(("origins", "directions", "viewdirs", "radii", "lossmult", "near", "far"),
                                                                           (o, d, d, 5e-3 * one, one, near, far))}
    return g, G.to_dev(G.rays_of(g))


@pytest.mark.parametrize("N", [1, 63, 64, 65, 1024])
def test_edge_rays(N):
    from mipnerf_pl_amd import Rays, ops
    g, rays = _edge_rays()
    occ, occ_bool = sphere_occupancy("s64")
    dims = LATTICES["s64"][0]
    live, first, last, near, far = ops.ray_span(occ, rays, N)
    assert torch.equal(live, ops.ray_occupancy(occ, rays, N))
    lv = live.cpu().numpy().astype(bool)
    args = _fixture_args(occ_bool, dims, g, N)
    (must, f_must, l_must), (may, f_may, l_may) = (cx.span(*args, margin=m) for m in (-MARGIN, MARGIN))
    assert not (must & ~lv).any() and not (lv & ~may).any()
    fi, la = first.cpu().numpy().astype(np.int64), last.cpu().numpy().astype(np.int64)
    assert ((f_may <= fi) & (fi <= f_must)).all() and ((l_must <= la) & (la <= l_may)).all()
    # the NaN ray is live over all of [near, far]; the ray from inside the ball starts inside the sphere; the ray through the centre meets it
    assert lv[0] and fi[0] == 0 and la[0] == N - 1
    assert lv[1] and fi[1] == 0 and lv[2]
    if N >= 63:
        assert lv[3:].any() and not lv[3:].all()                                       # the fan has both classes
    _, t = ops.sample_t_360(N, rays.near, rays.far, False)
    ok = torch.from_numpy(lv).to(DEV)
    ok[0] = False                                                                      # NaN fence posts do not compare
    assert torch.equal(near[ok], t.gather(1, first.long().clamp(0, N)[:, None])[ok])
    assert torch.equal(far[ok], t.gather(1, (last.long() + 1).clamp(0, N)[:, None])[ok])
    dead = ~torch.from_numpy(lv).to(DEV)
    assert (first[dead] == N).all() and (last[dead] == -1).all()
    assert torch.equal(near[dead], rays.near[dead]) and torch.equal(far[dead], rays.far[dead])
    # zero rays
    none = Rays(*[t_[:0] for t_ in rays])
    out = ops.ray_span(occ, none, N)
    assert [t_.shape[0] for t_ in out] == [0] * 5 and ops.ray_occupancy(occ, none, N).shape == (0,)
    # a box smaller than [-2, 2]^3, nothing occupied in it: what leaves it counts as occupied, or is clipped away
    small = ops.Occupancy(torch.zeros(15, 15, 1, dtype=torch.int32, device=DEV).view(torch.uint32), (16, 16, 16), (-0.5,) * 3, (0.5,) * 3,
                          space="contracted")
    assert (ops.ray_occupancy(small, rays, N, outside_occupied=False) == 0).all()
    on = ops.ray_span(small, rays, N, outside_occupied=True)
    assert (on[0] == 1).all()                                                          # every ray here has a frustum that leaves +-0.5
    want = cx.span(np.zeros((15, 15, 15), bool), (16, 16, 16), (-0.5,) * 3, (0.5,) * 3, *_fixture_args(None, None, g, N)[4:], margin=0.0,
                   outside_occupied=True)
    both = [cx.span(np.zeros((15, 15, 15), bool), (16, 16, 16), (-0.5,) * 3, (0.5,) * 3, *_fixture_args(None, None, g, N)[4:], margin=m,
                    outside_occupied=True) for m in (-MARGIN, MARGIN)]
    same = (both[0][1] == both[1][1]) & (both[0][2] == both[1][2])
    assert same.sum() >= len(same) - 2
    assert np.array_equal(on[1].cpu().numpy()[same], want[1][same]) and np.array_equal(on[2].cpu().numpy()[same], want[2][same])
    # all of the small box occupied: the same rays are live with the outside clipped away exactly when they pass through it
    full = ops.Occupancy((~small.bits.view(torch.int32) & 0x7FFF).view(torch.uint32), small.dims, small.lo, small.hi, space="contracted")
    inside = ops.ray_occupancy(full, rays, N, outside_occupied=False).cpu().numpy().astype(bool)
    must_in, may_in = (cx.classify(np.ones((15, 15, 15), bool), (16, 16, 16), (-0.5,) * 3, (0.5,) * 3, *_fixture_args(None, None, g, N)[4:], margin=m,
                                   outside_occupied=False) for m in (-MARGIN, MARGIN))
    assert not (must_in & ~inside).any() and not (inside & ~may_in).any() and inside[1]


# ---- 4. an analytic sphere from first principles ---------------------------------------------------------------------------------------
def _box_reach(t0, t1, o, d, radii, cone_scale):
    """[n, N]: an upper bound, from the stated form of the rule alone, on the distance between contract(p0) and any point of the frustum's
    box.  Case rmin >= 1: a box coordinate is u' f' with u' in [ulo_a, uhi_a] and f' in [flo, fhi], and contract(p0)_a = u0_a f0 with f0 in
    [flo, fhi], so they differ by at most fhi (|u1_a - u0_a| + e) + (fhi - flo).  Otherwise a box coordinate lies in the hull of the world
    interval W_a = [xlo_a, xhi_a] and slo W_a: within |p1_a - p0_a| + rho + (1 - slo) m_a of p0_a, m_a = max(|xlo_a|, |xhi_a|), and
    contract(p0)_a within (1 - slo) m_a of p0_a."""
    t0, t1 = t0[..., None], t1[..., None]
    o, d = o[:, None, :], d[:, None, :]
    rho = cone_scale * radii.reshape(-1, 1, 1) * t1
    p0, p1 = o + t0 * d, o + t1 * d
    tc = np.clip(-(o * d).sum(-1, keepdims=True) / (d * d).sum(-1, keepdims=True), t0, t1)
    rc = np.linalg.norm(o + tc * d, axis=-1, keepdims=True)
    n0, n1 = np.linalg.norm(p0, axis=-1, keepdims=True), np.linalg.norm(p1, axis=-1, keepdims=True)
    rmin, rmax = rc - rho, np.maximum(n0, n1) + rho
    with np.errstate(divide="ignore", invalid="ignore"):
        u0, u1 = p0 / n0, p1 / n1
        e = 1.0 - np.sqrt(np.maximum(0.0, (1.0 + (u0 * u1).sum(-1, keepdims=True)) / 2.0)) + rho / rmin
        flo, fhi = 2.0 - 1.0 / rmin, 2.0 - 1.0 / rmax
        out = fhi * (np.abs(u1 - u0) + e) + (fhi - flo)
    slo = np.where(rmax > 1, (2.0 - 1.0 / rmax) / rmax, 1.0)
    m = np.maximum(np.abs(np.minimum(p0, p1) - rho), np.abs(np.maximum(p0, p1) + rho))
    mixed = np.abs(p1 - p0) + rho + 2.0 * (1.0 - slo) * m
    return np.linalg.norm(np.where(rmin >= 1.0, out, mixed), axis=-1), cx.contract(p0)


@pytest.mark.parametrize("dilate", [0, 1])
@pytest.mark.parametrize("cone_scale", [1.0, 8.0])
def test_analytic_sphere_from_first_principles_in_contracted_space(dilate, cone_scale):
    """The (64, 64, 64) lattice, a sphere of radius R around c in contracted coordinates, threshold 0; the argument of
    test_gpu_occupancy.test_analytic_sphere_from_first_principles.  Dead: an occupied cell has a corner inside the sphere or lies `dilate`
    cells from one that has, so all of it is within R + (1 + dilate) h sqrt(3) of c; a cell in a frustum's range holds a point of its box,
    and no point of the box is farther than `_box_reach` from contract(p0): a ray with |contract(p0_i) - c| > R + reach_i + (2 + dilate) h
    sqrt(3) for every frustum touches no occupied cell (one diagonal is slack for fp32).  Live: a ray with a point p on its axis, near <= t
    <= far, whose image z = contract(p) is within R - h sqrt(3) of c: every corner of z's cell is within h sqrt(3) of z, hence inside the
    sphere, the cell is occupied, and z lies in the box of the frustum that holds p -- the rule is conservative (tests/test_cull360_cpu.py).
    The sphere lies in |z| < 1.05, where contraction is the identity or nearly so.  outside_occupied=False, as there."""
    from mipnerf_pl_amd import ops
    tag = "s64" if dilate == 0 else "s64-dilate1"
    dims, centre, R, _ = LATTICES[tag]
    centre = np.asarray(centre)
    occ, _ = sphere_occupancy(tag)
    g, rays = ray_set(RAY_SETS[0])
    N = 128
    h = 4.0 / 63
    live = ops.ray_occupancy(occ, rays, N, cone_scale=cone_scale, outside_occupied=False).cpu().numpy().astype(bool)
    o, d = g["rays_origins"].astype(np.float64), g["rays_directions"].astype(np.float64)
    t = cx.fence_posts(g["rays_near"], g["rays_far"], N)
    reach, z0 = _box_reach(t[:, :-1], t[:, 1:], o, d, g["rays_radii"].astype(np.float64), cone_scale)
    gap = np.linalg.norm(z0 - centre, axis=-1) - reach                                   # [n, N]
    surely_dead = (gap > R + (2 + dilate) * h * np.sqrt(3)).all(axis=1)
    # axis points: the fence posts, their midpoints and the point of the segment nearest c in world coordinates
    tc = np.clip(((centre - o) * d).sum(-1) / (d * d).sum(-1), t[:, 0], t[:, -1])[:, None]
    ts = np.concatenate([t, 0.5 * (t[:, 1:] + t[:, :-1]), tc], axis=1)
    z = cx.contract(o[:, None, :] + ts[..., None] * d[:, None, :])
    surely_live = (np.linalg.norm(z - centre, axis=-1) < R - h * np.sqrt(3)).any(axis=1)
    print(f"cull360 analytic sphere dilate {dilate} cone_scale {cone_scale}: surely dead {surely_dead.mean():.4f}, surely live "
          f"{surely_live.mean():.4f}, live {live.mean():.4f}")
    assert surely_dead.mean() > 0.03 and surely_live.mean() > 0.02, (surely_dead.mean(), surely_live.mean())     # hundreds of the 9035 rays each
    assert not live[surely_dead].any() and live[surely_live].all()


# ---- 5. frames of the trained field ---------------------------------------------------------------------------------------------------
FRAME_SET = "full360_1000x96"
FRAME_GRID = 64
FRAME_THRESHOLD = 0.5
FRAME_DILATE = 1


def field360():
    f = G.load_golden("trained_field_360")
    return {k[2:]: f[k] for k in f if k.startswith("p_")}


def model360(precision, num_samples=96):
    key = ("model", precision, num_samples)
    if key not in _CACHE:
        from mipnerf_pl_amd import MipNerf
        m = MipNerf(num_samples=num_samples, unbounded=True, precision=precision, density_bias=float(G.load_golden(FRAME_SET)["density_bias"]))
        m.load_state_dict({"mlp." + k: torch.from_numpy(v.copy()) for k, v in field360().items()}, strict=True)
        _CACHE[key] = m.to(DEV).eval()
    return _CACHE[key]


def frame_far_radius():
    g, _ = ray_set(FRAME_SET)
    reach = np.linalg.norm(g["rays_origins"].astype(np.float64) + g["rays_far"].astype(np.float64) * g["rays_directions"].astype(np.float64), axis=1)
    return float(reach.max()) * (FRAME_GRID - 1) / (FRAME_GRID - 3)


def frame_occupancy(threshold):
    """the fp32 field's grid: one grid for both precisions, so that their live sets are the same"""
    from mipnerf_pl_amd import ops
    key = ("frame_occ", threshold)
    if key not in _CACHE:
        _CACHE[key] = ops.field_occupancy(model360("fp32"), grid=FRAME_GRID, threshold=threshold, dilate=FRAME_DILATE, space="contracted",
                                          far_radius=frame_far_radius(), precision="fp32")
    return _CACHE[key]


def _outputs(frame):
    return [t.clone() for lv in range(len(frame.rgb)) for t in (frame.rgb[lv], frame.dist[lv], frame.acc[lv])]


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_frames_of_the_trained_field(precision):
    """trained_field_360 on the 1000 golden rays, chunk 300 (a ragged tail), a 64^3 grid over [-2, 2]^3 of the contracted space, dilate 1,
    far radius = the largest |o + far d| of the rays times 63 / 61.
    The threshold.  Nobody had measured this field's densities on a lattice.  `scripts/cull360_rate.py --step sweep` measured, on one
    MI355X, the culled share of these 1000 rays on this grid over the thresholds 0.01 .. 30 (profiles/cull360_rate.json keeps the sweep):
    0.005 at 0.01, 0.023 at 0.1, 0.068 at 0.3, 0.130 at 0.5, 0.259 at 1, 0.437 at 2, 0.749 at 5, 0.985 at 10 (the field is foggy: its
    largest lattice density is 10.7).  FRAME_THRESHOLD = 0.5 is the smallest value of the sweep whose share clears the lower end of
    [0.05, 0.9] with room to spare -- the least aggressive culling that still exercises both classes; the share it gives is recorded
    (G.record) and asserted to lie in that range.  At this threshold the accumulation bound 1 - exp(-threshold (far - near) |d|) is loose
    on rays this long ((far - near) |d| >= 15): measured, the culled rays' golden acc reaches 0.83 against a smallest bound of 0.9999."""
    from mipnerf_pl_amd import ops
    from mipnerf_pl_amd.model import CulledFrame, GraphedFrame
    gold = G.load_golden(FRAME_SET)
    g, rays = ray_set(FRAME_SET)
    n, N, chunk = int(gold["batch"]), int(gold["num_samples"]), 300
    assert n == 1000 and N == 96
    model = model360(precision)
    dev = torch.device(DEV)
    occ = frame_occupancy(FRAME_THRESHOLD)
    assert occ.space == "contracted" and occ.dims == (FRAME_GRID,) * 3 and occ.lo == LO and occ.hi == HI
    plain = GraphedFrame(model, n, chunk, True, dev, capture=False)
    culled = CulledFrame(model, n, chunk, True, dev, occ)
    with torch.no_grad():
        plain(rays)
        want = _outputs(plain)
        c_rgb, f_rgb, dist = culled(rays)
    got = _outputs(culled)
    live = culled.live.bool()
    share = 1.0 - culled.live_count / float(n)
    print(f"cull360 frame {precision}: threshold {FRAME_THRESHOLD}, occupied share {occ.occupied_fraction():.4f}, culled share {share:.4f}")
    G.record(f"cull360 frame {precision}", threshold=FRAME_THRESHOLD, culled_share=share, occupied_share=occ.occupied_fraction(),
             far_radius=frame_far_radius())
    assert torch.equal(culled.live, ops.ray_occupancy(occ, rays, N)) and culled.live_count == int(live.sum())
    assert 0.05 <= share <= 0.9
    assert c_rgb is culled.rgb[0] and f_rgb is culled.rgb[-1] and dist is culled.dist[-1]
    for a, b in zip(got, want):                                                        # live rays: the renderer's bits
        assert torch.equal(a[live], b[live])
    for l_ in range(2):                                                                # dead rays: background, acc 0, near
        assert (culled.rgb[l_][~live] == 1.0).all() and (culled.acc[l_][~live] == 0.0).all()
        assert torch.equal(culled.dist[l_][~live], rays.near[~live, 0])
    # what a culled ray could have accumulated: its density stays at or below the threshold along [near, far]
    dead = ~live.cpu().numpy()
    length = (g["rays_far"] - g["rays_near"])[:, 0].astype(np.float64) * np.linalg.norm(g["rays_directions"].astype(np.float64), axis=1)
    bound = 1.0 - np.exp(-FRAME_THRESHOLD * length)
    for key in ("l0_acc", "l1_acc"):
        acc = gold[key].astype(np.float64)
        print(f"cull360 frame {precision}: max golden {key} over the culled rays {acc[dead].max():.4f}, smallest bound {bound[dead].min():.4f}")
        assert (acc[dead] <= bound[dead]).all(), (key, float((acc[dead] - bound[dead]).max()))
    # all occupied: the full frame; nothing occupied: background
    everything = CulledFrame(model, n, chunk, True, dev, frame_occupancy(-1.0))
    nothing = CulledFrame(model, n, chunk, True, dev, frame_occupancy(1e9))
    with torch.no_grad():
        everything(rays)
        nothing(rays)
    assert everything.live_count == n and all(torch.equal(a, b) for a, b in zip(_outputs(everything), want))
    assert nothing.live_count == 0 and (nothing.rgb[-1] == 1.0).all() and (nothing.acc[-1] == 0.0).all()
    assert torch.equal(nothing.dist[-1], rays.near[:, 0])
    # tightened: the renderer on the rays with near' / far'
    _, first, last, near, far = ops.ray_span(occ, rays, N)
    tight = CulledFrame(model, n, chunk, True, dev, occ, tighten=True)
    with torch.no_grad():
        plain(rays._replace(near=near, far=far))
        want_tight = _outputs(plain)
        tight(rays)
    assert torch.equal(tight.live, culled.live) and torch.equal(tight.first, first) and torch.equal(tight.last, last)
    assert torch.equal(tight.near_span, near) and torch.equal(tight.far_span, far)
    for a, b in zip(_outputs(tight), want_tight):
        assert torch.equal(a[live], b[live])
    for l_ in range(2):
        assert (tight.rgb[l_][~live] == 1.0).all() and torch.equal(tight.dist[l_][~live], rays.near[~live, 0])
    assert (near[live] > rays.near[live]).any() or (far[live] < rays.far[live]).any()
    assert 0.0 < tight.span_share <= 1.0 and culled.span_share == pytest.approx(tight.span_share, abs=0.0)
    # a bounded model and this grid, this model and a world grid
    with pytest.raises(ValueError, match="contracted space"):
        CulledFrame(_bounded_model(), n, chunk, True, dev, occ)
    with pytest.raises(NotImplementedError, match="unbounded=True models are not supported"):
        CulledFrame(model, n, chunk, True, dev, ops.Occupancy(occ.bits, occ.dims, occ.lo, occ.hi))


def _bounded_model():
    from mipnerf_pl_amd import MipNerf
    return MipNerf(num_samples=32).to(DEV).eval()


# ---- 6. both command lines -------------------------------------------------------------------------------------------------------------
def _system360(num_samples=32):
    from mipnerf_pl_amd.system import DEFAULT_HPARAMS, MipNeRFSystem
    hp = dict(DEFAULT_HPARAMS)
    hp.update({"nerf.num_samples": num_samples, "nerf.unbounded": True, "nerf.density_bias": float(G.load_golden(FRAME_SET)["density_bias"]),
               "exp_name": "cli360", "val.batch_type": "single_image", "dataset_name": "blender"})
    system = MipNeRFSystem(hp, precision="fp32")
    missing, unexpected = system.load_state_dict({"mip_nerf.mlp." + k: torch.from_numpy(v.copy()) for k, v in field360().items()}, strict=True)
    assert not missing and not unexpected
    return system


def _files(root):
    out = {}
    for d, _, fs in os.walk(root):
        for f in fs:
            with open(os.path.join(d, f), "rb") as fh:
                out[os.path.relpath(os.path.join(d, f), root)] = fh.read()
    return out


def test_eval_command_line_with_cull_space_contracted(tmp_path, capsys):
    from dataset_fixture import write_blender
    from mipnerf_pl_amd import eval as eval_cli
    from PIL import Image
    data = write_blender(str(tmp_path / "data"), seed=6, counts=(("test", 2),), w=16, h=16)
    ckpt = str(tmp_path / "last.ckpt")
    _system360().save_checkpoint(ckpt)
    common = ["--ckpt", ckpt, "--data", data, "--scale", "1", "--save_image", "--chunk_size", "100", "--precision", "fp32", "--base_size", "16", "16"]
    plain, allocc, none = str(tmp_path / "plain"), str(tmp_path / "all"), str(tmp_path / "none")
    eval_cli.main(common + ["--out_dir", plain])
    assert "cull:" not in capsys.readouterr().out
    with pytest.raises(SystemExit, match=r"unbounded.*--cull_space contracted"):
        eval_cli.main(common + ["--out_dir", str(tmp_path / "refused"), "--cull"])
    assert not os.path.exists(str(tmp_path / "refused"))
    cull = ["--cull", "--cull_space", "contracted", "--cull_grid", "24"]
    # every density is > -1: the grid is all occupied, every ray live, every byte as without --cull
    eval_cli.main(common + ["--out_dir", allocc] + cull + ["--cull_threshold", "-1", "--cull_dilate", "0"])
    text = capsys.readouterr().out
    assert text.count("cull: occupied share of the 24^3 grid over +-2.0000 of the contracted space, far radius ") == 1 and "): 1.0000" in text
    assert "cull: mean live share per frame: 1.0000 (2 frames)" in text
    fp, fa = _files(plain), _files(allocc)
    assert fp.keys() == fa.keys() and len([k for k in fp if k.endswith(".png")]) >= 6
    assert all(fp[k] == fa[k] for k in fp), [k for k in fp if fp[k] != fa[k]]
    # nothing occupied: every ray culled, the same files, white frames; a far radius of the user's own is printed
    eval_cli.main(common + ["--out_dir", none] + cull + ["--cull_threshold", "1e9", "--cull_far_radius", "40"])
    text = capsys.readouterr().out
    assert "far radius 40.0000" in text and "): 0.0000" in text and "cull: mean live share per frame: 0.0000 (2 frames)" in text
    assert _files(none).keys() == fp.keys()
    assert (np.array(Image.open(os.path.join(none, "test", "cli360", "1", "00000_rgb.png"))) == 255).all()


def test_render_video_command_line_with_cull_space_contracted(tmp_path, capsys):
    from mipnerf_pl_amd import render_video
    from PIL import Image
    ckpt = str(tmp_path / "last.ckpt")
    _system360().save_checkpoint(ckpt)
    common = ["--ckpt", ckpt, "--scale", "1", "--n_poses", "2", "--chunk_size", "100", "--precision", "fp32", "--base_size", "16", "16"]
    plain, allocc, none = str(tmp_path / "plain"), str(tmp_path / "all"), str(tmp_path / "none")
    render_video.main(common + ["--out_dir", plain])
    assert "cull:" not in capsys.readouterr().out
    cull = ["--cull", "--cull_space", "contracted", "--cull_grid", "20"]
    render_video.main(common + ["--out_dir", allocc] + cull + ["--cull_threshold", "-1", "--cull_tighten"])
    text = capsys.readouterr().out
    assert text.count("cull: occupied share of the 20^3 grid over +-2.0000 of the contracted space, far radius ") == 1
    assert "cull: mean live share per frame: 1.0000 (2 frames); mean span share of the live rays: 1.0000" in text
    fp, fa = _files(plain), _files(allocc)
    assert fp.keys() == fa.keys() and sum(k.endswith("_rgb.png") for k in fp) == 2
    assert all(fp[k] == fa[k] for k in fp), [k for k in fp if fp[k] != fa[k]]          # near' = near and far' = far, bit for bit
    render_video.main(common + ["--out_dir", none] + cull + ["--cull_threshold", "1e9"])
    text = capsys.readouterr().out
    assert "cull: mean live share per frame: 0.0000 (2 frames)" in text
    assert (np.array(Image.open(os.path.join(none, "render_spheric", "cli360", "1", "00000_rgb.png"))) == 255).all()
    # a bounded checkpoint does not take the flag
    from mipnerf_pl_amd.system import DEFAULT_HPARAMS, MipNeRFSystem
    hp = dict(DEFAULT_HPARAMS)
    hp.update({"nerf.num_samples": 32, "exp_name": "cli", "val.batch_type": "single_image", "dataset_name": "blender"})
    bounded = str(tmp_path / "bounded.ckpt")
    MipNeRFSystem(hp, precision="fp32").save_checkpoint(bounded)
    with pytest.raises(SystemExit, match="bounded model"):
        render_video.main(["--ckpt", bounded, "--scale", "1", "--out_dir", str(tmp_path / "refused")] + cull)
    assert not os.path.exists(str(tmp_path / "refused"))
