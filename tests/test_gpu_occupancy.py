"""GPU: empty-space skipping for whole frames (csrc/kernels_occupancy.hip, model.CulledFrame).

  - occupancy bits, byte for byte against tests/occupancy_fixture.py, and the same bytes from two runs;
  - compaction and scatter, exact against numpy;
  - ray classification between the float64 brute force's must-live and may-live sets (bounding boxes shrunk / grown by 1e-3 h: the device's
    fp32 error on a coordinate is ~1e-6 against that margin of ~6e-5), and against analytic spheres from first principles;
  - CulledFrame: live rays bit for bit those of GraphedFrame, culled rays provably near-empty (a derived bound on the golden acc);
  - the whole 800 x 800 golden frame under the project's frame criteria, and both command lines.

The golden rays start at |o| = 4 and run to far = 6, so they leave the box +-2.0 the fixture field was examined in (coordinates up to 3.6):
on that box the classification runs with outside_occupied=False -- with it set every ray would be live and the tests vacuous -- and the
derived acc bound on every culled ray is what shows that nothing visible was dropped.  outside_occupied=True is tested on its own.
The fixture field is foggy (median density 4e-4, rising towards the box), which is why thresholds as high as 0.1 are used here."""
import os

import numpy as np
import pytest
import torch

import gpu_util as G
import occupancy_fixture as fx

pytestmark = pytest.mark.gpu
DEV = G.DEV
DIMS, LO, HI = (64, 64, 64), (-2.0,) * 3, (2.0,) * 3
RAY_SETS = ("fulltrained_c4_8192x256", "fulltrained_c2_4096x128")
MARGIN = 1e-3
_CACHE = {}


def trained_params():
    f = G.load_golden("trained_field")
    return {k[2:]: f[k] for k in f if k.startswith("p_")}


def trained_lattice():
    """the device's own lattice of the trained field, 64^3 over +-2.0, fp32: (device tensor, numpy copy)"""
    if "lattice" not in _CACHE:
        from mipnerf_pl_amd import ops
        model = G.make_model(trained_params(), 128, "fp32")
        sigma = ops.density_grid(model, DIMS, LO, HI)
        _CACHE["lattice"] = (sigma, sigma.cpu().numpy())
    return _CACHE["lattice"]


def golden_rays(name):
    if name not in _CACHE:
        g = G.load_golden(name)
        _CACHE[name] = (g, G.to_dev(G.rays_of(g)))
    return _CACHE[name]


def words_of(occ):
    return occ.bits.cpu().numpy()


def sphere_lattice(dims, lo, hi, centre, radius):
    """R - |x - c| on the lattice points (numpy float32 restatement of the lattice formulas): positive inside"""
    lo32, hi32 = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
    h = (hi32 - lo32) / (np.asarray(dims) - 1).astype(np.float32)
    axes = [lo32[a] + np.arange(dims[a]).astype(np.float32) * h[a] for a in range(3)]
    z, y, x = np.meshgrid(axes[2], axes[1], axes[0], indexing="ij")
    r = np.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2)
    return (np.float32(radius) - r).astype(np.float32)


# ---- bits --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [(64, 64, 64), (45, 23, 70), (20, 9, 7), (33, 4, 5), (34, 3, 3), (130, 5, 6), (2, 2, 2)])
@pytest.mark.parametrize("dilate", [0, 1, 3])
def test_sphere_bits_are_exact(dims, dilate):
    from mipnerf_pl_amd import ops
    lo, hi = (-1.0, -0.5, -1.5), (1.0, 1.0, 1.0)
    lat = sphere_lattice(dims, lo, hi, (0.1, 0.2, -0.3), 0.45)
    if dims[0] > 8:
        lat[0, 0, dims[0] - 2] = np.nan          # NaN is occupied; an isolated cell next to the row's end: the padding must stay 0
        lat[-1, -1, 0] = np.inf
    occ = ops.occupancy_grid(torch.from_numpy(lat).to(DEV), 0.0, lo, hi, dilate=dilate)
    assert occ.dims == dims and occ.bits.dtype == torch.uint32 and occ.bits.shape == (dims[2] - 1, dims[1] - 1, (dims[0] - 1 + 31) // 32)
    want = fx.occupancy_words(lat, 0.0, dilate)
    got = words_of(occ)
    assert got.tobytes() == want.tobytes()
    again = ops.occupancy_grid(torch.from_numpy(lat).to(DEV), 0.0, lo, hi, dilate=dilate)
    assert words_of(again).tobytes() == got.tobytes()
    cells = (dims[0] - 1) * (dims[1] - 1) * (dims[2] - 1)
    assert occ.occupied_fraction() == pytest.approx(fx.unpack(want, dims[0] - 1).sum() / cells, abs=1e-12)


def test_a_dilation_wider_than_a_word_is_exact():
    from mipnerf_pl_amd import ops
    lat = np.zeros((3, 3, 70), np.float32)
    lat[1, 1, 3] = 1.0
    lat[0, 0, 69] = 1.0
    for d in (33, 64, 100):
        occ = ops.occupancy_grid(torch.from_numpy(lat).to(DEV), 0.5, -1.0, 1.0, dilate=d)
        assert words_of(occ).tobytes() == fx.occupancy_words(lat, 0.5, d).tobytes(), d


@pytest.mark.parametrize("threshold,dilate", [(0.1, 0), (0.1, 1), (0.03, 0), (0.1, 3)])
def test_trained_field_bits_are_exact(threshold, dilate):
    from mipnerf_pl_amd import ops
    sigma, sigma_np = trained_lattice()
    occ = ops.occupancy_grid(sigma, threshold, LO, HI, dilate=dilate)
    want = fx.occupancy_words(sigma_np, threshold, dilate)
    assert words_of(occ).tobytes() == want.tobytes()
    assert words_of(ops.occupancy_grid(sigma, threshold, LO, HI, dilate=dilate)).tobytes() == want.tobytes()
    frac = occ.occupied_fraction()
    G.record(f"occupancy trained 64^3 thr {threshold} dilate {dilate}", occupied_fraction=frac)
    assert 0.05 < frac < 0.9
    # the convenience form is density_grid followed by occupancy_grid
    model = G.make_model(trained_params(), 128, "fp32")
    conv = ops.field_occupancy(model, grid=64, lo=-2.0, hi=2.0, threshold=threshold, dilate=dilate)
    assert words_of(conv).tobytes() == want.tobytes() and conv.dims == DIMS and conv.lo == LO and conv.hi == HI


def test_field_occupancy_refuses_the_unbounded_model_and_a_missing_box():
    from mipnerf_pl_amd import MipNerf, ops
    model = G.make_model(trained_params(), 128, "fp32")
    with pytest.raises(ValueError, match="box"):
        ops.field_occupancy(model, grid=16)
    with pytest.raises(NotImplementedError, match="unbounded=True models are not supported"):
        ops.field_occupancy(MipNerf(num_samples=32, unbounded=True), grid=16, lo=-1.0, hi=1.0)
    with pytest.raises(ValueError, match="dilate"):
        ops.occupancy_grid(torch.zeros(4, 4, 4, device=DEV), 0.5, -1.0, 1.0, dilate=-1)


# ---- compaction and scatter -----------------------------------------------------------------------------------------------------
def _random_rays(n, rng):
    from mipnerf_pl_amd import Rays
    return Rays(*[torch.from_numpy(rng.normal(size=(n, k)).astype(np.float32)).to(DEV) for k in (3, 3, 3, 1, 1, 1, 1)])


@pytest.mark.parametrize("n", [1, 3, 1000, 1024, 1025, 4097, 70001])
@pytest.mark.parametrize("kind", ["random", "sparse", "dead", "live"])
def test_compaction_and_scatter_are_exact(n, kind):
    from mipnerf_pl_amd import Rays, ops
    rng = np.random.default_rng(n)
    live_np = {"random": rng.random(n) < 0.4, "sparse": rng.random(n) < 0.01, "dead": np.zeros(n, bool), "live": np.ones(n, bool)}[kind]
    live_np = (live_np * rng.integers(1, 256, n)).astype(np.uint8)                     # any non-zero byte is live
    live = torch.from_numpy(live_np).to(DEV)
    rays = _random_rays(n, rng)
    out_rays = Rays(*[torch.full_like(t, -7.0) for t in rays])
    index = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    count = ops.compact_rays(live, rays, out_rays, index)
    want_idx, want_rays = fx.compact(live_np, [t.cpu().numpy() for t in rays])
    assert count == len(want_idx)
    assert np.array_equal(index[:count].cpu().numpy(), want_idx)
    assert (index[count:] == -1).all()                                                  # nothing written past the count
    for got, want in zip(out_rays, want_rays):
        assert np.array_equal(got[:count].cpu().numpy(), want)
        assert (got[count:] == -7.0).all()
    # scatter: two levels, compact results in buffers longer than the count
    comp = [(torch.from_numpy(rng.random((n, 3)).astype(np.float32)).to(DEV), torch.from_numpy(rng.random(n).astype(np.float32)).to(DEV),
             torch.from_numpy(rng.random(n).astype(np.float32)).to(DEV)) for _ in range(2)]
    for white in (True, False):
        full = [(torch.full((n, 3), -3.0, device=DEV), torch.full((n,), -3.0, device=DEV), torch.full((n,), -3.0, device=DEV)) for _ in range(2)]
        ops.scatter_frame(index, count, comp, full, live, rays.near, white)
        want = fx.scatter(want_idx, [tuple(t.cpu().numpy() for t in lv) for lv in comp], n, live_np, rays.near.cpu().numpy(), white)
        for lv in range(2):
            for got, w in zip(full[lv], want[lv]):
                assert np.array_equal(got.cpu().numpy(), w)
    # two runs, same bytes
    index2 = torch.full((n,), -1, dtype=torch.int32, device=DEV)
    out2 = Rays(*[torch.full_like(t, -7.0) for t in rays])
    assert ops.compact_rays(live, rays, out2, index2) == count and torch.equal(index2, index)
    assert all(torch.equal(a, b) for a, b in zip(out2, out_rays))


def test_zero_rays():
    from mipnerf_pl_amd import Rays, ops
    rays = Rays(*[torch.zeros(0, k, device=DEV) for k in (3, 3, 3, 1, 1, 1, 1)])
    occ = ops.occupancy_grid(torch.ones(4, 4, 4, device=DEV), 0.5, -1.0, 1.0, dilate=0)
    live = ops.ray_occupancy(occ, rays, 64)
    assert live.shape == (0,) and live.dtype == torch.uint8
    assert ops.compact_rays(live, rays, rays, torch.zeros(0, dtype=torch.int32, device=DEV)) == 0
    ops.scatter_frame(torch.zeros(0, dtype=torch.int32, device=DEV), 0, [(rays.origins, rays.near, rays.near)],
                      [(rays.origins, rays.near, rays.near)], live, rays.near, True)


# ---- classification -----------------------------------------------------------------------------------------------------------
def _fixture_sets(occ_bool, dims, lo, hi, g, N, **kw):
    args = (occ_bool, dims, lo, hi, g["rays_origins"], g["rays_directions"], g["rays_radii"], g["rays_near"], g["rays_far"], N)
    return fx.classify(*args, margin=-MARGIN, **kw), fx.classify(*args, margin=MARGIN, **kw)


@pytest.mark.parametrize("name", RAY_SETS)
@pytest.mark.parametrize("N", [128, 256])
@pytest.mark.parametrize("threshold,dilate", [(0.1, 0), (0.1, 1), (0.03, 0)])
def test_classification_lies_between_must_live_and_may_live(name, N, threshold, dilate):
    from mipnerf_pl_amd import ops
    sigma, _ = trained_lattice()
    g, rays = golden_rays(name)
    occ = ops.occupancy_grid(sigma, threshold, LO, HI, dilate=dilate)
    live = ops.ray_occupancy(occ, rays, N, outside_occupied=False).cpu().numpy().astype(bool)
    must, may = _fixture_sets(fx.unpack(words_of(occ), DIMS[0] - 1), DIMS, LO, HI, g, N, outside_occupied=False)     # from the device's bits
    n = len(live)
    band = int((may & ~must).sum())
    print(f"classification {name} N={N} thr={threshold} dilate={dilate}: live {live.mean():.4f} must {must.mean():.4f} may {may.mean():.4f} band {band}")
    G.record(f"ray_occupancy {name} N={N} thr={threshold} dilate={dilate}", live_share=live.mean(), band_rays=band)
    assert band <= 0.005 * n, "the inputs leave too many rays undecided for this check to mean much"
    assert not (must & ~live).any(), f"{int((must & ~live).sum())} rays that must be live were culled"
    assert not (live & ~may).any(), f"{int((live & ~may).sum())} rays are live that cannot be"
    assert 0.05 < 1.0 - live.mean() < 0.6                                                # both classes are there
    again = ops.ray_occupancy(occ, rays, N, outside_occupied=False).cpu().numpy().astype(bool)
    assert np.array_equal(again, live)


@pytest.mark.parametrize("name", RAY_SETS)
def test_outside_counts_as_occupied_or_is_clipped_away(name):
    """the box +-1.5: most of the rays have an end point outside it"""
    from mipnerf_pl_amd import ops
    sigma, _ = trained_lattice()
    g, rays = golden_rays(name)
    N = int(g["num_samples"])
    dims, lo, hi = (40, 40, 40), (-1.5,) * 3, (1.5,) * 3
    model = G.make_model(trained_params(), N, "fp32")
    occ = ops.field_occupancy(model, grid=40, lo=-1.5, hi=1.5, threshold=0.1, dilate=0)
    ends = np.concatenate([g["rays_origins"] + g["rays_near"] * g["rays_directions"], g["rays_origins"] + g["rays_far"] * g["rays_directions"]], 1)
    leaves = np.abs(ends).max(axis=1) > 1.5 + 0.1                                        # an end point well outside the box
    assert leaves.mean() > 0.5                                                           # most of them do leave it
    occ_bool = fx.unpack(words_of(occ), 39)
    for outside in (True, False):
        live = ops.ray_occupancy(occ, rays, N, outside_occupied=outside).cpu().numpy().astype(bool)
        must, may = _fixture_sets(occ_bool, dims, lo, hi, g, N, outside_occupied=outside)
        assert (may & ~must).sum() <= 0.005 * len(live)
        assert not (must & ~live).any() and not (live & ~may).any()
        if outside:
            assert live[leaves].all()
            assert np.array_equal(ops.ray_occupancy(occ, rays, N).cpu().numpy().astype(bool), live)      # the default is the conservative one
        else:
            assert 0.05 < 1.0 - live.mean() < 0.9 and not live[leaves].all()


@pytest.mark.parametrize("dilate", [0, 1])
@pytest.mark.parametrize("cone_scale", [1.0, 8.0])
def test_analytic_sphere_from_first_principles(dilate, cone_scale):
    """a sphere of radius R (lattice R - |x - c|, threshold 0).  Dead: an occupied cell has a corner inside the sphere or lies `dilate` cells
    from one that has, so all of it is within R + (1 + dilate) h sqrt(3) of the centre; a frustum's box reaches less than rho past its
    segment and a cell that meets it adds one more diagonal: a ray whose segment stays farther than R + rho_max + (2 + dilate) h sqrt(3)
    from the centre touches no occupied cell.  Live: a ray whose segment has a point p within R - h sqrt(3) of the centre: every corner of
    p's cell is within h sqrt(3) of p, hence inside the sphere, the cell is occupied, and p lies in some frustum's box.
    outside_occupied=False, so neither statement depends on the box holding the widened frusta."""
    from mipnerf_pl_amd import ops
    g, rays = golden_rays(RAY_SETS[0])
    N = 128
    dims, lo, hi = (96, 96, 96), (-4.0,) * 3, (4.0,) * 3
    h = 8.0 / 95
    centre, R = np.array([0.3, -0.2, 0.25]), 0.8
    lat = sphere_lattice(dims, lo, hi, centre, R)
    occ = ops.occupancy_grid(torch.from_numpy(lat).to(DEV), 0.0, lo, hi, dilate=dilate)
    live = ops.ray_occupancy(occ, rays, N, cone_scale=cone_scale, outside_occupied=False).cpu().numpy().astype(bool)
    o, d = g["rays_origins"].astype(np.float64), g["rays_directions"].astype(np.float64)
    near, far = g["rays_near"].astype(np.float64)[:, 0], g["rays_far"].astype(np.float64)[:, 0]
    tc = np.clip(((centre - o) * d).sum(-1) / (d * d).sum(-1), near, far)                # closest point of the segment
    dist = np.linalg.norm(o + tc[:, None] * d - centre, axis=-1)
    rho_max = cone_scale * g["rays_radii"][:, 0].astype(np.float64) * far
    surely_dead = dist > R + rho_max + (2 + dilate) * h * np.sqrt(3)
    surely_live = dist < R - h * np.sqrt(3)
    assert surely_dead.mean() > 0.1 and surely_live.mean() > 0.1, (surely_dead.mean(), surely_live.mean())
    assert not live[surely_dead].any() and live[surely_live].all()


# ---- the frame -------------------------------------------------------------------------------------------------------------------
def _outputs(frame):
    return [t.clone() for lv in range(len(frame.rgb)) for t in (frame.rgb[lv], frame.dist[lv], frame.acc[lv])]


@pytest.mark.parametrize("name,chunk", [(RAY_SETS[0], 3000), (RAY_SETS[1], 1500)])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("dilate,min_culled", [(0, 0.20), (1, 0.10)])
def test_live_rays_unchanged_and_dead_rays_harmless(name, chunk, precision, dilate, min_culled):
    from mipnerf_pl_amd import ops
    from mipnerf_pl_amd.model import CulledFrame, GraphedFrame
    threshold = 0.1
    g, rays = golden_rays(name)
    N, n = int(g["num_samples"]), int(g["batch"])
    assert n % chunk                                                                     # a ragged tail in the full frame
    model = G.make_model(trained_params(), N, precision)
    sigma, _ = trained_lattice()
    occ = ops.occupancy_grid(sigma, threshold, LO, HI, dilate=dilate)
    dev = torch.device(DEV)
    full = GraphedFrame(model, n, chunk, True, dev, capture=False)
    culled = CulledFrame(model, n, chunk, True, dev, occ, outside_occupied=False)
    assert (culled.n, culled.chunk, culled.white_bkgd) == (n, chunk, True)
    with torch.no_grad():
        full(rays)
        want = _outputs(full)
        c_rgb, f_rgb, dist = culled(rays)
    got = _outputs(culled)
    assert c_rgb is culled.rgb[0] and f_rgb is culled.rgb[-1] and dist is culled.dist[-1]
    live = culled.live.bool()
    assert culled.live_count == int(live.sum()) and 0 < culled.live_count < n
    assert culled.live_count % chunk                                                     # and a ragged tail in the compacted one
    assert torch.equal(culled.live, ops.ray_occupancy(occ, rays, N, outside_occupied=False))
    for a, b in zip(got, want):
        assert torch.equal(a[live], b[live])                                             # bit for bit: a ray does not see its neighbours
    dead = ~live
    for lv in range(2):
        assert (culled.rgb[lv][dead] == 1.0).all() and (culled.acc[lv][dead] == 0.0).all()
        assert torch.equal(culled.dist[lv][dead], rays.near[dead, 0])
    # what was dropped: every culled ray's golden acc stays under the opacity of a ray that meets density `threshold` all the way
    dead_np = dead.cpu().numpy()
    dn = np.linalg.norm(g["rays_directions"].astype(np.float64), axis=-1)
    bound = 1.0 - np.exp(-threshold * (g["rays_far"][:, 0].astype(np.float64) - g["rays_near"][:, 0]) * dn)
    share = float(dead_np.mean())
    worst = max(float(g["l0_acc"][dead_np].max()), float(g["l1_acc"][dead_np].max()))
    worst_seen = max(float(want[2][dead].max()), float(want[5][dead].max()))
    print(f"culled frame {name} {precision} dilate={dilate}: culled {share:.4f}, largest golden acc among culled {worst:.4f} (device {worst_seen:.4f}), "
          f"bound {bound.min():.3f}..{bound.max():.3f}")
    G.record(f"culled frame {name} {precision} thr {threshold} dilate {dilate}", culled_share=share, max_golden_acc_culled=worst,
             max_device_acc_culled=worst_seen, bound_min=bound.min())
    assert (g["l0_acc"][dead_np] <= bound[dead_np]).all() and (g["l1_acc"][dead_np] <= bound[dead_np]).all()
    assert share >= min_culled
    # a second frame through the same object: same bits
    with torch.no_grad():
        culled(rays)
    assert all(torch.equal(a, b) for a, b in zip(_outputs(culled), got))


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_all_live_all_dead_and_zero_rays(precision):
    from mipnerf_pl_amd import Rays, ops
    from mipnerf_pl_amd.model import CulledFrame, GraphedFrame
    g, rays = golden_rays(RAY_SETS[1])
    N, n, chunk = int(g["num_samples"]), int(g["batch"]), 1500
    model = G.make_model(trained_params(), N, precision)
    sigma, _ = trained_lattice()
    dev = torch.device(DEV)
    full = GraphedFrame(model, n, chunk, False, dev, capture=False)
    with torch.no_grad():
        full(rays)
    everything = ops.occupancy_grid(sigma, -1.0, LO, HI, dilate=0)                       # every density is > -1
    assert everything.occupied_fraction() == 1.0
    for outside in (True, False):                   # the rays run through the box: all live either way
        frame = CulledFrame(model, n, chunk, False, dev, everything, outside_occupied=outside)
        with torch.no_grad():
            frame(rays)
        assert frame.live_count == n
        assert all(torch.equal(a, b) for a, b in zip(_outputs(frame), _outputs(full)))
    nothing = ops.occupancy_grid(sigma, 1e9, LO, HI, dilate=3)
    assert nothing.occupied_fraction() == 0.0
    for white in (True, False):
        frame = CulledFrame(model, n, chunk, white, dev, nothing, outside_occupied=False)
        with torch.no_grad():
            frame(rays)
        assert frame.live_count == 0
        for lv in range(2):
            assert (frame.rgb[lv] == (1.0 if white else 0.0)).all() and (frame.acc[lv] == 0.0).all()
            assert torch.equal(frame.dist[lv], rays.near[:, 0])
    empty = CulledFrame(model, 0, chunk, True, dev, everything)
    c, f, d = empty(Rays(*[t[:0] for t in rays]))
    assert empty.live_count == 0 and c.shape == (0, 3) and f.shape == (0, 3) and d.shape == (0,)
    with pytest.raises(ValueError):
        frame(Rays(*[t[:10] for t in rays]))


def _psnr(a, b):
    return float(-10.0 * np.log10(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2) + 1e-30))


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_whole_frame_with_culling_meets_the_frame_criteria(precision):
    """the frame_c5_800x800 pose and size; threshold 0.03, dilate 0, 64^3 over +-2.0 (the camera sits at |o| = 4: outside_occupied=False, see
    the module docstring).  The project's frame criteria with culling on: fine rgb >= 55 dB against the reference's frame in both
    precisions, and the PSNR against the scene within 0.1 dB of the reference's."""
    from mipnerf_pl_amd import ops
    from mipnerf_pl_amd.datasets import RenderGen
    from mipnerf_pl_amd.evaluate import FrameEvaluator
    from mipnerf_pl_amd.model import CulledFrame
    g = G.load_golden("frame_c5_800x800")
    size, N, chunk = int(g["cfg_size"]), int(g["cfg_num_samples"]), int(g["cfg_chunk"])
    model = G.make_model(trained_params(), N, precision)
    dev = torch.device(DEV)
    occ = ops.field_occupancy(model, grid=64, lo=-2.0, hi=2.0, threshold=0.03, dilate=0)
    rays = RenderGen(float(g["focal"]), [size, size], scales=1, device=dev)[int(g["cfg_pose"])]
    ev = FrameEvaluator(model, size, size, chunk, True, dev, occupancy=occ)
    assert isinstance(ev.frame, CulledFrame)
    ev.frame.outside_occupied = False
    with torch.no_grad():
        rgb, dist, acc = ev.render(rays)
    fine = rgb.cpu().numpy()
    live = ev.frame.live.cpu().numpy().astype(bool).reshape(size, size)
    gt = g["gt_u8"].astype(np.float32) / 255.0
    culled_share = 1.0 - ev.frame.live_count / float(size * size)
    figures = dict(culled_share=culled_share, psnr_vs_reference_frame=_psnr(fine, g["fine_rgb"][0]), psnr_vs_scene=_psnr(fine, gt),
                   ref_psnr_vs_scene=float(g["psnr_fine"]), max_golden_acc_culled=float(g["acc"][~live].max()) if (~live).any() else 0.0)
    print(f"whole frame with culling {precision}: {figures}")
    G.record(f"frame_c5 culled {precision}", **figures)
    assert 0.005 < culled_share < 0.5                                                   # CPU, the reference's lattice: 2.1 %
    assert (rgb[torch.from_numpy(~live).to(DEV)] == 1.0).all()
    assert figures["psnr_vs_reference_frame"] >= 55.0, figures
    assert abs(figures["psnr_vs_scene"] - figures["ref_psnr_vs_scene"]) < 0.1, figures


# ---- command lines ---------------------------------------------------------------------------------------------------------------
def _system(params, num_samples, **hp_extra):
    from mipnerf_pl_amd.system import DEFAULT_HPARAMS, MipNeRFSystem
    hp = dict(DEFAULT_HPARAMS)
    hp.update({"nerf.num_samples": num_samples, "exp_name": "cli", "val.batch_type": "single_image", "dataset_name": "blender"})
    hp.update(hp_extra)
    system = MipNeRFSystem(hp, precision="fp32")
    if params is not None:
        missing, unexpected = system.load_state_dict({"mip_nerf.mlp." + k: torch.from_numpy(v.copy()) for k, v in params.items()}, strict=True)
        assert not missing and not unexpected
    return system


def _files(root):
    out = {}
    for d, _, fs in os.walk(root):
        for f in fs:
            with open(os.path.join(d, f), "rb") as fh:
                out[os.path.relpath(os.path.join(d, f), root)] = fh.read()
    return out


def test_eval_command_line_with_cull(tmp_path, capsys):
    from dataset_fixture import write_blender
    from mipnerf_pl_amd import eval as eval_cli
    from oracle import mipnerf_oracle as orc
    from PIL import Image
    data = write_blender(str(tmp_path / "data"), seed=6, counts=(("test", 2),), w=16, h=16)
    ckpt = str(tmp_path / "last.ckpt")
    _system(orc.make_params(seed=5, density_gain=40.0), 32).save_checkpoint(ckpt)
    common = ["--ckpt", ckpt, "--data", data, "--scale", "1", "--save_image", "--chunk_size", "100", "--precision", "fp32", "--base_size", "16", "16"]
    plain, allocc, none = str(tmp_path / "plain"), str(tmp_path / "all"), str(tmp_path / "none")
    eval_cli.main(common + ["--out_dir", plain])
    assert "cull:" not in capsys.readouterr().out
    # every density is > -1: the grid is all occupied, every ray live, every byte as without --cull
    eval_cli.main(common + ["--out_dir", allocc, "--cull", "--cull_grid", "24", "--cull_threshold", "-1", "--cull_dilate", "0"])
    text = capsys.readouterr().out
    assert "cull: occupied share of the 24^3 grid" in text and text.count("cull: occupied share") == 1 and "): 1.0000" in text
    assert "cull: mean live share per frame: 1.0000 (2 frames)" in text
    fp, fa = _files(plain), _files(allocc)
    assert fp.keys() == fa.keys() and len([k for k in fp if k.endswith(".png")]) >= 6
    assert all(fp[k] == fa[k] for k in fp), [k for k in fp if fp[k] != fa[k]]
    # nothing occupied and nothing outside the default box: every ray culled, the same files, white frames
    eval_cli.main(common + ["--out_dir", none, "--cull", "--cull_grid", "24", "--cull_threshold", "1e9"])
    text = capsys.readouterr().out
    assert "): 0.0000" in text and "cull: mean live share per frame: 0.0000 (2 frames)" in text
    fn = _files(none)
    assert fn.keys() == fp.keys()
    assert (np.array(Image.open(os.path.join(none, "test", "cli", "1", "00000_rgb.png"))) == 255).all()


def test_render_video_command_line_with_cull(tmp_path, capsys):
    from mipnerf_pl_amd import render_video
    from oracle import mipnerf_oracle as orc
    ckpt = str(tmp_path / "last.ckpt")
    _system(orc.make_params(seed=2, density_gain=40.0), 32).save_checkpoint(ckpt)
    common = ["--ckpt", ckpt, "--scale", "2", "--n_poses", "2", "--chunk_size", "160", "--precision", "fp32", "--base_size", "24", "24"]
    plain, allocc, some = str(tmp_path / "plain"), str(tmp_path / "all"), str(tmp_path / "some")
    render_video.main(common + ["--out_dir", plain])
    assert "cull:" not in capsys.readouterr().out
    render_video.main(common + ["--out_dir", allocc, "--cull", "--cull_grid", "20", "--cull_threshold", "-1"])
    text = capsys.readouterr().out
    assert text.count("cull: occupied share of the 20^3 grid") == 1 and "cull: mean live share per frame: 1.0000 (4 frames)" in text
    fp, fa = _files(plain), _files(allocc)
    assert fp.keys() == fa.keys() and sum(k.endswith("_rgb.png") for k in fp) == 4
    assert all(fp[k] == fa[k] for k in fp), [k for k in fp if fp[k] != fa[k]]
    # a bound of the user's own, smaller than the rays' reach: what lies outside counts as occupied, so every ray stays live
    render_video.main(common + ["--out_dir", some, "--cull", "--cull_grid", "20", "--cull_threshold", "1e9", "--cull_bound", "1.0"])
    text = capsys.readouterr().out
    assert "over +-1.0000" in text and "cull: mean live share per frame: 1.0000 (4 frames)" in text
    fs = _files(some)
    assert fs.keys() == fp.keys() and all(fp[k] == fs[k] for k in fp)


def test_cull_refuses_an_unbounded_checkpoint(tmp_path):
    from mipnerf_pl_amd import eval as eval_cli
    from mipnerf_pl_amd import render_video
    ckpt = str(tmp_path / "unbounded.ckpt")
    _system(None, 32, **{"nerf.unbounded": True}).save_checkpoint(ckpt)
    with pytest.raises(SystemExit, match="unbounded"):
        eval_cli.main(["--ckpt", ckpt, "--data", str(tmp_path), "--out_dir", str(tmp_path / "o"), "--scale", "1", "--cull"])
    with pytest.raises(SystemExit, match="unbounded"):
        render_video.main(["--ckpt", ckpt, "--out_dir", str(tmp_path / "o"), "--scale", "1", "--cull"])
    assert not os.path.exists(str(tmp_path / "o"))
