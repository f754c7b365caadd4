"""GPU: the occupied span of every ray (csrc/kernels_occupancy.hip k_ray_span, ops.ray_span) and tightened culling
(model.CulledFrame(tighten=True)).

  - liveness byte for byte that of ops.ray_occupancy;
  - first / last between the float64 brute force's must-hit and may-hit spans (tests/span_fixture.py, bounding boxes shrunk / grown by a
    margin of h), for every ray, with the share of rays the margin leaves undecided capped at 1 % so that the bracket means something;
  - near' / far' torch.equal to the sampler's own fence posts, linear and in disparity;
  - engineered grids with one or two occupied cells at the edges of the 64-frustum buckets, of the four-ray workgroups and of the 32-cell
    words, where must equals may and the expected values are exact;
  - CulledFrame(tighten=True) torch.equal to the renderer on the tightened rays, also when span_samples differs from the rendered count;
  - the golden 800 x 800 pose: PSNR against the scene with and without tightening, at 128 and at 64 samples.

Margins.  The device's fp32 error on a frustum coordinate |x| <= 4 is about 1e-6 (two roundings of o + t d and one of rho), i.e. 2e-5 h
on the 64^3 grid over +-2 (h = 0.0635) and 3e-5 h at 128^3.  The analytic-sphere inputs use the margin 1e-3 h (47 to 80 of 8192 rays
undecided).  The golden ray sets on the trained field's lattice leave 1.1 to 1.9 % of their rays undecided at that margin, with the
fixture alone (the foggy field's spans end at many more cell faces than a sphere's), which is over the 1 % cap: they use
MARGIN_GOLDEN = 2.5e-4 h, still twelve times the device's error."""
import os

import numpy as np
import pytest
import torch

import gpu_util as G
import occupancy_fixture as fx
import span_fixture as sx

pytestmark = pytest.mark.gpu
DEV = G.DEV
DIMS, LO, HI = (64, 64, 64), (-2.0,) * 3, (2.0,) * 3
RAY_SETS = ("fulltrained_c4_8192x256", "fulltrained_c2_4096x128")
MARGIN = 1e-3
MARGIN_GOLDEN = 2.5e-4
UNDECIDED_CAP = 0.01
_CACHE = {}


def trained_params():
    f = G.load_golden("trained_field")
    return {k[2:]: f[k] for k in f if k.startswith("p_")}


def trained_lattice():
    if "lattice" not in _CACHE:
        from mipnerf_pl_amd import ops
        _CACHE["lattice"] = ops.density_grid(G.make_model(trained_params(), 128, "fp32"), DIMS, LO, HI)
    return _CACHE["lattice"]


def golden_rays(name):
    if name not in _CACHE:
        g = G.load_golden(name)
        _CACHE[name] = ({k: g[k] for k in g if k.startswith("rays_")}, G.to_dev(G.rays_of(g)), int(g["num_samples"]), int(g["batch"]))
    return _CACHE[name]


def sphere_rays(n=8192, seed=0):
    """the inputs the 1 % cap was checked on: origins on |o| = 4, unit directions towards points uniform in [-1.6, 1.6]^3, radii 1e-3,
    near 2, far 6 (numpy dict in the golden files' layout, device Rays)"""
    key = ("sphere_rays", n, seed)
    if key not in _CACHE:
        rng = np.random.default_rng(seed)
        o = rng.normal(size=(n, 3))
        o = 4.0 * o / np.linalg.norm(o, axis=1, keepdims=True)
        d = rng.uniform(-1.6, 1.6, (n, 3)) - o
        d = d / np.linalg.norm(d, axis=1, keepdims=True)
        one = np.ones((n, 1))
        g = {"rays_" + k: np.ascontiguousarray(v, np.float32) for k, v in zip(("origins", "directions", "viewdirs", "radii", "lossmult", "near", "far"),
                                                                               (o, d, d, 1e-3 * one, one, 2.0 * one, 6.0 * one))}
        _CACHE[key] = (g, G.to_dev(G.rays_of(g)))
    return _CACHE[key]


def sphere_occupancy(grid):
    """values 1 inside the unit sphere, 0 outside, on grid^3 points over [-2, 2]^3; threshold 0.5, dilate 0"""
    from mipnerf_pl_amd import ops
    ax = np.float32(-2.0) + np.arange(grid).astype(np.float32) * (np.float32(4.0) / np.float32(grid - 1))
    z, y, x = np.meshgrid(ax, ax, ax, indexing="ij")
    lat = (x * x + y * y + z * z <= 1.0).astype(np.float32)
    return ops.occupancy_grid(torch.from_numpy(lat).to(DEV), 0.5, LO, HI, dilate=0), (grid,) * 3


# (tag) -> the configuration: occupancy, dims, numpy rays, device rays, N, keywords, margin
CONFIGS = ([("sphere", 64, 128, False, False), ("sphere", 33, 64, False, False), ("sphere", 128, 256, False, False),
            ("sphere", 64, 128, True, False), ("sphere", 64, 128, False, True)]
           + [(name, thr, N, dilate, None) for name in RAY_SETS for N in (128, 256) for thr, dilate in ((0.1, 0), (0.1, 1), (0.03, 0))])


def _ids(c):
    if c[0] == "sphere":
        return f"sphere-{c[1]}-N{c[2]}" + ("-disparity" if c[3] else "") + ("-outside" if c[4] else "")
    return f"{c[0]}-thr{c[1]}-N{c[2]}-dilate{c[3]}"


def evaluated(cfg):
    """device results and fixture spans of one configuration, computed once and shared by the tests below"""
    if cfg in _CACHE:
        return _CACHE[cfg]
    from mipnerf_pl_amd import ops
    if cfg[0] == "sphere":
        _, grid, N, disparity, outside = cfg
        occ, dims = sphere_occupancy(grid)
        g, rays = sphere_rays()
        kw, margin = dict(disparity=disparity, outside_occupied=outside), MARGIN
    else:
        name, thr, N, dilate, _ = cfg
        occ, dims = ops.occupancy_grid(trained_lattice(), thr, LO, HI, dilate=dilate), DIMS
        g, rays = golden_rays(name)[:2]
        kw, margin = dict(disparity=False, outside_occupied=False), MARGIN_GOLDEN
    live, first, last, near, far = ops.ray_span(occ, rays, N, **kw)
    ref_live = ops.ray_occupancy(occ, rays, N, **kw)
    occ_bool = fx.unpack(occ.bits.cpu().numpy(), dims[0] - 1)                               # from the device's bits
    args = (occ_bool, dims, LO, HI, g["rays_origins"], g["rays_directions"], g["rays_radii"], g["rays_near"], g["rays_far"], N)
    must, may = (sx.span(*args, margin=m, **kw) for m in (-margin, margin))
    res = dict(occ=occ, rays=rays, g=g, N=N, kw=kw, live=live, first=first, last=last, near=near, far=far, ref_live=ref_live, must=must,
               may=may)
    _CACHE[cfg] = res
    return res


# ---- 1. same liveness -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", CONFIGS, ids=_ids)
def test_liveness_is_that_of_ray_occupancy(cfg):
    from mipnerf_pl_amd import ops
    r = evaluated(cfg)
    assert r["live"].dtype == torch.uint8 and torch.equal(r["live"], r["ref_live"])
    assert 0 < int(r["live"].sum()) < r["live"].numel()                                    # both classes are there
    # the skipped outputs change nothing, and two runs give the same bytes
    only = ops.ray_span(r["occ"], r["rays"], r["N"], out=(torch.empty_like(r["live"]), None, None, None, None), **r["kw"])
    assert torch.equal(only[0], r["live"]) and only[1:] == (None, None, None, None)
    again = ops.ray_span(r["occ"], r["rays"], r["N"], **r["kw"])
    assert all(torch.equal(a, b) for a, b in zip(again, (r["live"], r["first"], r["last"], r["near"], r["far"])))


# ---- 2. the bracket, every ray ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", CONFIGS, ids=_ids)
def test_first_and_last_lie_between_the_must_and_may_spans(cfg):
    r = evaluated(cfg)
    N = r["N"]
    first, last = r["first"].cpu().numpy().astype(np.int64), r["last"].cpu().numpy().astype(np.int64)
    live = r["live"].cpu().numpy().astype(bool)
    (must_live, first_must, last_must), (may_live, first_may, last_may) = r["must"], r["may"]
    n = len(first)
    assert first.shape == last.shape == first_must.shape == (n,)                         # no ray is left out
    undecided = (first_must != first_may) | (last_must != last_may)
    share = float(undecided.mean())
    print(f"span bracket {_ids(cfg)}: undecided {int(undecided.sum())} of {n} rays = {share:.4%}; liveness undecided {int((may_live & ~must_live).sum())}")
    G.record(f"ray_span bracket {_ids(cfg)}", undecided_share=share, live_share=live.mean())
    assert share <= UNDECIDED_CAP, "the inputs leave too many rays undecided for the bracket to mean much"
    # a ray dead in one set has first = N, last = -1 there, so the same two inequalities hold for it
    assert (first_must[~must_live] == N).all() and (last_must[~must_live] == -1).all()
    assert (first_may[~may_live] == N).all() and (last_may[~may_live] == -1).all()
    bad_first = ~((first_may <= first) & (first <= first_must))
    bad_last = ~((last_must <= last) & (last <= last_may))
    assert not bad_first.any(), (int(bad_first.sum()), first[bad_first][:5], first_may[bad_first][:5], first_must[bad_first][:5])
    assert not bad_last.any(), (int(bad_last.sum()), last[bad_last][:5], last_must[bad_last][:5], last_may[bad_last][:5])
    assert (first[~live] == N).all() and (last[~live] == -1).all() and (first[live] <= last[live]).all()
    assert (first[live] >= 0).all() and (last[live] <= N - 1).all()


# ---- 3. exact fence posts --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", CONFIGS, ids=_ids)
def test_near_and_far_are_the_samplers_fence_posts(cfg):
    from mipnerf_pl_amd import ops
    r = evaluated(cfg)
    rays, N = r["rays"], r["N"]
    t = ops.sample_t(N, rays.near, rays.far, False, r["kw"]["disparity"])                  # the coarse level's deterministic t_samples
    live = r["live"].bool()
    first, last = r["first"].long(), r["last"].long()
    assert r["near"].shape == rays.near.shape and r["far"].shape == rays.far.shape
    want_near = t.gather(1, first.clamp(0, N)[:, None])
    want_far = t.gather(1, (last + 1).clamp(0, N)[:, None])
    assert torch.equal(r["near"][live], want_near[live]) and torch.equal(r["far"][live], want_far[live])
    assert torch.equal(r["near"][~live], rays.near[~live]) and torch.equal(r["far"][~live], rays.far[~live])
    assert (r["near"][live] < r["far"][live]).all()
    tight = float(((r["far"] - r["near"])[live] / (rays.far - rays.near)[live]).mean())
    print(f"span {_ids(cfg)}: mean (far' - near') / (far - near) over the live rays {tight:.4f}")


# ---- 4. bucket edges --------------------------------------------------------------------------------------------------------------
def _engineered(N, nx, cells_hit, firsts):
    """(Occupancy, box, numpy rays).  (nx, 4, 4) points over [0, nx - 1] x [0, 3]^2 (h = 1); the occupied cells are exactly (c, 1, 1) for c
    in `cells_hit` -- the packed words are written directly, a lattice cannot occupy one cell alone.  Ray r runs along +x at y = z = 1.5
    with near 1, far 2, d = (2 N, 0, 0) and o_x = cells_hit[0] - 2 firsts[r] - 0.5 - 2 N: frustum i is [k - 0.5 + 2 i, k + 1.5 + 2 i] with
    k = cells_hit[0] - 2 f, two cells long from a half-integer, so frustum f holds cell cells_hit[0] with half a cell to spare at both
    ends and no other frustum touches it: a cell c = cells_hit[0] + 2 j is met by frustum f + j alone.  radii 0.05: rho = 0.05 t is in
    [0.05, 0.1], so every bounding box ends >= 0.4 h from a face and none is thinner than the fixture's margin.  The rays start before the
    grid and end far behind it."""
    from mipnerf_pl_amd import ops
    occ_bool = np.zeros((3, 3, nx - 1), bool)
    for c in cells_hit:
        assert 0 <= c <= nx - 2 and (c - cells_hit[0]) % 2 == 0
        occ_bool[1, 1, c] = True
    words = np.ascontiguousarray(fx.pack(occ_bool))
    bits = torch.from_numpy(words.view(np.int32)).to(DEV).view(torch.uint32)
    dims, lo, hi = (nx, 4, 4), (0.0, 0.0, 0.0), (float(nx - 1), 3.0, 3.0)
    occ = ops.Occupancy(bits, dims, lo, hi)
    n = len(firsts)
    o = np.zeros((n, 3))
    o[:, 0] = [cells_hit[0] - 2 * f - 0.5 - 2 * N for f in firsts]
    o[:, 1:] = 1.5
    d = np.zeros((n, 3))
    d[:, 0] = 2.0 * N
    one = np.ones((n, 1))
    g = {"rays_" + k: np.ascontiguousarray(v, np.float32) for k, v in zip(("origins", "directions", "viewdirs", "radii", "lossmult", "near", "far"),
                                                                           (o, d, d / (2.0 * N), 0.05 * one, one, one, 2.0 * one))}
    return occ, occ_bool, (dims, lo, hi), g


def _check_engineered(N, nx, cells_hit, firsts, outside_occupied):
    """device against the fixture (where must equals may by construction); returns the fixture's (live, first, last)"""
    from mipnerf_pl_amd import ops
    occ, occ_bool, (dims, lo, hi), g = _engineered(N, nx, cells_hit, firsts)
    rays = G.to_dev(G.rays_of(g))
    live, first, last, near, far = ops.ray_span(occ, rays, N, outside_occupied=outside_occupied)
    # the rays differ only in their origin and many share one: the fixture sees each distinct ray once
    _, pick, back = np.unique(g["rays_origins"], axis=0, return_index=True, return_inverse=True)
    back = back.reshape(-1)
    args = (occ_bool, dims, lo, hi) + tuple(g["rays_" + k][pick] for k in ("origins", "directions", "radii", "near", "far")) + (N,)
    want = sx.span(*args, margin=0.0, outside_occupied=outside_occupied)
    for m in (-1e-2, 1e-2):
        other = sx.span(*args, margin=m, outside_occupied=outside_occupied)
        assert all(np.array_equal(a, b) for a, b in zip(want, other)), (N, nx, m)
    want = tuple(a[back] for a in want)
    assert np.array_equal(live.cpu().numpy().astype(bool), want[0]), (N, nx, cells_hit)
    assert np.array_equal(first.cpu().numpy(), want[1]), (N, nx, cells_hit, first.cpu().numpy()[:8], want[1][:8])
    assert np.array_equal(last.cpu().numpy(), want[2]), (N, nx, cells_hit, last.cpu().numpy()[:8], want[2][:8])
    assert torch.equal(live, ops.ray_occupancy(occ, rays, N, outside_occupied=outside_occupied))
    t = ops.sample_t(N, rays.near, rays.far, False, False)
    lv = live.bool()
    assert torch.equal(near[lv], t.gather(1, first.long().clamp(0, N)[:, None])[lv])
    assert torch.equal(far[lv], t.gather(1, (last.long() + 1).clamp(0, N)[:, None])[lv])
    assert torch.equal(near[~lv], rays.near[~lv]) and torch.equal(far[~lv], rays.far[~lv])
    return want


def _targets(N):
    return sorted({f for f in (0, 62, 63, 64, 65, N - 1) if 0 <= f < N})


@pytest.mark.parametrize("N", [1, 63, 64, 65, 128, 256, 1024])
def test_one_hit_frustum_at_the_bucket_word_and_workgroup_edges(N):
    """one occupied cell, met by frustum f alone, f over 0, 62, 63, 64, 65 and N - 1: first = last = f"""
    targets = _targets(N)
    for nx, count in zip((33, 34, 65, 65, 34), (1, 3, 4, 5, 4097)):                     # ragged against the four rays per workgroup
        firsts = [targets[(i + count) % len(targets)] for i in range(count)]
        cells = [32] if count > 5 else sorted(c for c in {0, 31, 32, nx - 2} if c <= nx - 2)      # the word edges and both ends of the row
        for c in cells:
            want = _check_engineered(N, nx, [c], firsts, outside_occupied=False)
            assert want[0].all() and want[1].tolist() == firsts and want[2].tolist() == firsts, (N, nx, c)


@pytest.mark.parametrize("N", [63, 64, 65, 128, 256, 1024])
def test_first_and_last_in_the_same_neighbouring_and_far_buckets(N):
    """two occupied cells 2 * delta apart: first = f comes from the one, last = f + delta from the other; delta = N - 1 with f = 0 is
    bucket 0 against the last bucket"""
    for delta in sorted({1, 2, 3, 30, 64, N - 1}):
        if delta > N - 1:
            continue
        c0 = 1
        nx = max(34, c0 + 2 * delta + 3)
        firsts = sorted({f for f in _targets(N) + [1, 61] if f + delta <= N - 1})
        assert firsts and firsts[0] == 0
        want = _check_engineered(N, nx, [c0, c0 + 2 * delta], firsts, outside_occupied=False)
        assert want[0].all() and want[1].tolist() == firsts and want[2].tolist() == [f + delta for f in firsts], (N, delta)
        # ... and a ray that reaches only the first of the two cells: first = last
        if N > 2:
            want = _check_engineered(N, nx, [c0, c0 + 2 * delta], [N - 1], outside_occupied=False)
            assert want[1].tolist() == [N - 1] and want[2].tolist() == [N - 1]


@pytest.mark.parametrize("N", [1, 64, 65, 1024])
def test_rays_that_start_outside_the_box(N):
    """cell 32 of 33: a ray aimed at frustum f starts at x = 31.5 - 2 f, outside the box from f = 16, and ends at 31.5 - 2 f + 2 N >= 33.5,
    past it.  With outside_occupied the frusta out there hit: last = N - 1 for every ray, first = 0 for the rays that start outside;
    clipped away, the span is the one frustum that meets the cell"""
    targets = _targets(N)
    tg = np.asarray(targets)
    want = _check_engineered(N, 34, [32], targets, outside_occupied=True)
    assert want[0].all() and (want[2] == N - 1).all() and (want[1][tg >= 16] == 0).all() and (want[1][tg < 16] == tg[tg < 16]).all()
    want = _check_engineered(N, 34, [32], targets, outside_occupied=False)
    assert want[1].tolist() == targets and want[2].tolist() == targets
    # nothing occupied: dead when clipped, live through the outside otherwise
    from mipnerf_pl_amd import ops
    occ, _, _, g = _engineered(N, 34, [32], targets)
    occ.bits.zero_()
    rays = G.to_dev(G.rays_of(g))
    live, first, last, _, _ = ops.ray_span(occ, rays, N, outside_occupied=False)
    assert (live == 0).all() and (first == N).all() and (last == -1).all()
    live, first, last, _, _ = ops.ray_span(occ, rays, N, outside_occupied=True)
    assert (live == 1).all() and (last == N - 1).all()


@pytest.mark.parametrize("N", [1, 63, 64, 65, 128, 256, 1024])
def test_all_occupied_and_all_empty_grids(N):
    from mipnerf_pl_amd import Rays, ops
    n = 261
    rng = np.random.default_rng(N)
    o = rng.uniform(0.2, 0.8, (n, 3))
    d = rng.uniform(1.0, 1.9, (n, 3))                       # stays inside [0, 3]^3: o + d < 2.7
    one = np.ones((n, 1))
    rays = Rays(*[torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV) for a in (o, d, d, 1e-3 * one, one, 0.0 * one, one)])
    full = ops.occupancy_grid(torch.ones(5, 6, 34, device=DEV), 0.5, 0.0, 3.0, dilate=0)
    empty = ops.occupancy_grid(torch.zeros(5, 6, 34, device=DEV), 0.5, 0.0, 3.0, dilate=0)
    for outside in (True, False):
        live, first, last, near, far = ops.ray_span(full, rays, N, outside_occupied=outside)
        assert (live == 1).all() and (first == 0).all() and (last == N - 1).all()
        assert torch.equal(near, rays.near) and torch.equal(far, rays.far)                # 0 + 1 * 0 and 0 + 1 * 1
        live, first, last, near, far = ops.ray_span(empty, rays, N, outside_occupied=outside)
        assert (live == 0).all() and (first == N).all() and (last == -1).all()
        assert torch.equal(near, rays.near) and torch.equal(far, rays.far)
    none = Rays(*[t[:0] for t in rays])
    out = ops.ray_span(full, none, N)
    assert [t.shape[0] for t in out] == [0] * 5 and out[1].dtype == torch.int32 and out[3].dtype == torch.float32
    with pytest.raises(ValueError, match="out"):
        ops.ray_span(full, rays, N, out=(torch.empty(n, dtype=torch.uint8, device=DEV), torch.empty(n, device=DEV), None, None, None))


# ---- 5. the tightened frame is the renderer on the tightened rays -------------------------------------------------------------------
def _outputs(frame):
    return [t.clone() for lv in range(len(frame.rgb)) for t in (frame.rgb[lv], frame.dist[lv], frame.acc[lv])]


def _frame_rays(n):
    from mipnerf_pl_amd import Rays
    _, rays, N, batch = golden_rays(RAY_SETS[1])
    assert n <= batch
    return Rays(*[t[:n].contiguous() for t in rays]), N


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_tightened_frame_is_the_renderer_on_the_tightened_rays(precision):
    from mipnerf_pl_amd import ops
    from mipnerf_pl_amd.model import CulledFrame, GraphedFrame
    chunk, n = 1024, 3 * 1024 + 17
    rays, N = _frame_rays(n)
    model = G.make_model(trained_params(), N, precision)
    occ = ops.occupancy_grid(trained_lattice(), 0.1, LO, HI, dilate=0)
    dev = torch.device(DEV)
    live, first, last, near, far = ops.ray_span(occ, rays, N, outside_occupied=False)
    plain = GraphedFrame(model, n, chunk, True, dev, capture=False)
    tight = CulledFrame(model, n, chunk, True, dev, occ, outside_occupied=False, tighten=True)
    assert tight.tighten is True and tight.span_samples == N
    with torch.no_grad():
        plain(rays._replace(near=near, far=far))
        want = _outputs(plain)
        c_rgb, f_rgb, dist = tight(rays)
    got = _outputs(tight)
    lv = live.bool()
    assert torch.equal(tight.live, live) and tight.live_count == int(lv.sum()) and 0 < tight.live_count < n
    assert torch.equal(tight.first, first) and torch.equal(tight.last, last)
    assert torch.equal(tight.near_span, near) and torch.equal(tight.far_span, far)
    assert c_rgb is tight.rgb[0] and f_rgb is tight.rgb[-1] and dist is tight.dist[-1]
    for a, b in zip(got, want):
        assert torch.equal(a[lv], b[lv])
    for l_ in range(2):                                     # dead pixels: the scatter rule with the ORIGINAL near
        assert (tight.rgb[l_][~lv] == 1.0).all() and (tight.acc[l_][~lv] == 0.0).all()
        assert torch.equal(tight.dist[l_][~lv], rays.near[~lv, 0])
    # the tightening did tighten, and the tightened frame is not the untightened one
    assert (near[lv] > rays.near[lv]).any() and (far[lv] < rays.far[lv]).any()
    loose = CulledFrame(model, n, chunk, True, dev, occ, outside_occupied=False)
    with torch.no_grad():
        loose(rays)
    assert torch.equal(loose.live, live) and not torch.equal(loose.rgb[-1], tight.rgb[-1])
    assert loose.span_share == pytest.approx(tight.span_share, abs=0.0)
    # a second frame through the same object: same bits
    with torch.no_grad():
        tight(rays)
    assert all(torch.equal(a, b) for a, b in zip(_outputs(tight), got))


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_all_occupied_tightening_changes_nothing(precision):
    """near 2 and far 6: near' = 2 + 4 * 0 and far' = 2 + 4 * 1 are exact in fp32, so the tightened frame is the plain frame"""
    from mipnerf_pl_amd import ops
    from mipnerf_pl_amd.model import CulledFrame, GraphedFrame
    chunk, n = 1024, 3 * 1024 + 17
    rays, N = _frame_rays(n)
    assert (rays.near == 2.0).all() and (rays.far == 6.0).all()
    model = G.make_model(trained_params(), N, precision)
    everything = ops.occupancy_grid(trained_lattice(), -1.0, LO, HI, dilate=0)
    dev = torch.device(DEV)
    plain = GraphedFrame(model, n, chunk, False, dev, capture=False)
    tight = CulledFrame(model, n, chunk, False, dev, everything, tighten=True)
    with torch.no_grad():
        plain(rays)
        tight(rays)
    assert tight.live_count == n and tight.span_share == 1.0
    assert all(torch.equal(a, b) for a, b in zip(_outputs(tight), _outputs(plain)))


# ---- 6. span_samples differs from the rendered count ---------------------------------------------------------------------------------
def test_span_samples_may_differ_from_the_rendered_count():
    from mipnerf_pl_amd import ops
    from mipnerf_pl_amd.model import CulledFrame, GraphedFrame
    chunk, n = 1024, 3 * 1024 + 17
    rays, N = _frame_rays(n)
    assert N == 128
    g = golden_rays(RAY_SETS[1])[0]
    model64 = G.make_model(trained_params(), 64, "fp32")
    occ = ops.occupancy_grid(trained_lattice(), 0.1, LO, HI, dilate=0)
    dev = torch.device(DEV)
    live, first, last, near, far = ops.ray_span(occ, rays, 128, outside_occupied=False)
    plain = GraphedFrame(model64, n, chunk, True, dev, capture=False)
    tight = CulledFrame(model64, n, chunk, True, dev, occ, outside_occupied=False, tighten=True, span_samples=128)
    with torch.no_grad():
        plain(rays._replace(near=near, far=far))
        tight(rays)
    lv = live.bool()
    assert tight.span_samples == 128 and model64.num_samples == 64
    assert torch.equal(tight.live, live) and torch.equal(tight.near_span, near) and torch.equal(tight.far_span, far)
    for a, b in zip(_outputs(tight), _outputs(plain)):
        assert torch.equal(a[lv], b[lv])
    # without span_samples the classification would follow the model's 64 frusta
    assert CulledFrame(model64, n, chunk, True, dev, occ, tighten=True).span_samples == 64
    # .span_share against the fixture.  A ray the margin leaves undecided moves its own term of the mean by at most 1 and the number of
    # terms by at most one: |share - fixture| <= 2 * undecided / live rays
    occ_bool = fx.unpack(occ.bits.cpu().numpy(), DIMS[0] - 1)
    args = (occ_bool, DIMS, LO, HI, g["rays_origins"][:n], g["rays_directions"][:n], g["rays_radii"][:n], g["rays_near"][:n], g["rays_far"][:n], 128)
    (ml, mf, mL), (yl, yf, yL), (_, zf, zL) = (sx.span(*args, margin=m, outside_occupied=False) for m in (-MARGIN_GOLDEN, MARGIN_GOLDEN, 0.0))
    undecided = int(((mf != yf) | (mL != yL)).sum())
    want = sx.span_share(zf, zL, 128)
    print(f"span share {tight.span_share:.5f}, fixture {want:.5f}, undecided rays {undecided} of {n}")
    assert undecided <= UNDECIDED_CAP * n
    assert abs(tight.span_share - want) <= 2.0 * undecided / max(1, int(ml.sum())) + 1e-12
    assert 0.0 < tight.span_share < 1.0


def _system(params, num_samples):
    from mipnerf_pl_amd.system import DEFAULT_HPARAMS, MipNeRFSystem
    hp = dict(DEFAULT_HPARAMS)
    hp.update({"nerf.num_samples": num_samples, "exp_name": "cli", "val.batch_type": "single_image", "dataset_name": "blender"})
    system = MipNeRFSystem(hp, precision="fp32")
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


def test_render_video_command_line_with_tightening_and_render_samples(tmp_path, capsys):
    """--render_samples 16 on a 32-sample checkpoint, alone and with --cull --cull_tighten on an all-occupied grid (near 2, far 6: the
    tightened rays are the rays, every byte as without --cull), and on the field's own grid: the span share is reported and smaller than 1"""
    from mipnerf_pl_amd import render_video
    from oracle import mipnerf_oracle as orc
    ckpt = str(tmp_path / "last.ckpt")
    _system(orc.make_params(seed=2, density_gain=40.0), 32).save_checkpoint(ckpt)
    common = ["--ckpt", ckpt, "--scale", "1", "--n_poses", "2", "--chunk_size", "160", "--precision", "fp32", "--base_size", "24", "24"]
    full, plain, allocc, some = (str(tmp_path / k) for k in ("full", "plain", "all", "some"))
    render_video.main(common + ["--out_dir", full])
    render_video.main(common + ["--out_dir", plain, "--render_samples", "16"])
    assert "cull:" not in capsys.readouterr().out
    ff, fp = _files(full), _files(plain)
    assert ff.keys() == fp.keys() and any(ff[k] != fp[k] for k in ff)                     # another sample count is another render
    render_video.main(common + ["--out_dir", allocc, "--render_samples", "16", "--cull", "--cull_tighten", "--cull_grid", "20", "--cull_threshold", "-1"])
    text = capsys.readouterr().out
    assert "cull: mean live share per frame: 1.0000 (2 frames); mean span share of the live rays: 1.0000" in text
    fa = _files(allocc)
    assert fp.keys() == fa.keys() and all(fp[k] == fa[k] for k in fp), [k for k in fp if fp[k] != fa[k]]
    render_video.main(common + ["--out_dir", some, "--render_samples", "16", "--cull", "--cull_tighten", "--cull_grid", "20", "--cull_threshold", "1e9",
                                "--cull_bound", "1.0"])
    text = capsys.readouterr().out              # nothing occupied inside +-1, everything outside it counts as occupied: a span with a hole
    assert "mean span share of the live rays:" in text and "mean live share per frame: 1.0000" in text


# ---- 7. quality on the golden 800 x 800 pose ----------------------------------------------------------------------------------------
def _psnr(a, b):
    return float(-10.0 * np.log10(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2) + 1e-30))


# fine-rgb PSNR against the scene's ground truth, measured on one MI355X (dB); the reference's frame has 30.440.  The field is foggy (2.1 %
# of the rays culled at this setting): its spans are long, see the span shares in DESIGN.md 4.8.
QUALITY_MEASURED = {
    ("fp32", "untightened_128"): 30.441, ("bf16", "untightened_128"): 30.450,
    ("fp32", "tightened_128"): 30.494, ("bf16", "tightened_128"): 30.501,
    ("fp32", "tightened_64"): 30.858, ("bf16", "tightened_64"): 30.869,
    ("fp32", "untightened_64"): 30.813, ("bf16", "untightened_64"): 30.824,
}
QUALITY_MARGIN = 0.05          # five times the 0.01 dB by which fp32 and bf16 differ on this frame


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_quality_of_the_tightened_golden_frame(precision):
    """threshold 0.03, dilate 0, 64^3 over +-2, outside_occupied=False (the whole-frame test's grid); span_samples stays 128 when the
    frame is rendered with 64 samples.  Each tightened render is held at its measured PSNR minus QUALITY_MARGIN."""
    from mipnerf_pl_amd import ops
    from mipnerf_pl_amd.datasets import RenderGen
    from mipnerf_pl_amd.evaluate import FrameEvaluator
    g = G.load_golden("frame_c5_800x800")
    size, N, chunk = int(g["cfg_size"]), int(g["cfg_num_samples"]), int(g["cfg_chunk"])
    assert N == 128
    dev = torch.device(DEV)
    gt = g["gt_u8"].astype(np.float32) / 255.0
    rays = RenderGen(float(g["focal"]), [size, size], scales=1, device=dev)[int(g["cfg_pose"])]
    figures = {}
    occ = None
    for tag, samples, tighten in (("untightened_128", 128, False), ("tightened_128", 128, True), ("tightened_64", 64, True),
                                  ("untightened_64", 64, False)):
        model = G.make_model(trained_params(), samples, precision)
        if occ is None:
            occ = ops.field_occupancy(model, grid=64, lo=-2.0, hi=2.0, threshold=0.03, dilate=0)
        ev = FrameEvaluator(model, size, size, chunk, True, dev, occupancy=occ, tighten=tighten, span_samples=128)
        ev.frame.outside_occupied = False
        with torch.no_grad():
            rgb, _, _ = ev.render(rays)
        figures[tag] = _psnr(rgb.cpu().numpy(), gt)
        figures[tag + "_live_share"] = ev.frame.live_count / float(size * size)
        if tighten:
            figures[tag + "_span_share"] = ev.frame.span_share
        del ev
    figures["ref_psnr_vs_scene"] = float(g["psnr_fine"])
    print(f"tightened golden frame {precision}: {figures}")
    G.record(f"frame_c5 tightened {precision}", **figures)
    assert abs(figures["untightened_128"] - QUALITY_MEASURED[(precision, "untightened_128")]) < QUALITY_MARGIN, figures
    for tag in ("tightened_128", "tightened_64"):
        measured = QUALITY_MEASURED[(precision, tag)]
        assert measured is not None, f"no measured value recorded for {tag}: {figures}"
        assert figures[tag] >= measured - QUALITY_MARGIN, (tag, figures)
    assert figures["tightened_128_live_share"] == figures["untightened_128_live_share"] == figures["tightened_64_live_share"]
