"""GPU: adaptive sample counts for whole frames (csrc/kernels_bucket.hip, ops.bucket_rays / ops.gather_frame,
model.CulledFrame(adaptive=True)).

  - ops.bucket_rays against the numpy partition of tests/adaptive_fixture.py: counts, slots and all seven gathered fields exactly, padding
    slots untouched, two calls the same bytes -- at ray counts around the 64-ray alignment and the 1024-ray blocks;
  - ops.gather_frame equal to ops.scatter_frame on a one-bucket ladder;
  - CulledFrame(adaptive=True): the pixels of bucket b torch.equal to GraphedFrame over an independently built model with c_b samples on
    the rays with near / far replaced by near' / far'; dead pixels by the scatter rule with the original near; ladder (N,) equal to
    CulledFrame(tighten=True); an all-occupied grid equal to the plain frame; span_samples != the rendered count; the unbounded-scene model
    with a contracted grid; no stale sibling after an in-place parameter update;
  - the golden 800 x 800 pose: PSNR against the scene, held at its measured value minus the project's QUALITY_MARGIN."""
import numpy as np
import pytest
import torch

import adaptive_fixture as ax
import gpu_util as G
import test_gpu_cull360 as C360
import test_gpu_span as SP

pytestmark = pytest.mark.gpu
DEV = G.DEV
SENTINEL = -777.0
LADDERS = {1: (128,), 4: (32, 64, 96, 128), 8: tuple(range(16, 129, 16))}
_CACHE = {}


# ---- 1. the partition -------------------------------------------------------------------------------------------------------------------
def _spans(buckets, ladder):
    """live / first / last (numpy) that put ray i into buckets[i] (-1: dead) with S = N = ladder[-1]: a span of exactly c_b frusta, which
    needs c_b samples, starting as far in as it fits"""
    N = ladder[-1]
    n = len(buckets)
    live = buckets >= 0
    span = np.where(live, np.asarray(ladder)[np.maximum(buckets, 0)], 0)
    first = np.where(live, np.arange(n) % (N - span + 1), N)
    last = np.where(live, first + span - 1, -1)
    return live.astype(np.uint8), first.astype(np.int32), last.astype(np.int32)


def _patterns(n, B):
    i = np.arange(n)
    out = {"one_bucket": np.full(n, B // 2), "all_dead": np.full(n, -1), "cycling": i % (B + 1) - 1}
    if B >= 3:
        cyc = i % (B - 1)
        out["empty_middle"] = np.where(cyc >= B // 2, cyc + 1, cyc)
    exact = 1024 if n >= 1024 else 64                      # bucket 0 holds an exact multiple of 64 (and of 1024 where n allows)
    out["exact_multiple"] = np.where(i < exact, 0, B - 1 if B > 1 else -1)
    return out


def _random_rays(n, seed):
    from mipnerf_pl_amd import Rays
    gen = torch.Generator().manual_seed(seed)
    return Rays(*[torch.rand(n, k, generator=gen).to(DEV) for k in (3, 3, 3, 1, 1, 1, 1)])


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1024, 1025, 3 * 1024 + 17])
def test_bucket_rays_is_the_padded_stable_partition(n):
    from mipnerf_pl_amd import Rays, ops
    rays = _random_rays(n, n)
    host = [t.cpu() for t in rays]
    for B, ladder in LADDERS.items():
        rows = n + 64 * B
        for name, buckets in _patterns(n, B).items():
            live, first, last = _spans(buckets, ladder)
            assert np.array_equal(ax.bucket(live, first, last, ladder[-1], ladder), buckets), (name, B)
            counts, base, slot = ax.partition(live, first, last, ladder[-1], ladder)
            assert base[-1] <= rows
            d_live, d_first, d_last = (torch.from_numpy(a).to(DEV) for a in (live, first, last))
            results = []
            for _ in range(2):
                out = Rays(*[torch.full((rows, t.shape[1]), SENTINEL, device=DEV) for t in rays])
                d_slot = torch.full((n,), -5, dtype=torch.int32, device=DEV)
                got = ops.bucket_rays(d_live, d_first, d_last, rays, ladder[-1], ladder, out, d_slot)
                results.append((got, d_slot.cpu(), [t.cpu() for t in out]))
            got, got_slot, got_out = results[0]
            assert got == counts, (name, B, got, counts)
            assert np.array_equal(got_slot.numpy(), slot), (name, B)
            lv = torch.from_numpy(live.astype(bool))
            where = torch.from_numpy(slot[live.astype(bool)])
            for k, src, dst in zip(Rays._fields, host, got_out):
                want = torch.full_like(dst, SENTINEL)
                want[where] = src[lv]
                assert torch.equal(dst, want), (name, B, k)          # every live ray at its slot, every other row untouched
            assert results[1][0] == got and torch.equal(results[1][1], got_slot)
            assert all(torch.equal(a, b) for a, b in zip(results[1][2], got_out))
    # a skipped field stays untouched, and the bindings refuse what the kernel must not see
    ladder = LADDERS[4]
    live, first, last = _spans(_patterns(n, 4)["cycling"], ladder)
    d_live, d_first, d_last = (torch.from_numpy(a).to(DEV) for a in (live, first, last))
    d_slot = torch.empty(n, dtype=torch.int32, device=DEV)
    short = Rays(*[torch.empty(n + 64 * 4 - 1, t.shape[1], device=DEV) for t in rays])
    with pytest.raises(ValueError, match="n \\+ 64 \\* B"):
        ops.bucket_rays(d_live, d_first, d_last, rays, 128, ladder, short, d_slot)
    with pytest.raises(ValueError, match="ladder"):
        ops.bucket_rays(d_live, d_first, d_last, rays, 128, (32, 32, 128), Rays(*[torch.empty(n + 192, t.shape[1], device=DEV) for t in rays]), d_slot)


def test_bucket_rays_with_differing_counts_and_no_rays():
    """S = 128 frusta with a 64-sample ladder and the reverse, every span length at every start; and zero rays"""
    from mipnerf_pl_amd import Rays, ops
    for S, ladder in ((128, (16, 32, 48, 64)), (64, (32, 64, 96, 128)), (100, (1, 2, 3, 4, 5, 6, 7))):
        first, last = np.triu_indices(S)                                    # every 0 <= first <= last < S
        n = len(first)
        live = (np.arange(n) % 7 != 3).astype(np.uint8)
        first, last = first.astype(np.int32), last.astype(np.int32)
        counts, base, slot = ax.partition(live, first, last, S, ladder)
        rays = _random_rays(n, S)
        out = Rays(*[torch.full((n + 64 * len(ladder), t.shape[1]), SENTINEL, device=DEV) for t in rays])
        d_slot = torch.empty(n, dtype=torch.int32, device=DEV)
        got = ops.bucket_rays(*(torch.from_numpy(a).to(DEV) for a in (live, first, last)), rays, S, ladder, out, d_slot)
        assert got == counts and min(counts) > 0 and np.array_equal(d_slot.cpu().numpy(), slot)
        lv = torch.from_numpy(live.astype(bool)).to(DEV)
        assert torch.equal(out.near[torch.from_numpy(slot[live.astype(bool)]).to(DEV)], rays.near[lv])
    none = _random_rays(0, 0)
    assert ops.bucket_rays(torch.empty(0, dtype=torch.uint8, device=DEV), torch.empty(0, dtype=torch.int32, device=DEV),
                           torch.empty(0, dtype=torch.int32, device=DEV), none, 128, (64, 128),
                           Rays(*[torch.empty(128, t.shape[1], device=DEV) for t in none]), torch.empty(0, dtype=torch.int32, device=DEV)) == [0, 0]


# ---- 2. the way back ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("white_bkgd", [True, False])
def test_gather_frame_is_scatter_frame_on_a_one_bucket_ladder(white_bkgd):
    from mipnerf_pl_amd import Rays, ops
    n = 3 * 1024 + 17
    rays = _random_rays(n, 5)
    gen = torch.Generator().manual_seed(9)
    for case in ("some", "none", "all"):
        live = {"some": (torch.rand(n, generator=gen) < 0.6), "none": torch.zeros(n, dtype=torch.bool), "all": torch.ones(n, dtype=torch.bool)}[case]
        live = live.to(torch.uint8).to(DEV)
        first = torch.zeros(n, dtype=torch.int32, device=DEV)
        last = torch.full((n,), 127, dtype=torch.int32, device=DEV)
        comp_rays = Rays(*[torch.zeros(n + 64, t.shape[1], device=DEV) for t in rays])
        index = torch.zeros(n, dtype=torch.int32, device=DEV)
        slot = torch.zeros(n, dtype=torch.int32, device=DEV)
        count = ops.compact_rays(live, rays, Rays(*[t[:n] for t in comp_rays]), index)
        assert ops.bucket_rays(live, first, last, rays, 128, (128,), comp_rays, slot) == [count]
        assert count == {"some": int(live.sum()), "none": 0, "all": n}[case]
        # the slots are the inverse of the index
        assert torch.equal(slot[index[:count].long()], torch.arange(count, dtype=torch.int32, device=DEV)) and int((slot < 0).sum()) == n - count
        compact = [(torch.rand(n + 64, 3, generator=gen).to(DEV), torch.rand(n + 64, generator=gen).to(DEV), torch.rand(n + 64, generator=gen).to(DEV))
                   for _ in range(2)]
        a, b = ([(torch.full((n, 3), SENTINEL, device=DEV), torch.full((n,), SENTINEL, device=DEV), torch.full((n,), SENTINEL, device=DEV))
                 for _ in range(2)] for _ in range(2))
        ops.scatter_frame(index, count, compact, a, live, rays.near, white_bkgd)
        ops.gather_frame(slot, compact, b, rays.near, white_bkgd)
        for la, lb in zip(a, b):
            for ta, tb in zip(la, lb):
                assert torch.equal(ta, tb) and not (tb == SENTINEL).any()
        dead = live == 0
        if dead.any():
            assert (b[1][0][dead] == (1.0 if white_bkgd else 0.0)).all() and (b[1][2][dead] == 0.0).all()
            assert torch.equal(b[1][1][dead], rays.near[dead, 0])
    with pytest.raises(ValueError, match="level counts"):
        ops.gather_frame(slot, compact[:1], b, rays.near, white_bkgd)


# ---- 3. frames ------------------------------------------------------------------------------------------------------------------------------
def _outputs(frame):
    return [t.clone() for lv in range(len(frame.rgb)) for t in (frame.rgb[lv], frame.dist[lv], frame.acc[lv])]


def _check_frame(frame, got, rays, occ, S, make, chunk, white_bkgd, span_kw):
    """the adaptive frame's outputs `got` against the fixture's partition of the device's own spans and, per bucket, against GraphedFrame
    over make(c_b) on the tightened rays; returns (live mask, buckets, counts)"""
    from mipnerf_pl_amd import ops
    from mipnerf_pl_amd.model import GraphedFrame
    n = rays.origins.shape[0]
    live, first, last, near, far = ops.ray_span(occ, rays, S, **span_kw)
    assert torch.equal(frame.live, live) and torch.equal(frame.first, first) and torch.equal(frame.last, last)
    assert torch.equal(frame.near_span, near) and torch.equal(frame.far_span, far)
    args = (live.cpu().numpy(), first.cpu().numpy(), last.cpu().numpy(), S, frame.ladder)
    buckets = ax.bucket(*args)
    counts, base, slot = ax.partition(*args)
    assert frame.bucket_counts == counts and sum(counts) == frame.live_count == int(live.sum())
    assert np.array_equal(frame.slot[:n].cpu().numpy(), slot)
    assert frame.sample_share == pytest.approx(ax.sample_share(*args), abs=1e-12)
    dev = torch.device(DEV)
    for k, c in enumerate(frame.ladder):
        if counts[k] == 0:
            continue
        ref = GraphedFrame(make(c), n, chunk, white_bkgd, dev, capture=False)
        with torch.no_grad():
            ref(rays._replace(near=near, far=far))
        mask = torch.from_numpy(buckets == k).to(DEV)
        for a, b in zip(got, _outputs(ref)):
            assert torch.equal(a[mask], b[mask]), (k, c)
    lv = live.bool()
    for l_ in range(len(frame.rgb)):                        # dead pixels: the scatter rule with the ORIGINAL near
        assert (frame.rgb[l_][~lv] == (1.0 if white_bkgd else 0.0)).all() and (frame.acc[l_][~lv] == 0.0).all()
        assert torch.equal(frame.dist[l_][~lv], rays.near[~lv, 0])
    return lv, buckets, counts


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_adaptive_frame_is_the_sibling_renderer_on_the_tightened_rays_per_bucket(precision):
    from mipnerf_pl_amd import ops
    from mipnerf_pl_amd.model import CulledFrame
    chunk, n = 1024, 3 * 1024 + 17
    rays, N = SP._frame_rays(n)
    params = SP.trained_params()
    model = G.make_model(params, N, precision)
    occ = ops.occupancy_grid(SP.trained_lattice(), 0.1, SP.LO, SP.HI, dilate=0)
    dev = torch.device(DEV)
    frame = CulledFrame(model, n, chunk, True, dev, occ, outside_occupied=False, adaptive=True)
    assert frame.adaptive is True and frame.tighten is True and frame.ladder == (32, 64, 96, 128) and frame.span_samples == N
    with torch.no_grad():
        c_rgb, f_rgb, dist = frame(rays)
    got = _outputs(frame)
    assert c_rgb is frame.rgb[0] and f_rgb is frame.rgb[-1] and dist is frame.dist[-1]
    lv, buckets, counts = _check_frame(frame, got, rays, occ, N, lambda c: G.make_model(params, c, precision), chunk, True,
                                       dict(outside_occupied=False))
    assert sum(c > 0 for c in counts) >= 2 and 0 < frame.live_count < n
    assert 0.25 <= frame.sample_share < 1.0 and frame.sample_share >= frame.span_share
    # a second frame through the same object: same bits
    with torch.no_grad():
        frame(rays)
    assert all(torch.equal(a, b) for a, b in zip(_outputs(frame), got))
    # without the flag nothing of this exists, and a ladder alone is refused
    loose = CulledFrame(model, n, chunk, True, dev, occ, outside_occupied=False, tighten=True)
    assert loose.adaptive is False and loose.ladder is None and loose.bucket_counts is None and not hasattr(loose, "slot")
    with pytest.raises(ValueError, match="adaptive"):
        CulledFrame(model, n, chunk, True, dev, occ, ladder=(64, 128))
    with pytest.raises(ValueError, match="strictly increasing"):
        CulledFrame(model, n, chunk, True, dev, occ, adaptive=True, ladder=(64, 96))


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_one_entry_ladder_is_the_tightened_frame(precision):
    from mipnerf_pl_amd import ops
    from mipnerf_pl_amd.model import CulledFrame
    chunk, n = 1024, 3 * 1024 + 17
    rays, N = SP._frame_rays(n)
    model = G.make_model(SP.trained_params(), N, precision)
    occ = ops.occupancy_grid(SP.trained_lattice(), 0.1, SP.LO, SP.HI, dilate=0)
    dev = torch.device(DEV)
    tight = CulledFrame(model, n, chunk, True, dev, occ, outside_occupied=False, tighten=True)
    frame = CulledFrame(model, n, chunk, True, dev, occ, outside_occupied=False, adaptive=True, ladder=(N,))
    with torch.no_grad():
        tight(rays)
        frame(rays)
    assert frame.bucket_counts == [tight.live_count] and frame.sample_share == 1.0 and 0 < tight.live_count < n
    assert all(torch.equal(a, b) for a, b in zip(_outputs(frame), _outputs(tight)))


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_all_occupied_adaptive_frame_is_the_plain_frame(precision):
    """near 2 and far 6: near' and far' are exact, every span is full, every ray lands in the top bucket"""
    from mipnerf_pl_amd import ops
    from mipnerf_pl_amd.model import CulledFrame, GraphedFrame
    chunk, n = 1024, 3 * 1024 + 17
    rays, N = SP._frame_rays(n)
    model = G.make_model(SP.trained_params(), N, precision)
    everything = ops.occupancy_grid(SP.trained_lattice(), -1.0, SP.LO, SP.HI, dilate=0)
    dev = torch.device(DEV)
    plain = GraphedFrame(model, n, chunk, False, dev, capture=False)
    frame = CulledFrame(model, n, chunk, False, dev, everything, adaptive=True)
    with torch.no_grad():
        plain(rays)
        frame(rays)
    assert frame.live_count == n and frame.bucket_counts == [0, 0, 0, n] and frame.sample_share == 1.0
    assert all(torch.equal(a, b) for a, b in zip(_outputs(frame), _outputs(plain)))


def test_span_samples_128_with_a_64_sample_model():
    from mipnerf_pl_amd import ops
    from mipnerf_pl_amd.model import CulledFrame
    chunk, n = 1024, 3 * 1024 + 17
    rays, N = SP._frame_rays(n)
    assert N == 128
    params = SP.trained_params()
    model64 = G.make_model(params, 64, "fp32")
    occ = ops.occupancy_grid(SP.trained_lattice(), 0.1, SP.LO, SP.HI, dilate=0)
    frame = CulledFrame(model64, n, chunk, True, torch.device(DEV), occ, outside_occupied=False, adaptive=True, span_samples=128,
                        ladder=(16, 32, 48, 64))
    with torch.no_grad():
        frame(rays)
    assert frame.span_samples == 128 and frame.ladder == (16, 32, 48, 64)
    _, _, counts = _check_frame(frame, _outputs(frame), rays, occ, 128, lambda c: G.make_model(params, c, "fp32"), chunk, True,
                                dict(outside_occupied=False))
    assert sum(c > 0 for c in counts) >= 2


def test_adaptive_frame_of_the_unbounded_scene_model():
    """test_gpu_cull360's smallest frame: 1000 golden rays, chunk 300, the contracted 64^3 grid at its threshold"""
    from mipnerf_pl_amd.model import CulledFrame
    gold = G.load_golden(C360.FRAME_SET)
    _, rays = C360.ray_set(C360.FRAME_SET)
    n, N, chunk = int(gold["batch"]), int(gold["num_samples"]), 300
    model = C360.model360("fp32")
    occ = C360.frame_occupancy(C360.FRAME_THRESHOLD)
    frame = CulledFrame(model, n, chunk, True, torch.device(DEV), occ, adaptive=True)
    assert frame.ladder == (24, 48, 72, 96) and N == 96
    with torch.no_grad():
        frame(rays)
    _, _, counts = _check_frame(frame, _outputs(frame), rays, occ, N, lambda c: C360.model360("fp32", c), chunk, True, {})
    assert 0 < frame.live_count < n and sum(c > 0 for c in counts) >= 2


def test_siblings_follow_an_in_place_parameter_update():
    from mipnerf_pl_amd import ops
    from mipnerf_pl_amd.model import CulledFrame
    chunk, n = 1024, 3 * 1024 + 17
    rays, N = SP._frame_rays(n)
    model = G.make_model(SP.trained_params(), N, "bf16")
    occ = ops.occupancy_grid(SP.trained_lattice(), 0.1, SP.LO, SP.HI, dilate=0)
    dev = torch.device(DEV)
    frame = CulledFrame(model, n, chunk, True, dev, occ, outside_occupied=False, adaptive=True)
    with torch.no_grad():
        frame(rays)
        before = _outputs(frame)
        for p in model.parameters():
            p.mul_(1.03125)
        frame(rays)
    after = _outputs(frame)
    fresh = CulledFrame(model, n, chunk, True, dev, occ, outside_occupied=False, adaptive=True)
    with torch.no_grad():
        fresh(rays)
    assert fresh.bucket_counts == frame.bucket_counts and sum(c > 0 for c in frame.bucket_counts) >= 2
    want = _outputs(fresh)
    buckets = ax.bucket(frame.live.cpu().numpy(), frame.first.cpu().numpy(), frame.last.cpu().numpy(), N, frame.ladder)
    for k in range(len(frame.ladder)):
        mask = torch.from_numpy(buckets == k).to(DEV)
        if not mask.any():
            continue
        assert all(torch.equal(a[mask], b[mask]) for a, b in zip(after, want)), k
        assert not torch.equal(after[3][mask], before[3][mask]), k                      # the update reached this bucket's sibling
    # ... and against models that never saw the old parameters
    state = {k: v.detach().cpu().numpy() for k, v in model.mlp.state_dict().items()}
    _check_frame(frame, after, rays, occ, N, lambda c: G.make_model(state, c, "bf16"), chunk, True, dict(outside_occupied=False))


def test_render_video_command_line_with_adaptive_counts(tmp_path, capsys):
    """--cull --cull_adaptive on an all-occupied grid (near 2, far 6: every span is full, every ray in the top bucket): every byte as
    without --cull, sample share 1; on a grid with a hole the sample share is reported and below 1; a ladder that does not end at the
    rendered count is refused"""
    from mipnerf_pl_amd import render_video
    from oracle import mipnerf_oracle as orc
    ckpt = str(tmp_path / "last.ckpt")
    SP._system(orc.make_params(seed=2, density_gain=40.0), 32).save_checkpoint(ckpt)
    common = ["--ckpt", ckpt, "--scale", "1", "--n_poses", "2", "--chunk_size", "160", "--precision", "fp32", "--base_size", "24", "24",
              "--render_samples", "16"]
    plain, allocc, some = (str(tmp_path / k) for k in ("plain", "all", "some"))
    render_video.main(common + ["--out_dir", plain])
    capsys.readouterr()
    render_video.main(common + ["--out_dir", allocc, "--cull", "--cull_adaptive", "--cull_grid", "20", "--cull_threshold", "-1"])
    text = capsys.readouterr().out
    assert ("cull: mean live share per frame: 1.0000 (2 frames); mean span share of the live rays: 1.0000; "
            "mean sample share of the live rays: 1.0000") in text
    fp, fa = SP._files(plain), SP._files(allocc)
    assert fp.keys() == fa.keys() and all(fp[k] == fa[k] for k in fp), [k for k in fp if fp[k] != fa[k]]
    render_video.main(common + ["--out_dir", some, "--cull", "--cull_adaptive", "--cull_ladder", "2", "4", "8", "16", "--cull_grid", "20",
                                "--cull_threshold", "1e9", "--cull_bound", "1.0"])
    text = capsys.readouterr().out              # nothing occupied inside +-1, everything outside it counts as occupied: a span with a hole
    assert "mean live share per frame: 1.0000" in text and "mean sample share of the live rays:" in text
    with pytest.raises(SystemExit, match="--cull_ladder"):
        render_video.main(common + ["--out_dir", some, "--cull", "--cull_adaptive", "--cull_ladder", "8", "32"])


# ---- 4. quality on the golden 800 x 800 pose -------------------------------------------------------------------------------------------
# fine-rgb PSNR of the adaptive frame (default ladder) against the scene's ground truth, measured on one MI355X (dB), next to the same
# run's untightened frame (test_gpu_span.QUALITY_MEASURED: 30.441 / 30.450; the reference's frame has 30.440).  Live share 0.979, sample
# share 0.635 (6.7 / 37.6 / 50.7 / 5.0 % of the live rays at 32 / 64 / 96 / 128 samples), span share 0.516.
QUALITY_MEASURED = {"fp32": 30.671, "bf16": 30.681}


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_quality_of_the_adaptive_golden_frame(precision):
    """the grid of test_quality_of_the_tightened_golden_frame (threshold 0.03, dilate 0, 64^3 over +-2, outside_occupied=False),
    span_samples 128, the default ladder.  The adaptive render is held at its measured PSNR minus test_gpu_span.QUALITY_MARGIN."""
    from mipnerf_pl_amd import ops
    from mipnerf_pl_amd.datasets import RenderGen
    from mipnerf_pl_amd.evaluate import FrameEvaluator
    g = G.load_golden("frame_c5_800x800")
    size, N, chunk = int(g["cfg_size"]), int(g["cfg_num_samples"]), int(g["cfg_chunk"])
    assert N == 128
    dev = torch.device(DEV)
    gt = g["gt_u8"].astype(np.float32) / 255.0
    rays = RenderGen(float(g["focal"]), [size, size], scales=1, device=dev)[int(g["cfg_pose"])]
    model = G.make_model(SP.trained_params(), N, precision)
    occ = ops.field_occupancy(model, grid=64, lo=-2.0, hi=2.0, threshold=0.03, dilate=0)
    figures = {}
    for tag, adaptive in (("untightened_128", False), ("adaptive_128", True)):
        ev = FrameEvaluator(model, size, size, chunk, True, dev, occupancy=occ, span_samples=128, adaptive=adaptive)
        ev.frame.outside_occupied = False
        with torch.no_grad():
            rgb, _, _ = ev.render(rays)
        figures[tag] = SP._psnr(rgb.cpu().numpy(), gt)
        figures[tag + "_live_share"] = ev.frame.live_count / float(size * size)
        if adaptive:
            figures["adaptive_128_sample_share"] = ev.frame.sample_share
            figures["adaptive_128_span_share"] = ev.frame.span_share
            for k, c in enumerate(ev.frame.bucket_counts):
                figures[f"adaptive_128_bucket{k}_share"] = c / float(max(1, ev.frame.live_count))
        del ev
    figures["ref_psnr_vs_scene"] = float(g["psnr_fine"])
    print(f"adaptive golden frame {precision}: {figures}")
    G.record(f"frame_c5 adaptive {precision}", **figures)
    assert abs(figures["untightened_128"] - SP.QUALITY_MEASURED[(precision, "untightened_128")]) < SP.QUALITY_MARGIN, figures
    measured = QUALITY_MEASURED[precision]
    assert measured is not None, f"no measured value recorded: {figures}"
    assert figures["adaptive_128"] >= measured - SP.QUALITY_MARGIN, figures
    assert figures["adaptive_128_live_share"] == figures["untightened_128_live_share"]
    assert figures["adaptive_128_span_share"] <= figures["adaptive_128_sample_share"] <= 1.0
