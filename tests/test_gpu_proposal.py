"""GPU: the density lattice as the proposal level (csrc/kernels_proposal.hip, ops.lattice_density, MipNerf._forward_native(proposal=),
model.GraphedFrame / CulledFrame(proposal=), the --proposal_grid command line).

  - ops.lattice_density torch.equal to the float32 restatement (tests/proposal_fixture.py) at the means ops.cast_rays returns;
  - _forward_native(proposal=) torch.equal, all five outputs of both levels, to the per-stage composition
    sample_t -> lattice_density -> volumetric_rendering_packed -> resample_t -> cast_ipe -> mlp -> volumetric_rendering;
  - GraphedFrame(proposal=): captured == eager == chunk by chunk, and it follows a swapped ProposalGrid;
  - CulledFrame(proposal=) plain, tightened, adaptive: live pixels torch.equal to GraphedFrame(proposal=) on the same rays;
  - refusals from Python and from the C entry point; the default path is untouched;
  - the golden 800 x 800 pose: PSNR against the scene with lattice proposals at 128^3 and 256^3 next to the two-level frame."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import adaptive_fixture as ax
import gpu_util as G
import proposal_fixture as px
import test_gpu_span as SP

pytestmark = pytest.mark.gpu
DEV = G.DEV
_CACHE = {}


# ---- 1. the stage on its own --------------------------------------------------------------------------------------------------------
LATTICES = {(2, 2, 2): ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0)), (5, 7, 9): ((-1.5, -0.7, -1.25), (1.25, 1.3, 1.0)),
            (64, 64, 64): ((-2.0, -2.0, -2.0), (2.0, 2.0, 2.0))}                      # [nz, ny, nx] -> box in (x, y, z) order


def _stage_rays(B, lo, hi, seed):
    """origins on |o| = 4 (outside every box), directions towards points of the box, near 2, far 6: every ray starts outside, most leave
    again.  Where B allows: ray 0 runs along +x INSIDE the hi faces of y and z (d_y = d_z = 0, so those coordinates of every mean are hi
    exactly) and ends exactly on the hi face of x (o_x + far = hi_x); the last ray is NaN."""
    rng = np.random.default_rng(seed)
    o = rng.normal(size=(B, 3))
    o = 4.0 * o / np.linalg.norm(o, axis=1, keepdims=True)
    target = np.asarray(lo) + (np.asarray(hi) - np.asarray(lo)) * rng.random((B, 3))
    d = target - o
    d = d / np.linalg.norm(d, axis=1, keepdims=True)
    near, far = np.full((B, 1), 2.0), np.full((B, 1), 6.0)
    if B >= 3:
        o[0], d[0] = (hi[0] - 6.0, hi[1], hi[2]), (1.0, 0.0, 0.0)
        o[B - 1] = np.nan
    one = np.ones((B, 1))
    f = [np.ascontiguousarray(a, np.float32) for a in (o, d, d, 1e-3 * one, one, near, far)]
    return G.to_dev(f)


@pytest.mark.parametrize("shape", list(LATTICES), ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("B,N", [(1, 1), (3, 85), (1, 257), (37, 64), (5, 1024)])
def test_lattice_density_equals_the_float32_restatement_at_the_cast_rays_means(shape, B, N):
    from mipnerf_pl_amd import ops
    lo, hi = LATTICES[shape]
    lat = px.random_lattice(shape, seed=B + N)
    grid = ops.ProposalGrid(torch.from_numpy(lat).to(DEV), lo, hi)
    assert grid.dims == (shape[2], shape[1], shape[0])
    rays = _stage_rays(B, lo, hi, seed=N)
    t = ops.sample_t(N, rays.near, rays.far, False, False)
    got = ops.lattice_density(grid, t, rays.origins, rays.directions, rays.radii)
    means, _ = ops.cast_rays(t, rays.origins, rays.directions, rays.radii)
    m = means.cpu().numpy()
    want = torch.from_numpy(px.trilinear_f32(lat, lo, hi, m))
    assert got.shape == (B, N) and torch.equal(got.cpu(), want)
    assert bool((got >= 0).all())
    if B >= 3:
        assert bool((got[B - 1] == 0).all())                                        # the NaN ray
        assert (m[0, :, 1] == np.float32(hi[1])).all() and (m[0, :, 2] == np.float32(hi[2])).all()     # inside two hi faces
        inside = np.isfinite(m).all(-1) & ((m >= np.float32(lo)) & (m <= np.float32(hi))).all(-1)
        assert inside.any() and (~inside).any()                                     # samples inside the box and outside it
    # the packed form the forward reads: colour 0 and the same density
    again = ops.lattice_density(grid, t, rays.origins, rays.directions, rays.radii)
    assert torch.equal(again, got)


# ---- 2. the chunk forward ------------------------------------------------------------------------------------------------------------
def _model(N, precision, **kw):
    return G.make_model(SP.trained_params(), N, precision, **kw)


def _proposal(kind, precision="fp32"):
    """'trained': the trained field's own 32^3 lattice over +-2; 'zero': all zero; 'slab': 50 on one z layer of a (5, 7, 9) lattice"""
    from mipnerf_pl_amd import ops
    key = ("proposal", kind, precision)
    if key not in _CACHE:
        if kind == "trained":
            _CACHE[key] = ops.field_proposal(_model(128, precision), grid=32, lo=-2.0, hi=2.0)
        elif kind == "zero":
            _CACHE[key] = ops.ProposalGrid(torch.zeros(16, 16, 16, device=DEV), -2.0, 2.0)
        else:
            lat = torch.zeros(5, 7, 9, device=DEV)
            lat[2] = 50.0
            _CACHE[key] = ops.ProposalGrid(lat, (-1.5, -1.0, -0.5), (1.5, 1.0, 0.5))
    return _CACHE[key]


def _composition(model, grid, rays, white_bkgd):
    """the two levels through the per-stage entry points"""
    from mipnerf_pl_amd import ops
    N = model.num_samples
    t0 = ops.sample_t(N, rays.near, rays.far, False, model.disparity)
    sigma = ops.lattice_density(grid, t0, rays.origins, rays.directions, rays.radii)
    packed = torch.cat([torch.zeros(*sigma.shape, 3, device=sigma.device), sigma[..., None]], dim=-1).contiguous()
    rgb0, dist0, acc0, w0 = ops.volumetric_rendering_packed(packed, t0, rays.directions, white_bkgd)
    t1 = ops.resample_t(t0, w0, False, model.resample_padding)
    enc = ops.cast_ipe(t1, rays.origins, rays.directions, rays.radii, model.min_deg_point, model.max_deg_point, precision=model.precision)
    venc = ops.pos_enc(rays.viewdirs, 0, model.deg_view)
    _, _, act = model.mlp(enc, venc, return_activated=True)
    rgb1, dist1, acc1, w1 = ops.volumetric_rendering(act[..., :3], act[..., 3:4], t1, rays.directions, white_bkgd)
    return [(rgb0, dist0, acc0, w0, t0), (rgb1, dist1, acc1, w1, t1)]


@pytest.mark.parametrize("kind", ["trained", "zero", "slab"])
@pytest.mark.parametrize("B,N", [(67, 64), (130, 128)])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_forward_with_a_proposal_is_the_per_stage_composition(precision, B, N, kind):
    from mipnerf_pl_amd import Rays
    _, all_rays, _, _ = SP.golden_rays(SP.RAY_SETS[1])
    rays = Rays(*[t[1000:1000 + B].contiguous() for t in all_rays])
    model = _model(N, precision)
    grid = _proposal(kind)
    ctx = model.mlp.native(torch.device(DEV))
    try:
        for white in (True, False):
            with torch.no_grad():
                want = _composition(model, grid, rays, white)
            bg = 1.0 if white else 0.0
            # level 0: colour 0 and the lattice's density -- the background times 1 - acc
            assert torch.equal(want[0][0], (bg * (1.0 - want[0][2]))[:, None].expand(-1, 3))
            if kind == "zero":
                assert bool((want[0][2] == 0).all()) and bool((want[0][3] == 0).all())
            else:
                assert bool((want[0][2] > 0).any())
            for fused_ipe in (1, 0):
                for fuse_small in (1, 0):
                    ctx.set_option(3, fused_ipe)
                    ctx.set_option(4, fuse_small)
                    with torch.no_grad():
                        got = model._forward_native(rays, False, white, proposal=grid)
                    for lvl in range(2):
                        for name, a, b in zip(G.NAMES, got[lvl], want[lvl]):
                            assert torch.equal(a, b), (white, fused_ipe, fuse_small, lvl, name, G.maxdiff(a, b))
    finally:
        ctx.set_option(3, 1)
        ctx.set_option(4, 1)
    # and it is not the two-level forward: the fine samples sit elsewhere
    with torch.no_grad():
        two = model._forward_native(rays, False, True)
    assert not torch.equal(two[1][4], got[1][4])


# ---- 3. frames -----------------------------------------------------------------------------------------------------------------------
def _outputs(frame):
    return [t.clone() for lv in range(len(frame.rgb)) for t in (frame.rgb[lv], frame.dist[lv], frame.acc[lv])]


def _chunked(model, rays, chunk, white, proposal=None):
    """the frame chunk by chunk through _forward_native: [rgb0, dist0, acc0, rgb1, dist1, acc1]"""
    from mipnerf_pl_amd import Rays
    n = rays.origins.shape[0]
    parts = []
    for lo in range(0, n, chunk):
        with torch.no_grad():
            kw = {} if proposal is None else {"proposal": proposal}
            parts.append(model._forward_native(Rays(*[t[lo:lo + chunk].contiguous() for t in rays]), False, white, **kw))
    return [torch.cat([p[lvl][k] for p in parts]) for lvl in range(2) for k in range(3)]


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_graphed_frame_with_a_proposal_captured_eager_and_chunk_by_chunk(precision):
    from mipnerf_pl_amd import Rays
    from mipnerf_pl_amd.model import GraphedFrame
    n, chunk = 150, 64
    _, all_rays, _, _ = SP.golden_rays(SP.RAY_SETS[1])
    rays = Rays(*[t[2000:2000 + n].contiguous() for t in all_rays])
    model = _model(64, precision)
    grid, other = _proposal("trained"), _proposal("slab")
    dev = torch.device(DEV)
    captured = GraphedFrame(model, n, chunk, True, dev, proposal=grid)
    eager = GraphedFrame(model, n, chunk, True, dev, capture=False, proposal=grid)
    with torch.no_grad():
        c_rgb, f_rgb, dist = captured(rays)
        eager(rays)
    assert captured.graph not in (None, False) and eager.graph is False
    assert c_rgb is captured.rgb[0] and f_rgb is captured.rgb[-1] and dist is captured.dist[-1]
    want = _chunked(model, rays, chunk, True, grid)
    for a, b, c in zip(_outputs(captured), _outputs(eager), want):
        assert torch.equal(a, c) and torch.equal(b, c)
    # rgb[0] is the lattice's silhouette against the white background
    assert torch.equal(captured.rgb[0], (1.0 - captured.acc[0])[:, None].expand(-1, 3))
    # another ProposalGrid object: the captured graph holds the old lattice's pointer, so the frame re-captures and follows
    old_graph = captured.graph
    captured.proposal = other
    with torch.no_grad():
        captured(rays)
    assert captured.graph is not old_graph and captured.graph not in (None, False)
    want_other = _chunked(model, rays, chunk, True, other)
    assert all(torch.equal(a, b) for a, b in zip(_outputs(captured), want_other))
    assert not torch.equal(want_other[3], want[3])
    # ... and back to none: the two-level frame
    captured.proposal = None
    with torch.no_grad():
        captured(rays)
    assert all(torch.equal(a, b) for a, b in zip(_outputs(captured), _chunked(model, rays, chunk, True)))


@pytest.mark.parametrize("mode", ["plain", "tightened", "adaptive"])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_culled_frame_with_a_proposal_is_the_graphed_frame_on_the_same_rays(precision, mode):
    from mipnerf_pl_amd import ops
    from mipnerf_pl_amd.model import CulledFrame, GraphedFrame
    n, chunk, N = 2048, 512, 64
    _, rays = SP.sphere_rays(n)
    occ, _ = SP.sphere_occupancy(64)
    model = _model(N, precision)
    grid = _proposal("trained")
    dev = torch.device(DEV)
    kw = dict(tighten=mode == "tightened", adaptive=mode == "adaptive")
    frame = CulledFrame(model, n, chunk, True, dev, occ, outside_occupied=False, proposal=grid, **kw)
    assert frame.proposal is grid
    with torch.no_grad():
        frame(rays)
    got = _outputs(frame)
    if mode == "plain":
        live = ops.ray_occupancy(occ, rays, N, outside_occupied=False)
        src = rays
    else:
        live, first, last, near, far = ops.ray_span(occ, rays, N, outside_occupied=False)
        src = rays._replace(near=near, far=far)
    lv = live.bool()
    assert torch.equal(frame.live, live) and 0 < frame.live_count == int(lv.sum()) < n
    if mode == "adaptive":
        buckets = ax.bucket(live.cpu().numpy(), first.cpu().numpy(), last.cpu().numpy(), N, frame.ladder)
        assert sum(c > 0 for c in frame.bucket_counts) >= 2
        jobs = [(_model(c, precision), torch.from_numpy(buckets == k).to(DEV)) for k, c in enumerate(frame.ladder) if frame.bucket_counts[k]]
    else:
        jobs = [(model, lv)]
    for m, mask in jobs:
        ref = GraphedFrame(m, n, chunk, True, dev, capture=False, proposal=grid)
        with torch.no_grad():
            ref(src)
        for a, b in zip(got, _outputs(ref)):
            assert torch.equal(a[mask], b[mask]), (mode, m.num_samples)
    for l_ in range(2):                                     # dead pixels: the existing rule
        assert (frame.rgb[l_][~lv] == 1.0).all() and (frame.acc[l_][~lv] == 0.0).all()
        assert torch.equal(frame.dist[l_][~lv], rays.near[~lv, 0])
    # the same frame without the lattice is another frame
    loose = CulledFrame(model, n, chunk, True, dev, occ, outside_occupied=False, **kw)
    assert loose.proposal is None
    with torch.no_grad():
        loose(rays)
    assert torch.equal(loose.live, live) and not torch.equal(loose.rgb[-1][lv], frame.rgb[-1][lv])


# ---- 4. the default path ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_frames_without_the_keyword_stay_the_two_level_forward(precision):
    from mipnerf_pl_amd import ops
    from mipnerf_pl_amd.model import CulledFrame, GraphedFrame
    n, chunk, N = 2048, 512, 64
    _, rays = SP.sphere_rays(n)
    occ, _ = SP.sphere_occupancy(64)
    model = _model(N, precision)
    dev = torch.device(DEV)
    want = _chunked(model, rays, chunk, True)
    plain = GraphedFrame(model, n, chunk, True, dev)
    culled = CulledFrame(model, n, chunk, True, dev, occ, outside_occupied=False)
    assert plain.proposal is None and culled.proposal is None
    with torch.no_grad():
        plain(rays)
        culled(rays)
    assert all(torch.equal(a, b) for a, b in zip(_outputs(plain), want))
    lv = ops.ray_occupancy(occ, rays, N, outside_occupied=False).bool()
    assert 0 < int(lv.sum()) < n
    assert all(torch.equal(a[lv], b[lv]) for a, b in zip(_outputs(culled), want))


# ---- 5. refusals -----------------------------------------------------------------------------------------------------------------------
def _c_forward_proposal(model, rays, grid):
    from mipnerf_pl_amd import _lib as L
    dev = torch.device(DEV)
    ctx = model.mlp.native(dev)
    B, N = rays.origins.shape[0], model.num_samples
    rp = L.RaysPtrs(*[t.data_ptr() for t in rays])
    outs = (L.LevelOut * 2)()
    keep = []
    for lvl in range(2):
        ts = [torch.empty(B, 3, device=dev), torch.empty(B, device=dev), torch.empty(B, device=dev), torch.empty(B, N, device=dev),
              torch.empty(B, N + 1, device=dev)]
        keep.append(ts)
        outs[lvl] = L.LevelOut(*[t.data_ptr() for t in ts])
    ws = ctx.workspace(B)
    rc = L.lib().mipnerf_forward_proposal(ctx.handle, B, C.byref(rp), grid.cdims, grid.clo, grid.chi, grid.lattice.data_ptr(), None, None, 1,
                                          model.precision, ws.data_ptr(), ws.numel(), outs, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, L.last_error()


def test_unbounded_and_one_level_models_are_refused_from_python_and_by_the_entry_point():
    from mipnerf_pl_amd import MipNerf, Rays
    from mipnerf_pl_amd import _lib as L
    from mipnerf_pl_amd import ops
    from mipnerf_pl_amd.model import CulledFrame, GraphedFrame
    _, all_rays, _, _ = SP.golden_rays(SP.RAY_SETS[1])
    rays = Rays(*[t[:8].contiguous() for t in all_rays])
    grid = _proposal("zero")
    dev = torch.device(DEV)
    torch.manual_seed(0)
    for model, word in ((MipNerf(num_samples=16, unbounded=True, precision="fp32").to(DEV).eval(), "unbounded"),
                        (MipNerf(num_samples=16, num_levels=1, precision="fp32").to(DEV).eval(), "two-level")):
        with pytest.raises(NotImplementedError, match=word):
            model._forward_native(rays, False, True, proposal=grid)
        with pytest.raises(NotImplementedError, match=word):
            GraphedFrame(model, 8, 8, True, dev, proposal=grid)
        rc, msg = _c_forward_proposal(model, rays, grid)
        assert rc == L.E_UNSUPPORTED and "forward_proposal" in msg, (rc, msg)
    with pytest.raises(NotImplementedError, match="unbounded"):
        ops.field_proposal(MipNerf(num_samples=16, unbounded=True, precision="fp32"), grid=8, lo=-1.0, hi=1.0)
    # a bounded two-level model passes the same call
    model = _model(16, "fp32")
    rc, msg = _c_forward_proposal(model, rays, grid)
    assert rc == L.OK, msg
    occ, _ = SP.sphere_occupancy(33)
    with pytest.raises(NotImplementedError, match="two-level"):
        CulledFrame(MipNerf(num_samples=16, num_levels=1, precision="fp32").to(DEV).eval(), 8, 8, True, dev, occ, proposal=grid)


# ---- 6. command line -------------------------------------------------------------------------------------------------------------------
def test_render_video_command_line_with_a_proposal_grid(tmp_path, capsys):
    from mipnerf_pl_amd import render_video
    from oracle import mipnerf_oracle as orc
    ckpt = str(tmp_path / "last.ckpt")
    SP._system(orc.make_params(seed=2, density_gain=40.0), 32).save_checkpoint(ckpt)
    out = str(tmp_path / "prop")
    render_video.main(["--ckpt", ckpt, "--scale", "1", "--n_poses", "2", "--chunk_size", "160", "--precision", "fp32", "--base_size", "24", "24",
                       "--out_dir", out, "--proposal_grid", "32"])
    text = capsys.readouterr().out
    assert "proposal: 32^3 density lattice over +-" in text and "built in" in text and text.count("proposal:") == 1 and "cull:" not in text
    files = SP._files(out)
    assert sum(k.endswith("_rgb.png") for k in files) == 2 and sum(k.endswith("_dist.png") for k in files) == 2


# ---- 7. quality on the golden 800 x 800 pose -------------------------------------------------------------------------------------------
# fine-rgb PSNR against the scene's ground truth, measured on one MI355X (dB).  The yardstick is the two-level frame: 30.441 (fp32) /
# 30.450 (bf16); the reference's frame has 30.440.  The lattice spans +-evaluate.cull_box of the frame (3.523 at 128^3, 3.495 at 256^3).
# Lattice proposals score LOWER than the two-level frame on this pose: by 0.029 / 0.028 dB at 128^3 and 0.022 / 0.022 dB at 256^3
# (fp32 / bf16).
QUALITY_MEASURED = {
    ("fp32", "proposal_128"): 30.411, ("bf16", "proposal_128"): 30.421,
    ("fp32", "proposal_256"): 30.418, ("bf16", "proposal_256"): 30.427,
}
TWO_LEVEL_MEASURED = {"fp32": 30.441, "bf16": 30.450}
QUALITY_MARGIN = SP.QUALITY_MARGIN          # 0.05 dB: five times the 0.01 dB by which fp32 and bf16 differ on this frame


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_quality_of_the_golden_frame_with_lattice_proposals(precision):
    """The two-level frame and lattice proposals at 128^3 and 256^3 over cull_box of the frame, same model and rays.  Each proposal render
    is held at its measured PSNR minus QUALITY_MARGIN; the gap to the two-level frame is recorded, not judged."""
    from mipnerf_pl_amd import evaluate
    from mipnerf_pl_amd.datasets import RenderGen
    from mipnerf_pl_amd.evaluate import FrameEvaluator
    g = G.load_golden("frame_c5_800x800")
    size, N, chunk = int(g["cfg_size"]), int(g["cfg_num_samples"]), int(g["cfg_chunk"])
    dev = torch.device(DEV)
    gt = g["gt_u8"].astype(np.float32) / 255.0
    rays = RenderGen(float(g["focal"]), [size, size], scales=1, device=dev)[int(g["cfg_pose"])]
    model = _model(N, precision)
    system = type("S", (), {"mip_nerf": model})()
    figures = {}
    for tag, n in (("two_level", None), ("proposal_128", 128), ("proposal_256", 256)):
        prop = None if n is None else evaluate.scene_proposal(system, [rays], grid=n, verbose=False)
        ev = FrameEvaluator(model, size, size, chunk, True, dev, proposal=prop)
        with torch.no_grad():
            rgb, _, _ = ev.render(rays)
        figures[tag] = SP._psnr(rgb.cpu().numpy(), gt)
        if prop is not None:
            figures[tag + "_gap_to_two_level"] = figures[tag] - figures["two_level"]
            figures[tag + "_bound"] = prop.hi[0]
        del ev, prop
    figures["ref_psnr_vs_scene"] = float(g["psnr_fine"])
    print(f"proposal golden frame {precision}: {figures}")
    G.record(f"frame_c5 proposal {precision}", **figures)
    assert abs(figures["two_level"] - TWO_LEVEL_MEASURED[precision]) < QUALITY_MARGIN, figures
    for tag in ("proposal_128", "proposal_256"):
        measured = QUALITY_MEASURED[(precision, tag)]
        assert measured is not None, f"no measured value recorded for {tag}: {figures}"
        assert figures[tag] >= measured - QUALITY_MARGIN, (tag, figures)
