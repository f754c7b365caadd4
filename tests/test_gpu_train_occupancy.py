"""GPU: span training -- the occupancy grid a training run refreshes (mipnerf_occupancy_refresh, ops.occupancy_refresh,
train_occupancy.TrainOccupancy) and the occupied spans inside the training step (GraphedTrainStep(occupancy=...), Trainer._tighten).

1. the refresh against a float32 restatement of its rule in numpy, NaN / inf included, eagerly and replayed from a graph;
2. the spans inside the step, bounded and unbounded: the static buffers are `ops.ray_span` of the step's rays and the step equals a step
   without a grid whose batch source tightens the rays itself, bit for bit;
3. a captured step reads the grid's words where they live: a refresh between two replays is seen by the next one;
4. off means off (checkpoint keys, CSV header), and a full grid is the old path bit for bit;
5. resume is exact, with the refresh falling on either side of the checkpoint;
6. the eager routes; 7. two ranks."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import dataset_fixture as fx
from tests import scene360_fixture as sf

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B, N = 128, 64


def _hp(data, out, dataset_name, **kw):
    from mipnerf_pl_amd import config as cfg
    hp = dict(cfg.DEFAULTS, data_path=str(data), out_dir=str(out), dataset_name=dataset_name, exp_name="t")
    if dataset_name == "llff":
        hp.update(cfg.SCENE360_PRESET, exp_name="t", factor=2)
    hp.update({"train.batch_size": B, "nerf.num_samples": N, "val.check_interval": 1000, "val.sample_num": 1,
               "val.chunk_size": 4096, "optimizer.lr_delay_steps": 0, "train.randomized": False})
    hp.update({k.replace("__", "."): v for k, v in kw.items()})
    return hp


def _occ_kw(**kw):
    base = {"train.occupancy.enabled": True, "train.occupancy.grid": 16, "train.occupancy.interval": 3}
    base.update({"train.occupancy." + k: v for k, v in kw.items()})
    return base


def _run(args, timeout=600, env_extra=None):
    env = dict(os.environ, **(env_extra or {}))
    out = subprocess.run([sys.executable, "-m"] + args, capture_output=True, text=True, timeout=timeout, cwd=REPO, env=env)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    return out.stdout


def _state(ck):
    (s,) = ck["optimizer_states"][0]["state"].values()
    return ck["state_dict"], s["exp_avg"], s["exp_avg_sq"], int(s["step"])


def _words(t):
    return t.view(torch.int32)


# ---- 1. the refresh against numpy ---------------------------------------------------------------------------------------------
def rule_decay_max(fresh, running, decay):
    """The header's rule in float32: d = decay * running (one multiply); the new value is fresh where fresh > d or either is NaN, else d."""
    with np.errstate(invalid="ignore"):
        d = (np.float32(decay) * running.astype(np.float32)).astype(np.float32)
        take = (fresh > d) | np.isnan(fresh) | np.isnan(d)
    return np.where(take, fresh, d).astype(np.float32)


def _lattices(dims, seed):
    """fresh and running [nz, ny, nx] around the threshold, with NaN and +-inf in both (alone, and at the same point)."""
    nx, ny, nz = dims
    rng = np.random.default_rng(seed)
    n = nx * ny * nz
    fresh = rng.normal(0.3, 0.5, n).astype(np.float32)
    running = rng.normal(0.3, 0.5, n).astype(np.float32)
    special = [np.nan, np.inf, -np.inf]
    for i in range(min(n, 8)):          # point i: a special value in fresh (i < 3), in running (3 <= i < 6), in both (6, 7)
        p = (i * 7919) % n if n > 8 else i
        if i < 3:
            fresh[p] = special[i]
        elif i < 6:
            running[p] = special[i - 3]
        else:
            fresh[p], running[p] = (np.nan, np.inf) if i == 6 else (np.inf, np.nan)
    return fresh.reshape(nz, ny, nx), running.reshape(nz, ny, nx)


def _same_lattice(a, b):
    nan = torch.isnan(a)
    return torch.equal(nan, torch.isnan(b)) and torch.equal(a[~nan], b[~nan])


@pytest.mark.parametrize("dims", [(70, 5, 4), (33, 3, 3), (2, 2, 2)])
@pytest.mark.parametrize("decay", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("dilate", [0, 1])
def test_refresh_equals_the_rule_restated_in_numpy(dims, decay, dilate):
    from mipnerf_pl_amd import ops
    nx, ny, nz = dims
    thr, lo, hi = 0.3, (-1.0,) * 3, (1.0,) * 3
    f_np, r_np = _lattices(dims, seed=nx + 10 * dilate)
    assert np.isnan(f_np).any() and np.isinf(f_np).any() and np.isnan(r_np).any() and np.isinf(r_np).any()
    want1 = rule_decay_max(f_np, r_np, decay)
    want2 = rule_decay_max(f_np, want1, decay)

    def fresh_state():
        bits = torch.full((nz - 1, ny - 1, (nx - 1 + 31) // 32), 0x5A5A5A5A, dtype=torch.int32, device=DEV).view(torch.uint32)
        occ = ops.Occupancy(bits, dims, lo, hi)
        occ.threshold, occ.dilate = thr, dilate
        scratch = torch.empty_like(bits) if dilate else None
        return occ, torch.from_numpy(f_np).to(DEV), torch.from_numpy(r_np).to(DEV), scratch
    occ, fresh, running, scratch = fresh_state()
    ptr = occ.bits.data_ptr()
    assert ops.occupancy_refresh(occ, fresh, running, decay, scratch=scratch) is occ
    assert occ.bits.data_ptr() == ptr
    assert _same_lattice(running, torch.from_numpy(want1).to(DEV))
    assert torch.equal(fresh.cpu().view(torch.int32), torch.from_numpy(f_np).view(torch.int32))           # fresh is only read
    built = ops.occupancy_grid(running, thr, lo, hi, dilate=dilate)
    assert torch.equal(_words(occ.bits), _words(built.bits))
    # a second identical run on fresh copies: the same bytes
    occ2, fresh2, running2, scratch2 = fresh_state()
    ops.occupancy_refresh(occ2, fresh2, running2, decay, scratch=scratch2)
    assert torch.equal(running.view(torch.int32), running2.view(torch.int32)) and torch.equal(_words(occ.bits), _words(occ2.bits))
    # the second application, eagerly
    ops.occupancy_refresh(occ, fresh, running, decay, scratch=scratch)
    assert _same_lattice(running, torch.from_numpy(want2).to(DEV))
    # captured and replayed twice = two applications
    occ3, fresh3, running3, scratch3 = fresh_state()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):              # (warm-up on a side stream, then the state the capture starts from)
        ops.occupancy_refresh(occ3, fresh3, running3, decay, scratch=scratch3)
    torch.cuda.current_stream().wait_stream(s)
    running3.copy_(torch.from_numpy(r_np))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.occupancy_refresh(occ3, fresh3, running3, decay, scratch=scratch3)
    g.replay()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(running3.view(torch.int32), running.view(torch.int32)) and torch.equal(_words(occ3.bits), _words(occ.bits))


def test_refresh_refuses_what_it_cannot_do():
    from mipnerf_pl_amd import ops
    bits = torch.zeros(3, 3, 1, dtype=torch.int32, device=DEV).view(torch.uint32)
    lat = torch.zeros(4, 4, 4, device=DEV)
    with pytest.raises(ValueError, match="threshold"):
        ops.occupancy_refresh(ops.Occupancy(bits, (4, 4, 4), (-1,) * 3, (1,) * 3), lat, lat.clone(), 0.5)
    occ = ops.Occupancy(bits, (4, 4, 4), (-1,) * 3, (1,) * 3)
    occ.threshold, occ.dilate = 0.0, 0
    with pytest.raises(ValueError, match="overlap"):
        ops.occupancy_refresh(occ, lat, lat, 0.5)
    with pytest.raises(ValueError, match="decay"):
        ops.occupancy_refresh(occ, lat, lat.clone(), 1.5)
    with pytest.raises(ValueError, match="lattice"):
        ops.occupancy_refresh(occ, lat[:3], lat.clone(), 0.5)


# ---- 2. / 3. spans inside the step -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scenes(tmp_path_factory):
    root = tmp_path_factory.mktemp("span_scenes")
    bounded = fx.write_multicam_scene(str(root / "ms"), counts=(("train", 3), ("val", 1), ("test", 1)), base=16, scales=2)
    unbounded = sf.write_scene360_llff(str(root / "s360"), views=6, w=24, h=18, steps=32)
    return {"bounded": (bounded, "multi_blender"), "unbounded": (unbounded, "llff")}


def sphere_occupancy(system, kind, grid=32):
    """A fixed analytic sphere: lattice value R - |p - c|, threshold 0.  Bounded: a world box that holds every training ray
    (`evaluate.cull_box`), so nothing is live for leaving the grid; unbounded: [-2, 2]^3 of the contracted space, the sphere inside the
    unit ball, where contraction is the identity."""
    from mipnerf_pl_amd import evaluate, ops
    ds = system.train_dataset
    if kind == "bounded":
        bound = evaluate.cull_box((ds.image_rays(i)[0] for i in range(ds.n_examples)), grid)
        centre, R, space = (0.1, 0.0, 0.05), 0.5, None
    else:
        bound, centre, R, space = 2.0, (0.05, 0.0, 0.1), 0.6, "contracted"
    ax = torch.linspace(-bound, bound, grid, device=DEV)
    z, y, x = torch.meshgrid(ax, ax, ax, indexing="ij")
    lattice = R - torch.sqrt((x - centre[0]) ** 2 + (y - centre[1]) ** 2 + (z - centre[2]) ** 2)
    occ = ops.occupancy_grid(lattice.contiguous(), 0.0, -bound, bound, dilate=0)
    occ.space = space
    return occ, lattice.contiguous()


def _make_step(scenes, kind, tmp_path, use_graph, with_occupancy, tighten_in_source=False, grid=32):
    """A GraphedTrainStep on the scene's training split whose batch comes from ops.gather_train_batch with the batch index read from the
    optimiser's device step counter (train.Trainer's arrangement)."""
    from mipnerf_pl_amd import ops
    from mipnerf_pl_amd.system import MipNeRFSystem
    from mipnerf_pl_amd.train import epoch_order, setup_seed
    from mipnerf_pl_amd.train_graph import GraphedTrainStep
    data, name = scenes[kind]
    hp = _hp(data, tmp_path / "o", name)
    setup_seed(hp["seed"])
    system = MipNeRFSystem(dict(hp, precision="bf16"), precision="bf16").to(DEV)
    system.setup()
    system.fused_adam = True
    opt = system.configure_optimizers()[0][0]
    opt._dev_step = torch.full((1,), opt.steps, dtype=torch.int64, device=DEV)
    opt._hyper = torch.zeros(4, dtype=torch.float32, device=DEV)
    ds = system.train_dataset
    d = ds._need_device()
    order = epoch_order(len(ds), hp["seed"], 0, 0, 1, DEV).contiguous()
    assert order.numel() >= 3 * B
    base = torch.zeros(1, dtype=torch.int64, device=DEV)
    occ, lattice = sphere_occupancy(system, kind, grid)
    tmp = (torch.zeros(B, dtype=torch.uint8, device=DEV), None, None, torch.zeros(B, 1, device=DEV), torch.zeros(B, 1, device=DEV))

    def batch_source():
        ops.gather_train_batch(order, d["offsets"], d["cameras"], d["pixels"], opt._dev_step, base, step.rays, step.gt)
        if tighten_in_source:
            ops.ray_span(occ, step.rays, N, disparity=system.mip_nerf.disparity, out=tmp)
            step.rays.near.copy_(tmp[3])
            step.rays.far.copy_(tmp[4])
    kw = dict(occupancy=occ) if with_occupancy else {}
    step = GraphedTrainStep(system, opt, B, DEV, use_graph=use_graph, batch_source=batch_source, **kw)
    return step, system, opt, ds, order, occ, lattice


@pytest.mark.parametrize("kind", ["bounded", "unbounded"])
def test_spans_inside_the_step_equal_ray_span_and_a_step_on_tightened_rays(scenes, tmp_path, kind):
    from mipnerf_pl_amd import ops
    ref, ref_system, ref_opt, *_ = _make_step(scenes, kind, tmp_path, use_graph=False, with_occupancy=False, tighten_in_source=True)
    for _ in range(3):
        ref()
    torch.cuda.synchronize()
    for use_graph in (True, False):
        step, system, opt, ds, order, occ, _ = _make_step(scenes, kind, tmp_path, use_graph=use_graph, with_occupancy=True)
        assert system.mip_nerf.unbounded == (kind == "unbounded") and (occ.space == "contracted") == (kind == "unbounded")
        seen_live, seen_late = [], False
        for k in range(3):
            step()
            assert step.capture_error is None and (step._graphs is not None) == use_graph
            want_rays, want_gt = ds.rays_at(order[k * B:(k + 1) * B])
            for name in want_rays._fields:             # near / far included: the gathered values stay
                assert torch.equal(getattr(step.rays, name), getattr(want_rays, name)), (kind, k, name)
            live, first, last, near, far = ops.ray_span(occ, step.rays, N, disparity=system.mip_nerf.disparity)
            for got, want, name in ((step.live, live, "live"), (step.first, first, "first"), (step.last, last, "last"),
                                    (step.near_span, near, "near_span"), (step.far_span, far, "far_span")):
                assert torch.equal(got, want), (kind, use_graph, k, name)
            seen_live.append(step.live.float().mean().item())
            seen_late = seen_late or bool((step.first[step.live.bool()] > 0).any())
            share, span = step.span_stats()
            assert share == pytest.approx(seen_live[-1]) and 0.0 < span <= 1.0
        print(f"span step {kind} graph={use_graph}: live share per step {seen_live}")
        assert all(0.0 < v < 1.0 for v in seen_live) and seen_late          # not vacuous: dead rays, live rays, and a tightened near
        torch.cuda.synchronize()
        assert torch.equal(system.mip_nerf.mlp._flat_param, ref_system.mip_nerf.mlp._flat_param), (kind, use_graph)
        assert torch.equal(opt.exp_avg, ref_opt.exp_avg) and torch.equal(opt.exp_avg_sq, ref_opt.exp_avg_sq), (kind, use_graph)
        assert opt.steps == ref_opt.steps == 3


def test_a_model_and_a_grid_of_different_spaces_are_refused(scenes, tmp_path):
    from mipnerf_pl_amd.train_graph import GraphedTrainStep
    step, system, opt, _, _, occ, _ = _make_step(scenes, "bounded", tmp_path, use_graph=False, with_occupancy=True)
    occ.space = "contracted"
    with pytest.raises(ValueError, match="this model is bounded"):
        GraphedTrainStep(system, opt, B, DEV, use_graph=False, occupancy=occ)
    step, system, opt, _, _, occ, _ = _make_step(scenes, "unbounded", tmp_path, use_graph=False, with_occupancy=True)
    occ.space = None
    with pytest.raises(NotImplementedError, match="unbounded=True models are not supported"):
        GraphedTrainStep(system, opt, B, DEV, use_graph=False, occupancy=occ)


def test_a_captured_step_reads_the_grid_not_a_snapshot(scenes, tmp_path):
    from mipnerf_pl_amd import ops
    step, system, opt, ds, order, occ, lattice = _make_step(scenes, "bounded", tmp_path, use_graph=True, with_occupancy=True)
    assert (occ.threshold, occ.dilate) == (0.0, 0)
    step()
    assert step._graphs is not None and 0.0 < step.live.float().mean().item() < 1.0
    ptr = occ.bits.data_ptr()
    running = lattice.clone()
    ops.occupancy_refresh(occ, torch.zeros_like(running), running, 0.0)          # max(0 * running, 0) = 0: nothing is above the threshold
    assert occ.bits.data_ptr() == ptr and not bool(_words(occ.bits).any())
    step()
    assert not bool(step.live.any()) and torch.equal(step.near_span, step.rays.near) and torch.equal(step.far_span, step.rays.far)
    assert bool((step.first == N).all()) and bool((step.last == -1).all())
    ops.occupancy_refresh(occ, torch.ones_like(running), running, 0.0)           # every cell occupied
    step()
    r = step.rays
    t, _ = ops.sample_along_rays(r.origins, r.directions, r.radii, N, r.near, r.far, False, system.mip_nerf.disparity, "cone")
    assert bool(step.live.all()) and bool((step.first == 0).all()) and bool((step.last == N - 1).all())
    assert torch.equal(step.near_span[:, 0], t[:, 0]) and torch.equal(step.far_span[:, 0], t[:, N])
    assert opt.steps == 3


# ---- 4. off means off; a full grid is the old path -------------------------------------------------------------------------------
def test_off_means_off_and_a_full_grid_is_the_old_path(tmp_path):
    """The Blender fixture: near 2, far 6, for which the end fence posts 2 + 4 * 0 and 2 + 4 * 1 are near and far exactly.  With threshold
    -1 every density exceeds it, every frustum hits, and the tightened step is the untightened one bit for bit -- through the captured
    step and the epoch's short eager batch."""
    from mipnerf_pl_amd.train import CSVLog, Trainer
    data = fx.write_blender(str(tmp_path / "d"))
    off = Trainer(_hp(data, tmp_path / "off", "blender", optimizer__max_steps=5), verbose=False, device=DEV, log_every_n_steps=2)
    assert off.occ is None and off.spe == 3 and off.last_bs == 104
    off.fit()
    on = Trainer(_hp(data, tmp_path / "on", "blender", optimizer__max_steps=5, **_occ_kw(threshold=-1.0)), verbose=False, device=DEV,
                 log_every_n_steps=2).fit()
    assert on.occ is not None and on.occ.refreshes == 2 and on.occ.occupancy.occupied_fraction() == 1.0
    assert bool(on.gstep.live.all()) and torch.equal(on.gstep.near_span, on.gstep.rays.near) and torch.equal(on.gstep.far_span, on.gstep.rays.far)
    for (k, a), (k2, b) in zip(off.system.state_dict().items(), on.system.state_dict().items()):
        assert k == k2 and torch.equal(a, b), k
    assert torch.equal(off.opt.exp_avg, on.opt.exp_avg) and torch.equal(off.opt.exp_avg_sq, on.opt.exp_avg_sq)
    ck_off = torch.load(str(tmp_path / "off" / "ckpt" / "t" / "last.ckpt"), map_location="cpu", weights_only=False)
    ck_on = torch.load(str(tmp_path / "on" / "ckpt" / "t" / "last.ckpt"), map_location="cpu", weights_only=False)
    assert set(ck_off["mipnerf_trainer"]) == {"global_step", "epoch", "batch", "topk", "rng"}
    assert set(ck_on["mipnerf_trainer"]) == set(ck_off["mipnerf_trainer"]) | {"occupancy"} and set(ck_on) == set(ck_off)
    assert not any("occupancy" in str(k) for k in ck_off["hyper_parameters"])
    header = open(os.path.join(off.logger.dir, "metrics.csv")).readline().strip()
    assert header == "step,lr,train/loss,train/psnr,val/loss,val/psnr" == ",".join(CSVLog.COLUMNS)
    header = open(os.path.join(on.logger.dir, "metrics.csv")).readline().strip()
    assert header == "step,lr,train/loss,train/psnr,val/loss,val/psnr,train/live_share,train/span_share"


# ---- 5. resume --------------------------------------------------------------------------------------------------------------------
def test_resume_is_exact_with_a_refreshed_grid(tmp_path):
    """tests/test_gpu_train_cli.py::test_resume_is_exact_with_randomized_draws with the feature on and a refresh every 3 steps: a
    checkpoint after step 4 (the next refresh, before step 6, is the resumed run's) and one after step 6 (the resumed run starts with a
    refresh)."""
    from mipnerf_pl_amd.train import Trainer, read_metrics
    data = fx.write_multicam(str(tmp_path / "d"))
    kw = dict(optimizer__max_steps=10, val__check_interval=2, train__randomized=True, **_occ_kw())
    straight = Trainer(_hp(data, tmp_path / "a", "multi_blender", **kw), verbose=False, device=DEV, log_every_n_steps=2).fit()
    assert straight.occ.refreshes == 4 and straight.spe == 4 and straight.last_bs == 120
    a = torch.load(str(tmp_path / "a" / "ckpt" / "t" / "last.ckpt"), map_location="cpu", weights_only=False)
    sa, ma, va, na = _state(a)
    rows = [r for r in read_metrics(os.path.join(straight.logger.dir, "metrics.csv")) if "train/loss" in r]
    assert len(rows) == 5
    for r in rows:
        assert 0.0 <= r["train/live_share"] <= 1.0 and (r["train/live_share"] == 0.0 or 0.0 <= r["train/span_share"] <= 1.0), r
    for until in (4, 6):
        b, c = tmp_path / f"b{until}", tmp_path / f"c{until}"
        Trainer(_hp(data, b, "multi_blender", **kw), verbose=False, device=DEV).fit(until=until)
        half = str(b / "ckpt" / "t" / "last.ckpt")
        hck = torch.load(half, map_location="cpu", weights_only=False)
        assert hck["global_step"] == until and hck["mipnerf_trainer"]["occupancy"]["refreshes"] == 2
        resumed = Trainer(_hp(data, c, "multi_blender", checkpoint__resume_path=half, **kw), verbose=False, device=DEV)
        assert torch.equal(resumed.occ.running.cpu(), hck["mipnerf_trainer"]["occupancy"]["running"])
        resumed.fit()
        ck = torch.load(str(c / "ckpt" / "t" / "last.ckpt"), map_location="cpu", weights_only=False)
        sc, mc, vc, nc = _state(ck)
        assert na == nc == 10 and ck["global_step"] == 10 and resumed.occ.refreshes == 4
        for k in sa:
            assert torch.equal(sa[k], sc[k]), (until, k)
        assert torch.equal(ma, mc) and torch.equal(va, vc), until
        oa, oc = a["mipnerf_trainer"]["occupancy"], ck["mipnerf_trainer"]["occupancy"]
        assert torch.equal(oa["running"].view(torch.int32), oc["running"].view(torch.int32)), until
        assert {k: v for k, v in oa.items() if k != "running"} == {k: v for k, v in oc.items() if k != "running"}
        assert torch.equal(_words(straight.occ.occupancy.bits), _words(resumed.occ.occupancy.bits)), until
    # another grid than the checkpoint's is refused
    with pytest.raises(ValueError, match="dims"):
        Trainer(_hp(data, tmp_path / "x", "multi_blender", checkpoint__resume_path=half, **dict(kw, **_occ_kw(grid=20))), verbose=False, device=DEV)


# ---- 6. the eager routes -------------------------------------------------------------------------------------------------------
def test_tighten_is_ray_span_of_the_batch(tmp_path):
    from mipnerf_pl_amd import ops
    from mipnerf_pl_amd.train import Trainer
    data = fx.write_multicam(str(tmp_path / "d"))
    tr = Trainer(_hp(data, tmp_path / "o", "multi_blender", optimizer__max_steps=2, **_occ_kw(span_samples=32)), verbose=False, device=DEV)
    tr.occ.refresh(tr.system)
    ids = torch.arange(7, 7 + 100, device=DEV)
    rays, gt = tr.system.train_dataset.rays_at(ids)
    (tight, gt2) = tr._tighten((rays, gt))
    live, first, last, near, far = ops.ray_span(tr.occ.occupancy, rays, 32, disparity=tr.system.mip_nerf.disparity)
    assert gt2 is gt and torch.equal(tight.near, near) and torch.equal(tight.far, far)
    for name in ("origins", "directions", "viewdirs", "radii", "lossmult"):
        assert getattr(tight, name) is getattr(rays, name)
    for got, want in zip(tr._span, (live, first, last)):
        assert torch.equal(got, want)
    share, span = tr._span_stats()
    assert share == pytest.approx(live.float().mean().item())


@pytest.mark.parametrize("flags", [["--precision", "fp32"], ["--no-graph"]])
def test_eager_routes_train_on_spans_and_keep_the_state(tmp_path, flags):
    data = fx.write_multicam(str(tmp_path / "d"))
    out = tmp_path / "out"
    _run(["mipnerf_pl_amd.train", "--data_path", data, "--out_dir", str(out), "--dataset_name", "multi_blender"] + flags +
         ["train.batch_size", "128", "nerf.num_samples", "64", "optimizer.max_steps", "5", "val.check_interval", "2", "val.sample_num", "1",
          "val.chunk_size", "4096", "train.occupancy.enabled", "True", "train.occupancy.grid", "16", "train.occupancy.interval", "3"])
    ck = torch.load(str(out / "ckpt" / "lego" / "last.ckpt"), map_location="cpu", weights_only=False)
    assert ck["global_step"] == 5 and _state(ck)[3] == 5
    occ = ck["mipnerf_trainer"]["occupancy"]
    assert occ["refreshes"] == 2 and tuple(occ["running"].shape) == (16, 16, 16) and occ["running"].dtype == torch.float32
    assert bool(torch.isfinite(occ["running"]).all()) and float(occ["running"].max()) > 0.0 and occ["interval"] == 3
    assert all(torch.isfinite(v).all() for v in ck["state_dict"].values())


# ---- 7. two ranks ----------------------------------------------------------------------------------------------------------------
def test_two_ranks_refresh_identical_grids(tmp_path):
    data = fx.write_multicam(str(tmp_path / "d"))
    out = tmp_path / "out"
    log = _run(["mipnerf_pl_amd.train", "--data_path", data, "--out_dir", str(out), "--dataset_name", "multi_blender",
                "--child_timeout", "500", "num_gpus", "2", "train.batch_size", "64", "nerf.num_samples", "64", "optimizer.max_steps", "4",
                "val.check_interval", "2", "val.sample_num", "1", "val.chunk_size", "4096", "train.occupancy.enabled", "True",
                "train.occupancy.grid", "16", "train.occupancy.interval", "3"], timeout=600, env_extra={"MIPNERF_TRAIN_SHARE_GPU": "1"})
    assert "replicas identical on 2 ranks (occupancy grid included)" in log, log[-2000:]
    ck = torch.load(str(out / "ckpt" / "lego" / "last.ckpt"), map_location="cpu", weights_only=False)
    assert ck["global_step"] == 4 and ck["mipnerf_trainer"]["occupancy"]["refreshes"] == 2
