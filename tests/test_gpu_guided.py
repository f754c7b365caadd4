"""GPU: error-guided batch sampling -- the kernels behind mipnerf_guided_* (ops.guided_refresh / guided_draw / guided_accumulate /
guided_apply over an ops.GuidedState), `train_guided.TrainGuided`, `GraphedTrainStep(guided=...)` and the Trainer's `train.guided.*` route.
Every comparison is exact: against the rule restated in numpy (tests/guided_fixture.py) with torch.equal / integer equality.

1. refresh (fold + mass + scan); 2. draw; 3. accumulate; 4. apply; 5. inside the captured step; 6. off means off; 7. resume is exact;
8. the eager routes."""
import functools
import os

import numpy as np
import pytest
import torch

from tests import dataset_fixture as fx
from tests import guided_fixture as gf

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
SMALL = ([(37, 29), (16, 16), (8, 40), (3, 5)], 8)          # 30 cells, 1664 pixels, edge tiles of every kind
BIG = ([(2100, 2100)], 8)                                   # 69,169 cells: more than one block and more than one pass of the one-workgroup scan
B, N = 64, 64


@functools.lru_cache(maxsize=None)
def _table(which):
    sizes, T = SMALL if which == "small" else BIG
    tab = gf.table(sizes, T)
    return tab, gf.cells(tab, T), T


def _state(which, ring=64):
    from mipnerf_pl_amd import ops
    tab, g, T = _table(which)
    st = ops.GuidedState(tab, T, ring, DEV)
    assert st.n_cells == len(g["n"]) and st.n_pixels == int(g["n"].sum())
    return st


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


def _put_u64(dst, arr):
    dst.copy_(torch.from_numpy(np.ascontiguousarray(arr, np.uint64).view(np.int64)))


def _bits(t):
    return t.view(torch.int32)


def _counters(n, rng, zero_sums):
    """sum / cnt with cnt = 0, sum = 0 at cnt > 0, cnt = 1 and large counts among them."""
    cnt = rng.integers(0, 9, n).astype(np.uint32)
    cnt[rng.integers(0, n, max(1, n // 7))] = 0
    cnt[1], cnt[2], cnt[n - 1] = 0, 1, 4099
    s = (rng.uniform(0.0, 0.4, n) * cnt * (1 << 24)).astype(np.uint64)
    s[0], cnt[0] = 0, 3
    s[cnt == 0] = 0
    if zero_sums:
        s[:] = 0
    return s, cnt


# ---- 1. refresh --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["small", "big"])
@pytest.mark.parametrize("rate", [1.0, 0.25])
@pytest.mark.parametrize("mix", [0.0, 0.5, 0.9])
@pytest.mark.parametrize("zero_map", [False, True])
def test_refresh_equals_the_rule(which, rate, mix, zero_map):
    from mipnerf_pl_amd import ops
    tab, g, T = _table(which)
    n = len(g["n"])
    rng = np.random.default_rng(n + int(10 * mix))
    st = _state(which)
    err = np.zeros(n, np.float32) if zero_map else rng.uniform(0.0, 0.5, n).astype(np.float32)
    seen = np.zeros(n, bool)
    st.err.copy_(torch.from_numpy(err))
    for round_ in range(2):                 # the second refresh reuses q / cdf / scratch in place and adds to the visited cells
        s, cnt = _counters(n, rng, zero_map)
        _put_u64(st.sum, s)
        st.cnt.copy_(torch.from_numpy(cnt.view(np.int32)))
        assert ops.guided_refresh(st, rate, mix) is st
        err = gf.fold(err, s, cnt, rate)
        seen |= cnt > 0
        q, cdf, Q, A = gf.mass(err, g["n"], mix)
        assert Q < (1 << 31) and (A == 0) == zero_map
        assert torch.equal(_bits(st.err).cpu(), torch.from_numpy(err.view(np.int32))), (which, round_)
        assert np.array_equal(st.q.cpu().numpy().astype(np.uint64), q) and np.array_equal(st.cdf.cpu().numpy().astype(np.uint64), cdf)
        assert st.header.tolist() == [Q, A, int(seen.sum()), n]
        assert not bool(st.sum.any()) and not bool(st.cnt.any())
        assert np.array_equal(st.seen.cpu().numpy().astype(bool), seen)


# ---- 2. draw ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["small", "big"])
@pytest.mark.parametrize("mix", [0.5, 0.9])
def test_draw_equals_the_rule(which, mix):
    from mipnerf_pl_amd import ops
    tab, g, T = _table(which)
    n, nd, ring, start = len(g["n"]), 4099, 5000, 3000                  # 4,099 draws: no multiple of the block; the ring slots wrap
    rng = np.random.default_rng(17)
    st = _state(which, ring)
    err = rng.uniform(0.0, 0.5, n).astype(np.float32)
    err[::3] = 0.0
    st.err.copy_(torch.from_numpy(err))
    ops.guided_refresh(st, 1.0, mix)
    _, cdf, Q, _ = gf.mass(err, g["n"], mix)
    assert int(st.header[0]) == Q
    edge = gf.boundary_r0(cdf)[:2000]
    r0 = np.concatenate([edge, rng.integers(0, 1 << 32, nd - len(edge), dtype=np.uint64)])
    r1 = rng.integers(0, 1 << 32, nd, dtype=np.uint64)
    r1[:4] = [0, (1 << 32) - 1, 0, (1 << 32) - 1]
    r0[2:4] = [(1 << 32) - 1, (1 << 32) - 1]
    r0[0] = 0
    r = torch.from_numpy(np.stack([r0, r1]).astype(np.int64)).to(DEV)
    order = torch.full((nd + 100,), -7, dtype=torch.int64, device=DEV)
    ops.guided_draw(st, r, order[50:50 + nd], ring_start=start)
    want_order, want_w, want_c = gf.draw(tab, T, cdf, r0, r1)
    assert bool((order[:50] == -7).all()) and bool((order[50 + nd:] == -7).all())
    assert torch.equal(order[50:50 + nd].cpu(), torch.from_numpy(want_order))
    slots = (start + np.arange(nd)) % ring
    ring_w, ring_c = np.ones(ring, np.float32), np.zeros(ring, np.int32)
    ring_w[slots], ring_c[slots] = want_w, want_c
    assert torch.equal(_bits(st.weight).cpu(), torch.from_numpy(ring_w.view(np.int32)))
    assert torch.equal(st.cell.cpu(), torch.from_numpy(ring_c))
    assert want_c.min() == 0 and want_c.max() == n - 1 and len(np.unique(want_c)) > min(n, 1000) // 2          # not vacuous
    # no draws: nothing is launched and nothing changes
    before = (order.clone(), st.weight.clone(), st.cell.clone())
    ops.guided_draw(st, r[:, :0].contiguous(), order[:0], ring_start=7)
    assert all(torch.equal(a, b) for a, b in zip(before, (order, st.weight, st.cell)))
    with pytest.raises(ValueError, match="guided_draw"):
        ops.guided_draw(st, r, order[:nd - 1])


# ---- 3. accumulate ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("spread", [False, True])
@pytest.mark.parametrize("device_index", [True, False])
def test_accumulate_equals_the_integer_sums(spread, device_index):
    from mipnerf_pl_amd import ops
    nb, ring, b = 4099, 6000, 1                                          # slots 4099 .. 5999, then 0 .. 2187: they wrap
    n_order = 2 * nb - 10                                                # the last 10 rays lie past the order and are left alone
    rng = np.random.default_rng(3 + spread)
    cells = rng.integers(0, 30, ring).astype(np.int32) if spread else np.full(ring, 7, np.int32)
    rgb = rng.uniform(0.0, 1.0, (nb, 3)).astype(np.float32)
    gt = rng.uniform(0.0, 1.0, (nb, 3)).astype(np.float32)
    rgb[5, 1] = np.nan
    rgb[9] = gt[9]
    want_s, want_c = np.zeros(30, np.uint64), np.zeros(30, np.uint32)
    want_s[3], want_c[3] = 11, 2                                         # the adds land on what is there
    runs = []
    for _ in range(2):
        st = _state("small", ring)
        st.cell.copy_(torch.from_numpy(cells))
        st.sum[3], st.cnt[3] = 11, 2
        kw = dict(step=torch.tensor([41], device=DEV), epoch_base=torch.tensor([40], device=DEV)) if device_index else dict(batch=b)
        ops.guided_accumulate(st, torch.from_numpy(rgb).to(DEV), torch.from_numpy(gt).to(DEV), n_order, **kw)
        runs.append((st.sum.clone(), st.cnt.clone()))
    gf.accumulate(want_s, want_c, cells, b, nb, n_order, rgb, gt)
    assert int(want_c.sum()) == 2 + nb - 10 - 1                          # every ray inside the order but the NaN one
    assert np.array_equal(_u64(runs[0][0]), want_s) and np.array_equal(runs[0][1].cpu().numpy().view(np.uint32), want_c)
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    # a batch index before the epoch leaves everything alone
    st = _state("small", ring)
    ops.guided_accumulate(st, torch.from_numpy(rgb).to(DEV), torch.from_numpy(gt).to(DEV), n_order, batch=-1)
    assert not bool(st.cnt.any()) and not bool(st.sum.any())


# ---- 4. apply ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device_index", [True, False])
def test_apply_multiplies_by_the_ring_weight(device_index):
    from mipnerf_pl_amd import ops
    nb, ring, b = 300, 500, 3                                            # slots 400 .. 499, 0 .. 199
    rng = np.random.default_rng(8)
    st = _state("small", ring)
    w = rng.uniform(0.1, 10.0, ring).astype(np.float32)
    st.weight.copy_(torch.from_numpy(w))
    lm = rng.choice(np.asarray([1.0, 4.0, 16.0, 0.3], np.float32), (nb, 1))
    kw = dict(step=torch.tensor([10], device=DEV), epoch_base=torch.tensor([7], device=DEV)) if device_index else dict(batch=b)
    for n_order, touched in ((10 * nb, nb), (b * nb + 77, 77), (b * nb, 0)):
        t = torch.from_numpy(lm).to(DEV)
        assert ops.guided_apply(st, t, n_order, **kw) is t
        want = lm.copy()
        i, sl = gf.slots(b, nb, ring, n_order)
        assert len(i) == touched
        want[i, 0] = lm[i, 0] * w[sl]
        assert torch.equal(_bits(t).cpu(), torch.from_numpy(want.view(np.int32))), n_order
    t = torch.from_numpy(lm).to(DEV)
    ops.guided_apply(st, t, 10 * nb, batch=-2)
    assert torch.equal(t.cpu(), torch.from_numpy(lm))
    with pytest.raises(ValueError, match="guided_apply"):
        ops.guided_apply(st, t, 10 * nb, step=torch.tensor([10], device=DEV))


# ---- 5. inside the captured step --------------------------------------------------------------------------------------------------
def _hp(data, out, **kw):
    from mipnerf_pl_amd import config as cfg
    hp = dict(cfg.DEFAULTS, data_path=str(data), out_dir=str(out), dataset_name="blender", exp_name="t")
    hp.update({"train.batch_size": B, "nerf.num_samples": N, "val.check_interval": 1000, "val.sample_num": 1, "val.chunk_size": 4096,
               "optimizer.lr_delay_steps": 0, "train.randomized": False})
    hp.update({k.replace("__", "."): v for k, v in kw.items()})
    return hp


def _guided_kw(**kw):
    base = {"train.guided.enabled": True, "train.guided.tile": 4, "train.guided.interval": 2}
    base.update({"train.guided." + k: v for k, v in kw.items()})
    return base


@pytest.mark.parametrize("use_graph", [True, False])
def test_the_step_weighs_and_records_what_the_sampler_drew(tmp_path, use_graph):
    from mipnerf_pl_amd import config as cfg
    from mipnerf_pl_amd import ops
    from mipnerf_pl_amd.system import MipNeRFSystem
    from mipnerf_pl_amd.train import setup_seed
    from mipnerf_pl_amd.train_graph import GraphedTrainStep
    from mipnerf_pl_amd.train_guided import TrainGuided
    data = fx.write_blender(str(tmp_path / "d"))                           # 3 train images of 12 x 10
    hp = _hp(data, tmp_path / "o", **_guided_kw())
    setup_seed(hp["seed"])
    system = MipNeRFSystem(dict(hp, precision="bf16"), precision="bf16").to(DEV)
    system.setup()
    system.fused_adam = True
    opt = system.configure_optimizers()[0][0]
    opt._dev_step = torch.full((1,), opt.steps, dtype=torch.int64, device=DEV)
    opt._hyper = torch.zeros(4, dtype=torch.float32, device=DEV)
    ds = system.train_dataset
    d = ds._need_device()
    n_order = len(ds)
    assert n_order == 360 and [tuple(v) for v in ds.sizes] == [(10, 12)] * 3
    tgd = TrainGuided.for_system(system, hp, DEV)
    st = tgd.state
    assert st.n_cells == 27 and st.ring_len == 2 * B and cfg.train_guided_settings(hp)["interval"] == 2
    order = torch.full((n_order,), -1, dtype=torch.int64, device=DEV)
    base = torch.zeros(1, dtype=torch.int64, device=DEV)

    def batch_source():
        ops.gather_train_batch(order, d["offsets"], d["cameras"], d["pixels"], opt._dev_step, base, step.rays, step.gt)
    with pytest.raises(ValueError, match="batch_source"):
        GraphedTrainStep(system, opt, B, DEV, use_graph=False, guided=st, guided_index=(opt._dev_step, base, n_order))
    step = GraphedTrainStep(system, opt, B, DEV, use_graph=use_graph, batch_source=batch_source, guided=st,
                            guided_index=(opt._dev_step, base, n_order))
    tab = gf.table(ds.sizes, 4)
    weights_seen = []
    for k in range(5):
        if tgd.refresh_due(k):
            tgd.refresh(order, k, B, n_order)
            assert not bool(st.cnt.any()) and tgd.segment == (k * B, min((k + 2) * B, n_order))
            ids = order[k * B:tgd.segment[1]]
            assert int(ids.min()) >= 0 and int(ids.max()) < n_order
        s0, c0 = _u64(st.sum).copy(), st.cnt.cpu().numpy().view(np.uint32).copy()
        ring_w, ring_c = st.weight.cpu().numpy(), st.cell.cpu().numpy()
        step()
        torch.cuda.synchronize()
        assert step.capture_error is None and (step._graphs is not None) == use_graph
        i, sl = gf.slots(k, B, st.ring_len, n_order)
        want_rays, want_gt = ds.rays_at(order[k * B:(k + 1) * B])
        assert torch.equal(step.gt, want_gt)
        want_lm = want_rays.lossmult.cpu().numpy()[:, 0] * ring_w[sl]
        assert torch.equal(_bits(step.rays.lossmult[:, 0]).cpu(), torch.from_numpy(want_lm.astype(np.float32).view(np.int32))), k
        # every drawn id lies in the cell its ring slot names
        g = gf.cells(tab, 4)
        ids = order[k * B:(k + 1) * B].cpu().numpy()
        c = ring_c[sl]
        p = ids - g["pix0"][c]
        x, y = p % g["W"][c], p // g["W"][c]
        assert ((x >= g["x0"][c]) & (x < g["x0"][c] + g["w"][c]) & (y >= g["y0"][c]) & (y < g["y0"][c] + g["h"][c])).all()
        # the growth of the counters is the rule applied to the step's own colours
        gf.accumulate(s0, c0, ring_c, k, B, n_order, step.fine_rgb.cpu().numpy(), step.gt.cpu().numpy())
        assert np.array_equal(_u64(st.sum), s0) and np.array_equal(st.cnt.cpu().numpy().view(np.uint32), c0), k
        assert int(c0.sum()) == B * (k % 2 + 1)                              # the capture's warm-up left nothing behind
        weights_seen.append(ring_w[sl].copy())
    # the refresh before replay 2 folded two steps' errors: the next replays read other weights than the uniform start's
    assert np.abs(weights_seen[0] - 1.0).max() <= 2e-7 and np.abs(weights_seen[1] - 1.0).max() <= 2e-7          # err = 1 everywhere: uniform
    assert len(np.unique(weights_seen[2])) > 1 and len(np.unique(weights_seen[4])) > 1
    assert tgd.refreshes == 3 and opt.steps == 5
    ess, visited = tgd.stats(4, n_order)
    assert 0.0 < ess <= 1.0 and 0.0 < visited <= 1.0 and visited == int(st.seen.sum()) / 27


# ---- 6. off means off ---------------------------------------------------------------------------------------------------------------
def test_off_means_off(tmp_path, monkeypatch):
    from mipnerf_pl_amd import _lib as L
    from mipnerf_pl_amd import ops
    from mipnerf_pl_amd.train import CSVLog, Trainer

    def refuse(*a, **k):
        raise AssertionError("a guided entry point was called by a run without train.guided.enabled")
    lib = L.lib()
    for name in ("guided_apply", "guided_accumulate", "guided_refresh", "guided_draw"):
        monkeypatch.setattr(ops, name, refuse)
        monkeypatch.setattr(lib, "mipnerf_" + name, refuse)
    data = fx.write_blender(str(tmp_path / "d"))
    off = Trainer(_hp(data, tmp_path / "off", optimizer__max_steps=7), verbose=False, device=DEV, log_every_n_steps=2)
    assert off.guided is None and off.spe == 6 and off.last_bs == 40 and off.gstep.guided is None and off.gstep._outs is None
    off.fit()                                       # five replays, the short eager batch, the next epoch's first
    assert not hasattr(off.system.mip_nerf, "keep_fine_rgb")
    ck = torch.load(str(tmp_path / "off" / "ckpt" / "t" / "last.ckpt"), map_location="cpu", weights_only=False)
    assert set(ck["mipnerf_trainer"]) == {"global_step", "epoch", "batch", "topk", "rng"}
    header = open(os.path.join(off.logger.dir, "metrics.csv")).readline().strip()
    assert header == "step,lr,train/loss,train/psnr,val/loss,val/psnr" == ",".join(CSVLog.COLUMNS)


# ---- 7. resume ------------------------------------------------------------------------------------------------------------------------
def _opt_state(ck):
    (s,) = ck["optimizer_states"][0]["state"].values()
    return ck["state_dict"], s["exp_avg"], s["exp_avg_sq"], int(s["step"])


def test_resume_is_exact(tmp_path):
    """2 * interval + 3 = 7 steps straight, against interval + 1 = 3 steps, a checkpoint, and the rest: the refreshes before batch 4 and
    before the next epoch's batch 0 lie after the resume point, and so does the epoch's short eager batch."""
    from mipnerf_pl_amd.train import Trainer, read_metrics
    data = fx.write_blender(str(tmp_path / "d"))
    kw = dict(optimizer__max_steps=7, val__check_interval=1, train__randomized=True, **_guided_kw())
    straight = Trainer(_hp(data, tmp_path / "a", **kw), verbose=False, device=DEV, log_every_n_steps=1).fit()
    assert straight.guided.refreshes == 4 and straight.spe == 6 and straight.last_bs == 40
    rows = [r for r in read_metrics(os.path.join(straight.logger.dir, "metrics.csv")) if "train/loss" in r]
    assert len(rows) == 7
    for r in rows:
        assert 0.0 < r["train/guided_ess"] <= 1.0 and 0.0 <= r["train/guided_visited"] <= 1.0, r
    assert rows[0]["train/guided_ess"] == pytest.approx(1.0, abs=1e-6) and rows[0]["train/guided_visited"] == 0.0
    assert rows[-1]["train/guided_visited"] > 0.0
    header = open(os.path.join(straight.logger.dir, "metrics.csv")).readline().strip()
    assert header == "step,lr,train/loss,train/psnr,val/loss,val/psnr,train/guided_ess,train/guided_visited"
    a = torch.load(str(tmp_path / "a" / "ckpt" / "t" / "last.ckpt"), map_location="cpu", weights_only=False)
    Trainer(_hp(data, tmp_path / "b", **kw), verbose=False, device=DEV).fit(until=3)
    half = str(tmp_path / "b" / "ckpt" / "t" / "last.ckpt")
    hck = torch.load(half, map_location="cpu", weights_only=False)
    assert hck["global_step"] == 3 and hck["mipnerf_trainer"]["guided"]["refreshes"] == 2
    assert hck["mipnerf_trainer"]["guided"]["segment"] == (2 * B, 4 * B) and int(hck["mipnerf_trainer"]["guided"]["cnt"].sum()) == B
    resumed = Trainer(_hp(data, tmp_path / "c", checkpoint__resume_path=half, **kw), verbose=False, device=DEV)
    assert torch.equal(resumed.order[2 * B:4 * B].cpu(), hck["mipnerf_trainer"]["guided"]["order"])
    resumed.fit()
    c = torch.load(str(tmp_path / "c" / "ckpt" / "t" / "last.ckpt"), map_location="cpu", weights_only=False)
    (sa, ma, va, na), (sc, mc, vc, nc) = _opt_state(a), _opt_state(c)
    assert na == nc == 7 and c["global_step"] == 7 and resumed.guided.refreshes == 4
    for k in sa:
        assert torch.equal(sa[k], sc[k]), k
    assert torch.equal(ma, mc) and torch.equal(va, vc)
    ga, gc = a["mipnerf_trainer"]["guided"], c["mipnerf_trainer"]["guided"]
    assert set(ga) == set(gc)
    for k in ga:
        if torch.is_tensor(ga[k]):
            bits = (lambda t: t.view(torch.int32)) if ga[k].dtype == torch.float32 else (lambda t: t)
            assert ga[k].dtype == gc[k].dtype and torch.equal(bits(ga[k]), bits(gc[k])), k
        else:
            assert ga[k] == gc[k], k
    for name in ("err", "sum", "cnt", "weight", "cell"):
        assert torch.equal(getattr(straight.guided.state, name), getattr(resumed.guided.state, name)), name
    assert int(ga["cnt"].sum()) == B                                      # the next epoch's first batch, after its refresh
    # a state of another tile is refused
    with pytest.raises(ValueError, match="tile"):
        Trainer(_hp(data, tmp_path / "x", checkpoint__resume_path=half, **dict(kw, **_guided_kw(tile=8))), verbose=False, device=DEV)


# ---- 8. the eager routes -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["fp32", "no-graph", "graph-short-batch"])
def test_eager_routes_weigh_and_record(tmp_path, route):
    from mipnerf_pl_amd.train import Trainer
    data = fx.write_blender(str(tmp_path / "d"))
    steps, rays = (6, B + 40) if route == "graph-short-batch" else (3, B)          # rays stepped since the refresh before batch 4 / batch 2
    hp = _hp(data, tmp_path / "o", optimizer__max_steps=100, **_guided_kw(), **({"train.occupancy.enabled": True, "train.occupancy.grid": 16}
                                                                                 if route == "no-graph" else {}))
    tr = Trainer(hp, precision="fp32" if route == "fp32" else "bf16", use_graph=route == "graph-short-batch", verbose=False, device=DEV)
    assert tr.graph_route == (route == "graph-short-batch") and (tr.occ is not None) == (route == "no-graph")
    tr.fit(until=steps)                     # (no validation after the last step: its forward would replace the step's colours)
    st = tr.guided.state
    assert tr.global_step == steps and tr.guided.refreshes == (3 if steps == 6 else 2)
    assert int(st.cnt.sum()) == rays and int(st.sum.sum()) > 0
    assert int(st.header[2]) > 0 and all(torch.isfinite(p).all() for p in tr.system.mip_nerf.parameters())
    # the last step's errors are the rule applied to its own colours
    b = steps - 1
    ids = tr.order[b * B:min((b + 1) * B, 360)]
    gt = tr.system.train_dataset.rays_at(ids)[1].cpu().numpy()
    want_s, want_c = np.zeros(st.n_cells, np.uint64), np.zeros(st.n_cells, np.uint32)
    if route == "graph-short-batch":
        gf.accumulate(want_s, want_c, st.cell.cpu().numpy(), b - 1, B, 360, tr.gstep.fine_rgb.cpu().numpy(), tr.gstep.gt.cpu().numpy())
    rgb = np.zeros((B, 3), np.float32)
    full_gt = np.zeros((B, 3), np.float32)
    rgb[:len(ids)], full_gt[:len(ids)] = tr.system.mip_nerf.last_fine_rgb.cpu().numpy(), gt
    gf.accumulate(want_s, want_c, st.cell.cpu().numpy(), b, B, 360, rgb, full_gt)
    assert np.array_equal(_u64(st.sum), want_s) and np.array_equal(st.cnt.cpu().numpy().view(np.uint32), want_c)
