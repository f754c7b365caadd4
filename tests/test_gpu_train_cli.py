"""GPU: the training command (mipnerf_pl_amd.train) and its in-graph batch producer (ops.gather_train_batch).

* the producer writes the bits `BaseDataset.rays_at` returns, eagerly and replayed from a captured graph as the device batch index advances;
* the trainer's graph route (one replay per full batch, the short last batch eager) equals the eager RayLoader + training_step_native +
  FlatAdam loop bit for bit;
* the command end to end on small scenes, exact resume, the fp32 / --no-graph routes and two ranks over gloo on one device."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import dataset_fixture as fx

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _hp(data, out, dataset_name, **kw):
    from mipnerf_pl_amd import config as cfg
    hp = dict(cfg.DEFAULTS, data_path=str(data), out_dir=str(out), dataset_name=dataset_name, exp_name="t")
    hp.update({"train.batch_size": 128, "nerf.num_samples": 64, "val.check_interval": 1000, "val.sample_num": 1,
               "val.chunk_size": 4096, "optimizer.lr_delay_steps": 0, "train.randomized": False})
    hp.update({k.replace("__", "."): v for k, v in kw.items()})
    return hp


def _run(args, timeout=600, env_extra=None):
    env = dict(os.environ, **(env_extra or {}))
    out = subprocess.run([sys.executable, "-m"] + args, capture_output=True, text=True, timeout=timeout, cwd=REPO, env=env)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    return out.stdout


def _state(ck):
    st = ck["optimizer_states"][0]["state"]
    (s,) = st.values()
    return ck["state_dict"], s["exp_avg"], s["exp_avg_sq"], int(s["step"])


# ---- the batch producer ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["blender", "multicam"])
@pytest.mark.parametrize("rank,world", [(0, 1), (1, 2)])
def test_gather_train_batch_equals_rays_at_eager_and_in_graph(tmp_path, kind, rank, world):
    from mipnerf_pl_amd import ops
    from mipnerf_pl_amd.datasets import Blender, Multicam
    from mipnerf_pl_amd.rays import Rays
    from mipnerf_pl_amd.train import epoch_order
    if kind == "blender":
        ds = Blender(fx.write_blender(str(tmp_path / "d")), split="train", device=DEV)
    else:
        ds = Multicam(fx.write_multicam(str(tmp_path / "d")), split="train", device=DEV)
    d = ds._need_device()
    order = epoch_order(ds.num_pixels, 4, 1, rank, world, DEV).contiguous()
    B = 48
    nb = (order.numel() + B - 1) // B
    rays = Rays(*[torch.empty(B, k, device=DEV) for k in (3, 3, 3, 1, 1, 1, 1)])
    gt = torch.empty(B, 3, device=DEV)
    step = torch.full((1,), 100, dtype=torch.int64, device=DEV)
    base = torch.full((1,), 100, dtype=torch.int64, device=DEV)

    def check(b):
        ids = order[b * B:(b + 1) * B]
        want_r, want_gt = ds.rays_at(ids)
        n = ids.numel()
        for k in Rays._fields:
            assert torch.equal(getattr(rays, k)[:n], getattr(want_r, k)), (kind, b, k)
            assert bool((getattr(rays, k)[n:] == -7.0).all()), (kind, b, k, "rays past the order must stay unwritten")
        assert torch.equal(gt[:n], want_gt) and bool((gt[n:] == -7.0).all())
    if kind == "multicam":
        assert len(set(ds.cameras[:, 25].tolist())) > 1          # lossmult differs per image

    def fill():
        for t in list(rays) + [gt]:
            t.fill_(-7.0)
    for b in range(nb):
        fill()
        step.fill_(100 + b)
        ops.gather_train_batch(order, d["offsets"], d["cameras"], d["pixels"], step, base, rays, gt)
        check(b)
    # captured: the batch index comes from the device; the step counter advances between replays
    step.fill_(100)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops.gather_train_batch(order, d["offsets"], d["cameras"], d["pixels"], step, base, rays, gt)
    for b in range(nb):
        fill()
        g.replay()
        check(b)
        step.add_(1)


# ---- graph route == eager loop -----------------------------------------------------------------------------------------------
def test_graph_route_equals_the_eager_loop_bit_for_bit(tmp_path):
    """The trainer's graph route (in-graph gather, one replay per full batch, the short batch eager) against the eager RayLoader loop on
    the same order: bit for bit against the same step launches issued eagerly on RayLoader's batches (copied into the step's buffers),
    and to round-off against training_step_native + FlatAdam.step for every batch (the bound tests/test_gpu_train.py holds for the
    graphed step against that hook loop)."""
    from mipnerf_pl_amd.datasets import RayLoader
    from mipnerf_pl_amd.system import MipNeRFSystem
    from mipnerf_pl_amd.train import Trainer, setup_seed, steps_per_epoch
    from mipnerf_pl_amd.train_graph import GraphedTrainStep
    data = fx.write_multicam(str(tmp_path / "d"))
    K = 6
    hp = _hp(data, tmp_path / "o", "multi_blender", optimizer__max_steps=K)
    tr = Trainer(hp, verbose=False, device=DEV)
    assert tr.spe == steps_per_epoch(504, 128) == 4 and tr.last_bs == 120     # the short batch is step 4 of the 6
    tr.fit()
    assert tr.gstep.use_graph and tr.gstep._graphs is not None

    def eager(launches):
        setup_seed(hp["seed"])
        system = MipNeRFSystem(dict(hp, precision="bf16"), precision="bf16").to(DEV)
        system.setup()
        system.fused_adam = True
        opts, scheds = system.configure_optimizers()
        opt, sched = opts[0], scheds[0]["scheduler"]
        step = GraphedTrainStep(system, opt, 128, DEV, use_graph=False) if launches else None
        loader = RayLoader(system.train_dataset, batch_size=128, shuffle=True, seed=hp["seed"])
        done = 0
        while done < K:
            for rays, gt in loader:
                if done == K:
                    break
                if step is not None and gt.shape[0] == 128:
                    for dst, src in zip(step.rays, rays):
                        dst.copy_(src)
                    step.gt.copy_(gt)
                    step()
                else:
                    opt.zero_grad()
                    system.training_step_native((rays, gt), done)
                    opt.step()
                    system.mip_nerf.mlp.native(DEV)        # re-pack before the next step's forward, as the trainer does
                sched.step()
                done += 1
        torch.cuda.synchronize()
        assert opt.steps == K
        return system, opt
    system, opt = eager(True)
    for (k, a), (k2, b) in zip(tr.system.state_dict().items(), system.state_dict().items()):
        assert k == k2 and torch.equal(a, b), k
    assert torch.equal(tr.opt.exp_avg, opt.exp_avg) and torch.equal(tr.opt.exp_avg_sq, opt.exp_avg_sq)
    assert tr.opt.steps == K and int(tr.opt._dev_step.item()) == K
    system, opt = eager(False)
    # Adam divides by sqrt(v): a round-off difference in a near-zero gradient element moves that parameter by up to ~lr (5e-4)
    diff = (tr.system.mip_nerf.mlp._flat_param - system.mip_nerf.mlp._flat_param).abs().max().item()
    assert diff <= 1e-4, diff


# ---- the command end to end ----------------------------------------------------------------------------------------------
def test_train_command_multicam_end_to_end_then_eval(tmp_path):
    from mipnerf_pl_amd.system import MipNeRFSystem
    from mipnerf_pl_amd.train import read_metrics
    from tests.lightning_standin import system_module_under_lightning
    data = fx.write_multicam_scene(str(tmp_path / "scene"))
    out = tmp_path / "out"
    _run(["mipnerf_pl_amd.train", "--data_path", data, "--out_dir", str(out), "--dataset_name", "multi_blender",
          "--log_every_n_steps", "10", "exp_name", "ms", "train.batch_size", "1024", "nerf.num_samples", "64", "optimizer.max_steps", "60",
          "optimizer.lr_delay_steps", "0", "val.check_interval", "20", "val.sample_num", "1", "val.chunk_size", "4096"], timeout=900)
    logs = out / "logs" / "ms" / "version_0"
    rows = read_metrics(str(logs / "metrics.csv"))
    train = [r["train/psnr"] for r in rows if "train/psnr" in r]
    val = [r for r in rows if "val/psnr" in r]
    assert len(train) == 6 and train[-1] > train[0] + 1.0, train
    assert [int(r["step"]) for r in val] == [19, 39, 59] and all(np.isfinite(r["val/loss"]) for r in val)
    assert all("lr" in r for r in rows if "train/psnr" in r)
    assert (logs / "hparams.yaml").exists()
    pngs = sorted(os.listdir(logs / "images"))
    assert len(pngs) == 6 and any("GT_coarse_fine" in p for p in pngs) and any("depth" in p for p in pngs)
    ckdir = out / "ckpt" / "ms"
    names = sorted(os.listdir(ckdir))
    tops = [n for n in names if n.startswith("epoch=")]
    assert "last.ckpt" in names and len(tops) == 2 and set(names) == set(tops) | {"last.ckpt"}, names
    assert all(n.endswith(".ckpt") and "-step=" in n for n in tops)
    ck = torch.load(str(ckdir / "last.ckpt"), map_location="cpu", weights_only=False)
    for k in ("epoch", "global_step", "pytorch-lightning_version", "state_dict", "optimizer_states", "lr_schedulers", "hparams_name",
              "hyper_parameters"):
        assert k in ck, k
    assert ck["global_step"] == 60 and ck["epoch"] == 0 and all(k.startswith("mip_nerf.mlp.") for k in ck["state_dict"])
    # the checkpoint loads unchanged: here, under the Lightning stand-in, and in the eval command
    MipNeRFSystem.load_from_checkpoint(str(ckdir / "last.ckpt"))
    system_module_under_lightning().MipNeRFSystem.load_from_checkpoint(str(ckdir / "last.ckpt"))
    _run(["mipnerf_pl_amd.eval", "--ckpt", str(ckdir / "last.ckpt"), "--data", data, "--out_dir", str(out), "--scale", "1",
          "--chunk_size", "4096"])
    psnrs = (out / "test" / "ms" / "psnrs.txt").read_text().split()
    assert len(psnrs) == 16 and all(np.isfinite(float(v)) for v in psnrs)


def test_train_command_blender(tmp_path):
    data = fx.write_blender(str(tmp_path / "d"))
    out = tmp_path / "out"
    _run(["mipnerf_pl_amd.train", "--data_path", data, "--out_dir", str(out), "--dataset_name", "blender", "train.batch_size", "128",
          "nerf.num_samples", "64", "optimizer.max_steps", "5", "val.check_interval", "2", "val.sample_num", "2", "val.chunk_size", "4096"])
    names = os.listdir(out / "ckpt" / "lego")
    assert "last.ckpt" in names and len(names) == 3
    ck = torch.load(str(out / "ckpt" / "lego" / "last.ckpt"), map_location="cpu", weights_only=False)
    assert ck["global_step"] == 5 and ck["hyper_parameters"]["dataset_name"] == "blender"


# ---- resume -------------------------------------------------------------------------------------------------------------------
def test_resume_is_exact_with_randomized_draws(tmp_path):
    from mipnerf_pl_amd.train import Trainer
    data = fx.write_multicam(str(tmp_path / "d"))
    kw = dict(optimizer__max_steps=10, val__check_interval=3, train__randomized=True)
    straight = Trainer(_hp(data, tmp_path / "a", "multi_blender", **kw), verbose=False, device=DEV).fit()
    Trainer(_hp(data, tmp_path / "b", "multi_blender", **kw), verbose=False, device=DEV).fit(until=3)
    half = str(tmp_path / "b" / "ckpt" / "t" / "last.ckpt")
    hck = torch.load(half, map_location="cpu", weights_only=False)
    assert hck["global_step"] == 3 and hck["mipnerf_trainer"]["batch"] == 3      # mid-epoch: the short last batch comes next
    resumed = Trainer(_hp(data, tmp_path / "c", "multi_blender", checkpoint__resume_path=half, **kw), verbose=False, device=DEV).fit()
    a = torch.load(str(tmp_path / "a" / "ckpt" / "t" / "last.ckpt"), map_location="cpu", weights_only=False)
    c = torch.load(str(tmp_path / "c" / "ckpt" / "t" / "last.ckpt"), map_location="cpu", weights_only=False)
    sa, ma, va, na = _state(a)
    sc, mc, vc, nc = _state(c)
    assert na == nc == 10 and a["global_step"] == c["global_step"] == 10
    for k in sa:
        assert torch.equal(sa[k], sc[k]), k
    assert torch.equal(ma, mc) and torch.equal(va, vc)
    assert straight.global_step == resumed.global_step == 10

    # the reference's checkpoint form: torch.optim.Adam's per-parameter state, no trainer record
    system = resumed.system
    params = list(system.mip_nerf.parameters())
    offs, off = {}, 0
    for p in system.mip_nerf.mlp.ordered_params():
        offs[id(p)] = off
        off += p.numel()
    _, m3, v3, n3 = _state(hck)
    state = {}
    for i, p in enumerate(params):
        o = offs[id(p)]
        state[i] = {"step": torch.tensor(float(n3)), "exp_avg": m3[o:o + p.numel()].view(p.shape).clone(),
                    "exp_avg_sq": v3[o:o + p.numel()].view(p.shape).clone()}
    ref = dict(hck)
    del ref["mipnerf_trainer"]
    ref["optimizer_states"] = [{"state": state, "param_groups": [{"lr": 5e-4, "betas": (0.9, 0.999), "eps": 1e-8, "weight_decay": 0,
                                                                  "amsgrad": False, "params": list(range(len(params)))}]}]
    path = str(tmp_path / "ref_form.ckpt")
    torch.save(ref, path)
    tr = Trainer(_hp(data, tmp_path / "e", "multi_blender", checkpoint__resume_path=path, **kw), verbose=False, device=DEV)
    assert tr.opt.steps == 3 and tr.global_step == 3
    assert torch.equal(tr.opt.exp_avg.cpu(), m3) and torch.equal(tr.opt.exp_avg_sq.cpu(), v3)
    tr.fit()
    assert tr.global_step == 10


# ---- fp32 / --no-graph -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [["--precision", "fp32"], ["--no-graph"]])
def test_eager_routes_write_a_loadable_checkpoint(tmp_path, flags):
    from mipnerf_pl_amd.system import MipNeRFSystem
    data = fx.write_multicam(str(tmp_path / "d"))
    out = tmp_path / "out"
    _run(["mipnerf_pl_amd.train", "--data_path", data, "--out_dir", str(out), "--dataset_name", "multi_blender"] + flags +
         ["train.batch_size", "128", "nerf.num_samples", "64", "optimizer.max_steps", "5", "val.check_interval", "2", "val.sample_num", "1",
          "val.chunk_size", "4096"])
    path = out / "ckpt" / "lego" / "last.ckpt"
    ck = torch.load(str(path), map_location="cpu", weights_only=False)
    assert ck["global_step"] == 5 and _state(ck)[3] == 5
    s = MipNeRFSystem.load_from_checkpoint(str(path))
    assert all(torch.isfinite(p).all() for p in s.parameters())


# ---- two ranks ---------------------------------------------------------------------------------------------------------------
def test_two_ranks_on_one_device_over_gloo(tmp_path):
    data = fx.write_multicam(str(tmp_path / "d"))
    out = tmp_path / "out"
    log = _run(["mipnerf_pl_amd.train", "--data_path", data, "--out_dir", str(out), "--dataset_name", "multi_blender",
                "--child_timeout", "500", "num_gpus", "2", "train.batch_size", "64", "nerf.num_samples", "64", "optimizer.max_steps", "6",
                "val.check_interval", "2", "val.sample_num", "1", "val.chunk_size", "4096"], timeout=600,
               env_extra={"MIPNERF_TRAIN_SHARE_GPU": "1"})
    assert "replicas identical on 2 ranks" in log, log[-2000:]
    assert sorted(os.listdir(out / "logs" / "lego")) == ["version_0"]
    names = os.listdir(out / "ckpt" / "lego")
    assert "last.ckpt" in names and len(names) == 3
    ck = torch.load(str(out / "ckpt" / "lego" / "last.ckpt"), map_location="cpu", weights_only=False)
    assert ck["global_step"] == 6
