"""CPU: host logic of the LightningModule mirror (no kernels): hyper-parameter contract, state_dict keys,
LR schedule, render-chunk slicing."""
import numpy as np
import torch

from mipnerf_pl_amd import Rays
from mipnerf_pl_amd.system import DEFAULT_HPARAMS, MipNeRFSystem, rearrange_render_image
from oracle import mipnerf_oracle as orc


def test_state_dict_keys_match_reference_checkpoints():
    sys_ = MipNeRFSystem(DEFAULT_HPARAMS)
    keys = list(sys_.state_dict().keys())
    assert keys == ["mip_nerf.mlp." + k for k in orc.param_shapes()]      # SURVEY.md section 5 (checkpoint surface)
    for k, shp in orc.param_shapes().items():
        assert tuple(sys_.state_dict()["mip_nerf.mlp." + k].shape) == shp


def test_lr_schedule_matches_reference_formula():
    sys_ = MipNeRFSystem(DEFAULT_HPARAMS)
    (opt,), (sch,) = sys_.configure_optimizers()
    assert sch["interval"] == "step" and isinstance(opt, torch.optim.Adam)
    s = sch["scheduler"]
    hp = DEFAULT_HPARAMS
    for step in (0, 1, 100, 2500, 5000, 500000, 1000000, 1200000):
        s.last_epoch = step
        delay = hp["optimizer.lr_delay_mult"] + (1 - hp["optimizer.lr_delay_mult"]) * np.sin(
            0.5 * np.pi * np.clip(step / hp["optimizer.lr_delay_steps"], 0, 1))
        t = np.clip(step / hp["optimizer.max_steps"], 0, 1)
        want = delay * np.exp(np.log(hp["optimizer.lr_init"]) * (1 - t) + np.log(hp["optimizer.lr_final"]) * t)
        assert abs(s.get_lr()[0] - want) <= 1e-12
    s.last_epoch = 0
    assert abs(s.get_lr()[0] - 5e-6) < 1e-12 and abs(MipNeRFSystem(DEFAULT_HPARAMS).configure_optimizers()[1][0][
        "scheduler"].get_last_lr()[0] - 5e-6) < 1e-12


def test_rearrange_render_image_chunks():
    H, W = 10, 13          # 130 rays, chunk 32 -> 4 full + ragged 2
    rays = Rays(*[torch.arange(H * W * k, dtype=torch.float32).reshape(1, H, W, k) for k in (3, 3, 3, 1, 1, 1, 1)])
    chunks, val_mask = rearrange_render_image(rays, 32)
    assert len(chunks) == 5 and [c.origins.shape[0] for c in chunks] == [32, 32, 32, 32, 2]
    assert val_mask.shape == (1, H, W, 1) and torch.equal(val_mask, rays.lossmult)
    assert torch.equal(torch.cat([c.directions for c in chunks]), rays.directions.reshape(-1, 3))
    # BASELINE configs[4]: 800x800 frame in 8192-ray chunks -> 79 chunks, ragged tail 1024
    n = 800 * 800
    assert -(-n // 8192) == 79 and n % 8192 == 1024


def test_checkpoint_roundtrip_in_lightning_format(tmp_path):
    """The checkpoint layout the reference's train.py writes / eval.py reads (Lightning): state_dict keys under
    `mip_nerf.mlp.` + hyper_parameters; must survive save -> load_from_checkpoint and accept a reference-style file."""
    import torch
    from mipnerf_pl_amd.system import DEFAULT_HPARAMS, MipNeRFSystem
    from oracle import mipnerf_oracle as orc
    hp = dict(DEFAULT_HPARAMS)
    hp["nerf.num_samples"] = 64
    system = MipNeRFSystem(hp)
    path = str(tmp_path / "ckpt.pt")
    if hasattr(system, "save_checkpoint"):
        system.save_checkpoint(path)
    else:      # real Lightning installed: write the same dict by hand
        torch.save({"state_dict": system.state_dict(), "hyper_parameters": hp}, path)
    ckpt = torch.load(path, weights_only=False)
    assert list(ckpt["state_dict"].keys()) == ["mip_nerf.mlp." + k for k in orc.param_shapes()]
    again = MipNeRFSystem.load_from_checkpoint(path)
    assert again.hparams["nerf.num_samples"] == 64
    for (k1, v1), (k2, v2) in zip(system.state_dict().items(), again.state_dict().items()):
        assert k1 == k2 and torch.equal(v1, v2)


def test_flat_mode_bookkeeping_survives_foreign_zero_grad():
    """MLP.flatten_parameters keeps names / shapes / leaf-ness; gradients reset by nn.Module.zero_grad() (set_to_none)
    must not leave a stale 'accumulated' flag behind; foreign .grad tensors are folded back into the flat buffer."""
    import torch
    from mipnerf_pl_amd import MipNerf
    m = MipNerf(num_samples=8)
    keys = list(m.state_dict().keys())
    mlp = m.mlp.flatten_parameters()
    assert list(m.state_dict().keys()) == keys and all(p.is_leaf and p.requires_grad for p in m.parameters())
    assert mlp.is_flat() and mlp.grads_are_flat()
    mlp._flat_grad.fill_(1.0)
    mlp._flat_grad_valid = True
    m.zero_grad()                                   # torch default: set_to_none=True
    assert not mlp.grads_are_flat()
    mlp.gather_foreign_grads()
    assert mlp.grads_are_flat() and mlp._flat_grad_valid is False
    w = m.mlp.color_layer.weight
    w.grad = torch.full_like(w, 3.0)                # a foreign gradient tensor (e.g. written by a generic autograd path)
    mlp.gather_foreign_grads()
    assert mlp.grads_are_flat() and mlp._flat_grad_valid is True and float(w.grad.mean()) == 3.0
    assert w.grad.data_ptr() != 0 and w.grad.data_ptr() >= mlp._flat_grad.data_ptr()


def test_flat_adam_state_dict_round_trip():
    """FlatAdam keeps its moments and step count in Optimizer.state, so a (Lightning) checkpoint's
    optimizer.state_dict() restores them like torch.optim.Adam's."""
    import torch
    from mipnerf_pl_amd import MipNerf
    from mipnerf_pl_amd.optim import FlatAdam
    m1, m2 = MipNerf(num_samples=8), MipNerf(num_samples=8)
    o1, o2 = FlatAdam(m1.mlp, lr=1e-3), FlatAdam(m2.mlp, lr=5e-4)
    st = o1.state[o1._key()]
    st["exp_avg"].uniform_(-1, 1)
    st["exp_avg_sq"].uniform_(0, 1)
    st["step"] += 7
    sd = o1.state_dict()
    assert len(sd["state"]) == 1 and set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}
    o2.load_state_dict(sd)
    assert o2.steps == 7 and o2.param_groups[0]["lr"] == 1e-3
    assert torch.equal(o2.exp_avg, o1.exp_avg) and torch.equal(o2.exp_avg_sq, o1.exp_avg_sq)
    assert o2.exp_avg.data_ptr() != o1.exp_avg.data_ptr()


def test_system_derives_from_lightning_module_when_available():
    """pytorch_lightning is not installed in this image, so the `_HAVE_PL` branch of system.py is exercised with a stand-in
    that has LightningModule's relevant surface (save_hyperparameters -> self.hparams as an attribute dict, self.log):
    the class must derive from it, build the same module tree / state_dict keys and run the host-side hooks."""
    import importlib
    import sys
    import types
    import torch

    class AttributeDict(dict):
        __getattr__ = dict.__getitem__

    class LightningModule(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self._hparams = AttributeDict()
            self._logged = {}

        @property
        def hparams(self):
            return self._hparams

        def save_hyperparameters(self, hp):
            self._hparams = AttributeDict(hp)

        def log(self, name, value, **kw):
            self._logged[name] = value

    stub = types.ModuleType("pytorch_lightning")
    stub.LightningModule = LightningModule
    import mipnerf_pl_amd.system as system_mod
    sys.modules["pytorch_lightning"] = stub
    try:
        mod = importlib.reload(system_mod)
        assert mod._HAVE_PL and issubclass(mod.MipNeRFSystem, LightningModule)
        s = mod.MipNeRFSystem(dict(mod.DEFAULT_HPARAMS))
        keys = list(s.state_dict().keys())
        assert keys[0] == "mip_nerf.mlp.layers.0.0.weight" and keys[-1] == "mip_nerf.mlp.color_layer.bias" and len(keys) == 24
        assert s.hparams['nerf.num_samples'] == 128
        (opt,), (sch,) = s.configure_optimizers()           # torch.optim.Adam + MipLRDecay (nerf_system.py:70-76)
        assert isinstance(opt, torch.optim.Adam) and sch["interval"] == "step"
        lr0 = opt.param_groups[0]["lr"]
        opt.step()
        sch["scheduler"].step()
        assert opt.param_groups[0]["lr"] > lr0                # warm-up
        s._log_lr()
        assert s._logged["lr"] == opt.param_groups[0]["lr"]   # nerf_system.py:117
    finally:
        del sys.modules["pytorch_lightning"]
        importlib.reload(system_mod)
    assert not system_mod._HAVE_PL


def test_same_seed_initialisation_equals_reference():
    """mip_nerf.py:19-73: a user who seeds torch and constructs MipNerf gets bit-for-bit the reference's initial weights
    (same Linear construction order, xavier_uniform on everything but color_layer) -- golden from the reference itself."""
    import os
    import numpy as np
    from mipnerf_pl_amd import MipNerf
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "init_seeded.npz"))
    for tag, kw in (("default", {}), ("w128", dict(mlp_net_width=128)), ("noview", dict(use_viewdirs=False, mlp_net_width_condition=256))):
        torch.manual_seed(int(g[tag + "_seed"]))
        sd = MipNerf(**kw).state_dict()
        for k, v in sd.items():
            a = v.numpy().ravel()
            assert np.array_equal(a[:8], g[f"{tag}_head_{k}"]), (tag, k)
            assert float(a.astype(np.float64).sum()) == float(g[f"{tag}_sum_{k}"]), (tag, k)


def test_bench_scale_model_and_pmc_round_rule(tmp_path):
    """bench.py helpers that need no GPU: the stated 1 / 2 / 4 / 8 expectation (VERDICT r03 #5a) and the rule that roofline.traffic only
    comes from THIS round's PMC passes (VERDICT r03 hygiene)."""
    import importlib.util
    import json
    import os
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    line = {"ms_per_step": 0.94, "train": {"ms_per_step": 4.2}, "render": {"ms_per_step": 144.0}}
    sm = bench.scale_model(line, 0.03, 4 * 612740)
    assert sm["predicted"]["1"] == {"train_ms_per_step": 4.2, "train_allreduce_ms": 0.0, "train_weak_efficiency": 1.0, "render_ms_per_frame": 144.0,
                                    "render_strong_efficiency": 1.0, "inference_weak_efficiency": 1.0}
    # ring all-reduce of 2.45 MB over 153 GB/s links + 3 us per hop + the measured launch: 8 GPUs = 30 + 28 + 42 us
    assert abs(sm["predicted"]["8"]["train_allreduce_ms"] - (0.03 + 2 * 7 / 8 * 2450960 / 153e9 * 1e3 + 14 * 3e-3)) < 1e-3
    assert sm["predicted"]["2"]["train_allreduce_ms"] < sm["predicted"]["4"]["train_allreduce_ms"] < sm["predicted"]["8"]["train_allreduce_ms"]
    assert 0.97 < sm["predicted"]["8"]["train_weak_efficiency"] < 1 and 0.99 < sm["predicted"]["8"]["render_strong_efficiency"] < 1
    assert bench.scale_model(line, {"error": "no rccl"}, 4 * 612740)["measured_inputs"]["allreduce_1rank_error"] == "no rccl"
    # PMC file of another round: refused, with the reason in the source string
    p = tmp_path / "mlp_pmc.json"
    p.write_text(json.dumps({"round": bench.CURRENT_ROUND - 1, "samples_per_launch": 524288, "hbm_bytes_per_launch": 1, "train_hbm_bytes_per_step": 2}))
    t, src = bench.pmc_traffic("inference", "bf16", 524288, path=str(p))
    assert t is None and "refused" in src
    p.write_text(json.dumps({"round": bench.CURRENT_ROUND, "samples_per_launch": 524288, "hbm_bytes_per_launch": 11, "train_hbm_bytes_per_step": 22,
                             "kernels": {"k_mlp_f32r": {"hbm_bytes_per_launch": 33}}}))
    assert bench.pmc_traffic("inference", "bf16", 524288, path=str(p))[0] == 11
    assert bench.pmc_traffic("inference", "fp32", 524288, path=str(p))[0] == 33
    assert bench.pmc_traffic("inference", "bf16", 1000, path=str(p)) == (None, None)
    assert bench.pmc_traffic("train", "bf16", path=str(p))[0] == 22
    # the committed file is this round's
    t, src = bench.pmc_traffic("inference", "bf16", 524288)
    assert t and t > 12124160 and "round" in src


def test_bench_write_outputs_caps_with_one_seeded_sample_of_rays(tmp_path):
    """bench.py --dump-outputs: float32 files named after the arrays; above the byte cap every array whose first axis is the rays keeps the
    same seeded rows (the same on every run), the rest is written whole."""
    import importlib.util
    import os
    import numpy as np
    spec = importlib.util.spec_from_file_location("bench_mod", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    rng = np.random.default_rng(1)
    arrays = {"level0_rgb": rng.random((1000, 3)), "level0_weights": rng.random((1000, 64)).astype(np.float32), "loss": np.float64(0.5)}
    assert bench.write_outputs(str(tmp_path / "all"), arrays) == ["level0_rgb", "level0_weights", "loss"]
    got = {k: np.load(tmp_path / "all" / (k + ".npy")) for k in arrays}
    assert all(a.dtype == np.float32 for a in got.values())
    assert np.array_equal(got["level0_rgb"], arrays["level0_rgb"].astype(np.float32)) and got["loss"] == 0.5
    cap = 100 * (3 + 64) * 4 + 4
    for run in ("a", "b"):
        bench.write_outputs(str(tmp_path / run), arrays, cap=cap)
    a = {k: np.load(tmp_path / "a" / (k + ".npy")) for k in arrays}
    assert sum(v.nbytes for v in a.values()) <= cap and a["level0_rgb"].shape == (100, 3) and a["level0_weights"].shape == (100, 64)
    rows = [int(np.flatnonzero((arrays["level0_rgb"].astype(np.float32) == r).all(1))[0]) for r in a["level0_rgb"]]
    assert rows == sorted(set(rows)) and np.array_equal(a["level0_weights"], arrays["level0_weights"][rows])
    assert all(np.array_equal(a[k], np.load(tmp_path / "b" / (k + ".npy"))) for k in arrays)


def test_unbounded_model_precision_rules_on_the_host():
    """MipNerf(unbounded=True): fp32 unless asked otherwise; bf16 is accepted (inference kernels exist since round 4) and can be switched to on
    a live model; an unknown precision is refused; the 672-wide first layer / skip concat follow from 42 features per degree"""
    import pytest
    from mipnerf_pl_amd import MipNerf
    from mipnerf_pl_amd import _lib as L
    m = MipNerf(num_samples=8, unbounded=True)
    assert m.precision == L.PREC_FP32 and m.mlp.precision == L.PREC_FP32
    assert tuple(m.mlp.layers[0][0].weight.shape) == (256, 672) and tuple(m.mlp.layers[5][0].weight.shape) == (256, 256 + 672)
    b = MipNerf(num_samples=8, unbounded=True, precision="bf16")
    assert b.precision == L.PREC_BF16 and b.mlp.precision == L.PREC_BF16
    assert m.set_precision("bf16") is m and m.precision == L.PREC_BF16 and m.mlp.precision == L.PREC_BF16
    m.set_precision("fp32")
    assert m.precision == L.PREC_FP32
    with pytest.raises(ValueError):
        m.set_precision("fp16")
    with pytest.raises(NotImplementedError):
        MipNerf(num_samples=8, unbounded=True, disparity=True)


def test_strict_lightning_standin_construct_configure_checkpoint(tmp_path):
    """VERDICT r05 #4, the CPU half (tests/lightning_standin.py: pytorch_lightning 1.5.2's LightningModule contract, strict): system.py's
    `_HAVE_PL` branch executes -- construction through `save_hyperparameters` (the hparams dict arrives through the constructor argument
    named `hparams`, as train.py:34 passes it), `configure_optimizers`, Lightning's checkpoint keys with the reference's parameter names,
    `load_from_checkpoint` through Lightning's constructor protocol, and the strictness itself (read-only properties, `log` outside a hook)."""
    import pytest
    import lightning_standin as pl
    mod = pl.system_module_under_lightning()
    import mipnerf_pl_amd.system as regular
    assert mod is not regular and not regular._HAVE_PL and mod._HAVE_PL
    hp = dict(mod.DEFAULT_HPARAMS)
    hp.update({"nerf.num_samples": 64, "exp_name": "cpu", "dataset_name": "blender"})
    system = mod.MipNeRFSystem(hp)
    assert isinstance(system, pl.LightningModule) and isinstance(system.hparams, pl.AttributeDict)
    assert system._hparams_name == "hparams" and system.hparams["nerf.num_samples"] == 64 and system.hparams_initial == system.hparams
    for name in ("hparams", "global_step", "current_epoch", "device"):
        with pytest.raises(AttributeError):
            setattr(system, name, 1)
    with pytest.raises(pl.MisconfigurationException):
        system.log("lr", 1.0)                                 # no trainer: self.log is an error
    drv = pl.LoopDriver(system)                               # configure_optimizers -> ([Adam], [{'scheduler': MipLRDecay, 'interval': 'step'}])
    assert type(drv.optimizer) is torch.optim.Adam and type(drv.scheduler).__name__ == "MipLRDecay"
    with pytest.raises(pl.MisconfigurationException):
        system._log_lr()                                      # a trainer, but no hook running
    drv._hook("_log_lr")
    assert float(drv.logged["_log_lr"]["lr"]) == pytest.approx(drv.optimizer.param_groups[0]["lr"])
    with pytest.raises(ValueError):
        drv._hook("log", "x", torch.zeros(2))                 # single-element values only
    path = str(tmp_path / "e.ckpt")
    ckpt = drv.save_checkpoint(path)
    assert list(ckpt["state_dict"]) == ["mip_nerf.mlp." + k for k in orc.param_shapes()] and ckpt["hparams_name"] == "hparams"
    assert ckpt["pytorch-lightning_version"] == "1.5.2" and set(ckpt) >= {"epoch", "global_step", "state_dict", "optimizer_states", "lr_schedulers", "hyper_parameters"}
    again = mod.MipNeRFSystem.load_from_checkpoint(path)
    assert again.hparams["exp_name"] == "cpu" and again.mip_nerf.num_samples == 64
    for (k1, v1), (k2, v2) in zip(system.state_dict().items(), again.state_dict().items()):
        assert k1 == k2 and torch.equal(v1, v2)
    # the regular (shim) class reads the same file: checkpoints interchange between an image with Lightning and one without
    third = regular.MipNeRFSystem.load_from_checkpoint(path)
    assert third.hparams["nerf.num_samples"] == 64 and torch.equal(third.state_dict()["mip_nerf.mlp.color_layer.bias"], system.state_dict()["mip_nerf.mlp.color_layer.bias"])
