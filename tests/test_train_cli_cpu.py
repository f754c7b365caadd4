"""CPU (no GPU): the training command's configuration semantics against the reference's own config loader (tests/golden/config_lego_merged.json,
scripts/make_golden_config.py), its epoch schedule as pure functions (sharding, steps per epoch, validation batches, top-k checkpoint
bookkeeping), the torch-Adam -> FlatAdam state mapping, and the C ABI of the in-graph batch producer."""
import argparse
import json
import os
import re
import types

import pytest
import torch

from mipnerf_pl_amd import config as cfg
from mipnerf_pl_amd import train as T

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden")


def _untag(v):
    if isinstance(v, dict) and "tuple" in v:
        return tuple(_untag(x) for x in v["tuple"])
    if isinstance(v, dict) and "none" in v:
        return None
    return v


def _golden(section):
    doc = json.load(open(os.path.join(GOLDEN, "config_lego_merged.json")))
    return doc["opts"], {k: (t, _untag(v)) for k, (t, v) in doc[section].items()}


def _typed(d):
    return {k: (type(v).__name__, v) for k, v in d.items()}


# ---- configuration -------------------------------------------------------------------------------------------------------
def test_load_equals_the_reference_loader_on_lego_yaml():
    _, want = _golden("loaded")
    assert _typed(cfg.load(os.path.join(GOLDEN, "config_lego.yaml"))) == want


def test_opts_merge_equals_the_reference_loader():
    opts, want = _golden("merged")
    got = cfg.merge_opts(cfg.load(os.path.join(GOLDEN, "config_lego.yaml")), opts)
    assert _typed(got) == want


def test_defaults_restate_lego_yaml_and_complete_the_system_defaults():
    from mipnerf_pl_amd.system import DEFAULT_HPARAMS
    assert _typed(cfg.DEFAULTS) == _typed(cfg.load(os.path.join(GOLDEN, "config_lego.yaml")))
    missing = set(DEFAULT_HPARAMS) - set(cfg.DEFAULTS)
    assert missing == {"nerf.unbounded"}          # this package's own key, not a reference one
    for k in ("seed", "num_gpus", "exp_name", "train.batch_type", "val.batch_type", "val.check_interval", "val.sample_num",
              "checkpoint.resume_path"):
        assert k in cfg.DEFAULTS and k not in DEFAULT_HPARAMS


def test_value_quirks(tmp_path):
    p = tmp_path / "q.yaml"
    p.write_text("optimizer:\n  lr_init: 5e-4\nnerf:\n  append_identity: Ture\n  shape: [1, 2, 3]\ncheckpoint:\n  resume_path: None\n"
                 "name: lego\nexpr: '1 + 1'\n")
    d = cfg.load(str(p))
    assert d["optimizer.lr_init"] == 0.0005 and isinstance(d["optimizer.lr_init"], float)
    assert d["nerf.append_identity"] == "Ture"
    assert d["nerf.shape"] == (1, 2, 3)
    assert d["checkpoint.resume_path"] is None
    assert d["name"] == "lego" and d["expr"] == "1 + 1"      # not a literal: stays a string
    assert cfg.parse_value("[4, 5]") == (4, 5) and cfg.parse_value("abc") == "abc" and cfg.parse_value("None") is None
    with pytest.raises(ValueError):
        cfg.merge_opts({}, ["a"])


def test_model_accepts_append_identity_ture_as_the_reference_does():
    from mipnerf_pl_amd.model import MipNerf
    m = MipNerf(num_samples=8, append_identity=cfg.DEFAULTS["nerf.append_identity"])
    assert m.mlp is not None


def test_merge_precedence(tmp_path):
    p = tmp_path / "c.yaml"
    p.write_text("exp_name: from_file\ntrain:\n  batch_size: 2048\nval:\n  sample_num: 2\n")
    args = argparse.Namespace(config=str(p), opts=["train.batch_size", "512", "extra.key", "7"], data_path="/data", exp_name="from_cli",
                              out_dir="/out")
    d = cfg.resolve(args)
    assert d["train.batch_size"] == 512            # opts over file over defaults
    assert d["val.sample_num"] == 2                # file over defaults
    assert d["val.check_interval"] == 10000        # defaults
    assert d["extra.key"] == 7
    assert d["exp_name"] == "from_file"            # a command-line argument never overrides a key
    assert d["data_path"] == "/data" and d["out_dir"] == "/out"
    d = cfg.resolve(argparse.Namespace(config=None, opts=[]))
    assert d == cfg.DEFAULTS | {"config": None, "opts": []}


def test_command_line_flags():
    a = T.build_parser().parse_args(["--data_path", "d", "--out_dir", "o", "--dataset_name", "blender", "train.batch_size", "64"])
    assert a.precision == "bf16" and a.use_graph and a.log_every_n_steps == 50 and a.opts == ["train.batch_size", "64"]
    a = T.build_parser().parse_args(["--data_path", "d", "--out_dir", "o", "--dataset_name", "multi_blender", "--precision", "fp32",
                                     "--no-graph", "--log_every_n_steps", "5"])
    assert a.precision == "fp32" and not a.use_graph and a.log_every_n_steps == 5


# ---- epoch schedule ------------------------------------------------------------------------------------------------------
class _IdDataset:
    """What RayLoader needs of a train split: its length, its device, and rays_at (here: the ids themselves)."""
    split, device = "train", torch.device("cpu")

    def __init__(self, n):
        self.n = n

    def __len__(self):
        return self.n

    def rays_at(self, ids):
        return ids.clone(), None


@pytest.mark.parametrize("world", [1, 2, 3])
@pytest.mark.parametrize("n,batch", [(1000, 64), (97, 10), (5, 4), (2, 3)])
def test_sharded_order_equals_rayloader(world, n, batch):
    from mipnerf_pl_amd.datasets import RayLoader
    for rank in range(world):
        loader = RayLoader(_IdDataset(n), batch_size=batch, shuffle=True, seed=4, rank=rank, world_size=world)
        for epoch in range(3):
            loader.set_epoch(epoch)
            want = torch.cat([ids for ids, _ in loader])
            got = T.epoch_order(n, 4, epoch, rank, world, torch.device("cpu"))
            assert torch.equal(got, want)
            assert len(loader) == T.steps_per_epoch(n, batch, world)
            sizes = [ids.numel() for ids, _ in loader]
            assert sizes[-1] == T.last_batch_size(n, batch, world) and all(s == batch for s in sizes[:-1])


def test_steps_per_epoch_and_short_batch():
    assert T.steps_per_epoch(10000, 4096) == 3 and T.last_batch_size(10000, 4096) == 1808
    assert T.steps_per_epoch(8192, 4096) == 2 and T.last_batch_size(8192, 4096) == 4096
    assert T.local_count(10001, 2) == 5001 and T.steps_per_epoch(10001, 1000, 2) == 6 and T.last_batch_size(10001, 1000, 2) == 1
    assert T.steps_per_epoch(640000 * 100, 3072) == 20834           # lego: 100 images of 800 x 800


def test_validation_batches():
    # every check_interval batches of an epoch, plus once after the final step
    runs = [(e, b) for e in range(3) for b in range(7) if e * 7 + b < 19 and T.should_validate(b, 3, e * 7 + b + 1, 19)]
    assert runs == [(0, 2), (0, 5), (1, 2), (1, 5), (2, 2), (2, 4)]
    assert not T.should_validate(0, 10000, 1, 5) and T.should_validate(4, 10000, 5, 5)


def test_top2_bookkeeping():
    k = T.TopK(2)
    assert k.update(20.0, 0, 9) == ("epoch=0-step=9.ckpt", [])
    assert k.update(22.0, 0, 19) == ("epoch=0-step=19.ckpt", [])
    assert k.update(21.0, 1, 29) == ("epoch=1-step=29.ckpt", ["epoch=0-step=9.ckpt"])
    assert k.update(19.0, 1, 39) == (None, [])
    assert k.update(21.0, 1, 49) == (None, [])                       # not strictly better than the worst kept
    assert k.update(float("nan"), 2, 59) == (None, [])
    assert k.update(23.0, 2, 69) == ("epoch=2-step=69.ckpt", ["epoch=1-step=29.ckpt"])
    assert set(k.best) == {"epoch=0-step=19.ckpt", "epoch=2-step=69.ckpt"}
    k2 = T.TopK(2)
    k2.load_state_dict(k.state_dict())
    assert k2.best == k.best
    assert k2.update(float("nan"), 3, 1) == (None, [])
    k3 = T.TopK(2)
    assert k3.update(float("nan"), 0, 0) == ("epoch=0-step=0.ckpt", [])


def test_torch_adam_state_maps_onto_the_flat_order_by_parameter_identity():
    from mipnerf_pl_amd.optim import FlatAdam
    from mipnerf_pl_amd.system import MipNeRFSystem
    system = MipNeRFSystem(dict(cfg.DEFAULTS, **{"nerf.num_samples": 8}))
    params = list(system.mip_nerf.parameters())
    adam = torch.optim.Adam(params, lr=1e-3)
    for i, p in enumerate(params):
        adam.state[p] = {"step": torch.tensor(7.0), "exp_avg": torch.full_like(p, float(i)), "exp_avg_sq": torch.full_like(p, i + 0.5)}
    sd = adam.state_dict()
    mlp = system.mip_nerf.mlp
    mlp.ordered_params = types.MethodType(lambda self: list(reversed(list(self.parameters()))), mlp)    # any flat order
    opt = FlatAdam(mlp, lr=5e-4)
    opt.load_state_dict(T.flat_adam_state_from_torch_adam(sd, system, opt))
    assert opt.steps == 7
    off = 0
    for p in mlp.ordered_params():
        i = next(j for j, q in enumerate(params) if q is p)
        n = p.numel()
        assert torch.all(opt.exp_avg[off:off + n] == float(i)) and torch.all(opt.exp_avg_sq[off:off + n] == i + 0.5)
        off += n
    assert off == opt.exp_avg.numel()


# ---- C ABI -----------------------------------------------------------------------------------------------------------------
def test_gather_train_batch_is_declared_and_exported():
    from mipnerf_pl_amd import _lib as L
    if not os.path.exists(L.LIB_PATH):
        from mipnerf_pl_amd import build
        build.build(verbose=False)
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "mipnerf_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+mipnerf_gather_train_batch\s*\(", src)
    assert hasattr(L.lib(), "mipnerf_gather_train_batch") and "mipnerf_gather_train_batch" in L.SIGNATURES
    assert L.lib().mipnerf_abi_version() == 6
    # argument validation happens before any HIP call
    assert L.lib().mipnerf_gather_train_batch(0, 0, None, 0, None, None, None, None, None, None, None, None) == L.E_INVALID
    assert b"gather_train_batch" in L.lib().mipnerf_last_error()
