"""CPU: span training's pieces that need no device -- the C entry point `mipnerf_occupancy_refresh` (declared, bound, exported, argument
validation), the `train.occupancy.*` configuration keys, the refresh schedule and the refusals of `TrainOccupancy.load_state_dict`."""
import argparse
import ctypes as C
import os
import re

import pytest
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the entry point ----------------------------------------------------------------------------------------------------------
def test_entry_point_is_declared_bound_and_exported():
    from mipnerf_pl_amd import _lib as L
    hdr = open(os.path.join(REPO, "include", "mipnerf_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    proto = re.search(r"int mipnerf_occupancy_refresh\(([^)]*)\)", code)
    assert proto is not None and "mipnerf_occupancy_refresh" in L.SIGNATURES
    assert len(proto.group(1).split(",")) == len(L.SIGNATURES["mipnerf_occupancy_refresh"][1]) == 9
    assert hasattr(L.lib(), "mipnerf_occupancy_refresh")
    assert L.lib().mipnerf_abi_version() == 6
    # the rule is stated once, in the header's comment
    h = re.sub(r"[\s*]+", " ", hdr)
    assert "running[p] = (fresh[p] > d || isnan(fresh[p]) || isnan(d)) ? fresh[p] : d" in h
    assert "Does not allocate or synchronise" in h[h.index("mipnerf_occupancy_refresh: the lattice"):h.index("mipnerf_ray_occupancy: live")]


def test_entry_point_validates_its_arguments_without_a_gpu():
    from mipnerf_pl_amd import _lib as L
    lib = L.lib()
    dims = (C.c_int32 * 3)(8, 8, 8)
    fresh, running, bits, scratch = 0x10000, 0x20000, 0x30000, 0x40000      # never dereferenced: every call below is refused before a launch

    def call(dims=dims, fresh=fresh, running=running, decay=0.95, thr=0.01, dilate=1, bits=bits, scratch=scratch):
        return lib.mipnerf_occupancy_refresh(dims, fresh, running, decay, thr, dilate, bits, scratch, None)
    for kw in (dict(dims=None), dict(fresh=None), dict(running=None), dict(bits=None)):
        assert call(**kw) == L.E_INVALID and "null" in L.last_error(), kw
    assert call(scratch=None) == L.E_INVALID and "scratch" in L.last_error()          # needed only when dilate > 0
    assert call(decay=1.5) == L.E_INVALID and "decay" in L.last_error()
    assert call(decay=-0.1) == L.E_INVALID and call(decay=float("nan")) == L.E_INVALID
    assert call(dilate=-1) == L.E_INVALID and "dilate" in L.last_error()
    assert call(thr=float("nan")) == L.E_INVALID
    assert call(dims=(C.c_int32 * 3)(1, 8, 8)) == L.E_INVALID
    assert call(dims=(C.c_int32 * 3)(2048, 2048, 2048)) == L.E_INVALID
    assert call(fresh=running) == L.E_INVALID and "overlap" in L.last_error()
    assert call(fresh=running + 4 * 511) == L.E_INVALID                               # the last point of one on the first of the other
    assert call(scratch=bits) == L.E_INVALID


# ---- configuration ------------------------------------------------------------------------------------------------------------
LEGO_KEYS = 49          # the keys of the reference configuration the defaults restate


def test_defaults_are_unchanged_and_the_keys_live_apart():
    from mipnerf_pl_amd import config as cfg
    assert len(cfg.DEFAULTS) == LEGO_KEYS and not any(k.startswith("train.occupancy") for k in cfg.DEFAULTS)
    assert cfg.TRAIN_OCCUPANCY_DEFAULTS == {
        "train.occupancy.enabled": False, "train.occupancy.grid": 128, "train.occupancy.threshold": 0.01, "train.occupancy.dilate": 1,
        "train.occupancy.decay": 0.95, "train.occupancy.interval": 16, "train.occupancy.bound": None, "train.occupancy.far_radius": None,
        "train.occupancy.span_samples": None}
    s = cfg.train_occupancy_settings(cfg.DEFAULTS)
    assert s == dict(enabled=False, grid=128, threshold=0.01, dilate=1, decay=0.95, interval=16, bound=None, far_radius=None,
                     span_samples=None)


def test_keys_parse_from_key_value_pairs():
    from mipnerf_pl_amd import config as cfg
    args = argparse.Namespace(config=None, dataset_name="blender", opts=[
        "train.occupancy.enabled", "True", "train.occupancy.grid", "32", "train.occupancy.threshold", "0.5", "train.occupancy.dilate", "0",
        "train.occupancy.decay", "0.5", "train.occupancy.interval", "3", "train.occupancy.bound", "1.5", "train.occupancy.far_radius", "40",
        "train.occupancy.span_samples", "64"])
    hp = cfg.resolve(args)
    s = cfg.train_occupancy_settings(hp)
    assert s == dict(enabled=True, grid=32, threshold=0.5, dilate=0, decay=0.5, interval=3, bound=1.5, far_radius=40.0, span_samples=64)
    assert isinstance(s["grid"], int) and isinstance(s["bound"], float)
    assert {k: v for k, v in hp.items() if k in cfg.DEFAULTS} == cfg.DEFAULTS           # nothing else moved


def test_keys_parse_from_a_config_file(tmp_path):
    from mipnerf_pl_amd import config as cfg
    path = tmp_path / "c.yaml"
    path.write_text("train:\n  occupancy:\n    enabled: true\n    interval: 8\n    bound: None\n")
    hp = cfg.resolve(argparse.Namespace(config=str(path), dataset_name="blender", opts=[]))
    s = cfg.train_occupancy_settings(hp)
    assert s["enabled"] is True and s["interval"] == 8 and s["bound"] is None and s["grid"] == 128


@pytest.mark.parametrize("key,value,word", [("grid", 3, "grid"), ("interval", 0, "interval"), ("decay", 1.5, "decay"), ("decay", -0.01, "decay")])
def test_settings_refusals(key, value, word):
    from mipnerf_pl_amd import config as cfg
    with pytest.raises(ValueError, match=word):
        cfg.train_occupancy_settings({"train.occupancy." + key: value})
    ok = {"grid": 4, "interval": 1, "decay": 1.0}[key]
    assert cfg.train_occupancy_settings({"train.occupancy." + key: ok})[key] == ok


def test_an_unknown_key_is_refused():
    from mipnerf_pl_amd import config as cfg
    with pytest.raises(ValueError, match="warmup"):
        cfg.train_occupancy_settings({"train.occupancy.warmup": 5})


# ---- the schedule -------------------------------------------------------------------------------------------------------------
def test_refresh_due_is_a_pure_function_of_the_step():
    from mipnerf_pl_amd.train_occupancy import refresh_due
    assert [s for s in range(10) if refresh_due(s, 3)] == [0, 3, 6, 9]
    assert all(refresh_due(s, 1) for s in range(5))
    assert [s for s in range(40) if refresh_due(s, 16)] == [0, 16, 32]
    assert refresh_due(0, 1000) and not refresh_due(999, 1000)


# ---- checkpoints --------------------------------------------------------------------------------------------------------------
def _occ(**kw):
    from mipnerf_pl_amd import config as cfg
    from mipnerf_pl_amd.train_occupancy import TrainOccupancy
    s = cfg.train_occupancy_settings({"train.occupancy.grid": kw.pop("grid", 8)})
    return TrainOccupancy(s, kw.pop("bound", 1.5), "cpu", **kw)


def test_state_dict_holds_the_lattice_and_the_settings():
    sd = _occ().state_dict()
    assert sd["running"].dtype == torch.float32 and sd["running"].device.type == "cpu" and tuple(sd["running"].shape) == (8, 8, 8)
    assert not bool(sd["running"].any())
    assert (sd["dims"], sd["bound"], sd["space"], sd["far_radius"]) == ((8, 8, 8), 1.5, None, None)
    assert (sd["threshold"], sd["dilate"], sd["decay"], sd["interval"]) == (0.01, 1, 0.95, 16)
    c = _occ(space="contracted", far_radius=30.0, bound=2.0)
    assert c.occupancy.space == "contracted" and c.state_dict()["far_radius"] == 30.0
    assert tuple(c.occupancy.bits.shape) == (7, 7, 1) and c.occupancy.bits.dtype == torch.uint32


def test_load_state_dict_refuses_another_grid():
    sd = _occ().state_dict()
    with pytest.raises(ValueError, match="dims"):
        _occ(grid=16).load_state_dict(sd)
    with pytest.raises(ValueError, match="box"):
        _occ(bound=2.0).load_state_dict(sd)
    with pytest.raises(ValueError, match="space"):
        _occ(space="contracted", far_radius=30.0).load_state_dict(sd)
    c = _occ(space="contracted", far_radius=30.0, bound=2.0)
    with pytest.raises(ValueError, match="far radius"):
        _occ(space="contracted", far_radius=31.0, bound=2.0).load_state_dict(c.state_dict())
    with pytest.raises(ValueError, match="far_radius"):
        _occ(space="contracted")


def test_spaces_of_model_and_grid_must_agree():
    from types import SimpleNamespace as NS
    from mipnerf_pl_amd.train_occupancy import check_spaces
    check_spaces(NS(unbounded=False), NS(space=None), "x")
    check_spaces(NS(unbounded=True), NS(space="contracted"), "x")
    with pytest.raises(NotImplementedError, match="unbounded=True models are not supported"):
        check_spaces(NS(unbounded=True), NS(space=None), "x")
    with pytest.raises(ValueError, match="this model is bounded"):
        check_spaces(NS(unbounded=False), NS(space="contracted"), "x")
