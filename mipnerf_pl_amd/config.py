"""Hyper-parameters of a training run, with the semantics of the reference's YAML configs (configs/*.yaml, configs/config.py).

A configuration is one FLAT dict: nested YAML sections become dotted keys (`train.batch_size`, `nerf.mlp.net_width`).
`DEFAULTS` is the reference's `configs/lego.yaml` (its train.py's default `--config`; the reference's `default.yaml` is empty), which
completes `system.DEFAULT_HPARAMS` with the run-level keys (`seed`, `num_gpus`, `exp_name`, `train.batch_type`, `val.*`,
`checkpoint.resume_path`, ...).  `parse_args` merges, later winning:

    DEFAULTS  <-  [SCENE360_PRESET]  <-  --config FILE  <-  trailing KEY VALUE pairs  <-  command-line arguments that are not yet keys

(the preset only for `--dataset_name llff | realdata360`: captured, unbounded scenes without a white background).

Every leaf value goes through the same rule: `yaml.safe_load` first, then a string is tried with `ast.literal_eval` (falling back to the
string itself), and a list becomes a tuple.  So the reference's quirks hold here too: `5e-4` (a string to YAML 1.1) becomes 0.0005,
`None` becomes None, and `append_identity: Ture` stays the string 'Ture' (truthy, as the model reads it).
"""
from __future__ import annotations

import argparse
import ast

DEFAULTS = {
    'seed': 4, 'num_gpus': 1, 'exp_name': 'lego',
    'train.batch_size': 3072, 'train.batch_type': 'all_images', 'train.num_work': 4, 'train.randomized': True,
    'train.white_bkgd': True,
    'val.batch_size': 1, 'val.batch_type': 'single_image', 'val.num_work': 4, 'val.randomized': False, 'val.white_bkgd': True,
    'val.check_interval': 10000, 'val.chunk_size': 8192, 'val.sample_num': 4,
    'nerf.num_samples': 128, 'nerf.num_levels': 2, 'nerf.resample_padding': 0.01, 'nerf.stop_resample_grad': True,
    'nerf.use_viewdirs': True, 'nerf.disparity': False, 'nerf.ray_shape': 'cone', 'nerf.min_deg_point': 0,
    'nerf.max_deg_point': 16, 'nerf.deg_view': 4, 'nerf.density_activation': 'softplus', 'nerf.density_noise': 0.0,
    'nerf.density_bias': -1.0, 'nerf.rgb_activation': 'sigmoid', 'nerf.rgb_padding': 0.001, 'nerf.disable_integration': False,
    'nerf.append_identity': 'Ture',
    'nerf.mlp.net_depth': 8, 'nerf.mlp.net_width': 256, 'nerf.mlp.net_depth_condition': 1, 'nerf.mlp.net_width_condition': 128,
    'nerf.mlp.net_activation': 'relu', 'nerf.mlp.skip_index': 4, 'nerf.mlp.num_rgb_channels': 3, 'nerf.mlp.num_density_channels': 1,
    'optimizer.lr_init': 0.0005, 'optimizer.lr_final': 5e-06, 'optimizer.lr_delay_steps': 2500, 'optimizer.lr_delay_mult': 0.01,
    'optimizer.max_steps': 1000000,
    'loss.disable_multiscale_loss': False, 'loss.coarse_loss_mult': 0.1,
    'checkpoint.resume_path': None,
}


# layered over the defaults for the captured-scene data sets: the unbounded model, no white background behind a photograph
SCENE360_DATASETS = ("llff", "realdata360")
SCENE360_PRESET = {'nerf.unbounded': True, 'train.white_bkgd': False, 'val.white_bkgd': False, 'exp_name': 'scene360'}


# Span training (train_occupancy.TrainOccupancy): not reference keys, so they stay out of DEFAULTS (which is the reference's lego.yaml)
# and are read with `train_occupancy_settings`.  `decay` and `interval` are instant-ngp's choices, not measurements of this project;
# `threshold` is the rendering default of `--cull` (a foggy field needs a higher one).
TRAIN_OCCUPANCY_DEFAULTS = {
    'train.occupancy.enabled': False, 'train.occupancy.grid': 128, 'train.occupancy.threshold': 0.01, 'train.occupancy.dilate': 1,
    'train.occupancy.decay': 0.95, 'train.occupancy.interval': 16, 'train.occupancy.bound': None, 'train.occupancy.far_radius': None,
    'train.occupancy.span_samples': None,
}


def train_occupancy_settings(config):
    """The `train.occupancy.*` keys of a configuration without the prefix, TRAIN_OCCUPANCY_DEFAULTS where a key is absent; a grid below
    4 points per axis, an interval below 1 step and a decay outside [0, 1] are refused."""
    n = len('train.occupancy.')
    s = {k[n:]: config.get(k, v) for k, v in TRAIN_OCCUPANCY_DEFAULTS.items()}
    unknown = sorted(k for k in config if str(k).startswith('train.occupancy.') and k not in TRAIN_OCCUPANCY_DEFAULTS)
    if unknown:
        raise ValueError(f"unknown key(s) {unknown}; train.occupancy has {sorted(TRAIN_OCCUPANCY_DEFAULTS)}")
    s['enabled'] = bool(s['enabled'])
    s['grid'], s['dilate'], s['interval'] = int(s['grid']), int(s['dilate']), int(s['interval'])
    s['threshold'], s['decay'] = float(s['threshold']), float(s['decay'])
    for k in ('bound', 'far_radius'):
        s[k] = None if s[k] is None else float(s[k])
    s['span_samples'] = None if s['span_samples'] is None else int(s['span_samples'])
    if s['grid'] < 4:
        raise ValueError(f"train.occupancy.grid must be at least 4 points per axis (got {s['grid']})")
    if s['interval'] < 1:
        raise ValueError(f"train.occupancy.interval must be at least 1 step (got {s['interval']})")
    if not 0.0 <= s['decay'] <= 1.0:
        raise ValueError(f"train.occupancy.decay must be in [0, 1] (got {s['decay']})")
    if s['dilate'] < 0:
        raise ValueError(f"train.occupancy.dilate must be >= 0 (got {s['dilate']})")
    return s


# Error-guided batch sampling (train_guided.TrainGuided): not reference keys either, read with `train_guided_settings`.  `tile` (pixels),
# `interval` (steps between two refreshes of the map), `mix` (lambda: the share of a batch drawn in proportion to the error) and `rate`
# (alpha of the running error) are choices, not measurements of this project.
TRAIN_GUIDED_DEFAULTS = {
    'train.guided.enabled': False, 'train.guided.tile': 16, 'train.guided.interval': 64, 'train.guided.mix': 0.5, 'train.guided.rate': 0.25,
}


def train_guided_settings(config):
    """The `train.guided.*` keys of a configuration without the prefix, TRAIN_GUIDED_DEFAULTS where a key is absent.  Refused: an unknown
    `train.guided.*` key, tile < 1, interval < 1, mix outside [0, 1), rate outside (0, 1]."""
    n = len('train.guided.')
    s = {k[n:]: config.get(k, v) for k, v in TRAIN_GUIDED_DEFAULTS.items()}
    unknown = sorted(k for k in config if str(k).startswith('train.guided.') and k not in TRAIN_GUIDED_DEFAULTS)
    if unknown:
        raise ValueError(f"unknown key(s) {unknown}; train.guided has {sorted(TRAIN_GUIDED_DEFAULTS)}")
    s['enabled'] = bool(s['enabled'])
    s['tile'], s['interval'] = int(s['tile']), int(s['interval'])
    s['mix'], s['rate'] = float(s['mix']), float(s['rate'])
    if s['tile'] < 1:
        raise ValueError(f"train.guided.tile must be at least 1 pixel (got {s['tile']})")
    if s['interval'] < 1:
        raise ValueError(f"train.guided.interval must be at least 1 step (got {s['interval']})")
    if not 0.0 <= s['mix'] < 1.0:
        raise ValueError(f"train.guided.mix must be in [0, 1) (got {s['mix']})")
    if not 0.0 < s['rate'] <= 1.0:
        raise ValueError(f"train.guided.rate must be in (0, 1] (got {s['rate']})")
    return s


def check_train_guided(config):
    """`train_guided_settings(config)`, and with the sampler enabled the configurations it does not serve are refused by key: more than
    one rank (one map per run; no collective is built) and a loss that ignores `lossmult` (the importance weights ride on it)."""
    s = train_guided_settings(config)
    if s['enabled']:
        if int(config.get('num_gpus', 1)) > 1:
            raise NotImplementedError(f"train.guided.enabled needs num_gpus 1 (got num_gpus {config.get('num_gpus')}): the error map is "
                                      "kept per run and is not shared between ranks")
        if config.get('loss.disable_multiscale_loss', False):
            raise ValueError("train.guided.enabled cannot be combined with loss.disable_multiscale_loss True: that loss ignores the "
                             "per-ray lossmult, which carries the importance weights")
    return s


def parse_value(v):
    """One leaf: a string through ast.literal_eval when it parses, a list as a tuple."""
    if isinstance(v, str):
        try:
            v = ast.literal_eval(v)
        except (ValueError, SyntaxError):
            pass
    if isinstance(v, list):
        v = tuple(v)
    return v


def flatten(tree, prefix=""):
    """Nested dict (a parsed YAML document) -> flat dict of dotted keys with parsed leaves.  None (an empty file) -> {}."""
    out = {}
    for k, v in (tree or {}).items():
        if isinstance(v, dict):
            out.update(flatten(v, f"{prefix}{k}."))
        else:
            out[prefix + str(k)] = parse_value(v)
    return out


def load(path):
    """The flat configuration of one YAML file."""
    import yaml
    with open(path) as f:
        return flatten(yaml.safe_load(f))


def merge_opts(config, opts):
    """Trailing `KEY VALUE ...` pairs of the command line into `config` (in place); values parsed like file values."""
    opts = list(opts or [])
    if len(opts) % 2:
        raise ValueError(f"opts must be KEY VALUE pairs, got {len(opts)} items: {opts}")
    for k, v in zip(opts[0::2], opts[1::2]):
        config[k] = parse_value(v)
    return config


def resolve(args: argparse.Namespace, defaults=None):
    """The configuration of a parsed command line: defaults (with SCENE360_PRESET over them when `args.dataset_name` is one of
    SCENE360_DATASETS), then `args.config`, then `args.opts`, then every other attribute of `args` whose name is not a key yet (so
    --data_path, --out_dir, --dataset_name land in the dict; a config key is not overridden)."""
    config = dict(DEFAULTS if defaults is None else defaults)
    if getattr(args, "dataset_name", None) in SCENE360_DATASETS:
        config.update(SCENE360_PRESET)
    if getattr(args, "config", None) is not None:
        config.update(load(args.config))
    merge_opts(config, getattr(args, "opts", None))
    for k, v in vars(args).items():
        if k not in config:
            config[k] = v
    return config


def parse_args(parser: argparse.ArgumentParser, argv=None):
    return resolve(parser.parse_args(argv))
