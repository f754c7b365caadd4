"""Exact-arithmetic cases of the MLP (models/mip_nerf.py:75-111) and its backward: small-integer weights, biases, encodings and
upstream gradients, chosen so that every product, every partial sum in any order, every bf16 store of an activation or delta and
the folded view matrix are exactly representable.  A correct kernel -- bf16 or fp32 operands, any dataflow, tile shape, MFMA shape
or reduction order -- must then return the float64 result bit for bit; an indexing, tail, ray-mapping, packing, fold, mask or
reduction error changes at least one integer.  CPU only (numpy + torch float64); nothing of the kernels or their plans is imported.

Recipe: every weight row has NNZ = 3 nonzeros (NNZ_HEAD = 8 for the density and colour heads) at random columns, each +-1; biases
are integers in {-1, 0, 1} (density bias 1, colour bias 0); encodings are integers in [-3, 3], view encodings in [-2, 2]; d_raw is
drawn from {-2, -1, 1, 2}, so no sample has a zero upstream gradient.  Sparse weights are inherent: dense integer layers leave
the 8 significand bits of bf16 within two layers.  The positions are random per case and seed, and the weight gradients are dense
where deltas and activations are live.

The conditions are CHECKED on the float64 pass (check_exact), never assumed; a draw that misses one advances the seed, at most
MAX_ROUNDS times.  The float64 pass is gpu_util.mlp_functional / mlp_grads."""
import collections

import numpy as np
import torch

import gpu_util as G
from oracle import mipnerf_oracle as orc

NNZ, NNZ_HEAD = 3, 8
ENC_RANGE, VENC_RANGE = 3, 2
D_RAW_VALUES = (-2, -1, 1, 2)
MAX_ROUNDS = 8
GRAD_LIMIT = 2.0 ** 22            # max |gradient entry| and max |raw|
SUM_LIMIT = 2.0 ** 24             # every integer up to here is a float32
MIN_SHARE, MIN_SHARE_M = 0.03, 65  # nonzero share of every used gradient tensor at M >= 65 (worst observed: 6 %, noview)


def bf16_exact(x):
    """every element of x (float64 tensor / array) is a bfloat16 value: it survives float32, and its low 16 float32 bits are 0"""
    a = np.asarray(x.detach() if torch.is_tensor(x) else x, dtype=np.float64)
    f = a.astype(np.float32)
    return bool(np.array_equal(f.astype(np.float64), a)) and not np.any(np.ascontiguousarray(f).view(np.uint32) & np.uint32(0xFFFF))


def draw(arch, B, N, seed, use_viewdirs=True):
    """one draw of the recipe: (params in make_params naming / shapes / order, enc [B,N,xyz_dim], venc [B,27], d_raw [B,N,4])"""
    rng = np.random.default_rng(seed)
    params = collections.OrderedDict()
    for k, shp in orc.param_shapes(**arch).items():
        head = k.startswith(("density_layer", "color_layer"))
        if k.endswith("weight"):
            rows, cols = shp
            nnz = min(cols, NNZ_HEAD if head else NNZ)
            where = np.argsort(rng.random((rows, cols)), axis=1)[:, :nnz]
            w = np.zeros(shp, np.float32)
            np.put_along_axis(w, where, rng.choice(np.float32([-1, 1]), (rows, nnz)), axis=1)
            params[k] = w
        elif head:
            params[k] = np.full(shp, 1.0 if k.startswith("density") else 0.0, np.float32)
        else:
            params[k] = rng.integers(-1, 2, shp).astype(np.float32)
    xyz = params["layers.0.0.weight"].shape[1]
    enc = rng.integers(-ENC_RANGE, ENC_RANGE + 1, (B, N, xyz)).astype(np.float32)
    venc = rng.integers(-VENC_RANGE, VENC_RANGE + 1, (B, 27)).astype(np.float32)
    d_raw = rng.choice(np.float32(D_RAW_VALUES), (B, N, 4))
    return params, enc, venc, d_raw


def float64_pass(params, enc, venc, d_raw, skip_index, use_viewdirs=True):
    """(raw [B,N,4], {name: gradient or None}, activations, deltas) in float64.  activations = every hidden layer's output and the
    bottleneck, deltas = the gradient with respect to each of them."""
    post = []
    raw, grads, _ = G.mlp_grads(params, enc, venc if use_viewdirs else None, d_raw, skip_index, torch.float64, post=post)
    return raw, grads, [t.detach() for t in post], [t.grad for t in post]


def check_exact(params, enc, venc, d_raw, raw, grads, acts, deltas, use_viewdirs=True):
    """None if the float64 pass meets every exactness condition, else the first one it misses (a string)"""
    M = enc.shape[0] * enc.shape[1]
    for name, seq in (("activation", acts), ("delta", deltas), ("input", (enc, venc, d_raw)), ("parameter", params.values())):
        for i, t in enumerate(seq):
            if not bf16_exact(t):
                return f"{name} {i} is not bf16-exact (max |.| = {float(np.abs(np.asarray(t)).max()):g})"
    if use_viewdirs:
        W = params["extra_layer.weight"].shape[0]
        Wv = params["view_layers.0.0.weight"].astype(np.float64)[:, :W]
        if not bf16_exact(Wv @ params["extra_layer.weight"].astype(np.float64)):
            return "the folded view matrix is not bf16-exact"
        if not bf16_exact(Wv @ params["extra_layer.bias"].astype(np.float64) + params["view_layers.0.0.bias"]):
            return "the folded view bias is not bf16-exact"
    if float(raw.abs().max()) >= GRAD_LIMIT:
        return "max |raw| >= 2^22"
    for k, g in grads.items():
        if g is None:
            continue
        if float(g.abs().max()) >= GRAD_LIMIT:
            return f"max |gradient| of {k} >= 2^22"
        nz = int(torch.count_nonzero(g))
        if nz == 0 or (M >= MIN_SHARE_M and nz < MIN_SHARE * g.numel()):
            return f"gradient of {k}: {nz} of {g.numel()} entries nonzero"
    # partial sums in ANY order stay integers below 2^24: a weight-gradient entry is a sum over samples of delta x activation, so
    # the sum over samples of (largest |delta| of the sample) x (largest |activation or input| of the sample, or 1 for a bias)
    # bounds the absolute sum behind every entry, whatever the layer
    dmax = torch.from_numpy(np.abs(d_raw).reshape(M, -1).max(1)).double()
    for d in deltas:
        dmax = torch.maximum(dmax, d.reshape(M, -1).abs().max(1).values)
    amax = torch.from_numpy(np.maximum(np.abs(enc).reshape(M, -1).max(1), 1.0)).double()
    amax = torch.maximum(amax, torch.from_numpy(np.repeat(np.abs(venc).max(1), enc.shape[1])).double())
    for a in acts:
        amax = torch.maximum(amax, a.reshape(M, -1).abs().max(1).values)
    if float((dmax * amax).sum()) >= SUM_LIMIT:
        return f"sum over samples of max |delta| x max |activation| = {float((dmax * amax).sum()):g} >= 2^24"
    return None


def exact_case(arch, B, N, seed, use_viewdirs=True):
    """arch = oracle make_params keywords (xyz_dim 96 or 672, any depth, skip period, one or two view layers).  Returns a dict:
    params, enc [B,N,xyz_dim], venc [B,27], d_raw [B,N,4] (float32 numpy), raw [B,N,4] and grads {name: tensor, None for a parameter
    the architecture does not use} (float64 torch), skip_index, use_viewdirs, seed (the seed actually used), rounds, and max_act /
    max_delta / max_grad / min_share of the accepted draw."""
    skip = arch.get("skip_index", 4)
    why = []
    for rounds in range(MAX_ROUNDS + 1):
        s = seed + rounds
        params, enc, venc, d_raw = draw(arch, B, N, s, use_viewdirs)
        raw, grads, acts, deltas = float64_pass(params, enc, venc, d_raw, skip, use_viewdirs)
        miss = check_exact(params, enc, venc, d_raw, raw, grads, acts, deltas, use_viewdirs)
        if miss is None:
            used = [g for g in grads.values() if g is not None]
            return dict(params=params, enc=enc, venc=venc, d_raw=d_raw, raw=raw, grads=grads, skip_index=skip,
                        use_viewdirs=use_viewdirs, seed=s, rounds=rounds,
                        max_act=max(float(a.abs().max()) for a in acts), max_delta=max(float(d.abs().max()) for d in deltas),
                        max_grad=max(float(g.abs().max()) for g in used),
                        min_share=min(int(torch.count_nonzero(g)) / g.numel() for g in used))
        why.append(f"seed {s}: {miss}")
    raise AssertionError(f"no exact draw within {MAX_ROUNDS} re-draws: " + "; ".join(why))


# ---- the cases of tests/test_gpu_mlp_exact.py (and of tests/test_exact_mlp_cpu.py, which proves them feasible without a GPU) ----------
# (B, N): M = B * N samples; the workgroup tile is 256 samples = 8 wave tiles of 32, and the view row of sample s is row s // N
SHAPES = [(1, 1),        # smallest case
          (1, 31),       # one short of a wave tile
          (3, 11),       # 33: the ray changes inside a wave tile; one row past it
          (5, 13),       # 65
          (3, 85),       # 255: one short of a workgroup tile
          (1, 257),      # one row past a workgroup tile
          (27, 19),      # 513
          (33, 65),      # 2145: nine workgroup tiles, the last with 97 rows
          (17, 241)]     # 4097: many wgrad work tiles per split, one row in the last tile
VARIANT_SHAPES = [(3, 11), (33, 65)]
# name -> (oracle make_params keywords, use_viewdirs)
ARCHS = {"default": ({}, True),
         "w128": (dict(net_width=128, net_width_condition=128), True),
         "noview": (dict(net_width_condition=256), False),       # gradients of unused parameters must be exactly zero
         "d6s3": (dict(net_depth=6, skip_index=3), True),
         "dc2": (dict(net_depth_condition=2), True),
         "unbounded": (dict(xyz_dim=672), True),                  # row-major 672-wide encodings
         "w512": (dict(net_width=512, net_width_condition=256), True),      # bf16 inference only
         "w200c72": (dict(net_width=200, net_width_condition=72), True)}    # zero-padded on the 256 / 128 kernels
CASES = [("default", B, N) for B, N in SHAPES] + [(a, B, N) for a in ARCHS if a != "default" for B, N in VARIANT_SHAPES]
_CACHE = {}


def case(name, B, N):
    """exact_case of a named architecture at seed 1000 B + N: computed once per process, shared, never modified"""
    key = (name, B, N)
    if key not in _CACHE:
        arch, views = ARCHS[name]
        _CACHE[key] = exact_case(arch, B, N, 1000 * B + N, views)
    return _CACHE[key]
