"""CPU: the exact-arithmetic cases of tests/exact_mlp_fixture.py (the anchor of tests/test_gpu_mlp_exact.py), without a GPU.

  * every (arch, B, N) the GPU module runs meets the exactness conditions within the fixture's 8 re-draws;
  * the fixture's float64 raw and gradients equal the oracle's fp32 numpy restatement (oracle.mlp_forward / mlp_backward) EXACTLY:
    two restatements, both in exact arithmetic;
  * the plan emulations (mlp_plan.emulate_wave, mlp_pre_plan.emulate_pre_wave, mlp_train_plan.emulate_train, all with bf16
    rounding) reproduce the fixture EXACTLY at M = 33 and 65: pack, bias, job and reduction tables, the fold and post_process,
    with equality where the real-valued tests allow 1e-2;
  * the anchor's own guard: four one-element errors a kernel could make each change raw or a gradient of the float64 pass."""
import functools

import numpy as np
import pytest
import torch

import exact_mlp_fixture as X
from mipnerf_pl_amd.mlp_plan import Arch, Plan, emulate_wave
from mipnerf_pl_amd.mlp_pre_plan import PrePlan, emulate_pre_wave
from mipnerf_pl_amd.mlp_train_plan import TrainPlan, emulate_train
from oracle import mipnerf_oracle as orc

EMU_SHAPES = [(3, 11), (5, 13)]          # M = 33 (the ray changes inside a wave tile, one row past it) and 65
# the generated variants (csrc/gen_mlp_bf16.py: VARIANTS) by their name in the fixture; w512 has no bf16 training kernels
FORWARD = ["default", "w128", "noview", "d6s3", "unbounded", "dc2", "w512"]
TRAINABLE = ["default", "w128", "noview", "d6s3", "dc2", "unbounded"]


def _arch(name):
    kw, views = X.ARCHS[name]
    if name == "unbounded":
        return Arch(xyz_dim=672, feat_per_deg=42, bf16_kernels=False)
    return Arch(use_viewdirs=views, **kw)


def _oracle_kw(name):
    kw = X.ARCHS[name][0]
    return dict(skip_index=kw.get("skip_index", 4), net_depth=kw.get("net_depth", 8), net_depth_condition=kw.get("net_depth_condition", 1))


def _flat_inputs(name, B, N):
    """the case as the emulations take it: flat parameters, enc [M, xyz], view [M, 32] (the ray's row repeated), d_raw [M, 4]"""
    c = X.case(name, B, N)
    arch = _arch(name)
    assert [n for n, _ in arch.param_shapes()] == list(c["params"])
    flat = np.concatenate([v.ravel() for v in c["params"].values()])
    view = np.zeros((B * N, 32), np.float32)
    if c["use_viewdirs"]:
        view[:, :27] = np.repeat(c["venc"], N, axis=0)
    return c, arch, flat, c["enc"].reshape(B * N, -1), view, c["d_raw"].reshape(B * N, 4)


def _by_wave(fn, enc, view):
    """a one-wavefront emulation (32 samples) over M samples; the last wave tile repeats its last sample, like the kernels' clamp"""
    M = enc.shape[0]
    rgb, den = [], []
    for t in range(0, M, 32):
        idx = np.minimum(np.arange(t, t + 32), M - 1)
        r, d = fn(enc[idx], view[idx])
        rgb.append(r)
        den.append(d)
    return np.concatenate([np.concatenate(rgb), np.concatenate(den)[:, None]], axis=1)[:M]


@pytest.mark.parametrize("name,B,N", X.CASES)
def test_every_gpu_case_meets_the_exactness_conditions(name, B, N):
    c = X.case(name, B, N)          # raises when no draw within 8 re-draws meets the conditions
    print(f"exact case {name} {B}x{N}: seed {c['seed']} ({c['rounds']} re-draws), largest activation {c['max_act']:g}, delta "
          f"{c['max_delta']:g}, gradient {c['max_grad']:g}, smallest nonzero share {c['min_share']:.3f}")
    assert c["rounds"] <= X.MAX_ROUNDS and c["max_act"] <= 256 and c["max_grad"] < 2 ** 22
    unused = [k for k, g in c["grads"].items() if g is None]
    assert (len(unused) == 4) == (name == "noview"), unused


def test_a_draw_that_is_not_exact_is_refused():
    """the fixture verifies, it does not assume: an activation above 256 that is odd, a fractional weight and a folded matrix
    entry that needs nine bits are each named"""
    assert X.bf16_exact(np.float64([256, -255, 0.5, 3 * 2.0 ** 20])) and not X.bf16_exact(np.float64([257]))
    assert not X.bf16_exact(np.float64([1 + 2.0 ** -30]))
    arch, views = X.ARCHS["default"]
    params, enc, venc, d_raw = X.draw(arch, 3, 11, 5)
    for k, v in (("layers.2.0.bias", 300.0), ("layers.1.0.weight", 0.3)):
        p = dict(params)
        p[k] = params[k].copy()
        p[k].flat[0] = v
        miss = X.check_exact(p, enc, venc, d_raw, *X.float64_pass(p, enc, venc, d_raw, 4))
        assert miss is not None and "not bf16-exact" in miss, (k, miss)
    p = dict(params)
    p["extra_layer.weight"] = np.full_like(params["extra_layer.weight"], 1.0)
    p["view_layers.0.0.weight"] = np.full_like(params["view_layers.0.0.weight"], 1.0)
    p["view_layers.0.0.weight"][:, 0] = 2.0          # folded entry 257
    assert not X.bf16_exact(p["view_layers.0.0.weight"].astype(np.float64)[:, :256] @ p["extra_layer.weight"].astype(np.float64))


@pytest.mark.parametrize("name,B,N", [c for c in X.CASES if c[1:] in [(3, 11), (33, 65), (1, 1), (1, 257)]])
def test_fixture_equals_the_oracle_exactly(name, B, N):
    c = X.case(name, B, N)
    venc = c["venc"] if c["use_viewdirs"] else None
    rgb, den = orc.mlp_forward(c["params"], c["enc"], venc, **_oracle_kw(name))
    assert np.array_equal(np.concatenate([rgb, den], -1).astype(np.float64), c["raw"].numpy())
    og = orc.mlp_backward(c["params"], c["enc"], venc, c["d_raw"][..., :3], c["d_raw"][..., 3:], **_oracle_kw(name))
    for k, g in c["grads"].items():
        want = np.zeros(og[k].shape) if g is None else g.numpy()
        assert np.array_equal(og[k].astype(np.float64), want), k


@pytest.mark.parametrize("B,N", EMU_SHAPES)
@pytest.mark.parametrize("name", FORWARD)
def test_forward_emulation_reproduces_the_fixture_exactly(name, B, N):
    """emulate_wave with bf16 rounding on the plain and the folded plan (the unbounded variant: its two-kernel and one-kernel forms)"""
    c, arch, flat, enc, view, _ = _flat_inputs(name, B, N)
    want = c["raw"].reshape(B * N, 4).numpy()
    if name == "unbounded":
        p = PrePlan.build(arch)
        forms = {"two-kernel": lambda e, v: emulate_pre_wave(p, flat, e, v, round_bf16=True),
                 "one-kernel": lambda e, v: emulate_wave(p.fused, flat, e, v, round_bf16=True)}
    else:
        plain, folded = Plan.build(arch), Plan.build(arch, fold_view=True)
        assert folded.fold_view == c["use_viewdirs"]
        forms = {"plain": lambda e, v: emulate_wave(plain, flat, e, v, round_bf16=True),
                 "folded": lambda e, v: emulate_wave(folded, flat, e, v, round_bf16=True)}
    for form, fn in forms.items():
        got = _by_wave(fn, enc, view)
        bad = np.argwhere(got.astype(np.float64) != want)
        assert bad.size == 0, (form, len(bad), bad[0].tolist())


@functools.lru_cache(maxsize=None)
def _train_plan(name, fold):
    return TrainPlan.build(_arch(name), pre_gemm=name == "unbounded", fold_view=fold)


@pytest.mark.parametrize("B,N", EMU_SHAPES)
@pytest.mark.parametrize("name", TRAINABLE)
def test_training_emulation_reproduces_the_fixture_exactly(name, B, N):
    """emulate_train with bf16 rounding (the plan the device runs: folded forward-with-save, unfolded for the pre-GEMM form): raw and
    every parameter gradient, unused parameters zero, every parameter fed by one partial position"""
    c, arch, flat, enc, view, d_raw = _flat_inputs(name, B, N)
    tp = _train_plan(name, True)
    g, seen, raw = emulate_train(tp, flat, enc, view, d_raw, round_bf16=True)
    offs, nparams = tp.fwd.param_offsets()
    assert int(seen[:nparams].max()) == 1 and g.size == nparams == flat.size
    bad = np.argwhere(raw.astype(np.float64) != c["raw"].reshape(B * N, 4).numpy())
    assert bad.size == 0, ("raw", len(bad), bad[0].tolist())
    for i, (k, want) in enumerate(c["grads"].items()):
        got = g[offs[i]:offs[i] + c["params"][k].size].astype(np.float64)
        want = np.zeros(got.size) if want is None else want.numpy().ravel()
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (k, len(bad), int(bad[0]), got[bad[0]], want[bad[0]])


def test_unfolded_training_emulation_reproduces_the_fixture_exactly():
    """the fold is exact on these cases, so the unfolded plan gives the same integers"""
    c, arch, flat, enc, view, d_raw = _flat_inputs("default", 3, 11)
    tp = _train_plan("default", False)
    g, _, raw = emulate_train(tp, flat, enc, view, d_raw, round_bf16=True)
    assert np.array_equal(raw.astype(np.float64), c["raw"].reshape(33, 4).numpy())
    assert np.array_equal(g.astype(np.float64), np.concatenate([v.numpy().ravel() for v in c["grads"].values()]))


# ---- sensitivity: what the equality on the device would have caught -------------------------------------------------------------
def _moved(c, raw, grads):
    """names of the tensors (raw or a parameter gradient) that differ from the case's"""
    out = [] if torch.equal(raw, c["raw"][:raw.shape[0], :raw.shape[1]]) else ["raw"]
    return out + [k for k, g in grads.items() if g is not None and not torch.equal(g, c["grads"][k])]


def test_one_element_errors_change_the_float64_result():
    """(33, 65) default case: a dropped last sample, the neighbour ray's view row, two swapped nonzero columns of a weight row and a
    folded-matrix nonzero moved by one column each change raw or a gradient, so the equality asserted on the device sees them."""
    c = X.case("default", 33, 65)
    p, enc, venc, d_raw, B, N = c["params"], c["enc"], c["venc"], c["d_raw"], 33, 65
    M = B * N
    # (1) sample 2144 dropped: its upstream gradient never arrives
    d = d_raw.copy()
    d.reshape(M, 4)[M - 1] = 0
    raw, g, _, _ = X.float64_pass(p, enc, venc, d, 4)
    moved = _moved(c, raw, g)
    assert "layers.0.0.weight" in moved and "color_layer.bias" in moved, moved
    # (2) view row (s + 1) // N: the last sample of every ray reads the next ray's view encoding
    rows = np.minimum((np.arange(M) + 1) // N, B - 1)
    raw, g, _, _ = X.float64_pass(p, enc.reshape(M, 1, 96), venc[rows], d_raw.reshape(M, 1, 4), 4)
    assert not torch.equal(raw.reshape(B, N, 4), c["raw"]) or _moved(c, c["raw"], g)
    # (3) two nonzero columns of a row of layers.5.0.weight (+1 and -1) swapped
    w = p["layers.5.0.weight"].copy()
    row = next(r for r in range(w.shape[0]) if w[r].min() < 0 < w[r].max())
    a, b = int(np.argmax(w[row])), int(np.argmin(w[row]))
    w[row, a], w[row, b] = w[row, b], w[row, a]
    raw, g, _, _ = X.float64_pass(dict(p, **{"layers.5.0.weight": w}), enc, venc, d_raw, 4)
    assert _moved(c, raw, g)
    # (4) one nonzero of the folded view matrix V = W_view0[:, :W] @ W_extra moved by one column, in the folded form of the view layer
    # (which, unperturbed, is the fixture's raw rgb)
    _, _, acts, _ = X.float64_pass(p, enc, venc, d_raw, 4)
    trunk = acts[7].reshape(M, 256)
    wv = torch.from_numpy(p["view_layers.0.0.weight"]).double()
    V = wv[:, :256] @ torch.from_numpy(p["extra_layer.weight"]).double()
    bias = wv[:, :256] @ torch.from_numpy(p["extra_layer.bias"]).double() + torch.from_numpy(p["view_layers.0.0.bias"]).double()
    view = torch.from_numpy(np.repeat(venc, N, axis=0)).double() @ wv[:, 256:].T + bias

    def rgb(Vm):
        return torch.relu(trunk @ Vm.T + view) @ torch.from_numpy(p["color_layer.weight"]).double().T
    assert torch.equal(rgb(V), c["raw"].reshape(M, 4)[:, :3])
    r = int(np.flatnonzero(p["color_layer.weight"][0])[0])          # a view unit the colour head reads
    col = int(torch.nonzero(V[r])[0])
    V2 = V.clone()
    V2[r, (col + 1) % 256], V2[r, col] = V[r, col], V[r, (col + 1) % 256]
    assert not torch.equal(rgb(V2), rgb(V))
