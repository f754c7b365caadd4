"""The bottleneck folded into view layer 0 (Plan.build(fold_view=True)): the plan the bf16 forward kernels run.

extra_layer has no activation and only view layer 0 reads it, so W_v[:, :W] (W_e x + b_e) = (W_v[:, :W] W_e) x + W_v[:, :W] b_e.  The
folded plan's head is the density tile alone and view0 reads the trunk output with derived tensors (mlp_plan.fold_params)."""
import importlib.util
import os
import sys

import numpy as np
import pytest

from mipnerf_pl_amd.mlp_plan import Arch, Plan, emulate_wave, fold_params
from mipnerf_pl_amd.mlp_train_plan import TrainPlan, emulate_train
from oracle import mipnerf_oracle as orc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "mipnerf_pl_amd", "csrc")


def _gen_bf16():
    spec = importlib.util.spec_from_file_location("gen_mlp_bf16", os.path.join(CSRC, "gen_mlp_bf16.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.path.insert(0, CSRC)
    spec.loader.exec_module(mod)
    return mod


VARIANTS = _gen_bf16().VARIANTS
ARCH_KW = ("net_width", "net_width_condition", "net_depth", "skip_index", "xyz_dim", "net_depth_condition")


def _params(arch, seed):
    params = orc.make_params(seed=seed, density_gain=10.0, **{k: getattr(arch, k) for k in ARCH_KW})
    assert [n for n, _ in arch.param_shapes()] == list(params.keys())
    return params, np.concatenate([v.ravel() for v in params.values()])


def _inputs(arch, seed=0):
    rng = np.random.default_rng(seed)
    enc = rng.uniform(-1, 1, (32, arch.xyz_dim)).astype(np.float32)
    v27 = rng.uniform(-1, 1, (32, 27)).astype(np.float32)
    view = np.zeros((32, 32), np.float32)
    view[:, :27] = v27
    return enc, v27, view


def test_shipped_shape_drops_the_bottleneck_chunks():
    plain, folded = Plan.build(), Plan.build(fold_view=True)
    assert (len(plain.chunks), plain.n_real_chunks, plain.n_tiles) == (1216, 1216, 78)
    assert (len(folded.chunks), folded.n_real_chunks, folded.n_tiles) == (1088, 1088, 70)      # 34 ring groups, no zero padding
    head = [op for op in folded.ops if op.name == "head"][0]
    assert len(head.tiles) == 1 and head.tiles[0].nrows == 1 and head.nk == 16                # the density tile alone, unchanged
    view0 = [op for op in folded.ops if op.name == "view0"][0]
    n = len(plain.arch.param_shapes())
    assert view0.nk == 18 and {(t.wt, t.bt) for t in view0.tiles} == {(n, n + 1)}
    offs, nreal = folded.param_offsets()
    assert offs[:n] == plain.param_offsets()[0] and nreal == plain.param_offsets()[1] and offs[n] == nreal


def test_fold_is_off_by_default_and_a_no_op_without_view_directions():
    assert not Plan.build().fold_view
    for arch in VARIANTS:
        if arch.use_viewdirs:
            continue
        a, b = Plan.build(arch), Plan.build(arch, fold_view=True)
        assert not b.fold_view and a.chunks == b.chunks and np.array_equal(a.pack_table(), b.pack_table())
        assert np.array_equal(a.bias_table(), b.bias_table())


@pytest.mark.parametrize("vi", [i for i, a in enumerate(VARIANTS) if a.use_viewdirs and a.bf16_kernels])
def test_folded_emulation_matches_oracle(vi):
    """fp32 emulation of the folded plan against the oracle MLP, to fp32 round-off like the unfolded plan's test."""
    arch = VARIANTS[vi]
    params, flat = _params(arch, 11 + vi)
    enc, v27, view = _inputs(arch, vi)
    rgb, dens = emulate_wave(Plan.build(arch, fold_view=True), flat, enc, view)
    rr, dd = orc.mlp_forward(params, enc[:, None, :], v27, skip_index=arch.skip_index, net_depth=arch.net_depth,
                             net_depth_condition=arch.net_depth_condition)
    np.testing.assert_allclose(rgb, rr[:, 0], atol=5e-6)
    np.testing.assert_allclose(dens, dd[:, 0, 0], atol=2e-5)


@pytest.mark.parametrize("vi", [i for i, a in enumerate(VARIANTS) if a.use_viewdirs and a.bf16_kernels])
def test_folded_bf16_keeps_density_bits_and_rgb_error(vi):
    """With bf16 operand rounding the density path is untouched (same chunks, same order): bit-identical.  rgb loses the roundings of
    the bottleneck output and of two weight matrices and gains one of the folded matrix: its error must not grow by more than half."""
    arch = VARIANTS[vi]
    params, flat = _params(arch, 31 + vi)
    enc, v27, view = _inputs(arch, 100 + vi)
    r0, d0 = emulate_wave(Plan.build(arch), flat, enc, view, round_bf16=True)
    r1, d1 = emulate_wave(Plan.build(arch, fold_view=True), flat, enc, view, round_bf16=True)
    assert np.array_equal(d0, d1)
    rr, _ = orc.mlp_forward(params, enc[:, None, :], v27, skip_index=arch.skip_index, net_depth=arch.net_depth,
                            net_depth_condition=arch.net_depth_condition)
    e0, e1 = np.abs(r0 - rr[:, 0]).max(), np.abs(r1 - rr[:, 0]).max()
    assert e1 <= 1.5 * e0, (e0, e1)


def test_fold_params_is_the_algebra():
    arch = Arch()
    params, flat = _params(arch, 5)
    d = fold_params(arch, flat)
    W, Wc = arch.net_width, arch.net_width_condition
    V, b = d[:Wc * (W + 27)].reshape(Wc, W + 27), d[Wc * (W + 27):]
    Wv, We = params["view_layers.0.0.weight"].astype(np.float64), params["extra_layer.weight"].astype(np.float64)
    np.testing.assert_allclose(V[:, :W], Wv[:, :W] @ We, rtol=1e-6, atol=1e-7)
    assert np.array_equal(V[:, W:], params["view_layers.0.0.weight"][:, W:])
    np.testing.assert_allclose(b, params["view_layers.0.0.bias"] + Wv[:, :W] @ params["extra_layer.bias"], rtol=1e-6, atol=1e-7)


def test_folded_tables_match_the_library():
    """Debug tables 6 / 7 (the bf16 forward stream and bias table the context packs) equal the folded Python plan for every variant;
    tables 0 / 1 stay the plain plan's."""
    from mipnerf_pl_amd import _lib as L
    lib = L.lib()
    for v, arch in enumerate(VARIANTS):
        plain, folded = Plan.build(arch), Plan.build(arch, fold_view=arch.bf16_kernels)
        for which, want in ((0, plain.pack_table()), (1, plain.bias_table()), (6, folded.pack_table()), (7, folded.bias_table())):
            want = want.astype(np.int32).ravel()
            n = lib.mipnerf_debug_table_variant(v, which, None, 0)
            got = np.empty(n, np.int32)
            assert lib.mipnerf_debug_table_variant(v, which, got.ctypes.data, n) == n
            np.testing.assert_array_equal(got, want, err_msg=f"variant {v} table {which}")
    for which, want in ((6, Plan.build(fold_view=True).pack_table()), (7, Plan.build(fold_view=True).bias_table())):
        n = lib.mipnerf_debug_table(which, None, 0)
        got = np.empty(n, np.int32)
        assert lib.mipnerf_debug_table(which, got.ctypes.data, n) == n
        np.testing.assert_array_equal(got, want.astype(np.int32).ravel())


def test_training_plan_tables_do_not_depend_on_the_fold():
    """Only the forward-with-save runs the folded plan: the dgrad stream, weight-gradient tables and blob are the same either way."""
    for arch in (Arch(), Arch(net_width=128, net_width_condition=128), Arch(net_depth_condition=2)):
        a, b = TrainPlan.build(arch, fold_view=False), TrainPlan.build(arch, fold_view=True)
        assert b.fwd.fold_view and not a.fwd.fold_view
        assert a.blob() == b.blob() and a.fwd_out == b.fwd_out


def test_training_emulation_default_follows_the_device():
    """The evidence for TrainPlan.build()'s default (folded, like the device kernels).  With bf16 rounding and white-noise upstream
    gradients, folded and unfolded emulations differ by up to ~5e-2 relative L2 on the view / bottleneck gradients (ReLU mask flips of
    the view layer): more than the 1e-2 the device is held to against TrainPlan.build()'s emulation, so the emulation must run the plan
    the device runs.  Both stay equally far from the fp32 oracle, and raw density is the same bits."""
    arch = Arch()
    S = 70
    rng = np.random.default_rng(10)
    params, flat = _params(arch, 7)
    enc = (rng.normal(size=(S, 96)) * 0.5).astype(np.float32)
    view = np.zeros((S, 32), np.float32)
    view[:, :27] = rng.normal(size=(S, 27))
    d_raw = rng.normal(size=(S, 4)).astype(np.float32)
    assert TrainPlan.build().fwd.fold_view
    g0, _, raw0 = emulate_train(TrainPlan.build(arch, fold_view=False), flat, enc, view, d_raw, round_bf16=True)
    g1, _, raw1 = emulate_train(TrainPlan.build(arch, fold_view=True), flat, enc, view, d_raw, round_bf16=True)
    assert np.array_equal(raw0[:, 3], raw1[:, 3])
    og = orc.mlp_backward(params, enc[:, None, :], view[:, :27], d_raw[:, None, :3], d_raw[:, None, 3:])
    off, gap, e0, e1 = 0, 0.0, 0.0, 0.0
    for k, v in og.items():
        n = v.size
        a, b, o = g0[off:off + n].astype(np.float64), g1[off:off + n].astype(np.float64), v.ravel().astype(np.float64)
        off += n
        gap = max(gap, np.linalg.norm(a - b) / np.linalg.norm(a))
        e0, e1 = max(e0, np.linalg.norm(a - o) / np.linalg.norm(o)), max(e1, np.linalg.norm(b - o) / np.linalg.norm(o))
    assert 1e-2 < gap < 0.1, gap                 # measured 4.7e-2 (extra_layer.weight)
    assert e1 <= 0.2 and e1 <= 1.5 * e0, (e0, e1)     # the device test's bound against fp32; measured 0.134 / 0.134
