"""CPU (no GPU): the C-ABI shared library loads, exports every symbol include/mipnerf_hip.h
declares, and its host-side plan expansion equals mipnerf_pl_amd/mlp_plan.py.  No compute calls."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from mipnerf_pl_amd import _lib as L
from mipnerf_pl_amd.mlp_plan import Plan, emulate_wave
from oracle import mipnerf_oracle as orc

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(L.LIB_PATH):
        from mipnerf_pl_amd import build
        build.build(verbose=False)
    return L.lib()


def header_functions():
    src = open(os.path.join(REPO, "include", "mipnerf_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(mipnerf_[a-z0-9_]+)\s*\(", src)))


def test_every_declared_symbol_is_exported(lib):
    names = header_functions()
    assert len(names) >= 20
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/mipnerf_hip.h but not exported"
    # and the Python binding covers exactly the header
    assert sorted(L.SIGNATURES) == names


def _dynamic_symbols(path):
    import subprocess
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return sorted(line.split()[-1] for line in out.splitlines() if line.strip())


def test_dynamic_symbol_table_is_exactly_the_c_abi(lib):
    """the libraries export the entry points their headers declare and NOTHING else -- no mip::launch_* C++ launchers,
    kernel handles or table blobs (a linker version script in build.py keeps `mipnerf_*` only)."""
    assert _dynamic_symbols(L.LIB_PATH) == header_functions()
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "mipnerf_diag.h")).read(), flags=re.S)
    assert _dynamic_symbols(L.DIAG_LIB_PATH) == sorted(set(re.findall(r"\b(mipnerf_[a-z0-9_]+)\s*\(", src)))


def test_abi_version_and_compiled_arch(lib):
    assert lib.mipnerf_abi_version() == 6
    cfg = L.Config()
    assert lib.mipnerf_compiled_arch(C.byref(cfg)) == 0
    assert (cfg.net_depth, cfg.net_width, cfg.net_depth_condition, cfg.net_width_condition, cfg.skip_index) == (8, 256, 1, 128, 4)
    assert (cfg.max_deg_point, cfg.deg_view) == (16, 4)


def test_error_reporting_without_gpu(lib):
    # argument validation happens before any HIP call
    assert lib.mipnerf_sample_along_rays(0, 64, None, None, None, 0, None, None) == L.E_INVALID
    assert b"sample_along_rays" in lib.mipnerf_last_error()
    with pytest.raises(ValueError):
        L.check(L.E_INVALID, "x")
    with pytest.raises(NotImplementedError):
        L.check(L.E_UNSUPPORTED, "x")


@pytest.mark.parametrize("which,ref", [(0, "pack_table"), (1, "bias_table"), (2, "pack_table_f32")])
def test_host_plan_tables_match_python_plan(lib, which, ref):
    plan = Plan.build()
    want = getattr(plan, ref)().astype(np.int32).ravel()
    n = lib.mipnerf_debug_table(which, None, 0)
    assert n == want.size
    got = np.empty(n, np.int32)
    assert lib.mipnerf_debug_table(which, got.ctypes.data, n) == n
    np.testing.assert_array_equal(got, want)


def test_f32_layer_descriptors(lib):
    plan = Plan.build()
    n = lib.mipnerf_debug_f32net(None, 0)
    buf = np.empty((n, 12), np.int32)
    lib.mipnerf_debug_f32net(buf.ctypes.data, buf.size)
    layers = plan.f32_layers()
    assert n == len(layers)
    chunk0 = 0
    W = plan.arch.net_width
    for i, (row, Ly) in enumerate(zip(buf, layers)):
        assert tuple(row[:5]) == (Ly["x_in0"], Ly["kb0"], Ly["x_in1"], Ly["kb1"], Ly["x_out"])
        assert row[5] == len(Ly["tiles"]) and row[6] == Ly["first_tile"] and row[7] == int(Ly["relu"]) and row[8] == Ly["kind"]
        assert row[9] == chunk0 and row[10] == int(Ly["kind"] == 1)
        chunk0 += len(Ly["tiles"]) * Ly["kb"]
        assert row[11] == 2 * W + 96 + 4
        # double buffering: a layer never writes the buffer it (or its second segment) reads
        assert row[4] != row[0] and (row[3] == 0 or row[2] == 2 * W)
        if i > 0 and Ly["kb0"] * 16 == W:
            assert row[0] == buf[i - 1][4]                     # reads what the previous layer wrote
    assert [r[8] for r in buf] == [0] * 8 + [1, 0, 2]
    assert (buf[5][0], buf[5][1], buf[5][2], buf[5][3]) == (W, 16, 2 * W, 6)     # skip concat: [x | encoding]


def test_register_dataflow_emulation_matches_oracle():
    """The k-permutation / D-layout repacking the bf16 kernel relies on, emulated in numpy in fp32
    (no bf16 rounding), reproduces the oracle MLP to fp32 round-off."""
    plan = Plan.build()
    params = orc.make_params(seed=11, density_gain=10.0)
    names = [n for n, _ in plan.arch.param_shapes()]
    assert names == list(params.keys())
    flat = np.concatenate([params[n].ravel() for n in names])
    rng = np.random.default_rng(0)
    enc = rng.uniform(-1, 1, (32, 96)).astype(np.float32)
    v27 = rng.uniform(-1, 1, (32, 27)).astype(np.float32)
    view = np.zeros((32, 32), np.float32)
    view[:, :27] = v27
    rgb, dens = emulate_wave(plan, flat, enc, view)
    rr, dd = orc.mlp_forward(params, enc[:, None, :], v27)
    np.testing.assert_allclose(rgb, rr[:, 0], atol=5e-6)
    np.testing.assert_allclose(dens, dd[:, 0, 0], atol=2e-5)


def _variants():
    import importlib.util
    import os
    spec = importlib.util.spec_from_file_location(
        "gen_mlp_bf16", os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "mipnerf_pl_amd", "csrc", "gen_mlp_bf16.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.VARIANTS


def test_architecture_variants_exported(lib):
    """Every MLP shape of gen_mlp_bf16.VARIANTS is carried by the library (mipnerf_variant_arch) and the C++ table
    expansion of each equals mlp_plan.py (bf16 stream incl. its zero padding, bias table, fp32 stream)."""
    variants = _variants()
    assert lib.mipnerf_num_variants() == len(variants) >= 6
    for v, arch in enumerate(variants):
        cfg, has_train = L.Config(), C.c_int(-1)
        assert lib.mipnerf_variant_arch(v, C.byref(cfg), C.byref(has_train)) == 0
        assert (cfg.net_depth, cfg.net_width, cfg.net_depth_condition, cfg.net_width_condition, cfg.skip_index,
                bool(cfg.use_viewdirs)) == (arch.net_depth, arch.net_width, arch.net_depth_condition, arch.net_width_condition,
                                            arch.skip_index, arch.use_viewdirs)
        # bf16 training kernels for every variant that has bf16 kernels and widths <= 256 (mlp_train_plan.py; round 5: two view layers train in
        # bf16 too; the 512-wide trunk has a bf16 inference kernel and trains in fp32)
        # ... or the two-kernel form's training kernels (round 5: the wide-encoding variant of the unbounded-scene model)
        from mipnerf_pl_amd import mlp_pre_plan
        assert has_train.value == int((arch.bf16_kernels and arch.net_width <= 256)
                                       or mlp_pre_plan.supported(arch))
        assert bool(cfg.unbounded) == (arch.feat_per_deg == 42) and (cfg.max_deg_point - cfg.min_deg_point) * arch.feat_per_deg == arch.xyz_dim
        plan = Plan.build(arch)
        for which, ref in ((0, "pack_table"), (1, "bias_table"), (2, "pack_table_f32")):
            want = getattr(plan, ref)().astype(np.int32).ravel()
            n = lib.mipnerf_debug_table_variant(v, which, None, 0)
            got = np.empty(n, np.int32)
            assert lib.mipnerf_debug_table_variant(v, which, got.ctypes.data, n) == n
            if which == 2:      # the C++ table is sized like the bf16 stream; the fp32 stream fills its real chunks
                assert n >= want.size and (got[want.size:] == -1).all()
                got = got[:want.size]
            np.testing.assert_array_equal(got, want)


def _read_plan_blob(b, plain, fwd):
    """capi.hip's plan_tables restated: the sections of mlp_plan.blob() as arrays, or None where the library refuses the blob.  The
    counts the library takes from the generated PlanDesc come from the two plans here."""
    w = np.frombuffer(b, np.int32)
    h = w[:16]
    fold = int(fwd.fold_view)
    if (h[0] != 0x504C4E31 or h[1] != len(plain.chunks) or h[2] != plain.n_tiles or h[3] != len(fwd.chunks) or h[4] != fwd.n_tiles or
            not 0 <= h[5] <= len(plain.chunks) or h[6] != len(plain.ops) or h[6] > 16 or h[7] != plain.param_offsets()[1] or h[8] != fold):
        return None
    if not fold and (h[3] != h[1] or h[4] != h[2]):
        return None
    sizes = [h[1] * 20, h[2] * 32] + ([h[3] * 20, h[4] * 32] if fold else []) + [h[5] * 20, h[6] * 12]
    if 16 + sum(sizes) != h[9]:
        return None
    parts = np.split(w[16:h[9]], np.cumsum(sizes)[:-1])
    names = ["pack", "bias"] + (["fwd_pack", "fwd_bias"] if fold else []) + ["pack_f32", "layers"]
    T = dict(zip(names, parts))
    if not fold:
        T["fwd_pack"], T["fwd_bias"] = T["pack"], T["bias"]
    return T


def _expand_chunk_records(desc, offs):
    """idx[hi * 32 + m][j] = offs[tensor] + (row0 + m) * ld + col[hi * 8 + j] for m < nrows, -1 where col < 0 or m >= nrows"""
    d = desc.reshape(-1, 20)
    tensor, row0, ld, nrows = (d[:, i, None, None, None] for i in range(4))
    col = d[:, 4:].reshape(-1, 2, 1, 8)
    m = np.arange(32).reshape(1, 1, 32, 1)
    idx = np.asarray(offs)[tensor] + (row0 + m) * ld + col
    return np.where((col >= 0) & (m < nrows), idx, -1).reshape(-1, 64, 8)


def _blob_archs():
    from mipnerf_pl_amd.mlp_plan import Arch
    return _variants() + [Arch(net_width=192, net_width_condition=64), Arch(net_width=64, net_width_condition=64)]


@pytest.mark.parametrize("ai", range(9))
def test_plan_blob_expands_to_the_python_tables(ai):
    """The chunk records, bias tables and counts of mlp_plan.blob() (what the library links in and expands) give back pack_table(),
    pack_table_f32() and both bias_table()s: every shape of VARIANTS and the two narrow ad-hoc shapes, with the forward plan plain and
    folded (1-row density tiles, the 3-row colour tile, the 27-column view segment, all-padding chunks, the skip concat, no view
    directions).  A blob with any one header count altered is refused by the reader's consistency checks."""
    from mipnerf_pl_amd import mlp_plan
    arch = _blob_archs()[ai]
    plain = Plan.build(arch)
    want = dict(pack=plain.pack_table(), pack_f32=plain.pack_table_f32(), bias=plain.bias_table().ravel())
    assert (want["pack"][plain.n_real_chunks:] == -1).all()
    for fold in (False, True):
        fwd = Plan.build(arch, fold_view=fold)
        blob = mlp_plan.blob(plain, fwd)
        T = _read_plan_blob(blob, plain, fwd)
        assert T is not None
        offs = fwd.param_offsets()[0]                 # the real tensors, then the derived ones of a folded plan
        np.testing.assert_array_equal(_expand_chunk_records(T["pack"], offs), want["pack"])
        np.testing.assert_array_equal(_expand_chunk_records(T["pack_f32"], offs), want["pack_f32"])
        np.testing.assert_array_equal(T["bias"], want["bias"])
        np.testing.assert_array_equal(_expand_chunk_records(T["fwd_pack"], offs), fwd.pack_table())
        np.testing.assert_array_equal(T["fwd_bias"], fwd.bias_table().ravel())
        assert fwd.fold_view == (fold and arch.use_viewdirs) and (fwd.fold_view or T["fwd_pack"] is T["pack"])
        for i in range(1, 10):
            bad = np.frombuffer(blob, np.int32).copy()
            bad[i] += 1
            assert _read_plan_blob(bad.tobytes(), plain, fwd) is None, f"header word {i} altered and the blob still accepted"


def test_variant_dataflow_emulation_matches_oracle():
    """Register dataflow of the generated bf16 kernels for the non-default shapes (half-width trunk; no view directions:
    density-only head, colour head on the trunk output), emulated in fp32, against the oracle MLP."""
    for arch in _variants()[1:]:
        plan = Plan.build(arch)
        params = orc.make_params(seed=21, density_gain=10.0, net_width=arch.net_width, net_width_condition=arch.net_width_condition,
                                 net_depth=arch.net_depth, skip_index=arch.skip_index, xyz_dim=arch.xyz_dim,
                                 net_depth_condition=arch.net_depth_condition)
        names = [n for n, _ in arch.param_shapes()]
        assert names == list(params.keys())
        flat = np.concatenate([params[n].ravel() for n in names])
        rng = np.random.default_rng(1)
        enc = rng.uniform(-1, 1, (32, arch.xyz_dim)).astype(np.float32)
        v27 = rng.uniform(-1, 1, (32, 27)).astype(np.float32)
        view = np.zeros((32, 32), np.float32)
        view[:, :27] = v27
        rgb, dens = emulate_wave(plan, flat, enc, view)
        rr, dd = orc.mlp_forward(params, enc[:, None, :], v27 if arch.use_viewdirs else None, skip_index=arch.skip_index,
                                 net_depth=arch.net_depth, net_depth_condition=arch.net_depth_condition)
        np.testing.assert_allclose(rgb, rr[:, 0], atol=5e-6)
        np.testing.assert_allclose(dens, dd[:, 0, 0], atol=2e-5)


def test_diagnostics_live_in_their_own_library(lib):
    """VERDICT r03 hygiene: the drop-in library is the hot path only -- the MFMA ceilings and the hand-off probe are exported by
    libmipnerf_diag.so (include/mipnerf_diag.h), header == exports == ctypes table, and NOT by libmipnerf_hip.so."""
    src = open(os.path.join(REPO, "include", "mipnerf_diag.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    names = sorted(set(re.findall(r"\b(mipnerf_[a-z0-9_]+)\s*\(", src)))
    assert names == sorted(L.DIAG_SIGNATURES) and len(names) == 3
    d = L.diag_lib()
    assert d is not None
    for n in names:
        assert hasattr(d, n)
        if n != "mipnerf_diag_last_error":
            assert not hasattr(lib, n), f"{n} still exported by the drop-in library"
    import subprocess
    syms = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True).stdout
    assert "ceiling" not in syms and "handoff" not in syms


def test_diagnostic_entry_points_validate_their_arguments(lib):
    """mipnerf_mfma_ceiling / mipnerf_handoff_probe reject bad arguments before touching the device; a later SUCCESSFUL validation
    does not clear the message."""
    out3, out6 = (C.c_double * 3)(), (C.c_double * 6)()
    lib = L.diag_lib()
    assert lib.mipnerf_mfma_ceiling(0, 3, 1, 1.0, out3, None) == L.E_INVALID          # waves per SIMD must be 1 or 2
    assert lib.mipnerf_mfma_ceiling(4, 2, 1, 1.0, out3, None) == L.E_INVALID          # feeding mode 0 ... 3
    assert lib.mipnerf_mfma_ceiling(0, 2, 1, 100.0, out3, None) == L.E_INVALID        # bounded run time
    assert lib.mipnerf_mfma_ceiling(0, 2, 1, 1.0, None, None) == L.E_INVALID
    assert lib.mipnerf_handoff_probe(1, 0, 0, 4, 131072, 0, 1, out6, None) == L.E_INVALID       # no tiles
    assert lib.mipnerf_handoff_probe(1, 0, 16, 4, 1000, 0, 1, out6, None) == L.E_INVALID        # tile too small
    assert lib.mipnerf_handoff_probe(1, 0, 16, 64, 1 << 22, 0, 1, out6, None) == L.E_INVALID    # ring x tile x 128 pairs > 4 GiB
    assert b"handoff_probe" in lib.mipnerf_diag_last_error()
    assert lib.mipnerf_handoff_probe(1, 5, 16, 4, 131072, 0, 1, out6, None) == L.E_INVALID      # no such protocol
    assert lib.mipnerf_handoff_probe(0, 4, 16, 4, 131072, 0, 1, out6, None) == L.E_INVALID      # fence-free protocols are same-XCD only
    assert lib.mipnerf_handoff_probe(1, 3, 16, 4, 262144, 0, 1, out6, None) == L.E_INVALID      # per-wave protocols: 64 / 128 KiB tiles


def _torch_mlp(params, arch, enc, venc):
    """plain-torch restatement of MLP.forward (mip_nerf.py:75-111) on a state dict -- only to compare a padded with an unpadded net"""
    import torch
    x = enc
    h = x
    for i in range(arch["net_depth"]):
        h = torch.relu(torch.nn.functional.linear(h, params[f"layers.{i}.0.weight"], params[f"layers.{i}.0.bias"]))
        if i % arch["skip_index"] == 0 and i > 0:
            h = torch.cat([h, x], -1)
    dens = torch.nn.functional.linear(h, params["density_layer.weight"], params["density_layer.bias"])
    b = torch.nn.functional.linear(h, params["extra_layer.weight"], params["extra_layer.bias"])
    v = torch.cat([b, venc], -1)
    for i in range(arch["net_depth_condition"]):
        v = torch.relu(torch.nn.functional.linear(v, params[f"view_layers.{i}.0.weight"], params[f"view_layers.{i}.0.bias"]))
    rgb = torch.nn.functional.linear(v, params["color_layer.weight"], params["color_layer.bias"])
    return torch.cat([rgb, dens], -1)


@pytest.mark.parametrize("w,wc,depth,skip,dc", [(200, 72, 8, 4, 1), (100, 40, 8, 4, 1), (40, 24, 6, 3, 1), (130, 90, 8, 4, 2)])
def test_width_padding_keeps_the_function_and_its_gradient(lib, w, wc, depth, skip, dc):
    """model.WidthPadding (host logic behind MLP widths that are not generated shapes): the variant search returns the smallest
    containing generated shape; scattering the true parameters into zeros of that shape gives a network with the SAME outputs,
    and the gather of its gradient IS the gradient of the true parameters (every padded entry's gradient is exactly 0)."""
    import torch
    from mipnerf_pl_amd import model as M
    arch = dict(net_depth=depth, net_width=w, net_depth_condition=dc, net_width_condition=wc, skip_index=skip, num_rgb_channels=3,
                num_density_channels=1, xyz_dim=96, view_dim=27)
    found = M.containing_variant(arch, True, False, False)
    assert found is not None and not found[1]
    padded_arch = found[0]
    assert padded_arch["net_width"] >= w and padded_arch["net_width"] % 32 == 0 and padded_arch["net_width_condition"] >= wc
    assert M.containing_variant(dict(arch, net_width=padded_arch["net_width"], net_width_condition=padded_arch["net_width_condition"]),
                                True, False, False)[1]                       # the containing shape itself is an exact match
    pad = M.WidthPadding(arch, padded_arch)
    layout = M.param_layout(arch)
    gen = torch.Generator().manual_seed(w)
    true = {n: (torch.rand(shp, generator=gen, dtype=torch.float64) - 0.5).requires_grad_() for n, shp, _ in layout}
    assert pad.true_numel == sum(p.numel() for p in true.values()) and len(set(pad.index.tolist())) == pad.true_numel
    flat = torch.zeros(pad.padded_numel, dtype=torch.float64)
    pad.scatter(list(true.values()), flat)
    flat.requires_grad_()
    padded = dict(zip([n for n, _, _ in layout], pad.padded_views(flat)))
    assert [tuple(v.shape) for v in padded.values()] == [shp for _, shp, _ in M.param_layout(padded_arch)]
    enc = torch.randn(50, 96, generator=gen, dtype=torch.float64)
    venc = torch.randn(50, 27, generator=gen, dtype=torch.float64)
    y0 = _torch_mlp(true, arch, enc, venc)
    y1 = _torch_mlp(padded, padded_arch, enc, venc)
    assert float((y0 - y1).abs().max()) <= 1e-13 * float(y0.abs().max())      # summation order of the BLAS only
    wgt = torch.randn(50, 4, generator=gen, dtype=torch.float64)
    (y0 * wgt).sum().backward()
    (y1 * wgt).sum().backward()
    g_true = torch.cat([p.grad.reshape(-1) for p in true.values()])
    assert float((pad.gather(flat.grad) - g_true).abs().max()) <= 1e-13 * float(g_true.abs().max())
    mask = torch.ones(pad.padded_numel, dtype=torch.bool)
    mask[pad.index] = False
    assert float(flat.grad[mask].abs().max()) == 0.0                        # padded entries never move under any optimiser
    # nothing wider than the widest generated shape
    assert M.containing_variant(dict(arch, net_width=600), True, False, False) is None


def test_launch_attribute_caches_are_per_device(lib):
    """hipFuncSetAttribute(MaxDynamicSharedMemorySize) is a per-DEVICE property: a launcher that remembers "done" once per process would
    launch its > 64-KiB-LDS kernel without the attribute on the second GPU a process touches (MLP.native(device) keeps one context per
    device).  Every cache in the hand-written and the generated sources must be indexed by the current device."""
    csrc = os.path.join(REPO, "mipnerf_pl_amd", "csrc")
    checked = 0
    for f in sorted(os.listdir(csrc)):
        if not f.endswith((".hip", ".hpp", ".py")):
            continue
        src = open(os.path.join(csrc, f)).read()
        if "hipFuncSetAttribute" not in src:
            continue
        checked += 1
        assert not re.search(r"static\s+bool\s+\w*attr\w*", src), f"{f}: per-process attribute cache"
        for m in re.finditer(r"static\s+int\s+(\w*attr\w*)\s*\[", src):
            assert re.search(r"hipGetDevice\s*\(", src), f"{f}: {m.group(1)} is not indexed by the device"
    assert checked >= 10


# Every build-time timing knob the generators, plan modules and build.py once read (rounds 1-6), each at a value other than its old default.
RETIRED_KNOBS = {
    "MLP_WAVES": "4", "MLP_PREFETCH": "6", "MLP_ABLATE_BARRIER": "1", "MLP_ABLATE_WAIT": "1", "MLP_ABLATE_LDA": "1", "MLP_SETPRIO": "0",
    "MLP_IPE_SHADOW": "1", "MLP_IPE_SHADOW_STRIDE": "2", "MLP_PRE_NT_LOADS": "0", "MLP_TRUNK_ABLATE_PRELOADS": "1", "MLP_FUSED_RING": "6",
    "MLP_FUSED_AHEAD": "5", "MLP_FUSED_OPAQUE": "0", "MLP_WIDE_PREFETCH": "6", "MLP_WIDE_CPW": "8", "MLP_WIDE_AHEAD": "3",
    "MLP_WIDE_SPARE_SLOT": "0", "MLP_TRAIN_PREFETCH": "6", "MLP_TRAIN_ABLATE_TMFMA": "1", "MLP_TRAIN_SKIP_STORES": "2,4",
    "MLP_TRAIN_SPREAD_STORES": "0", "MLP_TRAIN_COUNTED_VMCNT": "1", "MLP_F32R_PIECE_WINDOW": "0.25", "MLP_F32R_GEN_ABLATE": "15",
    "MLP_F32R_ABLATE": "1", "MLP_F32R_NAT_NT": "0", "MLP_PRE_DEPTH": "14", "MLP_PRE_DEPTH_SPLIT": "7", "MLP_PRE_NT_STORES": "0",
    "MLP_PRE_NT_PASS1": "0", "MLP_PRE_ABLATE_STORES": "1", "MLP_PRE_FORM": "once", "MLP_PRE_ONCE_DEPTH": "7", "MLP_PRE_ONCE_SLOTS": "6",
    "MLP_PRE_SPLIT": "1", "MLP_CHAIN": "1", "MLP_F32R_GROUP_CHUNKS": "24", "MLP_F32R_RING_SLOTS": "3", "MLP_SIN_TWOFLOAT": "1",
    "MLP_WAVE_DPP": "0", "MLP_WGRAD_NT": "0", "MLP_WGRAD_STAGES": "3", "MLP_WGRAD_TR": "1", "MLP_WGRAD_RECOMPUTE_PROBE": "1",
    "MLP_WGRAD_RECOMPUTE_SCHED": "1", "MLP_IPE360_ROW_PAD": "8",
}


def test_the_environment_cannot_change_the_product(tmp_path, monkeypatch):
    """The product library says one thing whatever shell it is built from: the four generators write byte-identical sources, tables and headers
    with every retired build knob set, build.py compiles with the same flags, and nothing in the package reads an MLP_* variable."""
    import importlib
    import subprocess
    import sys
    csrc = os.path.join(REPO, "mipnerf_pl_amd", "csrc")
    clean = {k: v for k, v in os.environ.items() if not k.startswith("MLP_")}
    outs = []
    for env in (clean, {**clean, **RETIRED_KNOBS}):
        out = tmp_path / f"gen{len(outs)}"
        out.mkdir()
        for gen in ("gen_mlp_bf16.py", "gen_mlp_train.py", "gen_mlp_f32r.py", "gen_pre_gemm.py"):
            subprocess.run([sys.executable, os.path.join(csrc, gen), str(out)], env=env, check=True, stdout=subprocess.DEVNULL)
        outs.append({f: (out / f).read_bytes() for f in sorted(os.listdir(out))})
    assert len(outs[0]) >= 30 and sorted(outs[0]) == sorted(outs[1])
    for f in outs[0]:
        assert outs[0][f] == outs[1][f], f"{f}: the environment changed a generated file"

    from mipnerf_pl_amd import build as b
    flags = (list(b.COMMON), list(b.UNITS))
    for k, v in RETIRED_KNOBS.items():
        monkeypatch.setenv(k, v)
    try:
        assert (list(importlib.reload(b).COMMON), list(b.UNITS)) == flags
    finally:
        monkeypatch.undo()
        importlib.reload(b)

    readers = []
    for root, _, files in os.walk(os.path.join(REPO, "mipnerf_pl_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".hpp", ".h", ".c", ".cpp")):
                src = open(os.path.join(root, f), errors="replace").read()
                readers += [f"{f}: {m.group(0)}" for m in re.finditer(r"(?:environ|getenv)[^\n]*\bMLP_\w*", src)]
    assert not readers, readers


def test_one_wave_per_simd_kernel_ring_is_consistent():
    """The 512-wide trunk's bf16 kernel (gen_mlp_bf16.waves_of: 4-wave workgroups, one wave per SIMD) keeps kAhead ring groups in flight with
    counted vmcnt waits in kSlots = kAhead + 2 slots (round 6: the spare slot means a boundary refills the slot of group g - 2, whose reads
    returned long ago, and need not drain the wave's in-flight A-fragment reads).  From the generated source: every chunk is read from the slot
    its group was issued into, every group boundary is there exactly once, group 0 waits for everything (the tile's encoding DMAs are younger than
    the ring's), every other boundary leaves exactly the 4 (kAhead - 1) DMAs of the groups behind it in flight, the group count keeps the ring
    phase tile-invariant, and the refill never depends on has_next."""
    src = open(os.path.join(REPO, "mipnerf_pl_amd", "csrc", "mlp_bf16_gen_v6.hip")).read()
    ahead = int(re.search(r"constexpr int kAhead = (\d+);", src).group(1))
    slots = int(re.search(r"constexpr int kSlots = (\d+);", src).group(1))
    ngroups = int(re.search(r"constexpr int kNumGroups = (\d+);", src).group(1))
    group_bytes = int(re.search(r"constexpr int kGroupBytes = (\d+);", src).group(1))
    ring_bytes = int(re.search(r"constexpr int kRingBytes = (\d+);", src).group(1))
    assert slots == ahead + 2 and ring_bytes == slots * group_bytes and group_bytes == 16 * 1024 and ngroups % slots == 0
    assert "__launch_bounds__(256, 1)" in src and "MIP_OPAQUE_STREAM_BASE" in src
    body = src[src.index("for (int tile = blockIdx.x;"):]
    body = body[:body.index("if (hi == 0 && s < M)")]
    offs = [int(x) for x in re.findall(r"A\d+ = LDA\((\d+)\);", body)]
    assert len(offs) == ngroups * 16
    for c, off in enumerate(offs):                      # chunk c of the stream: group c // 16 lives in slot (c // 16) % slots
        assert off == ((c // 16) % slots) * group_bytes + (c % 16) * 1024, (c, off)
    begins = [(kind, int(g), int(w)) for kind, g, w in re.findall(r"GROUP_BEGIN_DEEP(_NODRAIN)?\((\d+), (\d+)\);", body)]
    assert [g for _, g, _ in begins] == list(range(ngroups))
    assert begins[0][0] == "" and begins[0][2] == 0 and all(k == "_NODRAIN" and w == 4 * (ahead - 1) for k, _, w in begins[1:])
    # the prologue issues groups 0 .. kAhead - 1 into slots 0 .. kAhead - 1; the macros refill slot (g + kAhead) % kSlots with group g + kAhead
    pro = src[:src.index("for (int tile = blockIdx.x;")]
    assert [tuple(map(int, m)) for m in re.findall(r"issue_group<DMA>\(stream, smem, (\d+), (\d+), wave, lane16\);", pro)][-ahead:] == [(g, g) for g in range(ahead)]
    for name in ("GROUP_BEGIN_DEEP(g, WAITCNT)", "GROUP_BEGIN_DEEP_NODRAIN(g, WAITCNT)"):
        macro = src[src.index("#define " + name):]
        macro = macro[:macro.index("} while (0)")]
        assert "has_next" not in macro and "(g) + kAhead - kNumGroups" in macro and "((g) + kAhead) % kSlots" in macro
    nodrain = src[src.index("#define GROUP_BEGIN_DEEP_NODRAIN"):]
    assert "lgkmcnt" not in nodrain[:nodrain.index("} while (0)")]
    tail = src[src.index("if (hi == 0 && s < M)"):]
    assert 's_waitcnt vmcnt(0)' in tail[:tail.index("\n}\n")]


def test_one_wave_per_simd_kernel_ring_replayed():
    """ADVICE r05 (high) was a counted wait that leaned on DMAs which are not in flight on a workgroup's last tile.  An independent replay of the
    512-wide kernel's ring (the rule of the hardware: a wave's vector-memory operations retire in issue order, `vmcnt(K)` leaves K outstanding),
    two tiles back to back with the refill running around the stream: at every group boundary the wave's four DMAs of that group have retired
    when the wait returns, every A-fragment read comes from the slot its group was DMA'd into LAST, and no refill overwrites a slot before all 16
    chunks of the group it held have been read."""
    src = open(os.path.join(REPO, "mipnerf_pl_amd", "csrc", "mlp_bf16_gen_v6.hip")).read()
    ahead = int(re.search(r"constexpr int kAhead = (\d+);", src).group(1))
    slots = int(re.search(r"constexpr int kSlots = (\d+);", src).group(1))
    ngroups = int(re.search(r"constexpr int kNumGroups = (\d+);", src).group(1))
    pro = src[:src.index("for (int tile = blockIdx.x;")]
    body = src[src.index("for (int tile = blockIdx.x;"):]
    body = body[:body.index("if (hi == 0 && s < M)")]
    outstanding, holds, reads_done = [], {}, {}

    def issue(group_id, slot):
        prev = holds.get(slot)
        assert prev is None or reads_done.get(prev, 0) == 16, ("refill over unread chunks", group_id, prev, reads_done.get(prev, 0))
        holds[slot] = group_id
        outstanding.extend([group_id] * 4)
    for g, sl in re.findall(r"issue_group<DMA>\(stream, smem, (\d+), (\d+), wave, lane16\);", pro)[-ahead:]:
        issue((0, int(g)), int(sl))
    tok = re.compile(r"GROUP_BEGIN_DEEP(?:_NODRAIN)?\((\d+), (\d+)\);|A\d+ = LDA\((\d+)\);")
    for tile in range(2):
        chunk = 0
        for m in tok.finditer(body):
            if m.group(3) is None:
                g, k = int(m.group(1)), int(m.group(2))
                while len(outstanding) > k:
                    outstanding.pop(0)
                assert (tile, g) not in outstanding, ("group not landed at its boundary", tile, g, k)
                nxt = g + ahead
                issue((tile + nxt // ngroups, nxt % ngroups), nxt % slots)          # around the stream, unconditionally
            else:
                slot = int(m.group(3)) // (16 * 1024)
                gid = (tile, chunk // 16)
                assert holds.get(slot) == gid and gid not in outstanding, ("A fragment read from a slot that does not hold its group", gid, holds.get(slot))
                reads_done[gid] = reads_done.get(gid, 0) + 1
                chunk += 1
        assert chunk == ngroups * 16


def _call_extents(src, name):
    """(start, end) of every call `name(...)` in src, end at its matching parenthesis"""
    out = []
    for m in re.finditer(r"\b" + name + r"\(", src):
        depth, i = 1, m.end()
        while depth:
            depth += {"(": 1, ")": -1}.get(src[i], 0)
            i += 1
        out.append((m.start(), i))
    return out


def test_sample_count_limit_is_one_number_everywhere():
    """num_samples <= 1024 = 64 lanes x 16 samples: the header, the ctypes layer and the LDS row constant say the same, and every per-ray
    kernel (a template on K, the samples a lane holds) is launched through the one samples-per-lane dispatcher of lane_buckets.hpp."""
    csrc = os.path.join(REPO, "mipnerf_pl_amd", "csrc")
    hdr = open(os.path.join(REPO, "include", "mipnerf_hip.h")).read()
    rules = open(os.path.join(csrc, "lane_buckets.hpp")).read()
    per_lane = int(re.search(r"constexpr int kMaxSamplesPerLane = (\d+);", rules).group(1))
    assert int(re.search(r"#define MIPNERF_MAX_SAMPLES (\d+)", hdr).group(1)) == L.MAX_SAMPLES == 1024 == 64 * per_lane
    sources = {f: open(os.path.join(csrc, f)).read() for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".hpp"))}
    assert "constexpr int kPdfMaxBins = 64 * kMaxSamplesPerLane;" in rules
    assert sum(len(re.findall(r"\bkPdfMaxBins\s*=[^=]", s)) for s in sources.values()) == 1          # defined there and nowhere else
    assert not any(re.search(r"\bkMaxBins\b", s) for s in sources.values())
    assert re.search(r"static_assert\(MIPNERF_MAX_SAMPLES == mip::kPdfMaxBins\b", sources["capi.hip"])
    launched = set()
    for f in ("kernels_ray.hip", "kernels_train.hip", "kernels_resample_grad.hip", "kernels_occupancy.hip"):
        src = sources[f]
        assert "switch (K)" not in src and "case 16" not in src and not re.search(r"#\s*define\s+MIP_", src), f
        per_ray = set(re.findall(r"template <int K[^>]*>\s*__global__[^;{]*?\b(k_\w+)\(", src))      # kernel templates whose first argument is K
        inside = _call_extents(src, "for_lane_bucket")
        for m in re.finditer(r"hipLaunchKernelGGL\(\(?\s*(k_\w+)", src):
            if m.group(1) in per_ray:
                assert any(a < m.start() < b for a, b in inside), (f, m.group(1))
                assert re.match(r"<decltype\(k\)::value[,>]", src[m.end():]), (f, m.group(1))        # K is the dispatcher's constant
                launched.add(m.group(1))
        assert launched >= per_ray, (f, per_ray - launched)                                         # no per-ray kernel is left unlaunched
    assert len(launched) == 11, sorted(launched)
    # the sampler's draw step (the forward and its backward must draw the same u): one statement
    jitter = r"u_jitter = [^\n]*1\.1920928955078125e-07f"
    assert len(re.findall(jitter, rules)) == 1 == sum(len(re.findall(jitter, s)) for s in sources.values())


def _type_list(params):
    """The types of a C++ parameter list: names and default arguments dropped, whitespace normalised."""
    out = []
    for p in params.split(","):
        p = " ".join(p.split("=")[0].split())
        m = re.fullmatch(r"(.*[\s*&])([A-Za-z_]\w*)", p)
        if m and m.group(1).strip() != "const":          # "<type> <name>"; an unnamed "const float*" or "int" has no name to drop
            p = m.group(1)
        out.append(re.sub(r"\s*([*&])\s*", r"\1", p).strip())
    return out


def test_generated_launcher_signatures_have_one_source(tmp_path):
    """Every launch_* the generators define has ONE parameter list (gen_common.SIGNATURES): the type list of its definition equals that of
    its prototype in the generated dispatch header, of the function-pointer typedef of every table that holds it, and -- for the variant-0
    launchers, which kernels.hpp declares by hand -- of the declaration there."""
    import subprocess
    import sys
    csrc = os.path.join(REPO, "mipnerf_pl_amd", "csrc")
    for gen in ("gen_mlp_bf16.py", "gen_mlp_train.py", "gen_mlp_f32r.py", "gen_pre_gemm.py"):
        subprocess.run([sys.executable, os.path.join(csrc, gen), str(tmp_path)], check=True, stdout=subprocess.DEVNULL)
    defs, protos, typedefs, tabled = {}, {}, {}, {}
    for f in sorted(os.listdir(tmp_path)):
        src = open(os.path.join(tmp_path, f), errors="replace").read() if f.endswith((".hip", ".hpp")) else ""
        if f.endswith(".hip"):
            for m in re.finditer(r"^hipError_t (launch_\w+)\(([^()]*)\) \{", src, re.M):
                assert m.group(1) not in defs, m.group(1)
                defs[m.group(1)] = _type_list(m.group(2))
        elif f.endswith("_variants_gen.hpp"):
            for m in re.finditer(r"^hipError_t (launch_\w+)\(([^()]*)\);", src, re.M):
                assert m.group(1) not in protos, m.group(1)
                protos[m.group(1)] = _type_list(m.group(2))
            for m in re.finditer(r"^typedef hipError_t \(\*(\w+)\)\(([^()]*)\);", src, re.M):
                typedefs[m.group(1)] = _type_list(m.group(2))
            for m in re.finditer(r"^static const (\w+) k\w+\[\d+\] = \{([^}]*)\};", src, re.M):
                for name in re.findall(r"\blaunch_\w+", m.group(2)):
                    tabled.setdefault(name, []).append(m.group(1))
    hand = {m.group(1): _type_list(m.group(2))
            for m in re.finditer(r"^hipError_t (launch_\w+)\(([^()]*)\);", open(os.path.join(csrc, "kernels.hpp")).read(), re.M)}
    nunits = sum(f.endswith(".hip") for f in os.listdir(tmp_path))
    assert len(defs) == nunits >= 18 and len(typedefs) == 7          # one launcher per generated unit, one typedef per launcher kind
    variant0 = sorted(n for n in defs if not re.search(r"_v\d+$", n))
    assert variant0 == ["launch_mlp_bf16", "launch_mlp_bf16_dgrad", "launch_mlp_bf16_trainfwd"]
    for name, types in defs.items():
        assert len(types) >= 7 and all(types), (name, types)
        declared = hand if name in variant0 else protos
        assert declared.get(name) == types, (name, "declaration", declared.get(name), types)
        assert tabled.get(name), f"{name} is in no dispatch table"
        for t in tabled[name]:
            assert typedefs[t] == types, (name, t, typedefs[t], types)
    assert sorted(protos) == sorted(n for n in defs if n not in variant0)
