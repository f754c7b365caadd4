"""CPU (no GPU): the multi-scale converter's contract around the device kernel -- the golden of the unmodified reference converter
(tests/golden/pyramid_48x40.npz, scripts/make_golden_pyramid.py) is reproduced byte for byte by the rule the kernel header states,
the metadata writer equals the reference's metadata.json, the new entry point is declared, exported and bound, and it validates its
arguments before any launch."""
import ctypes as C
import json
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import pyramid_fixture as pf  # noqa: E402

G = np.load(os.path.join(HERE, "golden", "pyramid_48x40.npz"))


@pytest.fixture(scope="module")
def roots(tmp_path_factory):
    return pf.write_roots(tmp_path_factory.mktemp("pyr"))


@pytest.fixture(scope="module")
def lib():
    from mipnerf_pl_amd import _lib as L
    if not os.path.exists(L.LIB_PATH):
        from mipnerf_pl_amd import build
        build.build(verbose=False)
    return L.lib()


def golden_png(name, rel):
    files = list(G[f"{name}_files"])
    return G[f"{name}_png_{files.index(rel)}"]


@pytest.mark.parametrize("name", pf.ROOTS)
def test_stated_rule_reproduces_every_golden_byte(roots, name):
    """Sequential order ((p00 + p01) + p10) + p11 in float32, / 4, levels never re-quantised, bytes truncated: 0 mismatches against what
    the reference converter wrote, on random RGBA and on mostly binary alpha; and the pixel rows the reference's Multicam reads back are
    byte / 255 composited with three roundings."""
    checked = 0
    for split in pf.SPLITS:
        frames = pf.read_frames(roots[name], split)
        levels = pf.rule_pyramid(frames, pf.N_DOWN)
        for i in range(frames.shape[0]):
            for j in range(pf.N_DOWN):
                want = golden_png(name, f"images_{split}/{i:03d}_d{j}.png")
                assert want.shape == levels[j][i].shape == (pf.H >> j, pf.W >> j, 4)
                assert int(np.count_nonzero(levels[j][i] != want)) == 0, (name, split, i, j)
                checked += want.size
        if split == "train":
            for wb in ((1, 0) if name == "random" else (1,)):
                got = pf.rule_pixels(levels, bool(wb)).reshape(-1, 3)
                want = G[f"{name}_pixels_wb{wb}"]
                assert got.dtype == want.dtype == np.float32 and np.array_equal(got.view(np.int32), want.view(np.int32))
    assert checked == 7 * 4 * sum((pf.H >> j) * (pf.W >> j) for j in range(pf.N_DOWN)) and len(G[f"{name}_files"]) == 7 * pf.N_DOWN


def test_rule_is_not_vacuous(roots):
    """The golden tells the stated rule from its neighbours: rounding to nearest and a pairwise summation order both miss bytes."""
    frames = pf.read_frames(roots["random"], "train")
    v = frames.astype(np.float32) / np.float32(255.0)
    want1 = np.stack([golden_png("random", f"images_train/{i:03d}_d1.png") for i in range(frames.shape[0])])
    seq = (((v[:, 0::2, 0::2] + v[:, 0::2, 1::2]) + v[:, 1::2, 0::2]) + v[:, 1::2, 1::2]) / np.float32(4.0)
    assert np.array_equal((seq * np.float32(255.0)).astype(np.uint8), want1)
    assert np.count_nonzero(np.rint(seq * np.float32(255.0)).astype(np.uint8) != want1) > 1000
    want3 = np.stack([golden_png("random", f"images_train/{i:03d}_d3.png") for i in range(frames.shape[0])])
    requant = pf.rule_pyramid(pf.rule_pyramid(pf.rule_pyramid(frames, 2)[1], 2)[1], 2)[1]          # re-quantising every level
    assert np.count_nonzero(requant != want3) > 0


@pytest.mark.parametrize("name", pf.ROOTS)
def test_metadata_writer_equals_the_reference(roots, name):
    from mipnerf_pl_amd import convert_blender_data as conv
    metas, files = conv.scene_metadata(roots[name], pf.N_DOWN)
    got = json.loads(json.dumps(metas, ensure_ascii=False, indent=4))
    want = json.loads(str(G[f"{name}_metadata"]))
    assert got == want                                               # floats compared with ==
    assert list(got) == list(want) == list(pf.SPLITS)
    for split in want:
        assert list(got[split]) == list(want[split]), split           # key order
    assert json.dumps(metas, ensure_ascii=False, indent=4) == str(G[f"{name}_metadata"])
    assert [len(files[s]) for s in pf.SPLITS] == [3, 2, 2]


def test_indivisible_size_names_the_file(tmp_path):
    import dataset_fixture as fx
    from mipnerf_pl_amd import convert_blender_data as conv
    root = fx.write_blender(str(tmp_path / "b"), seed=1, w=12, h=10)
    with pytest.raises(ValueError, match=r"r_0\.png.*not divisible"):
        conv.scene_metadata(root, 3)
    conv.scene_metadata(root, 2)
    with pytest.raises(ValueError, match="n_down"):
        conv.scene_metadata(root, 0)


def test_symbol_declared_exported_and_bound(lib):
    from mipnerf_pl_amd import _lib as L
    from mipnerf_pl_amd import build, ops
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(REPO, "include", "mipnerf_hip.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+mipnerf_box_pyramid\s*\(", hdr)
    assert "mipnerf_box_pyramid" in L.SIGNATURES and len(L.SIGNATURES["mipnerf_box_pyramid"][1]) == 11
    assert hasattr(lib, "mipnerf_box_pyramid") and callable(ops.box_pyramid)
    assert ("kernels_pyramid.hip", ["-ffp-contract=off"]) in build.UNITS
    assert lib.mipnerf_abi_version() == 6
    assert int(re.search(r"#define MIPNERF_MAX_PYRAMID_LEVELS (\d+)", hdr).group(1)) == L.MAX_PYRAMID_LEVELS == 8
    import mipnerf_pl_amd.convert_blender_data as conv
    assert callable(conv.convert_to_nerfdata) and callable(conv.main)
    from mipnerf_pl_amd.datasets import Multicam
    assert callable(Multicam.from_blender)


def test_argument_validation_without_a_device(lib):
    from mipnerf_pl_amd import _lib as L
    buf = (C.c_uint8 * 4096)()
    p = (C.addressof(buf) + 15) & ~15                   # any aligned non-null address: validation never dereferences it
    call = lib.mipnerf_box_pyramid
    assert call(1, 8, 8, 0, p, p, None, 0, 1, None, None) == L.E_INVALID          # zero levels
    assert b"box_pyramid" in lib.mipnerf_last_error()
    assert call(1, 256, 256, 9, p, p, None, 0, 1, p, None) == L.E_INVALID         # nine levels
    assert call(1, 12, 16, 4, p, p, None, 0, 1, None, None) == L.E_INVALID        # height not divisible by 8
    assert b"divisible" in lib.mipnerf_last_error()
    assert call(1, 16, 12, 4, p, p, None, 0, 1, None, None) == L.E_INVALID        # width not divisible by 8
    assert call(1, 8, 8, 4, None, p, None, 0, 1, None, None) == L.E_INVALID       # null source
    assert call(1, 8, 8, 4, p, None, None, 0, 1, None, None) == L.E_INVALID       # null output
    assert call(1, 32, 32, 5, p, p, None, 0, 1, None, None) == L.E_INVALID        # five levels need the scratch
    assert call(0, 8, 8, 4, p, p, None, 0, 1, None, None) == L.E_INVALID          # no images
    assert call(1, 8, 8, 4, p + 4, p, None, 0, 1, None, None) == L.E_INVALID      # misaligned source
    assert call(1, 8, 8, 4, p, p, p, -1, 1, None, None) == L.E_INVALID            # negative row offset
    from mipnerf_pl_amd import ops
    with pytest.raises(ValueError):
        ops.pyramid_sizes(40, 48, 5)
    with pytest.raises(ValueError):
        ops.pyramid_sizes(40, 48, 9)
    assert ops.pyramid_sizes(40, 48, 4) == [(40, 48), (20, 24), (10, 12), (5, 6)]
