"""CPU: error-guided batch sampling's pieces that need no device -- the settings, the cell table, the rule's own guarantees (checked on the
numpy statement of it, tests/guided_fixture.py), the refusals, and the C entry points' argument validation."""
import os

import numpy as np
import pytest

from mipnerf_pl_amd import config as cfg
from mipnerf_pl_amd import train_guided as tg
from tests import guided_fixture as fx

SIZES = [(37, 29), (16, 16), (8, 40), (3, 5)]          # (h, w): the images 29 x 37, 16 x 16, 40 x 8, 5 x 3
T = 8


def test_settings_defaults_ranges_and_unknown_keys():
    s = cfg.train_guided_settings({})
    assert s == {"enabled": False, "tile": 16, "interval": 64, "mix": 0.5, "rate": 0.25}
    assert sorted(cfg.TRAIN_GUIDED_DEFAULTS) == sorted("train.guided." + k for k in s)
    assert not any(k.startswith("train.guided") for k in cfg.DEFAULTS) and not any(k.startswith("train.guided") for k in cfg.TRAIN_OCCUPANCY_DEFAULTS)
    s = cfg.train_guided_settings({"train.guided.enabled": 1, "train.guided.tile": "8", "train.guided.mix": 0, "train.guided.rate": 1})
    assert s["enabled"] is True and s["tile"] == 8 and s["mix"] == 0.0 and s["rate"] == 1.0
    with pytest.raises(ValueError, match=r"train\.guided\.tiles.*train\.guided\.enabled"):
        cfg.train_guided_settings({"train.guided.tiles": 4})
    for key, bad in (("tile", 0), ("interval", 0), ("mix", 1.0), ("mix", -0.1), ("rate", 0.0), ("rate", 1.5)):
        with pytest.raises(ValueError, match=f"train.guided.{key}"):
            cfg.train_guided_settings({f"train.guided.{key}": bad})


def test_refusals_name_the_key_and_need_no_device(monkeypatch):
    on = dict(cfg.DEFAULTS, **{"train.guided.enabled": True})
    assert cfg.check_train_guided(on)["enabled"]
    with pytest.raises(NotImplementedError, match="num_gpus"):
        cfg.check_train_guided(dict(on, num_gpus=2))
    with pytest.raises(ValueError, match="loss.disable_multiscale_loss"):
        cfg.check_train_guided(dict(on, **{"loss.disable_multiscale_loss": True}))
    assert not cfg.check_train_guided(dict(cfg.DEFAULTS, num_gpus=2))["enabled"]          # off: nothing is refused
    # the Trainer raises them before it builds the system, reads the data or touches a device
    from mipnerf_pl_amd import system, train
    monkeypatch.setattr(system, "MipNeRFSystem", lambda *a, **k: pytest.fail("the system was built before the refusal"))
    monkeypatch.setattr(train, "setup_seed", lambda *a, **k: pytest.fail("device work before the refusal"))
    with pytest.raises(NotImplementedError, match="num_gpus"):
        train.Trainer(dict(on, num_gpus=2), device="cpu")
    with pytest.raises(NotImplementedError, match="num_gpus"):
        train.Trainer(on, world=2, device="cpu")
    with pytest.raises(ValueError, match="loss.disable_multiscale_loss"):
        train.Trainer(dict(on, **{"loss.disable_multiscale_loss": True}), device="cpu")
    with pytest.raises(ValueError, match="train.guided.mix"):
        train.Trainer(dict(on, **{"train.guided.mix": 1.0}), device="cpu")


def test_cell_table_on_edge_tiles_of_every_kind():
    tab = tg.cell_table(SIZES, T)
    np.testing.assert_array_equal(tab, fx.table(SIZES, T))
    assert tab.dtype == np.int64 and tab.shape == (5, 4)
    assert tuple(tab[-1]) == (30, 1664, 0, 0)
    np.testing.assert_array_equal(tab[:-1, 0], [0, 20, 24, 29])
    np.testing.assert_array_equal(tab[:-1, 1], [0, 1073, 1329, 1649])
    g = fx.cells(tab, T)
    assert len(g["n"]) == 30 and int(g["n"].sum()) == 1664
    kinds = {(int(w), int(h)) for w, h in zip(g["w"], g["h"])}
    assert {(8, 8), (5, 8), (8, 5), (5, 5), (5, 3)} <= kinds          # full, right edge, bottom edge, corner, an image smaller than a tile
    # every pixel of every image lies in exactly one cell
    seen = np.zeros(1664, np.int32)
    for c in range(30):
        for y in range(g["y0"][c], g["y0"][c] + g["h"][c]):
            x0 = g["pix0"][c] + y * g["W"][c] + g["x0"][c]
            seen[x0:x0 + g["w"][c]] += 1
    assert (seen == 1).all()
    with pytest.raises(ValueError):
        tg.cell_table(SIZES, 0)
    with pytest.raises(ValueError):
        tg.cell_table([], 8)


def _maps(n_cells):
    rng = np.random.default_rng(5)
    rand = rng.uniform(0.0, 0.3, n_cells).astype(np.float32)
    third = rand.copy()
    third[::3] = 0.0
    return {"random": rand, "third_zero": third, "all_zero": np.zeros(n_cells, np.float32)}


@pytest.mark.parametrize("mix", [0.0, 0.5, 0.9])
@pytest.mark.parametrize("which", ["random", "third_zero", "all_zero"])
def test_the_estimator_stays_the_uniform_mean(mix, which):
    tab = fx.table(SIZES, T)
    g = fx.cells(tab, T)
    err = _maps(30)[which]
    q, cdf, Q, A = fx.mass(err, g["n"], mix)
    assert Q == int(cdf[-1]) < (1 << 31) and (q >= 1).all() and (A == 0) == (which == "all_zero")
    P = fx.cell_probabilities(cdf)
    assert abs(P.sum() - 1.0) < 1e-12 and np.abs(P - q / Q).max() <= 2.2e-10
    # one draw per cell, from the first r0 that lands in it: its weight
    r0 = np.asarray([0] + [-((-int(m) << 32) // Q) for m in cdf[:-1]], np.uint64)
    order, w, c = fx.draw(tab, T, cdf, r0, np.zeros(30, np.uint64))
    np.testing.assert_array_equal(c, np.arange(30))
    w = w.astype(np.float64)
    assert abs((P * w).sum() - 1.0) <= 1e-6
    assert w.max() <= (1.0 + 1e-5) / (1.0 - mix)
    f = np.random.default_rng(9).uniform(-2.0, 5.0, 30)
    uniform_mean = (g["n"] * f).sum() / g["n"].sum()
    assert abs((P * w * f).sum() - uniform_mean) <= 1e-6
    if mix == 0.0:
        assert np.abs(w - 1.0).max() <= 1e-6


@pytest.mark.parametrize("mix", [0.0, 0.5, 0.9])
def test_every_drawn_id_lies_inside_its_cell_and_image(mix):
    tab = fx.table(SIZES, T)
    g = fx.cells(tab, T)
    for err in _maps(30).values():
        _, cdf, Q, _ = fx.mass(err, g["n"], mix)
        r0 = fx.boundary_r0(cdf)
        assert len(r0) >= 2 + 3 * 29
        for r1 in (0, (1 << 32) - 1, 0x9e3779b9):
            order, w, c = fx.draw(tab, T, cdf, r0, np.full(len(r0), r1, np.uint64))
            assert c.min() >= 0 and c.max() <= 29 and np.isfinite(w).all() and (w > 0).all()
            img = np.searchsorted(tab[:, 1], order, side="right") - 1
            np.testing.assert_array_equal(img, g["img"][c])
            p = order - tab[img, 1]
            x, y = p % tab[img, 2], p // tab[img, 2]
            assert ((x >= g["x0"][c]) & (x < g["x0"][c] + g["w"][c]) & (y >= g["y0"][c]) & (y < g["y0"][c] + g["h"][c])).all()
            if r1 == 0:
                assert ((x == g["x0"][c]) & (y == g["y0"][c])).all()
            if r1 == (1 << 32) - 1:
                assert ((x == g["x0"][c] + g["w"][c] - 1) & (y == g["y0"][c] + g["h"][c] - 1)).all()
        # the cell of a draw is the first one whose cdf exceeds t, on both sides of every boundary
        t = (r0 * np.uint64(Q)) >> np.uint64(32)
        _, _, c = fx.draw(tab, T, cdf, r0, np.zeros(len(r0), np.uint64))
        assert (cdf[c] > t).all() and (np.where(c > 0, cdf[np.maximum(c, 1) - 1], 0) <= t).all()
        assert c[0] == 0 and c[-1] == 29


def test_fold_and_per_draw_error_of_the_fixture():
    rgb = np.asarray([[0.5, 0.25, 1.0], [0.1, 0.2, 0.3], [np.nan, 0.0, 0.0], [np.inf, 0.0, 0.0]], np.float32)
    gt = np.asarray([[0.0, 0.25, 0.0], [0.1, 0.2, 0.3], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]], np.float32)
    f, ok = fx.draw_error(rgb, gt)
    assert list(ok) == [True, True, False, False] and int(f[0]) == int(1.25 * (1 << 24)) and int(f[1]) == 0
    s, cnt = np.zeros(3, np.uint64), np.zeros(3, np.uint32)
    fx.accumulate(s, cnt, np.asarray([2, 2, 0, 1, 7, -1], np.int32), 0, 4, 3, rgb, gt)      # 3 of 4 rays lie inside the order
    assert list(cnt) == [0, 0, 2] and int(s[2]) == int(1.25 * (1 << 24))
    err = fx.fold(np.ones(3, np.float32), s, cnt, 0.25)
    assert err.dtype == np.float32 and err[0] == 1.0 and err[1] == 1.0 and err[2] == np.float32(1.0) + np.float32(0.25) * (np.float32(0.625) - np.float32(1.0))
    assert fx.fold(np.ones(3, np.float32), s, cnt, 1.0)[2] == np.float32(0.625)


def test_a_state_of_another_tile_or_other_images_is_refused():
    sd = {"tile": 8, "sizes": [(37, 29), (16, 16)]}
    tg.check_state(sd, 8, [(37, 29), (16, 16)])
    tg.check_state(sd, 8, [[37, 29], [16, 16]])
    with pytest.raises(ValueError, match="tile 8.*configured for 16"):
        tg.check_state(sd, 16, [(37, 29), (16, 16)])
    with pytest.raises(ValueError, match="other sizes"):
        tg.check_state(sd, 8, [(37, 29), (16, 17)])
    with pytest.raises(ValueError, match="other sizes"):
        tg.check_state(sd, 8, [(37, 29)])
    assert tg.refresh_due(0, 64) and tg.refresh_due(128, 64) and not tg.refresh_due(65, 64)


def test_entry_points_are_declared_bound_exported_and_validate_before_any_device_call():
    import re
    from mipnerf_pl_amd import _lib as L
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mipnerf_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = L.lib()
    assert lib.mipnerf_abi_version() == 6
    for name in ("mipnerf_guided_apply", "mipnerf_guided_accumulate", "mipnerf_guided_refresh", "mipnerf_guided_draw"):
        proto = re.search(r"int " + name + r"\(([^)]*)\)", code)
        assert proto is not None and len(proto.group(1).split(",")) == len(L.SIGNATURES[name][1]) and hasattr(lib, name)
    one = 8      # any non-null address: validation never dereferences
    assert lib.mipnerf_guided_apply(0, 0, 1, one, None, None, 0, one, None) == L.E_INVALID
    assert b"guided_apply" in lib.mipnerf_last_error()
    assert lib.mipnerf_guided_apply(4, 4, 4, one, one, None, 0, one, None) == L.E_INVALID          # step without epoch_base
    assert lib.mipnerf_guided_accumulate(4, 4, 4, one, 0, None, None, 0, one, one, one, one, None) == L.E_INVALID
    assert b"guided_accumulate" in lib.mipnerf_last_error()
    ok = (1, one, 8, 30, 0.25, 0.5, one, one, one, one, one, one, one, 4, one, None)

    def refresh(**kw):
        names = ("n_images", "table", "tile", "n_cells", "rate", "mix", "err", "sum", "cnt", "seen", "q", "cdf", "scratch", "words", "header", "stream")
        return lib.mipnerf_guided_refresh(*[kw.get(n, v) for n, v in zip(names, ok)])
    for bad in (dict(rate=0.0), dict(rate=1.5), dict(mix=1.0), dict(mix=-0.5), dict(n_cells=0), dict(n_cells=1 << 30), dict(tile=0), dict(table=None)):
        assert refresh(**bad) == L.E_INVALID, bad
        assert b"guided_refresh" in lib.mipnerf_last_error()
    assert refresh(words=3) == L.E_WORKSPACE and b"guided_refresh" in lib.mipnerf_last_error()
    assert lib.mipnerf_guided_draw(5, one, 1, one, 8, 30, one, one, one, one, one, 4, 0, None) == L.E_INVALID      # more draws than ring slots
    assert b"guided_draw" in lib.mipnerf_last_error()
    assert lib.mipnerf_guided_draw(-1, one, 1, one, 8, 30, one, one, one, one, one, 4, 0, None) == L.E_INVALID
    assert lib.mipnerf_guided_draw(0, None, 1, one, 8, 30, one, one, None, one, one, 4, 0, None) == L.OK           # no draws: no launch


def test_kernels_live_in_their_own_unit_built_without_contraction():
    from mipnerf_pl_amd import build
    assert ("kernels_guided.hip", ["-ffp-contract=off"]) in [(u, list(f)) for u, f in build.UNITS]
    src = open(os.path.join(build.CSRC, "kernels_guided.hip")).read()
    for k in ("k_guided_apply", "k_guided_accumulate", "k_guided_fold_mass", "k_guided_mass_q", "k_guided_draw"):
        assert f"\n{k}(" in src
    assert "template <int K" not in src and "asm" not in src
    assert "atomicAdd(float" not in src and "unsafeAtomicAdd" not in src          # integer atomics only
