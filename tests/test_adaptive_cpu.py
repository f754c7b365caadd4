"""CPU (no GPU): the rule of adaptive sample counts restated in numpy (tests/adaptive_fixture.py) against first principles, the default
ladders, argument validation of mipnerf_bucket_rays / mipnerf_gather_frame without a device, the agreement of the header, the binding and
the docstrings on the rule, and the command-line flags."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import adaptive_fixture as ax

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the rule ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S,N,ladder", [(128, 128, (32, 64, 96, 128)), (128, 64, (16, 32, 48, 64)), (64, 128, (32, 64, 96, 128)),
                                        (128, 128, (128,)), (100, 7, (1, 2, 3, 4, 5, 6, 7)), (5, 1024, (256, 512, 768, 1024))])
def test_need_at_a_ladder_entry_stays_and_one_more_moves_up(S, N, ladder):
    """every span length 1 .. S: need from the definition (the smallest integer >= span * N / S), 1 <= need <= N; need == c_b is bucket b
    and need == c_b + 1 is bucket b + 1; the full span is the top bucket"""
    span = np.arange(1, S + 1)
    first = np.zeros(S, np.int64)
    nd = ax.need(first, span - 1, S, N)
    want = np.array([next(k for k in range(1, N + 1) if k * S >= s * N) for s in span])
    assert np.array_equal(nd, want) and nd.min() >= 1 and nd.max() == N
    b = ax.bucket(np.ones(S, bool), first, span - 1, S, ladder)
    assert b[-1] == len(ladder) - 1 and (np.diff(b) >= 0).all() and b.min() >= 0
    for k, c in enumerate(ladder):
        assert (b[nd == c] == k).all()
        if k + 1 < len(ladder):
            assert (b[nd == c + 1] == k + 1).all()
        lo = ladder[k - 1] if k else 0
        assert np.array_equal(b == k, (nd > lo) & (nd <= c))
    # the spacing guarantee: c_bucket / N >= span / S, i.e. (far' - near') / c_b <= (far - near) / N on linear fence posts
    assert (np.asarray(ladder)[b] * S >= span * N).all()
    # a span that does not start at 0 counts the same
    assert np.array_equal(ax.bucket(np.ones(S, bool), first + 3, span + 2, S, ladder), b)


def test_both_directions_of_differing_counts_by_hand():
    # S = 128 frusta, N = 64 samples: 33 frusta need ceil(33 / 2) = 17 samples -> past 16, bucket 1; 32 frusta need 16 -> bucket 0
    assert ax.need([0, 0], [31, 32], 128, 64).tolist() == [16, 17]
    assert ax.bucket([1, 1], [0, 0], [31, 32], 128, (16, 32, 48, 64)).tolist() == [0, 1]
    # S = 64 frusta, N = 128 samples: 16 frusta need 32 -> bucket 0; 17 need 34 -> bucket 1; all 64 need 128 -> bucket 3
    assert ax.need([5, 5, 0], [20, 21, 63], 64, 128).tolist() == [32, 34, 128]
    assert ax.bucket([1, 1, 1], [5, 5, 0], [20, 21, 63], 64, (32, 64, 96, 128)).tolist() == [0, 1, 3]


def test_dead_rays_and_the_padded_stable_partition():
    S, ladder = 128, (32, 64, 96, 128)
    rng = np.random.default_rng(0)
    n = 700
    live = rng.random(n) < 0.8
    first = rng.integers(0, S, n)
    last = np.minimum(S - 1, first + rng.integers(0, S, n))
    first, last = np.where(live, first, S), np.where(live, last, -1)           # what ray_span writes for a dead ray
    b = ax.bucket(live, first, last, S, ladder)
    assert (b[~live] == -1).all() and (b[live] >= 0).all()
    counts, base, slot = ax.partition(live, first, last, S, ladder)
    assert sum(counts) == int(live.sum()) and base[0] == 0 and all(x % 64 == 0 for x in base)
    assert all(base[k + 1] - (base[k] + counts[k]) in range(64) for k in range(4)) and base[-1] <= n + 64 * 4
    assert (slot[~live] == -1).all() and len(set(slot[live].tolist())) == int(live.sum())
    for k in range(4):
        s = slot[b == k]
        assert np.array_equal(s, base[k] + np.arange(counts[k]))                # in the original order, without holes
    assert ax.sample_share(live, first, last, S, ladder) == pytest.approx(np.asarray(ladder)[b[live]].mean() / 128.0)
    assert np.isnan(ax.sample_share(np.zeros(3, bool), [S] * 3, [-1] * 3, S, ladder))
    assert ax.bases([0, 0, 0, 0]) == [0] * 5 and ax.bases([64, 1, 0, 128]) == [0, 64, 128, 128, 256]


@pytest.mark.parametrize("N", [1, 2, 3, 5, 64, 128, 1024])
def test_default_ladders(N):
    from mipnerf_pl_amd import ops
    lad = ops.sample_ladder(N)
    assert lad == ax.default_ladder(N) and isinstance(lad, tuple)
    assert lad[-1] == N and lad[0] >= 1 and 1 <= len(lad) <= 4 and all(a < b for a, b in zip(lad, lad[1:]))
    assert set(lad) == {int(np.ceil(N * k / 4.0)) for k in range(1, 5)}
    assert ops.sample_ladder(N, lad) == lad
    assert ops.sample_ladder(128) == (32, 64, 96, 128)


def test_ladder_validation():
    from mipnerf_pl_amd import ops
    assert ops.sample_ladder(128, [128]) == (128,) and ops.sample_ladder(64, (1, 2, 3, 4, 5, 6, 7, 64)) == (1, 2, 3, 4, 5, 6, 7, 64)
    for bad in ([], [64], [0, 128], [64, 64, 128], [96, 64, 128], [128, 129], list(range(120, 129)), [32.5, 128], ["x"], 128):
        with pytest.raises(ValueError, match="strictly increasing"):
            ops.sample_ladder(128, bad)
    for n in (0, 1025):
        with pytest.raises(ValueError, match="num_samples"):
            ops.sample_ladder(n)
    assert ops.bucket_bases([64, 1, 0, 128]) == ax.bases([64, 1, 0, 128])


# ---- validation without a device -------------------------------------------------------------------------------------------------
def _ladder(*c):
    return (C.c_int32 * len(c))(*c)


def test_bucket_rays_validates_its_arguments_without_a_gpu():
    from mipnerf_pl_amd import _lib as L
    lib = L.lib()
    rp, op = L.RaysPtrs(), L.RaysPtrs()
    counts = (C.c_int64 * 8)(*([7] * 8))
    lad = _ladder(32, 64, 96, 128)
    ws = lib.mipnerf_bucket_rays_workspace_bytes(4, 4)
    assert ws >= 256 + 16 and ws % 16 == 0
    good = dict(n=4, live=16, first=16, last=16, S=128, N=128, B=4, lad=lad, rays=C.byref(rp), out=C.byref(op), slot=16, ws=16, wsb=ws, counts=counts)

    def call(**kw):
        a = dict(good, **kw)
        return lib.mipnerf_bucket_rays(a["n"], a["live"], a["first"], a["last"], a["S"], a["N"], a["B"], a["lad"], a["rays"], a["out"], a["slot"],
                                       a["ws"], a["wsb"], a["counts"], None)
    for kw in (dict(live=None), dict(first=None), dict(last=None), dict(rays=None), dict(out=None), dict(slot=None), dict(ws=None),
               dict(lad=None), dict(counts=None)):
        assert call(**kw) == L.E_INVALID and "bucket_rays" in L.last_error() and "null" in L.last_error(), kw
    for kw in (dict(lad=_ladder(32, 64, 64, 128)), dict(lad=_ladder(64, 32, 96, 128)), dict(lad=_ladder(0, 64, 96, 128)),
               dict(lad=_ladder(32, 64, 96, 127)), dict(lad=_ladder(32, 64, 96, 129)), dict(B=0), dict(B=9), dict(B=-1)):
        assert call(**kw) == L.E_INVALID and "bucket_rays" in L.last_error() and "ladder" in L.last_error(), kw
    for kw in (dict(S=0), dict(S=L.MAX_SAMPLES + 1), dict(N=0), dict(N=L.MAX_SAMPLES + 1, lad=_ladder(32, 64, 96, L.MAX_SAMPLES + 1))):
        assert call(**kw) == L.E_INVALID and "bucket_rays" in L.last_error() and "num_samples" in L.last_error(), kw
    assert call(n=-1) == L.E_INVALID and "ray count" in L.last_error()
    assert call(n=1 << 31) == L.E_INVALID
    assert call(wsb=ws - 1) != L.OK and "workspace" in L.last_error()
    assert call(ws=8) == L.E_INVALID and "aligned" in L.last_error()
    # zero rays: zero counts and nothing launched, whatever the pointers
    assert call(n=0, live=None, first=None, last=None, rays=None, out=None, slot=None, ws=None, wsb=0) == L.OK
    assert list(counts)[:4] == [0, 0, 0, 0] and list(counts)[4:] == [7] * 4
    assert lib.mipnerf_bucket_rays_workspace_bytes(0, 4) > 0 and lib.mipnerf_bucket_rays_workspace_bytes(-1, 4) == 0
    assert lib.mipnerf_bucket_rays_workspace_bytes(4, 0) == 0 and lib.mipnerf_bucket_rays_workspace_bytes(4, 9) == 0
    # one entry per 1024 rays and bucket behind the 256-byte header
    assert lib.mipnerf_bucket_rays_workspace_bytes(640000, 8) >= 256 + 4 * 8 * 625


def test_gather_frame_validates_its_arguments_without_a_gpu():
    from mipnerf_pl_amd import _lib as L
    lib = L.lib()
    comp, full = (L.LevelOut * 2)(), (L.LevelOut * 2)()
    for arr in (comp, full):
        for l in range(2):
            arr[l] = L.LevelOut(16, 16, 16, None, None)
    assert lib.mipnerf_gather_frame(4, 4, 0, 16, 16, 1, comp, full, None) == L.E_INVALID and "gather_frame" in L.last_error()
    assert lib.mipnerf_gather_frame(4, 4, 5, 16, 16, 1, comp, full, None) == L.E_INVALID and "num_levels" in L.last_error()
    assert lib.mipnerf_gather_frame(-1, 4, 2, 16, 16, 1, comp, full, None) == L.E_INVALID and "ray count" in L.last_error()
    assert lib.mipnerf_gather_frame(4, -1, 2, 16, 16, 1, comp, full, None) == L.E_INVALID
    assert lib.mipnerf_gather_frame(4, 4, 2, None, 16, 1, comp, full, None) == L.E_INVALID and "null" in L.last_error()
    assert lib.mipnerf_gather_frame(4, 4, 2, 16, None, 1, comp, full, None) == L.E_INVALID
    assert lib.mipnerf_gather_frame(4, 4, 2, 16, 16, 1, None, full, None) == L.E_INVALID
    assert lib.mipnerf_gather_frame(4, 4, 2, 16, 16, 1, comp, None, None) == L.E_INVALID
    full[1] = L.LevelOut(16, None, 16, None, None)
    assert lib.mipnerf_gather_frame(4, 4, 2, 16, 16, 1, comp, full, None) == L.E_INVALID and "level 1" in L.last_error()
    assert lib.mipnerf_gather_frame(0, 0, 2, None, None, 1, None, None, None) == L.OK


# ---- one statement of the rule ----------------------------------------------------------------------------------------------------
def _squash(s):
    return re.sub(r"[\s*]+", " ", s)


def test_header_binding_and_docstrings_agree_on_the_rule():
    import inspect
    from mipnerf_pl_amd import _lib as L
    from mipnerf_pl_amd import build, model, ops
    hdr = open(os.path.join(REPO, "include", "mipnerf_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    for name in ("mipnerf_bucket_rays", "mipnerf_bucket_rays_workspace_bytes", "mipnerf_gather_frame"):
        proto = re.search(r"\b" + name + r"\(([^)]*)\)", code).group(1)
        assert len(proto.split(",")) == len(L.SIGNATURES[name][1]), name
    assert len(L.SIGNATURES["mipnerf_bucket_rays"][1]) == 15 and len(L.SIGNATURES["mipnerf_gather_frame"][1]) == 9
    # after the scatter's rules, inside the same block of rules
    assert hdr.index("mipnerf_scatter_frame: writes every pixel") < hdr.index("mipnerf_bucket_rays: a sample count per ray") \
        < hdr.index("mipnerf_gather_frame: writes every pixel") < hdr.index("int64_t mipnerf_occupancy_words(")
    h = _squash(hdr)
    for name, doc in (("ops.bucket_rays", ops.bucket_rays.__doc__), ("CulledFrame", model.CulledFrame.__doc__)):
        d = _squash(doc)
        for phrase in ["need = ((last - first + 1) N + S - 1) / S in integer division (1 <= need <= N)", "bucket = the smallest b with c_b >= need",
                       "a dead ray has bucket -1", "c_0 < c_1 < ... < c_{B-1} with 1 <= c_0", "c_{B-1} == N", "1 <= B <= 8",
                       "c_b samples per level on [near', far']", "coarse spacing is at most the untightened ray's"]:
            assert phrase in h, phrase
            assert phrase in d, (name, phrase)
    assert h.count("need = ((last - first + 1) N + S - 1) / S") == 1                      # stated once in the header
    for phrase in ["base_0 = 0, base_{b+1} = round_up(base_b + count_b, 64)", "keep their original order"]:
        assert phrase in h and phrase in _squash(ops.bucket_rays.__doc__), phrase
    assert "never written" in h and "SYNCHRONISATION" in h and "no atomics" in h
    assert "dead-pixel rule of mipnerf_scatter_frame" in h and "ORIGINAL near" in h and "ORIGINAL near" in _squash(ops.gather_frame.__doc__)
    doc = _squash(model.CulledFrame.__doc__)
    assert "adaptive=True" in doc and "bucket_counts" in doc and "sample_share" in doc and "NOT the untightened frame" in doc
    sig = inspect.signature(model.CulledFrame.__init__)
    assert list(sig.parameters)[-2:] == ["adaptive", "ladder"]
    assert sig.parameters["adaptive"].default is False and sig.parameters["ladder"].default is None
    assert list(inspect.signature(ops.bucket_rays).parameters) == ["live", "first", "last", "rays", "span_samples", "ladder", "out_rays", "slot",
                                                                   "workspace"]
    assert list(inspect.signature(ops.gather_frame).parameters) == ["slot", "compact_outputs", "full_outputs", "near", "white_bkgd"]
    assert list(inspect.signature(ops.sample_ladder).parameters) == ["num_samples", "ladder"]
    # a unit of its own: the per-ray K templates of kernels_occupancy.hip are counted elsewhere
    assert ("kernels_bucket.hip", []) in build.UNITS
    src = open(os.path.join(REPO, "mipnerf_pl_amd", "csrc", "kernels_bucket.hip")).read()
    assert "template <int K" not in src and "atomic" not in src.replace("No atomics", "")
    for k in ("k_bucket_count", "k_bucket_scan", "k_bucket_gather", "k_gather_frame"):
        assert re.search(r"__global__[^;{]*\b" + k + r"\(", src), k


# ---- command line ------------------------------------------------------------------------------------------------------------------
def test_adaptive_flags_and_their_defaults_on_both_command_lines():
    from mipnerf_pl_amd import eval as eval_cli
    from mipnerf_pl_amd import render_video
    for parser in (eval_cli.build_parser(), render_video.build_parser()):
        a = parser.parse_args(["--out_dir", "o", "--scale", "1"])
        assert a.cull_adaptive is False and a.cull_ladder is None and a.cull is False and a.cull_tighten is False
        a = parser.parse_args(["--out_dir", "o", "--scale", "1", "--cull", "--cull_adaptive", "--cull_ladder", "16", "32", "64"])
        assert a.cull is True and a.cull_adaptive is True and a.cull_ladder == [16, 32, 64] and a.cull_tighten is False
        text = _squash(parser.format_help())
        assert "--cull_adaptive" in text and "--cull_ladder C [C ...]" in text
        assert "Not the untightened frame" in text[text.index("--cull_adaptive"):] and "Guaranteed" in text
        assert "never wider than the untightened frame's" in text and "cells the grid proves empty" in text


def test_adaptive_refusals_come_before_anything_is_loaded(tmp_path):
    from types import SimpleNamespace
    from mipnerf_pl_amd import eval as eval_cli
    from mipnerf_pl_amd import render_video
    missing = str(tmp_path / "no_such.ckpt")               # never opened: the refusal comes first
    ev = ["--ckpt", missing, "--data", str(tmp_path), "--out_dir", str(tmp_path / "o"), "--scale", "1"]
    rv = ["--ckpt", missing, "--out_dir", str(tmp_path / "o"), "--scale", "1"]
    for main, base in ((eval_cli.main, ev), (render_video.main, rv)):
        with pytest.raises(SystemExit, match="--cull_adaptive.*--cull"):
            main(base + ["--cull_adaptive"])
        with pytest.raises(SystemExit, match="--cull_ladder.*--cull_adaptive"):
            main(base + ["--cull", "--cull_ladder", "64", "128"])
        for bad in (["64", "64", "128"], ["128", "64"], ["0", "128"], [str(c) for c in range(1, 10)]):
            with pytest.raises(SystemExit, match="strictly increasing"):
                main(base + ["--cull", "--cull_adaptive", "--cull_ladder"] + bad)
    assert not os.path.exists(str(tmp_path / "o"))
    render_video.refuse_adaptive_without_cull(SimpleNamespace(cull=True, cull_adaptive=True, cull_ladder=[64, 128]))
    render_video.refuse_adaptive_without_cull(SimpleNamespace(cull=True, cull_adaptive=True, cull_ladder=None))
    render_video.refuse_adaptive_without_cull(SimpleNamespace(cull=False, cull_adaptive=False, cull_ladder=None))
    # the ladder against the count the system renders with
    system = SimpleNamespace(mip_nerf=SimpleNamespace(num_samples=64))
    assert render_video.cli_ladder(SimpleNamespace(cull_adaptive=False, cull_ladder=None), system) is None
    assert render_video.cli_ladder(SimpleNamespace(cull_adaptive=True, cull_ladder=None), system) == (16, 32, 48, 64)
    assert render_video.cli_ladder(SimpleNamespace(cull_adaptive=True, cull_ladder=[8, 64]), system) == (8, 64)
    with pytest.raises(SystemExit, match="c_\\{B-1\\} == num_samples"):
        render_video.cli_ladder(SimpleNamespace(cull_adaptive=True, cull_ladder=[64, 128]), system)


def test_closing_line_reports_the_sample_share(capsys):
    from mipnerf_pl_amd.evaluate import report_live_share
    report_live_share([0.5, 1.0], [0.25, float("nan")], [0.5, float("nan")])
    assert capsys.readouterr().out.strip() == ("cull: mean live share per frame: 0.7500 (2 frames); mean span share of the live rays: 0.2500; "
                                               "mean sample share of the live rays: 0.5000")
    report_live_share([0.5], [0.25])
    assert capsys.readouterr().out.strip() == "cull: mean live share per frame: 0.5000 (1 frames); mean span share of the live rays: 0.2500"
