"""GPU: the sparse row table of the baked preview (libmipnerf_preview_sparse.so, `preview.SparseField`).  The dense march with the same
occupancy is an exact oracle -- a sample in a clear cell loads no row, so storing only the rows next to stored cells changes no output
byte -- and every comparison here is on bytes: the table and the count against the numpy restatement of
tests/preview_sparse_fixture.py, the compact rows against `dense_rows[mask]`, the sparse marches against `preview.march` /
`preview.march_pyramid` of the dense lattices, the sparse bake against the dense bake's `to_sparse()`, the command's PNGs.

Shapes: the lattices of the fixture (nx = 32 m + 1 among them) under the five occupancies; one lattice whose table has more than 4096
blocks of 256 words, where the one-workgroup scan takes a second round."""
import os
import re

import numpy as np
import pytest
import torch

import preview_fixture as pf
import preview_mip_fixture as mf
import preview_sparse_fixture as sf

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BG = (0.0, 0.25, 0.5)


def _occupancy(words, dims):
    from mipnerf_pl_amd import ops
    occ = ops.Occupancy(torch.from_numpy(np.ascontiguousarray(words).view(np.int32)).to(DEV).view(torch.uint32), dims, pf.LO, pf.HI)
    occ.threshold, occ.dilate = sf.THRESHOLD, 0
    return occ


def _dense(rows, dims, degree, occ):
    from mipnerf_pl_amd import preview
    return preview.BakedField(torch.from_numpy(np.ascontiguousarray(rows)).to(DEV), dims, pf.LO, pf.HI, degree, occ)


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def same_bytes(got, want, nan_ok=False):
    """every output array equal as bytes; `nan_ok`: a NaN where the other has one, bytes elsewhere"""
    for a, b in zip(got, want):
        assert a.shape == b.shape and a.dtype == b.dtype
        if nan_ok and a.dtype == torch.float32:
            assert torch.equal(torch.isnan(a), torch.isnan(b))
            keep = ~torch.isnan(a)
            assert torch.equal(_bits(a[keep].contiguous()), _bits(b[keep].contiguous()))
        else:
            assert torch.equal(_bits(a), _bits(b))


@pytest.fixture(scope="module")
def rays():
    return [torch.from_numpy(a).to(DEV) for a in pf.scene_rays()]


def run_march(field, rays, step_scale=0.5, t_min=0.0, max_steps=4096):
    from mipnerf_pl_amd import preview
    o, d, tn, tf = rays
    steps = torch.full((o.shape[0],), -7, dtype=torch.int32, device=DEV)
    rgb, acc, dist = preview.march(field, o, d, tn, tf, BG, step_scale, t_min, max_steps, steps=steps)
    return rgb, acc, dist, steps


def run_pyramid(pyr, rays, radii, footprint, step_scale=0.5, t_min=0.0, max_steps=4096):
    from mipnerf_pl_amd import preview
    o, d, tn, tf = rays
    steps = torch.full((o.shape[0],), -7, dtype=torch.int32, device=DEV)
    lod = torch.full((o.shape[0],), -7.0, device=DEV)
    rgb, acc, dist = preview.march_pyramid(pyr, o, d, radii, tn, tf, BG, footprint, step_scale, t_min, max_steps, steps=steps, lod=lod)
    return rgb, acc, dist, steps, lod


# ---- the table -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", sf.LATTICES)
def test_index_equals_the_numpy_table(dims):
    from mipnerf_pl_amd import preview
    for kind in sf.OCCUPANCIES:
        words = sf.occupancy_words(kind, dims)
        want, m, _ = sf.numpy_table(words, dims)
        occ = _occupancy(words, dims)
        table, total = preview.index_table(occ)
        again, total2 = preview.index_table(occ)
        assert total == total2 == m, kind
        assert table.cpu().numpy().view(np.uint32).tobytes() == want.tobytes(), kind
        assert torch.equal(table, again), kind


def test_index_over_more_blocks_than_one_scan_round_holds():
    """(33, 600, 900): 2 x 600 x 900 table words = 4219 blocks of 256, more than the 4096 block totals the one workgroup scans per round;
    the torch restatement (held to the numpy table in test_preview_sparse_cpu.py) is the reference at this size"""
    from mipnerf_pl_amd import ops, preview
    dims = (33, 600, 900)
    gen = torch.Generator(device=DEV).manual_seed(3)
    cells = torch.rand(899, 599, 32, device=DEV, generator=gen) < 0.05
    occ = ops.Occupancy(preview.cells_to_bits(cells), dims, pf.LO, pf.HI)
    table, total = preview.index_table(occ)
    want, m = preview.table_of_points(preview.baked_points(occ))
    assert total == m and 0 < m < 33 * 600 * 900 and torch.equal(table, want)
    assert int(table[-1, -1, -1, 1]) > 2 ** 22          # the ranks really run past the first round


# ---- gather and pack ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("degree", [0, 1, 2])
def test_gather_and_pack_equal_the_masked_dense_rows(degree):
    from mipnerf_pl_amd import preview
    rng = np.random.default_rng(40 + degree)
    for dims in ((33, 5, 4), (65, 4, 3), (8, 9, 10)):
        nx, ny, nz = dims
        nb = (degree + 1) ** 2
        sigma = rng.uniform(0, 50, (nz, ny, nx)).astype(np.float32)
        sigma.reshape(-1)[:8] = [1e6, 65504.0, 65519.0, 65520.0, np.inf, 0.0, 6e-8, 3.0]
        coef = rng.normal(0, 3, (nz, ny, nx, nb, 3)).astype(np.float32)
        coef.reshape(-1)[:5] = [1e6, -1e6, 2.0 ** -25, 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11]
        sig_t, coef_t = torch.from_numpy(sigma).to(DEV), torch.from_numpy(coef).to(DEV)
        dense = preview.pack_rows(sig_t, coef_t, degree)
        for kind in ("hollow", "set", "clear", "x31"):
            words = sf.occupancy_words(kind, dims)
            _, m, pts = sf.numpy_table(words, dims)
            mask = torch.from_numpy(pts).to(DEV).reshape(-1)
            want = dense.reshape(-1, dense.shape[-1])[mask]
            table, total = preview.index_table(_occupancy(words, dims))
            assert total == m == want.shape[0]
            got = preview.gather_rows(dense, table, total, degree)
            assert tuple(got.shape) == (m, pf.ROW_HALVES[degree]) and torch.equal(got.view(torch.int16), want.view(torch.int16))
            packed = torch.full((m, pf.ROW_HALVES[degree]), 7.0, dtype=torch.float16, device=DEV)
            preview.sparse_pack(sig_t.reshape(-1)[mask], coef_t.reshape(-1, nb, 3)[mask].contiguous(), degree, packed)
            assert torch.equal(packed.view(torch.int16), want.view(torch.int16))


# ---- one lattice -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("degree", [0, 1, 2])
@pytest.mark.parametrize("dilate", [0, 1])
def test_sparse_march_is_the_dense_march(rays, degree, dilate):
    from mipnerf_pl_amd import ops, preview
    rows, _ = pf.random_rows(degree, hollow=True)
    occ = ops.occupancy_grid(torch.from_numpy(rows[..., 0].astype(np.float32)).to(DEV), sf.THRESHOLD, pf.LO, pf.HI, dilate=dilate)
    dense = _dense(rows, pf.DIMS, degree, occ)
    sparse = dense.to_sparse()
    assert sparse.stored is None
    assert isinstance(sparse, preview.SparseField) and 0 < sparse.n_rows < 8 * 9 * 10 and sparse.nbytes < dense.nbytes
    assert torch.equal(sparse.rows.view(torch.int16), dense.rows.reshape(-1, dense.rows.shape[-1])[preview.baked_points(occ).reshape(-1)]
                       .view(torch.int16))
    want = run_march(dense, rays)
    same_bytes(run_march(sparse, rays), want)
    assert int(want[3].max()) > 0
    # several blocks of 64 samples and a step cap; the same through render_rays' dispatch
    same_bytes(run_march(sparse, rays, 0.1, 0.0, 70), run_march(dense, rays, 0.1, 0.0, 70))
    assert int(run_march(dense, rays, 0.1, 0.0, 70)[3].max()) > 64
    # the constructor accepts the table it would have made itself and the round trip to dense keeps the stored rows
    again = preview.SparseField(sparse.rows, sparse.table.clone(), sparse.dims, sparse.lo, sparse.hi, degree, occ)
    same_bytes(run_march(again, rays), want)
    same_bytes(run_march(sparse.to_dense(), rays), want)


def test_sparse_march_early_stop_on_the_opaque_fixture(rays):
    from mipnerf_pl_amd import ops
    rows, _ = pf.random_rows(2, opaque=True)
    occ = ops.occupancy_grid(torch.from_numpy(rows[..., 0].astype(np.float32)).to(DEV), 45.0, pf.LO, pf.HI, dilate=0)
    assert 0.5 < occ.occupied_fraction() < 0.95          # a corner exceeds 45 with probability 1 / 6: about a quarter of the cells are clear
    dense = _dense(rows, pf.DIMS, 2, occ)
    want = run_march(dense, rays, 0.1, 1e-3, 4096)
    full = run_march(dense, rays, 0.1, 0.0, 4096)
    assert bool((want[3] < full[3]).any())                          # the stop really cuts rays
    same_bytes(run_march(dense.to_sparse(), rays, 0.1, 1e-3, 4096), want)


def test_a_nan_row_poisons_the_same_rays(rays):
    from mipnerf_pl_amd import ops
    rows, _ = pf.random_rows(1, hollow=True)
    occ = ops.occupancy_grid(torch.from_numpy(rows[..., 0].astype(np.float32)).to(DEV), sf.THRESHOLD, pf.LO, pf.HI, dilate=0)
    rows = rows.copy()
    rows[4, 4, 6, 0] = np.nan
    rows[7, 2, 5, 3] = np.nan
    dense = _dense(rows, pf.DIMS, 1, occ)
    want = run_march(dense, rays)
    assert 0 < int(torch.isnan(want[1]).sum()) < pf.N_RAYS
    same_bytes(run_march(dense.to_sparse(), rays), want, nan_ok=True)


@pytest.mark.parametrize("dims", [(33, 5, 4), (65, 4, 3)])
def test_sparse_march_where_the_table_has_a_word_more_than_the_grid(rays, dims):
    for degree in (0, 1, 2):
        rows, words = sf.lattice_rows(dims, degree)
        dense = _dense(rows, dims, degree, _occupancy(words, dims))
        want = run_march(dense, rays)
        assert int(want[3].max()) > 0
        same_bytes(run_march(dense.to_sparse(), rays), want)
        same_bytes(run_march(dense.to_sparse(), rays, 0.1, 1e-3, 70), run_march(dense, rays, 0.1, 1e-3, 70))


def test_an_all_clear_occupancy_stores_nothing_and_marches_nothing(rays):
    rows, _ = pf.random_rows(1)
    dense = _dense(rows, pf.DIMS, 1, _occupancy(sf.occupancy_words("clear", pf.DIMS), pf.DIMS))
    sparse = dense.to_sparse()
    assert sparse.n_rows == 0 and sparse.rows.data_ptr() == 0 and sparse.stored_share() == 0.0
    want = run_march(dense, rays)
    got = run_march(sparse, rays)
    same_bytes(got, want)
    assert int(got[3].max()) == 0 and float(got[1].max()) == 0.0


# ---- the pyramid -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("degree", [0, 1, 2])
def test_sparse_pyramid_is_the_dense_pyramid(rays, degree):
    from mipnerf_pl_amd import ops, preview
    made = [r for r, _ in mf.scene_levels(degree, hollow=True)]
    fields = []
    for r, dims in zip(made, mf.LEVEL_DIMS):
        occ = ops.occupancy_grid(torch.from_numpy(r[..., 0].astype(np.float32)).to(DEV), sf.THRESHOLD, pf.LO, pf.HI, dilate=0)
        fields.append(_dense(r, dims, degree, occ))
    dense = preview.BakedPyramid(fields)
    sparse = dense.to_sparse()
    assert sparse.sparse and len(sparse) == 3 and sparse.levels[0].n_rows < 8 * 9 * 10
    # the cells a level keeps are those of the numpy restatement, and more than its own occupied ones somewhere
    words = [f.occupancy.bits.cpu().numpy().view(np.uint32) for f in fields]
    for lv, want in zip(sparse.levels, sf.pyramid_storage_words(words, mf.LEVEL_DIMS)):
        assert lv.stored.bits.cpu().numpy().view(np.uint32).tobytes() == want.tobytes()
    assert any(lv.n_rows > int(preview.baked_points(lv.occupancy).sum()) for lv in sparse.levels)
    radii = torch.from_numpy(mf.scene_radii()).to(DEV)
    for footprint in (mf.FOOTPRINT, 0.0):
        for setting in ((0.5, 0.0, 4096), (0.1, 1e-3, 70)):
            want = run_pyramid(dense, rays, radii, footprint, *setting)
            same_bytes(run_pyramid(sparse, rays, radii, footprint, *setting), want)
    assert float(run_pyramid(dense, rays, radii, mf.FOOTPRINT)[4].max()) > 0.3          # the levels really are mixed
    # L = 1: the plain march's bytes
    one = preview.BakedPyramid([sparse.levels[0].to_dense().to_sparse()])
    want = run_march(fields[0], rays)
    got = run_pyramid(one, rays, radii, mf.FOOTPRINT)
    same_bytes(got[:4], want)
    assert float(got[4].abs().max()) == 0.0
    # render_rays and PreviewFrame dispatch on the kind
    from mipnerf_pl_amd import Rays
    o, d, tn, tf = rays
    n = 256
    bundle = Rays(o[:n].view(16, 16, 3), d[:n].view(16, 16, 3), d[:n].view(16, 16, 3), radii[:n].view(16, 16, 1), torch.ones(16, 16, 1, device=DEV),
                  tn[:n].view(16, 16, 1), tf[:n].view(16, 16, 1))
    for a, b in ((sparse, dense), (sparse.levels[0].to_dense().to_sparse(), fields[0])):
        same_bytes(preview.render_rays(a, bundle, BG), preview.render_rays(b, bundle, BG))
        fa, fb = preview.PreviewFrame(a, 16, 16, BG), preview.PreviewFrame(b, 16, 16, BG)
        same_bytes(fa.render(bundle), fb.render(bundle))
        assert torch.equal(fa.steps, fb.steps)


def test_a_captured_replay_gives_the_bytes_of_the_eager_call(rays):
    from mipnerf_pl_amd import ops, preview
    made = [r for r, _ in mf.scene_levels(1, hollow=True)]
    fields = [_dense(r, dims, 1, ops.occupancy_grid(torch.from_numpy(r[..., 0].astype(np.float32)).to(DEV), sf.THRESHOLD, pf.LO, pf.HI, dilate=0))
              for r, dims in zip(made, mf.LEVEL_DIMS)]
    sparse = preview.BakedPyramid(fields).to_sparse()
    radii = torch.from_numpy(mf.scene_radii()).to(DEV)
    o, d, tn, tf = rays
    eager = [t.clone() for t in run_pyramid(sparse, rays, radii, mf.FOOTPRINT, 0.1, 1e-3, 4096)]
    static = (torch.zeros(pf.N_RAYS, 3, device=DEV), torch.zeros(pf.N_RAYS, device=DEV), torch.zeros(pf.N_RAYS, device=DEV))
    steps, lod = torch.zeros(pf.N_RAYS, dtype=torch.int32, device=DEV), torch.zeros(pf.N_RAYS, device=DEV)
    occ = fields[0].occupancy
    table = torch.zeros_like(sparse.levels[0].table)
    total = torch.zeros(1, dtype=torch.int32, device=DEV)
    from mipnerf_pl_amd import _lib as L
    import ctypes as C
    cdims = (C.c_int32 * 3)(*occ.dims)
    scratch = torch.zeros(max(1, L.preview_sparse_lib().mipnerf_preview_sparse_scratch_bytes(cdims) // 4), dtype=torch.int32, device=DEV)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                             # the index call and the march: neither allocates nor synchronises
        L.preview_sparse_check(L.preview_sparse_lib().mipnerf_preview_sparse_index(
            cdims, occ.bits.data_ptr(), table.data_ptr(), total.data_ptr(), scratch.data_ptr(), torch.cuda.current_stream().cuda_stream))
        preview.march_pyramid(sparse, o, d, radii, tn, tf, BG, mf.FOOTPRINT, 0.1, 1e-3, 4096, out=static, steps=steps, lod=lod)
    for t in static + (steps, lod, table, total):
        t.zero_()
    g.replay()
    torch.cuda.synchronize()
    same_bytes(list(static) + [steps, lod], eager)
    want, m = preview.index_table(occ)
    assert torch.equal(table, want) and int(total) == m


# ---- the bake ----------------------------------------------------------------------------------------------------------------------
def _model(num_samples=16, seed=0):
    from mipnerf_pl_amd import MipNerf
    from oracle import mipnerf_oracle as orc
    model = MipNerf(num_samples=num_samples, precision="fp32")
    model.load_state_dict({"mlp." + k: torch.from_numpy(v.copy()) for k, v in orc.make_params(seed=seed, density_gain=40.0).items()})
    return model.to(DEV).eval()


def _same_field(a, b):
    assert a.dims == b.dims and a.lo == b.lo and a.hi == b.hi and a.degree == b.degree and a.threshold == b.threshold
    assert torch.equal(a.rows.view(torch.int16), b.rows.view(torch.int16)) and torch.equal(a.table, b.table)
    assert torch.equal(a.occupancy.bits.view(torch.int32), b.occupancy.bits.view(torch.int32))
    assert (a.stored is None) == (b.stored is None)
    if a.stored is not None:
        assert torch.equal(a.stored.bits.view(torch.int32), b.stored.bits.view(torch.int32))


def test_sparse_bake_is_the_dense_bake_compacted():
    from mipnerf_pl_amd import ops, preview
    model = _model()
    lo, hi = (-1.0, -1.1, -1.2), (1.1, 1.2, 1.3)
    with torch.no_grad():
        sigma = ops.density_grid(model, (16, 16, 16), lo, hi)
    threshold = float(torch.quantile(sigma.reshape(-1), 0.9))
    how = dict(grid=16, lo=lo, hi=hi, threshold=threshold, dilate=0, precision="fp32")
    for degree in (1, 2):
        dense = preview.bake_field(model, degree=degree, **how)
        sparse = preview.bake_field(model, degree=degree, sparse=True, **how)
        assert isinstance(sparse, preview.SparseField) and 0 < sparse.n_rows < 16 ** 3 and sparse.stored is None
        _same_field(sparse, dense.to_sparse())
        assert abs(sparse.baked_share() - dense.baked_share()) < 1e-6 and sparse.stored_share() == sparse.n_rows / 16.0 ** 3
        assert sparse.dense_nbytes == dense.nbytes and sparse.nbytes < dense.nbytes
    dense = preview.bake_pyramid(model, levels=3, degree=1, **how)
    sparse = preview.bake_pyramid(model, levels=3, degree=1, sparse=True, **how)
    assert sparse.sparse and [b.dims for b in sparse.levels] == [b.dims for b in dense.levels] == [(16,) * 3, (8,) * 3, (4,) * 3]
    for a, b in zip(sparse.levels, dense.to_sparse().levels):
        _same_field(a, b)
    assert sparse.dense_nbytes == dense.nbytes


# ---- the command -------------------------------------------------------------------------------------------------------------------
def _pngs(root):
    out = {}
    for d, _, fs in os.walk(root):
        for f in fs:
            if f.endswith(".png") and f[:5].isdigit():
                with open(os.path.join(d, f), "rb") as fh:
                    out[os.path.relpath(os.path.join(d, f), root)] = fh.read()
    return out


def test_the_command_with_sparse_writes_the_same_pictures(tmp_path, capsys):
    from mipnerf_pl_amd import preview
    from mipnerf_pl_amd.system import DEFAULT_HPARAMS, MipNeRFSystem
    from oracle import mipnerf_oracle as orc
    hp = dict(DEFAULT_HPARAMS)
    hp.update({"nerf.num_samples": 32, "exp_name": "cli", "val.batch_type": "single_image", "dataset_name": "blender"})
    system = MipNeRFSystem(hp, precision="fp32")
    system.load_state_dict({"mip_nerf.mlp." + k: torch.from_numpy(v.copy()) for k, v in orc.make_params(seed=5, density_gain=40.0).items()}, strict=True)
    ckpt = str(tmp_path / "last.ckpt")
    system.save_checkpoint(ckpt)
    common = ["--ckpt", ckpt, "--grid", "24", "--n_poses", "2", "--scale", "1", "--base_size", "16", "16", "--precision", "fp32"]
    tail = r", stored share ([0-9.]+), sparse ([0-9.]+) MiB against ([0-9.]+) MiB dense"
    for i, mip in enumerate(([], ["--mip", "3"])):
        dense = _pngs(preview.main(common + mip + ["--out_dir", str(tmp_path / f"d{i}")]))
        line = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("preview:")][-1]
        assert "stored share" not in line
        folder = preview.main(common + mip + ["--out_dir", str(tmp_path / f"s{i}"), "--sparse", "--save_baked"])
        sline = [ln for ln in capsys.readouterr().out.splitlines() if ln.startswith("preview:") and "saved" not in ln][-1]
        m = re.search(tail + "$", sline)
        assert m, sline
        assert 0.0 < float(m.group(1)) <= 1.0 and float(m.group(2)) > 0.0 and float(m.group(3)) > 0.0
        # the rest of the line is the dense run's, timings and MiB aside
        strip = lambda s: re.sub(r"[0-9.]+ (MiB|ms)", "#", s)
        assert strip(sline[:m.start()]) == strip(line)
        assert len(dense) == 6 and _pngs(folder) == dense
        baked = os.path.join(folder, "baked.npz")
        assert preview.BakedPyramid.stored_sparse(baked) and preview.BakedPyramid.stored_levels(baked) == (3 if mip else None)
        again = preview.main(common + mip + ["--out_dir", str(tmp_path / f"b{i}"), "--sparse", "--baked", baked])
        assert "loaded in" in capsys.readouterr().out and _pngs(again) == dense
        with pytest.raises(SystemExit, match="holds sparse rows"):
            preview.main(common + mip + ["--out_dir", str(tmp_path / f"x{i}"), "--baked", baked])
