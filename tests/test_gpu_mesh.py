"""GPU: geometry out of a trained field (csrc/kernels_mesh.hip, mipnerf_pl_amd/mesh.py).

  - the density lattice against the oracle (integrated_pos_enc -> mlp_forward -> softplus(raw + density_bias)) fed the numpy float32
    restatement of the lattice formulas of include/mipnerf_hip.h;
  - the extraction, exact against tests/isosurface_fixture.py (edge keys, faces with their winding, positions, normals), and from first
    principles on the device's own output (closed, oriented, Euler characteristic, enclosed volume, radial normals);
  - extract_mesh, the PLY file and the command line end to end.

bf16 density bound (the project's rule, tests/gpu_util.py): 2 x the maximum of |sigma - ref| / (1 + |ref|) MEASURED on MI355X per case
against the same oracle values (every run records its figure with gpu_util.record)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import gpu_util as G
import isosurface_fixture as fx
from oracle import mipnerf_oracle as orc

pytestmark = pytest.mark.gpu
DEV = G.DEV
BOX = ((-1.5,) * 3, (1.5,) * 3)

# max |sigma - oracle| / (1 + |oracle|) of the bf16 lattice, measured on MI355X (bf16 results are deterministic for a given build)
MESH_BF16_MEASURED = {
    "trained_40": 1.22e-2,          # the trained field, 40^3 over [-1.5, 1.5]^3; density 0 .. 9.3
    "xavier_17x24x40": 2.71e-2,     # make_params(seed=0, density_gain=40), 17 x 24 x 40 over an off-centre box
}
FP32_BOUND = 2e-5         # what tests/test_gpu_stages.py::test_mlp_fp32 holds the fp32 MLP's density to


def trained_params():
    f = G.load_golden("trained_field")
    return {k[2:]: f[k] for k in f if k.startswith("p_")}


def lattice_means_vars(dims, lo, hi, cov_scale):
    """numpy float32 restatement of the contract: mean = lo + float(i) * h, h = (hi - lo) / float(n - 1), var = cov_scale * h * h / 12"""
    lo32, hi32 = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
    h = (hi32 - lo32) / (np.asarray(dims) - 1).astype(np.float32)
    axes = [lo32[a] + np.arange(dims[a]).astype(np.float32) * h[a] for a in range(3)]
    assert all(a.dtype == np.float32 for a in axes)
    z, y, x = np.meshgrid(axes[2], axes[1], axes[0], indexing="ij")
    means = np.stack([x, y, z], -1).reshape(-1, 3)
    var = np.float32(cov_scale) * h * h / np.float32(12)
    assert var.dtype == np.float32
    return means, np.broadcast_to(var, means.shape).copy()


def oracle_field(params, means, covs, viewdirs=None, **arch):
    """(rgb [M, 3], sigma [M]) of the oracle at given Gaussians; viewdirs None = a zero view encoding"""
    M = means.shape[0]
    out_rgb, out_sigma = [], []
    for s in range(0, M, 16384):
        enc = orc.integrated_pos_enc((means[s:s + 16384], covs[s:s + 16384]), 0, 16)
        venc = np.zeros((enc.shape[0], 27), np.float32) if viewdirs is None else orc.pos_enc(viewdirs[s:s + 16384], 0, 4)
        raw_rgb, raw_density = orc.mlp_forward(params, enc[:, None, :], venc, **arch)
        rgb = orc.sigmoid(raw_rgb[:, 0])
        out_rgb.append((rgb * np.float32(1 + 2 * 0.001) - np.float32(0.001)).astype(np.float32))
        out_sigma.append(orc.softplus(raw_density[:, 0, 0] + np.float32(-1.0)))
    return np.concatenate(out_rgb), np.concatenate(out_sigma)


_CASES = {}


def density_case(name):
    """(model params, dims, lo, hi, oracle sigma [nz, ny, nx]) -- the oracle runs once per session and case"""
    if name not in _CASES:
        if name == "trained_40":
            params, dims, lo, hi = trained_params(), (40, 40, 40), BOX[0], BOX[1]
        else:
            params, dims, lo, hi = orc.make_params(seed=0, density_gain=40.0), (17, 24, 40), (-1.0, -0.5, 0.25), (1.5, 1.0, 2.0)
        means, covs = lattice_means_vars(dims, lo, hi, 1.0)
        _, ref = oracle_field(params, means, covs)
        _CASES[name] = (params, dims, lo, hi, ref.reshape(dims[2], dims[1], dims[0]))
    return _CASES[name]


def rel_err(sigma, ref):
    return float(np.max(np.abs(sigma.astype(np.float64) - ref) / (1 + np.abs(ref))))


@pytest.mark.parametrize("name", ["trained_40", "xavier_17x24x40"])
def test_density_lattice_fp32_against_the_oracle(name):
    from mipnerf_pl_amd import ops
    params, dims, lo, hi, ref = density_case(name)
    if name == "trained_40":
        assert ref.max() > 9.0 and 3.5 < np.quantile(ref, 0.9) < 4.3          # the field the issue describes: 0 .. 9.3, 10 % above 3.9
    model = G.make_model(params, 64, "fp32")
    sigma = ops.density_grid(model, dims, lo, hi, cov_scale=1.0)
    assert sigma.shape == (dims[2], dims[1], dims[0]) and sigma.dtype == torch.float32
    err = rel_err(sigma.cpu().numpy(), ref)
    print(f"density_grid fp32 {name}: {err:.3e}")
    G.record("density_grid fp32 " + name, density_rel=err)
    assert err <= FP32_BOUND
    # a chunk smaller than the lattice that does not divide it: the same bits
    n = dims[0] * dims[1] * dims[2]
    for chunk in (5000, 1100, 77):
        assert n % (chunk - chunk % 256 if chunk > 256 else chunk)
        assert torch.equal(ops.density_grid(model, dims, lo, hi, chunk=chunk), sigma), chunk
    # the model given as its MLP, the precision by name
    assert torch.equal(ops.density_grid(model.mlp, dims, lo, hi, precision="fp32"), sigma)


@pytest.mark.parametrize("name", ["trained_40", "xavier_17x24x40"])
def test_density_lattice_bf16_against_the_oracle(name):
    from mipnerf_pl_amd import ops
    params, dims, lo, hi, ref = density_case(name)
    model = G.make_model(params, 64, "bf16")
    sigma = ops.density_grid(model, dims, lo, hi)
    err = rel_err(sigma.cpu().numpy(), ref)
    print(f"density_grid bf16 {name}: {err:.3e}")
    G.record("density_grid bf16 " + name, density_rel=err)
    for chunk in (5000, 1100):
        assert torch.equal(ops.density_grid(model, dims, lo, hi, chunk=chunk), sigma), chunk
    # one model serves both precisions
    fp32 = ops.density_grid(model, dims, lo, hi, precision="fp32")
    assert rel_err(fp32.cpu().numpy(), ref) <= FP32_BOUND
    assert err <= 2.0 * MESH_BF16_MEASURED[name]


def test_density_lattice_of_a_zero_padded_width():
    """an MLP that runs zero-padded on a wider generated shape goes through the same call, to the same bound"""
    import warnings
    from mipnerf_pl_amd import ops
    dims, lo, hi = (12, 10, 9), (-1.0, -1.0, -1.0), (1.0, 0.5, 1.25)
    params = orc.make_params(seed=3, density_gain=40.0, net_width=200, net_width_condition=72)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                      # "runs zero-padded on the 256 / 128 kernels"
        model = G.make_model(params, 32, "fp32", mlp_net_width=200, mlp_net_width_condition=72)
        sigma = ops.density_grid(model, dims, lo, hi)
    means, covs = lattice_means_vars(dims, lo, hi, 1.0)
    _, ref = oracle_field(params, means, covs)
    err = rel_err(sigma.cpu().numpy().reshape(-1), ref)
    print(f"density_grid fp32 padded 200 / 72: {err:.3e}")
    G.record("density_grid fp32 padded", density_rel=err)
    assert err <= FP32_BOUND
    with pytest.raises(ValueError):
        ops.density_grid(model, (1, 8, 8), lo, hi)
    with pytest.raises(ValueError):
        ops.density_grid(model, dims, lo, hi, cov_scale=-1.0)


@pytest.mark.parametrize("cov_scale", [1.0, 0.0])
def test_lattice_encoding_has_the_bits_of_the_per_point_encoder(cov_scale):
    """k_lattice_ipe shares its device code with k_integrated_pos_enc and the lattice formula is part of the contract: a lattice run equals
    the per-point path on the numpy float32 restatement of the means and variances BIT FOR BIT in fp32 (same encoder, same MLP kernel, a
    zero view encoding).  cov_scale = 0 are point queries: nothing damps sin(2^15 x), which one ulp of a mean would move by 4e-3 x."""
    from mipnerf_pl_amd import ops
    params, dims, lo, hi, _ = density_case("xavier_17x24x40")
    model = G.make_model(params, 64, "fp32")
    means, covs = lattice_means_vars(dims, lo, hi, cov_scale)
    assert covs.any() == (cov_scale > 0)
    enc = ops.integrated_pos_enc((torch.from_numpy(means).to(DEV), torch.from_numpy(covs).to(DEV)), 0, 16)
    with torch.no_grad():
        act = model.mlp(enc.reshape(-1, 1, 96), torch.zeros(enc.shape[0], 27, device=DEV), return_activated=True)[2]
    sigma = ops.density_grid(model, dims, lo, hi, cov_scale=cov_scale)
    assert torch.equal(sigma.reshape(-1), act[:, 0, 3])
    # ... and field_at is that per-point path
    z = torch.zeros(means.shape[0], 3, device=DEV)
    z[:, 2] = 1.0
    got = ops.field_at(model, torch.from_numpy(means).to(DEV), torch.from_numpy(covs).to(DEV), z)
    assert got.shape == (means.shape[0], 4) and torch.equal(got[:, 3], sigma.reshape(-1))


# ---- extraction, exact against the fixture -----------------------------------------------------------------------------------------
def noise_lattice():
    return np.random.default_rng(3).normal(size=(13, 17, 20)).astype(np.float32)


def tie_lattice():
    return np.random.default_rng(4).integers(-3, 4, size=(11, 12, 14)).astype(np.float32)


def non_finite_lattice():
    rng = np.random.default_rng(5)
    g = rng.normal(size=(9, 12, 10)).astype(np.float32)
    g.reshape(-1)[rng.choice(g.size, 90, replace=False)] = np.array([np.nan, np.inf, -np.inf] * 30, np.float32)
    return g


def check_against_fixture(grid, thr, lo, hi, tag):
    from mipnerf_pl_amd import ops
    grid = np.ascontiguousarray(grid, np.float32)
    gd = torch.from_numpy(grid).to(DEV)
    v, nrm, faces, edges = ops.isosurface(gd, thr, lo, hi, return_edges=True)
    again = ops.isosurface(gd, thr, lo, hi, return_edges=True)
    for a, b in zip((v, nrm, faces, edges), again):
        assert torch.equal(a, b) and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes(), tag       # two runs: identical bytes
    assert v.dtype == torch.float32 and nrm.dtype == torch.float32 and faces.dtype == torch.int32 and edges.dtype == torch.int64
    v3 = ops.isosurface(gd, thr, lo, hi)
    assert len(v3) == 3 and torch.equal(v3[0], v) and torch.equal(v3[2], faces)
    v, nrm, faces, edges = v.cpu().numpy(), nrm.cpu().numpy(), faces.cpu().numpy(), edges.cpu().numpy()
    m = fx.marching_tets(grid, thr, lo, hi)
    assert (len(v), len(faces)) == (len(m["vertices"]), len(m["faces"])), tag
    assert np.array_equal(edges, m["edges"]), tag                                           # as sets AND in the documented order
    assert np.array_equal(fx.canonical_faces(faces, edges, grid.size), fx.canonical_faces(m["faces"], m["edges"], grid.size)), tag
    if len(v) == 0:
        return v, nrm, faces, edges
    assert np.isfinite(v).all() and np.isfinite(nrm).all()
    pos_err = float(np.abs(v - m["vertices"]).max())
    pos_bound = 8 * 2.0 ** -23 * float(np.max(np.asarray(hi, np.float64) - np.asarray(lo, np.float64)))
    keep = ~m["weak"]
    assert m["weak"].mean() <= 0.01, tag
    zero_dev, zero_ref = ~nrm.any(1), ~m["normals"].any(1)
    assert np.array_equal(zero_dev[keep], zero_ref[keep]), tag
    sel = keep & ~zero_ref
    cos = (nrm[sel].astype(np.float64) * m["normals"][sel]).sum(1)
    length = np.linalg.norm(nrm[sel].astype(np.float64), axis=1)
    print(f"isosurface {tag}: V {len(v)} F {len(faces)} position error {pos_err:.2e} (bound {pos_bound:.2e}), "
          f"1 - min cosine {1 - cos.min() if len(cos) else 0:.2e}, left out {int(m['weak'].sum())}")
    G.record("isosurface " + tag, position=pos_err, one_minus_cos=1 - cos.min() if len(cos) else 0.0)
    assert pos_err <= pos_bound, tag
    assert len(cos) == 0 or (cos.min() >= 1 - 1e-5 and np.abs(length - 1).max() <= 1e-5), tag
    return v, nrm, faces, edges


@pytest.mark.parametrize("name", ["sphere", "torus", "noise", "ties", "non_finite"])
def test_extraction_matches_the_fixture(name):
    if name == "sphere":
        check_against_fixture(fx.sphere_field(64), 0.0, *BOX, name)
    elif name == "torus":
        check_against_fixture(fx.torus_field(64), 0.0, *BOX, name)
    elif name == "noise":
        v, _, faces, _ = check_against_fixture(noise_lattice(), 0.0, (-1.0,) * 3, (1.0,) * 3, name)
        assert not fx.is_closed(faces) and fx.directed_edges_unique(faces)                  # open at the box
    elif name == "ties":
        v, _, faces, _ = check_against_fixture(tie_lattice(), 1.0, (-1.0, -2.0, 0.0), (1.0, 1.0, 0.5), name)
        assert fx.zero_area_faces(v, faces) > 0 and fx.directed_edges_unique(faces)         # collapsed triangles are kept
    else:
        check_against_fixture(non_finite_lattice(), 0.25, (-1.0,) * 3, (1.0,) * 3, name)


def test_extraction_of_every_sign_pattern_of_a_cell():
    """2 x 2 x 2 lattices: all 16 cases of all six tetrahedra in every combination, each against the fixture"""
    mag = np.random.default_rng(0).uniform(0.5, 2.0, 8)
    from mipnerf_pl_amd import ops
    for pattern in range(256):
        inside = np.array([(pattern >> c) & 1 for c in range(8)], bool)
        f = np.where(inside, mag, -mag).astype(np.float32).reshape(2, 2, 2)
        v, nrm, faces, edges = [t.cpu().numpy() for t in ops.isosurface(torch.from_numpy(f).to(DEV), 0.0, (0.0,) * 3, (1.0, 2.0, 3.0),
                                                                        return_edges=True)]
        m = fx.marching_tets(f, 0.0, (0.0,) * 3, (1.0, 2.0, 3.0))
        assert np.array_equal(edges, m["edges"]), pattern
        assert np.array_equal(fx.canonical_faces(faces, edges, 8), fx.canonical_faces(m["faces"], m["edges"], 8)), pattern
        if len(v):
            assert np.abs(v - m["vertices"]).max() <= 8 * 2.0 ** -23 * 3.0


@pytest.mark.parametrize("const", [-1.0, 1.0])
def test_extraction_of_a_lattice_without_a_surface(const):
    from mipnerf_pl_amd import ops
    out = ops.isosurface(torch.full((5, 6, 7), const, device=DEV), 0.0, *BOX, return_edges=True)
    assert [tuple(t.shape) for t in out] == [(0, 3), (0, 3), (0, 3), (0, 2)]


def test_extraction_of_the_trained_field_matches_the_fixture_and_is_a_closed_surface():
    from mipnerf_pl_amd import ops
    params, dims, lo, hi, ref = density_case("trained_40")
    model = G.make_model(params, 64, "fp32")
    sigma = ops.density_grid(model, dims, lo, hi)
    v, _, faces, _ = check_against_fixture(sigma.cpu().numpy(), 5.0, lo, hi, "trained_40 fp32 at 5")
    assert fx.is_closed(faces) and fx.is_oriented(faces)
    chi = fx.euler_characteristic(len(v), faces)
    print(f"trained field at 5: V {len(v)} F {len(faces)} Euler characteristic {chi} (oracle lattice: 8434, 16852, 8)")
    mo = fx.marching_tets(ref, 5.0, lo, hi)                   # the oracle's lattice: the numbers of the issue
    assert (len(mo["vertices"]), len(mo["faces"]), fx.euler_characteristic(len(mo["vertices"]), mo["faces"])) == (8434, 16852, 8)


# ---- first principles on the device's own output ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,field,volume,chi,vol_err", [("sphere", fx.sphere_field, fx.SPHERE_VOLUME, 2, -0.00210),
                                                           ("torus", fx.torus_field, fx.TORUS_VOLUME, 0, -0.00826)])
def test_analytic_surfaces_from_first_principles(name, field, volume, chi, vol_err):
    from mipnerf_pl_amd import ops
    v, nrm, faces = [t.cpu().numpy() for t in ops.isosurface(torch.from_numpy(field(64)).to(DEV), 0.0, *BOX)]
    assert fx.is_closed(faces) and fx.is_oriented(faces)
    assert fx.euler_characteristic(len(v), faces) == chi
    err = fx.enclosed_volume(v, faces) / volume - 1
    print(f"{name} 64^3: volume error {err:.5f}")
    assert abs(err - vol_err) <= 1e-4
    if name == "sphere":
        r = v.astype(np.float64) - fx.CENTRE
        cos = (r / np.linalg.norm(r, axis=1)[:, None] * nrm).sum(1)          # central differences are exact for a quadratic
        print(f"sphere normals: 1 - min cosine {1 - cos.min():.2e}")
        assert cos.min() >= 1 - 1e-5


def test_large_sphere_across_workgroup_boundaries():
    """256^3: 65536 workgroups of the scans; a broken block base shows as an open or misoriented surface"""
    from mipnerf_pl_amd import ops
    g = torch.linspace(-1.5, 1.5, 256, dtype=torch.float64, device=DEV)
    z, y, x = torch.meshgrid(g, g, g, indexing="ij")
    f = (fx.SPHERE_R ** 2 - ((x - fx.CENTRE[0]) ** 2 + (y - fx.CENTRE[1]) ** 2 + (z - fx.CENTRE[2]) ** 2)).float()
    del x, y, z
    v, nrm, faces, edges = [t.cpu().numpy() for t in ops.isosurface(f, 0.0, *BOX, return_edges=True)]
    assert fx.is_closed(faces) and fx.is_oriented(faces) and fx.euler_characteristic(len(v), faces) == 2
    err = fx.enclosed_volume(v, faces) / fx.SPHERE_VOLUME - 1
    print(f"sphere 256^3: V {len(v)} F {len(faces)} volume error {err:.2e} (second-order convergence predicts -1.3e-4)")
    assert abs(err) < 0.0021
    key = edges.min(1) * f.numel() + edges.max(1)
    assert (np.diff(key) > 0).all()                                          # sorted by (smaller end, larger end), no vertex twice
    fl = f.reshape(-1)[torch.from_numpy(edges).to(DEV)].cpu().numpy()
    assert (fl[:, 0] > 0).all() and (fl[:, 1] <= 0).all()


def test_lattices_past_32_bit_indices_are_refused():
    from mipnerf_pl_amd import _lib as L
    nv, nf = C.c_int64(), C.c_int64()
    with pytest.raises(ValueError, match="2\\^31"):
        L.check(L.lib().mipnerf_isosurface_count((C.c_int32 * 3)(675, 675, 675), None, 0.0, None, 0, C.byref(nv), C.byref(nf), None))
    assert L.lib().mipnerf_isosurface_workspace_bytes(512, 512, 512) > 0     # 512^3 must work


# ---- end to end ------------------------------------------------------------------------------------------------------------------------
def _system(params, precision="fp32"):
    from mipnerf_pl_amd.system import DEFAULT_HPARAMS, MipNeRFSystem
    hp = dict(DEFAULT_HPARAMS)
    hp.update({"nerf.num_samples": 32, "exp_name": "exp", "val.batch_type": "single_image"})
    system = MipNeRFSystem(hp, precision=precision)
    missing, unexpected = system.load_state_dict({"mip_nerf.mlp." + k: torch.from_numpy(v.copy()) for k, v in params.items()}, strict=True)
    assert not missing and not unexpected
    return system.to(DEV).eval()


def test_extract_mesh_end_to_end_fp32(tmp_path):
    from mipnerf_pl_amd import ops
    from mipnerf_pl_amd.mesh import extract_mesh, lattice_variance, read_ply, write_ply
    params = trained_params()
    system = _system(params)
    dims = (48, 48, 48)
    mesh = extract_mesh(system, grid=48, lo=BOX[0], hi=BOX[1], threshold=5.0, precision="fp32")
    sigma = ops.density_grid(system, dims, *BOX, precision="fp32")
    v, nrm, faces = ops.isosurface(sigma, 5.0, *BOX)
    assert torch.equal(mesh.sigma, sigma) and torch.equal(mesh.vertices, v) and torch.equal(mesh.normals, nrm) and torch.equal(mesh.faces, faces)
    assert len(v) > 1000 and mesh.colors.dtype == torch.uint8 and mesh.colors.shape == v.shape
    # the colours: the oracle at the device's vertex positions and normals
    vn, nn = v.cpu().numpy(), nrm.cpu().numpy()
    var = np.broadcast_to(lattice_variance(dims, *BOX, 1.0), vn.shape).copy()
    want, _ = oracle_field(params, vn, var, viewdirs=-nn)
    err = G.maxdiff(mesh.rgb, want)
    print(f"vertex colours fp32: {err:.2e}")
    G.record("extract_mesh fp32 rgb", rgb=err)
    assert err <= G.TOL_FP32["rgb"]
    path = write_ply(str(tmp_path / "m.ply"), mesh.vertices, mesh.normals, mesh.faces, mesh.colors)
    rv, rn, rf, rc = read_ply(path)
    assert np.array_equal(rv, vn) and np.array_equal(rn, nn) and np.array_equal(rf, faces.cpu().numpy())
    want_u8 = (np.clip(want, 0, 1) * np.float32(255) + np.float32(0.5)).astype(np.uint8)
    assert np.abs(rc.astype(int) - want_u8.astype(int)).max() <= 1
    # no colours asked for: none computed
    bare = extract_mesh(system, grid=dims, lo=BOX[0], hi=BOX[1], threshold=5.0, precision="fp32", color=False)
    assert bare.colors is None and bare.rgb is None and torch.equal(bare.faces, faces)


def test_extract_mesh_bf16_against_the_fixture_on_its_own_lattice():
    from mipnerf_pl_amd.mesh import extract_mesh
    system = _system(trained_params(), precision="bf16")
    mesh = extract_mesh(system, grid=(40, 36, 32), lo=BOX[0], hi=BOX[1], threshold=5.0)
    m = fx.marching_tets(mesh.sigma.cpu().numpy(), 5.0, *BOX)
    assert (len(mesh.vertices), len(mesh.faces)) == (len(m["vertices"]), len(m["faces"])) and len(m["vertices"]) > 1000
    from mipnerf_pl_amd import ops
    edges = ops.isosurface(mesh.sigma, 5.0, *BOX, return_edges=True)[3].cpu().numpy()
    assert np.array_equal(edges, m["edges"])
    n = mesh.sigma.numel()
    assert np.array_equal(fx.canonical_faces(mesh.faces.cpu().numpy(), edges, n), fx.canonical_faces(m["faces"], m["edges"], n))
    assert np.abs(mesh.vertices.cpu().numpy() - m["vertices"]).max() <= 8 * 2.0 ** -23 * 3.0
    assert mesh.colors.shape == mesh.vertices.shape and torch.isfinite(mesh.rgb).all()


def test_command_line_end_to_end(tmp_path, capsys):
    from mipnerf_pl_amd import extract_mesh as cli
    from mipnerf_pl_amd.mesh import extract_mesh, read_ply
    system = _system(trained_params())
    system.hparams.update({"dataset_name": "blender", "exp_name": "cli"})
    ckpt = str(tmp_path / "last.ckpt")
    system.save_checkpoint(ckpt)
    out = str(tmp_path / "out")
    path = cli.main(["--ckpt", ckpt, "--out_dir", out, "--grid", "30", "28", "26", "--threshold", "5", "--precision", "fp32", "--save_density"])
    assert path == os.path.join(out, "mesh", "cli", "mesh_30x28x26.ply") and os.path.exists(path)
    mesh = extract_mesh(system, grid=(30, 28, 26), lo=BOX[0], hi=BOX[1], threshold=5.0, precision="fp32")
    rv, rn, rf, rc = read_ply(path)
    assert len(rv) > 300
    assert np.array_equal(rv, mesh.vertices.cpu().numpy()) and np.array_equal(rn, mesh.normals.cpu().numpy())
    assert np.array_equal(rf, mesh.faces.cpu().numpy()) and np.array_equal(rc, mesh.colors.cpu().numpy())
    vol = np.load(os.path.join(out, "mesh", "cli", "density_30x28x26.npy"))
    assert vol.shape == (26, 28, 30) and np.array_equal(vol, mesh.sigma.cpu().numpy())
    line = capsys.readouterr().out.splitlines()[-1]
    inside = 100.0 * float((vol > 5.0).mean())
    assert line == f"{path}: {len(rv)} vertices, {len(rf)} faces, {inside:.2f} % of the lattice points inside (density > 5)"
    # --bound against --aabb, and --no_color drops the three colour properties
    path2 = cli.main(["--ckpt", ckpt, "--out_dir", str(tmp_path / "out2"), "--grid", "30", "28", "26", "--threshold", "5", "--precision", "fp32",
                      "--aabb", "-1.5", "-1.5", "-1.5", "1.5", "1.5", "1.5", "--no_color"])
    rv2, rn2, rf2, rc2 = read_ply(path2)
    assert rc2 is None and np.array_equal(rv2, rv) and np.array_equal(rf2, rf)
    assert b"property uchar red" not in open(path2, "rb").read(400) and b"property uchar red" in open(path, "rb").read(400)
    assert not os.path.exists(os.path.join(str(tmp_path / "out2"), "mesh", "cli", "density_30x28x26.npy"))


def test_unbounded_models_are_refused():
    from mipnerf_pl_amd import MipNerf, ops
    from mipnerf_pl_amd.mesh import extract_mesh
    model = MipNerf(num_samples=16, unbounded=True).to(DEV)
    with pytest.raises(NotImplementedError):
        extract_mesh(model, grid=8)
    with pytest.raises(NotImplementedError):
        ops.density_grid(model.mlp, (8, 8, 8), *BOX)
    # ... and by the C entry point itself
    from mipnerf_pl_amd import _lib as L
    ctx = model.mlp.native(torch.device(DEV))
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=DEV)
    out = torch.empty(8, 8, 8, device=DEV)
    f3 = C.c_float * 3
    with pytest.raises(NotImplementedError):
        L.check(L.lib().mipnerf_density_grid(ctx.handle, (C.c_int32 * 3)(8, 8, 8), f3(-1, -1, -1), f3(1, 1, 1), 1.0, L.PREC_FP32,
                                             out.data_ptr(), ws.data_ptr(), ws.numel(), None))
