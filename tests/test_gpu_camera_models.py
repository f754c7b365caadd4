"""GPU: camera record modes 2 (radial-tangential) and 3 (equidistant fisheye) of the ray generator against the float64 restatement
(camera_models_fixture.py: COLMAP's forward models inverted by 60 Newton steps).

Common shape: a 37 x 29 image (1073 rays: odd, a ragged last block of the 256-thread launch, the last-row rule of the radii on 37 pixels),
fx = 24, fy = 24.5, principal point off-centre by (+0.7, -0.4), a rotation that is no axis permutation, and the seven parameter sets of
`camera_models_fixture.PARAM_SETS`.  The references are computed once per parameter set and shared."""
import functools

import numpy as np
import pytest
import torch

import camera_models_fixture as cm

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
CASES = range(len(cm.PARAM_SETS))

# float32 table: absolute bound on directions and viewdirs.  The float32 numpy restatement (8 steps) measures 1.4e-7 .. 2.5e-7 on the
# directions and 1.3e-7 .. 2.0e-7 on the viewdirs over the seven sets at this shape; 1e-6 leaves room for another summation order in the
# rotation and the normalisation.
DIR_TOL_F32 = 1e-6
# float32 table: relative bound on the radii = 4 x what the float32 numpy restatement (not the kernel) gives at this shape, per set:
#   SIMPLE_RADIAL -0.12: 3.63e-6   SIMPLE_RADIAL +0.08: 3.57e-6   RADIAL: 3.23e-6   OPENCV (-0.15, ..): 3.28e-6
#   OPENCV (-0.3, ..): 3.69e-6     FISHEYE (-0.03, ..): 3.74e-6   FISHEYE (0.05, ..): 4.72e-6
# (a radius is the norm of a difference of neighbouring directions, 4e-2 of their size here, so it keeps 1/25 of their relative accuracy)
RADII_FACTOR_F32 = 4.0


@functools.lru_cache(maxsize=None)
def reference(case):
    _, model, coeffs = cm.PARAM_SETS[case]
    ref = cm.rays(model, coeffs)
    ref["radii_f32_measured"] = cm.float32_restatement_error(model, coeffs)[2]
    return ref


def record(model, coeffs, dtype=torch.float32, pose=None, near=cm.NEAR, far=cm.FAR):
    from mipnerf_pl_amd import ops
    kw = {} if model == "pinhole" else dict(model=model, distortion=coeffs)
    return ops.camera_record(cm.c2w() if pose is None else pose, cm.W, cm.H, near, far, pix2cam=cm.pix2cam(), dtype=dtype, **kw)


def frame(rec):
    from mipnerf_pl_amd import ops
    rays = ops.generate_rays(rec.reshape(1, 32).to(DEV))
    torch.cuda.synchronize()
    return rays


def _np(t):
    return t.detach().cpu().numpy().astype(np.float64)


# ---- 1. the tables against the restatement ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=cm.PARAM_IDS)
def test_float32_table_against_the_restatement(case):
    _, model, coeffs = cm.PARAM_SETS[case]
    ref = reference(case)
    rays = frame(record(model, coeffs))
    d, v, r = _np(rays.directions).reshape(cm.H, cm.W, 3), _np(rays.viewdirs).reshape(cm.H, cm.W, 3), _np(rays.radii).reshape(cm.H, cm.W)
    e_d, e_v = np.abs(d - ref["directions"]).max(), np.abs(v - ref["viewdirs"]).max()
    e_r = np.abs(r / ref["radii"] - 1).max()
    tol_r = RADII_FACTOR_F32 * ref["radii_f32_measured"]
    print(f"{cm.PARAM_IDS[case]}: directions {e_d:.3e} viewdirs {e_v:.3e} (bound {DIR_TOL_F32:g}); radii rel {e_r:.3e} (bound {tol_r:.3e})")
    assert np.isfinite(d).all() and np.isfinite(v).all() and np.isfinite(r).all()
    assert e_d <= DIR_TOL_F32 and e_v <= DIR_TOL_F32
    assert e_r <= tol_r
    pose = cm.c2w().astype(np.float32)
    assert np.array_equal(_np(rays.origins), np.broadcast_to(pose[:, 3].astype(np.float64), (cm.W * cm.H, 3)))
    assert bool((rays.near == cm.NEAR).all()) and bool((rays.far == cm.FAR).all()) and bool((rays.lossmult == 1.0).all())


@pytest.mark.parametrize("case", CASES, ids=cm.PARAM_IDS)
def test_float64_table_against_the_restatement(case):
    """Float64 arithmetic agrees with the restatement to 1e-12 relative before the final rounding, so every float32 output is the float32
    rounding of the restatement or its neighbour."""
    _, model, coeffs = cm.PARAM_SETS[case]
    ref = reference(case)
    rays = frame(record(model, coeffs, dtype=torch.float64))
    for name, got in (("directions", rays.directions.reshape(cm.H, cm.W, 3)), ("viewdirs", rays.viewdirs.reshape(cm.H, cm.W, 3)),
                      ("radii", rays.radii.reshape(cm.H, cm.W))):
        want32 = ref[name].astype(np.float32)
        ulps = np.abs(_np(got) - want32.astype(np.float64)) / np.spacing(np.abs(want32)).astype(np.float64)
        print(f"{cm.PARAM_IDS[case]} {name}: max distance from the rounded restatement {ulps.max():.2f} ulp")
        assert ulps.max() <= 1.0, name


# ---- 2. zero coefficients are the pinhole ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_radial_with_zero_coefficients_equals_the_pinhole(dtype):
    a, b = frame(record("pinhole", None, dtype)), frame(record("radial", (0.0, 0.0, 0.0, 0.0), dtype))
    for k in a._fields:
        assert torch.equal(getattr(a, k), getattr(b, k)), k


# ---- 3. round trip through the forward model -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=cm.PARAM_IDS)
def test_directions_project_back_onto_their_pixels(case):
    """Derived bound: 1.8e-7 (float32 solve) x f = 24 is 4e-6 px; 1e-4 px asked."""
    _, model, coeffs = cm.PARAM_SETS[case]
    rays = frame(record(model, coeffs))
    rot32 = cm.c2w()[:, :3].astype(np.float32).astype(np.float64)                   # the rotation the float32 table holds
    d_cam = _np(rays.directions) @ np.linalg.inv(rot32).T
    px, py = cm.project(model, coeffs, d_cam)
    ys, xs = np.divmod(np.arange(cm.W * cm.H), cm.W)
    err = max(np.abs(px - (xs + 0.5)).max(), np.abs(py - (ys + 0.5)).max())
    print(f"{cm.PARAM_IDS[case]}: largest reprojection error {err:.3e} px")
    assert err <= 1e-4


# ---- 4. the in-graph batch producer writes the same bits -------------------------------------------------------------------------------
def test_gather_train_batch_equals_generate_rays_on_mixed_modes():
    from mipnerf_pl_amd import ops
    from mipnerf_pl_amd.rays import Rays
    pose2 = cm.c2w().copy()
    pose2[:, 3] = [-0.4, 0.9, 1.5]
    blender = ops.camera_record(cm.c2w(), 12, 10, 2.0, 6.0, focal=11.0, lossmult=4.0)
    table = torch.stack([blender, record("pinhole", None), record(*cm.PARAM_SETS[4][1:]), record(*cm.PARAM_SETS[5][1:], pose=pose2, near=0.3),
                         record(*cm.PARAM_SETS[0][1:], pose=pose2, far=9.0)]).to(DEV)
    assert table[:, 26].tolist() == [0.0, 1.0, 2.0, 3.0, 2.0]
    sizes = [120] + [cm.W * cm.H] * 4
    offsets = torch.tensor(np.concatenate([[0], np.cumsum(sizes)]), dtype=torch.int64, device=DEV)
    P = int(offsets[-1])
    g = torch.Generator().manual_seed(11)
    pixels = torch.rand(P, 3, generator=g).to(DEV)
    # the first 600 ids go round the five cameras pixel by pixel, so every wavefront holds all four modes; the rest is a permutation
    head = torch.stack([offsets[c] + torch.arange(120, device=DEV) for c in range(5)], 1).reshape(-1)
    rest = torch.randperm(P, generator=g).to(DEV)
    taken = torch.zeros(P, dtype=torch.bool, device=DEV)
    taken[head] = True
    order = torch.cat([head, rest[~taken[rest]]]).contiguous()
    assert order.numel() == P and int(order.unique().numel()) == P
    B = 300
    nb = (P + B - 1) // B
    assert P % B and B % 64 and B % 256
    rays = Rays(*[torch.empty(B, k, device=DEV) for k in (3, 3, 3, 1, 1, 1, 1)])
    gt = torch.empty(B, 3, device=DEV)
    step = torch.zeros(1, dtype=torch.int64, device=DEV)
    base = torch.zeros(1, dtype=torch.int64, device=DEV)
    for b in range(nb):
        for t in list(rays) + [gt]:
            t.fill_(-7.0)
        step.fill_(b)
        ops.gather_train_batch(order, offsets, table, pixels, step, base, rays, gt)
        ids = order[b * B:(b + 1) * B]
        n = ids.numel()
        cam = torch.searchsorted(offsets, ids, right=True) - 1
        want = ops.generate_rays(table, cam_idx=cam, pix_idx=ids - offsets[cam])
        if b == 0:
            assert sorted(set(table[cam[:64], 26].tolist())) == [0.0, 1.0, 2.0, 3.0]
        for k in Rays._fields:
            assert torch.equal(getattr(rays, k)[:n], getattr(want, k)), (b, k)
            assert bool((getattr(rays, k)[n:] == -7.0).all()), (b, k)
        assert torch.equal(gt[:n], pixels[ids]) and bool((gt[n:] == -7.0).all())
    assert n == P - (nb - 1) * B and n < B                                    # the last batch was short


# ---- 5. a capture as COLMAP leaves it --------------------------------------------------------------------------------------------------
def test_capture_with_distorted_cameras(tmp_path):
    from mipnerf_pl_amd import ops
    from mipnerf_pl_amd.datasets import RealData360
    radial = (1, "SIMPLE_RADIAL", 16, 12, (20.0, 8.2, 5.9, -0.12))
    fisheye = (2, "OPENCV_FISHEYE", 16, 12, (19.0, 19.5, 7.9, 6.1, 0.05, -0.01, 0.002, 0.0))
    one = str(tmp_path / "one")
    cm.write_capture(one, [radial])
    two = str(tmp_path / "two")
    ids = [1, 2, 2, 1, 2, 1, 1, 2, 1]
    cm.write_capture(two, [radial, fisheye], image_cameras=ids)
    for root, modes in ((one, [2.0] * 7), (two, [3.0 if ids[i] == 2 else 2.0 for i in range(1, 8)])):
        ds = RealData360(root, "train", factor=1, device=DEV)
        assert ds.cameras.shape == (7, 32) and ds.cameras[:, 26].tolist() == modes
        assert ds.num_pixels == 7 * 16 * 12
        g = torch.Generator().manual_seed(5)
        pick = torch.randperm(ds.num_pixels, generator=g)[:500].to(DEV)
        rays, pix = ds.rays_at(pick)
        cam = torch.div(pick, 16 * 12, rounding_mode="floor")
        want = ops.generate_rays(ds.cameras.to(DEV), cam_idx=cam, pix_idx=pick - cam * 16 * 12)
        for k in rays._fields:
            assert torch.equal(getattr(rays, k), getattr(want, k)), k
        # and the rays are the distorted camera's: image 0 of the split against the restatement with this camera's K
        K, model = ds.Ks[0], ("radial" if modes[0] == 2.0 else "fisheye")
        ref = cm.rays(model, tuple(ds.distortion[0]), pose=ds.camtoworlds[0], width=16, height=12, k=K)
        got = ds.image_rays(0)[0]
        assert np.abs(_np(got.directions) - ref["directions"]).max() <= 1e-6
        if model == "radial":       # not what a pinhole record of the same K gives
            pin = ops.generate_rays(ops.camera_record(ds.camtoworlds[0], 16, 12, 1.0, 2.0, pix2cam=ds.K_inv).reshape(1, 32).to(DEV))
            assert float((got.directions.reshape(-1, 3) - pin.directions).abs().max()) > 1e-3
        assert torch.equal(pix, ds._need_device()["pixels"][pick])


# ---- 6. cull defaults ------------------------------------------------------------------------------------------------------------------
def test_cull_defaults_of_distorted_and_pinhole_frames():
    from mipnerf_pl_amd.evaluate import corner_ray_bound, corner_ray_radius, cull_box, cull_far_radius
    from mipnerf_pl_amd.rays import Rays
    grid = 32
    _, model, coeffs = cm.PARAM_SETS[4]
    ref = reference(4)
    flat = frame(record(model, coeffs))
    rays = Rays(*[t.reshape(cm.H, cm.W, -1) for t in flat])
    origin = cm.c2w()[:, 3]
    ends = [origin + t * ref["directions"] for t in (cm.NEAR, cm.FAR)]
    brute_bound = max(np.abs(e).max() for e in ends)
    brute_radius = max(np.linalg.norm(e, axis=-1).max() for e in ends)
    assert cull_box([rays], grid, distorted=True) >= brute_bound
    assert cull_far_radius([rays], grid, distorted=[True]) >= brute_radius
    assert corner_ray_bound([rays], True) >= brute_bound * (1 - 1e-6) and corner_ray_radius([rays], True) >= brute_radius * (1 - 1e-6)
    pin = Rays(*[t.reshape(cm.H, cm.W, -1) for t in frame(record("pinhole", None))])
    corner_bound = corner_radius = 0.0                                                  # the corner rule, restated
    for y in (0, cm.H - 1):
        for x in (0, cm.W - 1):
            for t in (pin.near[y, x], pin.far[y, x]):
                p = pin.origins[y, x] + t * pin.directions[y, x]
                corner_bound, corner_radius = max(corner_bound, float(p.abs().max())), max(corner_radius, float(p.double().norm()))
    assert cull_box([pin], grid) == corner_bound * (grid - 1) / (grid - 3) == cull_box([pin], grid, distorted=[False])
    assert cull_far_radius([pin], grid) == corner_radius * (grid - 1) / (grid - 3) == cull_far_radius([pin], grid, distorted=False)
