"""Float64 restatement of the distorted camera models (TEST INFRASTRUCTURE): COLMAP's forward models, their inverse by Newton's method
run to 60 steps (far past convergence: 8 steps already agree with it to 3e-16), and the ray and radius formulas of the ray generator.
Written from the model definitions, not from csrc/camera_models.hpp or datasets.py; `dtype=np.float32` runs the same arithmetic in
float32 with `steps=8`, which is how the float32 tolerances of the GPU tests were measured (`float32_restatement_error`)."""
import os
import struct

import numpy as np

W, H = 37, 29                                    # 1073 rays: odd, a ragged last block, the last-row rule on 37 pixels
FX, FY = 24.0, 24.5
CX, CY = 0.5 * W + 0.7, 0.5 * H - 0.4
NEAR, FAR = 0.5, 7.0
K = np.array([[FX, 0.0, CX], [0.0, FY, CY], [0.0, 0.0, 1.0]])

# (COLMAP model, record model, the four record coefficients)
PARAM_SETS = (
    ("SIMPLE_RADIAL", "radial", (-0.12, 0.0, 0.0, 0.0)),
    ("SIMPLE_RADIAL", "radial", (0.08, 0.0, 0.0, 0.0)),
    ("RADIAL", "radial", (-0.2, 0.05, 0.0, 0.0)),
    ("OPENCV", "radial", (-0.15, 0.04, 1e-3, -2e-3)),
    ("OPENCV", "radial", (-0.3, 0.1, 2e-3, 1e-3)),
    ("OPENCV_FISHEYE", "fisheye", (-0.03, 0.01, -0.004, 0.001)),
    ("OPENCV_FISHEYE", "fisheye", (0.05, -0.01, 0.002, 0.0)),
)
PARAM_IDS = ["{}{}".format(n, i) for i, (n, _, _) in enumerate(PARAM_SETS)]
STRONG_BARREL = ("SIMPLE_RADIAL", "radial", (-0.9, 0.0, 0.0, 0.0))          # folds back inside the 37x29 image: refused at load time


def c2w():
    """A camera-to-world [3, 4] with a rotation that is no axis permutation, and an off-axis position."""
    a, b, c = 0.4, -0.7, 1.1
    rx = np.array([[1, 0, 0], [0, np.cos(a), -np.sin(a)], [0, np.sin(a), np.cos(a)]])
    ry = np.array([[np.cos(b), 0, np.sin(b)], [0, 1, 0], [-np.sin(b), 0, np.cos(b)]])
    rz = np.array([[np.cos(c), -np.sin(c), 0], [np.sin(c), np.cos(c), 0], [0, 0, 1]])
    return np.concatenate([rz @ ry @ rx, np.array([[0.3], [-1.2], [2.1]])], axis=1)


def pix2cam(k=K):
    """K^-1 with rows 1 and 2 negated, as load_realdata360 builds it."""
    m = np.linalg.inv(k)
    m[1:, :] *= -1
    return m


def distort_radial(k, x, y):
    k1, k2, p1, p2 = k
    r2 = x * x + y * y
    radial = 1 + k1 * r2 + k2 * r2 * r2
    return x * radial + 2 * p1 * x * y + p2 * (r2 + 2 * x * x), y * radial + 2 * p2 * x * y + p1 * (r2 + 2 * y * y)


def undistort_radial(k, xd, yd, steps=60):
    """Newton on distort(x, y) = (xd, yd) with the Jacobian by its four entries, from (xd, yd)."""
    k1, k2, p1, p2 = (xd.dtype.type(v) for v in k)
    x, y = xd.copy(), yd.copy()
    for _ in range(steps):
        fx, fy = distort_radial((k1, k2, p1, p2), x, y)
        r2 = x * x + y * y
        radial = 1 + k1 * r2 + k2 * r2 * r2
        d_radial_dr2 = k1 + 2 * k2 * r2
        a = radial + 2 * x * x * d_radial_dr2 + 2 * p1 * y + 6 * p2 * x            # d fx / d x
        b = 2 * x * y * d_radial_dr2 + 2 * p1 * x + 2 * p2 * y                      # d fx / d y
        c = 2 * x * y * d_radial_dr2 + 2 * p2 * y + 2 * p1 * x                      # d fy / d x
        d = radial + 2 * y * y * d_radial_dr2 + 2 * p2 * x + 6 * p1 * y            # d fy / d y
        det = a * d - b * c
        ex, ey = fx - xd, fy - yd
        x, y = x - (d * ex - b * ey) / det, y - (a * ey - c * ex) / det
    return x, y


def fisheye_theta_d(k, th):
    k1, k2, k3, k4 = k
    return th * (1 + k1 * th ** 2 + k2 * th ** 4 + k3 * th ** 6 + k4 * th ** 8)


def undistort_fisheye(k, thd, steps=60):
    k = tuple(thd.dtype.type(v) for v in k)
    k1, k2, k3, k4 = k
    th = thd.copy()
    for _ in range(steps):
        th = th - (fisheye_theta_d(k, th) - thd) / (1 + 3 * k1 * th ** 2 + 5 * k2 * th ** 4 + 7 * k3 * th ** 6 + 9 * k4 * th ** 8)
    return th


def normalised_points(width=W, height=H, k=K, extra_row=True, dtype=np.float64):
    """(xd, yd) [height (+1), width] of the pixel centres (y down), with one more row below the image for the radii."""
    m = pix2cam(k).astype(dtype)
    ys, xs = np.meshgrid(np.arange(height + (1 if extra_row else 0), dtype=dtype), np.arange(width, dtype=dtype), indexing="ij")
    px, py = xs + dtype(0.5), ys + dtype(0.5)
    c0 = m[0, 0] * px + m[0, 1] * py + m[0, 2]
    c1 = m[1, 0] * px + m[1, 1] * py + m[1, 2]
    return c0, -c1


def camera_directions(model, coeffs, xd, yd, steps=60):
    """Camera-space directions [..., 3] (x right, y up, looking down -z) of the distorted normalised points."""
    one = xd.dtype.type(1)
    if model == "pinhole":
        return np.stack([xd, -yd, -one * np.ones_like(xd)], -1)
    if model == "radial":
        xu, yu = undistort_radial(coeffs, xd, yd, steps)
        return np.stack([xu, -yu, -one * np.ones_like(xu)], -1)
    thd = np.sqrt(xd * xd + yd * yd)
    th = undistort_fisheye(coeffs, thd, steps)
    s = np.where(thd < 1e-8, one, np.sin(th) / np.where(thd < 1e-8, one, thd))
    return np.stack([s * xd, -(s * yd), -np.cos(th)], -1)


def rays(model, coeffs, pose=None, width=W, height=H, k=K, steps=60, dtype=np.float64):
    """dict(directions [H, W, 3], viewdirs [H, W, 3], radii [H, W]) of the distorted camera: direction = R @ camera direction, radius =
    |d(y, x) - d(y + 1, x)| * 2 / sqrt(12) with the last row taken from the row above."""
    pose = (c2w() if pose is None else np.asarray(pose)).astype(dtype)
    xd, yd = normalised_points(width, height, k, extra_row=False, dtype=dtype)
    d = camera_directions(model, coeffs, xd, yd, steps) @ pose[:3, :3].T
    dx = np.sqrt(np.sum((d[:-1] - d[1:]) ** 2, -1))
    dx = np.concatenate([dx, dx[-1:]], 0)
    return dict(directions=d, viewdirs=d / np.linalg.norm(d, axis=-1, keepdims=True), radii=dx * dtype(2) / np.sqrt(dtype(12)))


def project(model, coeffs, d_cam, k=K):
    """Float64 forward model: camera-space directions [..., 3] -> pixel coordinates (x, y), through distort and K."""
    d_cam = np.asarray(d_cam, np.float64)
    if model == "fisheye":
        r = np.sqrt(d_cam[..., 0] ** 2 + d_cam[..., 1] ** 2)
        th = np.arctan2(r, -d_cam[..., 2])
        s = np.where(r < 1e-12, 1.0, fisheye_theta_d(coeffs, th) / np.where(r < 1e-12, 1.0, r))
        xd, yd = s * d_cam[..., 0], -s * d_cam[..., 1]
    else:
        x, y = d_cam[..., 0] / -d_cam[..., 2], -d_cam[..., 1] / -d_cam[..., 2]
        xd, yd = (x, y) if model == "pinhole" else distort_radial(coeffs, x, y)
    return k[0, 0] * xd + k[0, 2], k[1, 1] * yd + k[1, 2]


def float32_restatement_error(model, coeffs):
    """What the float32 restatement (8 steps, float32 numpy) gives against the float64 one at the test shape: (largest absolute
    direction error, largest absolute viewdir error, largest relative radius error)."""
    ref, got = rays(model, coeffs), rays(model, coeffs, steps=8, dtype=np.float32)
    return (float(np.abs(got["directions"] - ref["directions"]).max()), float(np.abs(got["viewdirs"] - ref["viewdirs"]).max()),
            float(np.abs(got["radii"] / ref["radii"] - 1).max()))


# ---- COLMAP files ------------------------------------------------------------------------------------------------------------------
MODEL_IDS = {"SIMPLE_PINHOLE": 0, "PINHOLE": 1, "SIMPLE_RADIAL": 2, "RADIAL": 3, "OPENCV": 4, "OPENCV_FISHEYE": 5, "FULL_OPENCV": 6, "FOV": 7,
             "THIN_PRISM_FISHEYE": 10}


def colmap_params(name, coeffs, k=K):
    """The doubles COLMAP stores for `name` with the intrinsics `k` and the record coefficients `coeffs`."""
    fx, fy, cx, cy = k[0, 0], k[1, 1], k[0, 2], k[1, 2]
    return {"SIMPLE_PINHOLE": (fx, cx, cy), "PINHOLE": (fx, fy, cx, cy), "SIMPLE_RADIAL": (fx, cx, cy, coeffs[0]),
            "RADIAL": (fx, cx, cy, coeffs[0], coeffs[1]), "OPENCV": (fx, fy, cx, cy) + tuple(coeffs),
            "OPENCV_FISHEYE": (fx, fy, cx, cy) + tuple(coeffs)}[name]


def write_cameras_bin(fname, cameras):
    """`cameras`: [(camera_id, model id or name, width, height, params)]"""
    os.makedirs(os.path.dirname(fname), exist_ok=True)
    with open(fname, "wb") as f:
        f.write(struct.pack("<Q", len(cameras)))
        for camera_id, model, width, height, params in cameras:
            f.write(struct.pack("<iiQQ", camera_id, MODEL_IDS.get(model, model), width, height))
            f.write(struct.pack("<" + "d" * len(params), *params))


def write_images_bin(fname, images, points=3):
    """`images`: [(image_id, camera_id, file name)]; every image gets `points` 2D points so that a reader has to skip them."""
    os.makedirs(os.path.dirname(fname), exist_ok=True)
    with open(fname, "wb") as f:
        f.write(struct.pack("<Q", len(images)))
        for image_id, camera_id, name in images:
            f.write(struct.pack("<i", image_id))
            f.write(struct.pack("<7d", 1.0, 0.0, 0.0, 0.0, 0.1 * image_id, 0.2, 0.3))
            f.write(struct.pack("<i", camera_id))
            f.write(name.encode() + b"\x00")
            f.write(struct.pack("<Q", points))
            for j in range(points):
                f.write(struct.pack("<ddq", 1.5 * j, 2.5 * j, -1))


def write_capture(root, cameras, image_cameras=None, n=9, w=16, h=12, seed=3, factor=1, folder=None):
    """A capture as COLMAP leaves it: `n` PNGs of w x h in images/ (or `folder`), poses_bounds.npy, sparse/0/cameras.bin with `cameras`
    and, when `image_cameras` (one camera id per image) is given, sparse/0/images.bin.  Returns the image file names."""
    from PIL import Image
    rng = np.random.RandomState(seed)
    folder = os.path.join(root, folder or "images")
    os.makedirs(folder, exist_ok=True)
    names, rows = [], []
    for i in range(n):
        names.append(f"img_{i:03d}.png")
        Image.fromarray(rng.randint(0, 256, size=(h, w, 3)).astype(np.uint8)).save(os.path.join(folder, names[-1]))
        pos = rng.normal(size=3)
        pos[2] = abs(pos[2]) + 0.3
        pos = (3.0 + rng.rand()) * pos / np.linalg.norm(pos)
        z = pos / np.linalg.norm(pos)
        x = np.cross([0.0, 0.0, 1.0], z)
        x /= np.linalg.norm(x)
        y = np.cross(z, x)
        llff = np.stack([-y, x, z, pos, np.array([h, w, 20.0])], axis=1)                # (down, right, back) | t | hwf
        near = 0.5 + rng.rand()
        rows.append(np.concatenate([llff.reshape(-1), [near, near + 4.0 + 3.0 * rng.rand()]]))
    np.save(os.path.join(root, "poses_bounds.npy"), np.stack(rows))
    write_cameras_bin(os.path.join(root, "sparse", "0", "cameras.bin"), cameras)
    if image_cameras is not None:
        order = rng.permutation(n)                                                      # images.bin is in no particular order
        write_images_bin(os.path.join(root, "sparse", "0", "images.bin"), [(int(i) + 1, image_cameras[i], names[i]) for i in order])
    return names
