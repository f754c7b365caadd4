"""Device-resident datasets: the reference's on-disk formats feeding the device-side ray generator.

The reference (datasets/datasets.py) expands every pixel of every image into a 52-byte `Rays` row on the host at start-up
(64 M rays = 3.3 GB for lego) and pays a host gather + H2D copy per batch.  Here a dataset is: the images as one flat
`[P, 3]` fp32 device tensor, a camera table `[n_images, 32]` (`ops.camera_record`), and pixel offsets; a batch is drawn as
pixel ids ON the device and its rays come out of `k_generate_rays` (`ops.generate_rays`) -- nothing per-ray ever lives on
the host.  Same class names, constructor arguments, file formats, `__len__` / `__getitem__` meaning and `dataset_dict`
keys as the reference, so `MipNeRFSystem.setup` / `eval.py` read the same directories:

    Blender      `transforms_{split}.json` + RGBA PNGs, white-background compositing        datasets.py:171-263
    Multicam     `metadata.json` of convert_blender_data.py (pix2cam / cam2world / lossmult)  datasets.py:84-168
    RealData360  LLFF `poses_bounds.npy` + `images[_f]/` + COLMAP `sparse/0/cameras.bin`    datasets.py:266-474
                 (upstream never registers it; here it is `dataset_dict['llff']`); a capture with `images/` only is shrunk by
                 `factor` on the device at start-up (`ops.area_downscale`)
    RenderGen    the spherical render path of render_video.py:19-118 as a camera table
    PathGen      the interpolated path of utils/vis.py:92-121 (`gen_render_path`) through the poses of a RealData360 split

File parsing and pose algebra are host numpy (they run once); the per-ray arithmetic is the HIP kernel's.
"""
import json
import os
import struct

import numpy as np
import torch

from . import ops
from .rays import Rays, Rays_keys


# ---------------------------------------------------------------------------------------------------------------------
# host side: files -> (images, camera records)
# ---------------------------------------------------------------------------------------------------------------------
def _read_image(fname):
    from PIL import Image
    with open(fname, "rb") as f:
        return np.array(Image.open(f), dtype=np.float32) / 255.0


def _composite(image, white_bkgd):
    """datasets.py:108-110 / 201-203: RGBA over white when `white_bkgd`, then drop alpha."""
    if white_bkgd:
        image = image[..., :3] * image[..., -1:] + (1.0 - image[..., -1:])
    return np.ascontiguousarray(image[..., :3], dtype=np.float32)


def _halve(image):
    """`cv2.resize(image, (w//2, h//2), interpolation=cv2.INTER_AREA)` of datasets.py:193-196 for an exact factor 2: the mean of
    each 2x2 block (what INTER_AREA computes when the scale is integral)."""
    h2, w2 = image.shape[0] // 2, image.shape[1] // 2
    v = image[:h2 * 2, :w2 * 2].reshape(h2, 2, w2, 2, -1)
    return v.mean(axis=(1, 3), dtype=np.float32)


def load_blender(data_dir, split, white_bkgd=True, factor=0):
    """datasets.py:183-212.  Returns (images, records): `transform_matrix` is camera-to-world, focal from `camera_angle_x`."""
    with open(os.path.join(data_dir, f"transforms_{split}.json")) as fp:
        meta = json.load(fp)
    images, c2ws = [], []
    for frame in meta["frames"]:
        image = _read_image(os.path.join(data_dir, frame["file_path"] + ".png"))
        if factor == 2:
            image = _halve(image)
        elif factor > 0:
            raise ValueError(f"Blender dataset only supports factor=0 or 2, {factor} set.")
        images.append(_composite(image, white_bkgd))
        c2ws.append(np.array(frame["transform_matrix"], dtype=np.float32))
    h, w = images[0].shape[:2]
    focal = 0.5 * w / np.tan(0.5 * float(meta["camera_angle_x"]))
    records = [ops.camera_record(c2w, w, h, 2.0, 6.0, focal=focal) for c2w in c2ws]
    return images, records, dict(h=h, w=w, focal=focal, camtoworlds=c2ws)


def load_multicam(data_dir, split, white_bkgd=True):
    """datasets.py:98-113 + the per-image attributes `_generate_rays` broadcasts (:116-168)."""
    with open(os.path.join(data_dir, "metadata.json")) as fp:
        meta = json.load(fp)[split]
    meta = {k: np.array(meta[k]) for k in meta}
    images = [_composite(_read_image(os.path.join(data_dir, rel)), white_bkgd) for rel in meta["file_path"]]
    return images, _multicam_records(meta), dict(meta=meta)


def _multicam_records(meta):
    return [ops.camera_record(meta["cam2world"][i].astype(np.float32), float(meta["width"][i]), float(meta["height"][i]),
                              float(meta["near"][i]), float(meta["far"][i]),
                              pix2cam=meta["pix2cam"][i].astype(np.float32), lossmult=float(meta["lossmult"][i]))
            for i in range(len(meta["file_path"]))]


def load_multicam_from_blender(data_dir, split, white_bkgd=True, n_down=4, device=None):
    """The data set `load_multicam` reads from a converted directory, built from the Blender directory itself: the camera table from
    the converter's float64 metadata arithmetic (convert_blender_data.split_metadata), the pixel rows [P, 3] from the pyramid kernel
    (`ops.box_pyramid`: the values the written PNGs would decode and composite to) directly on `device`.  No PNG is written or re-read.
    Returns (pixels, records, info) with info['sizes'] = the (height, width) of every image."""
    from . import convert_blender_data as conv
    if device is None:
        raise RuntimeError("datasets: the multi-scale pyramid is made by the HIP kernel; need a HIP device (there is no host fallback)")
    device = torch.device(device)
    files, cams, angle = conv.read_transforms(data_dir, split)
    h, w = conv.check_frames(files, n_down)
    meta = conv.split_metadata(split, cams, h, w, angle, n_down)
    meta = {k: np.array(meta[k]) for k in meta}
    sizes = [(int(a), int(b)) for a, b in zip(meta["height"], meta["width"])]
    ppi = sum(a * b for a, b in sizes[:n_down])
    pixels = torch.empty(len(files) * ppi, 3, dtype=torch.float32, device=device)
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(conv.MAX_WORKERS) as pool, torch.cuda.device(device):
        for lo, frames in conv.frame_batches(files, h, w, pool):
            ops.box_pyramid(torch.from_numpy(frames).to(device), n_down, white_bkgd=bool(white_bkgd), out_rgb=pixels, rgb_row_offset=lo * ppi)
    return pixels, _multicam_records(meta), dict(meta=meta, sizes=sizes)


def _unit(v):
    return v / np.linalg.norm(v)


def _look_at(z, up, pos):
    """[x | y | z | pos] with z along `z`, x = up x z, y = z x x (datasets.py:432-439)."""
    z = _unit(z)
    x = _unit(np.cross(up, z))
    y = _unit(np.cross(z, x))
    return np.stack([x, y, z, pos], axis=1)


def _to44(p34):
    bottom = np.broadcast_to(np.array([0.0, 0.0, 0.0, 1.0], dtype=p34.dtype), p34.shape[:-2] + (1, 4))
    return np.concatenate([p34, bottom], axis=-2)


def recenter_poses(poses):
    """datasets.py:379-390: express every pose in the frame of the average pose (mean position, summed z and y axes)."""
    avg = _look_at(poses[:, :3, 2].sum(0), poses[:, :3, 1].sum(0), poses[:, :3, 3].mean(0))
    out = poses.copy()
    out[:, :3, :4] = (np.linalg.inv(_to44(avg.astype(np.float64))) @ _to44(poses[:, :3, :4].astype(np.float64)))[:, :3, :4]
    return out


def spherify_poses(poses):
    """datasets.py:445-474: move the origin to the point closest to all optical axes and make `up` = mean offset of the camera
    centres from it (the third axis of the new frame), with the fixed helper vector (.1, .2, .3) fixing the in-plane rotation."""
    d = poses[:, :3, 2:3]
    o = poses[:, :3, 3:4]
    a = np.eye(3) - d * np.transpose(d, [0, 2, 1])                   # projector orthogonal to each axis
    b = -a @ o
    center = np.squeeze(-np.linalg.inv((np.transpose(a, [0, 2, 1]) @ a).mean(0)) @ b.mean(0))
    v0 = _unit((poses[:, :3, 3] - center).mean(0))
    v1 = _unit(np.cross([0.1, 0.2, 0.3], v0))
    v2 = _unit(np.cross(v0, v1))
    frame = np.stack([v1, v2, v0, center], axis=1)
    reset = np.linalg.inv(_to44(frame[None])) @ _to44(poses[:, :3, :4])
    hwf = np.broadcast_to(poses[0, :3, -1:], reset[:, :3, -1:].shape)
    return np.concatenate([reset[:, :3, :4], hwf], axis=-1)


def read_colmap_pinhole(fname):
    """First camera of a COLMAP `cameras.bin` as K = [[fx,0,cx],[0,fy,cy],[0,0,1]] (datasets.py:392-413 reads exactly this much:
    count, (camera_id, model_id, width, height), four doubles)."""
    with open(fname, "rb") as f:
        struct.unpack("<Q", f.read(8))
        struct.unpack("<iiQQ", f.read(24))
        fx, fy, cx, cy = struct.unpack("<dddd", f.read(32))
    return np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])


# COLMAP camera models (src/colmap/sensor/models.h): id -> (name, number of parameters).  Ids 0-5 are read; the others are refused by name.
COLMAP_MODELS = {0: ("SIMPLE_PINHOLE", 3), 1: ("PINHOLE", 4), 2: ("SIMPLE_RADIAL", 4), 3: ("RADIAL", 5), 4: ("OPENCV", 8),
                 5: ("OPENCV_FISHEYE", 8), 6: ("FULL_OPENCV", 12), 7: ("FOV", 5), 8: ("SIMPLE_RADIAL_FISHEYE", 4), 9: ("RADIAL_FISHEYE", 5),
                 10: ("THIN_PRISM_FISHEYE", 12)}
COLMAP_MODELS_READ = 6
CAMERA_NEWTON_STEPS = 8                 # csrc/camera_models.hpp
ROUND_TRIP_TOL = 1e-6                   # normalised units: undistort, then distort, every border pixel (`check_invertible`)


def read_colmap_cameras(fname):
    """Every camera of a COLMAP `cameras.bin` as (camera_id, model_name, width, height, params): the models SIMPLE_PINHOLE, PINHOLE,
    SIMPLE_RADIAL, RADIAL, OPENCV and OPENCV_FISHEYE, `params` the model's doubles in COLMAP's order.  Any other model raises
    NotImplementedError with its name."""
    cameras = []
    with open(fname, "rb") as f:
        (count,) = struct.unpack("<Q", f.read(8))
        for _ in range(count):
            camera_id, model_id, width, height = struct.unpack("<iiQQ", f.read(24))
            if model_id not in COLMAP_MODELS or model_id >= COLMAP_MODELS_READ:
                name = COLMAP_MODELS.get(model_id, (f"model id {model_id}", 0))[0]
                raise NotImplementedError(f"{fname}: camera {camera_id} has the COLMAP model {name}; read are "
                                          + ", ".join(COLMAP_MODELS[i][0] for i in range(COLMAP_MODELS_READ))
                                          + " -- undistort the capture with COLMAP (colmap image_undistorter) first")
            name, n = COLMAP_MODELS[model_id]
            cameras.append((camera_id, name, int(width), int(height), struct.unpack("<" + "d" * n, f.read(8 * n))))
    return cameras


def read_colmap_image_cameras(fname):
    """{image file name: camera_id} of a COLMAP `images.bin` (the poses and the 2D points are skipped)."""
    out = {}
    with open(fname, "rb") as f:
        (count,) = struct.unpack("<Q", f.read(8))
        for _ in range(count):
            _image_id = struct.unpack("<i", f.read(4))
            f.read(56)                                                   # qvec[4], tvec[3]
            (camera_id,) = struct.unpack("<i", f.read(4))
            name = b""
            while True:
                c = f.read(1)
                if c in (b"\x00", b""):
                    break
                name += c
            (n2d,) = struct.unpack("<Q", f.read(8))
            f.seek(24 * n2d, 1)                                          # (x, y, point3D_id)
            out[name.decode()] = camera_id
    return out


def colmap_intrinsics(model_name, params):
    """(K, model of `ops.camera_record`, its four coefficients) of one `read_colmap_cameras` entry."""
    p = [float(v) for v in params]
    if model_name in ("SIMPLE_PINHOLE", "SIMPLE_RADIAL", "RADIAL"):
        fx, fy, cx, cy, rest = p[0], p[0], p[1], p[2], p[3:]
    else:
        fx, fy, cx, cy, rest = p[0], p[1], p[2], p[3], p[4:]
    K = np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])
    if model_name in ("SIMPLE_PINHOLE", "PINHOLE"):
        return K, "pinhole", (0.0, 0.0, 0.0, 0.0)
    if model_name == "OPENCV_FISHEYE":
        return K, "fisheye", tuple(rest)
    return K, "radial", tuple(rest + [0.0] * (4 - len(rest)))           # SIMPLE_RADIAL: k1; RADIAL: k1, k2; OPENCV: k1, k2, p1, p2


def distort_points(model, coeffs, x, y):
    """COLMAP's forward model in float64 numpy: undistorted normalised points -> distorted ones ('radial': k1, k2, p1, p2; 'fisheye':
    k1..k4, where (x, y) = tan(theta) times a unit vector; 'pinhole': unchanged)."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    if model == "pinhole":
        return x, y
    a, b, c, d = (float(v) for v in coeffs)
    if model == "radial":
        r2 = x * x + y * y
        radial = 1.0 + a * r2 + b * r2 * r2
        return x * radial + 2.0 * c * x * y + d * (r2 + 2.0 * x * x), y * radial + 2.0 * d * x * y + c * (r2 + 2.0 * y * y)
    r = np.sqrt(x * x + y * y)
    th = np.arctan(r)
    t2 = th * th
    thd = th * (1.0 + t2 * (a + t2 * (b + t2 * (c + t2 * d))))
    s = np.where(r < 1e-8, 1.0, thd / np.where(r < 1e-8, 1.0, r))
    return s * x, s * y


def undistort_points(model, coeffs, xd, yd, steps=CAMERA_NEWTON_STEPS):
    """The device's solve (csrc/camera_models.hpp) in float64 numpy: distorted normalised points -> ('radial') the undistorted points
    (xu, yu), ('fisheye') the angle theta and the distorted radius theta_d.  `steps` Newton steps from the distorted point, a step with a
    determinant below 1e-9 in magnitude is a zero step, a non-finite result falls back to the start."""
    xd, yd = np.asarray(xd, np.float64), np.asarray(yd, np.float64)
    a, b, c, d = (float(v) for v in coeffs)
    with np.errstate(all="ignore"):
        if model == "radial":
            x, y = xd.copy(), yd.copy()
            for _ in range(steps):
                fx, fy = distort_points(model, coeffs, x, y)
                fx, fy = fx - xd, fy - yd
                r2 = x * x + y * y
                radial = 1.0 + a * r2 + b * r2 * r2
                dr = 2.0 * (a + 2.0 * b * r2)
                j00 = radial + dr * x * x + 2.0 * c * y + 6.0 * d * x
                j01 = dr * x * y + 2.0 * c * x + 2.0 * d * y
                j11 = radial + dr * y * y + 2.0 * d * x + 6.0 * c * y
                det = j00 * j11 - j01 * j01
                ok = np.abs(det) > 1e-9
                inv = 1.0 / np.where(ok, det, 1.0)
                x = x - np.where(ok, (j11 * fx - j01 * fy) * inv, 0.0)
                y = y - np.where(ok, (j00 * fy - j01 * fx) * inv, 0.0)
            fin = np.isfinite(x) & np.isfinite(y)
            return np.where(fin, x, xd), np.where(fin, y, yd)
        thd = np.sqrt(xd * xd + yd * yd)
        th = thd.copy()
        for _ in range(steps):
            t2 = th * th
            f = th * (1.0 + t2 * (a + t2 * (b + t2 * (c + t2 * d)))) - thd
            df = 1.0 + t2 * (3.0 * a + t2 * (5.0 * b + t2 * (7.0 * c + t2 * (9.0 * d))))
            ok = np.abs(df) > 1e-9
            th = th - np.where(ok, f / np.where(ok, df, 1.0), 0.0)
        return np.where(np.isfinite(th), th, thd), thd


def round_trip_error(model, coeffs, K, width, height):
    """The largest distance, in normalised units, between a border pixel centre of a width x height image of the distorted camera (K,
    model, coeffs) and the image of its undistorted point under the forward model: what the device's 8-step solve leaves."""
    if model == "pinhole":
        return 0.0
    xs, ys = np.arange(width) + 0.5, np.arange(height) + 0.5
    px = np.concatenate([xs, xs, np.full(height, 0.5), np.full(height, width - 0.5)])
    py = np.concatenate([np.full(width, 0.5), np.full(width, height - 0.5), ys, ys])
    xd, yd = (px - K[0, 2]) / K[0, 0], (py - K[1, 2]) / K[1, 1]
    with np.errstate(all="ignore"):
        if model == "radial":
            xu, yu = undistort_points(model, coeffs, xd, yd)
            bx, by = distort_points(model, coeffs, xu, yu)
            err = np.sqrt((bx - xd) ** 2 + (by - yd) ** 2)
        else:
            th, thd = undistort_points(model, coeffs, xd, yd)
            a, b, c, d = (float(v) for v in coeffs)
            t2 = th * th
            err = np.abs(th * (1.0 + t2 * (a + t2 * (b + t2 * (c + t2 * d)))) - thd)
            err = np.where((th >= 0.0) & (th < np.pi), err, np.inf)           # a root outside [0, pi) is no viewing angle
    return float(np.max(np.where(np.isfinite(err), err, np.inf)))


def check_invertible(camera_id, model_name, model, coeffs, K, width, height):
    """Refuse a camera whose image border lies outside the invertible domain of its distortion model (a strong barrel model folds back
    before the border): every border pixel, undistorted as the device does and distorted back, must return to within 1e-6."""
    err = round_trip_error(model, coeffs, K, width, height)
    if not err <= ROUND_TRIP_TOL:
        raise ValueError(f"COLMAP camera {camera_id} ({model_name}, distortion {tuple(coeffs)}): undistorting the border of its {width}x{height} "
                         f"image and distorting it back misses by {err:.3g} in normalised units (limit {ROUND_TRIP_TOL:g}) -- the border lies "
                         "outside the model's invertible domain; undistort the capture with COLMAP (colmap image_undistorter) first")


def _image_files(imgdir):
    return [os.path.join(imgdir, f) for f in sorted(os.listdir(imgdir)) if f.endswith(("JPG", "jpg", "png"))]


def _split_indices(n, split):
    """Indices into the sorted file list: every 8th image is the test split, the others train (datasets.py:325-331)."""
    idx = np.arange(n)
    test = idx[::8]
    return np.array([i for i in idx if i not in test]) if split == "train" else test


def realdata360_files(data_dir, split, factor):
    """(files of `split`, number of files of all splits, shrink): the files of images_<factor>/ when that folder exists (shrink
    False), else those of images/ (shrink True: `load_realdata360` shrinks them by `factor` on the device).  Sorted by file name;
    the split is chosen before anything is decoded."""
    if factor <= 0:
        raise ValueError("RealData360 needs factor > 0 (images_<factor>/; datasets.py:312 divides by it)")
    imgdir = os.path.join(data_dir, f"images_{factor}")
    shrink = not os.path.exists(imgdir)
    if shrink:
        if not os.path.exists(os.path.join(data_dir, "images")):
            raise ValueError(f"Image folder {imgdir} does not exist.")
        imgdir = os.path.join(data_dir, "images")
    files = _image_files(imgdir)
    return [files[i] for i in _split_indices(len(files), split)], len(files), shrink


def _read_u8(fname):
    from PIL import Image
    with open(fname, "rb") as f:
        a = np.array(Image.open(f))
    if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] not in (3, 4):
        raise ValueError(f"{fname}: expected an 8-bit image of 3 or 4 channels, got {a.dtype} {a.shape}")
    return a


def decode_u8(files, workers=16):
    """`files` decoded on host threads (PIL releases the GIL while it decodes): uint8 [n, H, W, C]; ValueError when they differ in shape."""
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max(1, min(int(workers), len(files)))) as pool:
        frames = list(pool.map(_read_u8, files))
    for f, a in zip(files, frames):
        if a.shape != frames[0].shape:
            raise ValueError(f"{f}: {a.shape} differs from the first image's {frames[0].shape}")
    return np.stack(frames)


def _shrink_on_device(files, factor, device):
    if device is None:
        raise RuntimeError("datasets: images/ is shrunk by the HIP kernel; need a HIP device (there is no host fallback)")
    device = torch.device(device)
    with torch.cuda.device(device):
        return ops.area_downscale(torch.from_numpy(decode_u8(files)).to(device), factor)


def _capture_cameras(data_dir, files, factor, w, h):
    """({camera_id: dict(name, model, distortion, K, K_inv)} in file order, [camera_id of every file of `files`]) of a capture's
    sparse/0: K is divided by `factor` (the distortion coefficients are not: they live in normalised coordinates), K_inv = K^-1 with rows
    1 and 2 negated.  One camera: every image is its.  Several: sparse/0/images.bin names each image's; they may differ in model and
    parameters but not in image size, because the pixel table is stacked.  Every distorted camera passes `check_invertible` at (w, h)."""
    fname = os.path.join(data_dir, "sparse", "0", "cameras.bin")
    entries = read_colmap_cameras(fname)
    if not entries:
        raise ValueError(f"{fname} holds no camera")
    sizes = {(cw, ch) for _, _, cw, ch, _ in entries}
    if len(sizes) > 1:
        raise ValueError(f"{fname}: its cameras differ in image size ({', '.join(f'{a}x{b}' for a, b in sorted(sizes))}); a capture whose "
                         "images differ in size is not supported (the pixel table is stacked)")
    cams = {}
    for camera_id, name, _, _, params in entries:
        K, model, coeffs = colmap_intrinsics(name, params)
        K[:2, :] /= factor
        K_inv = np.linalg.inv(K)
        K_inv[1:, :] *= -1
        check_invertible(camera_id, name, model, coeffs, K, w, h)
        cams[camera_id] = dict(name=name, model=model, distortion=coeffs, K=K, K_inv=K_inv)
    if len(cams) == 1:
        return cams, [entries[0][0]] * len(files)
    iname = os.path.join(data_dir, "sparse", "0", "images.bin")
    if not os.path.exists(iname):
        raise FileNotFoundError(f"{fname} holds {len(cams)} cameras, so {iname} is needed to tell each image's camera, and it is missing")
    by_name = read_colmap_image_cameras(iname)
    by_stem = {os.path.splitext(k)[0]: v for k, v in by_name.items()}
    cam_of = []
    for f in files:
        base = os.path.basename(f)
        cid = by_name.get(base, by_stem.get(os.path.splitext(base)[0]))
        if cid is None:
            raise ValueError(f"{iname} names no image {base}")
        if cid not in cams:
            raise ValueError(f"{iname}: image {base} belongs to camera {cid}, which {fname} does not hold")
        cam_of.append(cid)
    return cams, cam_of


def load_realdata360(data_dir, split, white_bkgd=True, factor=0, device=None):
    """datasets.py:278-345.  `factor` must be > 0 (upstream divides by it at :312 and :335; with the shipped default 0 it
    produces infinities -- raised here instead).  Every 8th image is the test split.
    Without an images_<factor>/ folder but with images/ (a capture as COLMAP leaves it), the split's files of images/ are decoded to
    bytes, uploaded once and shrunk by `factor` on `device` straight into the pixel table (`ops.area_downscale`: the box mean rounded
    to a byte, i.e. the pixels an images_<factor>/ folder of those bytes would give); the first return value is then that [P, 3] device
    tensor and info['sizes'] the (height, width) of every image.
    Cameras: `read_colmap_cameras` of sparse/0/cameras.bin (SIMPLE_PINHOLE, PINHOLE, SIMPLE_RADIAL, RADIAL, OPENCV, OPENCV_FISHEYE; see
    `_capture_cameras` for several cameras and for the refusals).  A distorted camera's record carries its model and coefficients and the
    kernel undistorts every ray, so the photos are trained on and compared with as they are: info['models'] (COLMAP names), ['distortion']
    [n, 4] and ['Ks'] [n, 3, 3] are per image; ['K'] / ['K_inv'] stay those of the file's first camera."""
    files, n_files, shrink = realdata360_files(data_dir, split, factor)
    images = None if shrink else np.stack([_read_image(f) for f in _image_files(os.path.join(data_dir, f"images_{factor}"))], axis=0)
    arr = np.load(os.path.join(data_dir, "poses_bounds.npy"))
    if arr.shape[0] != n_files:
        raise RuntimeError(f"Mismatch between imgs {n_files} and poses {arr.shape[0]}")
    if images is None:
        pixels = _shrink_on_device(files, factor, device)           # [n_split, h, w, 3] on the device
        shape = (n_files,) + tuple(pixels.shape[1:])
    else:
        pixels, shape = None, images.shape
    poses = arr[:, :-2].reshape(-1, 3, 5).copy()                     # [n, 3, 5] = [R | t | (h, w, f)] in LLFF axis order
    bds = arr[:, -2:].astype(np.float32)
    poses[:, 0, 4], poses[:, 1, 4] = shape[1], shape[2]
    poses[:, 2, 4] /= factor
    poses = np.concatenate([poses[:, :, 1:2], -poses[:, :, 0:1], poses[:, :, 2:]], axis=2).astype(np.float32)   # (down,right,back) -> (right,up,back)
    poses = spherify_poses(recenter_poses(poses))
    sel = _split_indices(n_files, split)
    h, w = (int(v) for v in shape[1:3])
    all_files = _image_files(os.path.join(data_dir, "images" if shrink else f"images_{factor}"))
    cams, cam_of = _capture_cameras(data_dir, all_files, factor, w, h)
    first = cams[next(iter(cams))]
    K, K_inv = first["K"], first["K_inv"]
    per_image = [cams[cam_of[i]] for i in sel]
    records = [ops.camera_record(poses[i, :3, :4], w, h, float(bds[i, 0]), float(bds[i, 1]), pix2cam=c["K_inv"],
                                 **({} if c["model"] == "pinhole" else dict(model=c["model"], distortion=c["distortion"])))
               for i, c in zip(sel, per_image)]
    info = dict(h=h, w=w, K=K, K_inv=K_inv, bds=bds[sel], camtoworlds=poses[sel][:, :3, :4], focal=poses[0, -1, -1],
                models=[c["name"] for c in per_image], distortion=np.array([c["distortion"] for c in per_image], np.float64).reshape(-1, 4),
                Ks=np.stack([c["K"] for c in per_image]) if per_image else np.zeros((0, 3, 3)))
    if pixels is not None:
        return pixels.view(-1, 3), records, dict(info, sizes=[(h, w)] * len(sel))
    imgs = [np.ascontiguousarray(images[i, ..., :3], dtype=np.float32) for i in sel]
    return imgs, records, info


def create_spheric_poses(radius, n_poses=120):
    """utils/vis.py:159-198: `n_poses` camera-to-world matrices on a circle around the z axis, looking 36 degrees down."""
    phi = -np.pi / 5
    trans = np.eye(4)
    trans[2, 3] = radius
    rot_phi = np.array([[1, 0, 0, 0], [0, np.cos(phi), -np.sin(phi), 0], [0, np.sin(phi), np.cos(phi), 0], [0, 0, 0, 1]])
    swap = np.array([[-1, 0, 0, 0], [0, 0, 1, 0], [0, 1, 0, 0], [0, 0, 0, 1]])
    out = []
    for th in np.linspace(0, 2 * np.pi, n_poses + 1)[:-1]:
        rot_th = np.array([[np.cos(th), 0, -np.sin(th), 0], [0, 1, 0, 0], [np.sin(th), 0, np.cos(th), 0], [0, 0, 0, 1]])
        out.append((swap @ (rot_th @ rot_phi @ trans))[:3])
    return np.stack(out, 0)


def _matrix_to_euler_xyz(m):
    """Angles in degrees of the extrinsic x, y, z rotations that compose the rotation nearest to `m` [3, 3] (its orthogonal Procrustes
    projection U V^T, as scipy's Rotation.from_matrix takes a matrix that is only nearly orthogonal): m = Rz(c) Ry(b) Rx(a) -> (a, b, c),
    b in [-90, 90].  Not meant for b = +-90 (gimbal lock)."""
    u, _, vt = np.linalg.svd(np.asarray(m, np.float64))
    if np.linalg.det(u @ vt) < 0:
        u[:, -1] = -u[:, -1]
    r = u @ vt
    return np.degrees([np.arctan2(r[2, 1], r[2, 2]), -np.arcsin(np.clip(r[2, 0], -1.0, 1.0)), np.arctan2(r[1, 0], r[0, 0])])


def _euler_xyz_to_matrix(deg):
    (sa, sb, sc), (ca, cb, cc) = np.sin(np.radians(deg)), np.cos(np.radians(deg))
    return np.array([[cb * cc, sa * sb * cc - ca * sc, ca * sb * cc + sa * sc],
                     [cb * sc, sa * sb * sc + ca * cc, ca * sb * sc - sa * cc],
                     [-sb, sa * cb, ca * cb]])


def gen_render_path(c2ws, n_views=30):
    """utils/vis.py:92-121: a closed path through the poses `c2ws` [N, 3|4, 4] in their order: n_views // 3 poses per consecutive pair
    (and from the last back to the first), positions and extrinsic-xyz Euler angles in degrees interpolated linearly; an angle more
    than 180 degrees away from the FIRST pose's has 360 added (upstream's unwrap, whatever the sign).  Float64 [N * (n_views // 3), 4, 4]."""
    c2ws = np.asarray(c2ws, np.float64)
    weight = np.linspace(1.0, 0.0, int(n_views) // 3, endpoint=False).reshape(1, -1, 1)
    angles = []
    for i, m in enumerate(c2ws):
        e = _matrix_to_euler_xyz(m[:3, :3])
        if i:
            e[np.abs(e - angles[0]) > 180] += 360.0
        angles.append(e)
    angles, positions = np.stack(angles)[:, None], c2ws[:, None, :3, 3]
    angles = (weight * angles + (1.0 - weight) * np.roll(angles, -1, axis=0)).reshape(-1, 3)
    positions = (weight * positions + (1.0 - weight) * np.roll(positions, -1, axis=0)).reshape(-1, 3)
    out = np.tile(np.eye(4), (len(angles), 1, 1))
    for m, e, p in zip(out, angles, positions):
        m[:3, :3], m[:3, 3] = _euler_xyz_to_matrix(e), p
    return out


# ---------------------------------------------------------------------------------------------------------------------
# device side
# ---------------------------------------------------------------------------------------------------------------------
def _default_device():
    return torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else None


class BaseDataset(torch.utils.data.Dataset):
    """datasets.py:25-81 with the rays left implicit.  `split == 'train'`: `len` = number of pixels of all images
    (batch_type 'all_images'), item i = (ray i, pixel i); otherwise `len` = number of images and an item is a whole image
    `(Rays [H,W,k], image [H,W,3])` -- like upstream, the val split ignores the index and walks the images in order."""

    def __init__(self, data_dir, split, white_bkgd=True, batch_type="all_images", factor=0, device=None):
        super().__init__()
        self.near, self.far = 2, 6
        self.split, self.data_dir, self.white_bkgd, self.batch_type, self.factor = split, data_dir, white_bkgd, batch_type, factor
        self.it = -1
        if split == "train":
            assert batch_type == "all_images", "The batch_type can only be all_images with flatten"
        else:
            assert batch_type == "single_image", "The batch_type can only be single_image without flatten"
        dev = device if device is not None else _default_device()
        self._load_device = dev                 # for a loader that makes its pixels on the device (Multicam off a Blender directory)
        self._device_pixels = None
        self.images, records, info = self._load()
        for k, v in info.items():
            setattr(self, k, v)
        self.n_examples = len(records)
        self.cameras = torch.stack(records)                                    # [n, 32] host copy of the camera table
        if self.images is not None:
            self.sizes = [(im.shape[0], im.shape[1]) for im in self.images]
        self.offsets = np.concatenate([[0], np.cumsum([h * w for h, w in self.sizes])]).astype(np.int64)
        self.device = None
        self._dev = None
        if dev is not None:
            self.to(dev)

    def _load(self):
        raise ValueError("Implement in different dataset.")

    # -- device residency
    def to(self, device):
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("datasets: rays are generated by the HIP kernel; need a HIP device")
        if self._device_pixels is not None:
            pixels = self._device_pixels = self._device_pixels.to(device)
        else:
            pixels = torch.from_numpy(np.concatenate([im.reshape(-1, 3) for im in self.images], axis=0)).to(device)
        self._dev = dict(cameras=self.cameras.to(device), pixels=pixels,
                         offsets=torch.from_numpy(self.offsets).to(device))
        self.device = device
        return self

    def _need_device(self):
        if self._dev is None:
            raise RuntimeError("datasets: no HIP device (construct with device=... or call .to(device)); rays are computed by "
                               "k_generate_rays, there is no host fallback")
        return self._dev

    @property
    def num_pixels(self):
        return int(self.offsets[-1])

    def rays_at(self, ids):
        """(Rays [n,k], pixels [n,3]) of global pixel ids `ids` (int64 device tensor over the concatenation of all images)."""
        d = self._need_device()
        ids = ids.to(d["offsets"].device, torch.int64).reshape(-1).contiguous()
        cam = torch.searchsorted(d["offsets"], ids, right=True) - 1
        pix = ids - d["offsets"][cam]
        rays = ops.generate_rays(d["cameras"], cam_idx=cam, pix_idx=pix)
        return rays, d["pixels"][ids]

    def image_rays(self, i):
        """(Rays [H,W,k], image [H,W,3]) of image i."""
        d = self._need_device()
        h, w = self.sizes[i]
        cam = torch.full((h * w,), i, dtype=torch.int32, device=self.device)
        rays = ops.generate_rays(d["cameras"], cam_idx=cam, pix_idx=torch.arange(h * w, dtype=torch.int32, device=self.device))
        lo, hi = int(self.offsets[i]), int(self.offsets[i + 1])
        return Rays(*[t.reshape(h, w, -1) for t in rays]), d["pixels"][lo:hi].reshape(h, w, 3)

    def sample(self, batch_size, generator=None):
        """One training batch drawn uniformly over all pixels, entirely on the device."""
        d = self._need_device()
        ids = torch.randint(0, self.num_pixels, (batch_size,), device=self.device, generator=generator)
        return self.rays_at(ids)

    # -- torch Dataset protocol (datasets.py:72-81)
    def __len__(self):
        return self.num_pixels if self.split == "train" else self.n_examples

    def __getitem__(self, index):
        if self.split == "train":
            scalar = not torch.is_tensor(index) and np.ndim(index) == 0
            ids = torch.as_tensor(index, dtype=torch.int64).reshape(-1)
            rays, pix = self.rays_at(ids.to(self.device) if self.device is not None else ids)
            return (Rays(*[t[0] for t in rays]), pix[0]) if scalar else (rays, pix)
        if self.split == "val":
            index = (self.it + 1) % self.n_examples
            self.it += 1
        return self.image_rays(int(index))


class Blender(BaseDataset):
    """Blender Dataset (datasets.py:171-263)."""

    def __init__(self, data_dir, split="train", white_bkgd=True, batch_type="all_images", factor=0, device=None):
        super().__init__(data_dir, split, white_bkgd, batch_type, factor, device)

    def _load(self):
        return load_blender(self.data_dir, self.split, self.white_bkgd, self.factor)


class Multicam(BaseDataset):
    """Multicam (multi-scale Blender) Dataset (datasets.py:84-168).  `data_dir` is a directory written by convert_blender_data -- or
    a Blender scene directory itself (no `metadata.json`, but `transforms_{split}.json`): then the `n_down` levels of every frame
    are made on the device at start-up (`from_blender`), `images` is None and the pixels live on the device only."""

    def __init__(self, data_dir, split="train", white_bkgd=True, batch_type="all_images", device=None, n_down=4, blender=None):
        if blender is None:
            blender = (not os.path.exists(os.path.join(data_dir, "metadata.json"))
                       and os.path.exists(os.path.join(data_dir, f"transforms_{split}.json")))
        self.n_down, self.blender = int(n_down), bool(blender)
        super().__init__(data_dir, split, white_bkgd, batch_type, 0, device)

    @classmethod
    def from_blender(cls, data_dir, split="train", white_bkgd=True, batch_type="all_images", n_down=4, device=None):
        """The multi-scale data set of a Blender scene directory without a conversion step (see the class)."""
        return cls(data_dir, split, white_bkgd, batch_type, device=device, n_down=n_down, blender=True)

    def _load(self):
        if not self.blender:
            return load_multicam(self.data_dir, self.split, self.white_bkgd)
        self._device_pixels, records, info = load_multicam_from_blender(self.data_dir, self.split, self.white_bkgd, self.n_down, self._load_device)
        return None, records, info


class RealData360(BaseDataset):
    """RealData360 / LLFF Dataset (datasets.py:266-474); per-image near / far from `poses_bounds.npy`."""

    def __init__(self, data_dir, split="train", white_bkgd=True, batch_type="all_images", factor=4, device=None):
        super().__init__(data_dir, split, white_bkgd, batch_type, factor, device)

    def _load(self):
        images, records, info = load_realdata360(self.data_dir, self.split, self.white_bkgd, self.factor, self._load_device)
        if torch.is_tensor(images):             # made on the device from images/: no host copy
            self._device_pixels, images = images, None
        return images, records, info


class RenderGen(torch.utils.data.Dataset):
    """render_video.py:19-118: `scales` pyramids of the spherical path of `n_poses` poses (the reference's 120 by default); item i =
    Rays [H_i, W_i, k] of camera i."""

    def __init__(self, base_focal, base_size, scales=4, device=None, n_poses=120):
        super().__init__()
        self.near, self.far = 2, 6
        c2w = create_spheric_poses(4, n_poses)
        records, self.sizes = [], []
        for i in range(scales):
            w, h, f = base_size[0] / 2 ** i, base_size[1] / 2 ** i, base_focal / 2 ** i
            pix2cam = np.array([[1.0 / f, 0.0, -0.5 * w / f], [0.0, -1.0 / f, 0.5 * h / f], [0.0, 0.0, -1.0]])
            for m in c2w:
                # float64 table -> float64 ray arithmetic on the device, as the reference's numpy (its poses and pix2cam are float64)
                records.append(ops.camera_record(np.asarray(m, np.float64), w, h, self.near, self.far, pix2cam=pix2cam, dtype=torch.float64))
                self.sizes.append((int(h), int(w)))
        self._set_cameras(records, device)

    def _set_cameras(self, records, device):
        self.n_sample = len(records)
        self.cameras = torch.stack(records)
        dev = device if device is not None else _default_device()
        self.device = torch.device(dev) if dev is not None else None
        self._cams_dev = self.cameras.to(self.device) if self.device is not None else None

    def __len__(self):
        return self.n_sample

    def pixel_rays(self, cam_idx, pix_idx):
        """Rays [n, k] of single pixels: `pix_idx` (row-major within the image) of the cameras `cam_idx`, both integer device tensors [n]."""
        if self._cams_dev is None:
            raise RuntimeError("RenderGen: no HIP device; rays are computed by k_generate_rays")
        return ops.generate_rays(self._cams_dev, cam_idx=cam_idx.to(self.device, torch.int32), pix_idx=pix_idx.to(self.device, torch.int32))

    def __getitem__(self, index):
        if self._cams_dev is None:
            raise RuntimeError("RenderGen: no HIP device; rays are computed by k_generate_rays")
        h, w = self.sizes[index]
        cam = torch.full((h * w,), int(index), dtype=torch.int32, device=self.device)
        rays = ops.generate_rays(self._cams_dev, cam_idx=cam, pix_idx=torch.arange(h * w, dtype=torch.int32, device=self.device))
        return Rays(*[t.reshape(h, w, -1) for t in rays])


class PathGen(RenderGen):
    """The render path of a captured scene: `gen_render_path` through the poses of `dataset` (a RealData360 split; `poses` [n, 3|4, 4]
    given: those instead), one float32 camera record per pose built as `load_realdata360` builds the data set's (its size and pix2cam),
    near / far = the smallest / largest bound of the split.  Item i = Rays [h, w, k] of pose i.
    The records are IDEAL PINHOLE ones from the data set's `K_inv` (mode 1, no coefficients) even when the capture's camera is distorted:
    a fly-through is rendered undistorted, as multinerf renders its paths.  `eval` and the validation loop of `train` take their rays from
    the data set itself, i.e. from the distorted camera, because they are compared with the photos."""

    def __init__(self, dataset, n_views=30, poses=None, device=None):
        torch.utils.data.Dataset.__init__(self)
        self.poses = gen_render_path(dataset.camtoworlds, n_views) if poses is None else np.asarray(poses)
        self.near, self.far = float(dataset.bds.min()), float(dataset.bds.max())
        h, w = int(dataset.h), int(dataset.w)
        self.sizes = [(h, w)] * len(self.poses)
        self._set_cameras([ops.camera_record(m[:3, :4], w, h, self.near, self.far, pix2cam=dataset.K_inv) for m in self.poses],
                          device if device is not None else dataset.device)


class RayLoader:
    """What `DataLoader(dataset, shuffle, batch_size)` yields in nerf_system.py:78-93, without the host: a fresh device
    permutation of the pixel ids per epoch (train) or one image per item with the leading batch dimension of 1 (val / test).
    With world_size > 1 (default: the initialised torch.distributed group) every rank draws the SAME permutation (same seed,
    same epoch), PADS it to a multiple of world_size by wrapping around to its own start, and keeps every world_size-th id
    starting at its rank -- what Lightning's DistributedSampler (drop_last=False) does for the reference under
    train.py:56-60 -- so every rank sees the same number of rays and of batches per epoch (a rank with one batch more would
    wait forever in the gradient all-reduce) and the global batch is batch_size x world_size rays, disjoint except for the
    < world_size wrapped ids of the last batch."""

    def __init__(self, dataset, batch_size=1, shuffle=False, drop_last=False, seed=0, rank=None, world_size=None):
        self.dataset, self.batch_size, self.shuffle, self.drop_last = dataset, int(batch_size), shuffle, drop_last
        self.seed, self.epoch = int(seed), 0
        if world_size is None:
            import torch.distributed as dist
            on = dist.is_available() and dist.is_initialized()
            world_size, rank = (dist.get_world_size(), dist.get_rank()) if on else (1, 0)
        self.rank, self.world_size = int(rank or 0), int(world_size)

    def _local_count(self):
        n = len(self.dataset)
        if self.dataset.split != "train":
            return n
        return (n + self.world_size - 1) // self.world_size          # identical on every rank (padded permutation)

    def __len__(self):
        n = self._local_count()
        if self.dataset.split != "train":
            return n
        return n // self.batch_size if self.drop_last else (n + self.batch_size - 1) // self.batch_size

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def __iter__(self):
        ds = self.dataset
        if ds.split != "train":
            for i in range(len(ds)):
                rays, image = ds[i]
                yield Rays(*[t[None] for t in rays]), image[None]
            return
        n = len(ds)
        if self.shuffle:
            g = torch.Generator(device=ds.device)
            g.manual_seed(self.seed + self.epoch)
            order = torch.randperm(n, device=ds.device, generator=g)
        else:
            order = torch.arange(n, device=ds.device)
        self.epoch += 1
        pad = self._local_count() * self.world_size - n
        if pad:      # DistributedSampler's rule: wrap around, repeating the list when the pad exceeds it (n < world_size - 1)
            order = order.repeat(pad // max(n, 1) + 2)[:n + pad]
        order = order[self.rank::self.world_size]
        for b in range(len(self)):
            yield ds.rays_at(order[b * self.batch_size:(b + 1) * self.batch_size])


dataset_dict = {
    "blender": Blender,             # datasets/__init__.py:2-4
    "multi_blender": Multicam,
    "llff": RealData360,            # registered here, dead upstream
    "realdata360": RealData360,
}

__all__ = ["Blender", "Multicam", "RealData360", "RenderGen", "PathGen", "gen_render_path", "RayLoader", "dataset_dict", "Rays", "Rays_keys",
           "create_spheric_poses", "load_blender", "load_multicam", "load_multicam_from_blender", "load_realdata360"]
