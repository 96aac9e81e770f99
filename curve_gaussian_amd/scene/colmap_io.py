"""COLMAP scans (the Replica_Edge layout), host-side Python like the reference's:

* ``sparse/0/{cameras,images,points3D}.{bin,txt}`` readers and writers -- the COLMAP model formats that
  scene/colmap_loader.py reads, restated here.
* ``read_colmap`` -- ``readColmapSceneInfo`` + ``readColmapCameras`` (scene/dataset_readers.py:74-249) followed by
  ``loadCam`` + ``Camera`` (utils/camera_utils.py:22-67, scene/cameras.py:18-66): the cameras are
  ``dataset_io.EdgeCamera`` objects holding the edge map of each image.
* ``write_colmap`` -- the inverse, used to put synthetic Replica-like scans on disk (BASELINE cfg4).

Parity: tests/golden/colmap/ is a small scan whose expected values were produced by the reference's own readers
(tests/golden/make_colmap_golden.py)."""
import os
import struct
from typing import NamedTuple

import numpy as np
import torch

from ..ops.undistort import distortion_of, undistort_images
from ..synthetic import projection_matrix, world2view
from .dataset_io import BasicPointCloud, EdgeCamera, _pil_to_chw, focal2fov, fov2focal, read_ply_table

# model id -> (name, number of parameters): the COLMAP camera models (colmap src/colmap/sensor/models.h)
CAMERA_MODELS = {
    0: ("SIMPLE_PINHOLE", 3), 1: ("PINHOLE", 4), 2: ("SIMPLE_RADIAL", 4), 3: ("RADIAL", 5), 4: ("OPENCV", 8),
    5: ("OPENCV_FISHEYE", 8), 6: ("FULL_OPENCV", 12), 7: ("FOV", 5), 8: ("SIMPLE_RADIAL_FISHEYE", 4),
    9: ("RADIAL_FISHEYE", 5), 10: ("THIN_PRISM_FISHEYE", 12),
}
MODEL_IDS = {name: (mid, n) for mid, (name, n) in CAMERA_MODELS.items()}


class ColmapCamera(NamedTuple):
    id: int
    model: str
    width: int
    height: int
    params: np.ndarray


class ColmapImage(NamedTuple):
    id: int
    qvec: np.ndarray          # w, x, y, z (world -> camera rotation)
    tvec: np.ndarray          # world -> camera translation
    camera_id: int
    name: str
    xys: np.ndarray           # [n,2] keypoints
    point3D_ids: np.ndarray   # [n]


def qvec2rotmat(q):
    """Rotation matrix of the unit quaternion (w, x, y, z)."""
    w, x, y, z = q
    return np.array([[1 - 2 * y * y - 2 * z * z, 2 * x * y - 2 * w * z, 2 * z * x + 2 * w * y],
                     [2 * x * y + 2 * w * z, 1 - 2 * x * x - 2 * z * z, 2 * y * z - 2 * w * x],
                     [2 * z * x - 2 * w * y, 2 * y * z + 2 * w * x, 1 - 2 * x * x - 2 * y * y]])


def rotmat2qvec(R):
    """Unit quaternion (w, x, y, z) with w >= 0 of a rotation matrix (largest-eigenvector form)."""
    R = np.asarray(R, np.float64)
    (xx, xy, xz), (yx, yy, yz), (zx, zy, zz) = R
    K = np.array([[xx - yy - zz, yx + xy, zx + xz, zy - yz],
                  [yx + xy, yy - xx - zz, zy + yz, xz - zx],
                  [zx + xz, zy + yz, zz - xx - yy, yx - xy],
                  [zy - yz, xz - zx, yx - xy, xx + yy + zz]]) / 3.0
    vals, vecs = np.linalg.eigh(K)
    q = vecs[[3, 0, 1, 2], np.argmax(vals)]
    return -q if q[0] < 0 else q


# ------------------------------------------------------------------------------------------------ binary model
def _take(f, fmt):
    fmt = "<" + fmt
    n = struct.calcsize(fmt)
    b = f.read(n)
    if len(b) != n:
        raise ValueError("COLMAP binary model: unexpected end of file")
    return struct.unpack(fmt, b)


def read_cameras_binary(path):
    cams = {}
    with open(path, "rb") as f:
        (n,) = _take(f, "Q")
        for _ in range(n):
            cid, mid, w, h = _take(f, "iiQQ")
            if mid not in CAMERA_MODELS:
                raise ValueError(f"{path}: unknown COLMAP camera model id {mid}")
            name, npar = CAMERA_MODELS[mid]
            cams[cid] = ColmapCamera(cid, name, w, h, np.array(_take(f, "d" * npar)))
    return cams


def read_images_binary(path):
    imgs = {}
    with open(path, "rb") as f:
        (n,) = _take(f, "Q")
        for _ in range(n):
            props = _take(f, "idddddddi")
            name = bytearray()
            while True:
                c = f.read(1)
                if c in (b"\x00", b""):
                    break
                name += c
            (npts,) = _take(f, "Q")
            blob = f.read(24 * npts)
            if len(blob) != 24 * npts:
                raise ValueError("COLMAP binary model: unexpected end of file")
            tab = np.frombuffer(blob, dtype=[("x", "<f8"), ("y", "<f8"), ("id", "<i8")])
            imgs[props[0]] = ColmapImage(props[0], np.array(props[1:5]), np.array(props[5:8]), props[8],
                                         name.decode("utf-8"), np.stack([tab["x"], tab["y"]], 1).reshape(-1, 2),
                                         tab["id"].astype(np.int64))
    return imgs


def read_points3D_binary(path):
    """-> (xyz [N,3] float64, rgb [N,3] float64 in 0..255, error [N,1])."""
    with open(path, "rb") as f:
        (n,) = _take(f, "Q")
        xyz, rgb, err = np.empty((n, 3)), np.empty((n, 3)), np.empty((n, 1))
        for i in range(n):
            p = _take(f, "QdddBBBd")
            xyz[i], rgb[i], err[i] = p[1:4], p[4:7], p[7]
            (track,) = _take(f, "Q")
            f.seek(8 * track, os.SEEK_CUR)
    return xyz, rgb, err


# ------------------------------------------------------------------------------------------------ text model
def _data_lines(path):
    with open(path) as f:
        for line in f:
            line = line.strip()
            if line and not line.startswith("#"):
                yield line


def read_cameras_text(path):
    """Every camera model is accepted (the reference's reader asserts PINHOLE here, colmap_loader.py:172, while its binary
    reader and readColmapCameras accept SIMPLE_PINHOLE and OPENCV too: the text twin of a scan reads like the binary one)."""
    cams = {}
    for line in _data_lines(path):
        e = line.split()
        if e[1] not in MODEL_IDS:
            raise ValueError(f"{path}: unknown COLMAP camera model {e[1]}")
        cams[int(e[0])] = ColmapCamera(int(e[0]), e[1], int(e[2]), int(e[3]), np.array([float(v) for v in e[4:]]))
    return cams


def read_images_text(path):
    imgs = {}
    with open(path) as f:
        lines = [ln.rstrip("\n") for ln in f]
    i = 0
    while i < len(lines):
        line = lines[i].strip()
        i += 1
        if not line or line.startswith("#"):
            continue
        e = line.split()
        pts = lines[i].split() if i < len(lines) else []   # the keypoint line that follows (may be empty)
        i += 1
        xys = np.array([[float(pts[k]), float(pts[k + 1])] for k in range(0, len(pts), 3)]).reshape(-1, 2)
        pids = np.array([int(pts[k + 2]) for k in range(0, len(pts), 3)], dtype=np.int64)
        iid = int(e[0])
        imgs[iid] = ColmapImage(iid, np.array([float(v) for v in e[1:5]]), np.array([float(v) for v in e[5:8]]),
                                int(e[8]), e[9], xys, pids)
    return imgs


def read_points3D_text(path):
    rows = [ln.split() for ln in _data_lines(path)]
    xyz = np.array([[float(v) for v in r[1:4]] for r in rows]).reshape(-1, 3)
    rgb = np.array([[int(v) for v in r[4:7]] for r in rows], dtype=np.float64).reshape(-1, 3)
    err = np.array([[float(r[7])] for r in rows]).reshape(-1, 1)
    return xyz, rgb, err


# ------------------------------------------------------------------------------------------------ writers
def write_cameras_binary(path, cams):
    with open(path, "wb") as f:
        f.write(struct.pack("<Q", len(cams)))
        for c in cams.values():
            mid, npar = MODEL_IDS[c.model]
            assert len(c.params) == npar, (c.model, len(c.params))
            f.write(struct.pack("<iiQQ", c.id, mid, c.width, c.height) + struct.pack("<" + "d" * npar, *c.params))


def write_cameras_text(path, cams):
    with open(path, "w") as f:
        f.write("# Camera list with one line of data per camera:\n#   CAMERA_ID, MODEL, WIDTH, HEIGHT, PARAMS[]\n")
        for c in cams.values():
            f.write(" ".join([str(c.id), c.model, str(c.width), str(c.height)] + ["%.17g" % p for p in c.params]) + "\n")


def write_images_binary(path, imgs):
    with open(path, "wb") as f:
        f.write(struct.pack("<Q", len(imgs)))
        for im in imgs.values():
            f.write(struct.pack("<idddddddi", im.id, *im.qvec, *im.tvec, im.camera_id))
            f.write(im.name.encode("utf-8") + b"\x00")
            f.write(struct.pack("<Q", len(im.point3D_ids)))
            for (x, y), pid in zip(im.xys, im.point3D_ids):
                f.write(struct.pack("<ddq", x, y, int(pid)))


def write_images_text(path, imgs):
    with open(path, "w") as f:
        f.write("# Image list with two lines of data per image:\n"
                "#   IMAGE_ID, QW, QX, QY, QZ, TX, TY, TZ, CAMERA_ID, NAME\n#   POINTS2D[] as (X, Y, POINT3D_ID)\n")
        for im in imgs.values():
            f.write(" ".join([str(im.id)] + ["%.17g" % v for v in (*im.qvec, *im.tvec)] + [str(im.camera_id), im.name]) + "\n")
            f.write(" ".join("%.17g %.17g %d" % (x, y, int(p)) for (x, y), p in zip(im.xys, im.point3D_ids)) + "\n")


def write_points3D_binary(path, xyz, rgb, err=None):
    xyz, rgb = np.asarray(xyz, np.float64).reshape(-1, 3), np.asarray(rgb).reshape(-1, 3)
    err = np.zeros(len(xyz)) if err is None else np.asarray(err, np.float64).reshape(-1)
    with open(path, "wb") as f:
        f.write(struct.pack("<Q", len(xyz)))
        for i in range(len(xyz)):
            f.write(struct.pack("<QdddBBBdQ", i + 1, *xyz[i], *(int(v) for v in rgb[i]), err[i], 0))


def write_points3D_text(path, xyz, rgb, err=None):
    xyz, rgb = np.asarray(xyz, np.float64).reshape(-1, 3), np.asarray(rgb).reshape(-1, 3)
    err = np.zeros(len(xyz)) if err is None else np.asarray(err, np.float64).reshape(-1)
    with open(path, "w") as f:
        f.write("# 3D point list with one line of data per point:\n"
                "#   POINT3D_ID, X, Y, Z, R, G, B, ERROR, TRACK[] as (IMAGE_ID, POINT2D_IDX)\n")
        for i in range(len(xyz)):
            f.write("%d %.17g %.17g %.17g %d %d %d %.17g\n" % (i + 1, *xyz[i], *(int(v) for v in rgb[i]), err[i]))


# ------------------------------------------------------------------------------------------------ scene reader
EDGE_DIRS = {"DexiNed": "edge_DexiNed"}   # readColmapCameras: 'DexiNed', and edge_PidiNet for ANY other string


def edge_map_path(path, images, name, detector):
    """readColmapCameras :114-124: the replacements act on the whole joined path, as the reference's do."""
    image_path = os.path.join(path, "images" if images is None else images, name)
    return image_path.replace("images", EDGE_DIRS.get(detector, "edge_PidiNet")).replace(".jpg", ".png")


def load_resolution(orig_w, orig_h, resolution):
    """loadCam :22-42 with resolution_scale = 1: the (width, height) the edge map is resized to."""
    if resolution in [1, 2, 3, 4, 8]:
        return round(orig_w / resolution), round(orig_h / resolution)
    if resolution == -1:
        global_down = orig_w / 1600 if orig_w > 1600 else 1
    else:
        global_down = orig_w / resolution
    scale = float(global_down)
    return int(orig_w / scale), int(orig_h / scale)


def load_edge_image(file, resolution):
    """loadCam :44-47 + PILtoTorch: an image with more than three bands keeps its first three, otherwise every band
    (``L`` -> [1,H,W], ``RGB`` -> [3,H,W]); no RGBA conversion, unlike readEMAP."""
    from PIL import Image
    image = Image.open(file)
    res = load_resolution(image.size[0], image.size[1], resolution)
    bands = image.split()
    if len(bands) > 3:
        return torch.cat([_pil_to_chw(b, res) for b in bands[:3]], dim=0).float()
    return _pil_to_chw(image, res).float()


def camera_from_colmap(intr, extr, image_chw, znear=0.01, zfar=100.0):
    """readColmapCameras :93-142 + Camera :18-66 for one image."""
    R = np.transpose(qvec2rotmat(extr.qvec))
    T = np.array(extr.tvec)
    if intr.model == "SIMPLE_PINHOLE":
        fx = fy = intr.params[0]
    elif intr.model in ("PINHOLE", "OPENCV"):   # OPENCV's distortion coefficients are ignored, as in the reference
        fx, fy = intr.params[0], intr.params[1]
    else:
        raise ValueError(f"COLMAP camera model {intr.model} not handled: only undistorted datasets (PINHOLE, "
                         "SIMPLE_PINHOLE or OPENCV cameras) are supported")
    fovy, fovx = focal2fov(fy, intr.height), focal2fov(fx, intr.width)
    # principal point at the image centre: the file's cx, cy are ignored (:129-135)
    K = np.array([[fx, 0, intr.width / 2.0], [0, fy, intr.height / 2.0], [0, 0, 1]])
    wv = torch.tensor(world2view(R, T)).transpose(0, 1)     # (the transposed view itself, as Camera inverts it)
    proj = projection_matrix(znear, zfar, fovx, fovy).transpose(0, 1)
    full = (wv.unsqueeze(0).bmm(proj.unsqueeze(0))).squeeze(0).contiguous()
    center = wv.inverse()[3, :3].contiguous()
    wv = wv.contiguous()
    H, W = int(image_chw.shape[1]), int(image_chw.shape[2])
    return EdgeCamera(intr.id, extr.name.replace(".jpg", ".png"), R, T, K, fovx, fovy, H, W, image_chw.clamp(0.0, 1.0),
                      wv, full, center, znear, zfar)


def read_model(sparse_dir):
    """(cameras, images): ``*.bin`` first, the ``*.txt`` twin when that fails (readColmapSceneInfo :165-174)."""
    try:
        return (read_cameras_binary(os.path.join(sparse_dir, "cameras.bin")),
                read_images_binary(os.path.join(sparse_dir, "images.bin")))
    except Exception:
        return (read_cameras_text(os.path.join(sparse_dir, "cameras.txt")),
                read_images_text(os.path.join(sparse_dir, "images.txt")))


def nerfpp_radius(cameras):
    """getNerfppNorm (dataset_readers.py:46-67): 1.1 x the largest distance of a camera centre from their mean, evaluated
    like the reference (getWorld2View2 returns float32, so the inverse and the centres are float32)."""
    centres = np.hstack([np.linalg.inv(world2view(c.R, c.T))[:3, 3:4] for c in cameras])
    dist = np.linalg.norm(centres - np.mean(centres, axis=1, keepdims=True), axis=0, keepdims=True)
    return float(np.max(dist) * 1.1)


def read_point_cloud(sparse_dir):
    """``points3D.ply`` when present (fetchPly: positions, colours / 255, normals).  DEVIATION: without it the reference
    leaves the cloud None and fails later in create_from_pcd; here the cloud is built from ``points3D.bin`` (or
    ``.txt``) instead, as upstream 3DGS does, with zero normals."""
    ply = os.path.join(sparse_dir, "points3D.ply")
    if os.path.exists(ply):
        v = read_ply_table(ply)
        pts = np.stack([v["x"], v["y"], v["z"]], 1).astype(np.float64)
        cols = np.stack([v["red"], v["green"], v["blue"]], 1).astype(np.float64) / 255.0
        nrm = (np.stack([v["nx"], v["ny"], v["nz"]], 1).astype(np.float64) if "nx" in v else np.zeros_like(pts))
        return BasicPointCloud(points=pts, colors=cols, normals=nrm)
    try:
        xyz, rgb, _ = read_points3D_binary(os.path.join(sparse_dir, "points3D.bin"))
    except Exception:
        xyz, rgb, _ = read_points3D_text(os.path.join(sparse_dir, "points3D.txt"))
    return BasicPointCloud(points=xyz, colors=rgb / 255.0, normals=np.zeros_like(xyz))


def test_image_names(path, cam_extrinsics, llffhold):
    """readColmapSceneInfo :196-207 with eval: every llffhold-th COLMAP name after sorting, or sparse/0/test.txt."""
    if llffhold:
        names = sorted(e.name for e in cam_extrinsics.values())
        return [n for i, n in enumerate(names) if i % llffhold == 0]
    with open(os.path.join(path, "sparse/0", "test.txt")) as f:
        return [line.strip() for line in f]


def _undistorted_maps(path, images, detector, resolution, extrs, intrs, backend):
    """The edge maps of read_colmap(undistort=True): loaded as ever, then resampled in as few calls as the op's chunks allow."""
    import warnings
    maps = [load_edge_image(edge_map_path(path, images, extr.name, detector), resolution) for extr in extrs]
    args = [distortion_of(intr, int(m.shape[2]), int(m.shape[1])) for intr, m in zip(intrs, maps)]
    maps, blank = undistort_images(maps, [a[0] for a in args], [a[1] for a in args], [a[3] for a in args],
                                   [a[2] for a in args], fill=0.0, backend=backend)
    for extr, m, n_blank in zip(extrs, maps, blank.tolist()):
        if n_blank > BLANK_WARN_FRACTION * m.shape[1] * m.shape[2]:
            warnings.warn(f"read_colmap: {n_blank} of the {m.shape[1] * m.shape[2]} pixels of {extr.name} are blank after "
                          "undistortion (no source pixel reaches them)")
    return maps


BLANK_WARN_FRACTION = 0.25   # read_colmap(undistort=True) warns about an image with more blank pixels than this


def read_colmap(path, images=None, eval=False, llffhold=8, detector="DexiNed", resolution=-1, undistort=False,
                undistort_backend="gpu"):
    """readColmapSceneInfo + loadCam for a COLMAP scan -> (train_cameras, test_cameras, point_cloud, cameras_extent).

    Reference behaviours kept exactly: R = qvec2rotmat(qvec)^T and T = tvec; FoV from the focal lengths (SIMPLE_PINHOLE
    f for both axes, PINHOLE / OPENCV fx and fy, OPENCV distortion ignored, other models raise); K with cx = w/2,
    cy = h/2; ``uid`` = the CAMERA id, so two images of one camera share it; the edge map at ``<path>/<images or
    'images'>/<name>`` with 'images' replaced by ``edge_DexiNed`` (``edge_PidiNet`` for any other detector) and '.jpg' by
    '.png' over the whole path; image_name = name with '.jpg' -> '.png'; cameras sorted by image_name.
    ``eval``: the test names are every ``llffhold``-th COLMAP name after sorting (``llffhold`` 0 reads
    ``sparse/0/test.txt``), and a camera is a test camera when its image_name is in that list -- so a '.jpg' image, whose
    image_name became '.png', is never one: a scan of '.jpg' names gets no test cameras, as in the reference.  The train
    list holds EVERY camera, the test ones included (:222).  ``resolution`` as loadCam (1/2/3/4/8: divide, -1: at most
    1600 px wide, otherwise a target width); the extent is getNerfppNorm's over the train list.

    K of a SIMPLE_PINHOLE camera uses f for both axes (the reference reuses the fy of the camera read before it, or fails
    on the first).  Mask images and depth parameters are not read.

    ``undistort=True`` (not in the reference, which reads undistorted scans only) accepts SIMPLE_RADIAL, RADIAL and
    FULL_OPENCV cameras too and honours the file's distortion coefficients and principal point: the edge maps are loaded
    as above, resize included, and then resampled by ``ops.undistort.undistort_images`` (``undistort_backend``: "gpu",
    HIP, the images stay on the device; "host", numpy) into the camera that is built here anyway -- the file's focal
    lengths, principal point at the centre.  Every EdgeCamera field except ``original_image`` is what a PINHOLE camera
    with the same focal lengths gives without the flag.  An image of which more than a quarter comes out blank (no source
    pixel reaches it) is reported with ``warnings.warn``."""
    sparse = os.path.join(path, "sparse/0")
    cam_intrinsics, cam_extrinsics = read_model(sparse)
    test_names = test_image_names(path, cam_extrinsics, llffhold) if eval else []
    extrs = list(cam_extrinsics.values())
    intrs = [cam_intrinsics[extr.camera_id] for extr in extrs]
    maps = _undistorted_maps(path, images, detector, resolution, extrs, intrs, undistort_backend) if undistort else None
    cams, is_test = [], []
    for k, (extr, intr) in enumerate(zip(extrs, intrs)):
        if undistort:
            # the camera of the resampled map: the output focal lengths distortion_of gives at the file's own size
            _, _, (fx, fy), _ = distortion_of(intr, intr.width, intr.height)
            intr = intr._replace(model="PINHOLE", params=np.array([fx, fy, intr.width / 2.0, intr.height / 2.0]))
            image = maps[k]
        else:
            image = load_edge_image(edge_map_path(path, images, extr.name, detector), resolution)
        cam = camera_from_colmap(intr, extr, image)
        cams.append(cam)
        is_test.append(cam.image_name in test_names)
    order = sorted(range(len(cams)), key=lambda i: cams[i].image_name)
    train = [cams[i] for i in order]
    test = [cams[i] for i in order if is_test[i]]
    return train, test, read_point_cloud(sparse), nerfpp_radius(train)


def write_colmap(path, cameras, edge_maps, points, binary=True, detector="DexiNed"):
    """Writes a COLMAP scan (sparse/0 model + one edge map per image) from cameras that carry world_view_transform /
    FoVx / FoVy (e.g. curve_gaussian_amd.synthetic cameras) and [1,H,W] or [H,W] edge maps in [0,1]: one PINHOLE camera
    per image (ids from 1, principal point at the centre), images ``<i:05d>.png``, `points` an [N,3] array or an
    (xyz [N,3], rgb [N,3] in 0..255) pair.  Inverse of read_colmap up to the 8-bit quantisation of the images."""
    from PIL import Image
    sparse = os.path.join(path, "sparse/0")
    edge_dir = os.path.join(path, EDGE_DIRS.get(detector, "edge_PidiNet"))
    os.makedirs(sparse, exist_ok=True)
    os.makedirs(edge_dir, exist_ok=True)
    cams, imgs = {}, {}
    for i, (cam, em) in enumerate(zip(cameras, edge_maps)):
        em = em.detach().cpu().float()
        em = em[0] if em.dim() == 3 else em
        H, W = int(em.shape[0]), int(em.shape[1])
        w2c = cam.world_view_transform.detach().cpu().double().numpy().T      # stored transposed (cameras.py:59)
        fx, fy = fov2focal(cam.FoVx, W), fov2focal(cam.FoVy, H)
        cams[i + 1] = ColmapCamera(i + 1, "PINHOLE", W, H, np.array([fx, fy, W / 2.0, H / 2.0]))
        name = f"{i:05d}.png"
        imgs[i + 1] = ColmapImage(i + 1, rotmat2qvec(w2c[:3, :3]), w2c[:3, 3].copy(), i + 1, name, np.zeros((0, 2)),
                                  np.zeros(0, np.int64))
        Image.fromarray((em.clamp(0, 1) * 255.0).round().to(torch.uint8).numpy(), mode="L").save(
            os.path.join(edge_dir, name))
    if isinstance(points, (tuple, list)):
        xyz, rgb = points
    else:
        xyz, rgb = points, np.full((len(points), 3), 128)
    xyz = np.asarray(xyz.detach().cpu().numpy() if torch.is_tensor(xyz) else xyz, np.float64)
    if binary:
        write_cameras_binary(os.path.join(sparse, "cameras.bin"), cams)
        write_images_binary(os.path.join(sparse, "images.bin"), imgs)
        write_points3D_binary(os.path.join(sparse, "points3D.bin"), xyz, rgb)
    else:
        write_cameras_text(os.path.join(sparse, "cameras.txt"), cams)
        write_images_text(os.path.join(sparse, "images.txt"), imgs)
        write_points3D_text(os.path.join(sparse, "points3D.txt"), xyz, rgb)
