#!/usr/bin/env python
"""Generates the COLMAP scan fixture: a small scan under tests/golden/colmap/ (sparse/0 binary model, its text twin,
points3D.ply, test.txt, and edge maps under edge_DexiNed/ and edge_PidiNet/) and tests/golden/colmap/colmap.npz, by
IMPORTING the reference's scene/colmap_loader.py, scene/dataset_readers.py, utils/camera_utils.py and scene/cameras.py
and calling them on CPU (runs only where the reference checkout exists; the fixture files travel, the reference does not).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_colmap_golden.py

What is called: read_intrinsics_binary, read_extrinsics_binary, read_points3D_binary, read_extrinsics_text,
read_points3D_text (colmap_loader.py), readColmapSceneInfo (dataset_readers.py:160-249, eval False / True, llffhold 8, 3
and 0, both detectors) and loadCam + Camera (camera_utils.py:22-67, cameras.py:18-66, resolution -1 and 2).  The model
files themselves are written by this project's colmap_io writers.

How it is imported: through make_model_golden.import_reference, with placeholders for the packages this image lacks
(open3d, plyfile, cv2, ...), poisoned before anything is called; Camera's ``.cuda()`` / ``.to("cuda")`` run on the CPU
under a TorchFunctionMode.  Not pinned through the reference: read_intrinsics_text (it asserts PINHOLE, and the scan
holds three models) and fetchPly (plyfile is absent: the reference's cloud is then None) -- the expected cloud of
points3D.ply is the arrays this script writes."""
import contextlib
import io
import os
import shutil
import sys

import numpy as np
import torch
from PIL import Image
from torch.overrides import TorchFunctionMode

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, ROOT)
from make_model_golden import _ARMED, import_reference  # noqa: E402

from curve_gaussian_amd.scene import colmap_io as CI  # noqa: E402

OUT = os.path.join(HERE, "colmap")


class CudaOnCpu(TorchFunctionMode):
    """Tensor.cuda() and .to('cuda') stay on the CPU."""

    def __torch_function__(self, func, types, args=(), kwargs=None):
        kwargs = dict(kwargs or {})
        if func is torch.Tensor.cuda:
            return args[0]
        if func is torch.Tensor.to:
            args = tuple("cpu" if (isinstance(a, (str, torch.device)) and str(a).startswith("cuda")) else a for a in args)
            if "device" in kwargs and str(kwargs["device"]).startswith("cuda"):
                kwargs["device"] = "cpu"
        return func(*args, **kwargs)


def quat(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    return q if q[0] > 0 else -q


def edge_png(rng, w, h, mode):
    a = np.zeros((h, w, 4), np.uint8)
    for _ in range(max(3, w // 12)):                       # a few strokes, the rest black: small files
        y, x, n = rng.integers(0, h), rng.integers(0, w), rng.integers(3, 12)
        a[y, x:x + n, :] = rng.integers(60, 256, size=4)
        a[y:y + n, x, :] = rng.integers(60, 256, size=4)
    a[..., 3] = np.where(a[..., 3] > 0, a[..., 3], 255)
    if mode == "L":
        return Image.fromarray(a[..., 0], mode="L")
    return Image.fromarray(a[..., :3] if mode == "RGB" else a, mode=mode)


def write_scan(rng):
    shutil.rmtree(OUT, ignore_errors=True)
    sparse = os.path.join(OUT, "sparse/0")
    os.makedirs(sparse)
    cams = {
        2: CI.ColmapCamera(2, "PINHOLE", 48, 32, np.array([40.0, 44.0, 23.0, 17.5])),
        1: CI.ColmapCamera(1, "SIMPLE_PINHOLE", 48, 32, np.array([38.0, 20.0, 15.0])),
        3: CI.ColmapCamera(3, "OPENCV", 48, 32, np.array([36.0, 39.0, 24.5, 16.0, 0.1, -0.05, 0.001, 0.002])),
        7: CI.ColmapCamera(7, "PINHOLE", 1700, 20, np.array([900.0, 880.0, 850.0, 10.0])),
        5: CI.ColmapCamera(5, "PINHOLE", 40, 30, np.array([33.0, 31.0, 20.0, 15.0])),
    }
    # (image id, camera id, name, edge-map mode); ids not in name order; images 12 and 15 share camera 2
    spec = [(12, 2, "frame_004.jpg", "L"), (3, 1, "frame_000.png", "RGB"), (15, 2, "frame_008.png", "RGBA"),
            (4, 3, "frame_001.jpg", "RGBA"), (9, 5, "frame_002.png", "L"), (1, 7, "frame_009.png", "L"),
            (20, 5, "frame_003.png", "RGB"), (6, 3, "frame_006.jpg", "L"), (2, 1, "frame_005.png", "L"),
            (30, 5, "frame_007.png", "RGBA")]
    imgs = {}
    for iid, cid, name, mode in spec:
        npts = int(rng.integers(0, 3))
        imgs[iid] = CI.ColmapImage(iid, quat(rng), rng.normal(size=3), cid, name, rng.uniform(0, 40, (npts, 2)),
                                   rng.integers(-1, 50, npts))
        c = cams[cid]
        for det in ("edge_DexiNed", "edge_PidiNet"):
            os.makedirs(os.path.join(OUT, det), exist_ok=True)
            edge_png(rng, c.width, c.height, mode).save(os.path.join(OUT, det, name.replace(".jpg", ".png")))
    CI.write_cameras_binary(os.path.join(sparse, "cameras.bin"), cams)
    CI.write_images_binary(os.path.join(sparse, "images.bin"), imgs)
    CI.write_cameras_text(os.path.join(sparse, "cameras.txt"), cams)
    CI.write_images_text(os.path.join(sparse, "images.txt"), imgs)
    xyz = rng.normal(size=(40, 3))
    rgb = rng.integers(0, 256, (40, 3))
    err = rng.uniform(0, 2, 40)
    CI.write_points3D_binary(os.path.join(sparse, "points3D.bin"), xyz, rgb, err)
    CI.write_points3D_text(os.path.join(sparse, "points3D.txt"), xyz, rgb, err)
    # points3D.ply in storePly's layout (dataset_readers.py:148-158): float xyz, float normals, uchar colours
    ply_xyz = rng.normal(size=(25, 3)).astype("<f4")
    ply_nrm = rng.normal(size=(25, 3)).astype("<f4")
    ply_rgb = rng.integers(0, 256, (25, 3)).astype("u1")
    dt = np.dtype([(n, "<f4") for n in ("x", "y", "z", "nx", "ny", "nz")] + [(n, "u1") for n in ("red", "green", "blue")])
    tab = np.empty(25, dt)
    for i, n in enumerate(("x", "y", "z")):
        tab[n], tab["n" + n] = ply_xyz[:, i], ply_nrm[:, i]
    for i, n in enumerate(("red", "green", "blue")):
        tab[n] = ply_rgb[:, i]
    with open(os.path.join(sparse, "points3D.ply"), "wb") as f:
        f.write(("ply\nformat binary_little_endian 1.0\nelement vertex 25\n" + "".join(
            f"property {'uchar' if n in ('red', 'green', 'blue') else 'float'} {n}\n" for n in dt.names)
            + "end_header\n").encode("ascii"))
        f.write(tab.tobytes())
    with open(os.path.join(sparse, "test.txt"), "w") as f:
        f.write("frame_002.png\nframe_007.png\nframe_001.jpg\n")
    return {"ply_points": ply_xyz.astype(np.float64), "ply_colors": ply_rgb.astype(np.float64) / 255.0,
            "ply_normals": ply_nrm.astype(np.float64)}


class Args:
    def __init__(self, resolution):
        self.resolution = resolution
        self.data_device = "cpu"


def main():
    rng = np.random.default_rng(20261016)
    out = write_scan(rng)
    import_reference("scene")     # (the package first: utils.camera_utils and scene/__init__.py import each other)
    LDR = import_reference("scene.colmap_loader")
    DR = import_reference("scene.dataset_readers")
    CU = import_reference("utils.camera_utils")
    _ARMED[0] = True
    sparse = os.path.join(OUT, "sparse/0")
    intr = LDR.read_intrinsics_binary(os.path.join(sparse, "cameras.bin"))
    for k in sorted(intr):
        c = intr[k]
        out[f"cam{k}_model"], out[f"cam{k}_wh"], out[f"cam{k}_params"] = np.array(c.model), np.array([c.width, c.height]), c.params
    out["cam_ids"] = np.array(sorted(intr))
    for tag, ext in (("bin", LDR.read_extrinsics_binary(os.path.join(sparse, "images.bin"))),
                     ("txt", LDR.read_extrinsics_text(os.path.join(sparse, "images.txt")))):
        ids = list(ext)
        out[f"img_{tag}_ids"] = np.array(ids)
        out[f"img_{tag}_names"] = np.array([ext[i].name for i in ids])
        out[f"img_{tag}_camera_ids"] = np.array([ext[i].camera_id for i in ids])
        out[f"img_{tag}_qvec"] = np.stack([ext[i].qvec for i in ids])
        out[f"img_{tag}_tvec"] = np.stack([ext[i].tvec for i in ids])
        out[f"img_{tag}_xys"] = np.concatenate([ext[i].xys.reshape(-1, 2) for i in ids])
        out[f"img_{tag}_p3d"] = np.concatenate([ext[i].point3D_ids.reshape(-1) for i in ids]).astype(np.int64)
    for tag, (xyz, rgb, err) in (("bin", LDR.read_points3D_binary(os.path.join(sparse, "points3D.bin"))),
                                 ("txt", LDR.read_points3D_text(os.path.join(sparse, "points3D.txt")))):
        out[f"p3d_{tag}_xyz"], out[f"p3d_{tag}_rgb"], out[f"p3d_{tag}_err"] = xyz, rgb, err
    configs = []
    for det in ("DexiNed", "PidiNet"):
        for ev, hold in ((False, 8), (True, 8), (True, 3), (True, 0)):
            with contextlib.redirect_stdout(io.StringIO()):
                si = DR.readColmapSceneInfo(OUT, None, "", ev, False, llffhold=hold, detector=det)
            key = f"{det}_{int(ev)}_{hold}"
            configs.append(key)
            assert si.point_cloud is None       # fetchPly needs plyfile, which is absent here
            out[key + "_train"] = np.array([c.image_name for c in si.train_cameras])
            out[key + "_test"] = np.array([c.image_name for c in si.test_cameras])
            out[key + "_is_test"] = np.array([c.is_test for c in si.train_cameras])
            out[key + "_uid"] = np.array([c.uid for c in si.train_cameras])
            out[key + "_R"] = np.stack([c.R for c in si.train_cameras])
            out[key + "_T"] = np.stack([c.T for c in si.train_cameras])
            out[key + "_fovx"] = np.array([c.FovX for c in si.train_cameras])
            out[key + "_fovy"] = np.array([c.FovY for c in si.train_cameras])
            out[key + "_K"] = np.stack([c.K for c in si.train_cameras])
            out[key + "_extent"] = np.array(si.nerf_normalization["radius"])
            if ev and hold == 8:
                for res in (-1, 2):
                    with CudaOnCpu(), contextlib.redirect_stdout(io.StringIO()):
                        loaded = [CU.loadCam(Args(res), i, c, 1.0) for i, c in enumerate(si.train_cameras)]
                    for i, cam in enumerate(loaded):
                        k = f"{det}_r{res}_{i}"
                        out[k + "_image"] = cam.original_image.numpy().astype(np.float32)
                        out[k + "_wv"] = cam.world_view_transform.numpy()
                        out[k + "_full"] = cam.full_proj_transform.numpy()
                        out[k + "_center"] = cam.camera_center.numpy()
    out["configs"] = np.array(configs)
    np.savez_compressed(os.path.join(OUT, "colmap.npz"), **out)
    print("wrote", OUT, "files:", sum(len(f) for _, _, f in os.walk(OUT)),
          "npz bytes:", os.path.getsize(os.path.join(OUT, "colmap.npz")))


if __name__ == "__main__":
    main()
