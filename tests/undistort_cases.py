"""Shared by tests/test_undistort_cpu.py and tests/test_undistort_gpu.py: a small distorted COLMAP scan on disk, its PINHOLE
twin (cameras written out by hand), and the views of the parity test."""
import os

import numpy as np
import torch

from curve_gaussian_amd.scene import colmap_io as CIO

SCAN_W, SCAN_H = 48, 36
# camera id -> (model, params): one SIMPLE_RADIAL (f, cx, cy, k) and one OPENCV (fx, fy, cx, cy, k1, k2, p1, p2) camera
SCAN_CAMERAS = {
    1: ("SIMPLE_RADIAL", [40.0, 25.3, 17.1, -0.15]),
    2: ("OPENCV", [42.0, 39.0, 22.6, 19.4, -0.1, 0.02, 0.01, -0.015]),
}
# the same scan as a reader without the flag must see it after undistortion, written out by hand: PINHOLE cameras with the
# focal lengths above (f for both axes of SIMPLE_RADIAL) and the principal point at the centre of the 48 x 36 frame
TWIN_CAMERAS = {
    1: ("PINHOLE", [40.0, 40.0, 24.0, 18.0]),
    2: ("PINHOLE", [42.0, 39.0, 24.0, 18.0]),
}
SCAN_IMAGES = [("00000.png", 1), ("00001.png", 2), ("00002.png", 2)]   # (name, camera id)


def edge_map(seed, height=SCAN_H, width=SCAN_W):
    """An 8-bit map of a few soft curves plus noise, [H,W] uint8."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:height, 0:width]
    img = np.zeros((height, width))
    for _ in range(4):
        cx, cy, r = rng.uniform(0, width), rng.uniform(0, height), rng.uniform(5, 20)
        img += np.exp(-0.5 * ((np.hypot(xx - cx, yy - cy) - r) / 1.2) ** 2)
    img = np.clip(img + 0.05 * rng.random((height, width)), 0, 1)
    return (img * 255).round().astype(np.uint8)


def write_scan(path, cameras=SCAN_CAMERAS):
    """Three images, two cameras (id -> (model, params)), a few points."""
    from PIL import Image
    sparse, edges = os.path.join(path, "sparse/0"), os.path.join(path, "edge_DexiNed")
    os.makedirs(sparse, exist_ok=True)
    os.makedirs(edges, exist_ok=True)
    cams = {}
    for cid, (model, params) in cameras.items():
        cams[cid] = CIO.ColmapCamera(cid, model, SCAN_W, SCAN_H, np.array(params, np.float64))
    imgs = {}
    for k, (name, cid) in enumerate(SCAN_IMAGES):
        ang = 0.3 * k
        R = np.array([[np.cos(ang), 0, np.sin(ang)], [0, 1, 0], [-np.sin(ang), 0, np.cos(ang)]])
        imgs[k + 1] = CIO.ColmapImage(k + 1, CIO.rotmat2qvec(R), np.array([0.1 * k, -0.05, 2.0 + 0.2 * k]), cid, name,
                                      np.zeros((0, 2)), np.zeros(0, np.int64))
        Image.fromarray(edge_map(k), mode="L").save(os.path.join(edges, name))
    CIO.write_cameras_binary(os.path.join(sparse, "cameras.bin"), cams)
    CIO.write_images_binary(os.path.join(sparse, "images.bin"), imgs)
    rng = np.random.default_rng(7)
    CIO.write_points3D_binary(os.path.join(sparse, "points3D.bin"), rng.uniform(-0.5, 0.5, (40, 3)),
                              rng.integers(0, 255, (40, 3)))
    return path


# ---- the parity views: (model id, channels, H, W, (fx, fy, cx, cy), (out_fx, out_fy), coefficients), one per supported model
# plus a second OPENCV view.  37x53 and 53x37: odd sizes; 1x1: smaller than a workgroup; 64x64: whole workgroups; 70x130:
# a partial last workgroup.  The 1x1 and 64x64 views look mostly past the source, so blank pixels and fill taps occur.
PARITY_VIEWS = [
    (2, 1, 37, 53, (41.3, 41.3, 27.9, 17.7), (41.3, 41.3), (-0.15,)),
    (4, 3, 53, 37, (33.7, 35.1, 17.2, 27.9), (33.7, 35.1), (-0.12, 0.03, 0.011, -0.017)),
    (1, 2, 1, 1, (1.7, 1.9, 0.83, 0.41), (1.7, 1.9), ()),
    (6, 4, 64, 64, (50.3, 49.1, 37.3, 12.9), (47.7, 46.9), (0.21, -0.04, 0.004, 0.006, 0.013, 0.07, -0.02, 0.003)),
    (3, 1, 70, 130, (90.7, 90.7, 66.1, 33.8), (90.7, 90.7), (-0.2, 0.05)),
    (4, 1, 37, 53, (39.9, 44.4, 20.3, 25.6), (39.9, 44.4), (0.3, 0.1, -0.02, 0.025)),
    (0, 1, 16, 24, (20.3, 20.3, 14.7, 6.2), (20.3, 20.3), ()),
]


def parity_inputs(views=PARITY_VIEWS, seed=0):
    g = torch.Generator().manual_seed(seed)
    images = [torch.rand(c, h, w, generator=g) for _m, c, h, w, *_ in views]
    return (images, [v[0] for v in views], [v[4] for v in views], [v[6] for v in views], [v[5] for v in views])
