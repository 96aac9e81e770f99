"""Shared inputs of the edge-score tests (test_edge_score_cpu.py, test_edge_score_gpu.py): masks for the distance transform,
a brute-force transform, points and cameras for the prediction mask, and a tiny synthetic scan whose edge maps are drawn
from the very lines its parametric_edges.json holds."""
import functools
import json
import math
import os

import numpy as np
import torch

EDT_INF = 2147483647
SHAPES = [(1, 1), (1, 130), (130, 1), (37, 70)]
DENSITIES = [0.01, 0.5]


def random_mask(shape, density, seed):
    return (np.random.default_rng(seed).random(shape) < density).astype(np.uint8)


def special_masks(shape):
    """empty, full, a single feature in a corner"""
    corner = np.zeros(shape, np.uint8)
    corner[-1, 0] = 1
    return {"empty": np.zeros(shape, np.uint8), "full": np.ones(shape, np.uint8), "corner": corner}


@functools.lru_cache(maxsize=None)
def edt_views():
    """{name: uint8 [H,W]}: random masks of every shape at both densities, and the special masks of every shape."""
    out = {}
    for k, shape in enumerate(SHAPES):
        for j, density in enumerate(DENSITIES):
            out[f"{shape[0]}x{shape[1]}_d{density}"] = random_mask(shape, density, 100 + 10 * k + j)
        for name, m in special_masks(shape).items():
            out[f"{shape[0]}x{shape[1]}_{name}"] = m
    return out


def edt_stacks(extra_shapes=()):
    """{name: uint8 [3,H,W]}: per shape, (density 0.01, density 0.5, corner) and (empty, full, corner rotated to the other
    corner) -- three views of different content per call."""
    out = {}
    for k, shape in enumerate(list(SHAPES) + list(extra_shapes)):
        sp = special_masks(shape)
        out[f"{shape[0]}x{shape[1]}_random"] = np.stack([random_mask(shape, 0.01, 300 + 10 * k), random_mask(shape, 0.5, 301 + 10 * k),
                                                        sp["corner"]])
        out[f"{shape[0]}x{shape[1]}_special"] = np.stack([sp["empty"], sp["full"], sp["corner"][::-1, ::-1].copy()])
    return out


def edt_brute(mask):
    """int32 [H,W]: the minimum over the feature pixels of dx^2 + dy^2, by trying them all."""
    m = np.asarray(mask) != 0
    H, W = m.shape
    fy, fx = np.nonzero(m)
    if fy.size == 0:
        return np.full((H, W), EDT_INF, np.int32)
    yy, xx = np.mgrid[0:H, 0:W]
    d2 = (yy.reshape(-1, 1) - fy[None, :]) ** 2 + (xx.reshape(-1, 1) - fx[None, :]) ** 2
    return d2.min(1).reshape(H, W).astype(np.int32)


# ------------------------------------------------------------------------------------------------ points and cameras
MASK_H, MASK_W = 45, 67


def mask_cameras():
    """3 cameras as (intrinsics [3,4], w2c [3,3,4]) float64: the third is the identity pose with fx = fy = 1, cx = cy = 0, so
    that u = X / Z exactly and points can be put ON the image bounds."""
    from curve_gaussian_amd import synthetic as S
    cams = S.fibonacci_cameras(2, MASK_H, MASK_W)
    intr, w2c = [], []
    for c in cams:
        m = c.world_view_transform.double().numpy().T
        intr.append([MASK_W / (2 * math.tan(c.FoVx / 2)), MASK_H / (2 * math.tan(c.FoVy / 2)), MASK_W / 2.0, MASK_H / 2.0])
        w2c.append(m[:3, :4])
    intr.append([1.0, 1.0, 0.0, 0.0])
    w2c.append(np.eye(4)[:3, :4])
    return np.array(intr, np.float64), np.array(w2c, np.float64)


def mask_points():
    """About 500 float32 points: a cloud around the unit cube (in front of the first two cameras, partly outside their
    images), points behind every camera, points exactly on u = 0, u = width, v = 0 and v = height of the third camera, and
    runs of points that share a pixel."""
    rng = np.random.default_rng(7)
    cloud = rng.uniform(-0.6, 1.6, (380, 3))
    far = rng.uniform(-40.0, 40.0, (40, 3))                       # most of them behind one camera or another
    z = np.array([1.0, 2.0, 4.0, 0.5])
    on_u0 = np.stack([0.0 * z, 3.0 * z, z], 1)                    # u = 0: kept
    on_uw = np.stack([MASK_W * z, 3.0 * z, z], 1)                 # u = width: dropped
    on_v0 = np.stack([5.0 * z, 0.0 * z, z], 1)                    # v = 0: kept
    on_vh = np.stack([5.0 * z, MASK_H * z, z], 1)                 # v = height: dropped
    behind = np.stack([5.0 * z, 5.0 * z, -z], 1)                  # c2 < 0
    at_eye = np.array([[1.0, 1.0, 0.0]])                          # c2 = 0
    same = np.array([0.5, 0.5, 0.5]) + rng.uniform(-1e-4, 1e-4, (40, 3))   # a few pixels, many points each
    third = np.stack([rng.uniform(0, MASK_W, 30) * 2.0, rng.uniform(0, MASK_H, 30) * 2.0, np.full(30, 2.0)], 1)
    return np.concatenate([cloud, far, on_u0, on_uw, on_v0, on_vh, behind, at_eye, same, third]).astype(np.float32)


# ------------------------------------------------------------------------------------------------ masks to score
def score_stack(seed=11, V=4, H=37, W=70):
    """(pred, det) uint8 [V,H,W]: random sparse masks; view 1 has an empty prediction, view 2 an empty detection."""
    rng = np.random.default_rng(seed)
    pred = (rng.random((V, H, W)) < 0.03).astype(np.uint8)
    det = (rng.random((V, H, W)) < 0.05).astype(np.uint8)
    pred[1] = 0
    det[2] = 0
    return pred, det


# ------------------------------------------------------------------------------------------------ a tiny scan
SCAN_H, SCAN_W, SCAN_VIEWS = 48, 64, 3
SCAN_RESOLUTION = 0.004   # about a quarter of a pixel at these cameras
SCAN_EDGES = {
    "lines_end_pts": [[0.2, 0.2, 0.2, 0.8, 0.25, 0.3], [0.8, 0.25, 0.3, 0.75, 0.8, 0.7], [0.3, 0.7, 0.2, 0.25, 0.3, 0.8]],
    "curves_ctl_pts": [[0.2, 0.8, 0.8, 0.4, 0.9, 0.5, 0.6, 0.5, 0.6, 0.8, 0.6, 0.8]],
}


def scan_cameras():
    from curve_gaussian_amd import synthetic as S
    return S.fibonacci_cameras(SCAN_VIEWS, SCAN_H, SCAN_W)


def drawn_edge_maps(detector):
    """The edge maps of the scan, [1,H,W] float in [0,1]: the points of SCAN_EDGES at SCAN_RESOLUTION projected with plain
    float64 matrix products, 1 where a point falls (0 for DexiNed, whose maps are dark where the edge is)."""
    from curve_gaussian_amd.edge_extraction.abc import pred_points_and_directions
    pts = pred_points_and_directions(SCAN_EDGES, SCAN_RESOLUTION).points.astype(np.float32).astype(np.float64)
    maps = []
    for c in scan_cameras():
        w2c = c.world_view_transform.double().numpy().T
        cam = pts @ w2c[:3, :3].T + w2c[:3, 3]
        fx, fy = SCAN_W / (2 * math.tan(c.FoVx / 2)), SCAN_H / (2 * math.tan(c.FoVy / 2))
        u = fx * cam[:, 0] / cam[:, 2] + SCAN_W / 2.0
        v = fy * cam[:, 1] / cam[:, 2] + SCAN_H / 2.0
        ok = (cam[:, 2] > 0) & (u >= 0) & (u < SCAN_W) & (v >= 0) & (v < SCAN_H)
        m = np.zeros((SCAN_H, SCAN_W), np.float32)
        m[np.floor(v[ok]).astype(int), np.floor(u[ok]).astype(int)] = 1.0
        assert m.sum() > 20, "the scan's lines must be in view"
        maps.append(torch.from_numpy(1.0 - m if detector == "DexiNed" else m).unsqueeze(0))
    return maps


def write_scan(root, layout, detector, scan="room", with_prediction=True):
    """<root>/data/<scan> in the given layout with drawn edge maps, and <root>/out/<scan>/parametric_edges.json.
    Returns (base_dir, dataset_dir)."""
    from curve_gaussian_amd.scene import colmap_io as CIO
    from curve_gaussian_amd.scene import dataset_io as IO
    data, out = os.path.join(str(root), "data"), os.path.join(str(root), "out")
    scan_dir = os.path.join(data, scan)
    if layout == "colmap":
        CIO.write_colmap(scan_dir, scan_cameras(), drawn_edge_maps(detector), np.full((4, 3), 0.5), detector=detector)
    else:
        IO.write_emap(scan_dir, scan_cameras(), drawn_edge_maps(detector), detector=detector)
    os.makedirs(os.path.join(out, scan), exist_ok=True)
    if with_prediction:
        with open(os.path.join(out, scan, "parametric_edges.json"), "w") as f:
            json.dump(SCAN_EDGES, f)
    return out, data
