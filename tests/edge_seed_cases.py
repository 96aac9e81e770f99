"""Shared inputs of the edge-seed tests (test_edge_seed_cpu.py, test_edge_seed_gpu.py): distance transforms to pack, cameras
and masks to vote with, a grid whose centres sit ON the image bounds of the identity camera, and the drawn scan of
edge_score_cases seen from six cameras."""
import functools
import math
import os

import numpy as np
import torch

import edge_score_cases as EC

EDT_INF = EC.EDT_INF
MASK_H, MASK_W = EC.MASK_H, EC.MASK_W
BITS_WIDTHS = [1, 31, 32, 33, 67]
BITS_HEIGHT = 5


def bits_dist2(width, seed=0):
    """int32 [3,BITS_HEIGHT,width]: squared distances 0..8 around the tolerances 0 and 4; the last view has no feature."""
    d2 = np.random.default_rng(100 + width + seed).integers(0, 9, (3, BITS_HEIGHT, width)).astype(np.int32)
    d2[2] = EDT_INF
    return d2


# ------------------------------------------------------------------------------------------------ cameras and masks to vote with
VOTE_BOUNDS = ((-1.0, -0.75, -1.0), (2.0, 2.5, 2.25))   # around the unit cube; reaches behind the identity camera (z <= 0)
VOTE_GRIDS = [(1, 1, 1), (63, 1, 1), (65, 3, 2), (257, 2, 1)]
VOTE_VIEWS = [1, 3, 40]


@functools.lru_cache(maxsize=None)
def vote_cameras(V):
    """(intrinsics [V,4], w2c [V,3,4]) float64.  The LAST camera is always the identity camera of ``mask_cameras`` (u = X / Z:
    the boundary camera); V = 3 is ``mask_cameras`` itself, V = 40 puts 39 cameras on the sphere in front of it."""
    K3, M3 = EC.mask_cameras()
    if V == 1:
        return K3[2:], M3[2:]
    if V == 3:
        return K3, M3
    from curve_gaussian_amd import synthetic as S
    intr, w2c = [], []
    for c in S.fibonacci_cameras(V - 1, MASK_H, MASK_W):
        intr.append([MASK_W / (2 * math.tan(c.FoVx / 2)), MASK_H / (2 * math.tan(c.FoVy / 2)), MASK_W / 2.0, MASK_H / 2.0])
        w2c.append(c.world_view_transform.double().numpy().T[:3, :4])
    return np.concatenate([np.array(intr), K3[2:]]), np.concatenate([np.array(w2c), M3[2:]])


@functools.lru_cache(maxsize=None)
def vote_masks(V, density=0.03, seed=5):
    """uint8 [V,MASK_H,MASK_W] random masks; view 1 (when there is one) is empty."""
    m = (np.random.default_rng(seed + V).random((V, MASK_H, MASK_W)) < density).astype(np.uint8)
    if V > 1:
        m[1] = 0
    return m


# A grid for the identity camera (fx = fy = 1, cx = cy = 0: u = X / Z, v = Y / Z, image 67 x 45).  Every centre is exact in
# float32: X in {0, 33.5, 67, 100.5}, Y in {0, 22.5, 45, 67.5}, Z in {-1, 0, 1}.  At Z = 1: u = 0 and v = 0 are kept,
# u = 67 = W and v = 45 = H are dropped; Z = 0 (c2 = 0) and Z = -1 (c2 < 0) are dropped.
BOUNDARY_DIMS = (4, 4, 3)
BOUNDARY_BOUNDS = ((-16.75, -11.25, -1.5), (117.25, 78.75, 1.5))


def boundary_expected_seen():
    seen = np.zeros(BOUNDARY_DIMS[::-1], np.uint16)   # [k][j][i]
    seen[2, :2, :2] = 1
    return seen.reshape(-1)


# ------------------------------------------------------------------------------------------------ the drawn scan, six views
SEED_VIEWS = 6
SEED_H, SEED_W = EC.SCAN_H, EC.SCAN_W
SEED_BOUNDS = ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
SEED_GRID, SEED_CELL = 32, 2
# ceil(the largest pixel distance, over the sampled points and the six views, between a point's pixel and the pixel of its
# voxel's centre) + 1: the distance is 2.0 (computed by ``seed_pixel_distance``, asserted in test_edge_seed_cpu.py)
SEED_TOL_PX = 3


def seed_cameras():
    from curve_gaussian_amd import synthetic as S
    return S.fibonacci_cameras(SEED_VIEWS, SEED_H, SEED_W)


@functools.lru_cache(maxsize=None)
def seed_points_sampled():
    """float64 [n,3]: the points of SCAN_EDGES that ``drawn_edge_maps`` draws (float32 values)."""
    from curve_gaussian_amd.edge_extraction.abc import pred_points_and_directions
    return pred_points_and_directions(EC.SCAN_EDGES, EC.SCAN_RESOLUTION).points.astype(np.float32).astype(np.float64)


def _project(c, pts):
    """``drawn_edge_maps``' projection: plain float64 matrix products.  (u, v, depth)."""
    w2c = c.world_view_transform.double().numpy().T
    cam = pts @ w2c[:3, :3].T + w2c[:3, 3]
    fx, fy = SEED_W / (2 * math.tan(c.FoVx / 2)), SEED_H / (2 * math.tan(c.FoVy / 2))
    return fx * cam[:, 0] / cam[:, 2] + SEED_W / 2.0, fy * cam[:, 1] / cam[:, 2] + SEED_H / 2.0, cam[:, 2]


def seed_edge_maps(detector):
    """One [1,H,W] float map per camera of ``seed_cameras``, drawn as ``edge_score_cases.drawn_edge_maps`` draws its three."""
    maps = []
    for c in seed_cameras():
        u, v, z = _project(c, seed_points_sampled())
        ok = (z > 0) & (u >= 0) & (u < SEED_W) & (v >= 0) & (v < SEED_H)
        m = np.zeros((SEED_H, SEED_W), np.float32)
        m[np.floor(v[ok]).astype(int), np.floor(u[ok]).astype(int)] = 1.0
        assert m.sum() > 20, "the scan's lines must be in view"
        maps.append(torch.from_numpy(1.0 - m if detector == "DexiNed" else m).unsqueeze(0))
    return maps


def seed_voxel_centres():
    """float64 [n,3]: for every sampled point, the (float32) centre of the voxel of the SEED_GRID^3 grid that holds it."""
    lo, hi = (np.array(b, np.float64) for b in SEED_BOUNDS)
    step = (hi - lo) / SEED_GRID
    ijk = np.floor((seed_points_sampled() - lo) / step)
    return (lo + (ijk + 0.5) * step).astype(np.float32).astype(np.float64)


def seed_pixel_distance():
    """(the largest distance between a point's pixel and its voxel centre's pixel over points and views -- neither clipped
    to the image --, excluded bool [n]: the centre's pixel is outside an image or within SEED_TOL_PX of its border in
    some view)."""
    pts, cen = seed_points_sampled(), seed_voxel_centres()
    worst, excluded = 0.0, np.zeros(len(pts), bool)
    for c in seed_cameras():
        u, v, z = _project(c, pts)
        uc, vc, zc = _project(c, cen)
        assert (z > 0).all() and (zc > 0).all()
        pu, pv = np.floor(uc), np.floor(vc)
        worst = max(worst, float(np.hypot(np.floor(u) - pu, np.floor(v) - pv).max()))
        excluded |= (pu < SEED_TOL_PX) | (pu > SEED_W - 1 - SEED_TOL_PX) | (pv < SEED_TOL_PX) | (pv > SEED_H - 1 - SEED_TOL_PX)
    return worst, excluded


def seed_novel_cameras(detector="PidiNet"):
    """(NovelViewCamera s, uint8 maps) of the drawn scan, without a file in between."""
    from curve_gaussian_amd.edge_extraction.novel_view import NovelViewCamera
    cams = []
    for k, c in enumerate(seed_cameras()):
        w2c = c.world_view_transform.double().numpy().T
        cams.append(NovelViewCamera(f"v{k}", np.ascontiguousarray(w2c[:3, :3]), w2c[:3, 3].copy(),
                                    SEED_W / (2 * math.tan(c.FoVx / 2)), SEED_H / (2 * math.tan(c.FoVy / 2)), SEED_W / 2.0,
                                    SEED_H / 2.0, SEED_W, SEED_H))
    maps = [(m[0].numpy() * 255.0).round().astype(np.uint8) for m in seed_edge_maps(detector)]
    return cams, maps


SEED_OPTIONS = dict(grid=SEED_GRID, tol_px=SEED_TOL_PX, cell=SEED_CELL)


def sfm_points():
    """A stand-in SfM cloud for the COLMAP twin: 200 points uniform in the unit cube."""
    return np.random.default_rng(3).uniform(0.0, 1.0, (200, 3))


def write_seed_scan(root, layout, detector="DexiNed"):
    """The drawn scan, six views, as <root>/<layout>_scan in the given layout.  Returns its directory."""
    from curve_gaussian_amd.scene import colmap_io as CIO
    from curve_gaussian_amd.scene import dataset_io as IO
    scan_dir = os.path.join(str(root), f"{layout}_scan")
    if layout == "colmap":
        CIO.write_colmap(scan_dir, seed_cameras(), seed_edge_maps(detector), sfm_points(), detector=detector)
    else:
        IO.write_emap(scan_dir, seed_cameras(), seed_edge_maps(detector), detector=detector)
    return scan_dir
