"""Shared inputs of the edge-direction tests (test_edge_dir_cpu.py, test_edge_dir_gpu.py): synthetic tubes of kept voxels
around a line, the grids, masks and centres the moments kernel is held to, and a drawn scan whose tubes are thin enough
to have a direction."""
import functools
import itertools
import math

import numpy as np

import edge_score_cases as EC
import edge_seed_cases as SC

# ------------------------------------------------------------------------------------------------ tubes around a line
TUBE_DIMS = (17, 17, 17)
TUBE_CENTRE = (8, 8, 8)
TUBE_RADIUS = 1.5       # voxels, around the line
BALL_RADIUS = 6         # dir_radius


def lattice_directions():
    """The 13 lattice directions up to sign: 3 axes, 6 face diagonals, 4 body diagonals; the first non-zero entry is +1."""
    out = []
    for v in itertools.product((-1, 0, 1), repeat=3):
        nz = [c for c in v if c != 0]
        if nz and nz[0] == 1:
            out.append(v)
    assert len(out) == 13
    return out


def tube_mask(direction, offset=(0.0, 0.0, 0.0), tube_radius=TUBE_RADIUS, dims=TUBE_DIMS, centre=TUBE_CENTRE):
    """bool [nx ny nz] (x fastest): the voxels whose centre lies within ``tube_radius`` voxels of the line through the
    centre of voxel ``centre`` shifted by ``offset``, along ``direction``."""
    nx, ny, nz = dims
    d = np.asarray(direction, np.float64)
    d = d / np.linalg.norm(d)
    k, j, i = np.meshgrid(np.arange(nz), np.arange(ny), np.arange(nx), indexing="ij")
    q = np.stack([i, j, k], -1).astype(np.float64) - (np.asarray(centre, np.float64) + np.asarray(offset, np.float64))
    along = q @ d
    dist2 = (q * q).sum(-1) - along * along
    return (dist2 <= tube_radius * tube_radius).reshape(-1)


def angle_deg(a, b):
    """The angle in degrees between the lines along a and b (rows), sign ignored."""
    a, b = np.atleast_2d(a), np.atleast_2d(b)
    c = np.abs((a * b).sum(1)) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1))
    return np.degrees(np.arccos(np.clip(c, 0.0, 1.0)))


def generic_tubes(n=100, seed=0):
    """(directions [n,3] unit, offsets [n,3] in [-0.5, 0.5)) from default_rng(seed)."""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return d, rng.uniform(-0.5, 0.5, (n, 3))


# ------------------------------------------------------------------------------------------------ grids for the moments kernel
MOMENT_GRIDS = [(1, 1, 1), (5, 4, 3), (31, 3, 2), (33, 5, 4), (64, 6, 5), (70, 9, 7)]
MOMENT_RADII = [1, 6, 15]
MOMENT_MASKS = ["d0.05", "d0.5", "zeros", "ones"]
MOMENT_COUNTS = [0, 1, 3, 4, 5, 257]
BIG_DIMS = (33, 33, 33)   # all-one at r = 15: the largest sums


def moment_mask(dims, kind, seed=0):
    """bool [nx ny nz]: random at the density of ``kind`` ("d0.05", "d0.5"), all-zero or all-one."""
    n = dims[0] * dims[1] * dims[2]
    if kind == "zeros":
        return np.zeros(n, bool)
    if kind == "ones":
        return np.ones(n, bool)
    return np.random.default_rng(1000 * seed + 7 * n + len(kind)).random(n) < float(kind[1:])


def moment_centres(dims, count=None, seed=0):
    """int64 [N,3] centres inside the grid: every corner, every x of {0, 30, 31, 32, 33, nx - 1} that the grid has (at two
    (y, z)), then random ones; cut or filled to ``count`` when given."""
    nx, ny, nz = dims
    cen = [(x, y, z) for z in (0, nz - 1) for y in (0, ny - 1) for x in (0, nx - 1)]
    for x in (0, 30, 31, 32, 33, nx - 1):
        if 0 <= x < nx:
            cen += [(x, ny // 2, nz // 2), (x, 0, nz - 1)]
    rng = np.random.default_rng(seed + nx)
    want = len(cen) + 8 if count is None else count
    while len(cen) < want:
        cen.append((int(rng.integers(nx)), int(rng.integers(ny)), int(rng.integers(nz))))
    return np.array(cen[:want], np.int64).reshape(-1, 3)


# ------------------------------------------------------------------------------------------------ a drawn scan with thin tubes
# The six-view 48 x 64 scan of edge_seed_cases keeps tubes about 2.4 voxels in radius (3 px of tolerance on a 32^3 grid) and
# ghosts between them: too fat to be linear within 6 voxels.  The same drawn edges, twelve views of 96 x 128, a 48^3 grid
# and 2 px of tolerance give tubes of about one voxel.
DIR_VIEWS = 12
DIR_H, DIR_W = 96, 128
DIR_BOUNDS = SC.SEED_BOUNDS
DIR_OPTIONS = dict(grid=48, tol_px=2, cell=2)


def dir_cameras():
    from curve_gaussian_amd import synthetic as S
    return S.fibonacci_cameras(DIR_VIEWS, DIR_H, DIR_W)


@functools.lru_cache(maxsize=None)
def dir_samples():
    """(points float64 [n,3], unit tangents float64 [n,3]) of the drawn edges."""
    from curve_gaussian_amd.edge_extraction.abc import pred_points_and_directions
    pd = pred_points_and_directions(EC.SCAN_EDGES, EC.SCAN_RESOLUTION)
    t = pd.directions.astype(np.float64)
    return pd.points.astype(np.float32).astype(np.float64), t / np.linalg.norm(t, axis=1, keepdims=True)


def _intrinsics(c):
    return DIR_W / (2 * math.tan(c.FoVx / 2)), DIR_H / (2 * math.tan(c.FoVy / 2)), DIR_W / 2.0, DIR_H / 2.0


@functools.lru_cache(maxsize=None)
def dir_novel_cameras():
    """(NovelViewCamera s, uint8 PidiNet-style maps) of the drawn scan: every sampled point sets its pixel."""
    from curve_gaussian_amd.edge_extraction.novel_view import NovelViewCamera
    pts = dir_samples()[0]
    cams, maps = [], []
    for k, c in enumerate(dir_cameras()):
        w2c = c.world_view_transform.double().numpy().T
        fx, fy, cx, cy = _intrinsics(c)
        cam = pts @ w2c[:3, :3].T + w2c[:3, 3]
        u, v = fx * cam[:, 0] / cam[:, 2] + cx, fy * cam[:, 1] / cam[:, 2] + cy
        ok = (cam[:, 2] > 0) & (u >= 0) & (u < DIR_W) & (v >= 0) & (v < DIR_H)
        m = np.zeros((DIR_H, DIR_W), np.uint8)
        m[np.floor(v[ok]).astype(int), np.floor(u[ok]).astype(int)] = 255
        assert m.any(), "the scan's lines must be in view"
        cams.append(NovelViewCamera(f"v{k}", np.ascontiguousarray(w2c[:3, :3]), w2c[:3, 3].copy(), fx, fy, cx, cy, DIR_W, DIR_H))
        maps.append(m)
    return cams, maps


def nearest_tangents(seeds):
    """float64 [N,3]: for every seed the unit tangent of the nearest drawn sample."""
    pts, tan = dir_samples()
    near = np.argmin(((np.asarray(seeds)[:, None, :] - pts[None, :, :]) ** 2).sum(-1), axis=1)
    return tan[near]
