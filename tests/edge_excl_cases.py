"""Shared inputs of the ray-exclusive claim tests (test_edge_excl_cpu.py, test_edge_excl_gpu.py): a hand-made column of
voxels on one pixel of the identity camera, lists and supports for the vote grids of edge_seed_cases, images of the widths
around the word boundaries, a grid that lands on one pixel, and the ghost / coverage counts of the two drawn scans."""
import functools

import numpy as np
import torch

import edge_dir_cases as DC
import edge_score_cases as EC
import edge_seed_cases as SC
from curve_gaussian_amd.ops import edge_seed as SD

WINDOWS = [0, 1, 4]
MARGINS = [0, 1, 65535]
DENSITIES = [0.5, 1.0]
LIST_LENGTHS = [0, 1, 63, 64, 65, 257]


def identity_camera():
    """(intrinsics [1,4], w2c [1,3,4]): u = X / Z, v = Y / Z exactly."""
    K, M = EC.mask_cameras()
    return K[2:], M[2:]


def ones_bits(V, H, W):
    """The packed near masks of all-one masks: every pixel is near."""
    return SD.near_bits(np.zeros((V, H, W), np.int32), 0, backend="host")


def mask_bits(mask):
    """The packed near masks of bool [V,H,W] masks, the mask itself (tolerance 0)."""
    return SD.near_bits(np.where(mask, 0, EC.EDT_INF).astype(np.int32), 0, backend="host")


# ------------------------------------------------------------------------------------------------ the hand case
# Columns of four voxels along Z in front of the identity camera.  Z centres 1.0 .. 1.3 (step 0.1 from 0.95); the column
# i = 0 has X = 0 and lands on pixel (0, 0), the column i = 1 of the two-column grid has X = 1.5: u = 1.5 / Z lies in
# [1.15, 1.5], pixel (1, 0).  Y = 0 for all.
HAND_H, HAND_W = 3, 4
HAND_SUPPORT = [10, 30, 30, 20]


def hand_grid(columns):
    """(bounds, dims) of ``columns`` (1 or 2) columns of four voxels; voxel (i, 0, k) has the linear index k columns + i."""
    return ((-0.75, -0.5, 0.95), (-0.75 + 1.5 * columns, 0.5, 1.35)), (columns, 1, 4)


# ------------------------------------------------------------------------------------------------ lists for the vote grids
def random_list(dims, density, seed=0):
    """(index int32 [M] ascending, support uint16 [M] in [1, 65535]) from a random keep mask of the given density; supports
    are drawn from 16 values, so that equal supports meet."""
    n = dims[0] * dims[1] * dims[2]
    rng = np.random.default_rng(31 * n + int(100 * density) + seed)
    keep = rng.random(n) < density if density < 1.0 else np.ones(n, bool)
    index = np.nonzero(keep)[0].astype(np.int32)
    values = rng.integers(1, 65536, 16)
    values[0], values[1] = 1, 65535
    return index, values[rng.integers(0, 16, index.size)].astype(np.uint16)


@functools.lru_cache(maxsize=None)
def vote_bits(V):
    """The packed near masks of ``vote_masks(V)`` at 2 px: about a third of the pixels are near."""
    from curve_gaussian_amd.ops import edge_score as ES
    return SD.near_bits(ES.edt_squared(SC.vote_masks(V), "host"), 2, backend="host")


# ------------------------------------------------------------------------------------------------ widths around the word boundaries
WIDTH_H = SC.BITS_HEIGHT


@functools.lru_cache(maxsize=None)
def width_case(width):
    """(bounds, dims, K, M, bits, index, support) for an image of WIDTH_H x width under two cameras: the identity camera
    and the same shifted by half a pixel.  The grid spans Z in [1, 1.5] and more than the image in X and Y, so that voxels
    land on every column -- the first and the last included -- and outside; half of the pixels are near."""
    K1, M1 = identity_camera()
    K = np.concatenate([K1, K1 + np.array([[0.0, 0.0, 0.5, 0.5]])])
    M = np.concatenate([M1, M1])
    bounds = ((-1.0, -1.0, 1.0), (1.5 * width + 1.0, 1.5 * WIDTH_H + 1.0, 1.5))
    dims = (2 * width + 3, 2 * WIDTH_H + 3, 2)
    mask = np.random.default_rng(500 + width).random((2, WIDTH_H, width)) < 0.5
    mask[:, 0, 0] = mask[:, -1, -1] = True
    index, support = random_list(dims, 0.5, seed=width)
    return bounds, dims, K, M, mask_bits(mask), index, support


# ------------------------------------------------------------------------------------------------ one pixel for 257 voxels
CONTENTION_DIMS = (257, 1, 1)
CONTENTION_BOUNDS = ((10.0, 10.0, 100.0), (10.5, 10.5, 100.5))   # u = X / Z and v = Y / Z lie in [0.099, 0.105]: pixel (0, 0)


def contention_support():
    """uint16 [257]: the distinct values 1000 .. 1256 in a random order."""
    return np.random.default_rng(9).permutation(np.arange(1000, 1257)).astype(np.uint16)


# ------------------------------------------------------------------------------------------------ the drawn scans
GHOST_VOXELS = 3.0   # a seed further than this many voxels from the nearest drawn sample is a ghost


def ghosts_and_coverage(seeds, samples, voxel, cell):
    """(the seeds more than GHOST_VOXELS voxels from the nearest sample, the share of the samples with a seed within
    ``cell`` + 1 voxels)."""
    d = np.sqrt(((np.asarray(seeds)[:, None, :] - samples[None, :, :]) ** 2).sum(-1))
    return int((d.min(1) > GHOST_VOXELS * voxel).sum()), float((d.min(0) <= (cell + 1) * voxel).mean())


@functools.lru_cache(maxsize=None)
def six_view_seeds(exclusive, backend="host"):
    """(seeds, info) of the six-view drawn scan of edge_seed_cases on the host back end."""
    cams, maps = SC.seed_novel_cameras()
    return SD.seed_points(cams, maps, "PidiNet", SC.SEED_BOUNDS, backend=backend, exclusive=exclusive, **SC.SEED_OPTIONS)


@functools.lru_cache(maxsize=None)
def twelve_view_seeds(exclusive, backend="host"):
    """(seeds, info) of the twelve-view drawn scan of edge_dir_cases with directions on the host back end."""
    cams, maps = DC.dir_novel_cameras()
    return SD.seed_points(cams, maps, "PidiNet", DC.DIR_BOUNDS, backend=backend, directions=True, exclusive=exclusive,
                          **DC.DIR_OPTIONS)


def same_info(a, b):
    """Two seed_points infos are equal, the directions array included; the back end's name aside."""
    keys = set(a) - {"backend"}
    return keys == set(b) - {"backend"} and all(np.array_equal(a[k], b[k]) for k in keys)


def as_numpy(t):
    return t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
