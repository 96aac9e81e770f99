"""Shared inputs of the gated edge-vote tests (test_edge_vote_gate_cpu.py, test_edge_vote_gate_gpu.py): the grids, bounds,
views and cameras of edge_seed_cases at the widths of its packed masks, depth planes that reach every branch of the gate,
a per-(voxel, view) restatement of the gated vote in Python floats, and the solid scans the vote is held to."""
import functools

import numpy as np
import torch

import edge_seed_cases as SC
from curve_gaussian_amd.ops import edge_seed as SD

HEIGHT = SC.MASK_H
WIDTHS = SC.BITS_WIDTHS          # 1, 31, 32, 33, 67: the packed masks' stride and the depth rows' stride differ
PLANES = ("inf", "zero", "nan", "own", "own_up", "own_down", "mixed")
MIXED_SLACK = 0.05
SENTINEL = 0xABCD


# ------------------------------------------------------------------------------------------------ a view's inputs
@functools.lru_cache(maxsize=None)
def vote_bits(V, W):
    """int32 [V,HEIGHT,ceil(W/32)] CPU tensor: near bits of random squared distances 0 .. 8 at tolerance 2 (about half set)."""
    d2 = np.random.default_rng(300 + 7 * V + W).integers(0, 9, (V, HEIGHT, W)).astype(np.int32)
    return SD.near_bits(d2, 2, backend="host")


def centres64(dims, index=None):
    """float64 [n,3]: the float32 centres that are projected, widened."""
    c = SD.voxel_centres(SC.VOTE_BOUNDS, dims)
    return (c if index is None else c[np.asarray(index, np.int64)]).astype(np.float64)


def project(K, M, P):
    """(c2, u, v, keep) float64 / bool [V,n] of float64 points P [n,3]: the rule of cgs_project_points, one rounded operation
    per numpy call; ``keep`` against a HEIGHT x W image is formed by the caller from u and v."""
    M = np.asarray(M, np.float64).reshape(-1, 12)
    X, Y, Z = P[None, :, 0], P[None, :, 1], P[None, :, 2]
    m = lambda k: M[:, k:k + 1]
    with np.errstate(all="ignore"):
        c0 = ((m(0) * X + m(1) * Y) + m(2) * Z) + m(3)
        c1 = ((m(4) * X + m(5) * Y) + m(6) * Z) + m(7)
        c2 = ((m(8) * X + m(9) * Y) + m(10) * Z) + m(11)
        u = K[:, 0:1] * (c0 / c2) + K[:, 2:3]
        v = K[:, 1:2] * (c1 / c2) + K[:, 3:4]
    return c2, u, v


def kept(c2, u, v, W):
    with np.errstate(all="ignore"):
        return ~(c2 <= 0.0) & (u >= 0.0) & (u < float(W)) & (v >= 0.0) & (v < float(HEIGHT))


# ------------------------------------------------------------------------------------------------ depth planes
def own_planes(dims, V, W, ulps=0):
    """(depth float32 [V,HEIGHT,W], owner int64 [V,HEIGHT,W]): every pixel that a centre lands on holds that centre's own
    float64 camera depth rounded to float32 (of the LAST centre that lands there: ``owner``, -1 where none does), moved
    ``ulps`` float32 steps up (+1) or down (-1); +inf elsewhere."""
    K, M = SC.vote_cameras(V)
    c2, u, v = project(K, M, centres64(dims))
    keep = kept(c2, u, v, W)
    depth = np.full((V, HEIGHT, W), np.inf, np.float32)
    owner = np.full((V, HEIGHT, W), -1, np.int64)
    for i in range(V):
        at = np.nonzero(keep[i])[0]
        py, px = np.floor(v[i][at]).astype(np.int64), np.floor(u[i][at]).astype(np.int64)
        d = c2[i][at].astype(np.float32)
        if ulps:
            d = np.nextafter(d, np.float32(np.inf if ulps > 0 else -np.inf))
        depth[i, py, px], owner[i, py, px] = d, at   # numpy assigns in order: the last centre of a pixel stays
    return depth, owner


@functools.lru_cache(maxsize=None)
def _plane(kind, dims, V, W):
    shape = (V, HEIGHT, W)
    if kind == "inf":
        return np.full(shape, np.inf, np.float32)
    if kind == "zero":
        return np.zeros(shape, np.float32)
    if kind == "nan":
        return np.full(shape, np.nan, np.float32)
    if kind in ("own", "own_up", "own_down"):
        return own_planes(dims, V, W, {"own": 0, "own_up": 1, "own_down": -1}[kind])[0]
    assert kind == "mixed"
    rng = np.random.default_rng(500 + V + W + dims[0])
    d = rng.uniform(0.25, 4.0, shape).astype(np.float32)   # the cameras look at the grid from 0 to about 5 away
    pick = rng.integers(0, 8, shape)
    d[pick == 0], d[pick == 1], d[pick == 2] = np.inf, np.nan, 0.0
    return d


def plane(kind, dims, V, W):
    """(depth float32 [V,HEIGHT,W] -- a copy --, slack)."""
    return _plane(kind, tuple(dims), V, W).copy(), MIXED_SLACK if kind == "mixed" else 0.0


# ------------------------------------------------------------------------------------------------ brute force
def votes_brute(dims, K, M, bits, W, depth, slack):
    """(seen, hit, hidden) uint16 [n]: the gated vote, pair by pair in Python floats -- IEEE double, one rounded operation at a
    time, the header's order.  ``depth`` None: no gate."""
    P = centres64(dims)
    M = np.asarray(M, np.float64).reshape(-1, 12)
    words = bits.numpy().view(np.uint32)
    out = np.zeros((3, len(P)), np.uint16)
    for g, (X, Y, Z) in enumerate(P.tolist()):
        for i in range(len(K)):
            m, (fx, fy, cx, cy) = M[i].tolist(), np.asarray(K[i], np.float64).tolist()
            c0 = ((m[0] * X + m[1] * Y) + m[2] * Z) + m[3]
            c1 = ((m[4] * X + m[5] * Y) + m[6] * Z) + m[7]
            c2 = ((m[8] * X + m[9] * Y) + m[10] * Z) + m[11]
            if c2 <= 0.0 or c2 != c2:
                continue
            u, v = fx * (c0 / c2) + cx, fy * (c1 / c2) + cy
            if not (u >= 0.0 and u < float(W) and v >= 0.0 and v < float(HEIGHT)):
                continue
            px, py = int(np.floor(u)), int(np.floor(v))
            if depth is not None and c2 > float(depth[i, py, px]) + slack:
                out[2, g] += 1
                continue
            out[0, g] += 1
            out[1, g] += (int(words[i, py, px >> 5]) >> (px & 31)) & 1
    return out[0], out[1], out[2]


def run_votes(dims, V, W, depth, slack, backend, device=None, split=None, hidden=True):
    """numpy (seen, hit[, hidden]) of ``voxel_votes`` on the case; ``split``: the views of the first of two accumulating calls."""
    K, M = SC.vote_cameras(V)
    bits = vote_bits(V, W)
    on = dict(backend=backend, device=device)
    gate = {} if depth is None else dict(depth=depth, slack=slack, return_hidden=hidden)
    if split is None:
        out = SD.voxel_votes(SC.VOTE_BOUNDS, dims, K, M, bits, HEIGHT, W, **gate, **on)
    else:
        out = None
        for sel in (slice(0, split), slice(split, V)):
            g = dict(gate, depth=depth[sel]) if depth is not None else {}
            out = SD.voxel_votes(SC.VOTE_BOUNDS, dims, K[sel], M[sel], bits[sel], HEIGHT, W, counts=out, **g, **on)
    return tuple(t.cpu().numpy() for t in out)


def listed(dims, seed=0):
    """(index int32 [M] ascending inside the grid, support uint16 [M]): about two voxels in three, supports in [0, 65535]."""
    n = dims[0] * dims[1] * dims[2]
    rng = np.random.default_rng(700 + n + seed)
    index = np.nonzero(rng.random(n) < 0.67)[0].astype(np.int32)
    if index.size == 0:
        index = np.zeros(1, np.int32)
    return index, rng.integers(0, 65536, index.size).astype(np.uint16)


def run_claims(dims, V, W, index, support, depth, slack, backend, device=None, window=1, margin=0):
    """numpy (best int32 [V,HEIGHT,W], wins uint16 [M]) of ``ray_claims`` then ``ray_wins`` on the case."""
    K, M = SC.vote_cameras(V)
    bits = vote_bits(V, W)
    gate = {} if depth is None else dict(depth=depth, slack=slack)
    args = (SC.VOTE_BOUNDS, dims, index, support, K, M, bits)
    best = SD.ray_claims(*args, HEIGHT, W, backend=backend, device=device, **gate)
    wins = SD.ray_wins(*args, best, HEIGHT, W, window=window, margin=margin, backend=backend, device=device, **gate)
    return best.cpu().numpy(), wins.cpu().numpy()


def claims_brute(dims, V, W, index, support, depth, slack, window=1, margin=0):
    """(best int32 [V,HEIGHT,W], wins uint16 [M]) restated from ``project``: a listed voxel hits in a view that keeps its
    centre, does not hide it and has its near bit set; best is the largest support that hits a pixel, a view is won when
    support + margin reaches the largest best of the clipped window.  ``depth`` None: no gate."""
    K, M = SC.vote_cameras(V)
    words = vote_bits(V, W).numpy().view(np.uint32)
    support = np.asarray(support, np.int64)
    c2, u, v = project(K, M, centres64(dims, index))
    keep = kept(c2, u, v, W)
    best, hits = np.zeros((V, HEIGHT, W), np.int64), []
    for i in range(V):
        at = np.nonzero(keep[i])[0]
        py, px = np.floor(v[i][at]).astype(np.int64), np.floor(u[i][at]).astype(np.int64)
        ok = ((words[i, py, px >> 5] >> (px & 31).astype(np.uint32)) & np.uint32(1)) != 0
        if depth is not None:
            with np.errstate(all="ignore"):
                ok &= ~(c2[i][at] > depth[i, py, px].astype(np.float64) + slack)
        at, py, px = at[ok], py[ok], px[ok]
        np.maximum.at(best[i], (py, px), support[at])
        hits.append((at, py, px))
    wins = np.zeros(len(support), np.uint16)
    for i, (at, py, px) in enumerate(hits):
        pad = np.zeros((HEIGHT + 2 * window, W + 2 * window), np.int64)   # a clipped window: outside the image nothing is claimed
        pad[window:window + HEIGHT, window:window + W] = best[i]
        top = np.zeros(len(at), np.int64)
        for dy in range(2 * window + 1):
            for dx in range(2 * window + 1):
                top = np.maximum(top, pad[py + dy, px + dx])
        wins[at] += (support[at] + margin >= top).astype(np.uint16)
    return best.astype(np.int32), wins


# ------------------------------------------------------------------------------------------------ solids
SOLID_VIEWS, SOLID_H, SOLID_W = 24, 240, 320
SOLID_BOUNDS = ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
SOLID_GRID, SOLID_TOL_PX = 64, 2
GT_RESOLUTION = 0.005
VOXEL_DIAGONAL = float(np.sqrt(3.0)) / SOLID_GRID      # 0.0271
COVER_RADIUS = 2.0 * VOXEL_DIAGONAL                    # (a): every ground-truth sample has a kept centre this near
FAR = 0.02                                             # (b): no kept centre is farther than this from the ground truth


@functools.lru_cache(maxsize=None)
def solid(shape):
    from curve_gaussian_amd.scene import solid_scan as SS
    return SS.solid_scan(shape, SOLID_VIEWS, SOLID_H, SOLID_W, backend="host")


@functools.lru_cache(maxsize=None)
def ground_truth(shape):
    """float64 [n,3]: the solid's edges sampled at GT_RESOLUTION."""
    from curve_gaussian_amd.edge_extraction.abc import pred_points_and_directions
    return np.asarray(pred_points_and_directions(solid(shape).edges, GT_RESOLUTION).points, np.float64).reshape(-1, 3)


def nearest(a, b):
    """float64 [len(a)]: the distance from every row of a to the nearest row of b (inf when b is empty)."""
    if len(b) == 0:
        return np.full(len(a), np.inf)
    out = np.empty(len(a))
    for s in range(0, len(a), 512):
        d = a[s:s + 512, None, :] - b[None, :, :]
        out[s:s + 512] = np.sqrt((d * d).sum(2).min(1))
    return out


class Recorder:
    """``seed_points`` with the votes and the selection it made on the way: patches ``voxel_votes`` / ``select_voxels`` of
    ops.edge_seed for one call."""

    def __init__(self):
        self.counts, self.kept = None, None

    def __call__(self, scan, backend, device=None, **kw):
        import unittest.mock as mock
        votes, select = SD.voxel_votes, SD.select_voxels

        def rec_votes(*a, **k):
            self.counts = votes(*a, **k)
            return self.counts

        def rec_select(*a, **k):
            self.kept = select(*a, **k)
            return self.kept

        with mock.patch.object(SD, "voxel_votes", rec_votes), mock.patch.object(SD, "select_voxels", rec_select):
            seeds, info = SD.seed_points(scan.cameras, list(scan.maps), "PidiNet", SOLID_BOUNDS, grid=SOLID_GRID,
                                         tol_px=SOLID_TOL_PX, backend=backend, device=device, **kw)
        self.counts = tuple(c.cpu().numpy() for c in self.counts)
        return seeds, info


def solid_votes(shape, backend, device=None, **kw):
    """(seeds, info, kept bool [n], kept centres float64 [k,3], (seen, hit[, hidden]) numpy) of one ``seed_points`` call."""
    rec = Recorder()
    seeds, info = rec(solid(shape), backend, device, **kw)
    dims = info["dims"]
    cen = SD.voxel_centres(SOLID_BOUNDS, dims)[rec.kept].astype(np.float64)
    return seeds, info, rec.kept, cen, rec.counts


def check_solid(shape, backend, device=None):
    """Conditions (a), (b), (c) and (e) of the gated vote on one solid ((a) alone on l_bracket: one far voxel was seen there in
    the prototype).  Returns the gated call's (info, kept, counts) for the caller's own checks."""
    scan, gt = solid(shape), ground_truth(shape)
    seeds, info, keep, cen, counts = solid_votes(shape, backend, device, depth_maps=list(scan.depth))
    to_kept = nearest(gt, cen)
    print(f"{shape} [{backend}]: kept {int(keep.sum())}, seeds {info['seeds']}, hidden pairs {info['hidden_pairs']}, "
          f"worst sample->kept {to_kept.max():.4f} (bound {COVER_RADIUS:.4f}), "
          f"far kept {int((nearest(cen, gt) > FAR).sum()) if len(cen) else 0}")
    assert (to_kept <= COVER_RADIUS).all(), f"(a) {int((to_kept > COVER_RADIUS).sum())} of {len(gt)} samples are uncovered"
    if shape != "l_bracket":
        from_kept = nearest(cen, gt)
        assert (from_kept <= FAR).all(), f"(b) {int((from_kept > FAR).sum())} kept centres are far, worst {from_kept.max():.4f}"
        assert info["seeds"] > 0 and len(seeds) == info["seeds"], "(c)"
        _, info_o, keep_o, _, _ = solid_votes(shape, backend, device, occluder=scan.tris)
        assert np.array_equal(keep_o, keep), "(e) the occluder's planes keep what the scan's own depth maps keep"
        assert info_o["occluder"] is True and info["depth_maps"] is True
    assert info["depth_slack"] == SD.default_slack(SOLID_BOUNDS, info["dims"])
    assert abs(info["depth_slack"] - 0.5 * VOXEL_DIAGONAL) < 1e-15, "the default slack is half the voxel diagonal"
    seen, hit, hidden = counts
    assert info["hidden_pairs"] == int(hidden.astype(np.int64).sum()) > 0
    return info, keep, counts
