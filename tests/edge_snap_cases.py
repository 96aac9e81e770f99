"""Shared inputs of the edge-snapping tests (test_edge_snap_cpu.py, test_edge_snap_gpu.py): the brute-force normal
equations that define cgs_sample_snap_terms, random points, cameras and distance transforms for the kernel, and the
twelve-view drawn scan of edge_dir_cases with its four drawn edges perturbed by a pixel."""
import functools
import math

import numpy as np

import edge_dir_cases as DC
import edge_score_cases as EC
import edge_support_cases as SC
import edge_trim_cases as TC
from curve_gaussian_amd.ops import edge_snap as SN
from curve_gaussian_amd.ops import edge_support as SP

EDT_INF = EC.EDT_INF


# ------------------------------------------------------------------------------------------------ brute force
def snap_terms_brute(points, K, M, d2, cap2):
    """(float64 [P,10], int32 [P]), point by point in Python floats (IEEE float64, one rounded operation at a time): the
    definition of cgs_sample_snap_terms on zeroed sums.  The distances are math.sqrt of the integers, correctly rounded."""
    V = len(K)
    H, W = d2.shape[1], d2.shape[2]
    lut = [math.sqrt(k) for k in range(cap2 + 1)]
    pts = np.asarray(points, np.float32).astype(np.float64)
    terms = [[0.0] * 10 for _ in range(len(pts))]
    views = np.zeros(len(pts), np.int32)
    for v in range(V):
        m = [float(x) for x in np.asarray(M[v], np.float64).reshape(12)]
        fx, fy, cx, cy = (float(x) for x in K[v])
        for i in range(len(pts)):
            X, Y, Z = (float(x) for x in pts[i])
            c0 = ((m[0] * X + m[1] * Y) + m[2] * Z) + m[3]
            c1 = ((m[4] * X + m[5] * Y) + m[6] * Z) + m[7]
            c2 = ((m[8] * X + m[9] * Y) + m[10] * Z) + m[11]
            if not c2 > 0.0:
                continue
            x, y = c0 / c2, c1 / c2
            u, w = fx * x + cx, fy * y + cy
            if not (0.0 <= u < W and 0.0 <= w < H):
                continue
            a, b = u - 0.5, w - 0.5
            j0, i0 = math.floor(a), math.floor(b)
            if not (0 <= j0 and j0 + 1 <= W - 1 and 0 <= i0 and i0 + 1 <= H - 1):
                continue
            k = [int(d2[v, i0, j0]), int(d2[v, i0, j0 + 1]), int(d2[v, i0 + 1, j0]), int(d2[v, i0 + 1, j0 + 1])]
            if not all(0 <= q <= cap2 for q in k):   # before the table is indexed
                continue
            d00, d01, d10, d11 = (lut[q] for q in k)
            fa, fb = a - j0, b - i0
            ga, gb = 1.0 - fa, 1.0 - fb
            r = gb * (ga * d00 + fa * d01) + fb * (ga * d10 + fa * d11)
            gu = gb * (d01 - d00) + fb * (d11 - d10)
            gv = ga * (d10 - d00) + fa * (d11 - d01)
            su, sv = (gu * fx) / c2, (gv * fy) / c2
            gc = -(su * x + sv * y)
            g = [(m[n] * su + m[4 + n] * sv) + m[8 + n] * gc for n in range(3)]
            t = terms[i]
            for col, val in enumerate((g[0] * g[0], g[0] * g[1], g[0] * g[2], g[1] * g[1], g[1] * g[2], g[2] * g[2],
                                       g[0] * r, g[1] * r, g[2] * r, r * r)):
                t[col] = t[col] + val
            views[i] += 1
    return np.array(terms, np.float64).reshape(-1, 10), views


# ------------------------------------------------------------------------------------------------ random inputs for the kernel
PLANES = [(1, 9), (9, 1), (2, 2), (37, 70)]   # (H, W): two planes without a footprint, a single footprint, a general one
CAPTURES = [1, 3, 8]
POINT_COUNTS = [0, 1, 63, 64, 65, 257]
VIEW_COUNTS = [0, 1, 2, 13]
BIG_P = 4096 + 65
SPECIAL = 8   # rows that support_points fills


def snap_cameras(V, H, W):
    """edge_support_cases.support_cameras: the identity camera, the same shifted by half a pixel (so that u - 0.5 = X / Z
    exactly), then cameras turned and moved a little."""
    if V == 0:
        return np.zeros((0, 4)), np.zeros((0, 3, 4))
    return SC.support_cameras(V, W, H)


def snap_d2(V, H, W, cap2, seed=0, kind="random"):
    """int32 [V,H,W]: mostly values inside the capture (so that most footprints pass), the rest just past it, far past it
    or EDT_INF; ``kind="inf"``: EDT_INF everywhere, the transform of empty masks."""
    if kind == "inf":
        return np.full((V, H, W), EDT_INF, np.int32)
    rng = np.random.default_rng(5000 + 100 * V + 10 * H + W + cap2 + seed)
    d2 = rng.integers(0, cap2 + 1, (V, H, W)).astype(np.int32)
    pick = rng.random(d2.shape)
    d2[pick < 0.12] = cap2 + 1
    d2[pick < 0.08] = 10 * cap2 + 7
    d2[pick < 0.04] = EDT_INF
    return d2


def snap_points(P, H, W, seed=0):
    """float32 [P,3]: the cloud of edge_trim_cases.tally_points for a plane of H rows -- the special points (behind the
    camera, at its eye, exactly on the frame's bounds) first wherever P >= 8 -- and after them, where P allows, samples
    whose u - 0.5 or v - 0.5 is an exact integer in the first two cameras and samples within half a pixel of each of the
    four borders."""
    pts = TC.tally_points(P, W, seed) if H == SC.SUPPORT_H else SC.support_points(np.array([P]), W, seed, height=H)[0]
    zz = 2.0   # a power of two: X / Z is exact
    mj, mi = min(1, W - 1), min(1, H - 1)
    extra = np.array([[(mj + 0.5) * zz, (mi + 0.25) * zz, zz],      # u - 0.5 an integer in the identity camera
                      [(mj + 0.25) * zz, (mi + 0.5) * zz, zz],      # v - 0.5 an integer
                      [(mj + 0.5) * zz, (mi + 0.5) * zz, zz],       # both
                      [float(mj) * zz, float(mi) * zz, zz],         # both in the camera shifted by half a pixel
                      [0.25 * zz, (mi + 0.3) * zz, zz],             # within half a pixel of the left border
                      [(W - 0.25) * zz, (mi + 0.3) * zz, zz],       # of the right border
                      [(mj + 0.3) * zz, 0.25 * zz, zz],             # of the top border
                      [(mj + 0.3) * zz, (H - 0.25) * zz, zz],       # of the bottom border
                      [(W - 1.5) * zz, (H - 1.5) * zz, zz]], np.float32)   # the last footprint, exactly on its first pixel
    if P >= SPECIAL + len(extra):
        pts[SPECIAL:SPECIAL + len(extra)] = extra
    return pts


@functools.lru_cache(maxsize=None)
def kernel_case(P, V, H, W, capture_px, kind="random"):
    """(points, K, M, d2, cap2, (terms, views) of the brute force) -- computed once, shared, never written to."""
    cap2 = SN.capture_squared(capture_px)
    pts = snap_points(P, H, W)
    K, M = snap_cameras(V, H, W)
    d2 = snap_d2(V, H, W, cap2, kind=kind)
    want = snap_terms_brute(pts, K, M, d2, cap2)
    for arr in (pts, K, M, d2) + want:
        arr.setflags(write=False)
    return pts, K, M, d2, cap2, want


def same_bits(got, want):
    """Both members of (terms, views) equal, the float64 compared as their int64 bit patterns."""
    gt, gv = (np.ascontiguousarray(x.cpu().numpy() if hasattr(x, "cpu") else x) for x in got)
    wt, wv = (np.ascontiguousarray(x.cpu().numpy() if hasattr(x, "cpu") else x) for x in want)
    return (gt.shape == wt.shape and gv.shape == wv.shape and gt.dtype == np.float64 and gv.dtype == np.int32
            and np.array_equal(gt.view(np.int64), wt.view(np.int64)) and np.array_equal(gv, wv))


# ------------------------------------------------------------------------------------------------ the drawn scan, perturbed
SCAN_FRAMES_RATIO = SC.SCAN_FRAMES_RATIO
SIGMA = 4 * EC.SCAN_RESOLUTION   # one pixel per coordinate
SEED = 0
# The mean distance to the true edge after the snap, per edge (the curve, then the three lines), of a host run of this
# implementation at SEED (profiles/edge_snap.md), times 2 for the spread from seed to seed.
AFTER_MEASURED = (0.00102, 0.00309, 0.00420, 0.00028)
AFTER_BOUND = tuple(2 * x for x in AFTER_MEASURED)


def drawn_arrays():
    return SP._edge_arrays(EC.SCAN_EDGES["curves_ctl_pts"], EC.SCAN_EDGES["lines_end_pts"])


@functools.lru_cache(maxsize=None)
def perturbed_edges(seed=SEED, sigma=SIGMA):
    """The four drawn edges with Gaussian noise of ``sigma`` on every coordinate of every control point; shared ends get
    one draw, so they stay bitwise equal."""
    rng = np.random.default_rng(seed)
    c, l = drawn_arrays()
    c, l = c + rng.normal(0.0, sigma, c.shape), l + rng.normal(0.0, sigma, l.shape)
    l[1, 0] = l[0, 1]   # the corner the first two drawn lines share
    return {"curves_ctl_pts": c.reshape(-1, 12).tolist(), "lines_end_pts": l.reshape(-1, 6).tolist()}


def shifted_edge(pixels=10):
    """The first drawn line moved ``pixels`` pixels off every drawn edge, as the only edge of a dict."""
    _, l = drawn_arrays()
    return {"curves_ctl_pts": [], "lines_end_pts": (l[:1] + np.array([0.0, 0.0, -pixels * SIGMA])).reshape(1, 6).tolist()}


@functools.lru_cache(maxsize=None)
def scan_snap(which="perturbed", backend="host", budget_bytes=None, iterations=5):
    """snap_edges on the drawn scan at the settings of the issue: more than 6 of 12 views, everything else at its default."""
    edges = {"perturbed": perturbed_edges, "drawn": lambda: EC.SCAN_EDGES, "shifted": shifted_edge}[which]()
    cams, maps = DC.dir_novel_cameras()
    return SN.snap_edges(edges, cams, maps, "PidiNet", resolution=EC.SCAN_RESOLUTION, frames_ratio=SCAN_FRAMES_RATIO,
                         backend=backend, budget_bytes=budget_bytes, iterations=iterations)


def _segment_distance(p, a, b):
    """float [n]: the distance of every point p [n,3] to the nearest of the segments a[k] b[k]."""
    d = b - a
    t = np.clip(((p[:, None, :] - a[None]) * d[None]).sum(-1) / (d * d).sum(-1)[None], 0.0, 1.0)
    return np.sqrt((((a[None] + t[..., None] * d[None]) - p[:, None, :]) ** 2).sum(-1).min(1))


def distance_to_drawn(edge_dict):
    """float [4]: per edge (the curve, then the lines) the mean distance of its samples at SCAN_RESOLUTION to the drawn
    edge of the same index, the curve as a polyline of 2000 chords."""
    c, l = SP._edge_arrays(edge_dict["curves_ctl_pts"], edge_dict["lines_end_pts"])
    pts, off = SP.sample_edges(c, l, EC.SCAN_RESOLUTION)
    tc, tl = drawn_arrays()
    poly = TC.bezier_points(tc[0], np.linspace(0.0, 1.0, 2001))
    truth = [(poly[:-1], poly[1:])] + [(tl[k, :1], tl[k, 1:]) for k in range(len(tl))]
    return np.array([_segment_distance(pts[off[e]:off[e + 1]].astype(np.float64), *truth[e]).mean() for e in range(len(truth))])
