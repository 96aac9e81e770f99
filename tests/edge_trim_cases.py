"""Shared inputs of the edge-trimming tests (test_edge_trim_cpu.py, test_edge_trim_gpu.py): a brute-force tally, the random
points, cameras and distance transforms of edge_support_cases, and the twelve-view drawn scan of edge_dir_cases with its
four drawn edges over-extended at one end."""
import functools

import numpy as np

import edge_dir_cases as DC
import edge_score_cases as EC
import edge_support_cases as SC
from curve_gaussian_amd.ops import edge_support as SP
from curve_gaussian_amd.ops import edge_trim as ET

EDT_INF = EC.EDT_INF


# ------------------------------------------------------------------------------------------------ brute force
def tally_brute(points, K, M, d2, tol2):
    """int32 [P,1+T], point by point in Python floats (IEEE float64, one rounded operation at a time): the definition of
    cgs_sample_support on a zeroed tally."""
    V, T = len(K), len(tol2)
    H, W = d2.shape[1], d2.shape[2]
    pts = np.asarray(points, np.float32).astype(np.float64)
    out = np.zeros((len(pts), 1 + T), np.int32)
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
            u, w = fx * (c0 / c2) + cx, fy * (c1 / c2) + cy
            if not (0.0 <= u < W and 0.0 <= w < H):
                continue
            out[i, 0] += 1
            d = int(d2[v, int(np.floor(w)), int(np.floor(u))])
            for t in range(T):
                out[i, 1 + t] += d <= tol2[t]
    return out


# ------------------------------------------------------------------------------------------------ random inputs for the kernel
POINT_COUNTS = [0, 1, 63, 64, 65, 257, 4096 + 65]   # around a wave, more than one workgroup, many workgroups and a tail


def tally_points(P, width, seed=0):
    """float32 [P,3]: support_points' cloud as one edge, so that the special points (behind the camera, at its eye, exactly on
    the frame's bounds) come first wherever P >= 8."""
    return SC.support_points(np.array([P]), width, seed)[0]


# ------------------------------------------------------------------------------------------------ the drawn scan, over-extended
EXT = 0.4          # a line is extended by this share of its length
CURVE_T0 = -0.3    # the curve is re-cut over [CURVE_T0, 1]
SCAN_FRAMES_RATIO = SC.SCAN_FRAMES_RATIO
CUT_CAP = {1: 12, 2: 16}   # samples: (tolerance + sqrt(2) px of pixel quantisation) / 0.25 px per sample = 9.7 and 13.7,
                           # rounded up for foreshortening


def bezier_blossom(c, t1, t2, t3):
    """B(t1, t2, t3) of one cubic Bezier curve c [4,3] by de Casteljau, one parameter per level."""
    q = [(1 - t1) * c[k] + t1 * c[k + 1] for k in range(3)]
    r = [(1 - t2) * q[k] + t2 * q[k + 1] for k in range(2)]
    return (1 - t3) * r[0] + t3 * r[1]


def bezier_points(c, t):
    """The curve c [4,3] at the parameters t [n] in Bernstein form."""
    t = np.asarray(t, np.float64)[:, None]
    return (1 - t) ** 3 * c[0] + 3 * (1 - t) ** 2 * t * c[1] + 3 * (1 - t) * t ** 2 * c[2] + t ** 3 * c[3]


@functools.lru_cache(maxsize=None)
def extended_edges():
    """(edge_dict, true [E], at_end bool [E]) of the four drawn edges of EC.SCAN_EDGES, each over-extended at one end; edge
    order: the curve, then the three lines.  ``true``: the parameter in [0, 1] of the extended edge at which the drawn edge
    stops (at_end) or starts (not at_end); the other end is untouched."""
    l = np.asarray(EC.SCAN_EDGES["lines_end_pts"], np.float64).reshape(3, 2, 3)
    c = np.asarray(EC.SCAN_EDGES["curves_ctl_pts"], np.float64).reshape(4, 3)
    d = l[:, 1] - l[:, 0]
    lines = np.stack([np.stack([l[0, 0], l[0, 1] + EXT * d[0]]), np.stack([l[1, 0] - EXT * d[1], l[1, 1]]),
                      np.stack([l[2, 0], l[2, 1] + EXT * d[2]])])
    a, b = CURVE_T0, 1.0
    curve = np.stack([bezier_blossom(c, a, a, a), bezier_blossom(c, a, a, b), bezier_blossom(c, a, b, b),
                      bezier_blossom(c, b, b, b)])
    true = np.array([-CURVE_T0 / (1.0 - CURVE_T0), 1.0 / (1.0 + EXT), EXT / (1.0 + EXT), 1.0 / (1.0 + EXT)])
    edge_dict = {"curves_ctl_pts": curve.reshape(1, 12).tolist(), "lines_end_pts": lines.reshape(3, 6).tolist()}
    return edge_dict, true, np.array([False, True, False, True])


@functools.lru_cache(maxsize=None)
def scan_trim(which="extended", backend="host", tolerance_px=1, budget_bytes=None, max_gap=0, min_span=2):
    """trim_edges on the drawn scan at the settings of the issue -- more than 6 of 12 views, and the raw runs (max_gap 0,
    min_span 2) unless told otherwise.  ``which``: "extended" (extended_edges), "drawn" (EC.SCAN_EDGES) or "bogus"
    (edge_support_cases.scan_edges, the drawn edges and the chords)."""
    edges = {"extended": lambda: extended_edges()[0], "drawn": lambda: EC.SCAN_EDGES, "bogus": lambda: SC.scan_edges()[0]}
    cams, maps = DC.dir_novel_cameras()
    return ET.trim_edges(edges[which](), cams, maps, "PidiNet", resolution=EC.SCAN_RESOLUTION, tolerance_px=tolerance_px,
                         frames_ratio=SCAN_FRAMES_RATIO, max_gap=max_gap, min_span=min_span, backend=backend,
                         budget_bytes=budget_bytes)


def cut_errors(result):
    """float [E]: how many samples beyond the drawn edge's true end (or before its true start) the one span of every
    extended edge reaches; negative when it stops short."""
    _, true, at_end = extended_edges()
    n = np.diff(result["offsets"].astype(np.int64))
    a = np.array([s[0][0] for s in result["spans"]], np.float64)
    b = np.array([s[0][1] for s in result["spans"]], np.float64)
    return np.where(at_end, b - true * (n - 1), true * (n - 1) - a)
