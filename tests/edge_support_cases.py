"""Shared inputs of the edge-support tests (test_edge_support_cpu.py, test_edge_support_gpu.py): a brute-force count, random
edges, cameras and distance transforms for the kernel, and the twelve-view drawn scan of edge_dir_cases with bogus edges
that start and end on its drawn edges."""
import functools

import numpy as np

import edge_dir_cases as DC
import edge_score_cases as EC
import visibility_ref64 as R
from curve_gaussian_amd.ops import edge_score as ES
from curve_gaussian_amd.ops import edge_support as SP

EDT_INF = EC.EDT_INF


# ------------------------------------------------------------------------------------------------ brute force
def counts_brute(points, offsets, K, M, d2, tol2):
    """int32 [E,V,1+T], point by point in Python floats (IEEE float64, one rounded operation at a time): the definition of
    cgs_edge_support."""
    E, V, T = len(offsets) - 1, len(K), len(tol2)
    H, W = d2.shape[1], d2.shape[2]
    out = np.zeros((E, V, 1 + T), np.int32)
    pts = np.asarray(points, np.float32).astype(np.float64)
    for v in range(V):
        m = [float(x) for x in np.asarray(M[v], np.float64).reshape(12)]
        fx, fy, cx, cy = (float(x) for x in K[v])
        for e in range(E):
            for i in range(int(offsets[e]), int(offsets[e + 1])):
                X, Y, Z = (float(x) for x in pts[i])
                c0 = ((m[0] * X + m[1] * Y) + m[2] * Z) + m[3]
                c1 = ((m[4] * X + m[5] * Y) + m[6] * Z) + m[7]
                c2 = ((m[8] * X + m[9] * Y) + m[10] * Z) + m[11]
                if not c2 > 0.0:
                    continue
                u, w = fx * (c0 / c2) + cx, fy * (c1 / c2) + cy
                if not (0.0 <= u < W and 0.0 <= w < H):
                    continue
                out[e, v, 0] += 1
                d = int(d2[v, int(np.floor(w)), int(np.floor(u))])
                for t in range(T):
                    out[e, v, 1 + t] += d <= tol2[t]
    return out


# ------------------------------------------------------------------------------------------------ random inputs for the kernel
SUPPORT_H = 5
EDGE_COUNTS = [0, 1, 63, 64, 65, 257]
POINT_COUNTS = [0, 1, 2, 63, 64, 65, 4096]
WIDTHS = [1, 33, 67]
VIEW_COUNTS = [1, 2, 5]
TOLERANCES = [(2,), (0, 1, 2.5, 5)]   # T = 1 and T = 4


def support_cameras(V, width, height=SUPPORT_H):
    """(intrinsics [V,4], w2c [V,3,4]) float64: the identity camera of edge_excl_cases (u = X / Z, v = Y / Z exactly), the
    same shifted by half a pixel, then cameras turned and moved a little so that their products round."""
    rng = np.random.default_rng(100 * V + width)
    K = np.tile(np.array([[1.0, 1.0, 0.0, 0.0]]), (V, 1))
    M = np.tile(np.eye(4)[None, :3, :4], (V, 1, 1))
    if V > 1:
        K[1, 2:] = 0.5
    for v in range(2, V):
        a = rng.uniform(-0.2, 0.2)
        M[v, :3, :3] = np.array([[np.cos(a), 0.0, np.sin(a)], [0.0, 1.0, 0.0], [-np.sin(a), 0.0, np.cos(a)]])
        M[v, :3, 3] = rng.uniform(-0.5, 0.5, 3)
        K[v] = [rng.uniform(0.8, 1.3), rng.uniform(0.8, 1.3), rng.uniform(0.0, 1.0), rng.uniform(0.0, 1.0)]
    return K, M


def support_d2(V, width, seed=0, height=SUPPORT_H):
    """int32 [V,H,W]: random in [0, 30] with EDT_INF entries (about one in eight)."""
    rng = np.random.default_rng(7000 + 10 * V + width + seed)
    d2 = rng.integers(0, 31, (V, height, width)).astype(np.int32)
    d2[rng.random(d2.shape) < 0.125] = EDT_INF
    return d2


def edge_sizes(E, seed=0):
    """int [E]: points per edge drawn from POINT_COUNTS so that every value occurs where E allows it, mixed; the 4096-point
    edges are kept to a few, so that the brute force stays quick."""
    rng = np.random.default_rng(31 * E + seed)
    sizes = [POINT_COUNTS[k % len(POINT_COUNTS)] for k in range(E)]
    sizes = [s if s != 4096 or k < 2 * len(POINT_COUNTS) else 3 for k, s in enumerate(sizes)]
    return rng.permutation(np.array(sizes, np.int64)) if E else np.zeros(0, np.int64)


def support_points(sizes, width, seed=0, height=SUPPORT_H):
    """(points float32 [P,3], offsets int32 [E+1]) for the cameras of support_cameras: a cloud in front of them that covers
    the image and its surroundings, and -- in every edge with at least eight points -- points behind the camera, at its
    eye, exactly on u = 0, v = 0, u = width and v = height of the identity camera (kept, kept, dropped, dropped), and
    inside its last row and column."""
    rng = np.random.default_rng(900 + width + seed)
    offsets = np.zeros(len(sizes) + 1, np.int32)
    offsets[1:] = np.cumsum(sizes)
    P = int(offsets[-1])
    z = rng.uniform(1.0, 3.0, P)
    pts = np.stack([rng.uniform(-0.3 * width - 1, 1.3 * width + 1, P) * z, rng.uniform(-2.0, height + 2.0, P) * z, z], 1)
    zz = 2.0   # a power of two: X / Z is exact
    special = np.array([[3.0 * zz, 2.0 * zz, -zz], [1.0, 1.0, 0.0], [0.0, 2.0 * zz, zz], [0.25 * zz, 0.0, zz],
                        [width * zz, 2.0 * zz, zz], [0.25 * zz, height * zz, zz],
                        [(width - 0.5) * zz, (height - 0.5) * zz, zz], [(width - 0.25) * zz, 0.5 * zz, zz]])
    for e, n in enumerate(sizes):
        if n >= len(special):
            pts[offsets[e]:offsets[e] + len(special)] = special
    return pts.astype(np.float32), offsets


# ------------------------------------------------------------------------------------------------ the drawn scan with bogus edges
BOGUS = 40            # lines and curves drawn, each
MIN_CHORD = 0.25      # a bogus edge's ends are further apart than this
ALONG = 0.03          # a bogus edge none of whose samples is further than this from a drawn sample runs along a drawn edge
SCAN_FRAMES_RATIO = 0.5


def _bogus_candidates():
    rng = np.random.default_rng(0)
    s = DC.dir_samples()[0]
    lines, curves = [], []
    while len(lines) < BOGUS:
        a, b = s[rng.integers(len(s))], s[rng.integers(len(s))]
        if np.linalg.norm(a - b) > MIN_CHORD:
            lines.append(np.stack([a, b]))
    while len(curves) < BOGUS:
        c = s[rng.integers(len(s), size=4)]
        if np.linalg.norm(c[0] - c[3]) > MIN_CHORD:
            curves.append(c)
    return np.array(curves), np.array(lines)


def _off_the_drawn_edges(curves, lines):
    """bool per edge (curves first): does one of its own samples lie more than ALONG from the nearest drawn sample?"""
    s = DC.dir_samples()[0]
    pts, off = SP.sample_edges(curves, lines, EC.SCAN_RESOLUTION)
    pts = pts.astype(np.float64)
    far = np.sqrt(((pts[:, None, :] - s[None, :, :]) ** 2).sum(-1).min(1)) > ALONG
    return np.array([far[off[e]:off[e + 1]].any() for e in range(len(off) - 1)], bool)


@functools.lru_cache(maxsize=None)
def scan_edges():
    """(edge_dict, drawn bool [E]) of the drawn scan: the edges of EC.SCAN_EDGES first within their kind, then the bogus
    edges that do not run along a drawn edge.  Edge order: curves, then lines."""
    curves, lines = _bogus_candidates()
    off = _off_the_drawn_edges(curves, lines)
    curves, lines = curves[off[:len(curves)]], lines[off[len(off) - len(lines):]]
    drawn_c = np.asarray(EC.SCAN_EDGES["curves_ctl_pts"], np.float64).reshape(-1, 4, 3)
    drawn_l = np.asarray(EC.SCAN_EDGES["lines_end_pts"], np.float64).reshape(-1, 2, 3)
    edge_dict = {"curves_ctl_pts": np.concatenate([drawn_c, curves]).reshape(-1, 12).tolist(),
                 "lines_end_pts": np.concatenate([drawn_l, lines]).reshape(-1, 6).tolist()}
    drawn = np.concatenate([np.ones(len(drawn_c), bool), np.zeros(len(curves), bool), np.ones(len(drawn_l), bool),
                            np.zeros(len(lines), bool)])
    return edge_dict, drawn


@functools.lru_cache(maxsize=None)
def scan_support(backend="host", keep_tolerance_px=2, budget_bytes=None):
    """edge_support of the drawn scan with its bogus edges at the settings of the issue: more than 6 of 12 views,
    min_near 0.8, min_visible 0.5."""
    cams, maps = DC.dir_novel_cameras()
    return SP.edge_support(scan_edges()[0], cams, maps, "PidiNet", resolution=EC.SCAN_RESOLUTION,
                           keep_tolerance_px=keep_tolerance_px, min_visible=0.5, min_near=0.8,
                           frames_ratio=SCAN_FRAMES_RATIO, backend=backend, budget_bytes=budget_bytes)


def reference_rule_keeps():
    """bool [E]: the reference's control-point rule on the same scan (visibility_ref64, the float64 restatement of
    extract_para_edge.py: mean > 0.1 and max > 0.5 at the rounded projections of the control / end points, in more than
    ceil(0.05 F) frames)."""
    cams, maps = DC.dir_novel_cameras()
    edge_dict = scan_edges()[0]
    values = R.map_values(np.stack(maps).astype(np.float64), "PidiNet")
    intr = [np.array([[c.fx, 0.0, c.cx], [0.0, c.fy, c.cy], [0.0, 0.0, 1.0]]) for c in cams]
    c2w = []
    for c in cams:
        w2c = np.eye(4)
        w2c[:3, :3], w2c[:3, 3] = c.R, c.T
        c2w.append(np.linalg.inv(w2c))
    curves = np.asarray(edge_dict["curves_ctl_pts"]).reshape(-1, 4, 3)
    lines = np.asarray(edge_dict["lines_end_pts"]).reshape(-1, 6)
    counts = R.visibility_counts(curves, lines, values, intr, c2w, DC.DIR_H, DC.DIR_W)
    from curve_gaussian_amd.edge_extraction.para_edge import edge_visibility_frames
    return counts > edge_visibility_frames(len(cams))


def write_support_scan(root, scan="room"):
    """<root>/data/<scan>: the drawn scan in the EMAP layout (PidiNet maps), and <root>/out/<scan>/parametric_edges.json with
    the drawn and the bogus edges.  Returns (base_dir, dataset_dir)."""
    import json
    import os

    import torch
    from curve_gaussian_amd.scene import dataset_io as IO
    data, out = os.path.join(str(root), "data"), os.path.join(str(root), "out")
    maps = [torch.from_numpy(m.astype(np.float32) / 255.0).unsqueeze(0) for m in DC.dir_novel_cameras()[1]]
    IO.write_emap(os.path.join(data, scan), DC.dir_cameras(), maps, detector="PidiNet")
    os.makedirs(os.path.join(out, scan), exist_ok=True)
    with open(os.path.join(out, scan, "parametric_edges.json"), "w") as f:
        json.dump(scan_edges()[0], f)
    return out, data
