"""Float64 restatement of the reference's edge-map visibility check (edge_extraction/extract_para_edge.py:132-257),
written with its numpy expressions and vectorised over the edges of a frame, for the visibility tests.
tests/test_edge_visibility_cpu.py pins it to the reference-generated fixture (tests/golden/make_visibility_golden.py);
the GPU tests compare the kernel with it."""
import math

import numpy as np

from curve_gaussian_amd.scene.dataset_io import sample_edge_points


def map_values(maps_u8, detector):
    """get_edge_maps :49-53: u8 -> float64 value."""
    if detector == "DexiNed":
        return 1 - maps_u8 / 255.0
    if detector == "PidiNet":
        return maps_u8 / 255.0
    raise ValueError(f"Unknown detector: {detector}")


def edge_points(curves, lines):
    """The projected points of every edge, curves (4 control points) then lines (2 end points): (points [n,3],
    edge index [n], slot within the edge [n])."""
    c = np.asarray(curves, np.float64).reshape(-1, 4, 3)
    ln = np.asarray(lines, np.float64).reshape(-1, 2, 3)
    pts = np.concatenate([c.reshape(-1, 3), ln.reshape(-1, 3)])
    eid = np.concatenate([np.repeat(np.arange(len(c)), 4), len(c) + np.repeat(np.arange(len(ln)), 2)])
    slot = np.concatenate([np.tile(np.arange(4), len(c)), np.tile(np.arange(2), len(ln))])
    return pts, eid.astype(np.int64), slot.astype(np.int64)


def project(intrinsic, camtoworld, pts):
    """compute_visibility :173-176 + project2D_single :132-142: [n,2] projected coordinates (inf / NaN at depth 0)."""
    K = intrinsic[:3, :3]
    worldtocam = np.linalg.inv(camtoworld)
    R = worldtocam[:3, :3]
    T = worldtocam[:3, 3:]
    x = K @ (R @ pts.T + T)
    x = x.T
    with np.errstate(divide="ignore", invalid="ignore"):
        x = x / x[:, -1:]
    return x[:, :2]


def visibility_counts(curves, lines, values, intrinsics, camtoworld, h, w, threshold=0.1, return_uv=False):
    """compute_visibility :145-197 with the edge_visibility_matrix summed over frames: per edge, the number of frames in
    which mean(values) > threshold and max(values) > 0.5 over its projected points that land in the image.  The mean is
    summed left to right in point order and divided by the number of points, which is what np.mean does over <= 4
    float64 values.  `values`: float64 [F,H,W] (map_values).  return_uv=True also returns the projected coordinates
    [F,n,2]."""
    pts, eid, slot = edge_points(curves, lines)
    n_edges = int(np.asarray(curves).reshape(-1, 12).shape[0] + np.asarray(lines).reshape(-1, 6).shape[0])
    counts = np.zeros(n_edges, np.int64)
    uvs = []
    for f in range(len(values)):
        uv = project(np.asarray(intrinsics[f], np.float64), np.asarray(camtoworld[f], np.float64)[:4, :4], pts)
        if return_uv:
            uvs.append(uv)
        with np.errstate(invalid="ignore"):
            edge_uv = np.round(uv).astype(np.int32)
        u, v = edge_uv[:, 0], edge_uv[:, 1]
        valid = (u >= 0) & (u < w) & (v >= 0) & (v < h)
        val = np.zeros(len(pts))
        val[valid] = values[f][v[valid], u[valid]]
        s = np.zeros((n_edges, 4))
        mx = np.full((n_edges, 4), -np.inf)
        s[eid, slot] = np.where(valid, val, 0.0)                  # x + 0.0 == x: invalid points add nothing
        mx[eid, slot] = np.where(valid, val, -np.inf)
        nvalid = np.zeros(n_edges, np.int64)
        np.add.at(nvalid, eid, valid.astype(np.int64))
        total = ((s[:, 0] + s[:, 1]) + s[:, 2]) + s[:, 3]
        with np.errstate(divide="ignore", invalid="ignore"):
            mean = total / nvalid
        cell = (nvalid > 0) & (mean > threshold) & (mx.max(1) > 0.5)
        counts += cell
    return (counts, np.array(uvs).reshape(len(values), len(pts), 2)) if return_uv else counts


def parametric_edges(curves, lines, counts, n_frames):
    """get_parametric_edge :200-249 given the counts: (pred_points float32, return_edge_dict, curve_mask, line_mask)."""
    c = np.asarray(curves, np.float64).reshape(-1, 4, 3)
    ln = np.asarray(lines, np.float64).reshape(-1, 6)
    keep = counts > math.ceil(0.05 * n_frames)
    cm, lm = keep[:len(c)], keep[len(c):]
    c, ln = c[cm], ln[lm]
    return sample_edge_points(c, ln), {"curves_ctl_pts": c.tolist(), "lines_end_pts": ln.tolist()}, cm, lm
