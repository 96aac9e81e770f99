"""ABC evaluation: the host-side loaders (numpy, like scene.dataset_io) and the per-scan / per-dataset metrics of the
reference's evaluator (edge_extraction/eval_ABC.py:140-330, eval_utils.py:251-497), with every nearest-neighbour query
on the GPU (ops.nearest_neighbors)."""
import json
import logging
import os
from typing import NamedTuple

import numpy as np
import torch

from ..scene.dataset_io import bezier_curve_length
from . import ops

log = logging.getLogger(__name__)

_BEZIER = np.array([[-1, 3, -3, 1], [3, -6, 3, 0], [-3, 3, 0, 0], [1, 0, 0, 0]])
_RENAME = {"BSpline": "curve", "Circle": "curve", "Ellipse": "curve", "Line": "line"}


class PredEdges(NamedTuple):
    curve_points: np.ndarray       # [Nc,3] float64
    line_points: np.ndarray        # [Nl,3] float64
    curve_directions: np.ndarray   # [Nc,3] float64, unit derivative
    line_directions: np.ndarray    # [Nl,3] float64
    curve_counts: np.ndarray       # samples per curve
    line_counts: np.ndarray        # samples per line
    num_curves: int
    num_lines: int

    @property
    def points(self):
        """All pred points, curves first, as float32 (eval_ABC.py:165-169)."""
        return np.concatenate([self.curve_points, self.line_points], 0).reshape(-1, 3).astype(np.float32)

    @property
    def directions(self):
        """All pred directions, float32 like eval_ABC.py:152-163."""
        return np.concatenate([self.curve_directions, self.line_directions], 0).reshape(-1, 3).astype(np.float32)


def pred_points_and_directions(edge_dict_or_json_path, sample_resolution=0.005) -> PredEdges:
    """eval_utils.py:369-497 (colours left out): points every `sample_resolution` of arc length along each cubic Bezier
    (Simpson-rule length, scene.dataset_io.bezier_curve_length) and each line segment, both ends included, with the unit
    derivative at each point.  A line's direction is (p1 - p0) / (|p1 - p0| + 1e-6), as in the reference (:477)."""
    d = edge_dict_or_json_path
    if not isinstance(d, dict):
        with open(d) as f:
            d = json.load(f)
    curves = np.array(d["curves_ctl_pts"], dtype=np.float64).reshape(-1, 3).reshape(-1, 4, 3)
    lines = np.array(d["lines_end_pts"], dtype=np.float64).reshape(-1, 2, 3) if "lines_end_pts" in d else np.zeros((0, 2, 3))
    cp, cd, cn = [np.zeros((0, 3))], [np.zeros((0, 3))], []
    for c in curves:
        n = int(bezier_curve_length(c, 100) // sample_resolution)
        t = np.linspace(0, 1, n)
        U = np.array([t ** 3, t ** 2, t, [1] * n]).reshape(4, n)
        cp.append(np.matmul(np.matmul(U.T, _BEZIER), c).reshape(n, 3))
        # the derivative as the reference spells it out per coordinate (:416-452)
        du, dv = 3 * t ** 2, 2 * t
        der = np.stack([(-3 * c[0][k] + 9 * c[1][k] - 9 * c[2][k] + 3 * c[3][k]) * du
                        + (6 * c[0][k] - 12 * c[1][k] + 6 * c[2][k]) * dv + (-3 * c[0][k] + 3 * c[1][k])
                        for k in range(3)], 1).reshape(n, 3)
        cd.append(der / np.linalg.norm(der, axis=1, keepdims=True))
        cn.append(n)
    lp, ld, ln = [np.zeros((0, 3))], [np.zeros((0, 3))], []
    for e in lines:
        n = int(np.linalg.norm(e[0] - e[-1]) // sample_resolution)
        t = np.linspace(0, 1, n)
        lp.append(np.matmul(np.matmul(np.array([t, [1] * n]).T, np.array([[-1, 1], [1, 0]])), e).reshape(n, 3))
        dirn = e[1] - e[0]
        ld.append(np.repeat((dirn / (np.linalg.norm(dirn) + 1e-6))[None], n, 0))
        ln.append(n)
    return PredEdges(np.concatenate(cp), np.concatenate(lp), np.concatenate(cd), np.concatenate(ld),
                     np.array(cn, dtype=np.int64), np.array(ln, dtype=np.int64), len(curves), len(lines))


def abc_gt_points(data_base_dir, scan_name, edge_type="all", interval=0.005):
    """eval_utils.py:251-366: the sharp feature curves of an ABC scan (``chunk_0000_feats.json``, vertices of
    ``obj/<scan>*.obj``), sampled along their polylines and normalised by the bounding box of ``chunk_0000_stats.json``
    into the unit cube.  `edge_type`: "all", "curve" (BSpline / Circle / Ellipse) or "line".  Returns float32
    (raw vertices, sampled points) and float64 unit directions of the sampled points, or None when there are no sharp
    edges of that type."""
    objs_dir = os.path.join(data_base_dir, "obj")
    index_obj_names = {name[:8]: name for name in sorted(os.listdir(objs_dir))}
    with open(os.path.join(data_base_dir, "chunk_0000_feats.json")) as f:
        feats = json.load(f)
    with open(os.path.join(data_base_dir, "chunk_0000_stats.json")) as f:
        stats = json.load(f)
    x_min, y_min, z_min, x_max, y_max, z_max, x_range, y_range, z_range = stats[scan_name]["bbox"]
    scale = 1 / max(x_range, y_range, z_range)
    center = np.array([(x_min + x_max) / 2, (y_min + y_max) / 2, (z_min + z_max) / 2]) * scale
    shift = [0.5, 0.5, 0.5] - center
    with open(os.path.join(objs_dir, index_obj_names[scan_name]), encoding="utf-8") as f:
        rows = [ln.split(" ") for ln in f.readlines()]
    verts = [[float(v[1]), float(v[2]), float(v[3].replace("\n", ""))] for v in rows if v[0] == "v"]
    raw, pts, dirs = [], [], []
    for feat in feats[scan_name]:
        if edge_type != "all" and _RENAME[feat["type"]] != edge_type:
            continue
        if not feat["sharp"]:
            continue
        poly = np.array([verts[i] for i in feat["vert_indices"]])
        raw += poly.tolist()
        for k in range(len(poly) - 1):
            nxt, cur = poly[k + 1], poly[k]
            # Reference quirks (:331-345): each segment is sampled from `next` to `current` with
            # num = int(|next - current| // interval) points, both ends included -- every interior vertex is emitted
            # twice, each copy with its own segment's direction, and a segment shorter than `interval` adds nothing.
            num = int(np.linalg.norm(nxt - cur) // interval)
            s = np.linspace(0, 1, num)
            pts.append(s[:, None] * cur + (1 - s)[:, None] * nxt)
            dirs += [(nxt - cur) / np.linalg.norm(nxt - cur)] * num
    if not raw:
        return None
    # ... and the GT is then scaled and shifted by the bounding box of chunk_0000_stats.json (:352-354)
    raw = np.array(raw) * scale + shift
    pts = np.concatenate(pts).reshape(-1, 3) * scale + shift
    return raw.astype(np.float32), pts.astype(np.float32), np.array(dirs).reshape(-1, 3)


# ------------------------------------------------------------------------------------------ scan and dataset metrics
KEYS = ("chamfer", "acc", "simi", "num_lines", "num_curves", "comp", "comp_curve", "comp_line", "acc_curve", "acc_line",
        "precision_0.01", "recall_0.01", "fscore_0.01", "IOU_0.01", "precision_0.02", "recall_0.02", "fscore_0.02",
        "IOU_0.02", "precision_0.005", "recall_0.005", "fscore_0.005", "IOU_0.005")


def scan_metrics(pred_sampled, pred_points, pred_dirs, gt, gt_by_type, nn, num_curves, num_lines):
    """The metric part of process_scan (eval_ABC.py:185-237) given the point sets and an NN function
    nn(query, ref) -> (dist, index).  `gt` = (raw, sampled, directions); `gt_by_type` = {"curve": gt or None,
    "line": ...}.  Returns the per-scan values of the reference's metric lists and, per edge type, the counts that
    update_totals_and_metrics (:41-48) adds up."""
    _, gt_pts, gt_dirs = gt
    _, idx = nn(pred_points, gt_pts)
    simi = ops.similarity_from_index(pred_dirs, gt_dirs, idx)
    d_pg, _ = nn(pred_sampled, gt_pts)
    d_gp, _ = nn(gt_pts, pred_sampled)
    chamfer, acc, comp = ops.chamfer_from_distances(d_pg, d_gp)
    # eval_ABC.py:215-216: the reference appends num_lines under "num_curves" and num_curves under "num_lines"
    m = {"chamfer": chamfer, "acc": acc, "simi": simi, "comp": comp, "num_curves": num_lines, "num_lines": num_curves}
    for t, r in ops.precision_recall_from_distances(d_pg, d_gp).items():
        m[f"precision_{t}"], m[f"recall_{t}"], m[f"fscore_{t}"], m[f"IOU_{t}"] = (r["precision"], r["recall"],
                                                                                r["fscore"], r["iou"])
    per_type = {}
    for et in ("curve", "line"):
        g = gt_by_type.get(et)
        if g is None:
            continue
        e_pg, _ = nn(pred_sampled, g[1])
        e_gp, _ = nn(g[1], pred_sampled)
        _, e_acc, e_comp = ops.chamfer_from_distances(e_pg, e_gp)
        pr = ops.precision_recall_from_distances(e_pg, e_gp)
        m[f"comp_{et}"], m[f"acc_{et}"] = e_comp, e_acc
        per_type[et] = {"correct_gt": [pr[t]["correct_gt"] for t in ops.THRESHOLDS],
                        "correct_pred": [pr[t]["correct_pred"] for t in ops.THRESHOLDS],
                        "num_gt": pr[ops.THRESHOLDS[0]]["num_gt"], "num_pred": pr[ops.THRESHOLDS[0]]["num_pred"]}
    return m, per_type


def _gpu_nn(device):
    def nn(q, r):
        return ops.nearest_neighbors(torch.as_tensor(q).to(device, torch.float32).reshape(-1, 3),
                                     torch.as_tensor(r).to(device, torch.float32).reshape(-1, 3))
    return nn


def evaluate_abc_scan(parametric_edges_json, gt_dir, scan_name, device="cuda"):
    """process_scan (eval_ABC.py:140-237) for one scan: `parametric_edges_json` is the prediction (path or dict),
    `gt_dir` the ABC ``groundtruth`` directory.  Chamfer, precision and recall use the downsampled pred set
    (ops.downsample_point_cloud_average, 256 voxels per axis over the unit cube); the direction similarity uses the
    full one.  Returns (metrics, per_type_counts) as scan_metrics does, or None for an empty prediction or a scan with
    no sharp edges."""
    dev = torch.device(device)
    pred = pred_points_and_directions(parametric_edges_json)
    pts = pred.points
    if len(pts) == 0:
        log.info(f"Invalid prediction at {scan_name}")
        return None
    gt = abc_gt_points(gt_dir, scan_name, "all")
    if gt is None:
        return None
    pts_d = torch.from_numpy(pts).to(dev)
    sampled = ops.downsample_point_cloud_average(pts_d, 256, (0, 0, 0), (1, 1, 1))
    by_type = {et: abc_gt_points(gt_dir, scan_name, et) for et in ("curve", "line")}
    return scan_metrics(sampled, pts_d, torch.from_numpy(pred.directions).to(dev), gt, by_type, _gpu_nn(dev),
                        pred.num_curves, pred.num_lines)


def new_totals():
    keys = [f"thre{t}_correct_{w}_total" for w in ("gt", "pred") for t in ("5", "10", "20")]
    return {et: dict({k: 0 for k in keys}, num_gt_total=0, num_pred_total=0) for et in ("curve", "line")}


def accumulate(metrics, totals, scan_result):
    """Appends one scan's values to the metric lists and adds its per-type counts to `totals` (eval_ABC.py:41-48, 211-
    237).  The reference accumulates these totals but never prints them."""
    m, per_type = scan_result
    for k, v in m.items():
        metrics[k].append(v)
    for et, c in per_type.items():
        for i, t in enumerate(("5", "10", "20")):
            totals[et][f"thre{t}_correct_gt_total"] += c["correct_gt"][i]
            totals[et][f"thre{t}_correct_pred_total"] += c["correct_pred"][i]
        totals[et]["num_gt_total"] += c["num_gt"]
        totals[et]["num_pred_total"] += c["num_pred"]


def finalize_metrics(metrics):
    """eval_ABC.py:51-56: nan -> 0, mean over the scans, rounded to 4 decimals (the mean of an empty list is nan)."""
    out = {}
    for k, v in metrics.items():
        a = np.array(v, dtype=np.float64)
        a[np.isnan(a)] = 0
        out[k] = round(float(np.mean(a)) if a.size else float("nan"), 4)
    return out


def evaluate_abc(pred_base_dir, dataset_dir, device="cuda"):
    """main (eval_ABC.py:240-330): every scan directory under `dataset_dir` (sorted), with the prediction at
    <pred_base_dir>/<scan>/parametric_edges.json and the ground truth under <dirname(dataset_dir)>/groundtruth.
    Returns (finalised metrics, totals)."""
    metrics = {k: [] for k in KEYS}
    totals = new_totals()
    dataset_dir = os.path.normpath(dataset_dir)
    gt_dir = os.path.join(os.path.dirname(dataset_dir), "groundtruth")
    for scan in sorted(f.name for f in os.scandir(dataset_dir) if f.is_dir()):
        log.info(f"Processing: {scan}")
        path = os.path.join(pred_base_dir, scan, "parametric_edges.json")
        if not os.path.exists(path):
            log.info(f"Invalid prediction at {scan}")
            continue
        r = evaluate_abc_scan(path, gt_dir, scan, device)
        if r is not None:
            m = r[0]
            log.info(f"  Chamfer Distance: {m['chamfer']:.4f}, Accuracy: {m['acc']:.4f}, "
                     f"Completeness: {m['comp']:.4f}    Norm: {m['simi']:.4f}")
            accumulate(metrics, totals, r)
    return finalize_metrics(metrics), totals


def summary_lines(metrics, totals):
    """The reference's summary (eval_ABC.py:300-330)."""
    out = ["Summary:", f"  Number line/curve: {metrics['num_lines']}, {metrics['num_curves']}",
           f"  Accuracy: {metrics['acc']:.4f}", f"  Completeness: {metrics['comp']:.4f}", f"  Norm: {metrics['simi']:.4f}"]
    for name, key in (("Recall", "recall"), ("Precision", "precision"), ("F-Score", "fscore")):
        for mm, t in (("5", "0.005"), ("10", "0.01"), ("20", "0.02")):
            out.append(f"  {name} @ {mm} mm: {metrics[f'{key}_{t}']:.4f}")
    for et in ("curve", "line"):
        if totals[et]["num_gt_total"] > 0:
            out += [f"{et.capitalize()}:", f"  Completeness: {metrics[f'comp_{et}']}", f"  Accuracy: {metrics[f'acc_{et}']}"]
        else:
            out.append(f"{et.capitalize()}: No ground truth edges found.")
    return out
