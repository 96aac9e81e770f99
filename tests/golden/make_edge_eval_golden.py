#!/usr/bin/env python
"""Generates the edge-evaluation fixture: the synthetic ABC-style dataset under tests/golden/edge_eval/ (ground truth,
per-scan predictions) and tests/golden/edge_eval/edge_eval.npz, by IMPORTING the reference's own evaluator and calling
its functions on CPU (runs only where the reference checkout exists; the fixture files travel, the reference does not).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_edge_eval_golden.py

What is called: edge_extraction/eval_utils.py  get_gt_points :251-366, get_pred_points_and_directions :369-497,
bezier_curve_length :139-192 (per-curve sample counts), compute_chamfer_distance :118-131, compute_precision_recall_IOU
:195-249; edge_extraction/eval_ABC.py  compute_direction_similarity :27-38, update_totals_and_metrics :41-48,
finalize_metrics :51-56; edge_extraction/merging.py  merge_endpoints :10-54 (real scipy cdist / connected_components).
process_scan / main (eval_ABC.py:140-330) are restated below call for call (their plotting, logging and the voxel
downsampling are not called); the pred set fed to the metric functions is downsampled by `downsample_documented`, the
semantics ops.downsample_point_cloud_average documents, so nothing is pinned through point_cloud_utils' downsampling.

How it is imported: through make_model_golden.import_reference (empty placeholders for the absent packages, poisoned
before anything is called).  Exactly two substitutions, everything else is the reference's unmodified code:
  1. point_cloud_utils.k_nearest_neighbors(x, y, k=1) is an exact scipy cKDTree query (exact 1-NN distances are
     unambiguous).  Every other attribute of point_cloud_utils -- downsample_point_cloud_on_voxel_grid among them --
     stays poisoned.
  2. utils.vis_utils.get_fancy_color returns constant colours (seaborn is absent; colours enter no metric)."""
import json
import os
import shutil
import sys
import types

import numpy as np
import torch
from scipy.spatial import cKDTree

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_model_golden import _ARMED, import_reference  # noqa: E402

OUT = os.path.join(HERE, "edge_eval")
THRESH = [0.005, 0.01, 0.02]


def _pcu():
    m = types.ModuleType("point_cloud_utils")

    def k_nearest_neighbors(x, y, k=1, squared_distances=False, max_points_per_leaf=10):      # substitution 1
        assert k == 1 and not squared_distances
        d, i = cKDTree(np.asarray(y)).query(np.asarray(x), k=1)
        return d, i

    def _getattr(attr):
        if attr.startswith("__"):
            raise AttributeError(attr)
        raise RuntimeError(f"reference code reached for point_cloud_utils.{attr}: nothing may be pinned through it")

    m.k_nearest_neighbors = k_nearest_neighbors
    m.__getattr__ = _getattr
    return m


def downsample_documented(points, n=256, lo=(0.0, 0.0, 0.0), hi=(1.0, 1.0, 1.0)):
    """numpy statement of curve_gaussian_amd.edge_extraction.downsample_point_cloud_average's documented semantics."""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    p = p[((p >= lo) & (p <= hi)).all(1)]
    v = np.minimum(np.floor((p - lo) / ((hi - lo) / n)).astype(np.int64), n - 1)
    vid = (v[:, 0] * n + v[:, 1]) * n + v[:, 2]
    u, inv = np.unique(vid, return_inverse=True)
    s = np.zeros((len(u), 3))
    np.add.at(s, inv, p)
    c = np.bincount(inv, minlength=len(u)).astype(np.float64)
    return (s / c[:, None]).astype(np.float32)


# ------------------------------------------------------------------------------------------ synthetic dataset
SCANS = ["00000011", "00000022", "00000033"]


def _write_dataset(rng):
    """ABC layout: groundtruth/{chunk_0000_feats.json, chunk_0000_stats.json, obj/<scan>_*.obj}, data/<scan>/ and a
    prediction pred/<scan>/parametric_edges.json per scan."""
    if os.path.exists(OUT):
        shutil.rmtree(OUT)
    os.makedirs(os.path.join(OUT, "groundtruth", "obj"))
    feats, stats, preds = {}, {}, {}
    for si, scan in enumerate(SCANS):
        verts, fl = [], []

        def poly(pts, typ, sharp=True):
            base = len(verts)
            verts.extend(np.asarray(pts).tolist())
            fl.append({"type": typ, "sharp": sharp, "vert_indices": list(range(base, base + len(pts)))})

        off = np.array([3.0 * si, -2.0, 1.0])
        curves, lines = [], []
        if si < 2:
            # a circle (radius 6 of a 20-unit box: ~0.3 of the unit cube), closed polyline of 48 vertices
            a = np.linspace(0, 2 * np.pi, 49)
            circ = off + np.stack([6 * np.cos(a), 6 * np.sin(a), np.zeros_like(a)], 1)
            poly(circ, "Circle")
            # a B-spline-like wave with some vertices closer than 5 mm after scaling (0.1 units = 5 mm)
            x = np.concatenate([np.linspace(-8, -2, 13), [-1.96, -1.93], np.linspace(-1.0, 8, 10)])
            bs = off + np.stack([x, 2 * np.sin(x / 3), 3 + 0.2 * x], 1)
            poly(bs, "BSpline")
            # lines: three edges of a box, one of them not sharp
            poly(off + np.array([[-8, -8, -6], [8, -8, -6]]), "Line")
            poly(off + np.array([[8, -8, -6], [8, 8, -6]]), "Line")
            poly(off + np.array([[8, 8, -6], [-8, 8, -6]]), "Line", sharp=False)
            if si == 1:
                poly(off + np.array([[-8, 8, 6], [-8, 8, 6.05], [-8, 8, 9]]), "Line")   # a first segment < 5 mm
                poly(off + 6 * np.stack([np.cos(a[:25]), np.zeros(25), np.sin(a[:25])], 1), "Ellipse", sharp=False)
            # a box 20 wide in x sets the scale: 1/20 per unit
            lo_, hi_ = off - 10, off + 10
        else:
            poly(off + np.array([[-5, 0, 0], [5, 0, 0]]), "Line", sharp=False)
            poly(off + 6 * np.stack([np.cos(np.linspace(0, 3, 20)), np.sin(np.linspace(0, 3, 20)), np.zeros(20)], 1),
                 "BSpline", sharp=False)
            lo_, hi_ = off - 10, off + 10
        bbox = list(lo_) + list(hi_) + list(hi_ - lo_)
        stats[scan] = {"bbox": [float(b) for b in bbox]}
        feats[scan] = fl
        with open(os.path.join(OUT, "groundtruth", "obj", f"{scan}_synthetic_trimesh.obj"), "w") as f:
            for v in verts:
                f.write("v %.6f %.6f %.6f\n" % tuple(v))
            f.write("f 1 2 3\n")
        # prediction in the unit cube: the scaled features, perturbed by a few mm, as Beziers and lines
        scale = 1 / 20.0
        shift = 0.5 - (lo_ + hi_) / 2 * scale
        to_unit = lambda p: np.asarray(p) * scale + shift
        if si < 2:
            for q in range(4):                      # the circle as four noisy quarter Beziers, endpoints within 15 mm
                t0, t1 = q * np.pi / 2, (q + 1) * np.pi / 2
                k = 4 / 3 * np.tan(np.pi / 8) * 6
                p0 = off + [6 * np.cos(t0), 6 * np.sin(t0), 0]
                p3 = off + [6 * np.cos(t1), 6 * np.sin(t1), 0]
                p1 = p0 + k * np.array([-np.sin(t0), np.cos(t0), 0])
                p2 = p3 - k * np.array([-np.sin(t1), np.cos(t1), 0])
                cps = to_unit(np.stack([p0, p1, p2, p3])) + rng.normal(0, 0.003, (4, 3))
                curves.append(cps)
            xs = np.array([-8, -4, 0, 4, 8.0])
            wave = off + np.stack([xs, 2 * np.sin(xs / 3), 3 + 0.2 * xs], 1)
            curves.append(to_unit(wave[[0, 1, 2, 3]]) + rng.normal(0, 0.004, (4, 3)))
            lines.append(np.concatenate([to_unit(off + [-8, -8, -6]), to_unit(off + [0.3, -8, -6])]) + rng.normal(0, 0.004, 6))
            lines.append(np.concatenate([to_unit(off + [0.1, -8, -6]), to_unit(off + [8, -8, -6])]) + rng.normal(0, 0.004, 6))
            lines.append(np.concatenate([to_unit(off + [8, -7.9, -6]), to_unit(off + [8, 8, -6])]) + rng.normal(0, 0.004, 6))
            lines.append(np.concatenate([to_unit(off + [8, 8, -6]), to_unit(off + [-8, 8, -6])]) + rng.normal(0, 0.004, 6))
            lines.append(rng.uniform(0.2, 0.8, 6))  # a spurious one
        else:
            lines.append(np.array([0.3, 0.5, 0.5, 0.7, 0.5, 0.5]))
            curves.append(rng.uniform(0.3, 0.7, (4, 3)))
        preds[scan] = {"curves_ctl_pts": np.asarray(curves).reshape(-1, 4, 3).tolist(),
                       "lines_end_pts": np.asarray(lines).reshape(-1, 6).tolist()}
        os.makedirs(os.path.join(OUT, "data", scan))
        with open(os.path.join(OUT, "data", scan, "README"), "w") as f:
            f.write("scan directory placeholder: the evaluator lists the scans from here\n")
        os.makedirs(os.path.join(OUT, "pred", scan))
        with open(os.path.join(OUT, "pred", scan, "parametric_edges.json"), "w") as f:
            json.dump(preds[scan], f)
    with open(os.path.join(OUT, "groundtruth", "chunk_0000_feats.json"), "w") as f:
        json.dump(feats, f)
    with open(os.path.join(OUT, "groundtruth", "chunk_0000_stats.json"), "w") as f:
        json.dump(stats, f)


def main():
    sys.modules["point_cloud_utils"] = _pcu()
    EU = import_reference("edge_extraction.eval_utils")
    EA = import_reference("edge_extraction.eval_ABC")
    MRG = import_reference("edge_extraction.merging")
    EU.get_fancy_color = lambda num: torch.full((num, 3), 0.5)          # substitution 2
    _ARMED[0] = True
    torch.manual_seed(0)
    rng = np.random.default_rng(20261015)
    _write_dataset(rng)
    out = {"scans": np.array(SCANS)}
    gt_dir = os.path.join(OUT, "groundtruth")

    # ---------------------------------------------------------------- loaders
    for scan in SCANS:
        for et in ("all", "curve", "line"):
            raw, pts, dirs, _ = EU.get_gt_points(scan, et, return_direction=True, data_base_dir=gt_dir)
            out[f"gt_{scan}_{et}_none"] = np.array(raw is None)
            if raw is not None:
                out[f"gt_{scan}_{et}_raw"], out[f"gt_{scan}_{et}_pts"], out[f"gt_{scan}_{et}_dirs"] = raw, pts, dirs
        jp = os.path.join(OUT, "pred", scan, "parametric_edges.json")
        cpts, lpts, cdir, ldir, _, _, nc, nl = EU.get_pred_points_and_directions(jp)
        d = json.load(open(jp))
        out[f"pred_{scan}_curve_counts"] = np.array(
            [int(EU.bezier_curve_length(np.array(c), num_samples=100) // 0.005) for c in d["curves_ctl_pts"]], np.int64)
        out[f"pred_{scan}_line_counts"] = np.array(
            [int(np.linalg.norm(np.array(e[:3]) - np.array(e[3:])) // 0.005) for e in d["lines_end_pts"]], np.int64)
        out[f"pred_{scan}_curve_points"], out[f"pred_{scan}_line_points"] = cpts, lpts
        out[f"pred_{scan}_curve_dirs"] = np.asarray(cdir, np.float64).reshape(-1, 3)
        out[f"pred_{scan}_line_dirs"] = np.asarray(ldir, np.float64).reshape(-1, 3)
        out[f"pred_{scan}_num"] = np.array([nc, nl])

    # ---------------------------------------------------------------- process_scan / main, call for call
    metrics = {k: [] for k in ("chamfer", "acc", "simi", "num_lines", "num_curves", "comp", "comp_curve", "comp_line",
                               "acc_curve", "acc_line", "precision_0.01", "recall_0.01", "fscore_0.01", "IOU_0.01",
                               "precision_0.02", "recall_0.02", "fscore_0.02", "IOU_0.02", "precision_0.005",
                               "recall_0.005", "fscore_0.005", "IOU_0.005")}
    tkeys = ["thre5_correct_gt_total", "thre10_correct_gt_total", "thre20_correct_gt_total", "thre5_correct_pred_total",
             "thre10_correct_pred_total", "thre20_correct_pred_total", "num_gt_total", "num_pred_total"]
    totals = {"curve": {k: 0 for k in tkeys}, "line": {k: 0 for k in tkeys}}
    for scan in SCANS:
        jp = os.path.join(OUT, "pred", scan, "parametric_edges.json")
        cpts, lpts, cdir, ldir, _, _, nc, nl = EU.get_pred_points_and_directions(jp)                   # :146-149
        cdir = np.asarray(cdir).reshape(-1, 3).astype(np.float32) if len(cdir) else np.zeros((0, 3), np.float32)
        ldir = np.asarray(ldir).reshape(-1, 3).astype(np.float32) if len(ldir) else np.zeros((0, 3), np.float32)
        pred_dirs = np.concatenate([cdir, ldir], 0)
        pred_pts = np.concatenate([cpts, lpts], 0).reshape(-1, 3).astype(np.float32)
        sampled = downsample_documented(pred_pts)                                                     # :180-185
        out[f"pred_{scan}_sampled"] = sampled
        raw, gt_pts, gt_dirs, _ = EU.get_gt_points(scan, "all", data_base_dir=gt_dir, return_direction=True)
        out[f"scan_{scan}_valid"] = np.array(raw is not None)
        if raw is None:
            continue
        simi = EA.compute_direction_similarity(pred_pts, pred_dirs, gt_pts, gt_dirs)
        chamfer, acc, comp = EU.compute_chamfer_distance(sampled, gt_pts)
        # ties of the similarity's NN: pred points with more than one GT point at the minimal distance
        dd = np.linalg.norm(pred_pts[:, None, :].astype(np.float64) - gt_pts[None].astype(np.float64), axis=-1)
        out[f"scan_{scan}_simi_ties"] = np.array(int(((dd - dd.min(1, keepdims=True)) <= 1e-7).sum(1).__gt__(1).sum()))
        metrics["chamfer"].append(chamfer)
        metrics["acc"].append(acc)
        metrics["simi"].append(simi)
        metrics["comp"].append(comp)
        metrics["num_curves"].append(nl)
        metrics["num_lines"].append(nc)
        metrics = EU.compute_precision_recall_IOU(sampled, gt_pts, metrics, thresh_list=THRESH, edge_type="all")
        for k, v in metrics.items():
            out[f"scan_{scan}_{k}"] = np.array(v[-1] if v else np.nan, np.float64)
        for et in ("curve", "line"):
            r2, g2, _, _ = EU.get_gt_points(scan, et, return_direction=True, data_base_dir=gt_dir)
            if r2 is not None:
                res = EU.compute_precision_recall_IOU(sampled, g2, None, thresh_list=THRESH, edge_type=et)
                EA.update_totals_and_metrics(metrics, totals[et], res, et)
                cg, ng, cp, npred, a2, c2 = res
                out[f"scan_{scan}_{et}_counts"] = np.array(list(cg) + [ng] + list(cp) + [npred], np.int64)
                out[f"scan_{scan}_acc_{et}"], out[f"scan_{scan}_comp_{et}"] = np.array(a2), np.array(c2)
    fin = EA.finalize_metrics(metrics)
    out["final_keys"] = np.array(list(fin.keys()))
    out["final_values"] = np.array([fin[k] for k in fin], np.float64)
    out["totals_keys"] = np.array(tkeys)
    out["totals_curve"] = np.array([totals["curve"][k] for k in tkeys], np.int64)
    out["totals_line"] = np.array([totals["line"][k] for k in tkeys], np.int64)

    # ---------------------------------------------------------------- merge_endpoints (float64 and float32 inputs)
    g = np.random.default_rng(7)
    base = g.uniform(0.2, 0.8, (6, 3))
    near = lambda k, s=0.006: base[k] + g.normal(0, s, 3)
    lines = np.stack([np.concatenate([near(0), near(1)]), np.concatenate([near(1), near(2)]),
                      np.concatenate([near(3), g.uniform(0, 1, 3)]), np.concatenate([near(2), near(4)])])
    curves = np.stack([np.concatenate([near(0), g.uniform(0, 1, 6), near(5)]),
                       np.concatenate([near(4), g.uniform(0, 1, 6), near(3)]),
                       np.concatenate([g.uniform(0, 1, 3), g.uniform(0, 1, 6), g.uniform(0, 1, 3)])])
    cases = {"mixed": (lines, curves), "lines_only": (lines, np.zeros((0, 12))), "curves_only": (np.zeros((0, 6)), curves),
             "no_merge": (np.array([[0.1, 0.1, 0.1, 0.4, 0.1, 0.1]]), np.array([np.linspace(0.5, 0.9, 12)]))}
    for name, (ln, cv) in cases.items():
        ml, mc = MRG.merge_endpoints(ln.copy(), cv.copy(), distance_threshold=0.015)
        out[f"merge_{name}_lines_in"], out[f"merge_{name}_curves_in"] = ln, cv
        out[f"merge_{name}_lines"] = np.asarray(ml, np.float64).reshape(-1, 6)
        out[f"merge_{name}_curves"] = np.asarray(mc, np.float64).reshape(-1, 12)
    # a stand-in model's control points (float32, as train.py hands them over): [B,4,3] with is_bezier
    B = 9
    anchors = g.uniform(0.2, 0.8, (4, 3))
    cp = np.zeros((B, 4, 3))
    for b in range(B):
        cp[b, 0] = anchors[b % 4] + g.normal(0, 0.004, 3)
        cp[b, 3] = anchors[(b + 1) % 4] + g.normal(0, 0.004, 3)
        cp[b, 1:3] = cp[b, 0] + g.uniform(-0.05, 0.05, (2, 3))
    cp = cp.astype(np.float32)
    isb = np.array([True, False, True, True, False, True, False, True, True])
    ml, mc = MRG.merge_endpoints(cp[~isb][:, [0, -1], :].reshape(-1, 6), cp[isb].reshape(-1, 12), distance_threshold=0.015)
    out["model_curve_points"], out["model_is_bezier"] = cp, isb
    out["model_merged_lines"], out["model_merged_curves"] = np.asarray(ml), np.asarray(mc)
    np.savez_compressed(os.path.join(OUT, "edge_eval.npz"), **out)
    print("wrote", os.path.join(OUT, "edge_eval.npz"), "scans", SCANS, "final", fin)


if __name__ == "__main__":
    main()
