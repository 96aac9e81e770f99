"""Reprojection score of the extracted edges: ``parametric_edges.json`` projected into every camera of a scan and compared,
in pixels, with that camera's edge map -- precision, recall and F-score at pixel tolerances, 2D accuracy / completeness
(Chamfer) in pixels.  It needs no 3D ground truth, so it also scores Replica, COLMAP and photograph-only scans, and it
scores the product's output (after merging, line fitting, endpoint merging and the visibility check), not the Gaussian
render.  The reference has no counterpart: its eval_replica.py stops at pictures.

The edges are sampled as the novel-view code samples them (``abc.pred_points_and_directions``), every point the projection
rule of ``cgs_project_points`` keeps marks its pixel (``ops.edge_score.point_masks``), a pixel of the edge map is detected
when e > edge_threshold with e = 1 - u/255 (DexiNed) or u/255 (PidiNet) -- the conversions of ``para_edge`` -- and
``ops.edge_score.score_masks`` compares the two masks; its docstring freezes the aggregate.

KNOWN LIMIT: there is no depth.  An edge hidden behind a surface still projects into the view, finds no detected pixel
there and counts against precision and accuracy -- unless the caller has a depth source: with ``occluder`` (a triangle
mesh) or ``depth_maps`` (``--occluder`` / ``--depth_dir``) the hidden samples are left out (``ops.edge_occlusion``, whose
docstring freezes the rule and states its limits; UNTUNED defaults).  The reverse limit: an occluding contour of a curved
surface is a detected edge that no 3D edge explains and counts against recall -- unless ``ignore_contours``
(``--ignore_contours``, with an occluder) takes a zone around the mesh's predicted contours out of both masks
(``ops.mesh_contours``; UNTUNED defaults).

``python -m curve_gaussian_amd.edge_extraction.reprojection --base_dir <predictions> --dataset_dir <scans>`` scores every
scan, writes ``<base_dir>/<scan>/reprojection_score.json`` and prints one line per scan and their mean."""
import argparse
import json
import logging
import math
import os
import sys

import numpy as np
import torch

from ..ops import edge_occlusion as EO
from ..ops import edge_score as ES
from ..ops import mesh_contours as MC
from ..ops.edge_thin import thin_masks
from ..ops.view_chunks import check_edge_maps, detected_lut, detected_masks, view_chunks
from ..scene.dataset_io import fov2focal
from .abc import pred_points_and_directions
from .novel_view import NovelViewCamera, replica_scans
from .para_edge import EDGE_MAX_THRESHOLD, edge_map_paths, get_edge_maps

log = logging.getLogger(__name__)

SAMPLE_RESOLUTION = 0.0005   # the novel views' Replica value (eval_replica.py:113)
LAYOUTS = ("emap", "colmap")
SCORE_FILE = "reprojection_score.json"


def _pred_points(pred, sample_resolution):
    return np.ascontiguousarray(pred_points_and_directions(pred, sample_resolution).points, np.float32).reshape(-1, 3)


def _json_number(x):
    x = float(x)
    return x if math.isfinite(x) else None


def score_edges(pred, cameras, edge_maps_u8, detector, tolerances_px=(1, 2, 4), edge_threshold=EDGE_MAX_THRESHOLD,
                sample_resolution=SAMPLE_RESOLUTION, device=None, backend="gpu", budget_bytes=None, thin=False,
                occluder=None, depth_maps=None, depth_slack=EO.DEPTH_SLACK, depth_window=EO.DEPTH_WINDOW,
                ignore_contours=False, contour_radius_px=MC.CONTOUR_RADIUS_PX, crease_deg=MC.CREASE_DEG, near_clip=None):
    """pred: a ``parametric_edges.json`` path or its dict.  cameras: ``NovelViewCamera`` s (R, T world -> camera; fx, fy, cx,
    cy; size).  edge_maps_u8: one uint8 [H,W] map per camera (a list, or an [V,H,W] array), the stored bytes of the
    detector's maps, each of its camera's size.  Returns {"aggregate": ops.edge_score's aggregate over all views,
    "views": one row per camera in order (name, width, height, kept_points, n_pred, n_det, pred_hits, det_hits,
    accuracy_px, completeness_px, both_nonempty), "settings"}.  Views of one size are scored together, ``budget_bytes``
    (default ops.edge_score.BYTE_BUDGET) of masks and distance transforms at a time.  ``backend``: "gpu" (HIP; ``device``)
    or "host" (numpy).  ``thin``: every chunk's detected masks go through ``ops.edge_thin.thin_masks`` on the same back end
    first (a detector's response several pixels wide makes the recall measure its line width; untuned, limits in
    ops/edge_thin.py); "settings" then holds "thin": true, and nothing otherwise.

    Occlusion (``ops.edge_occlusion``; at most one of the two): ``occluder`` -- float32 [F,3,3] triangles or the path of an
    .obj / .ply mesh -- is rendered into every chunk's depth planes (``mesh_depth``); ``depth_maps`` -- one float [H,W]
    array of camera z per camera, NaN or <= 0 where there is no measurement (``check_depth_maps``) -- are taken as they
    are.  Either way the planes go through the window maximum of radius ``depth_window`` and the prediction masks come
    from ``point_masks_depth`` with ``depth_slack``: a hidden sample marks no pixel.  Every row of "views" then holds
    "hidden_points" (kept_points counts the seen samples that are not hidden), "settings" holds "occluder" (the path, or
    true) or "depth_maps": true, and "depth_slack" and "depth_window"; a chunk's working set grows by
    ``ops.edge_score.DEPTH_BYTES_PER_PIXEL``.  With neither, nothing changes: no key is added.

    A don't-care zone around occluding contours (``ops.mesh_contours``; needs ``occluder``, the mesh whose edges are
    tested): with ``ignore_contours`` every chunk predicts the smooth contours of the occluder -- folds up to ``crease_deg``,
    gated by the chunk's planes -- widens them to ``contour_radius_px`` with the score's distance transform and removes the
    zone from BOTH the prediction masks and the detected masks before they are compared: a pixel beside a contour is
    evidence neither way.  Every row of "views" then holds "contour_pixels" (the drawn contour pixels, before widening),
    "settings" holds "ignore_contours": true, "contour_radius_px" and "crease_deg"; a chunk's working set grows by
    ``ops.edge_score.CONTOUR_BYTES_PER_PIXEL``.  Both defaults are UNTUNED.  Without the flag no key is added and no
    output changes; with it and no occluder (``depth_maps`` have no mesh edges) it is a ValueError.

    ``near_clip`` (opt-in, with ``occluder`` only; ``edge_support``, ``trim_edges``, ``snap_edges`` and ``seed_points`` take it
    the same way): the near plane at which the occluder's triangles and contour rows are clipped instead of being dropped
    (``ops.edge_occlusion.mesh_depth``; ``EO.NEAR_CLIP``, UNTUNED), for cameras that stand INSIDE the occluder.  "settings"
    records "near_clip" only when it is given; with ``depth_maps`` or no depth source it is a ValueError (the caller's maps
    need no clipping)."""
    ES._check_backend(backend)
    EO.check_one_depth_source("score_edges", occluder, depth_maps)
    gated = occluder is not None or depth_maps is not None
    if ignore_contours and occluder is None:
        raise ValueError("score_edges: ignore_contours needs an occluder, the mesh whose contours are predicted"
                         + (" (depth_maps have no mesh edges)" if depth_maps is not None else ""))
    tolerances_px = [float(t) for t in tolerances_px]
    ES.tolerances_squared(tolerances_px)
    lut = detected_lut(detector, edge_threshold)
    cameras, maps = check_edge_maps("score_edges", cameras, edge_maps_u8)
    gate = EO.ChunkDepth("score_edges", cameras, occluder, depth_maps, depth_slack, depth_window, near_clip)
    pts = _pred_points(pred, sample_resolution)
    if backend == "gpu":
        device = ES._device_for([], "score_edges", device)
        pts_b = torch.from_numpy(pts).to(device)
    else:
        pts_b = pts
    gate.to(backend, device)
    if ignore_contours and gate.surfels is not None:
        raise ValueError("score_edges: ignore_contours takes a mesh (a point cloud has no mesh edges to predict contours from)")
    if ignore_contours:
        contour_radius_px = MC._check_radius("score_edges", contour_radius_px)
        contour_rows = MC.edge_rows(gate.tris, "smooth", crease_deg)   # once: the selection is the host's
        if backend == "gpu":
            contour_rows = torch.from_numpy(contour_rows).to(device)
    budget = ES.BYTE_BUDGET if budget_bytes is None else int(budget_bytes)
    V, n_tol = len(cameras), len(tolerances_px)
    per_view = {"n_pred": np.zeros(V, np.int64), "n_det": np.zeros(V, np.int64), "pred_hits": np.zeros((V, n_tol), np.int64),
                "det_hits": np.zeros((V, n_tol), np.int64), "sum_pred_to_det": np.zeros(V, np.float64),
                "sum_det_to_pred": np.zeros(V, np.float64), "both_nonempty": np.zeros(V, bool)}
    kept, hidden, contour_px = np.zeros(V, np.int64), np.zeros(V, np.int64), np.zeros(V, np.int64)
    bytes_per_pixel = ES.BYTES_PER_PIXEL + gate.bytes_per_pixel + (ES.CONTOUR_BYTES_PER_PIXEL if ignore_contours else 0)
    for H, W, sel, intr, w2c in view_chunks(cameras, bytes_per_pixel, budget):
        zone = None
        if gated:
            depth = gate.planes(H, W, sel, intr, w2c)
            pm, k, hid = EO.point_masks_depth(pts_b, intr, w2c, depth, gate.slack, backend=backend, device=device,
                                              return_counts=True)
            hidden[sel] = hid.cpu().numpy()
            if ignore_contours:
                drawn = MC.row_masks(contour_rows, intr, w2c, H, W, depth, gate.slack, backend=backend, device=device,
                                     near_clip=gate.near)
                contour_px[sel] = drawn.sum((1, 2), dtype=torch.int64).cpu().numpy()
                zone = MC.ignore_zone(drawn, contour_radius_px, backend=backend, device=device)
                del drawn
            del depth
        else:
            pm, k = ES.point_masks(pts_b, intr, w2c, H, W, backend=backend, device=device, return_kept=True)
        det = detected_masks(lut, maps, sel)
        if thin:
            det = thin_masks(det, backend=backend, device=device)
        if zone is not None:   # a pixel beside a contour is evidence neither way: out of both masks
            pm, det = pm * ~zone, det.to(zone.device) * ~zone
        res = ES.score_masks(pm, det, tolerances_px, backend=backend, device=device, budget_bytes=budget)
        kept[sel] = k.cpu().numpy()
        for name, a in per_view.items():
            a[sel] = res[name].numpy()
    agg = ES.aggregate_scores(tolerances_px, **per_view)
    rows = []
    for v, c in enumerate(cameras):
        both = bool(per_view["both_nonempty"][v])
        rows.append({"name": c.name, "width": int(c.width), "height": int(c.height), "kept_points": int(kept[v]),
                     "n_pred": int(per_view["n_pred"][v]), "n_det": int(per_view["n_det"][v]),
                     "pred_hits": [int(h) for h in per_view["pred_hits"][v]],
                     "det_hits": [int(h) for h in per_view["det_hits"][v]],
                     "accuracy_px": float(per_view["sum_pred_to_det"][v] / per_view["n_pred"][v]) if both else float("nan"),
                     "completeness_px": float(per_view["sum_det_to_pred"][v] / per_view["n_det"][v]) if both else float("nan"),
                     "both_nonempty": both})
        if gated:
            rows[-1]["hidden_points"] = int(hidden[v])
        if ignore_contours:
            rows[-1]["contour_pixels"] = int(contour_px[v])
    settings = {"detector": detector, "tolerances_px": tolerances_px, "edge_threshold": float(edge_threshold),
                "sample_resolution": float(sample_resolution), "backend": backend, "points": int(pts.shape[0])}
    if thin:
        settings["thin"] = True
    settings.update(gate.settings())
    if ignore_contours:
        settings.update({"ignore_contours": True, "contour_radius_px": contour_radius_px, "crease_deg": float(crease_deg)})
    return {"aggregate": agg, "views": rows, "settings": settings}


# ------------------------------------------------------------------------------------------------ cameras and maps of a scan
def scene_cameras(cams):
    """(NovelViewCamera s, uint8 maps) of the cameras a Scene trains on (``EdgeCamera``: read_emap, read_colmap): R is stored
    transposed there, the focal lengths are those of the field of view at the map's size and the principal point is the
    centre -- the camera the rasterizer uses; the map is channel 0 of ``original_image`` (a stored byte / 255), back as a
    byte."""
    out, maps = [], []
    for c in cams:
        H, W = int(c.image_height), int(c.image_width)
        out.append(NovelViewCamera(c.image_name, np.ascontiguousarray(np.asarray(c.R, np.float64).T),
                                   np.asarray(c.T, np.float64), fov2focal(c.FoVx, W), fov2focal(c.FoVy, H), W / 2.0, H / 2.0,
                                   W, H))
        maps.append(torch.round(c.original_image[0].detach().float().cpu() * 255.0).clamp_(0, 255).to(torch.uint8).numpy())
    return out, maps


def emap_cameras(scan_dir, detector):
    """(NovelViewCamera s, uint8 [F,H,W] maps) of an EMAP scan through ``get_edge_maps``: K = intrinsics[:3,:3] and
    w2c = inv(camtoworld), as the visibility check forms them; a view is named by its frame's ``rgb_path``."""
    maps, intrinsics, camtoworld, h, w = get_edge_maps(scan_dir, detector)
    meta, _ = edge_map_paths(scan_dir, detector)
    cams = []
    for fr, K, c2w in zip(meta["frames"], intrinsics, camtoworld):
        w2c = np.linalg.inv(np.asarray(c2w, np.float64))
        cams.append(NovelViewCamera(os.path.basename(fr["rgb_path"]), np.ascontiguousarray(w2c[:3, :3]), w2c[:3, 3].copy(),
                                    float(K[0][0]), float(K[1][1]), float(K[0][2]), float(K[1][2]), w, h))
    return cams, maps


def colmap_scan_cameras(scan_dir, detector, undistort=False, backend="gpu", resolution=-1):
    """(NovelViewCamera s, uint8 maps) of a COLMAP or Replica scan through ``read_colmap`` (every image; with ``undistort``
    the maps are resampled through each camera's lens model first, on ``backend``)."""
    from ..scene.colmap_io import read_colmap
    train, _, _, _ = read_colmap(scan_dir, detector=detector, resolution=resolution, undistort=undistort,
                                 undistort_backend=backend)
    return scene_cameras(train)


def scan_depth_maps(depth_dir, cams):
    """One array per camera from ``<depth_dir>/<stem of the camera's name>.npy`` (camera z; ``check_depth_maps`` states what
    an entry may hold).  FileNotFoundError, naming the path, for a missing map."""
    out = []
    for c in cams:
        path = os.path.join(depth_dir, os.path.splitext(os.path.basename(c.name))[0] + ".npy")
        if not os.path.isfile(path):
            raise FileNotFoundError(f"no depth map for {c.name}: {path}")
        out.append(np.load(path))
    return out


def write_score(path, result):
    """The result of score_edges (or a dict of them) as JSON; NaN is written as null."""
    def clean(x):
        if isinstance(x, dict):
            return {k: clean(v) for k, v in x.items()}
        if isinstance(x, (list, tuple)):
            return [clean(v) for v in x]
        if isinstance(x, float):
            return _json_number(x)
        return x
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(clean(result), f, indent=1)


def score_scan(base_dir, dataset_dir, scan, layout="emap", detector="DexiNed", undistort=False, tolerances_px=(1, 2, 4),
               edge_threshold=EDGE_MAX_THRESHOLD, sample_resolution=SAMPLE_RESOLUTION, device=None, backend="gpu",
               resolution=-1, thin=False, occluder=None, depth_dir=None, depth_slack=EO.DEPTH_SLACK,
               depth_window=EO.DEPTH_WINDOW, ignore_contours=False, contour_radius_px=MC.CONTOUR_RADIUS_PX,
               crease_deg=MC.CREASE_DEG, near_clip=None):
    """Scores ``<base_dir>/<scan>/parametric_edges.json`` against the ``detector`` edge maps of ``<dataset_dir>/<scan>`` and
    writes ``<base_dir>/<scan>/reprojection_score.json`` = {"scan", "aggregate", "views", "settings"}.  ``layout``: "emap"
    (meta_data.json; cameras and maps through get_edge_maps) or "colmap" (sparse/0, also Replica; through read_colmap, with
    ``undistort`` and ``resolution`` as there); ``thin`` as ``score_edges``.  ``occluder``: the name of a mesh file inside the scan directory
    (``mesh.ply``); ``depth_dir``: the name of a directory inside it that holds one ``<image stem>.npy`` depth map per
    camera (``scan_depth_maps``); with either, ``depth_slack`` and ``depth_window`` as ``score_edges``; ``ignore_contours``,
    ``contour_radius_px`` and ``crease_deg`` as there (they need ``occluder``), and so does ``near_clip`` (the near plane for
    cameras inside the occluder; None: no clipping).  Returns the dict, or None -- after reporting it -- for a scan without a
    prediction, as the reference's tools skip one."""
    ES._check_backend(backend)
    if layout not in LAYOUTS:
        raise ValueError(f"unknown layout {layout!r}: expected one of {LAYOUTS}")
    path = os.path.join(base_dir, scan, "parametric_edges.json")
    if not os.path.exists(path):
        log.info(f"Invalid prediction at {scan}")
        return None
    scan_dir = os.path.join(dataset_dir, scan)
    if layout == "emap":
        if undistort:
            raise ValueError("undistort applies to the colmap layout only")
        cams, maps = emap_cameras(scan_dir, detector)
    else:
        cams, maps = colmap_scan_cameras(scan_dir, detector, undistort, backend, resolution)
    if occluder is not None and depth_dir is not None:
        raise ValueError("score_scan: give an occluder or a depth_dir, not both")
    gate = near_clip_options("score_scan", near_clip, occluder)
    if occluder is not None:
        gate.update(occluder=os.path.join(scan_dir, occluder), depth_slack=depth_slack, depth_window=depth_window)
    elif depth_dir is not None:
        gate = dict(depth_maps=scan_depth_maps(os.path.join(scan_dir, depth_dir), cams), depth_slack=depth_slack,
                    depth_window=depth_window)
    res = score_edges(path, cams, maps, detector, tolerances_px, edge_threshold, sample_resolution, device, backend,
                      thin=thin, **gate, **contour_options(ignore_contours, contour_radius_px, crease_deg))
    res["settings"].update({"layout": layout, "undistort": bool(undistort)})
    out = {"scan": scan, **res}
    write_score(os.path.join(base_dir, scan, SCORE_FILE), out)
    return out


def score_scene(model_path, scene, detector, depth_dir=None, **kw):
    """The driver's ``--reprojection_score``: ``<model_path>/parametric_edges.json`` against the cameras the scene trained
    on and, separately, its test cameras (the held-out ones under ``--eval``; "test" is null when there are none).
    Writes ``<model_path>/reprojection_score.json`` = {"train": ..., "test": ...} and returns it.  ``kw`` go to
    ``score_edges`` (``occluder``: a mesh's path); ``depth_dir``: a directory of ``<image name>.npy`` depth maps
    (``scan_depth_maps``) for the cameras of both splits."""
    pred = os.path.join(model_path, "parametric_edges.json")
    out = {}
    for split, cams in (("train", scene.getTrainCameras()), ("test", scene.getTestCameras())):
        if not len(cams):
            out[split] = None
            continue
        nv_cams, maps = scene_cameras(cams)
        gate = {} if depth_dir is None else {"depth_maps": scan_depth_maps(depth_dir, nv_cams)}
        out[split] = score_edges(pred, nv_cams, maps, detector, **gate, **kw)
    write_score(os.path.join(model_path, SCORE_FILE), out)
    return out


# ------------------------------------------------------------------------------------------------ command line
def scan_line(scan, agg):
    parts = [f"{scan}: views {agg['views']}"]
    for t, p, r, f in zip(agg["tolerances_px"], agg["precision"], agg["recall"], agg["fscore"]):
        parts.append(f"P/R/F @ {t:g} px: {p:.4f} {r:.4f} {f:.4f}")
    parts.append(f"Accuracy: {agg['accuracy_px']:.4f} px")
    parts.append(f"Completeness: {agg['completeness_px']:.4f} px")
    parts.append(f"Chamfer: {agg['chamfer_px']:.4f} px ({agg['chamfer_views']} views)")
    return ", ".join(parts)


def summary_lines(aggregates):
    """The mean over the scored scans of every aggregate figure (NaN figures are left out of their mean)."""
    if not aggregates:
        return ["Summary: no scan scored."]
    mean = lambda xs: float(np.nanmean(xs)) if np.isfinite(xs).any() else float("nan")
    out = [f"Summary (mean over {len(aggregates)} scans):"]
    for k, t in enumerate(aggregates[0]["tolerances_px"]):
        for name, key in (("Precision", "precision"), ("Recall", "recall"), ("F-Score", "fscore")):
            out.append(f"  {name} @ {t:g} px: {mean(np.array([a[key][k] for a in aggregates], np.float64)):.4f}")
    for name, key in (("Accuracy", "accuracy_px"), ("Completeness", "completeness_px"), ("Chamfer", "chamfer_px")):
        out.append(f"  {name}: {mean(np.array([a[key] for a in aggregates], np.float64)):.4f} px")
    return out


def dataset_scans(dataset_dir, layout, scans_file=None):
    """The lines of `scans_file`, or every scan directory of `dataset_dir` of that layout, sorted."""
    if scans_file is not None or layout == "colmap":
        return replica_scans(dataset_dir, scans_file)
    return sorted(f.name for f in os.scandir(dataset_dir)
                  if f.is_dir() and os.path.isfile(os.path.join(f.path, "meta_data.json")))


def parser():
    ap = argparse.ArgumentParser(description="Score parametric edges in 2D against a scan's edge maps.")
    ap.add_argument("--base_dir", default="./output", help="directory holding <scan>/parametric_edges.json")
    ap.add_argument("--dataset_dir", required=True, help="directory holding the scans")
    ap.add_argument("--scans", default=None, help="file with one scan name per line (default: every scan of --dataset_dir)")
    ap.add_argument("--layout", choices=LAYOUTS, default="emap")
    ap.add_argument("--detector", default="DexiNed")
    ap.add_argument("--tolerances", nargs="+", type=float, default=[1, 2, 4], help="pixel tolerances")
    ap.add_argument("--edge_threshold", type=float, default=EDGE_MAX_THRESHOLD)
    ap.add_argument("--undistort", action="store_true", help="colmap layout: resample the edge maps through the lens model")
    ap.add_argument("--backend", choices=ES.SCORE_BACKENDS, default="gpu")
    ap.add_argument("--thin", action="store_true", help="thin the detected masks first (a thick detector response; untuned)")
    add_depth_arguments(ap)
    return ap


def contour_options(ignore_contours, contour_radius_px=MC.CONTOUR_RADIUS_PX, crease_deg=MC.CREASE_DEG):
    """The keyword arguments of ``score_edges`` for the don't-care zone: none without the flag."""
    if not ignore_contours:
        return {}
    return {"ignore_contours": True, "contour_radius_px": contour_radius_px, "crease_deg": crease_deg}


def near_clip_options(what, near_clip, occluder):
    """The keyword arguments of a scan-level operator for the near plane: none without it; a ValueError without an occluder."""
    if near_clip is None:
        return {}
    if occluder is None:
        raise ValueError(f"{what}: near_clip needs an occluder (depth maps need no clipping)")
    return {"near_clip": near_clip}


def add_gate_arguments(ap):
    """The depth source alone -- --occluder, --near_clip, --depth_dir, --depth_slack, --depth_window --, for the tools that
    have no contour options (the visibility filter and the drawn views); ``check_gate_arguments`` after parsing."""
    ap.add_argument("--occluder", default=None, metavar="FILE",
                    help="a mesh or point cloud file inside each scan directory (mesh.ply, .obj; a .ply without faces, such as "
                         "COLMAP's fused.ply, is drawn as disks): samples hidden behind it are left out")
    ap.add_argument("--near_clip", nargs="?", type=float, const=EO.NEAR_CLIP, default=None, metavar="VALUE",
                    help="with a mesh --occluder: clip the mesh at this camera depth instead of dropping a triangle that reaches "
                         f"behind the camera, for cameras INSIDE the mesh (bare flag: {EO.NEAR_CLIP}, world units; untuned; "
                         "an error with a point cloud)")
    ap.add_argument("--depth_dir", default=None, metavar="DIR",
                    help="a directory inside each scan holding <image stem>.npy depth maps (camera z) instead of a mesh")
    ap.add_argument("--depth_slack", type=float, default=EO.DEPTH_SLACK, help="world units behind the surface (untuned)")
    ap.add_argument("--depth_window", type=int, default=EO.DEPTH_WINDOW,
                    help="radius of the window maximum over the depth planes (untuned)")


def check_gate_arguments(ap, args):
    """The parser errors of ``add_gate_arguments``: both depth sources, and --near_clip without --occluder."""
    if args.occluder is not None and args.depth_dir is not None:
        ap.error("give one depth source: --occluder or --depth_dir, not both")
    if args.near_clip is not None and args.occluder is None:
        ap.error("--near_clip needs --occluder: the mesh that is clipped")


def gate_arguments(args):
    """The depth keywords of a scan driver from parsed ``add_gate_arguments``: {} without a depth source."""
    if args.occluder is None and args.depth_dir is None:
        return {}
    return dict(occluder=args.occluder, depth_dir=args.depth_dir, depth_slack=args.depth_slack,
                depth_window=args.depth_window, near_clip=args.near_clip)


def add_depth_arguments(ap):
    """The depth source of the score (shared with train.py --reprojection_score); without them nothing changes."""
    add_gate_arguments(ap)
    ap.add_argument("--ignore_contours", action="store_true",
                    help="with a mesh --occluder: leave a zone around the mesh's predicted occluding contours out of the score "
                         "(an error with a point cloud)")
    ap.add_argument("--contour_radius_px", type=float, default=MC.CONTOUR_RADIUS_PX, help="radius of that zone (untuned)")
    ap.add_argument("--crease_deg", type=float, default=MC.CREASE_DEG,
                    help="mesh edges folded by up to this angle are smooth: candidates for a contour (untuned)")


def main(argv=None):
    args = parser().parse_args(argv)
    aggregates = []
    for scan in dataset_scans(args.dataset_dir, args.layout, args.scans):
        res = score_scan(args.base_dir, args.dataset_dir, scan, args.layout, args.detector, args.undistort, args.tolerances,
                         args.edge_threshold, backend=args.backend, thin=args.thin, occluder=args.occluder,
                         depth_dir=args.depth_dir, depth_slack=args.depth_slack, depth_window=args.depth_window,
                         ignore_contours=args.ignore_contours, contour_radius_px=args.contour_radius_px,
                         crease_deg=args.crease_deg, near_clip=args.near_clip)
        if res is None:
            print(f"Invalid prediction at {scan}")
            continue
        aggregates.append(res["aggregate"])
        print(scan_line(scan, res["aggregate"]))
    for line in summary_lines(aggregates):
        print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
