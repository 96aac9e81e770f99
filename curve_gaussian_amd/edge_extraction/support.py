"""Per-edge 2D support of the extracted edges: every edge of ``parametric_edges.json`` sampled along its length, projected
into every camera of a scan and compared with that camera's detected edge pixels (``ops.edge_support``; its docstring
freezes the verdict).  Unlike the reference's visibility check, which looks at a curve's four control points or a line's
two end points, this says WHICH edge the images do not show along its length; unlike the reprojection score it is one
record per edge.  The reference has no counterpart.

KNOWN LIMITS: without a depth source an edge hidden behind a surface in most views loses its support there, which is why
the rule counts supporting frames and does not pool; a thick detector response inflates support; THE DEFAULTS ARE UNTUNED.
With ``--occluder`` (a mesh inside every scan directory) or ``--depth_dir`` (one ``<image stem>.npy`` per camera), and
``--depth_slack`` / ``--depth_window``, every 2D step run here -- the check, ``--snap`` and ``--trim`` (``--oriented``) --
counts a (sample, view) pair that the depth hides as not seen (``ops.edge_occlusion``: the one rule and its limits --
untuned, drawn solids only, concave edges, no near-plane clipping without ``--near_clip``); the files then record the depth settings and one
hidden total per edge.  Without the flags no file changes by a byte.

``python -m curve_gaussian_amd.edge_extraction.support --base_dir <predictions> --dataset_dir <scans>`` checks every scan,
writes ``<base_dir>/<scan>/edge_support.json`` -- one record per edge -- and, with ``--write_filtered``,
``parametric_edges_supported.json`` with the kept edges.  With ``--trim`` every edge of ``parametric_edges.json`` -- not only
the kept ones: the verdict drops an over-long true edge whole -- is also cut down to the spans of its length that the images
show (``ops.edge_trim``; its docstring freezes the rule and states the limits: no depth, UNTUNED defaults; the duplicates it
leaves are what ``--dedupe`` is for): ``parametric_edges_trimmed.json`` and ``edge_trim.json``, one record per edge.  ``--trim
--oriented`` counts a sample as near only where a detected pixel within the tolerance runs the way the sample's edge does
(``ops.edge_orient``: the rule and its limits; the same two files, fewer stubs where a chord crosses a real edge).  With
``--dedupe`` the parts of the edges that a longer edge already covers in 3D are dropped (``ops.edge_dedupe``; its docstring
freezes the rule and states the limits: the longer edge always wins, one pass, no image evidence, UNTUNED defaults) -- of
the trimmed pieces with ``--trim``, of the edges of ``parametric_edges.json`` without: ``parametric_edges_deduped.json`` and
``edge_dedupe.json``, one record per input edge.  With ``--join`` the ends that the cuts left a few samples short of one
another are rejoined at their junctions (``ops.edge_join``; its docstring freezes the rule and states the limits: 3D only,
hosts of T-junctions are not split, an end joins at most one thing, UNTUNED defaults) -- of the last product of the chain:
the deduped edges with ``--dedupe``, else the trimmed pieces with ``--trim``, else the edges of ``parametric_edges.json``:
``parametric_edges_joined.json`` and ``edge_graph.json``.  With ``--snap`` the edges are first MOVED onto the detected edges
(``ops.edge_snap``; its docstring freezes the rule and states the limits: no depth, a sample within the capture radius of
the wrong edge is pulled to it, not a filter, UNTUNED defaults): ``parametric_edges_snapped.json`` and ``edge_snap.json``, one
record per edge -- and the check and every later step then start from the snapped edges, their files naming
``parametric_edges_snapped.json`` as "input".  ``parametric_edges.json`` is never written, and no option rewrites another
option's files."""
import argparse
import json
import logging
import os
import sys

import numpy as np

from ..ops import edge_dedupe as ED
from ..ops import edge_join as EJ
from ..ops import edge_orient as OR
from ..ops import edge_snap as SN
from ..ops import edge_support as SP
from ..ops import edge_trim as ET
from .para_edge import EDGE_MAX_THRESHOLD, EDGE_VISIBILITY_FRAMES_RATIO
from .reprojection import (LAYOUTS, SAMPLE_RESOLUTION, _json_number, add_depth_arguments, colmap_scan_cameras, dataset_scans,
                           emap_cameras, scan_depth_maps, scene_cameras, write_score)

log = logging.getLogger(__name__)

SUPPORT_FILE = "edge_support.json"
FILTERED_FILE = "parametric_edges_supported.json"
TRIM_FILE = "edge_trim.json"
TRIMMED_FILE = "parametric_edges_trimmed.json"
DEDUPE_FILE = "edge_dedupe.json"
DEDUPED_FILE = "parametric_edges_deduped.json"
GRAPH_FILE = "edge_graph.json"
JOINED_FILE = "parametric_edges_joined.json"
SNAP_FILE = "edge_snap.json"
SNAPPED_FILE = "parametric_edges_snapped.json"
EDGES_FILE = "parametric_edges.json"


def filter_edge_dict(edge_dict, kept):
    """The edges of ``edge_dict`` whose entry of ``kept`` (bool [Nc + Nl], curves first, then lines) is set, as a new dict of
    lists in the layout of ``get_parametric_edge``: curves [n,4,3], lines [n,6]."""
    curves = np.asarray(edge_dict["curves_ctl_pts"], np.float64).reshape(-1, 4, 3)
    lines = np.asarray(edge_dict["lines_end_pts"], np.float64).reshape(-1, 6)
    kept = np.asarray(kept).reshape(-1)
    if kept.dtype != bool or kept.size != len(curves) + len(lines):
        raise ValueError(f"filter_edge_dict: kept must be bool [{len(curves) + len(lines)}] (got {kept.dtype} {kept.shape})")
    return {"curves_ctl_pts": curves[kept[:len(curves)]].tolist(), "lines_end_pts": lines[kept[len(curves):]].tolist()}


def edge_records(result):
    """One record per edge of an ``edge_support`` result: kind ("curve" / "line"), index within its kind, samples, seeing
    views, supporting views and pooled share per tolerance (NaN as None), kept -- and, for a depth-gated result only,
    "hidden_samples": the (sample, view) pairs of the edge that the depth hides, summed over the views."""
    nc = result["curves"]
    rows = []
    for e in range(len(result["n_points"])):
        rows.append({"kind": "curve" if e < nc else "line", "index": int(e if e < nc else e - nc),
                     "samples": int(result["n_points"][e]), "seeing_views": int(result["seeing_views"][e]),
                     "supporting_views": [int(s) for s in result["supporting_views"][e]],
                     "share": [_json_number(s) for s in result["share"][e]], "kept": bool(result["kept"][e])})
        if "hidden" in result:
            rows[-1]["hidden_samples"] = int(np.asarray(result["hidden"][e]).sum())
    return rows


def write_support(model_dir, edge_dict, result, write_filtered=False, extra=None):
    """``<model_dir>/edge_support.json`` = {"edges": edge_records, "kept", "total", "settings", **extra} and, with
    ``write_filtered``, ``<model_dir>/parametric_edges_supported.json``.  Returns the dict written."""
    out = {**(extra or {}), "edges": edge_records(result), "kept": int(np.count_nonzero(result["kept"])),
           "total": int(len(result["kept"])), "settings": dict(result["settings"])}
    write_score(os.path.join(model_dir, SUPPORT_FILE), out)
    if write_filtered:
        with open(os.path.join(model_dir, FILTERED_FILE), "w") as f:
            json.dump(filter_edge_dict(edge_dict, result["kept"]), f)
    return out


def trim_records(result, curves):
    """One record per edge of a ``trim_edges`` result (``curves``: how many of the edges are curves): kind, index within its
    kind, samples, spans as [a, b] pairs, and the kept share of its samples (None for an edge without samples) -- and, for a
    depth-gated result only, "hidden_views": the (sample, view) pairs of the edge that the depth hides, summed over its
    samples."""
    off = result["offsets"].astype(np.int64)
    n = np.diff(off)
    rows = []
    for e, spans in enumerate(result["spans"]):
        kept = sum(b - a + 1 for a, b in spans)
        rows.append({"kind": "curve" if e < curves else "line", "index": int(e if e < curves else e - curves),
                     "samples": int(n[e]), "spans": [[int(a), int(b)] for a, b in spans],
                     "kept_share": kept / int(n[e]) if n[e] > 0 else None})
        if "hidden" in result:
            rows[-1]["hidden_views"] = int(np.asarray(result["hidden"][off[e]:off[e + 1]]).sum())
    return rows


def write_trim(model_dir, edge_dict, result, extra=None):
    """``<model_dir>/edge_trim.json`` = {"edges": trim_records, "total", "pieces", "samples", "kept_samples", "settings",
    **extra} and ``<model_dir>/parametric_edges_trimmed.json``, the pieces.  Returns the first dict."""
    rows = trim_records(result, len(edge_dict["curves_ctl_pts"]))
    out = {**(extra or {}), "edges": rows, "total": len(rows), "pieces": int(len(result["source"])),
           "samples": int(sum(r["samples"] for r in rows)),
           "kept_samples": int(sum(b - a + 1 for r in rows for a, b in r["spans"])), "settings": dict(result["settings"])}
    write_score(os.path.join(model_dir, TRIM_FILE), out)
    with open(os.path.join(model_dir, TRIMMED_FILE), "w") as f:
        json.dump(result["edge_dict"], f)
    return out


def dedupe_records(result, curves):
    """One record per input edge of a ``dedupe_edges`` result (``curves``: how many of the edges are curves): kind, index
    within its kind, samples, redundant samples, ``covered_by`` -- the best-ranked coverer of each of them, as sorted edge
    indices over curves first, then lines; a second, lower-ranked coverer of a sample is not listed -- and the spans that
    are left, as [a, b] pairs."""
    off = result["offsets"].astype(np.int64)
    rows = []
    for e, spans in enumerate(result["spans"]):
        rows.append({"kind": "curve" if e < curves else "line", "index": int(e if e < curves else e - curves),
                     "samples": int(off[e + 1] - off[e]),
                     "redundant_samples": int(np.count_nonzero(result["redundant"][off[e]:off[e + 1]])),
                     "covered_by": [int(b) for b in result["covered_by"][e]], "spans": [[int(a), int(b)] for a, b in spans]})
    return rows


def write_dedupe(model_dir, edge_dict, result, extra=None):
    """``<model_dir>/edge_dedupe.json`` = {"edges": dedupe_records, "total", "pieces", "samples", "redundant_samples",
    "settings", **extra} and ``<model_dir>/parametric_edges_deduped.json``, the pieces.  Returns the first dict."""
    rows = dedupe_records(result, len(edge_dict["curves_ctl_pts"]))
    out = {**(extra or {}), "edges": rows, "total": len(rows), "pieces": int(len(result["source"])),
           "samples": int(sum(r["samples"] for r in rows)),
           "redundant_samples": int(sum(r["redundant_samples"] for r in rows)), "settings": dict(result["settings"])}
    write_score(os.path.join(model_dir, DEDUPE_FILE), out)
    with open(os.path.join(model_dir, DEDUPED_FILE), "w") as f:
        json.dump(result["edge_dict"], f)
    return out


def join_graph(result, curves):
    """The wireframe of a ``join_edges`` result (``curves``: how many of the edges are curves) as plain lists: "vertices"
    [Nv,3]; "edges", per edge its kind, index within its kind and the vertex ids of its first and last end (-1: the edge has
    no sample); "t_junctions", per T-attachment the end, its edge, the host edge, the sample and the parameter on the host,
    the distance, the vertex and whether the host itself moved; "moved", the displacement per end [2E]; "collapsed" and
    "released", as ``join_edges`` reports them; "counts"."""
    ev = result["edge_vertices"]
    edges = [{"kind": "curve" if e < curves else "line", "index": int(e if e < curves else e - curves),
              "vertices": [int(ev[e, 0]), int(ev[e, 1])]} for e in range(len(ev))]
    kind = result["attach"]["kind"]
    counts = {"edges": len(edges), "vertices": int(len(result["vertices"])), "t_junctions": len(result["t_junctions"]),
              "attached_ends": int(np.count_nonzero(kind != EJ.KIND_NONE)), "moved_ends": int(np.count_nonzero(result["moved"] > 0)),
              "collapsed": len(result["collapsed"]), "released": len(result["released"])}
    return {"vertices": result["vertices"].tolist(), "edges": edges, "t_junctions": [dict(t) for t in result["t_junctions"]],
            "moved": [float(m) for m in result["moved"]], "collapsed": list(result["collapsed"]),
            "released": list(result["released"]), "counts": counts}


def write_join(model_dir, edge_dict, result, extra=None):
    """``<model_dir>/edge_graph.json`` = {**join_graph, "settings", **extra} and ``<model_dir>/parametric_edges_joined.json``,
    the joined edges.  Returns the first dict."""
    out = {**(extra or {}), **join_graph(result, len(edge_dict["curves_ctl_pts"])), "settings": dict(result["settings"])}
    write_score(os.path.join(model_dir, GRAPH_FILE), out)
    with open(os.path.join(model_dir, JOINED_FILE), "w") as f:
        json.dump(result["edge_dict"], f)
    return out


def write_snap(model_dir, result, extra=None):
    """``<model_dir>/edge_snap.json`` = {"input": "parametric_edges.json", "edges": the records of ``snap_edges``, "total",
    "moved", "settings", **extra} and ``<model_dir>/parametric_edges_snapped.json``, the snapped edges.  Returns the first
    dict."""
    out = {**(extra or {}), "input": EDGES_FILE, "edges": [dict(r) for r in result["edges"]], "total": len(result["edges"]),
           "moved": int(np.count_nonzero(result["moved"])), "settings": dict(result["settings"])}
    write_score(os.path.join(model_dir, SNAP_FILE), out)
    with open(os.path.join(model_dir, SNAPPED_FILE), "w") as f:
        json.dump(result["edge_dict"], f)
    return out


def score_scan(base_dir, dataset_dir, scan, layout="emap", detector="DexiNed", undistort=False, write_filtered=False,
               device=None, backend="gpu", resolution=-1, trim_options=None, dedupe_options=None, join_options=None,
               snap_options=None, occluder=None, depth_dir=None, depth_slack=None, depth_window=None, **options):
    """Checks ``<base_dir>/<scan>/parametric_edges.json`` against the ``detector`` edge maps of ``<dataset_dir>/<scan>`` and
    writes ``<base_dir>/<scan>/edge_support.json`` (``write_support``).  ``layout``, ``undistort`` and ``resolution`` (of the
    images) as ``reprojection.score_scan``, the same camera loaders; ``options`` go to ``ops.edge_support.edge_support``
    (sampling ``resolution`` as ``sample_resolution``).  ``trim_options`` (a dict, possibly empty; None: no trimming) go to
    ``ops.edge_trim.trim_edges`` on the same cameras and maps, after the check and with its sampling resolution, edge
    threshold and ``thin`` unless they name their own: ``write_trim`` then adds its two files.  ``dedupe_options`` (a dict,
    possibly empty; None: no deduping) go to ``ops.edge_dedupe.dedupe_edges`` on the trimmed pieces when there are any and
    on the edges of the prediction otherwise, with the check's sampling resolution unless they name their own:
    ``write_dedupe`` then adds its two files, and "input" there names the file whose edges went in.  ``join_options`` (a
    dict, possibly empty; None: no joining) go to ``ops.edge_join.join_edges`` on the last product of the chain -- the
    deduped edges, else the trimmed pieces, else the edges of the prediction -- with the check's sampling resolution unless
    they name their own: ``write_join`` then adds its two files, "input" again the file whose edges went in.
    ``snap_options`` (a dict, possibly empty; None: no snapping) go to ``ops.edge_snap.snap_edges`` on the same cameras and
    maps, FIRST, with the check's sampling resolution, edge threshold and ``thin`` unless they name their own: ``write_snap``
    adds its two files, and the check and every later step start from the snapped edges -- ``edge_support.json`` and
    ``edge_trim.json`` then record "input": ``parametric_edges_snapped.json``, and so do the later files where they would have
    named ``parametric_edges.json``.  ``occluder`` (the name of a mesh file inside the scan directory) or ``depth_dir`` (the
    name of a directory inside it with one ``<image stem>.npy`` depth map per camera), at most one, with ``depth_slack`` and
    ``depth_window`` (None: the defaults of ``ops.edge_occlusion``), as ``reprojection.score_scan`` takes them: the depth
    source of the snapping, the check and the trimming alike; ``near_clip`` among the options (the near plane for cameras
    inside the occluder, ``ops.edge_occlusion``) goes to all three as well.  Returns the dict of ``write_support``, with the ones of ``write_trim``, ``write_dedupe`` and ``write_join`` under "trim", "dedupe" and "join"
    when there are any (and the one of ``write_snap`` under "snap"), or None -- after reporting it -- for a scan without a prediction."""
    SP._check_backend(backend)
    if layout not in LAYOUTS:
        raise ValueError(f"unknown layout {layout!r}: expected one of {LAYOUTS}")
    path = os.path.join(base_dir, scan, EDGES_FILE)
    if not os.path.exists(path):
        log.info(f"Invalid prediction at {scan}")
        return None
    with open(path) as f:
        edge_dict = json.load(f)
    scan_dir = os.path.join(dataset_dir, scan)
    if layout == "emap":
        if undistort:
            raise ValueError("undistort applies to the colmap layout only")
        cams, maps = emap_cameras(scan_dir, detector)
    else:
        cams, maps = colmap_scan_cameras(scan_dir, detector, undistort, backend, resolution)
    if "sample_resolution" in options:
        options["resolution"] = options.pop("sample_resolution")
    if occluder is not None and depth_dir is not None:
        raise ValueError("score_scan: give an occluder or a depth_dir, not both")
    if occluder is not None or depth_dir is not None:   # into options: the snapping and the trimming share them below
        if occluder is not None:
            options["occluder"] = os.path.join(scan_dir, occluder)
        else:
            options["depth_maps"] = scan_depth_maps(os.path.join(scan_dir, depth_dir), cams)
        options.update({k: v for k, v in (("depth_slack", depth_slack), ("depth_window", depth_window)) if v is not None})
    gate_keys = ("occluder", "depth_maps", "depth_slack", "depth_window", "near_clip")
    source, extra = EDGES_FILE, {"scan": scan}
    if snap_options is not None:   # first: everything below starts from the snapped edges
        shared = {k: options[k] for k in ("resolution", "edge_threshold", "thin") + gate_keys if k in options}
        snap = SN.snap_edges(edge_dict, cams, maps, detector, device=device, backend=backend, **{**shared, **snap_options})
        snap["settings"].update({"layout": layout, "undistort": bool(undistort)})
        snapped = write_snap(os.path.join(base_dir, scan), snap, extra={"scan": scan})
        edge_dict, source, extra = snap["edge_dict"], SNAPPED_FILE, {"scan": scan, "input": SNAPPED_FILE}
    res = SP.edge_support(edge_dict, cams, maps, detector, device=device, backend=backend, **options)
    res["settings"].update({"layout": layout, "undistort": bool(undistort)})
    out = write_support(os.path.join(base_dir, scan), edge_dict, res, write_filtered, extra=extra)
    if snap_options is not None:
        out["snap"] = snapped
    if trim_options is not None:
        shared = {k: options[k] for k in ("resolution", "edge_threshold", "thin") + gate_keys if k in options}
        trim = ET.trim_edges(edge_dict, cams, maps, detector, device=device, backend=backend, **{**shared, **trim_options})
        trim["settings"].update({"layout": layout, "undistort": bool(undistort)})
        out["trim"] = write_trim(os.path.join(base_dir, scan), edge_dict, trim, extra=extra)
    if dedupe_options is not None:
        given, name = (trim["edge_dict"], TRIMMED_FILE) if trim_options is not None else (edge_dict, source)
        shared = {k: options[k] for k in ("resolution",) if k in options}
        res = ED.dedupe_edges(given, device=device, backend=backend, **{**shared, **dedupe_options})
        out["dedupe"] = write_dedupe(os.path.join(base_dir, scan), given, res, extra={"scan": scan, "input": name})
    if join_options is not None:
        given, name = ((res["edge_dict"], DEDUPED_FILE) if dedupe_options is not None else
                       (trim["edge_dict"], TRIMMED_FILE) if trim_options is not None else (edge_dict, source))
        shared = {k: options[k] for k in ("resolution",) if k in options}
        joined = EJ.join_edges(given, device=device, backend=backend, **{**shared, **join_options})
        out["join"] = write_join(os.path.join(base_dir, scan), given, joined, extra={"scan": scan, "input": name})
    return out


def snap_scene(model_path, edge_dict, cameras, edge_maps, detector, **options):
    """The export's ``snap``: every edge of ``edge_dict`` moved onto the detected edges of the given cameras (as
    ``support_scene`` takes them; ``ops.edge_snap.snap_edges``).  Writes ``edge_snap.json`` and
    ``parametric_edges_snapped.json`` into ``model_path``, prints how many edges moved, and returns (the snapped dict, the
    ``snap_edges`` result)."""
    if edge_maps is None:
        cameras, edge_maps = scene_cameras(cameras)
    res = SN.snap_edges(edge_dict, cameras, edge_maps, detector, **options)
    os.makedirs(model_path, exist_ok=True)
    out = write_snap(model_path, res)
    print("snapped: ", out["moved"], "of", out["total"], "edges moved")
    return res["edge_dict"], res


def support_scene(model_path, edge_dict, cameras, edge_maps, detector, input_file=None, **options):
    """The export's ``support_checking``: ``edge_dict`` against the given cameras (``NovelViewCamera`` s and uint8 maps, or a
    Scene's ``EdgeCamera`` s when ``edge_maps`` is None: ``reprojection.scene_cameras``).  Writes ``edge_support.json`` and
    ``parametric_edges_supported.json`` into ``model_path``, prints the counts before and after, and returns
    (the filtered dict, the ``edge_support`` result).  ``input_file``: when the edges did not come from
    ``parametric_edges.json``, the file they came from, recorded as "input"."""
    if edge_maps is None:
        cameras, edge_maps = scene_cameras(cameras)
    res = SP.edge_support(edge_dict, cameras, edge_maps, detector, **options)
    os.makedirs(model_path, exist_ok=True)
    out = write_support(model_path, edge_dict, res, write_filtered=True, extra={"input": input_file} if input_file else None)
    print("before support checking: ", out["total"], "after support checking: ", out["kept"])
    return filter_edge_dict(edge_dict, res["kept"]), res


def trim_scene(model_path, edge_dict, cameras, edge_maps, detector, input_file=None, **options):
    """The export's ``trim``: every edge of ``edge_dict`` cut down to its supported spans in the given cameras (as
    ``support_scene`` takes them).  Writes ``edge_trim.json`` and ``parametric_edges_trimmed.json`` into ``model_path``, prints
    the counts before and after, and returns (the trimmed dict, the ``trim_edges`` result).  ``input_file`` as
    ``support_scene`` takes it."""
    if edge_maps is None:
        cameras, edge_maps = scene_cameras(cameras)
    res = ET.trim_edges(edge_dict, cameras, edge_maps, detector, **options)
    os.makedirs(model_path, exist_ok=True)
    out = write_trim(model_path, edge_dict, res, extra={"input": input_file} if input_file else None)
    print("before trimming: ", out["total"], "edges, after trimming: ", out["pieces"], "pieces")
    return res["edge_dict"], res


def dedupe_scene(model_path, edge_dict, input_file="parametric_edges.json", **options):
    """The export's ``dedupe``: every edge of ``edge_dict`` cut down to what no longer edge covers (``dedupe_edges``; no
    cameras: this is 3D only).  ``input_file``: the file the edges came from, recorded as "input".  Writes
    ``edge_dedupe.json`` and ``parametric_edges_deduped.json`` into ``model_path``, prints the counts before and after, and
    returns (the deduped dict, the ``dedupe_edges`` result)."""
    res = ED.dedupe_edges(edge_dict, **options)
    os.makedirs(model_path, exist_ok=True)
    out = write_dedupe(model_path, edge_dict, res, extra={"input": input_file})
    print("before deduping: ", out["total"], "edges, after deduping: ", out["pieces"], "pieces")
    return res["edge_dict"], res


def join_scene(model_path, edge_dict, input_file="parametric_edges.json", **options):
    """The export's ``join``: the edges of ``edge_dict`` rejoined at their junctions (``join_edges``; no cameras: this is 3D
    only).  ``input_file``: the file the edges came from, recorded as "input".  Writes ``edge_graph.json`` and
    ``parametric_edges_joined.json`` into ``model_path``, prints the counts, and returns (the joined dict, the ``join_edges``
    result)."""
    res = EJ.join_edges(edge_dict, **options)
    os.makedirs(model_path, exist_ok=True)
    out = write_join(model_path, edge_dict, res, extra={"input": input_file})
    print("joined: ", out["counts"]["edges"], "edges, ", out["counts"]["vertices"], "vertices, ", out["counts"]["t_junctions"],
          "T-junctions, ", out["counts"]["moved_ends"], "ends moved")
    return res["edge_dict"], res


# ------------------------------------------------------------------------------------------------ command line
def scan_line(scan, out):
    line = f"{scan}: views {out['settings']['views']}, edges {out['total']}, kept {out['kept']}"
    if "snap" in out:
        line += f"; snapped {out['snap']['moved']} of {out['snap']['total']} edges first"
    if "trim" in out:
        line += f"; trimmed to {out['trim']['pieces']} pieces, {out['trim']['kept_samples']} of {out['trim']['samples']} samples"
    if "dedupe" in out:
        line += (f"; deduped to {out['dedupe']['pieces']} pieces, {out['dedupe']['redundant_samples']} of "
                 f"{out['dedupe']['samples']} samples redundant")
    if "join" in out:
        counts = out["join"]["counts"]
        line += (f"; joined {counts['edges']} edges at {counts['vertices']} vertices, {counts['t_junctions']} T-junctions, "
                 f"{counts['moved_ends']} ends moved")
    return line


def parser():
    ap = argparse.ArgumentParser(description="Check every parametric edge along its length against a scan's edge maps.")
    ap.add_argument("--base_dir", default="./output", help="directory holding <scan>/parametric_edges.json")
    ap.add_argument("--dataset_dir", required=True, help="directory holding the scans")
    ap.add_argument("--scans", default=None, help="file with one scan name per line (default: every scan of --dataset_dir)")
    ap.add_argument("--layout", choices=LAYOUTS, default="emap")
    ap.add_argument("--detector", default="DexiNed")
    ap.add_argument("--undistort", action="store_true", help="colmap layout: resample the edge maps through the lens model")
    ap.add_argument("--tolerances", nargs="+", type=float, default=list(SP.TOLERANCES_PX), help="pixel tolerances (1 to 4)")
    ap.add_argument("--keep_tolerance", type=float, default=SP.KEEP_TOLERANCE_PX, help="the tolerance that decides 'kept'")
    ap.add_argument("--min_visible", type=float, default=SP.MIN_VISIBLE,
                    help="share of an edge's samples a view must see (untuned)")
    ap.add_argument("--min_near", type=float, default=SP.MIN_NEAR,
                    help="share of the seen samples that must lie near a detected pixel (untuned)")
    ap.add_argument("--frames_ratio", type=float, default=EDGE_VISIBILITY_FRAMES_RATIO,
                    help="an edge is kept when more than ceil(ratio * views) views support it")
    ap.add_argument("--sample_resolution", type=float, default=SAMPLE_RESOLUTION)
    ap.add_argument("--edge_threshold", type=float, default=EDGE_MAX_THRESHOLD)
    ap.add_argument("--write_filtered", action="store_true", help=f"also write {FILTERED_FILE} with the kept edges")
    ap.add_argument("--backend", choices=SP.SUPPORT_BACKENDS, default="gpu")
    ap.add_argument("--thin", action="store_true", help="thin the detected masks first (a thick detector response; untuned)")
    ap.add_argument("--snap", action="store_true",
                    help=f"FIRST move every edge onto the detected edges: {SNAPPED_FILE} and {SNAP_FILE}; the check and every "
                         f"later step start from the snapped edges (untuned; no depth; not a filter)")
    ap.add_argument("--snap_capture", type=float, default=SN.CAPTURE_PX,
                    help="snapping: pixel distance to a detected edge within which a view pulls a sample, 1 to 8 (untuned)")
    ap.add_argument("--snap_iterations", type=int, default=SN.ITERATIONS, help="snapping: steps and refits (untuned)")
    ap.add_argument("--snap_min_constrained", type=float, default=SN.MIN_CONSTRAINED,
                    help="snapping: share of an edge's samples that must be constrained for it to take part (untuned)")
    ap.add_argument("--trim", action="store_true",
                    help=f"also cut EVERY edge down to its supported spans: {TRIMMED_FILE} and {TRIM_FILE} (untuned; no depth)")
    ap.add_argument("--trim_tolerance", type=float, default=ET.TOLERANCE_PX,
                    help="trimming: pixel distance to a detected edge within which a sample counts as near (untuned)")
    ap.add_argument("--trim_max_gap", type=int, default=ET.MAX_GAP,
                    help="trimming: two supported runs at most this many samples apart are merged (untuned)")
    ap.add_argument("--trim_min_span", type=int, default=ET.MIN_SPAN,
                    help="trimming: a supported run of fewer samples is dropped (untuned)")
    ap.add_argument("--oriented", action="store_true",
                    help="trimming (needs --trim): a sample counts as near only where a detected pixel within the tolerance runs "
                         "the way its edge does (ops.edge_orient; untuned; thick strokes fall back to the distance test)")
    ap.add_argument("--orient_spread", type=int, default=OR.SPREAD,
                    help=f"oriented trimming: the octants of 22.5 degrees to either side that still agree, 0 to "
                         f"{OR.MAX_SPREAD} (untuned)")
    ap.add_argument("--dedupe", action="store_true",
                    help=f"also drop what a longer edge already covers in 3D -- of the trimmed pieces with --trim, of the "
                         f"edges otherwise: {DEDUPED_FILE} and {DEDUPE_FILE} (untuned; the longer edge always wins)")
    ap.add_argument("--dedupe_tolerance", type=float, default=None,
                    help=f"deduping: 3D distance within which a sample of a longer edge covers one (default: "
                         f"{ED.TOLERANCE_RESOLUTIONS:g} x --sample_resolution; untuned)")
    ap.add_argument("--dedupe_cos_min", type=float, default=ED.COS_MIN,
                    help="deduping: least |cosine| between the two edges' directions for a cover (untuned)")
    ap.add_argument("--dedupe_min_run", type=int, default=ED.MIN_RUN,
                    help="deduping: a run of fewer covered samples is not redundant (untuned)")
    ap.add_argument("--dedupe_min_span", type=int, default=ED.MIN_SPAN,
                    help="deduping: a free run of fewer samples is dropped (untuned)")
    ap.add_argument("--join", action="store_true",
                    help=f"also rejoin the ends at their junctions in 3D -- of the deduped edges with --dedupe, else of the "
                         f"trimmed pieces with --trim, else of the edges: {JOINED_FILE} and {GRAPH_FILE} (untuned; hosts of "
                         f"T-junctions are not split, an end joins at most one thing)")
    ap.add_argument("--join_tolerance", type=float, default=None,
                    help=f"joining: 3D distance within which an end attaches in any direction, and the half width of the "
                         f"tube ahead of it (default: {EJ.TOLERANCE_RESOLUTIONS:g} x --sample_resolution; untuned)")
    ap.add_argument("--join_reach", type=float, default=None,
                    help=f"joining: how far ahead along its tangent an end looks (default: {EJ.REACH_RESOLUTIONS:g} x "
                         f"--sample_resolution; untuned)")
    add_depth_arguments(ap)   # --occluder / --depth_dir, --depth_slack, --depth_window: gate the check, --snap and --trim
    return ap


def main(argv=None):
    ap = parser()
    args = ap.parse_args(argv)
    if args.oriented and not args.trim:
        ap.error("--oriented needs --trim: it changes how trimming tallies")
    trim = {"tolerance_px": args.trim_tolerance, "max_gap": args.trim_max_gap, "min_span": args.trim_min_span,
            "frames_ratio": args.frames_ratio} if args.trim else None
    if args.oriented:
        trim.update({"oriented": True, "spread": args.orient_spread})
    dedupe = {"tolerance": args.dedupe_tolerance, "cos_min": args.dedupe_cos_min, "min_run": args.dedupe_min_run,
              "min_span": args.dedupe_min_span} if args.dedupe else None
    join = {"tolerance": args.join_tolerance, "reach": args.join_reach} if args.join else None
    snap = {"capture_px": args.snap_capture, "iterations": args.snap_iterations, "min_constrained": args.snap_min_constrained,
            "frames_ratio": args.frames_ratio} if args.snap else None
    for scan in dataset_scans(args.dataset_dir, args.layout, args.scans):
        out = score_scan(args.base_dir, args.dataset_dir, scan, args.layout, args.detector, args.undistort,
                         args.write_filtered, backend=args.backend, tolerances_px=args.tolerances,
                         keep_tolerance_px=args.keep_tolerance, min_visible=args.min_visible, min_near=args.min_near,
                         frames_ratio=args.frames_ratio, sample_resolution=args.sample_resolution,
                         edge_threshold=args.edge_threshold, trim_options=trim, dedupe_options=dedupe,
                         join_options=join, **({"snap_options": snap} if snap is not None else {}),
                         **({"thin": True} if args.thin else {}),
                         **({"occluder": args.occluder, "depth_dir": args.depth_dir, "depth_slack": args.depth_slack,
                             "depth_window": args.depth_window}
                            if args.occluder is not None or args.depth_dir is not None else {}),
                         **({"near_clip": args.near_clip} if args.near_clip is not None else {}))
        if out is None:
            print(f"Invalid prediction at {scan}")
            continue
        print(scan_line(scan, out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
