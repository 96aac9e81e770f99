"""python -m curve_gaussian_amd.edge_extraction.visibility --edges <parametric_edges.json> --scan_dir <scan>
--detector {DexiNed,PidiNet} --out <dir>: filters an existing parametric_edges.json by the edge-map visibility check
(get_parametric_edge(visible_checking=True), the check on the GPU) and writes the kept edges' parametric_edges.json
and edge_points.ply to <dir>.  With --occluder FILE or --depth_dir DIR (inside --scan_dir; --depth_slack, --depth_window,
--near_clip as the score takes them) the check is depth-gated: a control or end point hidden behind the depth planes is
dropped before its frame's cell is formed (opt-in, UNTUNED, checked on drawn solids only)."""
import argparse
import json
import os
import sys

from ..scene.dataset_io import write_edge_files
from .para_edge import get_parametric_edge


def scan_gate_options(scan_dir, detector, occluder=None, depth_dir=None, depth_slack=None, depth_window=None,
                      near_clip=None):
    """The depth keywords of ``get_parametric_edge`` for a scan: ``occluder`` names a mesh file inside ``scan_dir``,
    ``depth_dir`` a directory inside it with one ``<image stem>.npy`` per frame (``reprojection.scan_depth_maps``, in the
    frames' order); {} with neither.  ``depth_slack`` / ``depth_window`` None keep the defaults."""
    if occluder is None and depth_dir is None:
        if near_clip is not None:
            raise ValueError("near_clip needs an occluder (depth maps need no clipping)")
        return {}
    if occluder is not None and depth_dir is not None:
        raise ValueError("give an occluder or a depth_dir, not both")
    gate = {k: v for k, v in (("depth_slack", depth_slack), ("depth_window", depth_window), ("near_clip", near_clip))
            if v is not None}
    if occluder is not None:
        gate["occluder"] = os.path.join(scan_dir, occluder)
    else:
        from .reprojection import emap_cameras, scan_depth_maps
        gate["depth_maps"] = scan_depth_maps(os.path.join(scan_dir, depth_dir), emap_cameras(scan_dir, detector)[0])
    return gate


def main(argv=None):
    ap = argparse.ArgumentParser(description="Keep the parametric edges the 2D edge maps of a scan show.")
    ap.add_argument("--edges", required=True, help="parametric_edges.json to filter")
    ap.add_argument("--scan_dir", required=True, help="scan directory holding meta_data.json and the edge maps")
    ap.add_argument("--detector", required=True, choices=["DexiNed", "PidiNet"], help="which edge maps to read")
    ap.add_argument("--out", required=True, help="output directory for parametric_edges.json and edge_points.ply")
    from .reprojection import add_gate_arguments, check_gate_arguments
    add_gate_arguments(ap)
    args = ap.parse_args(argv)
    check_gate_arguments(ap, args)
    with open(args.edges, encoding="UTF-8") as f:
        edge_dict = json.load(f)
    pts, kept = get_parametric_edge(True, edge_dict, args.scan_dir, args.detector,
                                    **scan_gate_options(args.scan_dir, args.detector, args.occluder, args.depth_dir,
                                                        args.depth_slack, args.depth_window, args.near_clip))
    write_edge_files(args.out, kept, pts)
    return 0


if __name__ == "__main__":
    sys.exit(main())
