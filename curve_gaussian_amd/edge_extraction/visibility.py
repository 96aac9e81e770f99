"""python -m curve_gaussian_amd.edge_extraction.visibility --edges <parametric_edges.json> --scan_dir <scan>
--detector {DexiNed,PidiNet} --out <dir>: filters an existing parametric_edges.json by the edge-map visibility check
(get_parametric_edge(visible_checking=True), the check on the GPU) and writes the kept edges' parametric_edges.json
and edge_points.ply to <dir>."""
import argparse
import json
import sys

from ..scene.dataset_io import write_edge_files
from .para_edge import get_parametric_edge


def main(argv=None):
    ap = argparse.ArgumentParser(description="Keep the parametric edges the 2D edge maps of a scan show.")
    ap.add_argument("--edges", required=True, help="parametric_edges.json to filter")
    ap.add_argument("--scan_dir", required=True, help="scan directory holding meta_data.json and the edge maps")
    ap.add_argument("--detector", required=True, choices=["DexiNed", "PidiNet"], help="which edge maps to read")
    ap.add_argument("--out", required=True, help="output directory for parametric_edges.json and edge_points.ply")
    args = ap.parse_args(argv)
    with open(args.edges, encoding="UTF-8") as f:
        edge_dict = json.load(f)
    pts, kept = get_parametric_edge(True, edge_dict, args.scan_dir, args.detector)
    write_edge_files(args.out, kept, pts)
    return 0


if __name__ == "__main__":
    sys.exit(main())
