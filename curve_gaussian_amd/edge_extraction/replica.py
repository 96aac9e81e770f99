"""python -m curve_gaussian_amd.edge_extraction.replica --base_dir <predictions> --dataset_dir <Replica_Edge dir>
[--scans FILE]: the reference's eval_replica.py (process_scan :100-212, main :216-258) on the GPU -- the predicted edges
of every scan drawn into every COLMAP camera, <base_dir>/<scan>/novel_view/<image name>.  Without --scans, every scan
directory of --dataset_dir that holds sparse/0.  With --occluder FILE or --depth_dir DIR (inside each scan of --dataset_dir)
the samples hidden behind the depth planes are not drawn and the images go to <base_dir>/<scan>/novel_view_visible/ (opt-in,
UNTUNED, drawn solids only)."""
import argparse
import sys

from .novel_view import render_replica_novel_views, replica_scans


def parser():
    ap = argparse.ArgumentParser(description="Project predicted edges into every camera of Replica scans.")
    ap.add_argument("--base_dir", default="./output/replica/", help="directory holding <scan>/parametric_edges.json")
    ap.add_argument("--dataset_dir", required=True, help="Replica_Edge directory holding <scan>/sparse/0")
    ap.add_argument("--scans", default=None, help="file with one scan name per line (default: every scan with sparse/0)")
    from .reprojection import add_gate_arguments
    add_gate_arguments(ap)
    return ap


def main(argv=None):
    ap = parser()
    args = ap.parse_args(argv)
    from .reprojection import check_gate_arguments, gate_arguments
    check_gate_arguments(ap, args)
    render_replica_novel_views(args.base_dir, args.dataset_dir, replica_scans(args.dataset_dir, args.scans),
                               **gate_arguments(args))
    return 0


if __name__ == "__main__":
    sys.exit(main())
