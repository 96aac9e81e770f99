"""python -m curve_gaussian_amd.edge_extraction --base_dir <predictions> --dataset_dir <ABC data dir>: the reference's
eval_ABC.py summary (eval_ABC.py:333-363), on the GPU.  With --render_mv, the multi-view projection of the predicted
edges instead (eval_ABC.py:180-185): <base_dir>/<scan>/novel_view/<frame>.png for every camera of transforms_video.json.
With --render_mv and --occluder FILE or --depth_dir DIR (inside each scan of --dataset_dir) the samples hidden behind the
depth planes are not drawn and the images go to <base_dir>/<scan>/novel_view_visible/ (opt-in, UNTUNED, drawn solids only)."""
import argparse
import logging
import sys

from .abc import evaluate_abc, summary_lines


def parser():
    ap = argparse.ArgumentParser(description="Evaluate parametric edges against ABC ground truth.")
    ap.add_argument("--base_dir", default="./output", help="directory holding <scan>/parametric_edges.json")
    ap.add_argument("--dataset_dir", required=True, help="ABC data directory (its sibling 'groundtruth' holds the GT)")
    ap.add_argument("--render_mv", action="store_true",
                    help="draw the predicted edges into every transforms_video.json camera instead of evaluating")
    from .reprojection import add_gate_arguments
    add_gate_arguments(ap)   # for --render_mv
    return ap


def main(argv=None):
    ap = parser()
    args = ap.parse_args(argv)
    from .reprojection import check_gate_arguments, gate_arguments
    check_gate_arguments(ap, args)
    if not args.render_mv and gate_arguments(args):
        ap.error("--occluder / --depth_dir gate the drawn views: they need --render_mv")
    logging.basicConfig(level=logging.INFO, format="%(message)s", stream=sys.stdout)
    if args.render_mv:
        from .novel_view import render_abc_novel_views
        render_abc_novel_views(args.base_dir, args.dataset_dir, **gate_arguments(args))
        return 0
    metrics, totals = evaluate_abc(args.base_dir, args.dataset_dir)
    for line in summary_lines(metrics, totals):
        print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
