"""python -m curve_gaussian_amd.edge_extraction --base_dir <predictions> --dataset_dir <ABC data dir>: the reference's
eval_ABC.py summary (eval_ABC.py:333-363), on the GPU.  With --render_mv, the multi-view projection of the predicted
edges instead (eval_ABC.py:180-185): <base_dir>/<scan>/novel_view/<frame>.png for every camera of transforms_video.json."""
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
    return ap


def main(argv=None):
    args = parser().parse_args(argv)
    logging.basicConfig(level=logging.INFO, format="%(message)s", stream=sys.stdout)
    if args.render_mv:
        from .novel_view import render_abc_novel_views
        render_abc_novel_views(args.base_dir, args.dataset_dir)
        return 0
    metrics, totals = evaluate_abc(args.base_dir, args.dataset_dir)
    for line in summary_lines(metrics, totals):
        print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
