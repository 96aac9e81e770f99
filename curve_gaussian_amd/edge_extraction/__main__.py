"""python -m curve_gaussian_amd.edge_extraction --base_dir <predictions> --dataset_dir <ABC data dir>: the reference's
eval_ABC.py summary (eval_ABC.py:333-363), on the GPU."""
import argparse
import logging
import sys

from .abc import evaluate_abc, summary_lines


def main(argv=None):
    ap = argparse.ArgumentParser(description="Evaluate parametric edges against ABC ground truth.")
    ap.add_argument("--base_dir", default="./output", help="directory holding <scan>/parametric_edges.json")
    ap.add_argument("--dataset_dir", required=True, help="ABC data directory (its sibling 'groundtruth' holds the GT)")
    args = ap.parse_args(argv)
    logging.basicConfig(level=logging.INFO, format="%(message)s", stream=sys.stdout)
    metrics, totals = evaluate_abc(args.base_dir, args.dataset_dir)
    for line in summary_lines(metrics, totals):
        print(line)
    return 0


if __name__ == "__main__":
    sys.exit(main())
