"""Edge evaluation: the project's counterpart of the reference's ``edge_extraction`` evaluator (eval_ABC.py,
eval_utils.py, merging.py).  Every nearest-neighbour query runs in the HIP kernel ``cgs_nn1`` (exact, brute force,
lowest index on ties); there is no CPU path for it -- CPU tensors raise.  The loaders are host-side numpy."""
from .abc import (PredEdges, abc_gt_points, evaluate_abc, evaluate_abc_scan, finalize_metrics, pred_points_and_directions,
                  scan_metrics, summary_lines)
from .ops import (THRESHOLDS, chamfer_distance, chamfer_from_distances, direction_similarity,
                  downsample_point_cloud_average, merge_endpoints, nearest_neighbors, precision_recall_from_distances,
                  precision_recall_iou, similarity_from_index)

__all__ = ["PredEdges", "THRESHOLDS", "abc_gt_points", "chamfer_distance", "chamfer_from_distances",
           "direction_similarity", "downsample_point_cloud_average", "evaluate_abc", "evaluate_abc_scan",
           "finalize_metrics", "merge_endpoints", "nearest_neighbors", "precision_recall_from_distances",
           "precision_recall_iou", "pred_points_and_directions", "scan_metrics", "similarity_from_index",
           "summary_lines"]
