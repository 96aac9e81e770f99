"""Edge evaluation: the project's counterpart of the reference's ``edge_extraction`` evaluator (eval_ABC.py,
eval_utils.py, merging.py).  Every nearest-neighbour query runs in the HIP kernel ``cgs_nn1`` (exact, brute force,
lowest index on ties); there is no CPU path for it -- CPU tensors raise.  The loaders are host-side numpy.

The extraction step's edge-map visibility check (extract_para_edge.py: get_edge_maps, compute_visibility,
get_parametric_edge) lives in ``para_edge``; its per-(edge, frame) work runs in the HIP kernel ``cgs_edge_visibility``.

The multi-view projection of the predicted edges (eval_ABC.py --render_mv, eval_replica.py) lives in ``novel_view``; its
per-(point, view) work runs in the HIP kernels ``cgs_project_points`` / ``cgs_render_points``.

Both take the depth gate of the 2D operators, opt-in (``ops.edge_occlusion``): ``get_parametric_edge`` with
``occluder`` / ``depth_maps`` (``cgs_edge_visibility_depth``) and ``project_points_depth`` / ``render_points_depth``
(``cgs_project_points_depth`` / ``cgs_render_points_depth``).  UNTUNED, checked on drawn solids only."""
from .abc import (PredEdges, abc_gt_points, evaluate_abc, evaluate_abc_scan, finalize_metrics, pred_points_and_directions,
                  scan_metrics, summary_lines)
from .ops import (THRESHOLDS, chamfer_distance, chamfer_from_distances, direction_similarity,
                  downsample_point_cloud_average, merge_endpoints, nearest_neighbors, precision_recall_from_distances,
                  precision_recall_iou, similarity_from_index)
from .novel_view import (NovelViewCamera, colmap_cameras, edge_point_colors, fancy_colors, project_points,
                         project_points_depth, render_abc_novel_views, render_points, render_points_depth,
                         render_replica_novel_views, transforms_video_cameras)
from .para_edge import (EDGE_MAX_THRESHOLD, EDGE_VISIBILITY_FRAMES_RATIO, EDGE_VISIBILITY_THRESHOLD, compute_visibility,
                        compute_visibility_depth, edge_visibility_counts, edge_visibility_counts_depth,
                        edge_visibility_frames, get_edge_maps, get_parametric_edge)

__all__ = ["EDGE_MAX_THRESHOLD", "EDGE_VISIBILITY_FRAMES_RATIO", "EDGE_VISIBILITY_THRESHOLD", "NovelViewCamera", "PredEdges",
           "THRESHOLDS", "abc_gt_points", "chamfer_distance", "chamfer_from_distances", "colmap_cameras", "compute_visibility",
           "compute_visibility_depth",
           "direction_similarity", "downsample_point_cloud_average", "edge_point_colors", "edge_visibility_counts", "edge_visibility_counts_depth",
           "edge_visibility_frames", "evaluate_abc", "evaluate_abc_scan", "fancy_colors", "finalize_metrics", "get_edge_maps",
           "get_parametric_edge", "merge_endpoints", "nearest_neighbors", "precision_recall_from_distances",
           "precision_recall_iou", "pred_points_and_directions", "project_points", "project_points_depth", "render_abc_novel_views", "render_points",
           "render_points_depth",
           "render_replica_novel_views", "scan_metrics", "similarity_from_index", "summary_lines",
           "transforms_video_cameras"]
