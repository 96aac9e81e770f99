"""ctypes binding of libcurvegs.so (C ABI declared in include/curvegs.h).

The product path has NO fallback: if the HIP library is missing or no GPU is present, calls raise.
``load()`` only dlopens the library (works on a CPU-only box, used by the "symbols exported" tests).
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CGS_LIB", os.path.join(_HERE, "libcurvegs.so"))  # CGS_LIB: A/B experiment builds

ALLOC_FN = C.CFUNCTYPE(C.c_void_p, C.c_void_p, C.c_size_t)
_vp, _i, _f, _i64 = C.c_void_p, C.c_int, C.c_float, C.c_int64

# name -> (restype, argtypes); kept in lock-step with include/curvegs.h (tests/test_abi.py parses the header)
SIGNATURES = {
    "cgs_last_error": (C.c_char_p, []),
    "cgs_version": (_i, []),
    "cgs_target_arch": (C.c_char_p, []),
    "cgs_geometry_bytes": (C.c_size_t, [_i]),
    "cgs_image_bytes": (C.c_size_t, [_i, _i]),
    "cgs_binning_bytes": (C.c_size_t, [_i64]),
    "cgs_rasterize_forward_static": (_i, [_vp, _vp, C.c_size_t, _vp, C.c_uint32, _i, _i, _i, _vp, _i, _i,
                                          _vp, _vp, _vp, _vp, _vp, _f, _vp, _vp, _vp, _vp, _vp, _vp, _f, _f,
                                          _vp, _vp, _vp, _i, _i, _vp, _vp]),
    "cgs_view_forward": (_i, [_i, _i, _vp, _vp, _vp, _vp, _f, _vp, _vp, _vp, _f, _vp, _vp, _vp, C.c_size_t, _vp, C.c_uint32,
                              _vp, _i, _i, _vp, _vp, _vp, _f, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "cgs_view_forward_checked": (_i64, [_i, _i, _vp, _vp, _vp, _vp, _f, _vp, _vp, _vp, _f, _vp, _vp, _vp, C.c_size_t, _vp,
                                        C.c_uint32, _vp, _i, _i, _vp, _vp, _vp, _f, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "cgs_view_forward_begin": (_i, [_i, _i, _vp, _vp, _vp, _vp, _f, _vp, _vp, _vp, _f, _vp, _vp, _vp, C.c_size_t, _vp,
                                    C.c_uint32, _vp, _i, _i, _vp, _vp, _vp, _f, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "cgs_view_forward_shared": (_i, [_i, _i, _vp, _vp, _vp, _vp, _f, _vp, _vp, _vp, _f, _vp, _vp, _vp, C.c_size_t, _vp,
                                     C.c_uint32, _vp, _i, _i, _vp, _vp, _vp, _f, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "cgs_view_forward_render": (_i, [_i, _i, _i, _vp, _vp, _vp, _vp, _f, _vp, _vp, _vp, _f, _vp, _vp, C.c_size_t, _vp, C.c_uint32,
                                     _vp, _i, _i, _vp, _vp, _vp, _f, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    # the siblings' arguments with the cgs_view_gate pointer before the stream
    "cgs_view_forward_depth": (_i, [_i, _i, _vp, _vp, _vp, _vp, _f, _vp, _vp, _vp, _f, _vp, _vp, _vp, C.c_size_t, _vp, C.c_uint32,
                                    _vp, _i, _i, _vp, _vp, _vp, _f, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "cgs_view_forward_render_depth": (_i, [_i, _i, _i, _vp, _vp, _vp, _vp, _f, _vp, _vp, _vp, _f, _vp, _vp, C.c_size_t, _vp,
                                           C.c_uint32, _vp, _i, _i, _vp, _vp, _vp, _f, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "cgs_view_backward_render": (_i, [_i, _i, _vp, _vp, _vp, _vp, _f, _vp, _vp, _vp, _f, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp,
                                      _f, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp]),
    "cgs_view_forward_wait": (_i64, [_i, C.POINTER(_i64)]),
    "cgs_view_forward_abandon": (None, [_i]),
    "cgs_render_epilogue": (_i, [_i, _i, _vp, _vp, _vp, _i, _vp, _vp, _vp]),
    "cgs_clamp_backward": (_i, [_i64, _vp, _vp, _vp, _vp]),
    "cgs_bucket_capacity_hint": (C.c_uint32, [_i, _i, _i]),
    "cgs_last_forward_visible": (_i64, []),
    "cgs_visible_indices": (_i, [_i, _vp, _vp, _i, _i, _vp, _vp]),
    "cgs_view_shared_begin": (_i, [_i, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "cgs_view_shared_end": (_i, [_i, _i, _vp, _vp, _vp, _vp, _f, _vp, _vp, _vp, _vp, _i, _vp]),
    "cgs_view_backward_scratch_floats": (C.c_size_t, [_i, _i]),
    "cgs_view_norms_backward_range": (_i, [C.POINTER(_i), C.POINTER(_i)]),
    "cgs_view_backward": (_i, [_i, _i, _vp, _vp, _vp, _vp, _f, _vp, _vp, _vp, _f, _vp, _vp, _vp, _vp, _vp, _i, _i, _vp, _vp, _vp,
                               _f, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _vp]),
    "cgs_image_status_offset": (C.c_size_t, [_i, _i]),
    "cgs_status_words": (_i, []),
    "cgs_bucket_capacity_limit": (C.c_uint32, []),
    "cgs_adam_step_flat_dev": (_i, [_i64, _vp, _vp, _vp, _vp, _vp, _i, _f, _f, _f, _i, _vp, _vp]),
    "cgs_adam_step_flat_dev_report": (_i, [_i64, _vp, _vp, _vp, _vp, _vp, _i, _f, _f, _f, _i, _vp, _vp, _vp, _i, _vp]),
    "cgs_adam_state_bytes": (C.c_size_t, []),
    "cgs_reset_binning_hints": (None, []),
    "cgs_last_forward_stats": (None, [C.POINTER(_i64), C.POINTER(_i64), C.POINTER(_i)]),
    "cgs_prof_enable": (None, [_i]),
    "cgs_prof_reset": (None, []),
    "cgs_prof_collect": (_i, [C.POINTER(C.c_char_p), C.POINTER(C.c_double), C.POINTER(_i64), _i]),
    "cgs_rasterize_forward": (_i64, [ALLOC_FN, _vp, ALLOC_FN, _vp, ALLOC_FN, _vp, _i, _i, _i, _vp, _i, _i,
                                     _vp, _vp, _vp, _vp, _vp, _f, _vp, _vp, _vp, _vp, _vp, _vp, _f, _f, _i,
                                     _vp, _vp, _vp, _i, _i, _vp, _i, _vp]),
    "cgs_rasterize_backward": (_i, [_i, _i, _i, _i64, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _vp, _f, _vp, _vp, _vp,
                                    _vp, _vp, _f, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                    _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _i, _vp]),
    "cgs_mark_visible": (_i, [_i, _vp, _vp, _vp, _vp, _vp]),
    "cgs_ssim_forward": (_i, [_i, _i, _i, _i, _f, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "cgs_ssim_backward": (_i, [_i, _i, _i, _i, _f, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "cgs_edge_aware_loss": (_i, [_i, _i, _i, _vp, _vp, _f, _vp, _vp, _vp]),
    "cgs_photometric_workspace_bytes": (C.c_size_t, [_i, _i]),
    "cgs_edge_count": (_i, [_i, _i, _i, _vp, _f, _vp, _vp]),
    "cgs_photometric_loss": (_i, [_i, _i, _vp, _vp, _f, _vp, _f, _f, _i, _vp, _vp, _vp, _vp]),
    "cgs_endpoint_connection_workspace_bytes": (C.c_size_t, [_i]),
    "cgs_endpoint_connection_loss": (_i, [_i, _vp, _f, _f, _vp, _vp, _vp, _i, _vp]),
    "cgs_photometric_loss_indexed": (_i, [_i, _i, _vp, _vp, _vp, _f, _vp, _f, _f, _i, _vp, _vp, _vp, _vp]),
    "cgs_curve_regularizers_workspace_bytes": (C.c_size_t, []),
    "cgs_curve_regularizers": (_i, [_i, _i, _vp, _vp, _vp, _vp, _f, _vp, _f, _f, _f, _vp, _vp, _vp, _vp, _vp, _vp]),
    "cgs_adam_step_flat": (_i, [_i64, _vp, _vp, _vp, _vp, C.c_char_p, _i, _f, _f, _f, _i, _i, _vp]),
    "cgs_knn_workspace_bytes": (C.c_size_t, [_i]),
    "cgs_knn_mean_dist2": (_i, [_i, _vp, _vp, _vp, _vp]),
    "cgs_nn1_workspace_bytes": (C.c_size_t, [_i]),
    "cgs_nn1": (_i, [_i, _vp, _i, _vp, _vp, _vp, _vp, _vp]),
    "cgs_edge_visibility": (_i, [_i, _vp, _i, _vp, _i, _vp, _vp, _i, _i, _vp, _i, _vp, _vp]),
    "cgs_view_metrics_workspace_bytes": (C.c_size_t, [_i]),
    "cgs_view_metrics": (_i, [_i, _vp, _vp, _vp, _vp, _vp]),
    "cgs_report_panels_workspace_bytes": (C.c_size_t, [_i]),
    "cgs_report_panels": (_i, [_i, _vp, _vp, _vp, _vp]),
    "cgs_densification_stats": (_i, [_i64, _vp, _vp, _i64, _vp, _vp, _vp, _vp, _vp]),
    "cgs_project_points": (_i, [_i, _vp, _i, _vp, _vp, _i, _i, _vp, _vp]),
    "cgs_render_points_workspace_bytes": (C.c_size_t, [_i, _i, _i, _i]),
    "cgs_render_points": (_i, [_i, _vp, _vp, _i, _vp, _vp, _i, _i, C.c_double, _vp, _vp, _vp, _vp, C.c_size_t, _vp]),
    "cgs_ellipsoid_mesh_body_bytes": (_i64, [_i, _i, C.POINTER(_i64), C.POINTER(_i64)]),
    "cgs_ellipsoid_mesh_vertices": (_i, [_i, _i, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp]),
    "cgs_ellipsoid_mesh_faces": (_i, [_i, _i, _i, _i, _vp, _vp, _vp]),
    "cgs_curve_straightness": (_i, [_i, _vp, _vp, _i, C.c_double, C.c_double, _vp, _vp, _vp, _vp]),
    "cgs_segment_merge_workspace_bytes": (C.c_size_t, [_i]),
    "cgs_segment_merge_labels": (_i, [_i, _vp, C.c_double, C.c_double, _vp, _vp, _vp, _vp]),
    "cgs_pair_consensus_fit": (_i, [_i, _vp, _i, _vp, _i, C.c_double, C.c_double, _vp, _vp, _vp, _vp, _vp]),
    "cgs_sample_curves_forward": (_i, [_i, _i, _vp, _vp, _vp, _vp, _f, _vp, _vp, _vp, _vp, _vp]),
    "cgs_sample_curves_backward": (_i, [_i, _i, _vp, _vp, _vp, _vp, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "cgs_splat_attrs_forward": (_i, [_i, _i, _vp, _vp, _vp, _vp, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "cgs_splat_attrs_backward": (_i, [_i, _i, _vp, _vp, _vp, _vp, _f, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                      _vp, _vp, _vp]),
    "cgs_undistort_images": (_i, [_i, _vp, _f, _vp, _vp]),
    "cgs_edge_gradients": (_i, [_i, _vp, _vp, _i, _vp]),
    "cgs_edge_trace": (_i, [_i, _vp, _f, _f, _i, _vp, _vp]),
    "cgs_point_mask": (_i, [_i, _vp, _i, _vp, _vp, _i, _i, _vp, _vp, _vp]),
    "cgs_edt_workspace_bytes": (C.c_size_t, [_i, _i, _i]),
    "cgs_edt_squared": (_i, [_i, _i, _i, _vp, _vp, _vp, _vp]),
    "cgs_edge_score_workspace_bytes": (C.c_size_t, [_i]),
    "cgs_edge_score_reduce": (_i, [_i, _i, _i, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp]),
    "cgs_pack_near_bits": (_i, [_i, _i, _i, _vp, _i, _vp, _vp]),
    "cgs_voxel_votes": (_i, [_i, _i, _i, _vp, _vp, _i, _vp, _vp, _i, _i, _vp, _i, _vp, _vp, _vp]),
    "cgs_voxel_moments": (_i, [_i, _i, _i, _vp, _i, _vp, _i, _vp, _vp]),
    "cgs_ray_claims": (_i, [_i, _i, _i, _vp, _vp, _i, _vp, _vp, _i, _vp, _vp, _i, _i, _vp, _i, _vp, _vp]),
    "cgs_ray_wins": (_i, [_i, _i, _i, _vp, _vp, _i, _vp, _vp, _i, _vp, _vp, _i, _i, _vp, _vp, _i, _i, _i, _vp, _vp]),
    "cgs_edge_support": (_i, [_i, _i, _vp, _vp, _i, _vp, _vp, _i, _i, _vp, _i, _vp, _vp, _vp]),
    "cgs_sample_support": (_i, [_i, _vp, _i, _vp, _vp, _i, _i, _vp, _i, _vp, _vp, _vp]),
    "cgs_thin_masks": (_i, [_i, _i, _i, _vp, _vp, _vp, _i, C.POINTER(_i), _vp]),
    "cgs_sample_cover_workspace_bytes": (C.c_size_t, [_i]),
    "cgs_sample_cover": (_i, [_i, _vp, _i, _vp, _vp, _f, _f, _vp, _vp, _vp]),
    "cgs_end_attach_workspace_bytes": (C.c_size_t, [_i, _i]),
    "cgs_end_attach": (_i, [_i, _vp, _i, _vp, _f, _f, _vp, _vp, _vp]),
    "cgs_mask_orientation": (_i, [_i, _i, _i, _vp, _vp, _vp]),
    "cgs_oriented_near": (_i, [_i, _i, _i, _vp, _i, _vp, _vp]),
    "cgs_sample_support_oriented": (_i, [_i, _vp, _vp, _i, _vp, _vp, _i, _i, _vp, _i, _vp, _vp]),
    "cgs_sample_snap_terms": (_i, [_i, _vp, _i, _vp, _vp, _i, _i, _vp, _i, _vp, _vp, _vp, _vp]),
    "cgs_mesh_depth": (_i, [_i, _vp, _i, _vp, _vp, _i, _i, _vp, _vp]),
    "cgs_depth_window_max": (_i, [_i, _i, _i, _i, _vp, _vp, _vp]),
    # the siblings' arguments up to their outputs, then depth, slack, the outputs (the gate's own counter last), stream
    "cgs_edge_visibility_depth": (_i, [_i, _vp, _i, _vp, _i, _vp, _vp, _i, _i, _vp, _i, _vp, C.c_double, _vp, _vp]),
    "cgs_project_points_depth": (_i, [_i, _vp, _i, _vp, _vp, _i, _i, _vp, C.c_double, _vp, _vp, _vp]),
    "cgs_render_points_depth": (_i, [_i, _vp, _vp, _i, _vp, _vp, _i, _i, _vp, C.c_double, C.c_double, _vp, _vp, _vp, _vp, _vp,
                                     C.c_size_t, _vp]),
    "cgs_point_mask_depth": (_i, [_i, _vp, _i, _vp, _vp, _i, _i, _vp, C.c_double, _vp, _vp, _vp, _vp]),
    # the siblings' arguments up to their outputs, then depth, slack, the outputs, hidden, stream
    "cgs_edge_support_depth": (_i, [_i, _i, _vp, _vp, _i, _vp, _vp, _i, _i, _vp, _i, _vp, _vp, C.c_double, _vp, _vp, _vp]),
    "cgs_sample_support_depth": (_i, [_i, _vp, _i, _vp, _vp, _i, _i, _vp, _i, _vp, _vp, C.c_double, _vp, _vp, _vp]),
    "cgs_sample_support_oriented_depth": (_i, [_i, _vp, _vp, _i, _vp, _vp, _i, _i, _vp, _i, _vp, C.c_double, _vp, _vp, _vp]),
    "cgs_sample_snap_terms_depth": (_i, [_i, _vp, _i, _vp, _vp, _i, _i, _vp, _i, _vp, _vp, C.c_double, _vp, _vp, _vp, _vp]),
    # the seed siblings' arguments, with depth and slack after the last per-view input (bits; best for the wins) and the
    # vote's hidden after hit
    "cgs_voxel_votes_depth": (_i, [_i, _i, _i, _vp, _vp, _i, _vp, _vp, _i, _i, _vp, _vp, C.c_double, _i, _vp, _vp, _vp, _vp]),
    "cgs_ray_claims_depth": (_i, [_i, _i, _i, _vp, _vp, _i, _vp, _vp, _i, _vp, _vp, _i, _i, _vp, _vp, C.c_double, _i, _vp,
                                  _vp]),
    "cgs_ray_wins_depth": (_i, [_i, _i, _i, _vp, _vp, _i, _vp, _vp, _i, _vp, _vp, _i, _i, _vp, _vp, _vp, C.c_double, _i, _i,
                                _i, _vp, _vp]),
    "cgs_mesh_contours": (_i, [_i, _vp, _i, _vp, _vp, _i, _i, _vp, C.c_double, _vp, _vp]),
    # the siblings with near before the output
    "cgs_mesh_depth_clipped": (_i, [_i, _vp, _i, _vp, _vp, _i, _i, C.c_double, _vp, _vp]),
    "cgs_mesh_contours_clipped": (_i, [_i, _vp, _i, _vp, _vp, _i, _i, _vp, C.c_double, C.c_double, _vp, _vp]),
    "cgs_surfel_depth": (_i, [_i, _vp, _vp, _vp, _i, _vp, _vp, _i, _i, _vp, _vp]),
    "cgs_stereo_sweep": (_i, [_i, _i, _i, _vp, _vp, _i, _vp, _i, _vp, _vp, _i, C.c_double, C.c_double, _i, _vp, _vp]),
    "cgs_stereo_consistency": (_i, [_i, _i, _i, _vp, _vp, _i, _vp, _vp, _vp, _i, _vp, _vp]),
    # (V, height, width, depth, intr, F, fsrc, into, v0, nv, warped, stream)
    "cgs_stereo_warp": (_i, [_i, _i, _i, _vp, _vp, _i, _vp, _vp, _i, _i, _vp, _vp]),
    # (V, height, width, depth, F, warped, tol, min_support, v0, nv, out, support, stream)
    "cgs_stereo_fuse": (_i, [_i, _i, _i, _vp, _i, _vp, _vp, _i, _i, _i, _vp, _vp, _vp]),
    # (nx, ny, nz, lo, step, V, intr, w2c, height, width, depth, trunc, accumulate, sum, weight, stream)
    "cgs_tsdf_integrate": (_i, [_i, _i, _i, _vp, _vp, _i, _vp, _vp, _i, _i, _vp, C.c_double, _i, _vp, _vp, _vp]),
    # (nx, ny, nz, sum, weight, min_weight, counts, stream)
    "cgs_tsdf_mesh_count": (_i, [_i, _i, _i, _vp, _vp, _i, _vp, _vp]),
    # (nx, ny, nz, lo, step, sum, weight, min_weight, offsets, T, tris, stream)
    "cgs_tsdf_mesh_emit": (_i, [_i, _i, _i, _vp, _vp, _vp, _vp, _i, _vp, _i64, _vp, _vp]),
}


class MetricView(C.Structure):
    """cgs_metric_view (include/curvegs.h)."""
    _fields_ = [("image", _vp), ("gt", _vp), ("channels", _i), ("height", _i), ("width", _i), ("x0", _i)]


class ReportView(C.Structure):
    """cgs_report_view (include/curvegs.h)."""
    _fields_ = [("render", _vp), ("gt", _vp), ("depth", _vp), ("rend_dir", _vp), ("rend_alpha", _vp), ("gt_channels", _i),
                ("height", _i), ("width", _i), ("written", C.c_uint), ("out_offset", C.c_size_t)]


class ViewGate(C.Structure):
    """cgs_view_gate (include/curvegs.h)."""
    _fields_ = [("planes", _vp), ("intr", _vp), ("w2c", _vp), ("view_index", _vp), ("slack", C.c_double), ("V", C.c_int32),
                ("view", C.c_int32), ("height", C.c_int32), ("width", C.c_int32)]


class UndistortView(C.Structure):
    """cgs_undistort_view (include/curvegs.h)."""
    _fields_ = [("src", _vp), ("dst", _vp), ("channels", _i), ("height", _i), ("width", _i), ("model", _i),
                ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double),
                ("out_fx", C.c_double), ("out_fy", C.c_double), ("k", C.c_double * 8)]


class EdgeGradientView(C.Structure):
    """cgs_edge_gradient_view (include/curvegs.h)."""
    _fields_ = [("pixels", _vp), ("gx", _vp), ("gy", _vp), ("m", _vp), ("height", _i), ("width", _i), ("channels", _i),
                ("reserved", _i)]


class EdgeTraceView(C.Structure):
    """cgs_edge_trace_view (include/curvegs.h)."""
    _fields_ = [("gx", _vp), ("gy", _vp), ("m", _vp), ("e", _vp), ("state", _vp), ("height", _i), ("width", _i)]


REPORT_MAX_VIEWS = 32   # CGS_REPORT_MAX_VIEWS
UNDISTORT_MAX_VIEWS = 24   # CGS_UNDISTORT_MAX_VIEWS
UNDISTORT_MAX_CHANNELS = 4   # CGS_UNDISTORT_MAX_CHANNELS
EDGE_MAX_VIEWS = 24   # CGS_EDGE_MAX_VIEWS
EDGE_MAX_RADIUS = 12   # CGS_EDGE_MAX_RADIUS
EDT_INF = 2147483647   # CGS_EDT_INF
EDT_MAX_SIZE = 16384   # CGS_EDT_MAX_SIZE
EDGE_SCORE_MAX_TOL = 8   # CGS_EDGE_SCORE_MAX_TOL
SEED_MAX_VIEWS = 65535   # CGS_SEED_MAX_VIEWS
SEED_MAX_RADIUS = 15   # CGS_SEED_MAX_RADIUS
SEED_MAX_WINDOW = 4   # CGS_SEED_MAX_WINDOW
EDGE_SUPPORT_MAX_TOL = 4   # CGS_EDGE_SUPPORT_MAX_TOL
THIN_PASS_ITERATIONS = 4   # CGS_THIN_PASS_ITERATIONS
THIN_TILE_WIDTH = 48   # CGS_THIN_TILE_WIDTH
THIN_TILE_HEIGHT = 240   # CGS_THIN_TILE_HEIGHT
ORIENT_RADIUS = 3   # CGS_ORIENT_RADIUS
ORIENT_MAX_TOL2 = 16   # CGS_ORIENT_MAX_TOL2
ORIENT_MAX_SPREAD = 4   # CGS_ORIENT_MAX_SPREAD
ORIENT_TILE_WIDTH = 64   # CGS_ORIENT_TILE_WIDTH
ORIENT_TILE_HEIGHT = 32   # CGS_ORIENT_TILE_HEIGHT
SNAP_MAX_CAP2 = 64   # CGS_SNAP_MAX_CAP2
SNAP_TERMS = 10   # CGS_SNAP_TERMS
DEPTH_MAX_WINDOW = 4   # CGS_DEPTH_MAX_WINDOW
STEREO_MAX_RADIUS = 8   # CGS_STEREO_MAX_RADIUS
STEREO_MAX_FUSE = 16   # CGS_STEREO_MAX_FUSE
TSDF_MAX_WEIGHT = 65535   # CGS_TSDF_MAX_WEIGHT
REPORT_PANELS = ("render", "ground_truth", "depth", "rend_dir", "rend_alpha")   # panel order of cgs_report_panels

_lib = None


class CurveGSError(RuntimeError):
    pass


def load() -> C.CDLL:
    """dlopen libcurvegs.so and attach signatures.  Raises if the library has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise CurveGSError(
            f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C curve_gaussian_amd/csrc`). There is no CPU fallback.")
    import torch  # noqa: F401  -- make sure torch's bundled libamdhip64.so.7 is the HIP runtime in this process
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


_shim = None
SHIM_PATH = os.path.join(_HERE, "_cgs_torch.so")
# _cgs_torch.so is linked against $ORIGIN/libcurvegs.so: with CGS_LIB pointing at an experiment build it would run the
# DEFAULT kernels (and hand out handles of another library instance) while ctypes drives the experiment -- an A/B run must
# use one library, so an overridden CGS_LIB selects the ctypes bindings.  Resolved once: use_shim() sits on the
# per-iteration path of the eager routes (two realpath() calls there cost 70 us per training iteration).
_LIB_IS_DEFAULT = os.path.realpath(LIB_PATH) == os.path.realpath(os.path.join(_HERE, "libcurvegs.so"))


def use_shim() -> bool:
    """The compiled torch <-> C-ABI host shim (csrc/torch_shim.cpp) is the default binding of the operator API and of the fused
    view route; CGS_TORCH_SHIM=0 selects the ctypes bindings instead (A/B measurements of the host floor).  Same library, same
    kernels either way."""
    if os.environ.get("CGS_TORCH_SHIM", "1") == "0":
        return False
    return _LIB_IS_DEFAULT


def shim():
    """import curve_gaussian_amd._cgs_torch (built by `make -C curve_gaussian_amd/csrc`).  Raises if it has not been built."""
    global _shim
    if _shim is not None:
        return _shim
    load()   # libcurvegs.so first (use_shim() is False when CGS_LIB names another build: the shim binds $ORIGIN/libcurvegs.so)
    if not os.path.exists(SHIM_PATH):
        raise CurveGSError(
            f"{SHIM_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C curve_gaussian_amd/csrc`); CGS_TORCH_SHIM=0 selects the ctypes bindings.")
    import importlib
    _shim = importlib.import_module("curve_gaussian_amd._cgs_torch")
    return _shim


def last_error() -> str:
    return load().cgs_last_error().decode("utf-8", "replace")


def check(rc, what: str):
    if rc < 0:
        raise CurveGSError(f"{what} failed (status {rc}): {last_error()}")
    return rc


def require_gpu_tensor(t, name: str):
    if not t.is_cuda:
        raise CurveGSError(f"{name} must be a GPU tensor (got device {t.device}); libcurvegs has no CPU path")


class _NoGuard:
    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False


_NO_GUARD = _NoGuard()


def device_guard(dev):
    """``torch.cuda.device(dev)`` only when `dev` is not already the current device (the context manager costs ~8 us of
    host time per op; the reference's shim has no device guard at all)."""
    import torch
    idx = dev.index
    if idx is None or idx == torch.cuda.current_device():
        return _NO_GUARD
    return torch.cuda.device(dev)


def raw_stream(dev):
    """hipStream_t of torch's current stream on `dev` as an int (one C call; torch.cuda.current_stream() builds a
    Stream object and is ~10x slower)."""
    import torch
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    return torch._C._cuda_getCurrentRawStream(idx)


def ptr(t):
    """Device pointer of a tensor, or NULL for None / empty tensors (the reference's 'empty tensor' convention)."""
    if t is None or t.numel() == 0:
        return None
    return C.c_void_p(t.data_ptr())


def prof_collect():
    lib = load()
    cap = 64
    names = (C.c_char_p * cap)()
    ms = (C.c_double * cap)()
    n_l = (_i64 * cap)()
    n = lib.cgs_prof_collect(names, ms, n_l, cap)
    return {names[i].decode(): (ms[i], int(n_l[i])) for i in range(min(n, cap))}
