"""CPU: the C-ABI library loads, exports every symbol declared in include/curvegs.h, and the Python operator layer
validates arguments like the reference before touching a GPU."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared_symbols():
    src = open(os.path.join(ROOT, "include", "curvegs.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(cgs_[a-z0-9_]+)\s*\(", src)) - {"cgs_alloc_fn"})


def test_library_exports_every_declared_symbol():
    from curve_gaussian_amd import _lib
    lib = _lib.load()
    names = _declared_symbols()
    assert len(names) >= 19
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/curvegs.h but not exported by libcurvegs.so"
        assert n in _lib.SIGNATURES, f"{n} has no ctypes signature in curve_gaussian_amd/_lib.py"
    assert lib.cgs_target_arch() == b"gfx950" and lib.cgs_version() >= 100


def test_workspace_size_queries_are_consistent():
    from curve_gaussian_amd import _lib
    lib = _lib.load()
    assert lib.cgs_geometry_bytes(1000) >= 1000 * (64 + 64 + 4 + 1)  # 64 B record + 64 B accumulators per splat
    assert lib.cgs_image_bytes(1600, 1600) >= 1600 * 1600 * 8 + 10000 * 16
    assert lib.cgs_binning_bytes(10 ** 6) >= 12 * 10 ** 6
    assert lib.cgs_geometry_bytes(2000) > lib.cgs_geometry_bytes(1000)
    assert lib.cgs_knn_workspace_bytes(3375) >= 3375 * 12


# ---------------------------------------------------------------------------------------------------------------------------
# Argument checks of the entries from the rasterizer to the mesh: one table.  Every entry has a baseline argument list that
# looks valid (dummy pointers: 64 is 16-byte aligned, 68 is not; none is ever dereferenced) and every row breaks it in one
# place, so that the entry returns before its first HIP call: -1 with the exact text of cgs_last_error(), 0 for an empty
# input, -3 for the operator forward whose allocation callbacks return NULL.  The baseline itself is never called and no row
# may pass validation (this file runs on GPU machines too, where a row that slipped through would launch on address 64).
A, MIS = ctypes.c_void_p(64), ctypes.c_void_p(68)

_SPLAT = ("{fn}: inconsistent inputs (need exactly one of shs/colors_precomp and one of (scales,rotations)/cov3D_precomp; "
          "all_map is required with render_geo)")
_VIEW_FWD_ARGS = ("B m curve_points width is_bezier coef eps norms opacity_logit mask_logit mask_thr colors_precomp "
                  "geometry_buffer binning_buffer binning_bytes image_buffer bucket_capacity background width_px height_px "
                  "viewmatrix projmatrix cam_pos tan_fovx tan_fovy out_color out_invdepth out_all_map radii xyz rotation "
                  "scaling stream")
_VIEW_FWD_BASE = dict(B=5, m=12, eps=1e-8, mask_logit=None, mask_thr=0.5, binning_bytes=1 << 30,
                      bucket_capacity=64, width_px=64, height_px=64, tan_fovx=0.3, tan_fovy=0.3, stream=None)
_VIEW_BWD_BASE = dict(B=5, m=12, eps=1e-8, mask_thr=0.5, width_px=64, height_px=64, tan_fovx=0.3,
                      tan_fovy=0.3, flags=0, stream=None)

# entry -> (argument names in ABI order, the baseline values that are not the dummy pointer); "alloc" is an allocation callback
# that returns NULL (with it the operator forward's baseline could only end in -3) and "views" two valid-looking descriptors
_ENTRIES = {
    "cgs_rasterize_forward": (
        "geometry_alloc geometry_user binning_alloc binning_user image_alloc image_user P D M background width height means3D "
        "shs colors_precomp opacities scales scale_modifier rotations cov3D_precomp all_map viewmatrix projmatrix cam_pos "
        "tan_fovx tan_fovy prefiltered out_color out_invdepth out_all_map antialiasing render_geo radii debug stream",
        dict(geometry_alloc="alloc", geometry_user=None, binning_alloc="alloc", binning_user=None, image_alloc="alloc",
             image_user=None, P=10, D=0, M=1, width=64, height=64, shs=None, scale_modifier=1.0, cov3D_precomp=None,
             tan_fovx=0.3, tan_fovy=0.3, prefiltered=0, antialiasing=0, render_geo=1, debug=0, stream=None)),
    "cgs_rasterize_forward_static": (
        "geometry_buffer binning_buffer binning_bytes image_buffer bucket_capacity P D M background width height means3D shs "
        "colors_precomp opacities scales scale_modifier rotations cov3D_precomp all_map viewmatrix projmatrix cam_pos "
        "tan_fovx tan_fovy out_color out_invdepth out_all_map antialiasing render_geo radii stream",
        dict(binning_bytes=1 << 30, bucket_capacity=64, P=10, D=0, M=1, width=64, height=64, shs=None, scale_modifier=1.0,
             cov3D_precomp=None, tan_fovx=0.3, tan_fovy=0.3, antialiasing=0, render_geo=1, stream=None)),
    "cgs_rasterize_backward": (
        "P D M R background width height means3D shs colors_precomp all_map opacities scales scale_modifier rotations "
        "cov3D_precomp viewmatrix projmatrix cam_pos tan_fovx tan_fovy radii geometry_buffer binning_buffer image_buffer "
        "dL_dout_color dL_dout_invdepth dL_dout_all_map dL_dmean2D dL_dconic dL_dopacity dL_dcolor dL_dinvdepth dL_dmean3D "
        "dL_dcov3D dL_dsh dL_dscale dL_drot dL_dall_map antialiasing render_geo debug stream",
        dict(P=10, D=0, M=1, R=100, width=64, height=64, shs=None, scale_modifier=1.0, cov3D_precomp=None, tan_fovx=0.3,
             tan_fovy=0.3, dL_dsh=None, antialiasing=0, render_geo=1, debug=0, stream=None)),
    "cgs_mark_visible": ("P means3D viewmatrix projmatrix present stream", dict(P=10, stream=None)),
    "cgs_sample_curves_forward": ("B m curve_points width is_bezier coef eps norms xyz rotation scaling stream",
                                  dict(B=5, m=12, eps=1e-8, stream=None)),
    "cgs_sample_curves_backward": (
        "B m curve_points width is_bezier coef eps norms dL_dxyz dL_drotation dL_dscaling dL_dcurve_points dL_dwidth scratch "
        "stream", dict(B=5, m=12, eps=1e-8, stream=None)),
    "cgs_view_forward": (_VIEW_FWD_ARGS, dict(_VIEW_FWD_BASE, colors_precomp=None)),
    "cgs_view_forward_checked": (_VIEW_FWD_ARGS, dict(_VIEW_FWD_BASE, colors_precomp=None)),
    "cgs_view_forward_begin": (_VIEW_FWD_ARGS, dict(_VIEW_FWD_BASE, colors_precomp=None)),
    "cgs_view_forward_shared": (_VIEW_FWD_ARGS, dict(_VIEW_FWD_BASE, colors_precomp=None)),
    "cgs_view_forward_render": (
        "checked B m curve_points width is_bezier coef eps norms opacity_logit mask_logit mask_thr geometry_buffer "
        "binning_buffer binning_bytes image_buffer bucket_capacity background width_px height_px viewmatrix projmatrix cam_pos "
        "tan_fovx tan_fovy out_color out_invdepth out_all_map radii out_color_clamped out_rend_dir stream",
        dict(_VIEW_FWD_BASE, checked=1)),
    "cgs_view_forward_wait": ("handle n_visible", dict(handle=0, n_visible=None)),
    "cgs_view_backward": (
        "B m curve_points width is_bezier coef eps norms opacity_logit mask_logit mask_thr colors_precomp geometry_buffer "
        "binning_buffer image_buffer background width_px height_px viewmatrix projmatrix cam_pos tan_fovx tan_fovy radii "
        "dL_dout_color dL_drotation_extra dL_dmeans2D dL_dcurve_points dL_dwidth dL_dopacity_logit dL_dmask_logit scratch "
        "flags stream", dict(_VIEW_BWD_BASE, colors_precomp=None)),
    "cgs_view_backward_render": (
        "B m curve_points width is_bezier coef eps norms opacity_logit mask_logit mask_thr geometry_buffer binning_buffer "
        "image_buffer background width_px height_px viewmatrix projmatrix cam_pos tan_fovx tan_fovy radii dL_dout_color "
        "color_raw dL_dmeans2D dL_dcurve_points dL_dwidth dL_dopacity_logit dL_dmask_logit scratch flags stream",
        _VIEW_BWD_BASE),
    "cgs_view_shared_begin": ("B m curve_points is_bezier coef norms scratch stream", dict(B=5, m=12, stream=None)),
    "cgs_view_shared_end": (
        "B m curve_points width is_bezier coef eps norms scratch dL_dcurve_points dL_dwidth accumulate stream",
        dict(B=5, m=12, eps=1e-8, accumulate=0, stream=None)),
    "cgs_visible_indices": ("P radii image_buffer width height out_indices stream",
                            dict(P=10, width=64, height=64, stream=None)),
    "cgs_splat_attrs_forward": (
        "B m rotation_raw xyz opacity_logit mask_logit mask_thr scaling campos viewmatrix rotation_n opacity scaling_out "
        "all_map stream", dict(B=5, m=12, mask_thr=0.5, stream=None)),
    "cgs_splat_attrs_backward": (
        "B m rotation_raw xyz opacity_logit mask_logit mask_thr scaling campos viewmatrix dL_drotation_n dL_dopacity "
        "dL_dscaling_out dL_dall_map dL_drotation_raw dL_dopacity_logit dL_dmask_logit dL_dscaling stream",
        dict(B=5, m=12, mask_thr=0.5, stream=None)),
    "cgs_ssim_forward": (
        "batch channels height width C1 C2 img1 img2 ssim_map dm_dmu1 dm_dsigma1_sq dm_dsigma12 stream",
        dict(batch=1, channels=3, height=8, width=8, C1=1e-4, C2=9e-4, stream=None)),
    "cgs_ssim_backward": (
        "batch channels height width C1 C2 img1 img2 dL_dmap dm_dmu1 dm_dsigma1_sq dm_dsigma12 dL_dimg1 stream",
        dict(batch=1, channels=3, height=8, width=8, C1=1e-4, C2=9e-4, stream=None)),
    "cgs_edge_aware_loss": ("channels height width image gt threshold scratch16 dL_dimage stream",
                            dict(channels=1, height=8, width=8, threshold=0.1, stream=None)),
    "cgs_render_epilogue": ("height width color_raw all_map viewmatrix clamp color_out dir_out stream",
                            dict(height=8, width=8, clamp=1, stream=None)),
    "cgs_clamp_backward": ("n raw g_in g_out stream", dict(n=64, stream=None)),
    "cgs_edge_count": ("channels height width gt threshold n_pos stream",
                       dict(channels=1, height=8, width=8, threshold=0.1, stream=None)),
    "cgs_photometric_loss": (
        "height width image gt threshold n_pos lambda_edge lambda_ssim clamp_input workspace dL_dimage loss stream",
        dict(height=8, width=8, threshold=0.1, lambda_edge=1.0, lambda_ssim=0.2, clamp_input=0, stream=None)),
    "cgs_photometric_loss_indexed": (
        "height width image gt_stack view_index threshold n_pos_table lambda_edge lambda_ssim clamp_input workspace dL_dimage "
        "loss stream", dict(height=8, width=8, threshold=0.1, lambda_edge=1.0, lambda_ssim=0.2, clamp_input=0, stream=None)),
    "cgs_curve_regularizers": (
        "B m rotation_raw opacity_logit width_log radii w_opacity opacity_gate w_smooth w_width width_threshold workspace loss "
        "dL_drotation_raw dL_dopacity_logit dL_dwidth_log stream",
        dict(B=5, m=12, w_opacity=0.1, w_smooth=0.1, w_width=0.1, width_threshold=0.5, stream=None)),
    "cgs_adam_step_flat": (
        "n params grads exp_avg exp_avg_sq segments n_segments beta1 beta2 eps step zero_grads stream",
        dict(n=64, segments=b"\0" * 64, n_segments=1, beta1=0.9, beta2=0.999, eps=1e-15, step=1, zero_grads=1, stream=None)),
    "cgs_adam_step_flat_dev": (
        "n params grads exp_avg exp_avg_sq device_state n_segments beta1 beta2 eps zero_grads skip_flag stream",
        dict(n=64, n_segments=1, beta1=0.9, beta2=0.999, eps=1e-15, zero_grads=1, stream=None)),
    "cgs_adam_step_flat_dev_report": (
        "n params grads exp_avg exp_avg_sq device_state n_segments beta1 beta2 eps zero_grads skip_flag report_seq report_ring "
        "report_len stream", dict(n=64, n_segments=1, beta1=0.9, beta2=0.999, eps=1e-15, zero_grads=1, report_len=8,
                                  stream=None)),
    "cgs_endpoint_connection_loss": (
        "B curve_points distance_threshold weight workspace loss dL_dcurve_points accumulate stream",
        dict(B=5, distance_threshold=0.1, weight=1.0, accumulate=0, stream=None)),
    "cgs_knn_mean_dist2": ("P points mean_dist2 workspace stream", dict(P=10, stream=None)),
    "cgs_densification_stats": (
        "P radii dL_dmeans2D grad_stride max_radii2D xyz_gradient_accum denom skip_flag stream",
        dict(P=10, grad_stride=3, stream=None)),
    "cgs_view_metrics": ("n_views views workspace sums means stream", dict(n_views=2, views="views", stream=None)),
    "cgs_ellipsoid_mesh_body_bytes": ("P resolution vertex_bytes face_bytes",
                                      dict(P=10, resolution=8, vertex_bytes=None, face_bytes=None)),
    "cgs_ellipsoid_mesh_vertices": ("first count xyz rot scale rgb V0 unit_vertices out stream",
                                    dict(first=0, count=10, V0=114, stream=None)),
    "cgs_ellipsoid_mesh_faces": ("first count V0 F0 template_faces out stream",
                                 dict(first=0, count=10, V0=114, F0=224, stream=None)),
}


def _metric_views(**broken):
    """Two valid-looking cgs_metric_view descriptors, the SECOND one broken (its index is part of the message)."""
    from curve_gaussian_amd import _lib
    fields = dict(image=64, gt=64, channels=3, height=8, width=16, x0=0)
    return (_lib.MetricView * 2)(_lib.MetricView(**fields), _lib.MetricView(**dict(fields, **broken)))


def _rejection_rows(lib):
    """(entry, {argument: broken value}, expected status, expected cgs_last_error() or None)."""
    rows = []

    def add(fn, msg, *changes, status=-1):
        rows.extend((fn, c, status, None if msg is None else msg.format(fn=fn)) for c in changes)

    def each(value, names):
        return [{n: value} for n in names.split()]

    def cap_msg(fn, cap, got, tiles=16):   # bucket_cap_ok (a 64 x 64 frame has 16 tiles)
        return (f"{fn}: bucket capacity {cap} needs {lib.cgs_binning_bytes(cap * tiles)} binning bytes (got {got}; "
                f"limit {limit} per tile)")

    limit = lib.cgs_bucket_capacity_limit()
    # ---- the operator API
    fn = "cgs_rasterize_forward"
    for c in [dict(P=-1), dict(width=0), dict(height=-4)] + each(None, "out_color out_invdepth out_all_map background "
                                                                 "viewmatrix projmatrix"):
        add(fn, f"{fn}: invalid argument (P={c.get('P', 10)} W={c.get('width', 64)} H={c.get('height', 64)} or NULL "
                "output/camera pointer)", c)
    splat = each(None, "means3D opacities radii colors_precomp scales rotations all_map") + [
        dict(shs=A), dict(cov3D_precomp=A), dict(shs=A, colors_precomp=None, cam_pos=None),
        dict(shs=A, colors_precomp=None, M=0)]
    add(fn, _SPLAT, *splat)
    add(fn, "{fn}: rotations/all_map must be 16-byte aligned", dict(rotations=MIS), dict(all_map=MIS))
    # (reached before any device work; the baseline's three callbacks all return NULL, the row names the first to be asked)
    add(fn, "{fn}: geometry/image allocation callback returned NULL", dict(geometry_alloc="alloc"), status=-3)
    fn = "cgs_rasterize_forward_static"
    add(fn, "{fn}: invalid argument (P=0 W=64 H=64, NULL pointer or zero capacity)", dict(P=0))
    add(fn, "{fn}: invalid argument (P=10 W=64 H=0, NULL pointer or zero capacity)", dict(height=0))
    add(fn, "{fn}: invalid argument (P=10 W=-1 H=64, NULL pointer or zero capacity)", dict(width=-1))
    add(fn, "{fn}: invalid argument (P=10 W=64 H=64, NULL pointer or zero capacity)", dict(bucket_capacity=0),
        *each(None, "out_color out_invdepth out_all_map background viewmatrix projmatrix geometry_buffer binning_buffer "
                    "image_buffer"))
    add(fn, _SPLAT, *splat)
    add(fn, "{fn}: rotations/all_map must be 16-byte aligned", dict(rotations=MIS), dict(all_map=MIS))
    add(fn, cap_msg(fn, limit + 1, 1 << 30), dict(bucket_capacity=limit + 1))
    add(fn, cap_msg(fn, 64, 4096), dict(binning_bytes=4096))
    add(fn, cap_msg(fn, 2048, 1 << 40, tiles=1 << 20),   # 2^31 slots: one too many, whatever the buffer
        dict(width=16384, height=16384, bucket_capacity=2048, binning_bytes=1 << 40))
    add(fn, _SPLAT, dict(means3D=None, binning_bytes=4096))   # the splat inputs are checked before the capacity
    fn = "cgs_rasterize_backward"
    add(fn, None, dict(P=0), dict(P=0, width=0, rotations=MIS), status=0)   # an empty cloud: a no-op before any check
    add(fn, "{fn}: invalid argument", dict(P=-1), dict(width=0), dict(height=0), dict(shs=A),
        dict(shs=A, dL_dsh=A, dL_dcolor=None),
        *each(None, "geometry_buffer binning_buffer image_buffer radii dL_dout_color dL_dmean2D dL_dopacity dL_dmean3D "
                    "dL_dcov3D dL_dall_map dL_dout_invdepth dL_dinvdepth dL_dscale dL_drot"))
    add(fn, "{fn}: dL_dcolor may only be NULL when no depth / all_map gradients flow in", dict(dL_dcolor=None),
        dict(dL_dcolor=None, render_geo=0), dict(dL_dcolor=None, dL_dout_all_map=None),
        dict(dL_dcolor=None, rotations=MIS))   # (before the alignment)
    add(fn, "{fn}: rotations/dL_dconic/dL_drot must be 16-byte aligned", *each(MIS, "rotations dL_dconic dL_drot dL_dall_map"))
    fn = "cgs_mark_visible"
    add(fn, None, dict(P=0), dict(P=0, means3D=None), status=0)
    add(fn, "{fn}: invalid argument", dict(P=-1), *each(None, "means3D viewmatrix present"))
    # ---- curve sampling
    fn = "cgs_sample_curves_forward"
    add(fn, None, dict(B=0), dict(B=0, m=0, curve_points=MIS), status=0)
    add(fn, "{fn}: invalid argument (NULL or misaligned pointer, B=-1 m=12)", dict(B=-1))
    add(fn, "{fn}: invalid argument (NULL or misaligned pointer, B=5 m=0)", dict(m=0))
    add(fn, "{fn}: invalid argument (NULL or misaligned pointer, B=5 m=33)", dict(m=33))
    add(fn, "{fn}: invalid argument (NULL or misaligned pointer, B=5 m=12)",
        *each(None, "curve_points width coef norms xyz rotation scaling"), *each(MIS, "curve_points rotation coef"))
    fn = "cgs_sample_curves_backward"
    add(fn, None, dict(B=0), dict(B=0, m=0, curve_points=MIS), status=0)
    add(fn, "{fn}: invalid argument", dict(B=-1), dict(m=0), dict(m=33), dict(scratch=None),
        *each(None, "curve_points width coef norms dL_dcurve_points dL_dwidth"),
        *each(MIS, "curve_points dL_drotation dL_dcurve_points coef"))
    # ---- the fused view route: one validation behind the five forwards (all report as cgs_view_forward), one behind the
    # two backwards (as cgs_view_backward)
    for fn in ("cgs_view_forward", "cgs_view_forward_checked", "cgs_view_forward_begin", "cgs_view_forward_shared",
               "cgs_view_forward_render"):
        msg = "cgs_view_forward: invalid argument (B={B} m={m} W={W} H={H}, NULL / misaligned pointer or zero capacity)"
        for c in (dict(B=0), dict(B=-1), dict(m=0), dict(m=33), dict(B=1 << 24, m=16), dict(width_px=0), dict(height_px=-2)):
            add(fn, msg.format(B=c.get("B", 5), m=c.get("m", 12), W=c.get("width_px", 64), H=c.get("height_px", 64)), c)
        plain = msg.format(B=5, m=12, W=64, H=64)
        add(fn, plain, dict(bucket_capacity=0), dict(out_invdepth=None), dict(curve_points=MIS), dict(coef=MIS),
            *each(None, "curve_points width coef norms opacity_logit geometry_buffer binning_buffer image_buffer background "
                        "viewmatrix projmatrix cam_pos out_color radii"))
        if fn == "cgs_view_forward_render":   # (no colours, no xyz / rotation / scaling outputs)
            add(fn, "cgs_view_forward: the direction map needs the all_map output", dict(out_all_map=None),
                dict(out_all_map=None, out_invdepth=None), dict(out_all_map=None, B=0))
            add(fn, plain, dict(out_all_map=None, out_rend_dir=None), dict(checked=0, radii=None))
        else:
            add(fn, plain, dict(out_all_map=None), dict(out_all_map=None, out_invdepth=None, colors_precomp=A),
                dict(rotation=None), dict(scaling=None), dict(rotation=MIS))
        add(fn, cap_msg("cgs_view_forward", limit + 1, 1 << 30), dict(bucket_capacity=limit + 1))
        add(fn, cap_msg("cgs_view_forward", 64, 4096), dict(binning_bytes=4096))
        add(fn, cap_msg("cgs_view_forward", 2048, 1 << 40, tiles=1 << 20),   # 2^31 slots: one too many, whatever the buffer
            dict(width_px=16384, height_px=16384, bucket_capacity=2048, binning_bytes=1 << 40))
        add(fn, plain, dict(binning_bytes=4096, radii=None))   # (before the capacity)
    fn = "cgs_view_forward_wait"
    for h in (-1, 64, 1 << 20):   # outside the pool of 64 slots: never a handle, whatever else the process has in flight
        add(fn, f"{fn}: handle {h} is not an outstanding checked forward", dict(handle=h))
    for fn in ("cgs_view_backward", "cgs_view_backward_render"):
        add(fn, "cgs_view_backward: invalid argument", dict(B=0), dict(B=-1), dict(m=0), dict(m=33), dict(width_px=0),
            dict(height_px=0),
            *each(None, "curve_points width coef norms opacity_logit geometry_buffer binning_buffer image_buffer background "
                        "viewmatrix projmatrix cam_pos radii dL_dout_color dL_dmeans2D dL_dcurve_points dL_dwidth "
                        "dL_dopacity_logit scratch dL_dmask_logit"),
            *each(MIS, "curve_points coef dL_dcurve_points"))
    add("cgs_view_backward", "{fn}: invalid argument", dict(dL_drotation_extra=MIS))
    fn = "cgs_view_shared_begin"
    add(fn, "{fn}: invalid argument", dict(B=0), dict(B=-1), dict(m=0), dict(m=33),
        *each(None, "curve_points coef norms scratch"), *each(MIS, "curve_points coef"))
    fn = "cgs_view_shared_end"
    add(fn, "{fn}: invalid argument", dict(B=0), dict(B=-1), dict(m=0), dict(m=33),
        *each(None, "curve_points width coef norms scratch dL_dcurve_points dL_dwidth"),
        *each(MIS, "curve_points coef dL_dcurve_points"))
    fn = "cgs_visible_indices"
    add(fn, "{fn}: invalid argument", dict(P=0), dict(P=-1), dict(width=0), dict(height=0),
        *each(None, "radii image_buffer out_indices"))
    # ---- splat attributes
    fn = "cgs_splat_attrs_forward"
    add(fn, None, dict(B=0), dict(B=0, m=0, rotation_raw=MIS), status=0)
    add(fn, "{fn}: invalid argument", dict(B=-1), dict(m=0), dict(scaling=None),
        *each(None, "rotation_raw xyz opacity_logit campos viewmatrix rotation_n opacity all_map"),
        *each(MIS, "rotation_raw rotation_n all_map"))
    fn = "cgs_splat_attrs_backward"
    add(fn, None, dict(B=0), dict(B=0, m=0, rotation_raw=MIS), status=0)
    add(fn, "{fn}: invalid argument", dict(B=-1), dict(m=0),
        *each(None, "rotation_raw xyz opacity_logit campos viewmatrix dL_drotation_raw dL_dopacity_logit"),
        *each(MIS, "rotation_raw dL_drotation_n dL_dall_map dL_drotation_raw"))
    # ---- SSIM and the losses
    for fn, ptrs in (("cgs_ssim_forward", "img1 img2 ssim_map dm_dsigma1_sq dm_dsigma12"),
                     ("cgs_ssim_backward", "img1 img2 dL_dmap dm_dmu1 dm_dsigma1_sq dm_dsigma12 dL_dimg1")):
        # an empty image is a no-op BEFORE the checks: (0, 3, -8, 8) is not rejected for its negative height
        add(fn, None, dict(batch=0), dict(channels=0), dict(height=0), dict(width=0), dict(batch=0, height=-8),
            dict(width=0, img1=None), dict(batch=-1, channels=0), status=0)
        add(fn, "{fn}: invalid argument", dict(batch=-1), dict(channels=-3), dict(height=-8), dict(width=-8),
            dict(batch=65536, channels=1), dict(batch=256, channels=256), *each(None, ptrs))
    fn = "cgs_edge_aware_loss"
    add(fn, "{fn}: invalid argument", dict(channels=0), dict(height=0), dict(width=-1), *each(None, "image gt scratch16"))
    fn = "cgs_render_epilogue"
    add(fn, None, dict(color_out=None, dir_out=None), status=0)   # nothing to write
    add(fn, "{fn}: invalid argument", dict(height=0), dict(width=0), dict(color_raw=None), dict(all_map=None),
        dict(viewmatrix=None), dict(height=0, color_out=None, dir_out=None))   # (the size is checked before the no-op)
    fn = "cgs_clamp_backward"
    add(fn, None, dict(n=0), dict(n=0, raw=None, g_in=None, g_out=None), status=0)
    add(fn, "{fn}: invalid argument", dict(n=-1), dict(n=-1, raw=None), *each(None, "raw g_in g_out"))
    fn = "cgs_edge_count"
    add(fn, "{fn}: invalid argument", dict(channels=0), dict(height=0), dict(width=0), *each(None, "gt n_pos"))
    fn = "cgs_photometric_loss"
    add(fn, "{fn}: invalid argument", dict(height=0), dict(width=0), *each(None, "image gt n_pos workspace dL_dimage loss"))
    fn = "cgs_photometric_loss_indexed"
    add(fn, "{fn}: invalid argument", dict(height=0), dict(width=0),
        *each(None, "image gt_stack view_index n_pos_table workspace dL_dimage loss"))
    # ---- regularizers, Adam, the endpoint loss
    fn = "cgs_curve_regularizers"
    add(fn, "{fn}: invalid argument (NULL / misaligned pointer, B=0 m=12)", dict(B=0))
    add(fn, "{fn}: invalid argument (NULL / misaligned pointer, B=-1 m=12)", dict(B=-1))
    add(fn, "{fn}: invalid argument (NULL / misaligned pointer, B=5 m=1)", dict(m=1))
    add(fn, "{fn}: invalid argument (NULL / misaligned pointer, B=5 m=33)", dict(m=33))
    add(fn, "{fn}: invalid argument (NULL / misaligned pointer, B=5 m=12)",
        *each(None, "rotation_raw opacity_logit width_log radii workspace loss dL_drotation_raw dL_dopacity_logit "
                    "dL_dwidth_log"), *each(MIS, "rotation_raw dL_drotation_raw"))
    fn = "cgs_adam_step_flat"
    add(fn, None, dict(n=0), dict(n=0, params=None, step=0), status=0)
    add(fn, "{fn}: invalid argument", dict(n=-1), dict(n_segments=0), dict(n_segments=1 << 20), dict(step=0),
        *each(None, "params grads exp_avg exp_avg_sq segments"))
    fn = "cgs_adam_step_flat_dev"
    add(fn, None, dict(n=0), dict(n=0, params=None, n_segments=0), status=0)
    add(fn, "{fn}: invalid argument", dict(n=-1), dict(n_segments=0), dict(n_segments=1 << 20),
        *each(None, "params grads exp_avg exp_avg_sq device_state"))
    fn = "cgs_adam_step_flat_dev_report"
    add(fn, None, dict(n=0), dict(n=0, report_seq=None, report_len=0), status=0)
    add(fn, "{fn}: invalid argument", dict(n=-1), dict(n_segments=0), dict(n_segments=1 << 20), dict(report_len=0),
        *each(None, "params grads exp_avg exp_avg_sq device_state report_seq report_ring"))
    fn = "cgs_endpoint_connection_loss"
    add(fn, "{fn}: invalid argument (NULL pointer, B=0 or threshold <= 0)", dict(B=0))
    add(fn, "{fn}: invalid argument (NULL pointer, B=-1 or threshold <= 0)", dict(B=-1))
    add(fn, "{fn}: invalid argument (NULL pointer, B=5 or threshold <= 0)", dict(distance_threshold=0.0),
        dict(distance_threshold=-1.0), dict(distance_threshold=float("nan")),
        *each(None, "curve_points workspace loss dL_dcurve_points"))
    # ---- KNN, densification, metrics
    fn = "cgs_knn_mean_dist2"
    add(fn, None, dict(P=0), dict(P=0, points=None, mean_dist2=None, workspace=None), status=0)
    add(fn, "{fn}: invalid argument", dict(P=-1), *each(None, "points mean_dist2 workspace"))
    fn = "cgs_densification_stats"
    add(fn, None, dict(P=0), dict(P=0, radii=None), status=0)
    add(fn, "{fn}: invalid argument (P=-1, grad_stride=3)", dict(P=-1))
    add(fn, "{fn}: invalid argument (P=10, grad_stride=1)", dict(grad_stride=1))
    add(fn, "{fn}: invalid argument (P=0, grad_stride=1)", dict(P=0, grad_stride=1))   # (the stride: before the no-op)
    add(fn, "{fn}: invalid argument (NULL pointer)", *each(None, "radii dL_dmeans2D max_radii2D xyz_gradient_accum denom"))
    fn = "cgs_view_metrics"
    add(fn, None, dict(n_views=0), dict(n_views=0, views=None), status=0)
    add(fn, "{fn}: invalid argument (n_views=-1)", dict(n_views=-1))
    add(fn, "{fn}: invalid argument (n_views=65536)", dict(n_views=65536), dict(n_views=65536, views=None))
    add(fn, "{fn}: invalid argument (NULL pointer)", *each(None, "views workspace sums"))
    add(fn, "{fn}: invalid argument (view 1: NULL pointer)", dict(views=_metric_views(image=None)),
        dict(views=_metric_views(gt=None)), dict(views=_metric_views(gt=None, channels=0)))
    for bad in (dict(channels=0), dict(height=0), dict(width=0), dict(x0=-1), dict(x0=16)):
        d = dict(dict(channels=3, height=8, width=16, x0=0), **bad)
        add(fn, "{fn}: invalid argument (view 1: channels=%d, height=%d, width=%d, x0=%d)"
            % (d["channels"], d["height"], d["width"], d["x0"]), dict(views=_metric_views(**bad)))
    # ---- the ellipsoid mesh
    fn = "cgs_ellipsoid_mesh_body_bytes"
    add(fn, "{fn}: invalid argument (P=-1, resolution=8)", dict(P=-1))
    add(fn, "{fn}: invalid argument (P=10, resolution=1)", dict(resolution=1))
    add(fn, "{fn}: invalid argument (P=10, resolution=1025)", dict(resolution=1025))
    add(fn, "{fn}: 2048 splats of 2095106 vertices: a vertex index would not fit in an int", dict(P=2048, resolution=1024))
    fn = "cgs_ellipsoid_mesh_vertices"
    add(fn, None, dict(count=0), dict(count=0, xyz=None, out=MIS), status=0)
    add(fn, "{fn}: invalid argument (first=-1, count=10, V0=114)", dict(first=-1))
    add(fn, "{fn}: invalid argument (first=0, count=-1, V0=114)", dict(count=-1))
    add(fn, "{fn}: invalid argument (first=0, count=10, V0=0)", dict(V0=0))
    add(fn, "{fn}: invalid argument (first=1048576, count=0, V0=4096)",   # before the no-op
        dict(first=1 << 20, count=0, V0=4096))
    add(fn, "{fn}: invalid argument (NULL pointer)", *each(None, "xyz rot scale rgb unit_vertices out"))
    add(fn, "{fn}: out must be 16-byte aligned", dict(out=MIS))
    fn = "cgs_ellipsoid_mesh_faces"
    add(fn, None, dict(count=0), dict(count=0, template_faces=None, out=MIS), status=0)
    add(fn, "{fn}: invalid argument (first=-1, count=10, V0=114, F0=224)", dict(first=-1))
    add(fn, "{fn}: invalid argument (first=0, count=-1, V0=114, F0=224)", dict(count=-1))
    add(fn, "{fn}: invalid argument (first=0, count=10, V0=0, F0=224)", dict(V0=0))
    add(fn, "{fn}: invalid argument (first=0, count=10, V0=114, F0=0)", dict(F0=0))
    add(fn, "{fn}: splats [1048576, 1048576) of 4096 vertices: a vertex index would not fit in an int",
        dict(first=1 << 20, count=0, V0=4096))   # before the no-op
    add(fn, "{fn}: invalid argument (NULL pointer)", *each(None, "template_faces out"))
    add(fn, "{fn}: out must be 16-byte aligned", dict(out=MIS))
    return rows


def test_argument_checks_of_the_older_entries_are_pinned():
    from curve_gaussian_amd import _lib
    lib = _lib.load()
    special = {"alloc": _lib.ALLOC_FN(lambda user, nbytes: None), "views": _metric_views()}
    rows = _rejection_rows(lib)
    assert {r[0] for r in rows} == set(_ENTRIES)
    for fn, changes, status, message in rows:
        names, base = _ENTRIES[fn]
        names = names.split()
        assert len(names) == len(_lib.SIGNATURES[fn][1]) and set(base) | set(changes) <= set(names), (fn, changes)
        assert changes and status in (0, -1, -3) and (message is None) == (status == 0), (fn, changes)
        values = dict({n: A for n in names}, **base)
        values.update(changes)
        rc = getattr(lib, fn)(*[special.get(v, v) if isinstance(v, str) else v for v in (values[n] for n in names)])
        assert rc == status, (fn, changes, rc, lib.cgs_last_error())
        if status < 0:   # (the text is sticky: it says nothing after a 0)
            assert lib.cgs_last_error().decode() == message, (fn, changes)
    # a bad handle is a silent no-op for cgs_view_forward_abandon: nothing returned, the error text untouched
    before = lib.cgs_last_error()
    for handle in (-1, 64, 1 << 20):
        assert lib.cgs_view_forward_abandon(handle) is None
    assert lib.cgs_last_error() == before


def test_rasterizer_argument_checks_match_reference():
    """GaussianRasterizer.forward raises before any device work (reference __init__.py:189-193)."""
    from curve_gaussian_amd.diff_cur_rasterization import GaussianRasterizationSettings, GaussianRasterizer
    fields = GaussianRasterizationSettings._fields
    # the reference's 14 fields in the reference's order (:153-167), then the optional extensions with defaults
    assert fields[:14] == ("image_height", "image_width", "tanfovx", "tanfovy", "bg", "scale_modifier", "viewmatrix",
                           "projmatrix", "sh_degree", "campos", "prefiltered", "debug", "antialiasing", "render_geo")
    assert fields[14:] == ("static_bucket_cap", "status_sink", "options")
    assert GaussianRasterizationSettings._field_defaults == {"static_bucket_cap": 0, "status_sink": None, "options": 0}
    rs = GaussianRasterizationSettings(8, 8, 0.3, 0.3, torch.zeros(3), 1.0, torch.eye(4), torch.eye(4), 0,
                                       torch.zeros(3), False, False, False, True)
    r = GaussianRasterizer(rs)
    m = torch.zeros(4, 3)
    with pytest.raises(Exception, match="SHs or precomputed colors"):
        r(means3D=m, means2D=m, opacities=torch.zeros(4, 1), scales=m, rotations=torch.zeros(4, 4))
    with pytest.raises(Exception, match="SHs or precomputed colors"):
        r(means3D=m, means2D=m, opacities=torch.zeros(4, 1), shs=torch.zeros(4, 1), colors_precomp=torch.zeros(4, 1),
          scales=m, rotations=torch.zeros(4, 4))
    with pytest.raises(Exception, match="scale/rotation pair or precomputed 3D covariance"):
        r(means3D=m, means2D=m, opacities=torch.zeros(4, 1), colors_precomp=torch.zeros(4, 1), scales=m)
    with pytest.raises(Exception, match="scale/rotation pair or precomputed 3D covariance"):
        r(means3D=m, means2D=m, opacities=torch.zeros(4, 1), colors_precomp=torch.zeros(4, 1), scales=m,
          rotations=torch.zeros(4, 4), cov3D_precomp=torch.zeros(4, 6))


def test_host_shim_loads_and_mirrors_the_reference_pybind_module(monkeypatch):
    """curve_gaussian_amd._cgs_torch (csrc/torch_shim.cpp) is what `diff_cur_rasterization._C` resolves to: the three entry
    points of the reference's pybind module (ext.cpp:15-19) with its argument counts, plus the extensions; CGS_TORCH_SHIM=0
    selects the ctypes bindings over the same library."""
    from curve_gaussian_amd import _lib
    from curve_gaussian_amd import diff_cur_rasterization as D
    shim = _lib.shim()
    for name in ("rasterize_gaussians", "rasterize_gaussians_backward", "mark_visible", "rasterize_gaussians_static",
                 "forward_status", "view_forward", "view_backward", "view_wait", "view_abandon"):
        assert callable(getattr(shim, name)), name
    assert _lib.use_shim()
    monkeypatch.setattr(D._ExtProxy, "_impl", None)
    assert D._C.rasterize_gaussians is shim.rasterize_gaussians
    # RasterizeGaussiansCUDA takes 22 arguments (rasterize_points.h:18-44): one short is a TypeError before any device work
    with pytest.raises(TypeError):
        shim.rasterize_gaussians(*([torch.zeros(3)] * 21))
    with pytest.raises(RuntimeError, match=r"means3D must have dimensions \(num_points, 3\)"):   # rasterize_points.cu:60-62
        shim.rasterize_gaussians(torch.zeros(3), torch.zeros(5), torch.ones(5, 1), torch.ones(5, 1), torch.ones(5, 3),
                                 torch.ones(5, 4), 1.0, torch.empty(0), torch.ones(5, 4), torch.eye(4), torch.eye(4), 0.5, 0.5, 16,
                                 16, torch.empty(0), 0, torch.zeros(3), False, False, True, False)
    monkeypatch.setenv("CGS_TORCH_SHIM", "0")
    monkeypatch.setattr(D._ExtProxy, "_impl", None)
    assert D._C.mark_visible is not None and isinstance(D._ExtProxy._impl, D._Ext)
    monkeypatch.setattr(D._ExtProxy, "_impl", None)


def test_product_has_no_cpu_fallback():
    from curve_gaussian_amd import _lib
    from curve_gaussian_amd.diff_cur_rasterization import _C
    from curve_gaussian_amd.fused_ssim import fused_ssim
    from curve_gaussian_amd.ops.curve_sampling import sample_curves
    from curve_gaussian_amd.simple_knn import distCUDA2
    with pytest.raises(_lib.CurveGSError, match="GPU tensor"):
        _C.mark_visible(torch.zeros(3, 3), torch.eye(4), torch.eye(4))
    with pytest.raises(_lib.CurveGSError, match="GPU tensor"):
        fused_ssim(torch.zeros(1, 1, 8, 8), torch.zeros(1, 1, 8, 8))
    with pytest.raises(_lib.CurveGSError, match="GPU tensor"):
        sample_curves(torch.zeros(2, 4, 3), torch.zeros(2, 1))
    with pytest.raises(_lib.CurveGSError, match="GPU tensor"):
        distCUDA2(torch.zeros(5, 3))
    e = torch.empty(0)
    with pytest.raises(RuntimeError, match="means3D must have dimensions"):
        _C.rasterize_gaussians(torch.zeros(3), torch.zeros(4), e, e, e, e, 1.0, e, e, torch.eye(4), torch.eye(4), 0.5, 0.5, 8, 8, e, 0,
                               torch.zeros(3), False, False, True, False)


def test_sampling_coefficients_match_reference_expressions():
    from curve_gaussian_amd.ops.curve_sampling import sample_coefficients
    from oracle import torch_ref as TR
    m = 12
    c = sample_coefficients(m, "cpu")
    t = TR.sample_t(m)[:, 0, 0]
    assert torch.equal(c[:, 0], (1 - t) ** 3) and torch.equal(c[:, 9], 6 * (1 - t) * t)
    assert torch.allclose(c[:, :4].sum(1), torch.ones(m), atol=1e-6)
    assert torch.equal(c[:, 13], 1 - (t - 0.5 / m))
