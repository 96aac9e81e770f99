"""The extraction step's edge-map visibility check (edge_extraction/extract_para_edge.py:21-57, 145-257 of the
reference): which fitted curves and lines the 2D edge detector actually saw.

``get_edge_maps`` reads a scan's edge maps on the host as raw 8-bit values; ``compute_visibility`` counts, in the HIP
kernel ``cgs_edge_visibility``, the frames in which every edge is seen and applies the reference's thresholds;
``get_parametric_edge`` is the reference's entry point of the same name, with its signature and return value.

The depth gate (opt-in; ``ops.edge_occlusion``): ``edge_visibility_counts_depth`` / ``compute_visibility_depth``
drop a control or end point that a frame's depth plane hides before the frame's cell is formed (``cgs_edge_visibility_depth``,
or numpy written operation for operation with ``backend="host"``: the two agree bit for bit), ``scan_visibility_counts_depth``
builds a scan's planes a chunk of frames at a time, and ``get_parametric_edge`` takes ``occluder`` / ``depth_maps``.  Without
them nothing changes.  ``DEPTH_WINDOW`` AND ``DEPTH_SLACK`` ARE UNTUNED: only the drawn solids of scene/solid_scan.py have
been checked, no real scan."""
import json
import math
import os

import numpy as np
import torch

from .. import _lib as L
from ..ops import edge_occlusion as EO
from ..ops import edge_score as ES
from ..ops.view_chunks import check_budget, view_chunks
from ..scene.dataset_io import DETECTOR_DIRS, sample_edge_points

# The reference's hard-coded thresholds (extract_para_edge.py:189-192, 212-214)
EDGE_VISIBILITY_THRESHOLD = 0.1      # mean of the edge-map values at the projected points
EDGE_MAX_THRESHOLD = 0.5             # max of the same values
EDGE_VISIBILITY_FRAMES_RATIO = 0.05  # an edge is kept if seen in more than ceil(0.05 * frames) frames

VISIBILITY_BYTE_BUDGET = 1 << 30     # bytes of maps and depth planes per chunk of frames of the gated check

# Image modes converted to 8-bit grayscale when a map is not already one (see get_edge_maps)
_CONVERTIBLE_MODES = ("1", "P", "LA", "RGB", "RGBA")


def edge_visibility_frames(n_frames):
    """extract_para_edge.py:215-217: the number of frames an edge must be seen in MORE than."""
    return math.ceil(EDGE_VISIBILITY_FRAMES_RATIO * n_frames)


def edge_map_paths(scan_dir, detector):
    """The edge-map file of every frame of ``meta_data.json``, by the extraction step's rules (get_edge_maps :27-45):
    DexiNed maps are ``edge_DexiNed/<rgb_path>``, PidiNet maps ``edge_PidiNet/<rgb_path[:-4]>.png`` (training's
    read_emap takes rgb_path verbatim for both).  Returns (meta, paths); an unknown detector raises ValueError."""
    with open(os.path.join(scan_dir, "meta_data.json"), encoding="UTF-8") as f:
        meta = json.load(f)
    if detector == "DexiNed":
        paths = [os.path.join(scan_dir, DETECTOR_DIRS[detector], fr["rgb_path"]) for fr in meta["frames"]]
    elif detector == "PidiNet":
        paths = [os.path.join(scan_dir, DETECTOR_DIRS[detector], fr["rgb_path"][:-4] + ".png") for fr in meta["frames"]]
    else:
        raise ValueError(f"Unknown detector: {detector}")
    return meta, paths


def read_edge_map_u8(path):
    """One edge map as uint8 [H,W]: an 8-bit grayscale (mode "L") PNG gives its stored values, as cv2.imread(path, 0)
    does.  Other images (the reference decodes them with OpenCV, which is not available here) are converted with PIL's
    ``convert("L")``, L = (299 R + 587 G + 114 B) / 1000 rounded, alpha and palette resolved first: UNPINNED against
    the reference.  Modes with more than 8 bits per channel raise ValueError."""
    from PIL import Image
    if not os.path.isfile(path):
        raise FileNotFoundError(f"edge map not found: {path}")
    with Image.open(path) as img:
        if img.mode != "L":
            if img.mode not in _CONVERTIBLE_MODES:
                raise ValueError(f"edge map {path}: unsupported image mode {img.mode!r}")
            img = img.convert("L")
        return np.array(img, dtype=np.uint8)


def get_edge_maps(scan_dir, detector):
    """extract_para_edge.py:21-57 without the float conversion: (maps uint8 [F,H,W], intrinsics [F,..], camtoworld
    [F,4,4], h, w), with h, w the meta's ``height`` / ``width``.  The kernel turns a gathered byte u into the
    reference's value, 1 - u/255.0 (DexiNed) or u/255.0 (PidiNet).  Raises ValueError for an unknown detector, a scan
    without frames and a map whose size is not (h, w); FileNotFoundError, naming the path, for a missing map."""
    meta, paths = edge_map_paths(scan_dir, detector)
    h, w = int(meta["height"]), int(meta["width"])
    if not paths:
        raise ValueError(f"scan {scan_dir} has no frames in meta_data.json")
    maps = np.empty((len(paths), h, w), dtype=np.uint8)
    for i, p in enumerate(paths):
        m = read_edge_map_u8(p)
        if m.shape != (h, w):
            raise ValueError(f"edge map {p} is {m.shape[0]}x{m.shape[1]}, meta_data.json says {h}x{w}")
        maps[i] = m
    intrinsics = np.stack([np.array(fr["intrinsics"]) for fr in meta["frames"]])
    camtoworld = np.stack([np.array(fr["camtoworld"])[:4, :4] for fr in meta["frames"]])
    return maps, intrinsics, camtoworld, h, w


def _host64(x):
    if isinstance(x, torch.Tensor):
        x = x.detach().cpu().numpy()
    return np.asarray(x, dtype=np.float64)


def edge_visibility_counts(curves, lines, maps_u8, intrinsics, camtoworld, detector):
    """Per edge (curves first, then lines), the number of frames in which it is seen (``cgs_edge_visibility``):
    int32 [Nc + Nl] on the maps' device.  curves [Nc,4,3] (or [Nc,12]), lines [Nl,2,3] (or [Nl,6]) and maps_u8 uint8
    [F,H,W] are GPU tensors on one device; intrinsics [F,>=3,>=3] and camtoworld [F,4,4] are host arrays (or tensors):
    K = intrinsics[:3,:3] and w2c = np.linalg.inv(camtoworld) are formed on the host, frame by frame, as the
    reference does (:173-176)."""
    if detector == "DexiNed":
        invert = 1
    elif detector == "PidiNet":
        invert = 0
    else:
        raise ValueError(f"Unknown detector: {detector}")
    for t, name in ((curves, "curves"), (lines, "lines"), (maps_u8, "maps_u8")):
        L.require_gpu_tensor(t, name)
    dev = maps_u8.device
    for t, name in ((curves, "curves"), (lines, "lines"), (intrinsics, "intrinsics"), (camtoworld, "camtoworld")):
        if isinstance(t, torch.Tensor) and t.device != dev:
            raise L.CurveGSError(f"{name} is on {t.device}, maps_u8 on {dev}: all tensors must be on one device")
    if maps_u8.dtype != torch.uint8 or maps_u8.dim() != 3:
        raise L.CurveGSError(f"maps_u8 must be uint8 [F,H,W] (got {maps_u8.dtype} {tuple(maps_u8.shape)})")
    F, H, W = (int(s) for s in maps_u8.shape)
    K = _host64(intrinsics)
    c2w = _host64(camtoworld)
    if K.shape[0] != F or c2w.shape[0] != F or K.shape[1] < 3 or K.shape[2] < 3 or c2w.shape[1:] != (4, 4):
        raise L.CurveGSError(f"intrinsics / camtoworld must be [F,3+,3+] / [F,4,4] with F = {F} "
                             f"(got {K.shape}, {c2w.shape})")
    K = np.ascontiguousarray(K[:, :3, :3])
    w2c = np.stack([np.linalg.inv(c2w[f])[:3, :4] for f in range(F)]) if F else np.zeros((0, 3, 4))
    lib = L.load()
    with L.device_guard(dev):
        c = curves.to(torch.float64).reshape(-1, 12).contiguous()
        ln = lines.to(torch.float64).reshape(-1, 6).contiguous()
        maps = maps_u8.contiguous()
        nc, nl = c.shape[0], ln.shape[0]
        counts = torch.empty((nc + nl,), dtype=torch.int32, device=dev)
        if nc + nl > 0:
            Kd = torch.from_numpy(K).to(dev)
            Md = torch.from_numpy(np.ascontiguousarray(w2c)).to(dev)
            rc = lib.cgs_edge_visibility(nc, L.ptr(c), nl, L.ptr(ln), F, L.ptr(Kd), L.ptr(Md), H, W, L.ptr(maps),
                                         invert, L.ptr(counts), L.raw_stream(dev))
            L.check(rc, "cgs_edge_visibility")
    return counts


def compute_visibility(curves, lines, maps_u8, intrinsics, camtoworld, detector):
    """extract_para_edge.py:145-197 on the GPU, with the thresholds of get_parametric_edge: an edge is visible in a
    frame if the edge-map values at its projected control / end points have mean > 0.1 and max > 0.5, and it is kept
    if it is visible in more than ceil(0.05 * F) frames.  Arguments as edge_visibility_counts.  Returns
    (curve_mask bool [Nc], line_mask bool [Nl]) on the maps' device."""
    counts = edge_visibility_counts(curves, lines, maps_u8, intrinsics, camtoworld, detector)
    keep = counts > edge_visibility_frames(int(maps_u8.shape[0]))
    nc = int(curves.reshape(-1, 12).shape[0])
    return keep[:nc], keep[nc:]


# ------------------------------------------------------------------------------------------------ the depth gate
def _invert_of(detector):
    if detector == "DexiNed":
        return 1
    if detector == "PidiNet":
        return 0
    raise ValueError(f"Unknown detector: {detector}")


def _frame_cells_host(pts, valid, K, M, emap, invert, plane, slack):
    """One frame of ``cgs_edge_visibility_depth`` in numpy, operation for operation: (visible bool [E], touched bool [E]).
    pts float64 [E,4,3] (a line's slots 2 and 3 are not ``valid``); K [3,3], M [3,4]; emap uint8 [H,W]; plane float32 [H,W]."""
    H, W = emap.shape
    X, Y, Z = pts[..., 0], pts[..., 1], pts[..., 2]
    with np.errstate(all="ignore"):
        c0 = ((M[0, 0] * X + M[0, 1] * Y) + M[0, 2] * Z) + M[0, 3]
        c1 = ((M[1, 0] * X + M[1, 1] * Y) + M[1, 2] * Z) + M[1, 3]
        c2 = ((M[2, 0] * X + M[2, 1] * Y) + M[2, 2] * Z) + M[2, 3]
        x0 = (K[0, 0] * c0 + K[0, 1] * c1) + K[0, 2] * c2
        x1 = (K[1, 0] * c0 + K[1, 1] * c1) + K[1, 2] * c2
        x2 = (K[2, 0] * c0 + K[2, 1] * c1) + K[2, 2] * c2
        ur, vr = x0 / x2, x1 / x2
        u, v = np.rint(ur), np.rint(vr)
        keep = valid & (u >= 0.0) & (u < float(W)) & (v >= 0.0) & (v < float(H))   # NaN and +-inf fail
        gate = keep & (ur >= 0.0) & (vr >= 0.0)   # a point kept by rounding from [-0.5, 0) has no plane pixel
    hid = EO.hidden_host(c2.ravel(), ur.ravel(), vr.ravel(), gate.ravel(), plane, slack).reshape(keep.shape)
    vis = keep & ~hid
    raw = np.zeros(keep.shape, np.float64)
    raw[vis] = emap[v[vis].astype(np.int64), u[vis].astype(np.int64)] / 255.0
    val = np.where(vis, 1.0 - raw if invert else raw, 0.0)   # x + 0.0 == x: a dropped point adds nothing
    total = ((val[:, 0] + val[:, 1]) + val[:, 2]) + val[:, 3]
    nv = vis.sum(1)
    mx = np.where(vis, val, -np.inf).max(1)
    with np.errstate(all="ignore"):
        cell = (nv > 0) & (total / nv > EDGE_VISIBILITY_THRESHOLD) & (mx > EDGE_MAX_THRESHOLD)
    return cell, hid.any(1)


def edge_visibility_counts_depth(curves, lines, maps_u8, intrinsics, camtoworld, detector, depth, slack=EO.DEPTH_SLACK,
                                 backend="gpu", device=None):
    """``edge_visibility_counts`` with the depth gate: int32 [Nc + Nl, 2] -- [:, 0] the frames in which the edge is seen,
    [:, 1] the frames in which the gate dropped at least one of its points.  ``depth``: float32 [F,H,W], camera z per frame,
    +inf where there is no surface; a control or end point that the check keeps (its ROUNDED pixel is in the image) is dropped,
    exactly as an out-of-image point is, iff its raw coordinates (u, v) = (x0 / x2, x1 / x2) are >= 0 and its camera depth c2
    (the third row of w2c X) has c2 > float64(depth[f][floor(v)][floor(u)]) + slack (``nv_hidden``).  The edge map is still
    read at the rounded pixel.  With an all-+inf depth [:, 0] is ``edge_visibility_counts`` and [:, 1] is 0.
    ``backend="gpu"``: ``cgs_edge_visibility_depth``; arrays and CPU tensors are uploaded, the result stays on the device.
    ``"host"``: numpy written operation for operation, a CPU tensor; the two agree bit for bit."""
    ES._check_backend(backend)
    invert = _invert_of(detector)
    maps = maps_u8 if torch.is_tensor(maps_u8) else torch.from_numpy(np.ascontiguousarray(maps_u8))
    if maps.dtype != torch.uint8 or maps.dim() != 3:
        raise ValueError(f"maps_u8 must be uint8 [F,H,W] (got {maps.dtype} {tuple(maps.shape)})")
    F, H, W = (int(s) for s in maps.shape)
    K = _host64(intrinsics)
    c2w = _host64(camtoworld)
    if K.ndim != 3 or c2w.ndim != 3 or K.shape[0] != F or c2w.shape[0] != F or K.shape[1] < 3 or K.shape[2] < 3 \
            or c2w.shape[1:] != (4, 4):
        raise ValueError(f"intrinsics / camtoworld must be [F,3+,3+] / [F,4,4] with F = {F} (got {K.shape}, {c2w.shape})")
    K = np.ascontiguousarray(K[:, :3, :3])
    w2c = np.stack([np.linalg.inv(c2w[f])[:3, :4] for f in range(F)]) if F else np.zeros((0, 3, 4))
    c = torch.as_tensor(curves).detach().to(torch.float64).reshape(-1, 12)
    ln = torch.as_tensor(lines).detach().to(torch.float64).reshape(-1, 6)
    nc, nl = int(c.shape[0]), int(ln.shape[0])
    what = "edge_visibility_counts_depth"
    if backend == "host":
        d, slack = EO.operator_depth(what, depth, slack, F, H, W, "host")
        pts = np.zeros((nc + nl, 4, 3), np.float64)
        pts[:nc] = ES._host(c).reshape(nc, 4, 3)
        pts[nc:, :2] = ES._host(ln).reshape(nl, 2, 3)
        valid = np.ones((nc + nl, 4), bool)
        valid[nc:, 2:] = False
        emaps = ES._host(maps)
        counts = np.zeros((nc + nl, 2), np.int32)
        for f in range(F):
            cell, touched = _frame_cells_host(pts, valid, K[f], w2c[f], emaps[f], invert, d[f], slack)
            counts[:, 0] += cell
            counts[:, 1] += touched
        return torch.from_numpy(counts)
    dev = ES._device_for([maps, c, ln] + ([depth] if torch.is_tensor(depth) else []), what, device)
    d, slack = EO.operator_depth(what, depth, slack, F, H, W, "gpu", dev)
    with L.device_guard(dev):
        c, ln, maps = c.to(dev).contiguous(), ln.to(dev).contiguous(), maps.to(dev).contiguous()
        counts = torch.zeros((nc + nl, 2), dtype=torch.int32, device=dev)
        if nc + nl > 0:
            Kd = torch.from_numpy(K).to(dev)
            Md = torch.from_numpy(np.ascontiguousarray(w2c)).to(dev)
            rc = L.load().cgs_edge_visibility_depth(nc, L.ptr(c), nl, L.ptr(ln), F, L.ptr(Kd), L.ptr(Md), H, W, L.ptr(maps),
                                                    invert, L.ptr(d), slack, L.ptr(counts), L.raw_stream(dev))
            L.check(rc, "cgs_edge_visibility_depth")
    return counts


def compute_visibility_depth(curves, lines, maps_u8, intrinsics, camtoworld, detector, depth, slack=EO.DEPTH_SLACK,
                             backend="gpu", device=None, return_counts=False):
    """``compute_visibility`` with the depth gate, the reference's thresholds unchanged: an edge is kept if it is visible in
    more than ceil(0.05 * F) frames, a frame's cell being formed from the points that ``depth`` does not hide.  Arguments as
    ``edge_visibility_counts_depth``.  Returns (curve_mask bool [Nc], line_mask bool [Nl]) and, with return_counts, the
    int32 [Nc + Nl, 2] counts."""
    counts = edge_visibility_counts_depth(curves, lines, maps_u8, intrinsics, camtoworld, detector, depth, slack, backend,
                                          device)
    keep = counts[:, 0] > edge_visibility_frames(int(maps_u8.shape[0]))
    nc = int(torch.as_tensor(curves).reshape(-1, 12).shape[0])
    return (keep[:nc], keep[nc:], counts) if return_counts else (keep[:nc], keep[nc:])


def check_pinhole_intrinsics(what, intrinsics):
    """The planes of an occluder are drawn by a pinhole camera (fx, fy, cx, cy) = (K00, K11, K02, K12): ValueError for a K
    with K01, K10, K20 or K21 nonzero, or K22 != 1, whose image those planes are not in."""
    for f, K in enumerate(np.asarray(intrinsics, np.float64)):
        if K[0, 1] != 0.0 or K[1, 0] != 0.0 or K[2, 0] != 0.0 or K[2, 1] != 0.0 or K[2, 2] != 1.0:
            raise ValueError(f"{what}: the intrinsics of frame {f} are not a pinhole camera's (K01, K10, K20, K21 must be 0 "
                             f"and K22 1; got {K[:3, :3].tolist()}): an occluder's depth planes are drawn for "
                             "(fx, fy, cx, cy) only; give depth_maps in this K's image instead")


def scan_visibility_counts_depth(curves, lines, scan_dir, detector, occluder=None, depth_maps=None,
                                 depth_slack=EO.DEPTH_SLACK, depth_window=EO.DEPTH_WINDOW, near_clip=None, backend="gpu",
                                 device=None, budget_bytes=None):
    """The gated counts of a whole EMAP scan: (int32 [Nc + Nl, 2] numpy array, the number of frames).  The cameras and maps
    come from ``reprojection.emap_cameras``, the planes from ``ops.edge_occlusion.ChunkDepth`` over ``view_chunks`` -- a chunk
    of frames at a time, ``budget_bytes`` (default VISIBILITY_BYTE_BUDGET) of maps and planes -- and the chunks' integer
    counts are added, so the result does not depend on the chunking.  One of ``occluder`` (triangles or a mesh file's path;
    the intrinsics must then be a pinhole camera's, ``check_pinhole_intrinsics``) and ``depth_maps`` (one float [H,W] array
    per frame, in K's image; K is not restricted) is required; ``near_clip`` needs the occluder."""
    from .reprojection import emap_cameras   # (reprojection imports this module)
    what = "get_parametric_edge"
    ES._check_backend(backend)
    EO.check_one_depth_source(what, occluder, depth_maps)
    if occluder is None and depth_maps is None:
        raise ValueError(f"{what}: the gated check needs an occluder or depth_maps")
    if near_clip is not None and occluder is None:
        raise ValueError(f"{what}: near_clip needs an occluder (the caller's depth maps need no clipping)")
    budget = check_budget(what, budget_bytes, VISIBILITY_BYTE_BUDGET)
    cams, maps = emap_cameras(scan_dir, detector)   # (a scan without frames raises here)
    meta, _ = edge_map_paths(scan_dir, detector)
    intrinsics = np.stack([np.array(fr["intrinsics"], np.float64) for fr in meta["frames"]])
    camtoworld = np.stack([np.array(fr["camtoworld"], np.float64)[:4, :4] for fr in meta["frames"]])
    if occluder is not None:
        check_pinhole_intrinsics(what, intrinsics)
    gate = EO.ChunkDepth(what, cams, occluder, depth_maps, depth_slack, depth_window, near_clip)
    if backend == "gpu":
        device = ES._device_for([], what, device)
    gate.to(backend, device)
    c = np.asarray(curves, np.float64).reshape(-1, 12)
    ln = np.asarray(lines, np.float64).reshape(-1, 6)
    if backend == "gpu":
        c, ln = torch.from_numpy(c).to(device), torch.from_numpy(ln).to(device)
    counts = np.zeros((c.shape[0] + ln.shape[0], 2), np.int32)
    for H, W, sel, intr, w2c in view_chunks(cams, gate.bytes_per_pixel + 1, budget):   # + 1: the map's byte
        planes = gate.planes(H, W, sel, intr, w2c)
        counts += edge_visibility_counts_depth(c, ln, maps[sel], intrinsics[sel], camtoworld[sel], detector, planes,
                                               gate.slack, backend, device).cpu().numpy()
    return counts, len(cams)


def _edge_arrays(edge_dict):
    curves = np.array(edge_dict["curves_ctl_pts"]).reshape(-1, 12).reshape(-1, 4, 3)
    lines = np.array(edge_dict["lines_end_pts"]).reshape(-1, 6)
    return curves, lines


def get_parametric_edge(visible_checking, merged_edge_dict, meta_data_dir=None, detector=None, *, occluder=None,
                        depth_maps=None, depth_slack=EO.DEPTH_SLACK, depth_window=EO.DEPTH_WINDOW, near_clip=None,
                        backend="gpu"):
    """extract_para_edge.py:200-257: (pred_points float32 [N,3], return_edge_dict) with return_edge_dict =
    {"curves_ctl_pts": [n,4,3], "lines_end_pts": [n,6]} and the points sampled every 5 mm along its edges.  With
    visible_checking=True only the edges that compute_visibility keeps are returned (maps of `detector` read from
    `meta_data_dir`, the check on the current GPU) and the reference's "before / after visible checking" counts are
    printed; meta_data_dir is then required (the reference's train.py never passes it).

    The depth gate (keyword arguments only; opt-in, UNTUNED, drawn solids only): with ``occluder`` -- float32 [F,3,3]
    triangles or the path of an .obj / .ply mesh -- or ``depth_maps`` -- one float [H,W] array of camera z per frame -- the
    check is ``scan_visibility_counts_depth``: a control or end point hidden behind the frame's depth plane (window maximum
    of radius ``depth_window``, ``depth_slack`` world units behind the surface) is dropped before the frame's cell is formed,
    so an edge inside a solid no longer reads whatever detected pixel it lands on.  ``near_clip`` as ``mesh_depth`` (with an
    occluder only).  A line more is printed: the (edge, frame) cells in which the gate dropped a point.  ``backend="host"``
    runs the gated check in numpy (the same counts to the bit).  Without a depth source nothing changes: the ungated check
    has no host back end and nothing to clip, so ``backend="host"`` and ``near_clip`` are then ValueErrors."""
    curves, lines = _edge_arrays(merged_edge_dict)
    EO.check_one_depth_source("get_parametric_edge", occluder, depth_maps)
    gated = occluder is not None or depth_maps is not None
    if near_clip is not None and occluder is None:
        raise ValueError("get_parametric_edge: near_clip needs an occluder (the caller's depth maps need no clipping)")
    if not gated and backend != "gpu":
        raise ValueError("get_parametric_edge: without a depth source the check runs on the GPU only (backend='gpu')")
    if gated and not visible_checking:
        raise ValueError("get_parametric_edge: a depth source gates the visibility check; it needs visible_checking=True")
    if visible_checking and meta_data_dir is None:
        raise ValueError("get_parametric_edge(visible_checking=True) needs meta_data_dir, the scan directory "
                         "holding meta_data.json and the edge maps")
    if visible_checking and gated:
        counts, n_frames = scan_visibility_counts_depth(curves, lines, meta_data_dir, detector, occluder, depth_maps,
                                                        depth_slack, depth_window, near_clip, backend)
        keep = counts[:, 0] > edge_visibility_frames(n_frames)
        cm, lm = keep[:len(curves)], keep[len(curves):]
        print("before visible checking: ", len(curves) + len(lines), "after visible checking: ",
              int(cm.sum()) + int(lm.sum()))
        print("depth gate: dropped a point in", int(counts[:, 1].sum()), "of", len(keep) * n_frames, "(edge, frame) cells")
        curves, lines = curves[cm], lines[lm]
    elif visible_checking:
        maps, intrinsics, camtoworld, _, _ = get_edge_maps(meta_data_dir, detector)
        dev = torch.device("cuda", torch.cuda.current_device())
        cm, lm = compute_visibility(torch.from_numpy(curves).to(dev), torch.from_numpy(lines).to(dev),
                                    torch.from_numpy(maps).to(dev), intrinsics, camtoworld, detector)
        cm, lm = cm.cpu().numpy(), lm.cpu().numpy()
        print("before visible checking: ", len(curves) + len(lines), "after visible checking: ",
              int(cm.sum()) + int(lm.sum()))
        curves, lines = curves[cm], lines[lm]
    return sample_edge_points(curves, lines), {"curves_ctl_pts": curves.tolist(), "lines_end_pts": lines.tolist()}
