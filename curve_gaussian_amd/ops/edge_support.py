"""Per-edge 2D support of extracted edges: every edge checked ALONG ITS LENGTH against the detected edge pixels of every
view (cgs_edge_support, include/curvegs.h; csrc/edge_support.hip).  The reference's visibility check
(``get_parametric_edge(visible_checking=True)``, cgs_edge_visibility) looks at a Bezier curve's four control points -- two
of which do not lie on the curve -- or at a line's two end points, so a chord that merely starts and ends on real edges
passes it; the reprojection score (ops/edge_score.py) is one number per scan and cannot say which edge is wrong.  The
reference has no counterpart.

  sample_edges     the samples of every edge by the per-edge rule of ``dataset_io.sample_edge_points`` (curves first,
                   then lines) and the range of points each edge owns
  support_counts   int32 [E,V,1+T]: per (edge, view) the samples the projection rule of ``cgs_project_points`` keeps
                   (float32 points, float64 arithmetic, to the letter) and, per tolerance, those of them whose pixel
                   (floor(u), floor(v)) lies within the tolerance of a detected pixel (``edt_squared`` of the detected mask)
  support_verdict  host integers: which views see an edge, which support it, and which edges enough views support
  edge_support     the three on a scan's cameras and stored edge maps

The verdict, frozen; n = the number of samples of edge e, seen / near = counts[e,v,0] / counts[e,v,1+t]:
  view v SEES edge e          iff n > 0 and seen >= ceil(min_visible * n)
  view v SUPPORTS e at t      iff it sees it and near >= ceil(min_near * seen)
  edge e is KEPT at t         iff its supporting views number MORE than ceil(frames_ratio * frames)
                              (the reference's frame rule, ``para_edge.edge_visibility_frames``)
  share[e][t]                 = sum_v near / sum_v seen over all views, NaN when nothing is seen (reported, not used)
The thresholds are built in float64 on the host, as ``edge_seed.need_table`` builds them.

DEPTH (opt-in).  Without a depth source an edge hidden behind a surface in most views loses its support
there, which is why the rule counts supporting FRAMES and does not pool the samples of all views -- and a hidden edge
collects support it cannot have from the front edges it projects behind.  With ``depth`` (``support_counts``) or
``occluder`` / ``depth_maps`` (``edge_support``) a (sample, view) pair that the view's depth plane hides -- the one rule of
ops/edge_occlusion.py, ``nv_hidden`` -- counts as NOT SEEN and is tallied in "hidden" instead.  The verdict's formulas do
not change, only their inputs: a view whose VISIBLE samples number fewer than ceil(min_visible * n) does not see the edge.
The gate's limits are those of ops/edge_occlusion.py: untuned window and slack, checked on the drawn solids of
scene/solid_scan.py only; a concave edge can be hidden by its own faces; no near-plane clipping unless ``near_clip`` is given.

KNOWN LIMITS.  A thick detector response inflates support: a
chord across a wide response lies "on" it (``thin=True`` thins the detected masks first: ops/edge_thin.py, DESIGN.md 4.8n;
untuned, checked on dilated drawn maps only).  THE DEFAULTS OF ``edge_support`` ARE UNTUNED: one run on the drawn test scan
(tests/edge_support_cases.py), no real scan.

Two back ends: ``"gpu"``, HIP, and ``"host"``, numpy -- the same rules in integers, so the counts agree exactly."""
import math

import numpy as np
import torch

from .. import _lib as L
from ..edge_extraction.para_edge import EDGE_MAX_THRESHOLD, EDGE_VISIBILITY_FRAMES_RATIO
from ..edge_extraction.reprojection import SAMPLE_RESOLUTION
from ..scene.dataset_io import bezier_curve_length
from . import edge_occlusion as EO
from . import edge_score as ES
from .edge_thin import thin_masks
from .view_chunks import check_budget, check_edge_maps, detected_lut, detected_masks, view_chunks

SUPPORT_BACKENDS = ES.SCORE_BACKENDS
MAX_TOL = L.EDGE_SUPPORT_MAX_TOL
BYTE_BUDGET = ES.BYTE_BUDGET   # bytes of masks, transforms and scratch per chunk of views in edge_support
BYTES_PER_PIXEL = 7            # one uint8 mask, one uint16 column pass, one int32 transform
# UNTUNED, like the defaults of ops/edge_seed.py: one run on the drawn test scan, no real scan
TOLERANCES_PX = (1, 2, 4)
KEEP_TOLERANCE_PX = 2
MIN_VISIBLE = 0.5
MIN_NEAR = 0.8

_BEZIER = np.array([[-1, 3, -3, 1], [3, -6, 3, 0], [-3, 3, 0, 0], [1, 0, 0, 0]], dtype=np.float64)


def _edge_arrays(curves, lines):
    return (np.asarray(curves, dtype=np.float64).reshape(-1, 4, 3), np.asarray(lines, dtype=np.float64).reshape(-1, 2, 3))


# ------------------------------------------------------------------------------------------------ samples
def sample_edges(curves, lines, resolution):
    """(points float32 [P,3], offsets int32 [E+1]) of the curves ([Nc,4,3] or [Nc,12]) and then the lines ([Nl,2,3] or
    [Nl,6]): edge e owns points[offsets[e]:offsets[e+1]].  The per-edge rule of ``dataset_io.sample_edge_points``, operation
    for operation -- ``int(length // resolution)`` samples at ``np.linspace(0, 1, n)``, the same Bezier matrix form -- so
    ``points`` equals its result exactly; an edge shorter than ``resolution`` has no points."""
    curves, lines = _edge_arrays(curves, lines)
    parts, sizes = [], []
    for curve in curves:
        n = int(bezier_curve_length(curve, 100) // resolution)
        t = np.linspace(0, 1, n)
        U = np.array([t ** 3, t ** 2, t, np.ones_like(t)])
        parts.append(U.T.dot(_BEZIER).dot(curve))
        sizes.append(n)
    for line in lines:
        n = int(np.linalg.norm(line[0] - line[1]) // resolution)
        t = np.linspace(0, 1, n)
        parts.append(np.outer(t, line[1] - line[0]) + line[0])
        sizes.append(n)
    total = int(sum(sizes))
    if total > np.iinfo(np.int32).max:
        raise ValueError(f"sample_edges: {total} samples: at most 2^31 - 1 (raise the resolution)")
    pts = np.concatenate(parts).astype(np.float32) if parts else np.zeros((0, 3), np.float32)
    offsets = np.zeros(len(sizes) + 1, np.int32)
    offsets[1:] = np.cumsum(np.asarray(sizes, np.int64))
    return pts.reshape(-1, 3), offsets


# ------------------------------------------------------------------------------------------------ counts
def _check_backend(backend):
    if backend not in SUPPORT_BACKENDS:
        raise ValueError(f"unknown edge support backend {backend!r}: expected one of {SUPPORT_BACKENDS}")


def _tolerances(tolerances_px):
    tol2 = ES.tolerances_squared(tolerances_px)
    if not (1 <= len(tol2) <= MAX_TOL):
        raise ValueError(f"between 1 and {MAX_TOL} tolerances (got {len(tol2)})")
    return tol2


def _points(points):
    """float32 [P,3], as given: a tensor (any device) or an array.  Another dtype is an error -- the float32 point is what
    is projected, and rounding it here would hide from the caller which point that is."""
    dtype = points.dtype if torch.is_tensor(points) else np.asarray(points).dtype
    if dtype not in (torch.float32, np.float32):
        raise ValueError(f"points must be float32 (got {dtype})")
    pts = points.detach() if torch.is_tensor(points) else torch.from_numpy(np.ascontiguousarray(points))
    if pts.dim() != 2 or pts.shape[1] != 3:
        raise ValueError(f"points must be [P,3] (got {tuple(pts.shape)})")
    return pts


def _offsets(offsets, P):
    """int32 [E+1] on the host, checked: integers, non-decreasing, offsets[0] = 0, offsets[E] = P."""
    off = ES._host(offsets)
    if off.ndim != 1 or off.size < 1 or not np.issubdtype(off.dtype, np.integer):
        raise ValueError(f"offsets must be an integer [E+1] array (got {off.dtype} {off.shape})")
    off = off.astype(np.int64)
    if off[0] != 0 or off[-1] != P or (np.diff(off) < 0).any():
        raise ValueError(f"offsets must be non-decreasing from 0 to the number of points, {P} (got {off[0]} .. {off[-1]})")
    return np.ascontiguousarray(off.astype(np.int32))


def _d2(d2, V):
    dtype = d2.dtype if torch.is_tensor(d2) else np.asarray(d2).dtype
    if dtype not in (torch.int32, np.int32):
        raise ValueError(f"d2 must be int32, the result of edt_squared (got {dtype})")
    t = d2.detach() if torch.is_tensor(d2) else torch.from_numpy(np.ascontiguousarray(d2))
    if t.dim() != 3 or t.shape[0] != V:
        raise ValueError(f"d2 must be [V,H,W] with V = {V} cameras (got {tuple(t.shape)})")
    if V > 0:
        ES._check_size("support_counts: d2", t.shape[1], t.shape[2])
    return t.contiguous()


def _host_only(who, *tensors):
    """``backend="host"``: none of the tensors (None: not given) may be on a GPU."""
    if any(t is not None and t.is_cuda for t in tensors):
        raise ValueError(f"{who}: backend='host' takes host arrays and CPU tensors")


def _one_device(who, anchor_name, anchor, device, uploaded=(), resident=()):
    """``backend="gpu"``: the device of the call, which is the anchor's (d2 or near; CurveGSError unless it is on a GPU).
    ``device``, when given, must be it.  So must the device of every (name, tensor) of ``uploaded`` that is on a GPU -- one
    on the host is the caller's to upload -- and of every (name, tensors) of ``resident``, the outputs (None: not given)."""
    L.require_gpu_tensor(anchor, f"{who}: {anchor_name}")
    dev = anchor.device
    if device is not None and torch.device(device) != dev and torch.device(device) != torch.device(dev.type):
        raise L.CurveGSError(f"{who}: {anchor_name} is on {dev}, device={device}: all tensors must be on one device")
    for name, t in uploaded:
        if t.is_cuda and t.device != dev:
            raise L.CurveGSError(f"{who}: {name} are on {t.device}, {anchor_name} on {dev}: all tensors must be on one device")
    for name, tensors in resident:
        devices = [t.device for t in tensors if t is not None]
        if any(d != dev for d in devices):
            raise L.CurveGSError(f"{who}: {name} is on {' and '.join(map(str, devices))}, {anchor_name} on {dev}: all tensors "
                                 "must be on one device")
    return dev


def _counts_host(pts, off, K, M, d2, tol2, depth=None, slack=0.0, hidden=None):
    """``depth`` float32 [V,H,W] or None; ``hidden`` int32 [E,V] or None, written when there is a depth."""
    E, V, T = off.size - 1, K.shape[0], len(tol2)
    H, W = d2.shape[1], d2.shape[2]
    lo, hi = off[:-1].astype(np.int64), off[1:].astype(np.int64)
    out = np.zeros((E, V, 1 + T), np.int32)
    flags = np.empty((1 + T, pts.shape[0]), np.int64)
    run = np.zeros((1 + T, pts.shape[0] + 1), np.int64)
    for v in range(V):   # one view at a time: [P] temporaries
        if depth is None:
            u, w, keep = (x[0] for x in ES.project_points_host(pts, K[v:v + 1], M[v:v + 1], H, W))
        else:   # a hidden sample counts as not seen
            u, w, keep, hid = EO.gate_view_host(pts, K[v], M[v], depth[v], slack)
            if hidden is not None:
                hrun = np.concatenate([[0], np.cumsum(hid, dtype=np.int64)])
                hidden[:, v] = hrun[hi] - hrun[lo]
        d = np.full(pts.shape[0], ES.EDT_INF, np.int64)
        d[keep] = d2[v][np.floor(w[keep]).astype(np.int64), np.floor(u[keep]).astype(np.int64)]
        flags[0] = keep
        for t, t2 in enumerate(tol2):
            flags[1 + t] = keep & (d <= t2)
        np.cumsum(flags, axis=1, out=run[:, 1:])
        out[:, v, :] = (run[:, hi] - run[:, lo]).T
    return out


def support_counts(points, offsets, intrinsics, w2c, d2, tolerances_px, backend="gpu", device=None, depth=None,
                   slack=EO.DEPTH_SLACK, return_hidden=False):
    """int32 [E,V,1+T].  points float32 [P,3] and offsets int32 [E+1] as ``sample_edges`` gives them; intrinsics [V,4] =
    (fx, fy, cx, cy) and w2c [V,3,4] float64 host arrays or tensors; d2 int32 [V,H,W], ``edt_squared`` of every view's detected
    mask; 1 to 4 pixel tolerances, squared by ``edge_score.tolerances_squared``.  counts[e,v,0] = the points of edge e that
    ``cgs_project_points`` keeps in view v; counts[e,v,1+t] = those of them with d2[v][floor(v)][floor(u)] <= floor(t^2).

    ``backend="gpu"``: ``cgs_edge_support``.  d2 must be on a GPU (``edt_squared`` leaves it there; CurveGSError
    otherwise), ``device``, when given, must be that GPU, and so must the device of points that are on a GPU; points and
    offsets on the host are uploaded.  The result stays on the device.  ``backend="host"``: numpy, a CPU tensor.

    ``depth`` (None: no gate, the call above and nothing else): float32 [V,H,W] of d2's size, camera z, +inf where there is
    no surface.  A sample that view v keeps is HIDDEN there iff c2 > float64(depth[v][floor(v)][floor(u)]) + ``slack``
    (finite, >= 0; ``cgs_edge_support_depth``): it counts as not seen -- in counts[e,v,0] no more than in the near columns.
    ``return_hidden`` (needs ``depth``): also int32 [E,V], the hidden samples of every (edge, view); counts[e,v,0] + hidden[e,v]
    is the ungated counts[e,v,0].  depth on the host is uploaded for ``backend="gpu"``."""
    _check_backend(backend)
    if return_hidden and depth is None:
        raise ValueError("support_counts: return_hidden needs depth")
    tol2 = _tolerances(tolerances_px)
    pts = _points(points)
    off = _offsets(offsets, int(pts.shape[0]))
    V, K, M = ES._cameras(intrinsics, w2c)
    d2 = _d2(d2, V)
    E, T = off.size - 1, len(tol2)
    if backend == "host":
        _host_only("support_counts", d2, pts)
        hidden = None
        if depth is not None:
            depth, slack = EO.operator_depth("support_counts", depth, slack, V, int(d2.shape[1]), int(d2.shape[2]), "host")
            hidden = np.zeros((E, V), np.int32)
        counts = torch.from_numpy(_counts_host(pts.numpy(), off, K, M, d2.numpy(), tol2, depth, slack, hidden))
        return (counts, torch.from_numpy(hidden)) if return_hidden else counts
    dev = _one_device("support_counts", "d2", d2, device, uploaded=[("points", pts)])
    if E * V * (1 + T) > np.iinfo(np.int64).max // 4:
        raise ValueError("support_counts: the counts do not fit")
    with L.device_guard(dev):
        pts = pts.to(dev).contiguous()
        out = torch.empty((E, V, 1 + T), dtype=torch.int32, device=dev)
        if depth is not None:
            depth, slack = EO.operator_depth("support_counts", depth, slack, V, int(d2.shape[1]), int(d2.shape[2]), "gpu", dev)
            hidden = torch.empty((E, V), dtype=torch.int32, device=dev) if return_hidden else None
        if E > 0 and V > 0:
            off_d = torch.from_numpy(off).to(dev)
            tol_d = torch.tensor(tol2, dtype=torch.int32).to(dev)
            Kd, Md = ES.cameras_on(dev, K, M)
            args = [E, int(pts.shape[0]), L.ptr(pts), L.ptr(off_d), V, L.ptr(Kd), L.ptr(Md), int(d2.shape[1]),
                    int(d2.shape[2]), L.ptr(d2), T, L.ptr(tol_d)]
            if depth is None:
                L.check(L.load().cgs_edge_support(*args, L.ptr(out), L.raw_stream(dev)), "cgs_edge_support")
            else:
                L.check(L.load().cgs_edge_support_depth(*args, L.ptr(depth), slack, L.ptr(out), L.ptr(hidden),
                                                        L.raw_stream(dev)), "cgs_edge_support_depth")
    return (out, hidden) if return_hidden else out


# ------------------------------------------------------------------------------------------------ verdict
def _ratio01(name, x):
    x = float(x)
    if not (0.0 <= x <= 1.0):
        raise ValueError(f"{name} must lie in [0, 1] (got {x})")
    return x


def support_verdict(counts, n_points, frames, min_visible=MIN_VISIBLE, min_near=MIN_NEAR,
                    frames_ratio=EDGE_VISIBILITY_FRAMES_RATIO, keep_index=0):
    """The verdict of the module docstring from counts [E,V,1+T] (tensor or array, either back end's) and n_points [E], the
    samples of every edge; ``frames`` is the number of views the frame rule speaks of (V for a whole scan).  Host integers;
    the thresholds ceil(min_visible * n) and ceil(min_near * seen) are formed in float64.  Returns numpy arrays:
    "seeing_views" int64 [E], "supporting_views" int64 [E,T], "share" float64 [E,T] (NaN where no view sees a sample) and
    "kept" bool [E], the verdict at tolerance ``keep_index``."""
    c, n = ES._host(counts).astype(np.int64), ES._host(n_points).astype(np.int64).reshape(-1)
    if c.ndim != 3 or c.shape[2] < 2 or c.shape[0] != n.size:
        raise ValueError(f"counts must be [E,V,1+T] and n_points [E] (got {c.shape}, {n.shape})")
    min_visible, min_near = _ratio01("min_visible", min_visible), _ratio01("min_near", min_near)
    frames_ratio = _ratio01("frames_ratio", frames_ratio)
    T = c.shape[2] - 1
    if not (0 <= int(keep_index) < T):
        raise ValueError(f"keep_index must lie in [0, {T}) (got {keep_index})")
    seen, near = c[:, :, 0], c[:, :, 1:]
    need_seen = np.ceil(min_visible * n.astype(np.float64)).astype(np.int64)
    sees = (n[:, None] > 0) & (seen >= need_seen[:, None])
    need_near = np.ceil(min_near * seen.astype(np.float64)).astype(np.int64)
    supports = sees[:, :, None] & (near >= need_near[:, :, None])
    supporting = supports.sum(1).astype(np.int64)
    total_seen = seen.sum(1)
    with np.errstate(divide="ignore", invalid="ignore"):
        share = np.where(total_seen[:, None] > 0, near.sum(1).astype(np.float64) / total_seen[:, None].astype(np.float64),
                         np.nan)
    kept = supporting[:, int(keep_index)] > math.ceil(frames_ratio * int(frames))
    return {"seeing_views": sees.sum(1).astype(np.int64), "supporting_views": supporting, "share": share, "kept": kept}


# ------------------------------------------------------------------------------------------------ a scan
def edge_support(edge_dict, cameras, edge_maps_u8, detector, resolution=SAMPLE_RESOLUTION, tolerances_px=TOLERANCES_PX,
                 keep_tolerance_px=KEEP_TOLERANCE_PX, min_visible=MIN_VISIBLE, min_near=MIN_NEAR,
                 frames_ratio=EDGE_VISIBILITY_FRAMES_RATIO, edge_threshold=EDGE_MAX_THRESHOLD, backend="gpu", device=None,
                 budget_bytes=None, thin=False, occluder=None, depth_maps=None, depth_slack=EO.DEPTH_SLACK,
                 depth_window=EO.DEPTH_WINDOW, near_clip=None):
    """edge_dict: {"curves_ctl_pts", "lines_end_pts"} (a ``parametric_edges.json``).  cameras: ``NovelViewCamera`` s;
    edge_maps_u8: one uint8 [H,W] map per camera, the stored bytes of the detector's maps, as ``score_edges`` takes them.
    ``resolution``: the sampling step (default: ``reprojection.SAMPLE_RESOLUTION``, the novel views' Replica value); ``keep_tolerance_px``: the one of
    ``tolerances_px`` that decides "kept".

    A pixel is detected when ``reprojection.detected_lut(detector, edge_threshold)`` says so; every view's detected mask
    goes through ``edt_squared``.  Views of one size are processed together, ``budget_bytes`` (default BYTE_BUDGET) of masks
    and transforms at a time (7 bytes per pixel) and at least one view; every (edge, view) cell depends on its view alone,
    so the chunking cannot change a bit.  THE DEFAULTS ARE UNTUNED (one run on the drawn test scan, no real scan), there is
    no depth and a thick detector response inflates support: see the module docstring.  ``thin``: every chunk's detected
    masks go through ``edge_thin.thin_masks`` on the same back end before the transform (2 bytes per pixel, released before
    the transform is allocated; untuned, limits in ops/edge_thin.py); "settings" then holds "thin": True, and nothing
    otherwise.

    Depth (opt-in; at most one of the two, with the meaning and the checks of ``score_edges``): ``occluder`` -- float32
    [F,3,3] triangles or the path of an .obj / .ply mesh -- or ``depth_maps`` -- one float [H,W] array of camera z per
    camera -- give every chunk its depth planes (``edge_occlusion.ChunkDepth``: the window maximum of radius
    ``depth_window``, 8 bytes per pixel more), and ``support_counts`` holds every sample against them with ``depth_slack``: a
    hidden (sample, view) pair counts as not seen.  The verdict's formulas are the frozen ones; only their inputs change, so
    a view whose VISIBLE samples number fewer than ceil(min_visible * n) does not see the edge.  The result then also holds
    "hidden": int32 [E,V] CPU tensor, and "settings" the keys ``score_edges`` records ("occluder" or "depth_maps",
    "depth_slack", "depth_window").  With neither, nothing changes: no key is added.  The window and the slack are untuned and
    checked on the drawn solids only; concave edges can be hidden by their own faces; there is no near-plane clipping unless ``near_clip`` is given (``score_edges``).

    Returns {"counts": int32 [E,V,1+T] CPU tensor, "n_points": int64 [E], "curves": Nc, "lines": Nl, the arrays of
    ``support_verdict`` ("seeing_views", "supporting_views", "share", "kept"), "settings"}; edges are ordered
    curves first, then lines."""
    _check_backend(backend)
    resolution = float(resolution)
    tolerances_px = [float(t) for t in tolerances_px]
    tol2 = _tolerances(tolerances_px)
    if float(keep_tolerance_px) not in tolerances_px:
        raise ValueError(f"edge_support: keep_tolerance_px {keep_tolerance_px} is not one of tolerances_px {tolerances_px}")
    keep_index = tolerances_px.index(float(keep_tolerance_px))
    lut = detected_lut(detector, edge_threshold)
    cameras, maps = check_edge_maps("edge_support", cameras, edge_maps_u8)
    budget = check_budget("edge_support", budget_bytes, BYTE_BUDGET)
    gate = EO.ChunkDepth("edge_support", cameras, occluder, depth_maps, depth_slack, depth_window, near_clip)
    curves, lines = _edge_arrays(edge_dict["curves_ctl_pts"], edge_dict["lines_end_pts"])
    pts, off = sample_edges(curves, lines, resolution)
    E, V, T = off.size - 1, len(cameras), len(tol2)
    if backend == "gpu":
        device = ES._device_for([], "edge_support", device)
        pts_b = torch.from_numpy(pts).to(device)
    else:
        pts_b = pts
    gate.to(backend, device)
    counts = np.zeros((E, V, 1 + T), np.int32)
    hidden = np.zeros((E, V), np.int32)
    for H, W, sel, intr, w2c in view_chunks(cameras, BYTES_PER_PIXEL + gate.bytes_per_pixel, budget):
        det = detected_masks(lut, maps, sel)
        if thin:
            det = thin_masks(det, backend=backend, device=device)
        d2 = ES.edt_squared(det, backend=backend, device=device)
        del det
        if gate.gated:
            c, h = support_counts(pts_b, off, intr, w2c, d2, tolerances_px, backend=backend,
                                  depth=gate.planes(H, W, sel, intr, w2c), slack=gate.slack, return_hidden=True)
            counts[:, sel, :], hidden[:, sel] = c.cpu().numpy(), h.cpu().numpy()
        else:
            counts[:, sel, :] = support_counts(pts_b, off, intr, w2c, d2, tolerances_px, backend=backend).cpu().numpy()
        del d2
    n_points = np.diff(off.astype(np.int64))
    out = {"counts": torch.from_numpy(counts), "n_points": n_points, "curves": int(len(curves)), "lines": int(len(lines))}
    if gate.gated:
        out["hidden"] = torch.from_numpy(hidden)
    out.update(support_verdict(counts, n_points, V, min_visible, min_near, frames_ratio, keep_index))
    out["settings"] = {"detector": detector, "resolution": resolution, "tolerances_px": tolerances_px,
                       "keep_tolerance_px": float(keep_tolerance_px), "min_visible": float(min_visible),
                       "min_near": float(min_near), "frames_ratio": float(frames_ratio),
                       "edge_threshold": float(edge_threshold), "backend": backend, "views": V, "points": int(pts.shape[0])}
    if thin:
        out["settings"]["thin"] = True
    out["settings"].update(gate.settings())
    return out
