"""Reprojection score of extracted edges: predicted edge pixels against detected edge pixels, view by view, in pixels
(cgs_point_mask / cgs_edt_squared / cgs_edge_score_reduce, include/curvegs.h; csrc/edge_score.hip).  Needs no 3D ground
truth.  The reference has no counterpart.

  point_masks   the prediction mask of every camera: pixel (floor(u), floor(v)) of every point that ``project_points``
                keeps (the projection rule of cgs_project_points, float64, to the letter)
  edt_squared   the exact squared Euclidean distance transform of a stack of masks, int32: the minimum over the set pixels
                of dx^2 + dy^2, ``EDT_INF`` everywhere in a view without one.  Two passes: per column the distance g to the
                nearest set pixel of the column; per pixel the minimum of d^2 + g[x -+ d]^2 outward over d while d^2 is
                below the best so far
  score_masks   per view: n_pred, n_det, the predicted pixels within a tolerance of a detected one (and the reverse), the
                sums of the distances in both directions; and the aggregate over the views

The aggregate, micro-averaged over the views (frozen):
  precision[t]    = sum_v pred_hits[v][t] / sum_v n_pred[v]        pred_hits: predicted pixels with a detected pixel within
  recall[t]       = sum_v det_hits[v][t]  / sum_v n_det[v]         tolerance t (Euclidean, dist^2 <= t^2); det_hits likewise
  fscore[t]       = 2 P R / (P + R), 0 when P + R = 0
  accuracy_px     = sum_v sum_pred_to_det[v] / sum_v n_pred[v]     over the views in which BOTH masks are non-empty
  completeness_px = sum_v sum_det_to_pred[v] / sum_v n_det[v]      over the same views
  chamfer_px      = accuracy_px + completeness_px
  chamfer_views   = the number of those views
A zero denominator gives NaN (fscore: NaN when precision or recall is NaN).  A view in which either mask is empty counts
n_pred and n_det, has zero hits and adds nothing to the two distance sums.

Two back ends: ``"gpu"``, HIP, and ``"host"``, numpy -- the same rules in integers, for a machine without a GPU and what
the tests hold the kernels against.  Counts and distance transforms agree exactly between them; the two float64 sums
differ in summation order only."""
import ctypes as C
import math

import numpy as np
import torch

from .. import _lib as L
from .view_chunks import check_budget

SCORE_BACKENDS = ("gpu", "host")
EDT_INF = L.EDT_INF
BYTE_BUDGET = 1 << 30    # bytes of masks, transforms and scratch per chunk of views in score_masks
BYTES_PER_PIXEL = 12     # two uint8 masks, two int32 transforms, one uint16 column pass
DEPTH_BYTES_PER_PIXEL = 8   # score_edges with a depth source, per pixel more: the float32 depth plane and its window maximum
CONTOUR_BYTES_PER_PIXEL = 8   # score_edges with ignore_contours, per pixel more: the uint8 contour mask, its int32 transform
                              # with the uint16 column pass, and the bool zone


def _check_backend(backend):
    if backend not in SCORE_BACKENDS:
        raise ValueError(f"unknown edge score backend {backend!r}: expected one of {SCORE_BACKENDS}")


def _check_size(what, height, width):
    height, width = int(height), int(width)
    if not (1 <= height <= L.EDT_MAX_SIZE and 1 <= width <= L.EDT_MAX_SIZE):
        raise ValueError(f"{what}: height and width must lie in [1, {L.EDT_MAX_SIZE}] (got {height}x{width})")
    return height, width


def _as_masks(masks, what):
    """uint8 (or bool) [V,H,W] -> a contiguous uint8 tensor, as given where nothing needs converting."""
    if isinstance(masks, np.ndarray):
        masks = torch.from_numpy(np.ascontiguousarray(masks))
    if not torch.is_tensor(masks) or masks.dtype not in (torch.uint8, torch.bool) or masks.dim() != 3:
        raise ValueError(f"{what} must be a uint8 or bool [V,H,W] stack of masks")
    if masks.dtype == torch.bool:
        masks = masks.to(torch.uint8)
    if masks.shape[0] > 0:
        _check_size(what, masks.shape[1], masks.shape[2])
    return masks.contiguous()


def _device_for(tensors, what, device=None):
    if device is not None:
        return torch.device(device)
    dev = next((t.device for t in tensors if torch.is_tensor(t) and t.is_cuda), None)
    if dev is None:
        if not torch.cuda.is_available():
            raise L.CurveGSError(f"{what}: backend='gpu' needs a GPU (backend='host' computes on the CPU)")
        dev = torch.device("cuda", torch.cuda.current_device())
    return dev


def tolerances_squared(tolerances_px):
    """floor(t^2) of every tolerance: for an integer dist^2, dist^2 <= t^2 iff dist^2 <= floor(t^2)."""
    tol = [float(t) for t in tolerances_px]
    if len(tol) > L.EDGE_SCORE_MAX_TOL:
        raise ValueError(f"at most {L.EDGE_SCORE_MAX_TOL} tolerances (got {len(tol)})")
    for t in tol:
        if not (0.0 <= t <= L.EDT_MAX_SIZE):
            raise ValueError(f"a tolerance must lie in [0, {L.EDT_MAX_SIZE}] pixels (got {t})")
    return [int(math.floor(t * t)) for t in tol]


# ------------------------------------------------------------------------------------------------ point masks
def _host(x):
    """A tensor (any device) or an array as a numpy array."""
    return x.detach().cpu().numpy() if torch.is_tensor(x) else np.asarray(x)


def _cameras(intrinsics, w2c, error=ValueError):
    """(V, K [V,4], M [V,12]) contiguous float64 host arrays of a camera stack, checked; ``error``: what a bad shape raises."""
    K, M = (np.asarray(_host(x), dtype=np.float64) for x in (intrinsics, w2c))
    V = K.shape[0] if K.ndim == 2 else -1
    if K.shape != (V, 4) or M.size != 12 * V:
        raise error(f"intrinsics must be [V,4] and w2c [V,3,4] (got {K.shape}, {M.shape})")
    return V, np.ascontiguousarray(K), np.ascontiguousarray(M.reshape(V, 12))


def cameras_on(dev, K, M):
    """The checked host arrays of ``_cameras`` as tensors on ``dev``."""
    return torch.from_numpy(K).to(dev), torch.from_numpy(M).to(dev)


def project_points_host(points, K, M, height, width):
    """The rule of cgs_project_points in numpy float64, operation for operation (numpy evaluates one rounded operation
    per ufunc call: nothing is contracted): (u, v, keep), each [V,P]."""
    P = np.asarray(points, np.float32).reshape(-1, 3).astype(np.float64)
    X, Y, Z = P[None, :, 0], P[None, :, 1], P[None, :, 2]
    m = lambda k: M[:, k:k + 1]
    with np.errstate(all="ignore"):
        c0 = ((m(0) * X + m(1) * Y) + m(2) * Z) + m(3)
        c1 = ((m(4) * X + m(5) * Y) + m(6) * Z) + m(7)
        c2 = ((m(8) * X + m(9) * Y) + m(10) * Z) + m(11)
        u = K[:, 0:1] * (c0 / c2) + K[:, 2:3]
        v = K[:, 1:2] * (c1 / c2) + K[:, 3:4]
        keep = ~(c2 <= 0.0) & (u >= 0.0) & (u < float(width)) & (v >= 0.0) & (v < float(height))   # NaN fails the image test
    return u, v, keep


def point_masks(points, intrinsics, w2c, height, width, backend="gpu", device=None, return_kept=False):
    """uint8 [V,height,width]: 1 at pixel (floor(u), floor(v)) of every point that ``cgs_project_points`` keeps in view v,
    0 elsewhere.  points float32 [P,3] (tensor or array); intrinsics [V,4] = (fx, fy, cx, cy) and w2c [V,3,4] float64 host
    arrays or tensors.  With return_kept, also the int32 [V] number of kept points per view.
    ``backend="gpu"``: ``cgs_point_mask``; the points are uploaded when they are not on a GPU (``device``: which one), the
    result stays on the device.  ``backend="host"``: numpy, CPU tensors."""
    _check_backend(backend)
    height, width = _check_size("point_masks", height, width)
    V, K, M = _cameras(intrinsics, w2c)
    pts = points if torch.is_tensor(points) else torch.from_numpy(np.ascontiguousarray(points, np.float32).reshape(-1, 3))
    if pts.dim() != 2 or pts.shape[1] != 3:
        raise ValueError(f"points must be [P,3] (got {tuple(pts.shape)})")
    pts = pts.detach().to(torch.float32)
    if backend == "host":
        mask = np.zeros((V, height, width), np.uint8)
        kept = np.zeros((V,), np.int32)
        host_pts = pts.cpu().numpy()
        for i in range(V):   # one view at a time: [P] temporaries
            u, v, keep = project_points_host(host_pts, K[i:i + 1], M[i:i + 1], height, width)
            u, v = u[0][keep[0]], v[0][keep[0]]
            mask[i, np.floor(v).astype(np.int64), np.floor(u).astype(np.int64)] = 1
            kept[i] = u.size
        mask = torch.from_numpy(mask)
        return (mask, torch.from_numpy(kept)) if return_kept else mask
    dev = _device_for([pts], "point_masks", device)
    with L.device_guard(dev):
        pts = pts.to(dev).contiguous()
        mask = torch.empty((V, height, width), dtype=torch.uint8, device=dev)
        kept = torch.empty((V,), dtype=torch.int32, device=dev)
        if V > 0:
            Kd, Md = cameras_on(dev, K, M)
            rc = L.load().cgs_point_mask(int(pts.shape[0]), L.ptr(pts), V, L.ptr(Kd), L.ptr(Md), height, width, L.ptr(mask),
                                         L.ptr(kept), L.raw_stream(dev))
            L.check(rc, "cgs_point_mask")
    return (mask, kept) if return_kept else mask


# ------------------------------------------------------------------------------------------------ distance transform
_NO_FEATURE = 1 << 20   # host column pass: above every distance, its square still fits an int64


def _edt_columns_host(m):
    """g [H,W] int64: the distance to the nearest set pixel of the same column, _NO_FEATURE where the column has none."""
    H, W = m.shape
    rows = np.arange(H, dtype=np.int64)[:, None]
    above = np.maximum.accumulate(np.where(m, rows, -_NO_FEATURE), axis=0)           # the last set row <= y
    below = np.minimum.accumulate(np.where(m, rows, 2 * _NO_FEATURE)[::-1], axis=0)[::-1]   # the first set row >= y
    return np.minimum(np.minimum(rows - above, below - rows), _NO_FEATURE)


def edt_squared_host(mask):
    """One view, numpy, integers: int32 [H,W].  The row pass visits d = 1, 2, ... for all pixels at once and keeps, from
    the moment they are few, only the pixels whose search is still open (d^2 < best)."""
    m = np.asarray(mask) != 0
    H, W = m.shape
    if not m.any():
        return np.full((H, W), EDT_INF, np.int32)
    g = _edt_columns_host(m)
    g2 = np.where(g >= _NO_FEATURE, np.int64(EDT_INF), g * g)
    best = g2.copy()
    d = 1
    while d < W and (d * d < best).any() and 4 * np.count_nonzero(d * d < best) > best.size:   # dense steps
        np.minimum(best[:, d:], d * d + g2[:, :-d], out=best[:, d:])      # the neighbour at x - d
        np.minimum(best[:, :-d], d * d + g2[:, d:], out=best[:, :-d])     # the neighbour at x + d
        d += 1
    ys, xs = np.nonzero(d * d < best)
    while d < W and ys.size:                                               # sparse steps: the open pixels only
        b = best[ys, xs]
        left, right = xs - d >= 0, xs + d < W
        b[left] = np.minimum(b[left], d * d + g2[ys[left], xs[left] - d])
        b[right] = np.minimum(b[right], d * d + g2[ys[right], xs[right] + d])
        best[ys, xs] = b
        d += 1
        open_ = d * d < b
        ys, xs = ys[open_], xs[open_]
    return np.minimum(best, EDT_INF).astype(np.int32)


def edt_squared(masks, backend="gpu", device=None):
    """masks: uint8 or bool [V,H,W], nonzero = feature pixel.  Returns int32 [V,H,W]: the exact squared Euclidean distance
    of every pixel to the nearest feature pixel of its view, ``EDT_INF`` everywhere in a view without one.  H and W lie in
    [1, 16384].  ``backend="gpu"``: ``cgs_edt_squared``, the result stays on the device.  ``backend="host"``: numpy."""
    _check_backend(backend)
    masks = _as_masks(masks, "edt_squared: masks")
    V, H, W = (int(s) for s in masks.shape)
    if backend == "host":
        m = _host(masks)
        out = np.empty((V, H, W), np.int32)
        for v in range(V):
            out[v] = edt_squared_host(m[v])
        return torch.from_numpy(out)
    dev = _device_for([masks], "edt_squared", device)
    lib = L.load()
    with L.device_guard(dev):
        masks = masks.to(dev)
        out = torch.empty((V, H, W), dtype=torch.int32, device=dev)
        if V > 0:
            ws = torch.empty((lib.cgs_edt_workspace_bytes(V, H, W),), dtype=torch.uint8, device=dev)
            rc = lib.cgs_edt_squared(V, H, W, L.ptr(masks), L.ptr(ws), L.ptr(out), L.raw_stream(dev))
            L.check(rc, "cgs_edt_squared")
    return out


# ------------------------------------------------------------------------------------------------ reduction and score
def _reduce_host(pred, det, pred_d2, det_d2, tol2):
    V, n_tol = pred.shape[0], len(tol2)
    counts = np.zeros((V, 2 + 2 * n_tol), np.int64)
    sums = np.zeros((V, 2), np.float64)
    both = np.zeros((V,), np.uint8)
    for v in range(V):
        p, q = pred[v] != 0, det[v] != 0
        counts[v, 0], counts[v, 1] = p.sum(), q.sum()
        if counts[v, 0] == 0 or counts[v, 1] == 0:
            continue
        both[v] = 1
        dp, dq = det_d2[v][p], pred_d2[v][q]
        for t, t2 in enumerate(tol2):
            counts[v, 2 + t] = np.count_nonzero(dp <= t2)
            counts[v, 2 + n_tol + t] = np.count_nonzero(dq <= t2)
        sums[v, 0] = np.sqrt(dp.astype(np.float64)).sum()
        sums[v, 1] = np.sqrt(dq.astype(np.float64)).sum()
    return counts, sums, both


def _reduce_gpu(pred, det, pred_d2, det_d2, tol2):
    dev = pred.device
    lib = L.load()
    V, H, W = (int(s) for s in pred.shape)
    n_tol = len(tol2)
    counts = torch.empty((V, 2 + 2 * n_tol), dtype=torch.int64, device=dev)
    sums = torch.empty((V, 2), dtype=torch.float64, device=dev)
    both = torch.empty((V,), dtype=torch.uint8, device=dev)
    ws = torch.empty((lib.cgs_edge_score_workspace_bytes(V),), dtype=torch.uint8, device=dev)
    tol_c = (C.c_int * max(n_tol, 1))(*tol2)
    rc = lib.cgs_edge_score_reduce(V, H, W, L.ptr(pred), L.ptr(det), L.ptr(pred_d2), L.ptr(det_d2), n_tol,
                                   C.cast(tol_c, C.c_void_p), L.ptr(ws), L.ptr(counts), L.ptr(sums), L.ptr(both),
                                   L.raw_stream(dev))
    L.check(rc, "cgs_edge_score_reduce")
    return counts.cpu().numpy(), sums.cpu().numpy(), both.cpu().numpy()


def _ratio(num, den):
    return float(num) / float(den) if den else float("nan")


def aggregate_scores(tolerances_px, n_pred, n_det, pred_hits, det_hits, sum_pred_to_det, sum_det_to_pred, both_nonempty):
    """The aggregate of the module docstring from per-view arrays (numpy; hits are [V,n_tol])."""
    both = np.asarray(both_nonempty).astype(bool)
    precision = [_ratio(pred_hits[:, t].sum(), n_pred.sum()) for t in range(len(tolerances_px))]
    recall = [_ratio(det_hits[:, t].sum(), n_det.sum()) for t in range(len(tolerances_px))]
    fscore = [(2.0 * p * r / (p + r) if p + r > 0.0 else (0.0 if p + r == 0.0 else float("nan")))
              for p, r in zip(precision, recall)]
    accuracy = _ratio(sum_pred_to_det[both].sum(), n_pred[both].sum())
    completeness = _ratio(sum_det_to_pred[both].sum(), n_det[both].sum())
    return {"tolerances_px": [float(t) for t in tolerances_px], "precision": precision, "recall": recall, "fscore": fscore,
            "accuracy_px": accuracy, "completeness_px": completeness, "chamfer_px": accuracy + completeness,
            "chamfer_views": int(both.sum()), "views": int(both.shape[0]), "n_pred": int(n_pred.sum()),
            "n_det": int(n_det.sum())}


def score_masks(pred_masks, det_masks, tolerances_px=(1, 2, 4), backend="gpu", device=None, budget_bytes=None):
    """pred_masks, det_masks: uint8 or bool [V,H,W] (tensors or arrays), nonzero = edge pixel.  Returns a dict of CPU tensors
    per view -- ``n_pred``, ``n_det`` int64 [V]; ``pred_hits``, ``det_hits`` int64 [V,n_tol]; ``sum_pred_to_det``,
    ``sum_det_to_pred`` float64 [V]; ``both_nonempty`` bool [V] -- and ``"aggregate"``, the dict the module docstring
    defines (precision, recall, fscore per tolerance; accuracy_px, completeness_px, chamfer_px, chamfer_views; views,
    n_pred, n_det).

    The views are processed in chunks of at most ``budget_bytes`` (default BYTE_BUDGET) of masks, distance transforms and
    scratch, 12 bytes per pixel, and at least one view; every view is reduced on its own, so the result does not depend
    on the chunking.  ``backend="gpu"``: masks not on a GPU are uploaded chunk by chunk (``device``: which GPU);
    ``backend="host"``: numpy."""
    _check_backend(backend)
    tol2 = tolerances_squared(tolerances_px)
    pred = _as_masks(pred_masks, "score_masks: pred_masks")
    det = _as_masks(det_masks, "score_masks: det_masks")
    if pred.shape != det.shape:
        raise ValueError(f"score_masks: pred_masks {tuple(pred.shape)} and det_masks {tuple(det.shape)} differ in shape")
    budget = check_budget("score_masks", budget_bytes, BYTE_BUDGET)
    V, H, W = (int(s) for s in pred.shape)
    per = max(1, budget // (BYTES_PER_PIXEL * H * W)) if V else 1
    dev = _device_for([pred, det], "score_masks", device) if backend == "gpu" else None
    parts = []
    for v0 in range(0, V, per):
        p, q = pred[v0:v0 + per], det[v0:v0 + per]
        if backend == "host":
            p, q = _host(p), _host(q)
            pd2, qd2 = edt_squared(p, "host").numpy(), edt_squared(q, "host").numpy()
            parts.append(_reduce_host(p, q, pd2, qd2, tol2))
        else:
            with L.device_guard(dev):
                p, q = p.to(dev).contiguous(), q.to(dev).contiguous()
                parts.append(_reduce_gpu(p, q, edt_squared(p, "gpu", dev), edt_squared(q, "gpu", dev), tol2))
    n_tol = len(tol2)
    counts = np.concatenate([c for c, _, _ in parts]) if parts else np.zeros((0, 2 + 2 * n_tol), np.int64)
    sums = np.concatenate([s for _, s, _ in parts]) if parts else np.zeros((0, 2), np.float64)
    both = np.concatenate([b for _, _, b in parts]) if parts else np.zeros((0,), np.uint8)
    out = {"n_pred": counts[:, 0], "n_det": counts[:, 1], "pred_hits": counts[:, 2:2 + n_tol],
           "det_hits": counts[:, 2 + n_tol:], "sum_pred_to_det": sums[:, 0], "sum_det_to_pred": sums[:, 1],
           "both_nonempty": both.astype(bool)}
    agg = aggregate_scores(list(tolerances_px), **out)
    out = {k: torch.from_numpy(np.ascontiguousarray(a)) for k, a in out.items()}
    out["aggregate"] = agg
    return out
