"""Device side of the edge evaluation: the exact 1-NN op over ``cgs_nn1``, the metric arithmetic as pure functions of
the NN distances, voxel-average downsampling and the endpoint merge, all with torch ops on the input's device."""
import math

import torch

from .. import _lib as L

THRESHOLDS = (0.005, 0.01, 0.02)


def nearest_neighbors(query, ref):
    """Exact 1-NN (``cgs_nn1``): for every row of `query` [N,3] the distance to the nearest row of `ref` [M,3] and its
    index.  Returns (dist float32 [N], index int64 [N]); ties go to the LOWEST index.  GPU tensors only, on the current
    stream; M = 0 with N > 0 raises."""
    L.require_gpu_tensor(query, "query")
    L.require_gpu_tensor(ref, "ref")
    if query.device != ref.device:
        raise L.CurveGSError(f"query and ref are on different devices ({query.device}, {ref.device})")
    if query.dim() != 2 or query.shape[1] != 3 or ref.dim() != 2 or ref.shape[1] != 3:
        raise L.CurveGSError(f"query and ref must be [N,3] and [M,3] (got {tuple(query.shape)}, {tuple(ref.shape)})")
    lib = L.load()
    dev = query.device
    with L.device_guard(dev):
        q = query.float().contiguous()
        r = ref.float().contiguous()
        n, m = q.shape[0], r.shape[0]
        dist = torch.empty((n,), dtype=torch.float32, device=dev)
        index = torch.empty((n,), dtype=torch.int32, device=dev)
        if n > 0:
            ws = torch.empty((int(lib.cgs_nn1_workspace_bytes(n)),), dtype=torch.uint8, device=dev)
            rc = lib.cgs_nn1(n, L.ptr(q), m, L.ptr(r), L.ptr(dist), L.ptr(index), L.ptr(ws), L.raw_stream(dev))
            L.check(rc, "cgs_nn1")
    return dist, index.long()


# ------------------------------------------------------------------------------------------ metrics from NN distances
def chamfer_from_distances(d_pred_to_gt, d_gt_to_pred):
    """eval_utils.py:77-115 (whose variable names are swapped but whose results are not): acc = mean over pred points of
    the distance to the nearest GT point, comp = mean over GT points of the distance to the nearest pred point,
    chamfer = acc + comp.  Returns Python floats (chamfer, acc, comp)."""
    acc = float(torch.as_tensor(d_pred_to_gt).double().mean())
    comp = float(torch.as_tensor(d_gt_to_pred).double().mean())
    return acc + comp, acc, comp


def precision_recall_from_distances(d_pred_to_gt, d_gt_to_pred, thresholds=THRESHOLDS):
    """eval_utils.py:195-249 for every threshold from ONE pair of NN passes (the reference redoes both per threshold).
    Counts use strict `< thresh`; F-score = 2pr/(p+r), nan when p = r = 0 (0 after finalisation); IoU =
    min(cp, cg) / (n_pred + n_gt - max(cp, cg)).  Returns {thresh: dict(precision, recall, fscore, iou, correct_pred,
    correct_gt, num_pred, num_gt)}."""
    dp = torch.as_tensor(d_pred_to_gt)
    dg = torch.as_tensor(d_gt_to_pred)
    n_pred, n_gt = int(dp.numel()), int(dg.numel())
    th = torch.tensor(list(thresholds), dtype=dp.dtype, device=dp.device)
    cps = (dp[None, :] < th[:, None]).sum(1).tolist()
    cgs = (dg[None, :] < th.to(dg.dtype).to(dg.device)[:, None]).sum(1).tolist()
    out = {}
    for t, cp, cg in zip(thresholds, cps, cgs):
        p, r = cp / n_pred, cg / n_gt
        f = 2 * p * r / (p + r) if (p + r) > 0 else math.nan
        iou = min(cp, cg) / (n_pred + n_gt - max(cp, cg))
        out[t] = dict(precision=p, recall=r, fscore=f, iou=iou, correct_pred=int(cp), correct_gt=int(cg),
                      num_pred=n_pred, num_gt=n_gt)
    return out


def similarity_from_index(pred_dirs, gt_dirs, nn_index):
    """eval_ABC.py:27-38 given the nearest GT point of every pred point: mean over pred points of
    |cos(pred_dir, gt_dir[nn])|, in float64."""
    a = torch.as_tensor(pred_dirs).double()
    b = torch.as_tensor(gt_dirs).to(a.device).double()[torch.as_tensor(nn_index).to(a.device).long()]
    cos = (a * b).sum(1) / (a.norm(dim=1) * b.norm(dim=1))
    return float(cos.abs().mean())


# ------------------------------------------------------------------------------------------ GPU metric entry points
def _pts(x, dev):
    return torch.as_tensor(x).to(dev, torch.float32).reshape(-1, 3).contiguous()


def chamfer_distance(pred, gt):
    """(chamfer, acc, comp) between point sets `pred` and `gt` ([N,3] / [M,3], GPU tensors)."""
    dev = pred.device
    d_pg, _ = nearest_neighbors(_pts(pred, dev), _pts(gt, dev))
    d_gp, _ = nearest_neighbors(_pts(gt, dev), _pts(pred, dev))
    return chamfer_from_distances(d_pg, d_gp)


def precision_recall_iou(pred, gt, thresholds=THRESHOLDS):
    """Precision, recall, F-score, IoU and the raw counts at every threshold (see precision_recall_from_distances),
    from one NN pass in each direction."""
    dev = pred.device
    d_pg, _ = nearest_neighbors(_pts(pred, dev), _pts(gt, dev))
    d_gp, _ = nearest_neighbors(_pts(gt, dev), _pts(pred, dev))
    return precision_recall_from_distances(d_pg, d_gp, thresholds)


def direction_similarity(pred_pts, pred_dirs, gt_pts, gt_dirs):
    """eval_ABC.py:27-38: mean over pred points of the absolute cosine between the pred direction and the direction of
    the nearest GT point (the lowest-index one among equally near GT points).  Takes the FULL pred point set."""
    dev = pred_pts.device
    _, idx = nearest_neighbors(_pts(pred_pts, dev), _pts(gt_pts, dev))
    return similarity_from_index(torch.as_tensor(pred_dirs).to(dev), torch.as_tensor(gt_dirs).to(dev), idx)


def downsample_point_cloud_average(points, num_voxels_per_axis=256, min_bound=(0.0, 0.0, 0.0), max_bound=(1.0, 1.0, 1.0)):
    """Voxel-average downsampling (eval_utils.py:500-538 -> point_cloud_utils.downsample_point_cloud_on_voxel_grid),
    with torch ops on the points' device, accumulated in float64.

    Semantics (chosen here; point_cloud_utils is not available to pin them, so they are UNPINNED against the
    reference): voxel_size = (max_bound - min_bound) / num_voxels_per_axis; a point with any coordinate below min_bound
    or above max_bound is dropped; the voxel of a kept point is floor((p - min_bound) / voxel_size) per axis, computed in
    float64 and clamped to num_voxels_per_axis - 1, so a point exactly on max_bound falls into the last voxel.  Each
    occupied voxel yields the float64 mean of its points, returned as float32 [V,3] in ascending voxel order
    (x-major).  No metric depends on the order of the rows."""
    p = torch.as_tensor(points).reshape(-1, 3)
    dev = p.device
    p64 = p.double()
    n = torch.as_tensor(num_voxels_per_axis, dtype=torch.int64).expand(3).to(dev)
    lo = torch.as_tensor(min_bound, dtype=torch.float64, device=dev)
    hi = torch.as_tensor(max_bound, dtype=torch.float64, device=dev)
    size = (hi - lo) / n.double()
    keep = ((p64 >= lo) & (p64 <= hi)).all(1)
    p64 = p64[keep]
    v = torch.minimum(torch.floor((p64 - lo) / size).long(), n - 1)
    vid = (v[:, 0] * n[1] + v[:, 1]) * n[2] + v[:, 2]
    uniq, inv = torch.unique(vid, sorted=True, return_inverse=True)
    s = torch.zeros((uniq.numel(), 3), dtype=torch.float64, device=dev).index_add_(0, inv, p64)
    c = torch.zeros((uniq.numel(),), dtype=torch.float64, device=dev).index_add_(
        0, inv, torch.ones_like(inv, dtype=torch.float64))
    return (s / c[:, None]).float()


# ------------------------------------------------------------------------------------------ endpoint merge
def _components(pts, threshold, chunk=4096):
    """Connected components of the graph "|a - b| <= threshold" (scipy cdist + csgraph.connected_components in the
    reference), labelled by the smallest member index: the edges are found chunk by chunk in float64 and the labels
    spread by min-propagation with pointer jumping until they no longer change."""
    n = pts.shape[0]
    src, dst = [], []
    for a in range(0, n, chunk):
        d = (pts[a:a + chunk, None, :] - pts[None, :, :]).pow(2).sum(-1).sqrt()
        i, j = torch.nonzero(d <= threshold, as_tuple=True)
        keep = (i + a) != j
        src.append(i[keep] + a)
        dst.append(j[keep])
    src, dst = torch.cat(src), torch.cat(dst)
    label = torch.arange(n, device=pts.device)
    while True:
        new = label.clone().scatter_reduce_(0, src, label[dst], reduce="amin")
        new = new[new]
        if torch.equal(new, label):
            return label
        label = new


def merge_endpoints(lines, curves, distance_threshold=0.015):
    """edge_extraction/merging.py:10-54 with torch ops on the input's device: the endpoints of the line segments
    (lines [N,6]) and of the cubic Beziers (curves [M,12], first and last control point) are grouped into the connected
    components of "distance <= distance_threshold", and every endpoint of a component of two or more is replaced by the
    component's mean.  The middle control points of the curves are kept.  Returns (lines [N,6], curves [M,12]), new
    tensors of the inputs' dtype."""
    lines = torch.as_tensor(lines)
    curves = torch.as_tensor(curves)
    dev = lines.device if lines.numel() else curves.device
    dtype = lines.dtype if lines.numel() else curves.dtype
    lines = lines.reshape(-1, 6).to(dev, dtype)
    curves = curves.reshape(-1, 12).to(dev, dtype)
    n_l, n_c = lines.shape[0], curves.shape[0]
    if n_l == 0 and n_c == 0:
        return lines.clone(), curves.clone()
    ends = torch.cat([lines.reshape(-1, 3), curves[:, [0, 1, 2, 9, 10, 11]].reshape(-1, 3)], 0)
    label = _components(ends.double(), distance_threshold)
    cnt = torch.zeros(ends.shape[0], dtype=torch.float64, device=dev).index_add_(
        0, label, torch.ones(ends.shape[0], dtype=torch.float64, device=dev))
    s = torch.zeros((ends.shape[0], 3), dtype=torch.float64, device=dev).index_add_(0, label, ends.double())
    mean = (s / cnt.clamp(min=1)[:, None]).to(dtype)
    merged = torch.where((cnt[label] > 1)[:, None], mean[label], ends)
    out_l = merged[:2 * n_l].reshape(-1, 6)
    ce = merged[2 * n_l:].reshape(-1, 6)
    out_c = curves.clone()
    out_c[:, :3] = ce[:, :3]
    out_c[:, 9:] = ce[:, 3:]
    return out_l, out_c
