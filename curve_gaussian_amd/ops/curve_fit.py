"""Device side of fit_curve_to_line / merge_curves (scene/topology.py, backend="gpu"): the three data-parallel parts of the
two edits over the HIP kernels of csrc/curve_fit.hip.  float32 model tensors in, float64 arithmetic, deterministic results.
GPU tensors only, on the current stream; there is no CPU path."""
import torch

from .. import _lib as L

MAX_SAMPLES = 256        # CGS_CURVE_FIT_MAX_SAMPLES
MAX_SEGMENTS = 12288     # CGS_SEGMENT_MERGE_MAX


def _curve_points(curve_points, name="curve_points"):
    L.require_gpu_tensor(curve_points, name)
    if curve_points.dim() != 3 or tuple(curve_points.shape[1:]) != (4, 3):
        raise L.CurveGSError(f"{name} must be [B,4,3] (got {tuple(curve_points.shape)})")
    return curve_points.detach().float().contiguous()


def curve_straightness(curve_points, is_bezier, threshold, threshold_max, sample_num=100):
    """``cgs_curve_straightness``: is_curve_straight for every curve at once.  curve_points [B,4,3], is_bezier [B] (bool or
    uint8) -> (mean_dist float64 [B], max_dist float64 [B], straight bool [B]): the mean and maximum distance of the
    `sample_num` samples of each curve to the segment fitted through them, and is_bezier & (mean_dist < threshold) &
    (max_dist < threshold_max)."""
    cp = _curve_points(curve_points)
    L.require_gpu_tensor(is_bezier, "is_bezier")
    dev = cp.device
    B = cp.shape[0]
    if is_bezier.device != dev or tuple(is_bezier.shape) != (B,):
        raise L.CurveGSError(f"is_bezier must be [{B}] on {dev} (got {tuple(is_bezier.shape)} on {is_bezier.device})")
    lib = L.load()
    with L.device_guard(dev):
        isb = is_bezier.to(torch.uint8).contiguous()
        mean = torch.empty((B,), dtype=torch.float64, device=dev)
        mx = torch.empty((B,), dtype=torch.float64, device=dev)
        straight = torch.empty((B,), dtype=torch.uint8, device=dev)
        rc = lib.cgs_curve_straightness(B, L.ptr(cp), L.ptr(isb), int(sample_num), float(threshold), float(threshold_max),
                                        L.ptr(mean), L.ptr(mx), L.ptr(straight), L.raw_stream(dev))
        L.check(rc, "cgs_curve_straightness")
    return mean, mx, straight.bool()


def segment_merge_labels(seg, distance_threshold, similarity_threshold):
    """``cgs_segment_merge_labels``: seg [n,6] (start, end) -> (labels int64 [n], n_components int).  Segments a < b are
    joined when |cos| of their directions >= similarity_threshold and the smaller distance of b's end points to segment a
    <= distance_threshold; labels[i] is the smallest index of i's connected component.  n <= MAX_SEGMENTS.  Reading
    n_components synchronises with the stream."""
    L.require_gpu_tensor(seg, "seg")
    if seg.dim() != 2 or seg.shape[1] != 6:
        raise L.CurveGSError(f"seg must be [n,6] (got {tuple(seg.shape)})")
    lib = L.load()
    dev = seg.device
    with L.device_guard(dev):
        s = seg.detach().float().contiguous()
        n = s.shape[0]
        labels = torch.empty((n,), dtype=torch.int32, device=dev)
        ncomp = torch.zeros((1,), dtype=torch.int32, device=dev)
        ws = torch.empty((int(lib.cgs_segment_merge_workspace_bytes(min(n, MAX_SEGMENTS))),), dtype=torch.uint8, device=dev)
        rc = lib.cgs_segment_merge_labels(n, L.ptr(s), float(distance_threshold), float(similarity_threshold), L.ptr(ws),
                                          L.ptr(labels), L.ptr(ncomp), L.raw_stream(dev))
        L.check(rc, "cgs_segment_merge_labels")
        return labels.long(), int(ncomp.item())


def pair_consensus_fit(curve_points, pairs, sample_num=100, ransac_thresh=0.005, error_threshold=0.02):
    """``cgs_pair_consensus_fit``: for every row (i, j) of pairs [K,2] one cubic Bezier through the 2 * sample_num samples of
    curves i and j, ordered along the line that the most samples lie within `ransac_thresh` of (searched exhaustively over all
    two-point lines).  -> (ctrl float32 [K,4,3], rmse float64 [K], inliers int64 [K], ok bool [K]); ok = a line was found and
    rmse <= error_threshold."""
    cp = _curve_points(curve_points)
    L.require_gpu_tensor(pairs, "pairs")
    dev = cp.device
    if pairs.device != dev or pairs.dim() != 2 or pairs.shape[1] != 2:
        raise L.CurveGSError(f"pairs must be [K,2] on {dev} (got {tuple(pairs.shape)} on {pairs.device})")
    if pairs.is_floating_point():
        raise L.CurveGSError(f"pairs must hold integer curve indices (got {pairs.dtype})")
    lib = L.load()
    B, K = cp.shape[0], pairs.shape[0]
    with L.device_guard(dev):
        if K > 0 and (int(pairs.min()) < 0 or int(pairs.max()) >= B):
            raise L.CurveGSError(f"pairs must index curves 0 .. {B - 1}")
        pr = pairs.to(torch.int32).contiguous()
        ctrl = torch.empty((K, 4, 3), dtype=torch.float32, device=dev)
        rmse = torch.empty((K,), dtype=torch.float64, device=dev)
        inl = torch.empty((K,), dtype=torch.int32, device=dev)
        ok = torch.empty((K,), dtype=torch.uint8, device=dev)
        rc = lib.cgs_pair_consensus_fit(B, L.ptr(cp), K, L.ptr(pr), int(sample_num), float(ransac_thresh),
                                        float(error_threshold), L.ptr(ctrl), L.ptr(rmse), L.ptr(inl), L.ptr(ok),
                                        L.raw_stream(dev))
        L.check(rc, "cgs_pair_consensus_fit")
    return ctrl, rmse, inl.long(), ok.bool()
