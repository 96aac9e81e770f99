"""GPU: cgs_point_mask / cgs_edt_squared / cgs_edge_score_reduce (csrc/edge_score.hip) against the host back end of
ops.edge_score, the chunking of score_masks, and score_scan on the device against its host result."""
import numpy as np
import pytest
import torch

import edge_score_cases as SC
from curve_gaussian_amd.edge_extraction import novel_view as NV
from curve_gaussian_amd.edge_extraction import reprojection as RP
from curve_gaussian_amd.ops import edge_score as ES

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
# 3 x 2500: a row wider than a workgroup (and than any LDS tile), the longest search; 70 x 37: a row shorter than a wave
GPU_SHAPES = [(3, 2500), (70, 37)]
STACKS = SC.edt_stacks(GPU_SHAPES)


@pytest.mark.parametrize("name", sorted(STACKS))
def test_edt_is_bit_identical_to_the_host(name):
    stack = STACKS[name]
    assert stack.shape[0] == 3
    got = ES.edt_squared(torch.from_numpy(stack), backend="gpu")
    assert got.is_cuda and got.dtype == torch.int32 and tuple(got.shape) == stack.shape
    want = ES.edt_squared(stack, backend="host")
    assert torch.equal(got.cpu(), want)
    if name.endswith("_special"):
        assert (got[0] == ES.EDT_INF).all() and (got[1] == 0).all()   # the sentinel; the full view


def test_edt_of_one_view_does_not_depend_on_its_neighbours():
    stack = torch.from_numpy(STACKS["37x70_random"]).to(DEV)
    whole = ES.edt_squared(stack, backend="gpu")
    for v in range(3):
        assert torch.equal(ES.edt_squared(stack[v:v + 1], backend="gpu")[0], whole[v])


def test_point_mask_against_the_host_and_project_points():
    intr, w2c = SC.mask_cameras()
    pts = SC.mask_points()
    assert 450 <= len(pts) <= 550
    mask, kept = ES.point_masks(torch.from_numpy(pts).to(DEV), intr, w2c, SC.MASK_H, SC.MASK_W, backend="gpu", return_kept=True)
    want_mask, want_kept = ES.point_masks(pts, intr, w2c, SC.MASK_H, SC.MASK_W, backend="host", return_kept=True)
    assert mask.is_cuda and mask.dtype == torch.uint8 and kept.dtype == torch.int32
    assert torch.equal(mask.cpu(), want_mask) and torch.equal(kept.cpu(), want_kept)
    uv = NV.project_points(torch.from_numpy(pts).to(DEV), intr, w2c, SC.MASK_H, SC.MASK_W)
    assert torch.equal((~torch.isnan(uv[..., 0])).sum(1).to(torch.int32), kept)
    assert int(mask[0].sum()) < int(kept[0])   # several points in one pixel
    # a dirty output buffer: the call zeroes the mask itself
    again = ES.point_masks(torch.from_numpy(pts[:0]).to(DEV), intr, w2c, SC.MASK_H, SC.MASK_W, backend="gpu")
    assert int(again.sum()) == 0


def _reduce(pred, det, tol2, backend):
    if backend == "host":
        return ES._reduce_host(pred, det, ES.edt_squared(pred, "host").numpy(), ES.edt_squared(det, "host").numpy(), tol2)
    p, q = torch.from_numpy(pred).to(DEV), torch.from_numpy(det).to(DEV)
    return ES._reduce_gpu(p, q, ES.edt_squared(p, "gpu"), ES.edt_squared(q, "gpu"), tol2)


def test_reduce_against_the_host_and_twice():
    """Counts identical; the two float64 sums within 1e-11 relative: every term is a correctly rounded square root, only
    the summation order differs, n 2^-53 with n < 10^4 terms is about 1e-12 and the tolerance leaves a decade over it."""
    pred, det = SC.score_stack(V=4, H=130, W=150)
    assert pred[0].sum() < 10 ** 4 and det[0].sum() < 10 ** 4
    tol2 = ES.tolerances_squared((1, 2, 4, 7.5))
    counts, sums, both = _reduce(pred, det, tol2, "gpu")
    want_counts, want_sums, want_both = _reduce(pred, det, tol2, "host")
    assert counts.dtype == np.int64 and np.array_equal(counts, want_counts) and np.array_equal(both, want_both)
    assert both.tolist() == [1, 0, 0, 1] and (sums[1:3] == 0.0).all() and (counts[1:3, 2:] == 0).all()
    rel = np.abs(sums - want_sums) / np.maximum(np.abs(want_sums), 1e-300)
    print(f"largest relative difference of the sums: {rel.max():.3e}")
    assert (rel[[0, 3]] <= 1e-11).all()
    counts2, sums2, both2 = _reduce(pred, det, tol2, "gpu")
    assert np.array_equal(counts, counts2) and np.array_equal(both, both2)
    assert np.array_equal(sums.view(np.int64), sums2.view(np.int64))   # bit for bit


def test_chunking_changes_nothing():
    pred, det = SC.score_stack()
    whole = ES.score_masks(pred, det, (1, 2, 4), backend="gpu")
    single = ES.score_masks(pred, det, (1, 2, 4), backend="gpu", budget_bytes=1)   # one view per chunk
    for k, v in whole.items():
        if k == "aggregate":
            assert repr(v) == repr(single[k])
        else:
            assert torch.equal(v, single[k]), k
    host = ES.score_masks(pred, det, (1, 2, 4), backend="host")
    for k in ("n_pred", "n_det", "pred_hits", "det_hits", "both_nonempty"):
        assert torch.equal(whole[k], host[k]), k


def test_score_scan_gpu_equals_host(tmp_path):
    base, data = SC.write_scan(tmp_path, "colmap", "DexiNed")
    kw = dict(layout="colmap", detector="DexiNed", sample_resolution=SC.SCAN_RESOLUTION)
    host = RP.score_scan(base, data, "room", backend="host", **kw)
    gpu = RP.score_scan(base, data, "room", backend="gpu", **kw)
    assert gpu["aggregate"]["fscore"][0] == 1.0
    for key in ("precision", "recall", "fscore", "chamfer_views", "views", "n_pred", "n_det"):
        assert gpu["aggregate"][key] == host["aggregate"][key], key
    for key in ("accuracy_px", "completeness_px", "chamfer_px"):
        assert gpu["aggregate"][key] == pytest.approx(host["aggregate"][key], rel=1e-11, abs=0.0), key
    for a, b in zip(gpu["views"], host["views"]):
        for key in ("name", "kept_points", "n_pred", "n_det", "pred_hits", "det_hits", "both_nonempty"):
            assert a[key] == b[key], key
