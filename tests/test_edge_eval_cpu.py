"""CPU side of the edge evaluation against the reference-generated fixture (tests/golden/make_edge_eval_golden.py): the
loaders, the endpoint merge, the metric arithmetic given NN distances, and the argument checks of cgs_nn1 and of the
Python op."""
import os

import numpy as np
import pytest
import torch

from curve_gaussian_amd import _lib
from curve_gaussian_amd import edge_extraction as EE
from curve_gaussian_amd.scene import dataset_io as IO

GOLD = os.path.join(os.path.dirname(__file__), "golden", "edge_eval")
G = np.load(os.path.join(GOLD, "edge_eval.npz"))
SCANS = [str(s) for s in G["scans"]]


def _exact_dists(a, b):
    """float32 norms of the exact (lowest-index) 1-NN, the way the reference's chamfer re-measures them."""
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    idx = np.argmin(((a64[:, None, :] - b64[None]) ** 2).sum(-1), axis=1)
    return np.linalg.norm(b[idx] - a, axis=-1)


@pytest.mark.parametrize("scan", SCANS)
def test_gt_loader_matches_reference(scan):
    for et in ("all", "curve", "line"):
        got = EE.abc_gt_points(os.path.join(GOLD, "groundtruth"), scan, et)
        assert (got is None) == bool(G[f"gt_{scan}_{et}_none"])
        if got is None:
            continue
        raw, pts, dirs = got
        assert raw.dtype == np.float32 and pts.dtype == np.float32
        assert pts.shape == G[f"gt_{scan}_{et}_pts"].shape and dirs.shape == G[f"gt_{scan}_{et}_dirs"].shape
        np.testing.assert_allclose(raw, G[f"gt_{scan}_{et}_raw"], rtol=0, atol=1e-7)
        np.testing.assert_allclose(pts, G[f"gt_{scan}_{et}_pts"], rtol=0, atol=1e-7)
        np.testing.assert_allclose(dirs, G[f"gt_{scan}_{et}_dirs"], rtol=0, atol=1e-7)


def test_gt_loader_quirks():
    """Interior vertices are emitted twice (one copy per adjacent segment) and segments shorter than 5 mm add nothing."""
    raw, pts, dirs = EE.abc_gt_points(os.path.join(GOLD, "groundtruth"), "00000022", "line")
    u, c = np.unique(pts, axis=0, return_counts=True)
    assert (c >= 2).any()
    assert EE.abc_gt_points(os.path.join(GOLD, "groundtruth"), "00000033", "all") is None


@pytest.mark.parametrize("scan", SCANS)
def test_pred_loader_matches_reference(scan):
    p = EE.pred_points_and_directions(os.path.join(GOLD, "pred", scan, "parametric_edges.json"))
    np.testing.assert_array_equal(p.curve_counts, G[f"pred_{scan}_curve_counts"])
    np.testing.assert_array_equal(p.line_counts, G[f"pred_{scan}_line_counts"])
    assert (p.num_curves, p.num_lines) == tuple(G[f"pred_{scan}_num"])
    for k, ref in (("curve_points", "curve_points"), ("line_points", "line_points"), ("curve_directions", "curve_dirs"),
                   ("line_directions", "line_dirs")):
        got = getattr(p, k)
        assert got.shape == G[f"pred_{scan}_{ref}"].reshape(-1, 3).shape, k
        np.testing.assert_allclose(got, G[f"pred_{scan}_{ref}"].reshape(-1, 3), rtol=0, atol=1e-7)


@pytest.mark.parametrize("case", ["mixed", "lines_only", "curves_only", "no_merge"])
def test_merge_endpoints_matches_reference(case):
    li, ci = G[f"merge_{case}_lines_in"], G[f"merge_{case}_curves_in"]
    ml, mc = EE.merge_endpoints(torch.from_numpy(li), torch.from_numpy(ci), 0.015)
    assert ml.dtype == torch.float64 and mc.dtype == torch.float64
    np.testing.assert_allclose(ml.numpy(), G[f"merge_{case}_lines"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(mc.numpy(), G[f"merge_{case}_curves"], rtol=0, atol=1e-12)
    if case == "no_merge":
        np.testing.assert_array_equal(ml.numpy(), li)
        np.testing.assert_array_equal(mc.numpy(), ci)
    if case == "mixed":
        assert not np.array_equal(ml.numpy(), li)


def test_merge_endpoints_empty():
    ml, mc = EE.merge_endpoints(torch.zeros(0, 6), torch.zeros(0, 12))
    assert ml.shape == (0, 6) and mc.shape == (0, 12)


@pytest.mark.parametrize("scan", [s for s in SCANS if bool(G[f"scan_{s}_valid"])])
def test_metric_arithmetic_matches_reference(scan):
    """Chamfer / precision / recall / F-score / IoU from exact NN distances (computed here in numpy) equal the fixture."""
    gt = G[f"gt_{scan}_all_pts"]
    sampled = G[f"pred_{scan}_sampled"]
    d_pg, d_gp = _exact_dists(sampled, gt), _exact_dists(gt, sampled)
    ch, acc, comp = EE.chamfer_from_distances(torch.from_numpy(d_pg), torch.from_numpy(d_gp))
    for k, v in (("chamfer", ch), ("acc", acc), ("comp", comp)):
        np.testing.assert_allclose(v, float(G[f"scan_{scan}_{k}"]), rtol=0, atol=1e-6, err_msg=k)
    pr = EE.precision_recall_from_distances(torch.from_numpy(d_pg), torch.from_numpy(d_gp))
    for t, r in pr.items():
        for k, name in (("precision", "precision"), ("recall", "recall"), ("fscore", "fscore"), ("iou", "IOU")):
            np.testing.assert_allclose(r[k], float(G[f"scan_{scan}_{name}_{t}"]), rtol=0, atol=1e-12, err_msg=f"{k}@{t}")
    for et in ("curve", "line"):
        if f"scan_{scan}_{et}_counts" not in G:
            continue
        g2 = G[f"gt_{scan}_{et}_pts"]
        pr2 = EE.precision_recall_from_distances(torch.from_numpy(_exact_dists(sampled, g2)),
                                                 torch.from_numpy(_exact_dists(g2, sampled)))
        got = ([pr2[t]["correct_gt"] for t in EE.THRESHOLDS] + [pr2[0.005]["num_gt"]] +
               [pr2[t]["correct_pred"] for t in EE.THRESHOLDS] + [pr2[0.005]["num_pred"]])
        np.testing.assert_array_equal(got, G[f"scan_{scan}_{et}_counts"])


def test_fscore_nan_and_finalisation():
    pr = EE.precision_recall_from_distances(torch.tensor([1.0, 2.0]), torch.tensor([3.0]))
    assert all(np.isnan(r["fscore"]) for r in pr.values())
    assert EE.finalize_metrics({"fscore_0.01": [float("nan"), 0.5], "acc": [0.123456]}) == {"fscore_0.01": 0.25,
                                                                                            "acc": 0.1235}


def test_nn1_rejects_bad_arguments_without_a_gpu():
    lib = _lib.load()
    assert lib.cgs_nn1(0, None, 0, None, None, None, None, None) == 0          # empty query: no-op
    bad = [(5, 0), (-1, 4), (4, -1)]
    for nq, nr in bad:
        assert lib.cgs_nn1(nq, None, nr, None, None, None, None, None) == -1
        assert b"invalid argument" in lib.cgs_last_error()
    # NULL pointers with valid sizes
    assert lib.cgs_nn1(4, None, 4, None, None, None, None, None) == -1
    assert lib.cgs_nn1_workspace_bytes(1000) >= 8000


def test_op_rejects_cpu_tensors():
    with pytest.raises(_lib.CurveGSError, match="GPU tensor"):
        EE.nearest_neighbors(torch.zeros(4, 3), torch.zeros(5, 3))
    with pytest.raises(_lib.CurveGSError, match="GPU tensor"):
        EE.chamfer_distance(torch.zeros(4, 3), torch.zeros(5, 3))


def test_write_parametric_edges_merge_matches_reference(tmp_path):
    class M:
        pass
    g = M()
    g.get_curve_points = torch.from_numpy(G["model_curve_points"])
    g.is_bezier = torch.from_numpy(G["model_is_bezier"])
    d, _ = IO.write_parametric_edges(g, str(tmp_path), merge_endpoints=True)
    np.testing.assert_allclose(np.array(d["lines_end_pts"]).reshape(-1, 6), G["model_merged_lines"], rtol=0, atol=2e-7)
    np.testing.assert_allclose(np.array(d["curves_ctl_pts"]).reshape(-1, 12), G["model_merged_curves"], rtol=0, atol=2e-7)
    d0, _ = IO.write_parametric_edges(g, str(tmp_path / "plain"))
    assert not np.allclose(np.array(d0["lines_end_pts"]).reshape(-1, 6), G["model_merged_lines"], atol=1e-6)
