"""GPU: the exact 1-NN kernel (cgs_nn1) against float64 brute force, and the edge metrics on the reference-generated
fixture (tests/golden/make_edge_eval_golden.py)."""
import os

import numpy as np
import pytest
import torch

from curve_gaussian_amd import edge_extraction as EE

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden", "edge_eval")
G = np.load(os.path.join(GOLD, "edge_eval.npz"))
SCANS = [str(s) for s in G["scans"] if bool(G[f"scan_{s}_valid"])]
DEV = torch.device("cuda:0")


def _brute(q, r, chunk=128):
    """Per query: the float64 distance to the nearest ref point, the lowest argmin of the fp32 squared distance
    (dx*dx + dy*dy) + dz*dz -- the kernel's definition."""
    q64, r64 = q.astype(np.float64), r.astype(np.float64)
    d64, i32 = np.empty(len(q)), np.empty(len(q), np.int64)
    for a in range(0, len(q), chunk):
        dd = np.sqrt(((q64[a:a + chunk, None, :] - r64[None]) ** 2).sum(-1))
        d64[a:a + chunk] = dd.min(1)
        diff = q[a:a + chunk, None, :] - r[None]                           # float32
        s = (diff[..., 0] * diff[..., 0] + diff[..., 1] * diff[..., 1]) + diff[..., 2] * diff[..., 2]
        i32[a:a + chunk] = np.argmin(s, axis=1)
    return d64, i32


def _check(q, r):
    dq, dr = torch.from_numpy(q).to(DEV), torch.from_numpy(r).to(DEV)
    d, i = EE.nearest_neighbors(dq, dr)
    d2, i2 = EE.nearest_neighbors(dq, dr)
    torch.cuda.synchronize()
    assert torch.equal(d, d2) and torch.equal(i, i2), "two runs differ"
    d, i = d.cpu().numpy(), i.cpu().numpy()
    d64, i32 = _brute(q, r)
    assert np.all(np.abs(d - d64) <= 1e-7 + 1e-6 * d64), float(np.abs(d - d64).max())
    # the returned index is one of the (float64) nearest within the tolerance ...
    di = np.linalg.norm(q.astype(np.float64) - r[i].astype(np.float64), axis=1)
    assert np.all(di <= d64 + 1e-7 + 1e-6 * d64)
    # ... and exactly the lowest index of the fp32 minimum (the kernel's tie rule)
    np.testing.assert_array_equal(i, i32)
    return d, i


@pytest.mark.parametrize("n,m", [(1, 1), (63, 65), (64, 64), (65, 1000), (2000, 7), (20000, 50000)])
def test_nn_random_both_directions(n, m):
    g = np.random.default_rng(n * 7919 + m)
    q = g.random((n, 3), dtype=np.float32)
    r = g.random((m, 3), dtype=np.float32)
    _check(q, r)
    _check(r, q)


def test_nn_duplicates_and_ties():
    g = np.random.default_rng(1)
    base = g.random((300, 3), dtype=np.float32)
    r = np.concatenate([base, base[::-1], base[:50]])               # every point two or three times
    _, i = _check(base, r)
    np.testing.assert_array_equal(i, np.arange(300))                # the first copy wins
    # symmetric constellations: a query at the centre of +-e along each axis (identical fp32 distances)
    c = np.float32(0.5)
    e = np.float32(0.125)
    r2 = np.array([[c + e, c, c], [c - e, c, c], [c, c + e, c], [c, c - e, c], [c, c, c + e], [c, c, c - e]], np.float32)
    r2 = np.concatenate([g.random((700, 3), dtype=np.float32) * 0.1 + 0.9, r2[::-1], r2])
    d, i = _check(np.array([[c, c, c]], np.float32), r2)
    assert i[0] == 700 and abs(d[0] - e) <= 1e-7


def test_nn_far_clusters():
    g = np.random.default_rng(2)
    q = np.concatenate([g.normal(0, 1e-3, (500, 3)), g.normal(100, 1e-3, (500, 3))]).astype(np.float32)
    r = np.concatenate([g.normal(100, 1e-3, (900, 3)), g.normal(-50, 1.0, (300, 3)), g.normal(0, 1e-3, (700, 3))]).astype(np.float32)
    _check(q, r)
    _check(r, q)


def test_nn_empty_and_errors():
    d, i = EE.nearest_neighbors(torch.zeros(0, 3, device=DEV), torch.zeros(5, 3, device=DEV))
    assert d.shape == (0,) and i.shape == (0,)
    with pytest.raises(Exception, match="invalid argument"):
        EE.nearest_neighbors(torch.zeros(3, 3, device=DEV), torch.zeros(0, 3, device=DEV))


def _sim_numpy(pp, pd, gp, gd):
    """eval_ABC.py:27-38 with the lowest-index nearest GT point."""
    _, idx = _brute(pp, gp)
    a, b = pd.astype(np.float64), gd[idx].astype(np.float64)
    return float(np.mean(np.abs((a * b).sum(1) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1)))))


@pytest.mark.parametrize("scan", SCANS)
def test_scan_metrics_match_reference(scan):
    gt = torch.from_numpy(G[f"gt_{scan}_all_pts"]).to(DEV)
    sampled = torch.from_numpy(G[f"pred_{scan}_sampled"]).to(DEV)
    ch, acc, comp = EE.chamfer_distance(sampled, gt)
    for k, v in (("chamfer", ch), ("acc", acc), ("comp", comp)):
        assert abs(v - float(G[f"scan_{scan}_{k}"])) <= 1e-6, k
    pr = EE.precision_recall_iou(sampled, gt)
    d_pg = EE.nearest_neighbors(sampled, gt)[0].cpu().numpy()
    d_gp = EE.nearest_neighbors(gt, sampled)[0].cpu().numpy()
    for t, r in pr.items():
        # counts may differ only by the points whose distance is within 1e-6 of the threshold (expected: none)
        near_p, near_g = int((np.abs(d_pg - t) <= 1e-6).sum()), int((np.abs(d_gp - t) <= 1e-6).sum())
        cp_ref = round(float(G[f"scan_{scan}_precision_{t}"]) * len(d_pg))
        cg_ref = round(float(G[f"scan_{scan}_recall_{t}"]) * len(d_gp))
        assert abs(r["correct_pred"] - cp_ref) <= near_p and abs(r["correct_gt"] - cg_ref) <= near_g
        if near_p == 0 and near_g == 0:
            for k, name in (("precision", "precision"), ("recall", "recall"), ("fscore", "fscore"), ("iou", "IOU")):
                ref = float(G[f"scan_{scan}_{name}_{t}"])
                assert (np.isnan(ref) and np.isnan(r[k])) or abs(r[k] - ref) <= 1e-6, f"{k}@{t}"
    for et in ("curve", "line"):
        key = f"scan_{scan}_{et}_counts"
        if key not in G:
            continue
        g2 = torch.from_numpy(G[f"gt_{scan}_{et}_pts"]).to(DEV)
        pr2 = EE.precision_recall_iou(sampled, g2)
        got = ([pr2[t]["correct_gt"] for t in EE.THRESHOLDS] + [pr2[0.005]["num_gt"]] +
               [pr2[t]["correct_pred"] for t in EE.THRESHOLDS] + [pr2[0.005]["num_pred"]])
        np.testing.assert_array_equal(got, G[key])
        _, a2, c2 = EE.chamfer_distance(sampled, g2)
        assert abs(a2 - float(G[f"scan_{scan}_acc_{et}"])) <= 1e-6 and abs(c2 - float(G[f"scan_{scan}_comp_{et}"])) <= 1e-6


@pytest.mark.parametrize("scan", SCANS)
def test_direction_similarity(scan):
    pp = np.concatenate([G[f"pred_{scan}_curve_points"], G[f"pred_{scan}_line_points"]]).reshape(-1, 3).astype(np.float32)
    pd = np.concatenate([G[f"pred_{scan}_curve_dirs"], G[f"pred_{scan}_line_dirs"]]).reshape(-1, 3).astype(np.float32)
    gp, gd = G[f"gt_{scan}_all_pts"], G[f"gt_{scan}_all_dirs"]
    s = EE.direction_similarity(torch.from_numpy(pp).to(DEV), torch.from_numpy(pd).to(DEV), torch.from_numpy(gp).to(DEV),
                                torch.from_numpy(gd).to(DEV))
    assert abs(s - _sim_numpy(pp, pd, gp, gd)) <= 1e-6
    # cKDTree's choice among the duplicated GT vertices is unspecified: the bound is the share of tied pred points
    bound = int(G[f"scan_{scan}_simi_ties"]) / len(pp)
    assert abs(s - float(G[f"scan_{scan}_simi"])) <= bound + 1e-6


def test_evaluate_abc_matches_reference_aggregate():
    m, totals = EE.evaluate_abc(os.path.join(GOLD, "pred"), os.path.join(GOLD, "data"))
    ref = dict(zip([str(k) for k in G["final_keys"]], G["final_values"]))
    assert set(m) == set(ref)
    # both rounded to 4 decimals; the similarity may also move by the mean share of pred points with a tied nearest GT
    # point (cKDTree's choice among duplicated GT vertices is unspecified, see test_direction_similarity)
    n_pred = {s: len(G[f"pred_{s}_curve_points"].reshape(-1, 3)) + len(G[f"pred_{s}_line_points"].reshape(-1, 3)) for s in SCANS}
    tie_share = float(np.mean([int(G[f"scan_{s}_simi_ties"]) / n_pred[s] for s in SCANS]))
    bad = [(k, m[k], v) for k, v in ref.items() if abs(m[k] - v) > 1e-4 + 1e-9 + (tie_share if k == "simi" else 0.0)]
    assert not bad, bad
    tk = [str(k) for k in G["totals_keys"]]
    assert [totals["curve"][k] for k in tk] == G["totals_curve"].tolist()
    assert [totals["line"][k] for k in tk] == G["totals_line"].tolist()
    r = EE.evaluate_abc_scan(os.path.join(GOLD, "pred", SCANS[0], "parametric_edges.json"), os.path.join(GOLD, "groundtruth"),
                             SCANS[0])
    assert abs(r[0]["chamfer"] - float(G[f"scan_{SCANS[0]}_chamfer"])) <= 1e-6


def _downsample_numpy(p, n=256):
    lo, hi = np.zeros(3), np.ones(3)
    p = p.astype(np.float64)
    p = p[((p >= lo) & (p <= hi)).all(1)]
    v = np.minimum(np.floor((p - lo) / ((hi - lo) / n)).astype(np.int64), n - 1)
    keys = {}
    for key, pt in zip(map(tuple, v), p):
        keys.setdefault(key, []).append(pt)
    return np.array([np.mean(keys[k], axis=0) for k in sorted(keys)], np.float32)


def test_downsample_matches_documented_semantics():
    g = np.random.default_rng(3)
    p = np.concatenate([g.random((5000, 3)) * 1.2 - 0.1, g.random((2000, 3)) * 0.01 + 0.3,
                        [[1.0, 1.0, 1.0], [0.0, 0.5, 1.0], [1.0 + 1e-6, 0.5, 0.5]]]).astype(np.float32)
    got = EE.downsample_point_cloud_average(torch.from_numpy(p).to(DEV), 256).cpu().numpy()
    want = _downsample_numpy(p)
    assert got.shape == want.shape
    # as sets: sort both lexicographically
    o1, o2 = np.lexsort(got.T[::-1]), np.lexsort(want.T[::-1])
    np.testing.assert_allclose(got[o1], want[o2], rtol=0, atol=1e-6)
