"""CPU: the host back end of ops.edge_score (distance transform against brute force and scipy, hand-made scores, argument
errors) and edge_extraction.reprojection on tiny synthetic scans (score_scan, its JSON, the command line)."""
import json
import math
import os

import numpy as np
import pytest
import torch

import edge_score_cases as SC
from curve_gaussian_amd.edge_extraction import reprojection as RP
from curve_gaussian_amd.ops import edge_score as ES


def test_constants_match_the_header():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "curvegs.h")).read()
    assert f"#define CGS_EDT_INF {ES.EDT_INF} " in header and ES.EDT_INF == SC.EDT_INF == 2 ** 31 - 1
    assert f"#define CGS_EDT_MAX_SIZE {ES.L.EDT_MAX_SIZE}\n" in header
    assert f"#define CGS_EDGE_SCORE_MAX_TOL {ES.L.EDGE_SCORE_MAX_TOL}\n" in header


@pytest.mark.parametrize("name", sorted(SC.edt_views()))
def test_host_edt_equals_brute_force(name):
    mask = SC.edt_views()[name]
    got = ES.edt_squared(mask[None], backend="host")
    assert got.dtype == torch.int32 and tuple(got.shape) == (1,) + mask.shape
    assert np.array_equal(got[0].numpy(), SC.edt_brute(mask))
    if name.endswith("_empty"):
        assert (got == ES.EDT_INF).all()
    if name.endswith("_full"):
        assert (got == 0).all()


@pytest.mark.parametrize("name", sorted(n for n, m in SC.edt_views().items() if m.any()))   # (scipy defines no empty case)
def test_host_edt_equals_scipy(name):
    ndi = pytest.importorskip("scipy.ndimage")
    mask = SC.edt_views()[name]
    want = np.rint(ndi.distance_transform_edt(mask == 0) ** 2).astype(np.int64)
    assert np.array_equal(ES.edt_squared(mask[None], backend="host")[0].numpy().astype(np.int64), want)


def test_host_edt_takes_bool_and_stacks():
    stack = SC.edt_stacks()["37x70_random"]
    got = ES.edt_squared(torch.from_numpy(stack).bool(), backend="host")
    for v in range(3):
        assert np.array_equal(got[v].numpy(), SC.edt_brute(stack[v]))


def _line_mask(H, W, x, y0, y1):
    m = np.zeros((H, W), np.uint8)
    m[y0:y1, x] = 1
    return m


def test_identical_masks_score_one():
    pred, _ = SC.score_stack()
    pred[1] = pred[0]   # (no empty view here)
    res = ES.score_masks(pred, pred.copy(), (1, 2, 4), backend="host")
    a = res["aggregate"]
    assert a["precision"] == [1.0, 1.0, 1.0] and a["recall"] == [1.0, 1.0, 1.0] and a["fscore"] == [1.0, 1.0, 1.0]
    assert a["accuracy_px"] == 0.0 and a["completeness_px"] == 0.0 and a["chamfer_px"] == 0.0
    assert a["chamfer_views"] == a["views"] == pred.shape[0]
    assert torch.equal(res["n_pred"], res["n_det"]) and torch.equal(res["pred_hits"][:, 0], res["n_pred"])


def test_a_shift_of_three_pixels():
    """A vertical line and the same line 3 px to the right, both inside the image: every pixel's nearest neighbour in the
    other mask is its own row's, 3 px away."""
    pred = _line_mask(30, 40, 10, 5, 25)[None]
    det = _line_mask(30, 40, 13, 5, 25)[None]
    res = ES.score_masks(pred, det, (1, 2, 4), backend="host")
    a = res["aggregate"]
    assert a["precision"] == [0.0, 0.0, 1.0] and a["recall"] == [0.0, 0.0, 1.0] and a["fscore"] == [0.0, 0.0, 1.0]
    assert a["accuracy_px"] == 3.0 and a["completeness_px"] == 3.0 and a["chamfer_px"] == 6.0 and a["chamfer_views"] == 1
    assert res["n_pred"].tolist() == [20] and res["det_hits"].tolist() == [[0, 0, 20]]
    assert res["sum_pred_to_det"].tolist() == [60.0]


def test_an_empty_prediction():
    det = _line_mask(30, 40, 13, 5, 25)[None]
    res = ES.score_masks(np.zeros_like(det), det, (1, 2, 4), backend="host")
    a = res["aggregate"]
    assert a["recall"] == [0.0, 0.0, 0.0] and all(math.isnan(p) for p in a["precision"])
    assert all(math.isnan(f) for f in a["fscore"])
    assert a["chamfer_views"] == 0 and math.isnan(a["accuracy_px"]) and math.isnan(a["chamfer_px"])
    assert res["both_nonempty"].tolist() == [False] and res["n_det"].tolist() == [20] and res["n_pred"].tolist() == [0]
    # next to a scored view, the empty one counts its pixels but stays out of the Chamfer terms
    pred2 = np.concatenate([np.zeros_like(det), det])
    res2 = ES.score_masks(pred2, np.concatenate([det, det]), (1,), backend="host")
    a2 = res2["aggregate"]
    assert a2["recall"] == [0.5] and a2["precision"] == [1.0] and a2["fscore"] == [2 * 0.5 / 1.5]
    assert a2["chamfer_views"] == 1 and a2["completeness_px"] == 0.0 and a2["accuracy_px"] == 0.0
    assert res2["sum_det_to_pred"].tolist() == [0.0, 0.0] and res2["det_hits"].tolist() == [[0], [20]]


def test_both_empty_everywhere_gives_nan_not_an_exception():
    z = np.zeros((2, 5, 6), np.uint8)
    a = ES.score_masks(z, z, (1, 2), backend="host")["aggregate"]
    assert all(math.isnan(x) for x in a["precision"] + a["recall"] + a["fscore"]) and a["chamfer_views"] == 0


def test_host_chunking_changes_nothing():
    pred, det = SC.score_stack()
    whole = ES.score_masks(pred, det, (1, 2.5, 4), backend="host")
    single = ES.score_masks(pred, det, (1, 2.5, 4), backend="host", budget_bytes=1)
    for k, v in whole.items():
        assert (v == single[k]) if k == "aggregate" else torch.equal(v, single[k]), k
    assert whole["both_nonempty"].tolist() == [True, False, False, True]


def test_host_point_masks_edge_cases():
    intr, w2c = SC.mask_cameras()
    pts = SC.mask_points()
    mask, kept = ES.point_masks(pts, intr, w2c, SC.MASK_H, SC.MASK_W, backend="host", return_kept=True)
    assert mask.dtype == torch.uint8 and tuple(mask.shape) == (3, SC.MASK_H, SC.MASK_W) and int(mask.max()) == 1
    assert all(0 < int(k) < len(pts) for k in kept)
    third = mask[2].numpy()
    assert third[3, 0] == 1 and third[0, 5] == 1              # on u = 0 and on v = 0: kept
    one = ES.point_masks(np.array([[SC.MASK_W, 3.0, 1.0], [5.0, SC.MASK_H, 1.0], [5.0, 5.0, -1.0], [1.0, 1.0, 0.0]], np.float32),
                         intr[2:], w2c[2:], SC.MASK_H, SC.MASK_W, backend="host", return_kept=True)
    assert int(one[0].sum()) == 0 and one[1].tolist() == [0]   # u = width, v = height, behind, at the eye: dropped
    # several points in one pixel: fewer set pixels than kept points
    assert int(mask[0].sum()) < int(kept[0])


def test_argument_errors():
    m = np.zeros((1, 4, 5), np.uint8)
    for fn in (lambda: ES.edt_squared(m, backend="cpu"), lambda: ES.score_masks(m, m, backend="cuda"),
               lambda: ES.point_masks(np.zeros((1, 3), np.float32), np.zeros((1, 4)), np.zeros((1, 3, 4)), 4, 5, backend="x")):
        with pytest.raises(ValueError, match="unknown edge score backend"):
            fn()
    with pytest.raises(ValueError, match="unknown edge score backend"):
        RP.score_edges(SC.SCAN_EDGES, [], [], "PidiNet", backend="numpy")
    with pytest.raises(ValueError, match=r"uint8 or bool \[V,H,W\]"):
        ES.edt_squared(np.zeros((4, 5), np.uint8), backend="host")
    with pytest.raises(ValueError, match=r"uint8 or bool \[V,H,W\]"):
        ES.edt_squared(np.zeros((1, 4, 5), np.float32), backend="host")
    with pytest.raises(ValueError, match="differ in shape"):
        ES.score_masks(m, np.zeros((1, 5, 4), np.uint8), backend="host")
    with pytest.raises(ValueError, match="at most 8 tolerances"):
        ES.score_masks(m, m, tuple(range(9)), backend="host")
    with pytest.raises(ValueError, match="a tolerance must lie"):
        ES.score_masks(m, m, (-1,), backend="host")
    with pytest.raises(ValueError, match="budget_bytes must be positive"):
        ES.score_masks(m, m, backend="host", budget_bytes=0)
    with pytest.raises(ValueError, match=r"height and width must lie in \[1, 16384\]"):
        ES.point_masks(np.zeros((1, 3), np.float32), np.zeros((1, 4)), np.zeros((1, 3, 4)), 0, 5, backend="host")
    with pytest.raises(ValueError, match=r"height and width must lie in \[1, 16384\]"):
        ES.edt_squared(np.zeros((1, 1, 16385), np.uint8), backend="host")
    with pytest.raises(ValueError, match=r"intrinsics must be \[V,4\]"):
        ES.point_masks(np.zeros((1, 3), np.float32), np.zeros((1, 3)), np.zeros((1, 3, 4)), 4, 5, backend="host")
    with pytest.raises(ValueError, match="Unknown detector"):
        RP.detected_lut("Canny", 0.5)


def test_c_abi_rejects_bad_arguments_without_a_gpu():
    from curve_gaussian_amd import _lib as L
    lib = L.load()
    assert lib.cgs_edt_squared(0, 4, 4, None, None, None, None) == 0           # V = 0 is a no-op
    assert lib.cgs_edt_squared(1, 4, 16385, None, None, None, None) == -1 and b"cgs_edt_squared" in lib.cgs_last_error()
    assert lib.cgs_edt_squared(1, 0, 4, None, None, None, None) == -1
    assert lib.cgs_edt_squared(1, 4, 4, None, None, None, None) == -1 and b"NULL" in lib.cgs_last_error()
    assert lib.cgs_point_mask(-1, None, 1, None, None, 4, 4, None, None, None) == -1
    assert lib.cgs_point_mask(0, None, 0, None, None, 4, 4, None, None, None) == 0
    assert lib.cgs_point_mask(1, None, 1, None, None, 4, 4, None, None, None) == -1
    assert lib.cgs_edge_score_reduce(1, 4, 4, None, None, None, None, 9, None, None, None, None, None, None) == -1
    assert lib.cgs_edge_score_reduce(0, 4, 4, None, None, None, None, 0, None, None, None, None, None, None) == 0
    assert lib.cgs_edt_workspace_bytes(3, 10, 20) >= 3 * 10 * 20 * 2 and lib.cgs_edge_score_workspace_bytes(2) > 0


def test_detected_lut_uses_para_edges_conversions():
    from curve_gaussian_amd.edge_extraction.para_edge import EDGE_MAX_THRESHOLD
    dex, pidi = RP.detected_lut("DexiNed", EDGE_MAX_THRESHOLD), RP.detected_lut("PidiNet", EDGE_MAX_THRESHOLD)
    assert dex[:127].all() and not dex[128:].any() and dex[127] == (1 - 127 / 255.0 > 0.5)
    assert pidi[128:].all() and not pidi[:128].any()


@pytest.mark.parametrize("layout, detector", [("colmap", "DexiNed"), ("emap", "PidiNet")])
def test_score_scan_on_a_drawn_scan(tmp_path, layout, detector):
    base, data = SC.write_scan(tmp_path, layout, detector)
    res = RP.score_scan(base, data, "room", layout=layout, detector=detector, sample_resolution=SC.SCAN_RESOLUTION,
                        backend="host")
    a = res["aggregate"]
    assert a["tolerances_px"] == [1.0, 2.0, 4.0]
    assert a["fscore"][0] == 1.0 and a["precision"][0] == 1.0 and a["recall"][0] == 1.0
    assert a["chamfer_px"] <= 2.0 and a["chamfer_views"] == a["views"] == SC.SCAN_VIEWS
    with open(os.path.join(base, "room", "reprojection_score.json")) as f:
        saved = json.load(f)
    assert set(saved) == {"scan", "aggregate", "views", "settings"} and saved["scan"] == "room"
    assert set(saved["aggregate"]) == {"tolerances_px", "precision", "recall", "fscore", "accuracy_px", "completeness_px",
                                       "chamfer_px", "chamfer_views", "views", "n_pred", "n_det"}
    assert saved["aggregate"] == a
    names = [r["name"] for r in saved["views"]]
    assert names == ([f"{i:05d}.png" for i in range(3)] if layout == "colmap" else [f"{i}_colors.png" for i in range(3)])
    assert set(saved["views"][0]) == {"name", "width", "height", "kept_points", "n_pred", "n_det", "pred_hits", "det_hits",
                                      "accuracy_px", "completeness_px", "both_nonempty"}
    assert saved["views"][0]["width"] == SC.SCAN_W and saved["views"][0]["n_pred"] > 20
    assert saved["settings"] == {"detector": detector, "tolerances_px": [1.0, 2.0, 4.0], "edge_threshold": 0.5,
                                 "sample_resolution": SC.SCAN_RESOLUTION, "backend": "host", "points": saved["settings"]["points"],
                                 "layout": layout, "undistort": False}


def test_a_wrong_prediction_scores_low(tmp_path):
    """The same scan with the prediction moved: the score must see it (a score that is always 1 measures nothing)."""
    base, data = SC.write_scan(tmp_path, "emap", "PidiNet")
    moved = {k: (np.array(v).reshape(-1, 3) + [0.0, 0.0, 0.15]).reshape(np.array(v).shape).tolist() for k, v in SC.SCAN_EDGES.items()}
    with open(os.path.join(base, "room", "parametric_edges.json"), "w") as f:
        json.dump(moved, f)
    a = RP.score_scan(base, data, "room", layout="emap", detector="PidiNet", sample_resolution=SC.SCAN_RESOLUTION,
                      backend="host")["aggregate"]
    assert a["fscore"][0] < 0.5 and a["accuracy_px"] > 1.0


def test_cli_skips_a_scan_without_prediction(tmp_path, capsys):
    base, data = SC.write_scan(tmp_path, "emap", "PidiNet", scan="a_scored")
    SC.write_scan(tmp_path, "emap", "PidiNet", scan="b_missing", with_prediction=False)
    rc = RP.main(["--base_dir", base, "--dataset_dir", data, "--layout", "emap", "--detector", "PidiNet", "--backend", "host",
                  "--tolerances", "1", "2"])
    out = capsys.readouterr().out
    assert rc == 0
    assert "Invalid prediction at b_missing" in out and "a_scored: views 3" in out and "b_missing:" not in out
    assert "Summary (mean over 1 scans):" in out and "F-Score @ 1 px:" in out and "Chamfer:" in out
    assert os.path.exists(os.path.join(base, "a_scored", "reprojection_score.json"))
    assert not os.path.exists(os.path.join(base, "b_missing", "reprojection_score.json"))


def test_train_flag_is_off_by_default():
    from curve_gaussian_amd import train as T
    assert T.build_parser().parse_args([]).reprojection_score is False
    assert T.build_parser().parse_args(["--reprojection_score"]).reprojection_score is True


def test_score_scene_splits_train_and_test(tmp_path):
    """What the driver's --reprojection_score calls: the scene's train and test cameras scored separately."""
    from curve_gaussian_amd.scene import colmap_io as CIO
    base, data = SC.write_scan(tmp_path, "colmap", "DexiNed")
    train, test, _, _ = CIO.read_colmap(os.path.join(data, "room"), eval=True, llffhold=2, detector="DexiNed")

    class FakeScene:
        def getTrainCameras(self):
            return train

        def getTestCameras(self):
            return test
    model = os.path.join(base, "room")
    out = RP.score_scene(model, FakeScene(), "DexiNed", sample_resolution=SC.SCAN_RESOLUTION, backend="host")
    assert out["train"]["aggregate"]["views"] == 3 and out["test"]["aggregate"]["views"] == 2
    assert out["train"]["aggregate"]["fscore"][0] == 1.0 and out["test"]["aggregate"]["fscore"][0] == 1.0
    with open(os.path.join(model, "reprojection_score.json")) as f:
        assert set(json.load(f)) == {"train", "test"}
