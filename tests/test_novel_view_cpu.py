"""CPU: the novel-view camera loaders, per-edge colours and the float64 restatement of projection and compositing
against the reference-generated fixture (tests/golden/make_novel_view_golden.py) and hand-computed pixels; argument
checks of the C ABI and of the Python layer; both command lines."""
import os

import numpy as np
import pytest
import torch

from curve_gaussian_amd import _lib
from curve_gaussian_amd.edge_extraction import novel_view as NV
from curve_gaussian_amd.edge_extraction import pred_points_and_directions
from curve_gaussian_amd.scene import colmap_io as CIO

import novel_view_ref64 as R

GOLD = os.path.join(os.path.dirname(__file__), "golden", "novel_view")
G = np.load(os.path.join(GOLD, "novel_view.npz"))
ABC_DATA = os.path.join(GOLD, "abc", "data")
REP_DATA = os.path.join(GOLD, "replica", "data")


def _abc_cams():
    return NV.transforms_video_cameras(os.path.join(ABC_DATA, "00000001"))


def _rep_cams():
    return NV.colmap_cameras(os.path.join(REP_DATA, "room0"))


# ------------------------------------------------------------------------------------------------ camera loaders
def test_transforms_video_cameras_match_reference():
    cams = _abc_cams()
    assert [c.name for c in cams] == list(G["abc_names"])
    for v, c in enumerate(cams):
        np.testing.assert_array_equal(c.R, G["abc_R"][v].T)      # CameraInfo.R is stored transposed
        np.testing.assert_array_equal(c.T, G["abc_T"][v])
        assert (c.width, c.height) == (G["abc_width"][v], G["abc_height"][v])
        assert (c.fx, c.fy, c.cx, c.cy) == (G["abc_fx"][v], G["abc_fy"][v], G["abc_cx"][v], G["abc_cy"][v])
    assert len({(c.width, c.height) for c in cams}) == 2


def test_transforms_video_missing_edge_map_names_the_path(tmp_path):
    import shutil
    scan = tmp_path / "00000001"
    shutil.copytree(os.path.join(ABC_DATA, "00000001"), scan)
    os.remove(scan / "edge_DexiNed" / "r_1.png")
    with pytest.raises(FileNotFoundError, match="edge_DexiNed/r_1.png"):
        NV.transforms_video_cameras(str(scan))
    with pytest.raises(FileNotFoundError, match="edge_PidiNet/r_0.png"):
        NV.transforms_video_cameras(str(scan), "PidiNet")


def test_colmap_cameras_match_reference():
    cams = _rep_cams()
    assert [c.name for c in cams] == list(G["rep_names"])
    for v, c in enumerate(cams):
        np.testing.assert_array_equal(c.R, G["rep_R"][v])
        np.testing.assert_array_equal(c.T, G["rep_T"][v])
        assert (c.fx, c.fy, c.cx, c.cy) == tuple(G["rep_intr"][v])
        assert (c.width, c.height) == (G["rep_W"][v], G["rep_H"][v])


def _scan_with_model(tmp_path, model, params):
    sp = tmp_path / "scan" / "sparse" / "0"
    sp.mkdir(parents=True)
    CIO.write_cameras_binary(str(sp / "cameras.bin"), {3: CIO.ColmapCamera(3, model, 40, 30, np.array(params, float))})
    CIO.write_images_binary(str(sp / "images.bin"), {7: CIO.ColmapImage(7, np.array([1.0, 0, 0, 0]), np.array([0.5, 0, 1]), 3,
                                                                        "a.png", np.zeros((0, 2)), np.zeros(0, np.int64))})
    return str(tmp_path / "scan")


def test_colmap_simple_pinhole_and_other_models(tmp_path):
    (c,) = NV.colmap_cameras(_scan_with_model(tmp_path / "s", "SIMPLE_PINHOLE", [33.5, 20.0, 15.25]))
    assert (c.fx, c.fy, c.cx, c.cy, c.width, c.height, c.name) == (33.5, 33.5, 20.0, 15.25, 40, 30, "a.png")
    np.testing.assert_array_equal(c.R, np.eye(3))
    with pytest.raises(ValueError, match="OPENCV"):
        NV.colmap_cameras(_scan_with_model(tmp_path / "o", "OPENCV", [30, 31, 20, 15, 0.1, 0, 0, 0]))


# ------------------------------------------------------------------------------------------------ projection restatement
def _check_kept(pts, cam, uv_rec, c_rec=None, cols=None):
    keep, u, v = R.project(pts, cam.R, cam.T, cam.fx, cam.fy, cam.cx, cam.cy, cam.width, cam.height)
    got = np.stack([u[keep], v[keep]], 1)
    assert got.shape == uv_rec.shape
    # 1e-12 relative, with the image extent as the scale of coordinates near 0 (the reference's R @ X may use FMAs)
    np.testing.assert_allclose(got, uv_rec, rtol=1e-12, atol=1e-12 * max(cam.width, cam.height))
    if c_rec is not None:
        np.testing.assert_array_equal(cols[keep], c_rec)
    return keep


def test_restated_projection_matches_reference_abc():
    for v, cam in enumerate(_abc_cams()):
        _check_kept(G["abc_points"], cam, G[f"abc_uv_{v}"], G[f"abc_c_{v}"], G["abc_colors"])


def _rep_pred():
    return pred_points_and_directions(os.path.join(GOLD, "replica", "pred", "room0", "parametric_edges.json"),
                                      NV.REPLICA_SAMPLE_RESOLUTION)


def test_restated_projection_and_colours_match_reference_replica():
    pred = _rep_pred()
    pts, cols = pred.points, NV.edge_point_colors(pred, int(G["seed"]))
    for v, cam in enumerate(_rep_cams()):
        if f"rep_uv_{v}" in G:
            _check_kept(pts, cam, G[f"rep_uv_{v}"], G[f"rep_c_{v}"], cols)
        else:
            assert not R.project(pts, cam.R, cam.T, cam.fx, cam.fy, cam.cx, cam.cy, cam.width, cam.height)[0].any()
    assert "rep_uv_1" not in G


def test_colours_match_reference_abc():
    pred = pred_points_and_directions(os.path.join(GOLD, "abc", "pred", "00000001", "parametric_edges.json"))
    pts, cols = pred.points, NV.edge_point_colors(pred, int(G["seed"]))
    for v, cam in enumerate(_abc_cams()):
        _check_kept(pts, cam, G[f"abc_mv_uv_{v}"], G[f"abc_mv_c_{v}"], cols)
    other = NV.edge_point_colors(pred, int(G["seed"]) + 1)
    assert not np.array_equal(other, cols)          # the seed matters


def test_planted_projections_are_exact():
    cam = _rep_cams()[0]
    pl = G["rep_planted"].reshape(-1, 3)
    keep, u, v = R.project(pl, cam.R, cam.T, cam.fx, cam.fy, cam.cx, cam.cy, cam.width, cam.height)
    W, H = cam.width, cam.height
    exp_u = [0.0, 0.3125, W - 2.0 ** -10, W - 2.0 ** -10 - 0.3125, W, W - 0.3125]
    np.testing.assert_array_equal(u[:6], exp_u)
    np.testing.assert_array_equal(keep[:6], [1, 1, 1, 1, 0, 1])
    np.testing.assert_array_equal(v[[6, 8, 9, 10, 11]], [0.0, H - 2.0 ** -10, H - 2.0 ** -10 - 0.3125, H, H - 0.3125])
    np.testing.assert_array_equal(keep[6:12], [1, 1, 1, 1, 0, 1])
    np.testing.assert_array_equal(keep[14:18], [0, 1, 0, 0])             # depth 0 / its partner, depth -0.25 pair
    assert (u[15], v[15]) == (cam.cx, cam.cy)
    # the recorded kept set holds these exact values
    rec = G["rep_uv_0"]
    for uu, vv in ((0.0, 10.0), (W - 2.0 ** -10, 12.0), (20.0, 0.0), (22.0, H - 2.0 ** -10)):
        assert ((rec[:, 0] == uu) & (rec[:, 1] == vv)).sum() == 1
    assert not ((rec[:, 0] == W) | (rec[:, 1] == H)).any()


# ------------------------------------------------------------------------------------------------ compositing restatement
@pytest.mark.parametrize("alpha", [0.5, 1.0, 0.1])
def test_composite_restatement_hand_computed(alpha):
    bg = np.array([1.0, 0.75, 0.25])
    c = np.array([[0.2, 0.4, 0.6], [0.9, 0.1, 0.3]] + [[0.5, 0.5, 0.5]] * 28 + [[0.0, 1.0, 0.0]])
    # pixel 0: point 0; pixel 1: points 1, 2; pixel 3: points 3..32 (30 points); pixel 2 empty
    pix = np.array([0, 1, 1] + [3] * 30)
    cols = np.concatenate([c[:1], c[1:3], np.concatenate([[c[0]], c[3:30], [c[-1]], [c[1]]])])
    out = R.composite(pix, cols, alpha, bg, 4)
    a, om = alpha, 1 - alpha
    np.testing.assert_allclose(out[0], bg * om + a * c[0], rtol=0, atol=1e-15)
    np.testing.assert_allclose(out[1], bg * om ** 2 + a * om * c[1] + a * c[2], rtol=0, atol=1e-15)
    np.testing.assert_array_equal(out[2], bg)
    # 30 points: first c[0] (r = 29), 27 grey (r = 28..2), then green (r = 1), then c[1] (r = 0)
    grey = sum(a * om ** r for r in range(2, 29)) * 0.5
    exp = bg * om ** 30 + a * om ** 29 * c[0] + grey + a * om * np.array([0.0, 1.0, 0.0]) + a * c[1]
    np.testing.assert_allclose(out[3], exp, rtol=0, atol=1e-14)
    # the order of the points matters
    rev = R.composite(pix[::-1], cols[::-1], alpha, bg, 4)
    assert not np.allclose(rev[1], out[1])
    if alpha == 1.0:
        np.testing.assert_array_equal(out[3], c[1])


def test_keep_cut_bound():
    """The kernel composites the newest K points, K = min{k : (1-a)^k <= 2^-25}: the restatement with the tail dropped
    differs from the full one by at most 2^-25."""
    rng = np.random.default_rng(3)
    for alpha, K in ((0.5, 25), (0.1, 165), (1.0, 1)):
        om = 1 - alpha
        assert om ** K <= 2.0 ** -25 and (K == 1 or om ** (K - 1) > 2.0 ** -25)
        n = 400
        cols = rng.uniform(0, 1, (n, 3))
        full = R.composite(np.zeros(n, np.int64), cols, alpha, np.ones(3), 1)
        w = alpha * om ** np.arange(K)[::-1]
        cut = np.ones(3) * om ** n + (w[:, None] * cols[-K:]).sum(0)
        assert np.abs(full - cut).max() <= 2.0 ** -25


# ------------------------------------------------------------------------------------------------ argument checks
def _lib_or_skip():
    return _lib.load()


def test_abi_rejects_invalid_arguments_without_a_gpu():
    import ctypes
    lib = _lib_or_skip()
    bg = (ctypes.c_double * 3)(1, 1, 1)
    d = ctypes.c_void_p(8)
    assert lib.cgs_project_points(-1, None, 1, None, None, 4, 4, None, None) == -1
    assert b"invalid argument" in lib.cgs_last_error()
    assert lib.cgs_project_points(5, None, 2, None, None, 0, 4, None, None) == -1
    assert lib.cgs_project_points(5, None, 2, None, None, 4, 4, None, None) == -1
    assert b"NULL" in lib.cgs_last_error()
    assert lib.cgs_project_points(0, None, 2, None, None, 4, 4, None, None) == 0      # P = 0: no-op
    assert lib.cgs_project_points(3, None, 0, None, None, 4, 4, None, None) == 0      # V = 0: no-op
    ws1 = lib.cgs_render_points_workspace_bytes(100, 1, 8, 8)
    assert ws1 >= 2 * 64 * 4 + 100 * 4
    assert lib.cgs_render_points_workspace_bytes(100, 4, 8, 8) > ws1
    args = lambda P, V, H, W, a, ws_bytes, ptr=d: (P, ptr, ptr, V, ptr, ptr, H, W, a, bg, ptr, None, ptr, ws_bytes, None)
    assert lib.cgs_render_points(*args(-1, 1, 8, 8, 0.5, ws1)) == -1
    assert lib.cgs_render_points(*args(100, 1, 0, 8, 0.5, ws1)) == -1
    assert lib.cgs_render_points(*args(100, 1, 8, 8, 1.5, ws1)) == -1
    assert b"alpha" in lib.cgs_last_error()
    assert lib.cgs_render_points(*args(100, 1, 8, 8, float("nan"), ws1)) == -1
    assert lib.cgs_render_points(*args(100, 2, 8, 8, 0.5, ws1 - 1)) == -1
    assert b"workspace" in lib.cgs_last_error()
    assert lib.cgs_render_points(*args(100, 2, 8, 8, 0.5, ws1, None)) == -1
    assert b"NULL" in lib.cgs_last_error()
    assert lib.cgs_render_points(*args(100, 0, 8, 8, 0.5, 0, None)) == 0              # V = 0: no-op


def test_cpu_tensors_raise():
    pts = torch.zeros(4, 3)
    intr, w2c = NV.camera_arrays(_rep_cams())
    with pytest.raises(_lib.CurveGSError, match="GPU tensor"):
        NV.project_points(pts, intr, w2c, 48, 64)
    with pytest.raises(_lib.CurveGSError, match="GPU tensor"):
        NV.render_points(pts, torch.zeros(4, 3), intr, w2c, 48, 64)


# ------------------------------------------------------------------------------------------------ command lines
def test_edge_extraction_command_line():
    from curve_gaussian_amd.edge_extraction import __main__ as M
    a = M.parser().parse_args(["--dataset_dir", "d"])
    assert (a.base_dir, a.dataset_dir, a.render_mv) == ("./output", "d", False)
    a = M.parser().parse_args(["--base_dir", "b", "--dataset_dir", "d", "--render_mv"])
    assert (a.base_dir, a.dataset_dir, a.render_mv) == ("b", "d", True)


def test_replica_command_line_and_scan_list(tmp_path):
    from curve_gaussian_amd.edge_extraction import replica as RP
    a = RP.parser().parse_args(["--dataset_dir", "d"])
    assert (a.base_dir, a.dataset_dir, a.scans) == ("./output/replica/", "d", None)
    a = RP.parser().parse_args(["--base_dir", "b", "--dataset_dir", "d", "--scans", "s.txt"])
    assert (a.base_dir, a.scans) == ("b", "s.txt")
    with pytest.raises(SystemExit):
        RP.parser().parse_args(["--base_dir", "b"])
    assert NV.replica_scans(REP_DATA) == ["room0"]
    (tmp_path / "room1" / "sparse" / "0").mkdir(parents=True)
    (tmp_path / "room0" / "sparse").mkdir(parents=True)          # no sparse/0: not a scan
    (tmp_path / "office2" / "sparse" / "0").mkdir(parents=True)
    assert NV.replica_scans(str(tmp_path)) == ["office2", "room1"]
    (tmp_path / "list.txt").write_text("room0\n\noffice2\n")
    assert NV.replica_scans(str(tmp_path), str(tmp_path / "list.txt")) == ["room0", "office2"]
