"""Host: the depth gate on the drawn views (edge_extraction.novel_view: project_points_depth with backend="host", the
depth arguments of the scan drivers) -- against the float64 restatement of the ungated projection (novel_view_ref64) and the
per-pair loop of edge_visgate_cases.py."""
import numpy as np
import pytest
import torch

import edge_visgate_cases as C
import novel_view_ref64 as R
from curve_gaussian_amd import _lib
from curve_gaussian_amd.edge_extraction import novel_view as NV
from curve_gaussian_amd.ops import edge_occlusion as EO


@pytest.mark.parametrize("P,V,slack", [(1, 1, 0.0), (255, 3, 0.001), (400, 2, 0.05)])
def test_host_projection_splits_the_ungated_keep_into_seen_and_hidden(P, V, slack):
    pts, _ = C.view_points(P, seed=P)
    intr, w2c = C.view_cameras(V, seed=V)
    planes = C.view_planes(V, seed=P + V)
    uv, hidden = NV.project_points_depth(pts, intr, w2c, planes, slack, return_hidden=True, backend="host")
    assert uv.dtype == torch.float64 and tuple(uv.shape) == (V, P, 2)
    assert hidden.dtype == torch.uint8 and tuple(hidden.shape) == (V, P)
    uv, hidden = uv.numpy(), hidden.numpy().astype(bool)
    seen = ~np.isnan(uv[..., 0])
    np.testing.assert_array_equal(np.isnan(uv[..., 0]), np.isnan(uv[..., 1]))
    want_seen, want_hidden = C.hidden_brute(pts, intr, w2c.reshape(V, 12), planes, slack)
    np.testing.assert_array_equal(hidden, want_hidden)
    np.testing.assert_array_equal(seen, want_seen)
    for i in range(V):
        keep, u, v = R.project(pts, w2c[i, :, :3], w2c[i, :, 3], *intr[i], C.W, C.H)
        np.testing.assert_array_equal(seen[i] | hidden[i], keep)
        assert not (seen[i] & hidden[i]).any()
        np.testing.assert_array_equal(uv[i, seen[i], 0], u[seen[i]])
        np.testing.assert_array_equal(uv[i, seen[i], 1], v[seen[i]])
    if P > 1:
        assert hidden.any() and seen.any(), "the case has both verdicts"
    only = NV.project_points_depth(pts, intr, w2c, planes, slack, backend="host")
    np.testing.assert_array_equal(np.isnan(only.numpy()), np.isnan(uv))


def test_an_all_inf_plane_hides_nothing_and_a_nan_plane_neither():
    pts, _ = C.view_points(300)
    intr, w2c = C.view_cameras(2)
    for fill in (np.inf, np.nan):
        uv, hidden = NV.project_points_depth(pts, intr, w2c, np.full((2, C.H, C.W), fill, np.float32), 0.0,
                                             return_hidden=True, backend="host")
        assert not hidden.any()
        for i in range(2):
            keep, _, _ = R.project(pts, w2c[i, :, :3], w2c[i, :, 3], *intr[i], C.W, C.H)
            np.testing.assert_array_equal(~np.isnan(uv[i, :, 0].numpy()), keep)


def test_argument_checks():
    pts, col = C.view_points(4)
    intr, w2c = C.view_cameras(2)
    planes = C.view_planes(2)
    with pytest.raises(ValueError, match="slack"):
        NV.project_points_depth(pts, intr, w2c, planes, -0.1, backend="host")
    with pytest.raises(ValueError, match="depth must be float32"):
        NV.project_points_depth(pts, intr, w2c, planes[:1], 0.0, backend="host")
    with pytest.raises(ValueError, match="depth must be float32"):
        NV.project_points_depth(pts, intr, w2c, planes.astype(np.float64), 0.0, backend="host")
    with pytest.raises(ValueError, match="backend"):
        NV.project_points_depth(pts, intr, w2c, planes, 0.0, backend="cpu")
    with pytest.raises(_lib.CurveGSError, match="GPU tensor"):   # GPU only, like render_points
        NV.render_points_depth(torch.from_numpy(pts), torch.from_numpy(col), intr, w2c, planes, 0.0)
    with pytest.raises(_lib.CurveGSError, match="GPU tensor"):   # the existing entries as they were
        NV.project_points(torch.from_numpy(pts), intr, w2c, C.H, C.W)
    with pytest.raises(_lib.CurveGSError, match="GPU tensor"):
        NV.render_points(torch.from_numpy(pts), torch.from_numpy(col), intr, w2c, C.H, C.W)


def test_scan_depth_of_the_drivers(tmp_path):
    cams = [NV.NovelViewCamera("a.png", np.eye(3), np.zeros(3), 10.0, 10.0, 8.0, 6.0, C.W, C.H)]
    assert NV.scan_depth("t", str(tmp_path), cams) is None
    with pytest.raises(ValueError, match="not both"):
        NV.scan_depth("t", str(tmp_path), cams, occluder="mesh.ply", depth_dir="depth")
    with pytest.raises(ValueError, match="near_clip needs an occluder"):
        NV.scan_depth("t", str(tmp_path), cams, depth_dir="depth", near_clip=0.01)
    with pytest.raises(FileNotFoundError, match="a.npy"):
        NV.scan_depth("t", str(tmp_path), cams, depth_dir="depth")
    (tmp_path / "depth").mkdir()
    np.save(tmp_path / "depth" / "a.npy", np.full((C.H, C.W), 2.0, np.float32))
    EO.write_triangle_ply(str(tmp_path / "mesh.ply"), np.zeros((1, 3, 3), np.float32))
    gate = NV.scan_depth("t", str(tmp_path), cams, depth_dir="depth", depth_slack=0.01, depth_window=2)
    assert gate.gated and gate.settings() == {"depth_maps": True, "depth_slack": 0.01, "depth_window": 2}
    gate = NV.scan_depth("t", str(tmp_path), cams, occluder="mesh.ply", near_clip=0.02)
    assert gate.settings()["occluder"] == str(tmp_path / "mesh.ply") and gate.settings()["near_clip"] == 0.02
    assert NV.VISIBLE_DIR == "novel_view_visible"
