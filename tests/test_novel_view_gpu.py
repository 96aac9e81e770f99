"""GPU: the novel-view kernels (cgs_project_points / cgs_render_points) against the reference-generated fixture
(tests/golden/make_novel_view_golden.py) and the float64 restatement (tests/novel_view_ref64.py, itself pinned by
tests/test_novel_view_cpu.py), and both drivers end to end."""
import os
import shutil

import numpy as np
import pytest
import torch
from PIL import Image

from curve_gaussian_amd.edge_extraction import novel_view as NV
from curve_gaussian_amd.edge_extraction import pred_points_and_directions

import novel_view_ref64 as R

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden", "novel_view")
G = np.load(os.path.join(GOLD, "novel_view.npz"))
ABC_DATA = os.path.join(GOLD, "abc", "data")
REP_DATA = os.path.join(GOLD, "replica", "data")
DEV = torch.device("cuda:0")
SEED = int(G["seed"])


def _rep():
    pred = pred_points_and_directions(os.path.join(GOLD, "replica", "pred", "room0", "parametric_edges.json"),
                                      NV.REPLICA_SAMPLE_RESOLUTION)
    return pred.points, NV.edge_point_colors(pred, SEED), NV.colmap_cameras(os.path.join(REP_DATA, "room0"))


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(DEV)


def _kept(uv):
    return ~np.isnan(uv[:, 0])


def test_project_points_reproduces_the_reference():
    # ABC: project_points_to_camera on the reference's own cameras; views of two sizes, one call per size
    cams = NV.transforms_video_cameras(os.path.join(ABC_DATA, "00000001"))
    pts = G["abc_points"]
    for v, c in enumerate(cams):
        intr, w2c = NV.camera_arrays([c])
        uv = NV.project_points(_dev(pts), intr, w2c, c.height, c.width)[0].cpu().numpy()
        k = _kept(uv)
        assert np.isnan(uv[~k]).all()
        rec = G[f"abc_uv_{v}"]
        assert k.sum() == len(rec)
        np.testing.assert_allclose(uv[k], rec, rtol=1e-12, atol=1e-12 * max(c.width, c.height))
        np.testing.assert_array_equal(G["abc_colors"][k], G[f"abc_c_{v}"])
    # Replica: process_scan's kept sets, the planted boundary cases bit-exact
    pts, cols, cams = _rep()
    same = [v for v, c in enumerate(cams) if (c.width, c.height) == (cams[0].width, cams[0].height)]
    assert len(same) == 4
    intr, w2c = NV.camera_arrays([cams[v] for v in same])
    uv = NV.project_points(_dev(pts), intr, w2c, cams[0].height, cams[0].width).cpu().numpy()
    for v, c in enumerate(cams):
        if v not in same:
            continue
        u = uv[same.index(v)]
        k = _kept(u)
        if f"rep_uv_{v}" not in G:
            assert not k.any()
            continue
        rec = G[f"rep_uv_{v}"]
        assert k.sum() == len(rec)
        np.testing.assert_allclose(u[k], rec, rtol=1e-12, atol=1e-12 * max(c.width, c.height))
        np.testing.assert_array_equal(cols[k], G[f"rep_c_{v}"])
    pl = G["rep_planted"].reshape(-1, 3)
    c0 = cams[0]
    up = NV.project_points(_dev(pl), *NV.camera_arrays([c0]), c0.height, c0.width)[0].cpu().numpy()
    keep, u, v = R.project(pl, c0.R, c0.T, c0.fx, c0.fy, c0.cx, c0.cy, c0.width, c0.height)
    np.testing.assert_array_equal(_kept(up), keep)
    np.testing.assert_array_equal(up[keep], np.stack([u[keep], v[keep]], 1))     # bit for bit
    assert keep[:6].tolist() == [True, True, True, True, False, True]


def _ref_images(pts, cols, cams, alpha, bg=(1.0, 1.0, 1.0)):
    return [R.render(pts, cols, c.R, c.T, c.fx, c.fy, c.cx, c.cy, c.width, c.height, alpha, bg) for c in cams]


@pytest.mark.parametrize("alpha", [0.5, 1.0, 0.1])
def test_render_points_fixture(alpha):
    pts, cols, cams = _rep()
    for size in {(c.height, c.width) for c in cams}:
        sel = [c for c in cams if (c.height, c.width) == size]
        bg = (1.0, 0.5, 0.0)
        out, kept = NV.render_points(_dev(pts), _dev(cols), *NV.camera_arrays(sel), *size, alpha, bg, return_kept=True)
        out = out.cpu().numpy()
        assert out.shape == (len(sel),) + size + (3,) and out.dtype == np.float32
        for k, (ref, n) in enumerate(_ref_images(pts, cols, sel, alpha, bg)):
            assert int(kept[k]) == n
            assert np.abs(out[k] - ref).max() <= 4e-6


def _random_scene(P, V, seed=7):
    g = np.random.default_rng(seed)
    pts = g.uniform(-0.5, 0.5, (P, 3))
    pts[: P // 200] = 0.02 + g.normal(0, 2e-5, (P // 200, 3))      # a knot: > 1000 points in one pixel of most views
    pts = pts.astype(np.float32)
    cols = g.uniform(0, 1, (P, 3)).astype(np.float32)
    cams = []
    for v in range(V):
        a, b = g.uniform(-0.4, 0.4, 2)
        Ry = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        Rx = np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]])
        Rm = Ry @ Rx
        T = np.array([0.0, 0.0, 2.0]) + g.uniform(-0.1, 0.1, 3)
        f = g.uniform(150, 220)
        cams.append(NV.NovelViewCamera(f"v{v}", Rm, T, f, f * g.uniform(0.95, 1.05), 160 + g.uniform(-3, 3),
                                       120 + g.uniform(-3, 3), 320, 240))
    return pts, cols, cams


def test_render_points_random_scene_deterministic_and_chunked():
    P, V = 2_000_000, 48
    pts, cols, cams = _random_scene(P, V)
    dp, dc = _dev(pts), _dev(cols)
    intr, w2c = NV.camera_arrays(cams)
    # reference grouping once per view (independent of alpha)
    groups = []
    for c in cams:
        keep, u, v = R.project(pts, c.R, c.T, c.fx, c.fy, c.cx, c.cy, c.width, c.height)
        groups.append((np.floor(v[keep]).astype(np.int64) * c.width + np.floor(u[keep]).astype(np.int64), keep))
    assert max(np.bincount(p).max() for p, _ in groups) > 1000
    for alpha in (0.5, 1.0, 0.1):
        out = NV.render_points(dp, dc, intr, w2c, 240, 320, alpha)
        for v, (pix, keep) in enumerate(groups):
            ref = R.composite(pix, cols[keep], alpha, np.ones(3), 240 * 320).reshape(240, 320, 3)
            err = np.abs(out[v].cpu().numpy() - ref).max()
            assert err <= 4e-6, (alpha, v, err)
        if alpha == 0.5:
            again = NV.render_points(dp, dc, intr, w2c, 240, 320, alpha)
            assert torch.equal(out, again), "two runs differ"
            from curve_gaussian_amd import _lib
            ws1 = _lib.load().cgs_render_points_workspace_bytes(P, 1, 240, 320)
            for budget in (ws1, 5 * ws1 // 2):
                chunked = NV.render_points(dp, dc, intr, w2c, 240, 320, alpha, workspace_bytes=budget)
                assert torch.equal(out, chunked), f"chunked ({budget} bytes) differs"


def test_render_points_edge_sizes():
    pts, cols, cams = _rep()
    intr, w2c = NV.camera_arrays(cams[:2])
    empty = torch.zeros((0, 3), device=DEV)
    out = NV.render_points(empty, empty, intr, w2c, 48, 64, 0.5, (0.25, 0.5, 1.0))   # P = 0: the background
    assert out.shape == (2, 48, 64, 3)
    assert torch.equal(out, torch.tensor([0.25, 0.5, 1.0], device=DEV).expand(2, 48, 64, 3))
    out = NV.render_points(_dev(pts), _dev(cols), np.zeros((0, 4)), np.zeros((0, 3, 4)), 48, 64)
    assert out.shape == (0, 48, 64, 3)


def _check_pngs(out_dir, names, pts, cols, cams):
    for name, c in zip(names, cams):
        path = os.path.join(out_dir, name)
        if not name.endswith(".png"):
            continue
        got = np.asarray(Image.open(path).convert("RGB"), np.int64)
        ref, _ = R.render(pts, cols, c.R, c.T, c.fx, c.fy, c.cx, c.cy, c.width, c.height)
        exp = np.round(255 * ref)
        tie = np.abs(ref * 255 - np.floor(ref * 255) - 0.5) < 255 * 1e-5
        assert got.shape == exp.shape
        assert (got == exp)[~tie].all(), name


def test_drivers_end_to_end(tmp_path):
    # ABC --render_mv
    base = tmp_path / "abc"
    shutil.copytree(os.path.join(GOLD, "abc", "pred"), base)
    st = NV.render_abc_novel_views(str(base), ABC_DATA, seed=SEED)
    files = sorted(os.path.relpath(os.path.join(r, f), base) for r, _, fs in os.walk(base) for f in fs
                   if f.endswith(".png"))
    assert files == sorted(n + ".png" for n in G["abc_saved"])
    assert st["00000001"]["views"] == 4 and st["00000001"]["written"] == 4
    pred = pred_points_and_directions(os.path.join(base, "00000001", "parametric_edges.json"))
    cams = NV.transforms_video_cameras(os.path.join(ABC_DATA, "00000001"))
    _check_pngs(os.path.join(base, "00000001", "novel_view"), [c.name + ".png" for c in cams], pred.points,
                NV.edge_point_colors(pred, SEED), cams)
    # Replica: the view that culls every point writes nothing, as in the reference
    base = tmp_path / "replica"
    shutil.copytree(os.path.join(GOLD, "replica", "pred"), base)
    st = NV.render_replica_novel_views(str(base), REP_DATA, seed=SEED)
    files = sorted(os.path.relpath(os.path.join(r, f), base) for r, _, fs in os.walk(base) for f in fs
                   if f != "parametric_edges.json")
    assert files == sorted(G["rep_saved"])
    assert st["room0"]["written"] == 4 and st["room0"]["views"] == 5
    pts, cols, cams = _rep()
    _check_pngs(os.path.join(base, "room0", "novel_view"), [c.name for c in cams], pts, cols, cams)
    with Image.open(os.path.join(base, "room0", "novel_view", "frame_000.jpg")) as im:
        assert im.format == "JPEG" and im.size == (64, 48)
