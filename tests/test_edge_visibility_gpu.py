"""GPU: the edge-map visibility kernel (cgs_edge_visibility) against the reference-generated fixture
(tests/golden/make_visibility_golden.py) and against the float64 restatement (tests/visibility_ref64.py, itself pinned
to the fixture by tests/test_edge_visibility_cpu.py), exact counts everywhere."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from curve_gaussian_amd import _lib
from curve_gaussian_amd import edge_extraction as EE
from curve_gaussian_amd import synthetic as S
from curve_gaussian_amd.scene import dataset_io as IO

import visibility_ref64 as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(os.path.dirname(__file__), "golden", "visibility")
G = np.load(os.path.join(GOLD, "visibility.npz"))
DETECTORS = ("DexiNed", "PidiNet")
DEV = torch.device("cuda:0")


def _kernel_counts(curves, lines, maps_u8, K, c2w, det):
    c = torch.from_numpy(np.asarray(curves, np.float64).reshape(-1, 4, 3)).to(DEV)
    ln = torch.from_numpy(np.asarray(lines, np.float64).reshape(-1, 2, 3)).to(DEV)
    m = maps_u8 if isinstance(maps_u8, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(maps_u8)).to(DEV)
    a = EE.edge_visibility_counts(c, ln, m, K, c2w, det)
    b = EE.edge_visibility_counts(c, ln, m, K, c2w, det)
    torch.cuda.synchronize()
    assert torch.equal(a, b), "two runs differ"
    assert a.dtype == torch.int32 and a.device == m.device
    return a.cpu().numpy().astype(np.int64)


# ------------------------------------------------------------------------------------------ the reference's fixture
@pytest.mark.parametrize("det", DETECTORS)
def test_fixture_counts_masks_and_output(det, capsys):
    maps, K, c2w, h, w = EE.get_edge_maps(GOLD, det)
    np.testing.assert_array_equal(_kernel_counts(G["curves"], G["lines"], maps, K, c2w, det), G[f"{det}_counts"])
    cm, lm = EE.compute_visibility(torch.from_numpy(G["curves"]).to(DEV), torch.from_numpy(G["lines"]).to(DEV),
                                   torch.from_numpy(maps).to(DEV), K, c2w, det)
    assert cm.dtype == torch.bool and cm.device.type == "cuda"
    np.testing.assert_array_equal(torch.cat([cm, lm]).cpu().numpy(), G[f"{det}_mask"])
    d = {"lines_end_pts": G["lines"].reshape(-1, 6).tolist(), "curves_ctl_pts": G["curves"].tolist()}
    pts, ret = EE.get_parametric_edge(True, d, GOLD, det)
    np.testing.assert_array_equal(np.asarray(ret["curves_ctl_pts"]).reshape(-1, 4, 3), G[f"{det}_curves"])
    np.testing.assert_array_equal(np.asarray(ret["lines_end_pts"]).reshape(-1, 6), G[f"{det}_lines"])
    np.testing.assert_array_equal(pts, G[f"{det}_points"])
    assert pts.dtype == np.float32
    n_all, n_kept = len(G[f"{det}_counts"]), int(G[f"{det}_mask"].sum())
    assert f"before visible checking:  {n_all} after visible checking:  {n_kept}" in capsys.readouterr().out


@pytest.mark.parametrize("det", DETECTORS)
def test_planted_cases_alone_equal_the_restatement(det):
    """Each planted edge of the fixture on its own (one-edge launches) and all of them together."""
    maps, K, c2w, h, w = EE.get_edge_maps(GOLD, det)
    vals = R.map_values(maps, det)
    nc, nl = len(G["planted_curve_names"]), len(G["planted_line_names"])
    curves, lines = G["curves"][:nc], G["lines"][:nl]
    want = R.visibility_counts(curves, lines, vals, K, c2w, h, w)
    np.testing.assert_array_equal(_kernel_counts(curves, lines, maps, K, c2w, det), want)
    np.testing.assert_array_equal(want, np.concatenate([G[f"{det}_counts"][:nc],
                                                        G[f"{det}_counts"][len(G["curves"]):][:nl]]))
    for i in range(nc):
        got = _kernel_counts(curves[i:i + 1], np.zeros((0, 2, 3)), maps, K, c2w, det)
        assert got[0] == want[i], G["planted_curve_names"][i]
    for i in range(nl):
        got = _kernel_counts(np.zeros((0, 4, 3)), lines[i:i + 1], maps, K, c2w, det)
        assert got[0] == want[nc + i], G["planted_line_names"][i]


# ------------------------------------------------------------------------------------------ random scenes at scale
def _rot(axis_angle):
    a = np.asarray(axis_angle, np.float64)
    t = np.linalg.norm(a)
    k = a / t
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(t) * Kx + (1 - np.cos(t)) * Kx @ Kx


def _scene(n_curves, n_lines, F, H, W, seed):
    """Random cameras round a box of edges (3 % of the points behind the cameras), u8 maps with 4 % of the pixels lit
    (PidiNet; DexiNed gets 255 - u8).
    Points whose projection in some frame lies within 1e-6 px of a rounding boundary are redrawn, so that BLAS and the
    kernel cannot round a coordinate differently; the caller asserts the margin."""
    g = np.random.default_rng(seed)
    K = np.zeros((F, 4, 4))
    c2w = np.zeros((F, 4, 4))
    for f in range(F):
        fx, fy = g.uniform(0.8, 1.1, 2) * W
        K[f] = [[fx, 0, W / 2 + g.uniform(-3, 3), 0], [0, fy, H / 2 + g.uniform(-3, 3), 0], [0, 0, 1, 0], [0, 0, 0, 1]]
        c2w[f, :3, :3] = _rot(g.normal(0, 0.15, 3))
        c2w[f, :3, 3] = g.uniform(-0.3, 0.3, 3)
        c2w[f, 3, 3] = 1
    n = 4 * n_curves + 2 * n_lines

    def draw(k):
        p = g.uniform([-1.2, -0.9, 1.5], [1.2, 0.9, 4.0], (k, 3))
        behind = g.random(k) < 0.03
        p[behind, 2] = -p[behind, 2]
        return p

    pts = draw(n)
    for _ in range(20):
        bad = np.zeros(n, bool)
        for f in range(F):
            uv = R.project(K[f], c2w[f], pts)
            with np.errstate(invalid="ignore"):
                bad |= (np.abs(uv - np.floor(uv) - 0.5) <= 2e-6).any(1)
        if not bad.any():
            break
        pts[bad] = draw(int(bad.sum()))
    maps = np.where(g.random((F, H, W)) < 0.04, g.integers(0, 256, (F, H, W)), 0).astype(np.uint8)
    return pts[:4 * n_curves].reshape(-1, 4, 3), pts[4 * n_curves:].reshape(-1, 2, 3), maps, K, c2w


def _check_scene(n_curves, n_lines, F, H=480, W=640, seed=0):
    curves, lines, pid, K, c2w = _scene(n_curves, n_lines, F, H, W, seed)
    for det in DETECTORS:
        maps = pid if det == "PidiNet" else 255 - pid
        dmaps = torch.from_numpy(maps).to(DEV)
        want, uv = R.visibility_counts(curves, lines, R.map_values(maps, det), K, c2w, H, W, return_uv=True)
        fin = np.isfinite(uv)
        margin = np.abs(uv[fin] - np.floor(uv[fin]) - 0.5)
        assert margin.size == 0 or margin.min() > 1e-6, f"a coordinate within {margin.min():.3g} px of a rounding edge"
        got = _kernel_counts(curves, lines, dmaps, K, c2w, det)
        np.testing.assert_array_equal(got, want)
        if n_curves + n_lines and F > 1:
            assert 0 < (want > EE.edge_visibility_frames(F)).sum() < n_curves + n_lines
    return want


def test_scale_20000_edges_70_frames():
    want = _check_scene(12000, 8000, 70)
    assert len(np.unique(want)) > 10


@pytest.mark.parametrize("F", [1, 64, 65])
def test_frame_counts(F):
    _check_scene(700, 500, F, H=120, W=160, seed=F)


@pytest.mark.parametrize("nc,nl", [(0, 0), (900, 0), (0, 900)])
def test_empty_curves_only_lines_only(nc, nl):
    _check_scene(nc, nl, 9, H=120, W=160, seed=nc + 2 * nl)
    if nc + nl == 0:
        cm, lm = EE.compute_visibility(torch.zeros((0, 4, 3), dtype=torch.float64, device=DEV),
                                       torch.zeros((0, 2, 3), dtype=torch.float64, device=DEV),
                                       torch.zeros((3, 8, 8), dtype=torch.uint8, device=DEV),
                                       np.tile(np.eye(3), (3, 1, 1)), np.tile(np.eye(4), (3, 1, 1)), "DexiNed")
        assert cm.shape == (0,) and lm.shape == (0,)


def test_maps_over_2_gib_use_64_bit_offsets():
    """3 frames of 30000^2 bytes (2.7e9 B): the only bright pixels sit past byte 2^31, in the last frame, so every
    edge pointing at one is seen in exactly one frame; an edge pointing at the same pixel of a dark frame is not."""
    S_ = 30000
    maps = torch.zeros((3, S_, S_), dtype=torch.uint8, device=DEV)
    targets = [(15001, 20000), (S_ - 1, S_ - 1), (0, 11583), (7, S_ - 1)]       # (u, v) in frame 2, offset > 2^31
    for u, v in targets:
        assert 2 * S_ * S_ + v * S_ + u > 2 ** 31
        maps[2, v, u] = 255
    K = np.tile(np.array([[1000.0, 0, 0], [0, 1000.0, 0], [0, 0, 1]]), (3, 1, 1))
    c2w = np.tile(np.eye(4), (3, 1, 1))
    pt = lambda u, v: [u / 1000.0, v / 1000.0, 1.0]                           # u, v integers: far from x.5
    lines = np.array([[pt(u, v), pt(u, v)] for u, v in targets] + [[pt(100, 100), pt(200, 11583)]])
    curves = np.array([[pt(*targets[0]), pt(*targets[1]), pt(5, 5), pt(S_ + 10, 3)]])
    for det, want in (("PidiNet", [1, 1, 1, 1, 1, 0]), ("DexiNed", [3, 2, 2, 2, 2, 3])):
        got = _kernel_counts(curves, lines, maps, K, c2w, det)
        np.testing.assert_array_equal(got, want)
    del maps
    torch.cuda.empty_cache()


def test_cpu_tensors_and_mixed_devices_raise():
    c = torch.zeros((1, 4, 3), dtype=torch.float64, device=DEV)
    ln = torch.zeros((1, 2, 3), dtype=torch.float64, device=DEV)
    maps = torch.zeros((1, 8, 8), dtype=torch.uint8, device=DEV)
    K, c2w = np.eye(3)[None], np.eye(4)[None]
    with pytest.raises(_lib.CurveGSError, match="GPU tensor"):
        EE.compute_visibility(c.cpu(), ln, maps, K, c2w, "DexiNed")
    with pytest.raises(_lib.CurveGSError, match="GPU tensor"):
        EE.compute_visibility(c, ln, maps.cpu(), K, c2w, "PidiNet")
    with pytest.raises(_lib.CurveGSError, match="one device"):
        EE.compute_visibility(c, ln, maps, torch.eye(3)[None], c2w, "DexiNed")
    if torch.cuda.device_count() > 1:
        with pytest.raises(_lib.CurveGSError, match="one device"):
            EE.compute_visibility(c, ln.to("cuda:1"), maps, K, c2w, "DexiNed")
    with pytest.raises(ValueError, match="Unknown detector"):
        EE.compute_visibility(c, ln, maps, K, c2w, "HED")


# ------------------------------------------------------------------------------------------ end to end
def test_end_to_end_writer_and_cli(tmp_path):
    """A synthetic model's edges, a scan written by write_emap whose DexiNed maps draw some of them (dark pixels) and
    not others, then write_parametric_edges(visible_checking=True) and the CLI against the restatement."""
    g = np.random.default_rng(5)
    B = 40
    cp = g.uniform(0.3, 0.7, (B, 4, 3))
    cp[B - 6:] += np.array([0.0, 0.0, 9.0])                                    # off-screen edges: far above the box
    is_bez = g.random(B) < 0.6

    class Model:
        pass
    model = Model()
    model.get_curve_points = torch.from_numpy(cp.astype(np.float32))
    model.is_bezier = torch.from_numpy(is_bez)
    cams = S.fibonacci_cameras(20, 96, 128)
    scan = str(tmp_path / "scan")
    IO.write_emap(scan, cams, [torch.ones(96, 128) for _ in cams])
    meta = json.load(open(os.path.join(scan, "meta_data.json")))
    K = np.array([f["intrinsics"] for f in meta["frames"]])
    c2w = np.array([f["camtoworld"] for f in meta["frames"]])
    merged = IO.extract_curves(model)
    curves = np.array(merged["curves_ctl_pts"]).reshape(-1, 4, 3)
    lines = np.array(merged["lines_end_pts"]).reshape(-1, 2, 3)
    shown_c, shown_l = np.arange(len(curves)) % 3 != 0, np.arange(len(lines)) % 3 != 0
    pts = np.concatenate([curves[shown_c].reshape(-1, 3), lines[shown_l].reshape(-1, 3)])
    maps = []
    for f in range(len(cams)):
        m = torch.ones(96, 128)
        uv = np.round(R.project(K[f], c2w[f], pts)).astype(np.int64)
        ok = (uv[:, 0] >= 0) & (uv[:, 0] < 128) & (uv[:, 1] >= 0) & (uv[:, 1] < 96)
        m[uv[ok, 1], uv[ok, 0]] = 0.0                                          # DexiNed: dark = edge
        maps.append(m)
    IO.write_emap(scan, cams, maps)
    u8, K2, c2w2, h, w = EE.get_edge_maps(scan, "DexiNed")
    counts = R.visibility_counts(curves, lines, R.map_values(u8, "DexiNed"), K2, c2w2, h, w)
    want_pts, want_dict, cm, lm = R.parametric_edges(curves, lines, counts, len(cams))
    assert 0 < cm.sum() + lm.sum() < len(counts)

    out = str(tmp_path / "out")
    d, p = IO.write_parametric_edges(model, out, visible_checking=True, scan_dir=scan)
    assert d == want_dict and json.load(open(os.path.join(out, "parametric_edges.json"))) == want_dict
    np.testing.assert_array_equal(p, want_pts)

    full = str(tmp_path / "full")
    IO.write_parametric_edges(model, full)
    cli_out = str(tmp_path / "cli")
    r = subprocess.run([sys.executable, "-m", "curve_gaussian_amd.edge_extraction.visibility", "--edges",
                        os.path.join(full, "parametric_edges.json"), "--scan_dir", scan, "--detector", "DexiNed",
                        "--out", cli_out], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert f"before visible checking:  {len(counts)} after visible checking:  {int(cm.sum() + lm.sum())}" in r.stdout
    for name in ("parametric_edges.json", "edge_points.ply"):
        assert open(os.path.join(cli_out, name), "rb").read() == open(os.path.join(out, name), "rb").read(), name
