"""Host: the depth gate on the control-point visibility check (edge_extraction.para_edge: edge_visibility_counts_depth,
compute_visibility_depth, scan_visibility_counts_depth, get_parametric_edge with occluder / depth_maps) -- the numpy back end
against the per-point loop of edge_visgate_cases.py and against counts written out by hand, the identity with an all-+inf
depth, the box with 200 segments inside it, the independence of the frame chunking, the argument checks, the writer's call
path, and the C ABI's rejections through the library."""
import json
import os

import numpy as np
import pytest
import torch

import edge_visgate_cases as C
import visibility_ref64 as R
from curve_gaussian_amd import _lib
from curve_gaussian_amd import edge_extraction as EE
from curve_gaussian_amd.edge_extraction import para_edge as PE
from curve_gaussian_amd.ops import edge_occlusion as EO
from curve_gaussian_amd.scene import dataset_io as IO
from curve_gaussian_amd.scene import solid_scan as SS

GOLD = os.path.join(os.path.dirname(__file__), "golden", "visibility")
G = np.load(os.path.join(GOLD, "visibility.npz"))


def _host(s, detector=None, depth=None, slack=None):
    return PE.edge_visibility_counts_depth(s["curves"], s["lines"], s["maps"], s["K"], s["c2w"],
                                           detector or s.get("detector", "PidiNet"), s["depth"] if depth is None else depth,
                                           s["slack"] if slack is None else slack, backend="host").numpy()


# ------------------------------------------------------------------------------------------------ the rule
def test_planted_scene_equals_the_hand_written_counts_and_the_per_point_loop():
    s = C.planted_scene()
    got = _host(s)
    assert got.dtype == np.int32 and got.shape == (9, 2)
    np.testing.assert_array_equal(got, s["want"])
    brute, _ = C.visibility_brute(s["curves"], s["lines"], s["maps"], s["K"], s["c2w"], "PidiNet", s["depth"], s["slack"])
    np.testing.assert_array_equal(got, brute)


def test_the_boundary_is_strict():
    """c2 == 2.0 exactly (identity rotation): a plane of 2.0 with slack 0 does not hide, one float32 ulp nearer does."""
    s = C.planted_scene()
    one = dict(s, curves=np.zeros((0, 4, 3)), lines=np.array([[[0.25, 0.25, 2.0], [0.25, 0.25, 2.0]]]))
    for value, want in ((np.float32(2.0), [3, 0]), (np.nextafter(np.float32(2), np.float32(0)), [1, 2])):
        depth = np.full((3, C.H, C.W), np.inf, np.float32)
        depth[:2] = value
        np.testing.assert_array_equal(_host(one, depth=depth, slack=0.0), [want])


@pytest.mark.parametrize("shape", [(7, 5, 3), (0, 6, 2), (5, 0, 1)])
@pytest.mark.parametrize("detector", ["PidiNet", "DexiNed"])
def test_random_scenes_equal_the_per_point_loop(shape, detector):
    s = C.random_scene(*shape, seed=sum(shape))
    brute, kept = C.visibility_brute(s["curves"], s["lines"], s["maps"], s["K"], s["c2w"], detector, s["depth"], s["slack"])
    np.testing.assert_array_equal(_host(s, detector), brute)
    assert kept > 0 and brute[:, 0].sum() > 0


@pytest.mark.parametrize("size", C.RANDOM_SIZES)
@pytest.mark.parametrize("shape", C.RANDOM_SHAPES)
def test_the_gpu_tests_random_scenes_have_both_verdicts(shape, size):
    """The cap of the GPU test, checked where it is chosen: the cells the gate touches are 10 % to 90 % of the cells that
    keep a point."""
    if shape[0] + shape[1] == 0:
        return
    s = C.random_scene(*shape, *size, seed=1)
    plain = _host(s, depth=np.full_like(s["depth"], np.inf))
    # a cell keeps a point iff it is visible on an all-255 map
    kept = _host(dict(s, maps=np.full_like(s["maps"], 255)), depth=np.full_like(s["depth"], np.inf))[:, 0].sum()
    touched = _host(s)[:, 1].sum()
    assert 0.1 * kept <= touched <= 0.9 * kept, (touched, kept)
    assert not plain[:, 1].any()


# ------------------------------------------------------------------------------------------------ identity
@pytest.mark.parametrize("det", ["DexiNed", "PidiNet"])
def test_an_all_inf_depth_is_the_ungated_count(det):
    maps, intr, c2w, h, w = EE.get_edge_maps(GOLD, det)
    depth = np.full(maps.shape, np.inf, np.float32)
    got = PE.edge_visibility_counts_depth(G["curves"], G["lines"], maps, intr, c2w, det, depth, backend="host").numpy()
    want = R.visibility_counts(G["curves"], G["lines"], R.map_values(maps, det), intr, c2w, h, w)
    np.testing.assert_array_equal(got[:, 0], want)
    np.testing.assert_array_equal(got[:, 0], G[f"{det}_counts"])
    assert not got[:, 1].any()
    cm, lm = PE.compute_visibility_depth(G["curves"], G["lines"], maps, intr, c2w, det, depth, backend="host")
    np.testing.assert_array_equal(torch.cat([cm, lm]).numpy(), G[f"{det}_mask"])


def test_a_nan_depth_hides_nothing_and_a_zero_depth_everything_in_front():
    s = C.random_scene(6, 6, 3, seed=3)
    plain = _host(s, depth=np.full_like(s["depth"], np.inf))
    np.testing.assert_array_equal(_host(s, depth=np.full_like(s["depth"], np.nan)), plain)
    none = _host(s, depth=np.zeros_like(s["depth"]))
    assert not none[:, 0].any() and none[:, 1].sum() > 0


# ------------------------------------------------------------------------------------------------ the box
@pytest.fixture(scope="module")
def box(tmp_path_factory):
    scan = SS.solid_scan("box", C.BOX_VIEWS, C.BOX_H, C.BOX_W, backend="host")
    path = str(tmp_path_factory.mktemp("visgate") / "box")
    SS.write_solid_scan(path, scan, depth=True)
    maps, intr, c2w, h, w = EE.get_edge_maps(path, "PidiNet")
    truth = np.asarray(scan.edges["lines_end_pts"], np.float64).reshape(-1, 2, 3)
    bogus = C.interior_segments(scan.tris)
    lines = np.concatenate([truth, bogus])
    K4, M = np.array([[c.fx, c.fy, c.cx, c.cy] for c in scan.cameras]), \
        np.array([np.concatenate([c.R, c.T[:, None]], 1) for c in scan.cameras])
    planes = EO.mesh_depth(scan.tris, K4, M, h, w, backend="host")
    gated = PE.edge_visibility_counts_depth(np.zeros((0, 4, 3)), lines, maps, intr, c2w, "PidiNet", planes,
                                            backend="host").numpy()
    ungated = R.visibility_counts(np.zeros((0, 4, 3)), lines, R.map_values(maps, "PidiNet"), intr, c2w, h, w)
    return dict(scan=scan, path=path, lines=lines, gated=gated, ungated=ungated, n_truth=len(truth), maps=maps, intr=intr,
                c2w=c2w, planes=planes)


def test_the_gate_keeps_the_box_and_nothing_inside_it(box):
    need = EE.edge_visibility_frames(C.BOX_VIEWS)
    n, gated, ungated = box["n_truth"], box["gated"], box["ungated"]
    assert n == 12
    assert (gated[:n, 0] > need).all(), gated[:n]
    assert not gated[n:, 0].any(), "a segment inside the closed convex solid was seen"
    assert (gated[:, 0] <= ungated).all()                   # 0 / 255 maps: dropping points cannot create a visible cell
    kept_ungated = int((ungated[n:] > need).sum())
    print(f"ungated check keeps {kept_ungated} of {len(ungated) - n} interior segments; gated keeps "
          f"{int((gated[n:, 0] > need).sum())}; truth counts {gated[:n, 0].tolist()} gated, {ungated[:n].tolist()} ungated")
    assert kept_ungated >= 40                               # the defect exists; not a measurement of the new code
    assert (ungated[:n] > need).all()


def test_get_parametric_edge_returns_exactly_the_box(box, capsys):
    d = {"curves_ctl_pts": [], "lines_end_pts": box["lines"].reshape(-1, 6).tolist()}
    pts, ret = EE.get_parametric_edge(True, d, box["path"], "PidiNet", occluder=os.path.join(box["path"], "mesh.ply"),
                                      backend="host")
    assert ret == {"curves_ctl_pts": [], "lines_end_pts": box["lines"][:12].reshape(-1, 6).tolist()}
    np.testing.assert_array_equal(pts, IO.sample_edge_points(np.zeros((0, 4, 3)), box["lines"][:12].reshape(-1, 6)))
    out = capsys.readouterr().out
    assert "before visible checking:  212 after visible checking:  12" in out
    assert f"depth gate: dropped a point in {int(box['gated'][:, 1].sum())} of {212 * C.BOX_VIEWS} (edge, frame) cells" in out
    # the scan's own depth maps (the plain z-buffer) through depth_maps: K is not restricted, the window is applied
    depth_maps = [np.load(os.path.join(box["path"], "depth", f"{i}_colors.npy")) for i in range(C.BOX_VIEWS)]
    _, ret2 = EE.get_parametric_edge(True, d, box["path"], "PidiNet", depth_maps=depth_maps, backend="host")
    assert ret2 == ret


@pytest.mark.parametrize("budget", [1, None])
def test_frame_chunking_does_not_change_the_counts(box, budget):
    got, n_frames = PE.scan_visibility_counts_depth(np.zeros((0, 4, 3)), box["lines"], box["path"], "PidiNet",
                                                    occluder=box["scan"].tris, backend="host", budget_bytes=budget)
    assert n_frames == C.BOX_VIEWS
    np.testing.assert_array_equal(got, box["gated"])


# ------------------------------------------------------------------------------------------------ argument checks
def test_argument_checks(box, tmp_path):
    d = {"curves_ctl_pts": [], "lines_end_pts": box["lines"][:3].reshape(-1, 6).tolist()}
    tris, path = box["scan"].tris, box["path"]
    maps = [np.full((C.BOX_H, C.BOX_W), 1.0, np.float32)] * C.BOX_VIEWS
    with pytest.raises(ValueError, match="not both"):
        EE.get_parametric_edge(True, d, path, "PidiNet", occluder=tris, depth_maps=maps, backend="host")
    with pytest.raises(ValueError, match="near_clip needs an occluder"):
        EE.get_parametric_edge(True, d, path, "PidiNet", depth_maps=maps, near_clip=0.01, backend="host")
    with pytest.raises(ValueError, match="near_clip needs an occluder"):
        EE.get_parametric_edge(True, d, path, "PidiNet", near_clip=0.01)
    with pytest.raises(ValueError, match="visible_checking=True"):
        EE.get_parametric_edge(False, d, path, "PidiNet", occluder=tris, backend="host")
    with pytest.raises(ValueError, match="slack"):
        EE.get_parametric_edge(True, d, path, "PidiNet", occluder=tris, depth_slack=-1.0, backend="host")
    # a K with skew: an occluder's planes are not in its image; the caller's depth maps may be
    import shutil
    skew = str(tmp_path / "skew")
    shutil.copytree(path, skew)
    meta = json.load(open(os.path.join(skew, "meta_data.json")))
    meta["frames"][5]["intrinsics"][0][1] = 0.5
    json.dump(meta, open(os.path.join(skew, "meta_data.json"), "w"))
    with pytest.raises(ValueError, match="frame 5 are not a pinhole"):
        EE.get_parametric_edge(True, d, skew, "PidiNet", occluder=tris, backend="host")
    EE.get_parametric_edge(True, d, skew, "PidiNet", depth_maps=maps, backend="host")
    for bad in ([[1.0, 0, 0], [0.1, 1, 0], [0, 0, 1]], [[1.0, 0, 0], [0, 1, 0], [0.1, 0, 1]], [[1.0, 0, 0], [0, 1, 0], [0, 0.1, 1]],
                [[1.0, 0, 0], [0, 1, 0], [0, 0, 2]]):
        with pytest.raises(ValueError, match="pinhole"):
            PE.check_pinhole_intrinsics("t", np.array([bad]))


def test_existing_functions_still_reject_cpu_tensors():
    c, ln = torch.zeros((1, 4, 3), dtype=torch.float64), torch.zeros((1, 2, 3), dtype=torch.float64)
    with pytest.raises(_lib.CurveGSError, match="GPU tensor"):
        EE.edge_visibility_counts(c, ln, torch.zeros((1, 4, 4), dtype=torch.uint8), np.eye(3)[None], np.eye(4)[None], "DexiNed")


# ------------------------------------------------------------------------------------------------ call path
def test_depth_options_alone_leave_the_visibility_check_ungated(monkeypatch, tmp_path):
    calls = []

    def fake(visible_checking, merged, scan_dir=None, detector=None, **kw):
        calls.append((visible_checking, scan_dir, detector, kw))
        return np.zeros((0, 3), np.float32), {"curves_ctl_pts": [], "lines_end_pts": []}
    monkeypatch.setattr(PE, "get_parametric_edge", fake)
    monkeypatch.setattr(IO, "extract_curves", lambda *a, **k: {"curves_ctl_pts": [], "lines_end_pts": []})
    depth = {"occluder": "mesh.ply", "depth_slack": 0.002, "depth_window": 1}
    IO.write_parametric_edges(None, str(tmp_path / "a"), visible_checking=True, scan_dir="scan", detector="PidiNet",
                              depth_options=depth)
    assert calls == [(True, "scan", "PidiNet", {})]
    IO.write_parametric_edges(None, str(tmp_path / "b"), visible_checking=True, scan_dir="scan", detector="PidiNet",
                              depth_options=depth, visibility_options={"occluder": "m.ply", "near_clip": 0.01})
    assert calls[1] == (True, "scan", "PidiNet", {"occluder": "m.ply", "near_clip": 0.01})


def test_command_lines_reject_bad_depth_sources(capsys):
    from curve_gaussian_amd.edge_extraction import __main__ as ABC
    from curve_gaussian_amd.edge_extraction import replica, visibility
    base = ["--edges", "e.json", "--scan_dir", "s", "--detector", "PidiNet", "--out", "o"]
    for main, argv in ((visibility.main, base), (ABC.main, ["--dataset_dir", "d", "--render_mv"]),
                       (replica.main, ["--dataset_dir", "d"])):
        for extra, text in ((["--occluder", "mesh.ply", "--depth_dir", "depth"], "not both"),
                            (["--near_clip"], "--near_clip needs --occluder"),
                            (["--depth_dir", "depth", "--near_clip", "0.02"], "--near_clip needs --occluder")):
            with pytest.raises(SystemExit) as e:
                main(argv + extra)
            assert e.value.code == 2 and text in capsys.readouterr().err


def test_train_gate_visibility_needs_a_depth_source_and_the_check(tmp_path):
    from curve_gaussian_amd import train as T
    base = ["-s", str(tmp_path), "-m", str(tmp_path / "out")]
    with pytest.raises(SystemExit):
        T.parse_args(base + ["--gate_visibility"])
    with pytest.raises(SystemExit):
        T.parse_args(base + ["--gate_visibility", "--occluder", "mesh.ply", "--depth_dir", "depth"])
    with pytest.raises(SystemExit):   # the run's visible_checking is off
        T.parse_args(base + ["--gate_visibility", "--occluder", "mesh.ply"])
    assert not T.parse_args(base)[1].visible_checking
    _, opt, args = T.parse_args(base + ["--visible_checking", "--gate_visibility", "--occluder", "mesh.ply", "--near_clip"])
    assert opt.visible_checking and args.gate_visibility and args.near_clip == EO.NEAR_CLIP

    class Args:
        gate_visibility, gate_edge_checks, occluder, depth_dir, depth_slack, depth_window, near_clip = True, False, "mesh.ply", \
            None, 0.002, 2, 0.01
    assert T.gate_options(Args, "/scan", None) == {}
    assert T.gate_options(Args, "/scan", None, flag="gate_visibility") == {
        "occluder": "/scan/mesh.ply", "depth_slack": 0.002, "depth_window": 2, "near_clip": 0.01}


# ------------------------------------------------------------------------------------------------ ABI
def test_abi_rejects_invalid_arguments_before_launch():
    lib = _lib.load()
    p = _lib.ptr(torch.zeros(64, dtype=torch.float64))
    INVALID = -1   # CGS_ERR_INVALID_ARGUMENT
    nan, inf = float("nan"), float("inf")
    vis = lambda **k: [k.get(a, d) for a, d in (("nc", 1), ("c", p), ("nl", 0), ("l", None), ("F", 1), ("K", p), ("M", p),
                                                ("H", 4), ("W", 4), ("maps", p), ("inv", 1), ("depth", p), ("slack", 0.0),
                                                ("out", p), ("stream", None))]
    proj = lambda **k: [k.get(a, d) for a, d in (("P", 1), ("pts", p), ("V", 1), ("K", p), ("M", p), ("H", 4), ("W", 4),
                                                 ("depth", p), ("slack", 0.0), ("uv", p), ("hid", None), ("stream", None))]
    rend = lambda **k: [k.get(a, d) for a, d in (("P", 1), ("pts", p), ("col", p), ("V", 1), ("K", p), ("M", p), ("H", 4),
                                                 ("W", 4), ("depth", p), ("slack", 0.0), ("alpha", 0.5), ("bg", p), ("out", p),
                                                 ("kept", None), ("hid", None), ("ws", p), ("wsb", 1 << 20), ("stream", None))]
    cases = [("cgs_edge_visibility_depth", vis, [dict(depth=None), dict(slack=-1.0), dict(slack=nan), dict(slack=inf),
                                                 dict(nc=-1), dict(nl=-1), dict(F=-1), dict(H=0), dict(W=-3), dict(c=None),
                                                 dict(K=None), dict(M=None), dict(maps=None), dict(out=None)]),
             ("cgs_project_points_depth", proj, [dict(depth=None), dict(slack=-1.0), dict(slack=nan), dict(slack=inf),
                                                 dict(P=-1), dict(V=-1), dict(H=0), dict(W=-1), dict(pts=None), dict(uv=None)]),
             ("cgs_render_points_depth", rend, [dict(depth=None), dict(slack=-1.0), dict(slack=nan), dict(slack=inf),
                                                dict(P=-1), dict(V=-1), dict(H=0), dict(W=-1), dict(alpha=1.5), dict(out=None),
                                                dict(ws=None), dict(wsb=0)])]
    for name, make, bads in cases:
        for bad in bads:
            assert getattr(lib, name)(*make(**bad)) == INVALID, (name, bad)
            assert f"{name}: invalid argument" in _lib.last_error(), (name, bad)
    # the empty calls are no-ops that touch nothing
    assert lib.cgs_edge_visibility_depth(*vis(nc=0, c=None, K=None, M=None, maps=None, depth=None, out=None)) == 0
    assert lib.cgs_project_points_depth(*proj(P=0, pts=None, depth=None, uv=None)) == 0
    assert lib.cgs_render_points_depth(*rend(V=0, depth=None, out=None, ws=None)) == 0
