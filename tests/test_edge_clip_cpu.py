"""CPU: near-plane clipping (cgs_mesh_depth_clipped / cgs_mesh_contours_clipped, include/curvegs.h) on the host back end of
ops.edge_occlusion / ops.mesh_contours -- in images of 1 x 1, 5 x 33 and 5 x 67, bit for bit against the brute-force restatements of edge_clip_cases.py, against an
independent float64 ray cast, on the shared-edge pair (no crack), on the indoor fixture ``solid_scan("room")``, through the
operators and command lines, and the C ABI's argument checks.  Without the option nothing changes: held to what
the commit before the option wrote (tests/golden/edge_clip_parent.json)."""
import ctypes
import itertools
import json
import os
import sys

import numpy as np
import pytest

import edge_clip_cases as C
import mesh_contours_cases as MCC
from curve_gaussian_amd.edge_extraction import reprojection as R
from curve_gaussian_amd.edge_extraction import support as SUP
from curve_gaussian_amd.ops import edge_occlusion as EO
from curve_gaussian_amd.ops import edge_seed as SD
from curve_gaussian_amd.ops import edge_snap as SN
from curve_gaussian_amd.ops import edge_support as SP
from curve_gaussian_amd.ops import edge_trim as TR
from curve_gaussian_amd.ops import mesh_contours as MC
from curve_gaussian_amd.ops.view_chunks import camera_arrays
from curve_gaussian_amd.scene import solid_scan as SS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOM = (12, 60, 80)   # views, height, width of the indoor fixture


def _host(tris, K, M, W, near=C.NEAR):
    return EO.mesh_depth(tris, K, M, C.height(W), W, window=0, backend="host", near_clip=near).numpy()


# ------------------------------------------------------------------------------------------------ the z-buffer
def test_host_planes_equal_the_brute_force_bit_for_bit():
    for W, V in itertools.product(C.WIDTHS, C.VIEWS):
        K, M = C.cameras(V, C.height(W), W)
        for name in list(C.SINGLES) + list(C.PAIRS):
            tris = C.single(name) if name in C.SINGLES else C.pair(name)
            assert C.same_bits(_host(tris, K, M, W), C.zbuffer_clipped_brute(tris, K, M, C.height(W), W)), (name, W, V)
    for F, W, V in [(F, 33, 2) for F in C.FACES] + [(65, 1, 1), (65, 67, 5), (257, 67, 1)]:
        K, M = C.cameras(V, C.height(W), W)
        assert C.same_bits(_host(C.cloud(F), K, M, W), C.reference_cloud(F, W, V)), (F, W, V)


def test_the_special_triangles_do_what_the_rule_says():
    K, M = C.cameras(1, C.height(33), 33)
    plane = lambda name, near=C.NEAR: _host(C.single(name), K, M, 33, near)[0]
    unclipped = lambda name: EO.mesh_depth(C.single(name), K, M, C.height(33), 33, window=0, backend="host").numpy()[0]
    for name in C.EXPECT_EMPTY:
        assert np.isinf(plane(name)).all(), name
    # three IN, a vertex exactly at near, a triangle lying in the plane: the bits of the unclipped entry
    for name in ("three_in", "vertex_at_near", "in_the_plane"):
        assert C.same_bits(plane(name), unclipped(name)) and np.isfinite(plane(name)).any(), name
    assert set(np.unique(plane("in_the_plane"))) == {np.float32(C.NEAR), np.float32(np.inf)}
    # one ulp below the plane the vertex is OUT: the unclipped entry still draws the triangle (c2 > 0), the clipped one
    # draws the two pieces, which cover less and nothing nearer than near
    below, at = plane("vertex_ulp_below"), plane("vertex_at_near")
    assert np.isfinite(below).any() and below.min() >= np.float32(C.NEAR)
    assert (np.isfinite(below) <= np.isfinite(at)).all()
    # one and two IN, each rotation of the vertices: the same plane, and the unclipped entry drops them whole
    for group in (("one_in_0", "one_in_1", "one_in_2"), ("two_in_0", "two_in_1", "two_in_2", "far_behind")):
        planes = [plane(n) for n in group]
        assert np.isfinite(planes[0]).any(), group
        assert all(np.isinf(unclipped(n)).all() for n in group), group
    for a, b in (("one_in_0", "one_in_1"), ("one_in_0", "one_in_2"), ("two_in_0", "two_in_1"), ("two_in_0", "two_in_2")):
        close = np.isclose(plane(a), plane(b), rtol=1e-6, atol=0.0) | (np.isinf(plane(a)) & np.isinf(plane(b)))
        assert close.all(), (a, b)   # (another rotation is another operation order: close, not equal)
    # the floor under the hovering camera: every pixel, in every test image
    for W in C.WIDTHS:
        Kw, Mw = C.cameras(1, C.height(W), W)
        assert np.isfinite(_host(C.single("floor"), Kw, Mw, W)).all(), W
    assert np.isinf(unclipped("floor")).all()
    # a larger near cuts more away
    assert np.isfinite(plane("one_in_0", 1.0)).sum() < np.isfinite(plane("one_in_0", C.NEAR)).sum()


def test_a_shared_straddling_edge_leaves_no_crack():
    """The union of both pieces' coverage contains every pixel centre inside the clipped quadrilateral's projection."""
    quad = np.array(C._on_plane(C.QUAD_XY), np.float32).astype(np.float64)   # the float32 vertices the entry sees
    for W in C.WIDTHS:
        K, M = C.cameras(1, C.height(W), W)
        poly = C.clipped_polygon(quad, C.NEAR)
        assert len(poly) == 4
        inside = C.centres_inside([(p[0] / p[2], p[1] / p[2]) for p in poly], C.height(W), W, margin=1e-6)
        assert inside.all(), "the clipped quadrilateral covers the whole image of camera 0"
        want = None
        for name in C.PAIRS:
            got = _host(C.pair(name), K, M, W)[0]
            brute = C.zbuffer_clipped_brute(C.pair(name), K, M, C.height(W), W)[0]
            assert C.same_bits(got, brute), (name, W)
            assert np.isfinite(brute[inside]).all(), (name, W, "a pixel between the two pieces is +inf")
            # each triangle alone leaves pixels open: it is the union that closes
            alone = [_host(C.pair(name)[k:k + 1], K, M, W)[0] for k in range(2)]
            if W > 1:
                assert all(np.isinf(a).any() for a in alone), (name, W)
            assert C.same_bits(np.minimum(alone[0], alone[1]), got)
            # the cut of the shared edge is taken from its IN end whichever way the edge is listed: the same cut to the bit
            cuts = []
            for t in C.pair(name).astype(np.float64):
                for piece in C.pieces_of([tuple(v) for v in t], C.NEAR):
                    cuts += [v for v in piece if v[2] == C.NEAR]
            assert len(set(cuts)) == 3, (name, "A-C's cut is shared; B-C and A-D have their own")
            want = got if want is None else want
            close = np.isclose(got, want, rtol=1e-6, atol=0.0)
            assert close.all(), name


RAY_CAST_CASES = [("floor", 33, 1), ("floor", 67, 1), ("floor", 1, 1), ("abc_acd", 33, 1), ("abc_acd", 67, 1), ("abc_acd", 1, 1),
                  ("two_in_0", 33, 1), ("one_in_0", 67, 1)] + [(F, W, V) for F in (63, 65, 257) for W, V in ((1, 1), (33, 2), (67, 5))]


def check_ray_cast(planes_of):
    """Assertion 4 on the small cases, shared with the GPU tests: ``planes_of(tris, K, M, W)`` -> float32 [V,H,W].  The
    independent truth is a float64 ray cast of the UNCLIPPED triangles; the clipped planes agree within 2 float32 ulps where
    both are finite, and at most 0.1 % of a case's pixels may differ in coverage (a cap; at these sizes that is one pixel of
    the 5 x 67 x 5 cases and none elsewhere).  Returns the largest relative error."""
    worst = 0.0
    for what, W, V in RAY_CAST_CASES:
        tris = C.cloud(what) if isinstance(what, int) else C.single(what) if what in C.SINGLES else C.pair(what)
        H = C.height(W)
        K, M = C.cameras(V, H, W)
        border, rel = C.against_ray_cast(planes_of(tris, K, M, W), C.ray_cast(tris, K, M, H, W, C.NEAR))
        assert border <= C.BORDER_CAP * V * H * W and rel <= C.ULP2, (what, W, V, border, rel)
        worst = max(worst, rel)
    return worst


def test_planes_agree_with_a_ray_cast_of_the_unclipped_triangles():
    """The independent truth: the floor, the pair, single triangles, the clouds around the camera, and the room.  Measured
    on the host: 5.95e-8 at most, no pixel left out anywhere."""
    worst = check_ray_cast(_host)
    V, H, W = ROOM
    scan = SS.solid_scan("room", V, H, W, backend="host")
    K, M = camera_arrays(scan.cameras)
    border, rel = C.against_ray_cast(scan.depth, C.ray_cast(scan.tris, K, M.reshape(V, 3, 4), H, W, EO.NEAR_CLIP))
    print(f"ray cast: room border pixels {border}, largest relative error {max(worst, rel):.3g}")
    assert border == 0, "on the room fixture the host back end leaves out none"
    assert rel <= C.ULP2, rel


def test_with_every_vertex_in_front_the_planes_and_masks_are_the_unclipped_ones():
    for shape in SS.SHAPES:
        tris, _ = SS.solid_geometry(shape)
        K, M = MCC.cube_cameras(3, 24, 32)
        a = EO.mesh_depth(tris, K, M, 24, 32, backend="host")
        b = EO.mesh_depth(tris, K, M, 24, 32, backend="host", near_clip=EO.NEAR_CLIP)
        assert C.same_bits(a.numpy(), b.numpy()) and np.isfinite(a.numpy()).any(), shape
        for kind in MC.KINDS:
            rows = MC.edge_rows(tris, kind)
            m0 = MC.row_masks(rows, K, M, 24, 32, a, backend="host")
            m1 = MC.row_masks(rows, K, M, 24, 32, a, backend="host", near_clip=EO.NEAR_CLIP)
            assert C.same_bits(m0.numpy(), m1.numpy()), (shape, kind)
            assert C.same_bits(MC.row_masks(rows, K, M, 24, 32, backend="host").numpy(),
                               MC.row_masks(rows, K, M, 24, 32, backend="host", near_clip=EO.NEAR_CLIP).numpy())


# ------------------------------------------------------------------------------------------------ the contours
def test_host_contours_equal_the_brute_force_bit_for_bit():
    K, M = MCC.camera(MCC.EYE_SIDE)
    drawn = {}
    for name, (row, _) in C.TENT_ROWS.items():
        got = MC.row_masks(row, K, M, MCC.H, MCC.W, backend="host", near_clip=C.NEAR).numpy()
        assert C.same_bits(got, C.contours_clipped_brute(row, K, M, MCC.H, MCC.W)), name
        drawn[name] = got[0]
        plain = MC.row_masks(row, K, M, MCC.H, MCC.W, backend="host").numpy()
        assert C.same_bits(plain, MCC.contours_brute(row, K, M, MCC.H, MCC.W)), name
    # both ends IN (one exactly at near): the bytes of the unclipped entry
    for name in ("both_in", "b_at_near"):
        assert C.same_bits(drawn[name][None], MC.row_masks(C.TENT_ROWS[name][0], K, M, MCC.H, MCC.W, backend="host").numpy())
    assert C.same_bits(drawn["both_in"], MCC.HAND_CASES["side"][2])
    # one end OUT: skipped whole without clipping, drawn from the IN end with it; both OUT and a NaN end draw nothing
    for name in ("b_behind", "a_behind", "b_in_front_of_near"):
        assert drawn[name].any(), name
        if name != "b_in_front_of_near":   # (0 < B2 < near: the unclipped entry still draws it)
            assert not MC.row_masks(C.TENT_ROWS[name][0], K, M, MCC.H, MCC.W, backend="host").numpy().any(), name
    assert drawn["b_behind"][5, 18] == 1 and drawn["a_behind"][10, 18] == 1, "the IN end's pixel, worked out in the tent"
    assert not drawn["both_out"].any() and not drawn["nan_end"].any()
    # random rows around a camera inside them, with and without a depth plane
    for E, (W, V) in zip(C.ROWS, itertools.cycle([(33, 2), (67, 5), (1, 1)])):
        K, M = C.cameras(V, C.height(W), W)
        rows = C.cloud_rows(E)
        depth = EO.depth_window_max(C.reference_cloud(65, W, V), 1, backend="host").numpy()
        for d, slack in ((None, 0.0), (depth, 0.01)):
            got = MC.row_masks(rows, K, M, C.height(W), W, d, slack, backend="host", near_clip=C.NEAR).numpy()
            assert C.same_bits(got, C.contours_clipped_brute(rows, K, M, C.height(W), W, d, slack)), (E, W, V, d is None)


# ------------------------------------------------------------------------------------------------ the indoor fixture
def check_room(backend):
    """The point of the feature, shared with the GPU tests.  Returns the clipped scan."""
    V, H, W = ROOM
    room = SS.solid_scan("room", V, H, W, backend=backend)
    assert room.tris.shape == (24, 3, 3) and len(room.edges["lines_end_pts"]) == 24 and room.edges["curves_ctl_pts"] == []
    assert np.isfinite(room.depth).all(), "inside a closed room every pixel has a surface"
    assert ((room.maps != 0).sum((1, 2)) > 0).all(), "every view keeps some samples"
    unclipped = SS.solid_scan("room", V, H, W, backend=backend, clip=False)
    assert np.isinf(unclipped.depth).any(), "without clipping the walls that reach behind the camera are dropped"
    assert (room.hidden != unclipped.hidden).any() and (room.hidden >= unclipped.hidden).all()
    # scoring the ground truth with the mesh as the occluder and near_clip reproduces the maps
    res = R.score_edges(room.edges, room.cameras, room.maps, "PidiNet", backend=backend, occluder=room.tris,
                        near_clip=EO.NEAR_CLIP)
    agg = res["aggregate"]
    assert agg["precision"] == [1.0, 1.0, 1.0] and agg["recall"] == [1.0, 1.0, 1.0], agg
    assert agg["n_pred"] == agg["n_det"] == int((room.maps != 0).sum())
    assert [row["hidden_points"] for row in res["views"]] == room.hidden.tolist()
    assert res["settings"]["near_clip"] == EO.NEAR_CLIP and list(res["settings"])[-1] == "near_clip"
    # ... and without near_clip it does not: the gate sees through the dropped walls
    res0 = R.score_edges(room.edges, room.cameras, room.maps, "PidiNet", backend=backend, occluder=room.tris)
    assert "near_clip" not in res0["settings"]
    assert [row["hidden_points"] for row in res0["views"]] == unclipped.hidden.tolist() != room.hidden.tolist()
    for row, row0 in zip(res["views"], res0["views"]):
        assert row["kept_points"] + row["hidden_points"] == row0["kept_points"] + row0["hidden_points"]
    return room


def test_the_room_needs_clipping_and_its_ground_truth_scores_one_with_it():
    room = check_room("host")
    eyes = np.array([-c.R.T @ c.T for c in room.cameras])
    (x0, y0), (x1, y1), z0, z1 = SS.ROOM_BOX
    assert (np.minimum(eyes - [x0, y0, z0], [x1, y1, z1] - eyes) >= 0.1).all(), "every eye is 0.1 inside the room"
    (px0, py0), (px1, py1), _, pz1 = SS.ROOM_PILLAR
    gap = np.maximum(np.maximum([px0, py0] - eyes[:, :2], eyes[:, :2] - [px1, py1]), 0.0)
    assert (np.hypot(gap[:, 0], gap[:, 1]) >= 0.1).all(), "and 0.1 from the pillar"
    assert "room" not in SS.SHAPES and SS.INDOOR_SHAPES == ("room",)
    # most (triangle, view) pairs of the walls straddle the camera plane
    K, M = camera_arrays(room.cameras)
    z = np.einsum("vk,ftk->vft", M.reshape(-1, 3, 4)[:, 2, :3], room.tris.astype(np.float64)) + M.reshape(-1, 3, 4)[:, 2, 3][:, None, None]
    assert ((z <= 0).any(2) & (z > 0).any(2)).sum() > 50


# ------------------------------------------------------------------------------------------------ operators, settings
def _box():
    return SS.solid_scan("box", 3, 24, 32, backend="host")


def test_near_clip_is_checked_and_recorded_only_when_given():
    s = _box()
    g = EO.ChunkDepth("x", s.cameras, occluder=s.tris, near_clip=0.02)
    assert g.settings() == {"occluder": True, "depth_slack": EO.DEPTH_SLACK, "depth_window": EO.DEPTH_WINDOW, "near_clip": 0.02}
    assert list(g.settings())[-1] == "near_clip"
    assert "near_clip" not in EO.ChunkDepth("x", s.cameras, occluder=s.tris).settings()
    assert EO.NEAR_CLIP == 0.01
    for bad in (0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="near_clip must be finite and > 0"):
            EO.ChunkDepth("x", s.cameras, occluder=s.tris, near_clip=bad)
        with pytest.raises(ValueError, match="near_clip must be finite and > 0"):
            EO.mesh_depth(s.tris, *camera_arrays(s.cameras), 24, 32, backend="host", near_clip=bad)
        with pytest.raises(ValueError, match="near_clip must be finite and > 0"):
            MC.row_masks(np.zeros((0, 4, 3), np.float32), *camera_arrays(s.cameras), 24, 32, backend="host", near_clip=bad)
    # with depth_maps, or with no depth source, every scan-level operator rejects it
    calls = {
        "score_edges": lambda **kw: R.score_edges(s.edges, s.cameras, s.maps, "PidiNet", backend="host", **kw),
        "edge_support": lambda **kw: SP.edge_support(s.edges, s.cameras, s.maps, "PidiNet", backend="host", **kw),
        "trim_edges": lambda **kw: TR.trim_edges(s.edges, s.cameras, s.maps, "PidiNet", backend="host", **kw),
        "snap_edges": lambda **kw: SN.snap_edges(s.edges, s.cameras, s.maps, "PidiNet", backend="host", iterations=1, **kw),
        "seed_points": lambda **kw: SD.seed_points(s.cameras, s.maps, "PidiNet", ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0)), grid=8,
                                                   backend="host", **kw),
    }
    for name, call in calls.items():
        for kw in (dict(depth_maps=list(s.depth)), {}):
            with pytest.raises(ValueError, match=f"{name}: near_clip needs an occluder"):
                call(near_clip=0.01, **kw)
        res = call(occluder=s.tris, near_clip=0.01)
        res = res[1] if isinstance(res, tuple) else res
        settings = res["settings"] if "settings" in res else res
        assert settings["near_clip"] == 0.01, name
        # seen from outside the clipped planes are the unclipped ones: nothing else in the result moves
        plain = call(occluder=s.tris)
        plain = plain[1] if isinstance(plain, tuple) else plain
        assert "near_clip" not in (plain["settings"] if "settings" in plain else plain), name
        strip = lambda d: json.dumps({k: v for k, v in d.items() if k != "settings"}, sort_keys=True, default=_plain)
        rest = lambda d: {k: v for k, v in (d["settings"] if "settings" in d else d).items() if k != "near_clip"}
        assert strip(res) == strip(plain) or "settings" not in res, name
        assert json.dumps(rest(res), default=_plain) == json.dumps(rest(plain), default=_plain), name


def _plain(o):
    return np.asarray(o.cpu() if hasattr(o, "cpu") else o).tolist()


def _key_order(o):
    """The keys of a parsed JSON value, in their order, all the way down."""
    if isinstance(o, dict):
        return [(k, _key_order(v)) for k, v in o.items()]
    if isinstance(o, list):
        return [_key_order(v) for v in o]
    return type(o).__name__


def test_without_the_option_every_output_is_what_the_commit_before_it_wrote(tmp_path, capsys):
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    try:
        from make_edge_clip_golden import DST, recordings
    finally:
        sys.path.pop(0)
    want = json.load(open(DST))
    got = recordings(str(tmp_path))
    capsys.readouterr()
    assert sorted(got) == sorted(want)
    for name in want:
        g, w = json.loads(got[name]), json.loads(want[name])
        # the settings byte for byte; every key, in its order; every number exactly as parsed (not as printed: the recorded
        # float64 results of the numpy back end are compared as numbers, so only a different VALUE fails)
        if name.startswith("settings_"):
            assert got[name] == want[name], name
        elif "settings" in w:
            assert json.dumps(g["settings"]) == json.dumps(w["settings"]), name
        assert _key_order(g) == _key_order(w), name
        assert g == w, name
    assert want["settings_none"] == "{}" and all("near_clip" not in text for text in want.values())


def test_command_lines(tmp_path, capsys, monkeypatch):
    scan_dir = tmp_path / "data" / "room"
    V, H, W = 6, 30, 40
    assert SS.main(["room", str(scan_dir), "--views", str(V), "--height", str(H), "--width", str(W), "--backend", "host"]) == 0
    assert f"room: {V} views of {W}x{H}, 24 triangles, 24 lines, 0 curves" in capsys.readouterr().out
    scan = SS.solid_scan("room", V, H, W, backend="host")
    out = tmp_path / "out"
    os.makedirs(out / "room")
    with open(out / "room" / "parametric_edges.json", "w") as f:
        json.dump(scan.edges, f)
    common = ["--base_dir", str(out), "--dataset_dir", str(tmp_path / "data"), "--detector", "PidiNet", "--backend", "host",
              "--occluder", "mesh.ply"]
    score = out / "room" / R.SCORE_FILE
    # the bare flag is NEAR_CLIP, a value is itself, and without the flag nothing is recorded
    for flags, near in ((["--near_clip"], EO.NEAR_CLIP), (["--near_clip", "0.02"], 0.02), ([], None)):
        assert R.main(common + flags) == 0
        got = json.loads(score.read_text())
        assert got["settings"].get("near_clip") == near, flags
        if near == EO.NEAR_CLIP:   # the planes the maps were drawn with
            assert got["aggregate"]["precision"] == [1.0, 1.0, 1.0] == got["aggregate"]["recall"], got["aggregate"]
            hidden_clipped = [row["hidden_points"] for row in got["views"]]
        elif near is None:
            assert [row["hidden_points"] for row in got["views"]] != hidden_clipped, "the gate sees through the dropped walls"
    with pytest.raises(ValueError, match="near_clip needs an occluder"):
        R.main(common[:-2] + ["--near_clip"])
    sup_common = common + ["--tolerances", "1", "2", "--keep_tolerance", "1", "--snap", "--snap_iterations", "1", "--trim"]
    assert SUP.main(sup_common + ["--near_clip"]) == 0
    for n in (SUP.SUPPORT_FILE, SUP.TRIM_FILE, SUP.SNAP_FILE):
        assert json.loads((out / "room" / n).read_text())["settings"]["near_clip"] == EO.NEAR_CLIP, n
    assert SUP.main(sup_common) == 0
    for n in (SUP.SUPPORT_FILE, SUP.TRIM_FILE, SUP.SNAP_FILE):
        assert "near_clip" not in json.loads((out / "room" / n).read_text())["settings"], n
    capsys.readouterr()
    from curve_gaussian_amd import edge_seed_cli as CLI
    args = CLI.parser().parse_args(["--scan", str(scan_dir), "--out", "x.ply", "--occluder", "mesh.ply", "--near_clip"])
    assert CLI.seed_options(args)["near_clip"] == EO.NEAR_CLIP
    args = CLI.parser().parse_args(["--scan", str(scan_dir), "--out", "x.ply", "--occluder", "mesh.ply"])
    assert "near_clip" not in CLI.seed_options(args)
    from curve_gaussian_amd import train
    base = ["-s", str(scan_dir), "-m", str(out / "m")]
    _, _, a = train.parse_args(base + ["--occluder", "mesh.ply", "--near_clip", "--gate_edge_checks"])
    assert a.near_clip == EO.NEAR_CLIP and a.init_near_clip is None
    assert train.gate_options(a, str(scan_dir), scan.cameras)["near_clip"] == EO.NEAR_CLIP
    dataset, _, a = train.parse_args(base + ["--init", "edge_votes", "--init_occluder", "mesh.ply", "--init_near_clip", "0.03"])
    assert dataset.init_options["near_clip"] == 0.03 and a.near_clip is None
    dataset, _, a = train.parse_args(base + ["--init", "edge_votes", "--init_occluder", "mesh.ply"])
    assert "near_clip" not in dataset.init_options
    for bad in (["--near_clip"], ["--init_near_clip"]):
        with pytest.raises(SystemExit):
            train.parse_args(base + bad)
    capsys.readouterr()


# ------------------------------------------------------------------------------------------------ the C ABI
def test_abi_argument_checks_are_pinned():
    """Status and the exact text of cgs_last_error() for every rejection of the two entries; the pointers are dummies that
    are never dereferenced, and no row passes validation with work to do (V = 0 is the only accepted call)."""
    from curve_gaussian_amd import _lib
    from test_edge_occlusion_cpu import _pinned
    lib = _lib.load()
    p, q = ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 24)

    def mesh(F=3, tris=p, V=2, intr=p, w2c=p, H=4, W=6, near=0.01, depth=p):
        return lib.cgs_mesh_depth_clipped(F, tris, V, intr, w2c, H, W, near, depth, None)

    plane = "the plane is finite and > 0)"
    _pinned(lib, "cgs_mesh_depth_clipped", "cgs_mesh_depth_clipped: invalid argument ", mesh,
            [(dict(F=-1), "(F=-1, V=2)"), (dict(V=-1, H=0), "(F=3, V=-1)"),
             (dict(H=0, near=0.0), "(height=0, width=6; sizes lie in [1, 16384])"),
             (dict(W=16385, V=0), "(height=4, width=16385; sizes lie in [1, 16384])"),
             (dict(near=0.0), f"(near=0; {plane}"), (dict(near=-0.5, V=0), f"(near=-0.5; {plane}"),
             (dict(near=float("nan"), tris=None), f"(near=nan; {plane}"), (dict(near=float("inf")), f"(near=inf; {plane}"),
             (dict(tris=None), "(NULL pointer; F=3)"), (dict(intr=None), "(NULL pointer; F=3)"),
             (dict(w2c=None, V=0), "(NULL pointer; F=3)"), (dict(depth=None, F=0), "(NULL pointer; F=0)")],
            [dict(V=0), dict(V=0, F=0, tris=None)])

    def contours(E=3, edges=p, V=2, intr=p, w2c=p, H=4, W=6, depth=p, slack=0.001, near=0.01, mask=q):
        return lib.cgs_mesh_contours_clipped(E, edges, V, intr, w2c, H, W, depth, slack, near, mask, None)

    _pinned(lib, "cgs_mesh_contours_clipped", "cgs_mesh_contours_clipped: invalid argument ", contours,
            [(dict(E=-1), "(E=-1, V=2)"), (dict(V=-1, W=0), "(E=3, V=-1)"),
             (dict(H=16385), "(height=16385, width=6; sizes lie in [1, 16384])"),
             (dict(W=0, V=0), "(height=4, width=0; sizes lie in [1, 16384])"),
             (dict(slack=-1e-3, near=0.0), "(slack=-0.001; with a depth plane the slack is finite and >= 0)"),
             (dict(slack=float("nan"), V=0), "(slack=nan; with a depth plane the slack is finite and >= 0)"),
             (dict(near=0.0), f"(near=0; {plane}"), (dict(near=-1.0, depth=None, slack=-1.0), f"(near=-1; {plane}"),
             (dict(near=float("nan"), V=0), f"(near=nan; {plane}"), (dict(near=float("inf"), mask=None), f"(near=inf; {plane}"),
             (dict(edges=None), "(NULL pointer; E=3)"), (dict(intr=None), "(NULL pointer; E=3)"),
             (dict(w2c=None, V=0), "(NULL pointer; E=3)"), (dict(mask=None, E=0), "(NULL pointer; E=0)")],
            [dict(V=0), dict(V=0, E=0, edges=None), dict(V=0, depth=None, slack=float("nan"))])
    i, vp, d = ctypes.c_int, ctypes.c_void_p, ctypes.c_double
    assert _lib.SIGNATURES["cgs_mesh_depth_clipped"] == (i, [i, vp, i, vp, vp, i, i, d, vp, vp])
    assert _lib.SIGNATURES["cgs_mesh_contours_clipped"] == (i, [i, vp, i, vp, vp, i, i, vp, d, d, vp, vp])
    header = open(os.path.join(ROOT, "include", "curvegs.h")).read()
    assert "p2 = near" in header and "0 < c2 < near is still SEEN" in header
