"""CPU: plane-sweep stereo (cgs_stereo_sweep / cgs_stereo_consistency, include/curvegs.h) on the host back end of
ops.stereo_depth: against the brute force of stereo_cases.py bit for bit, the named cases, one exact construction, the
purpose -- a gate fed stereo maps scores the box's ground truth with a higher precision than no gate -- and the tool."""
import ctypes
import json
import os
import re

import numpy as np
import pytest

import stereo_cases as SC
from curve_gaussian_amd import _lib
from curve_gaussian_amd.ops import edge_occlusion as EO
from curve_gaussian_amd.ops import stereo_depth as SD
from curve_gaussian_amd.scene import solid_scan as SS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def host_sweep(case):
    return SD.sweep(*SC.sweep_args(case), backend="host").numpy()


# ------------------------------------------------------------------------------------------------ the brute force
@pytest.mark.parametrize("H,W,R", [(1, 1, 0), (1, 1, 1), (5, 7, 0), (5, 7, 1), (9, 11, 0), (9, 11, 1)])
def test_host_equals_brute_force(H, W, R):
    case = SC.random_case(3, H, W, 4, 3, R, 7 * H + R)
    assert (case["src"] == -1).sum() == 3                       # one -1 among every view's sources
    got, want = host_sweep(case), SC.brute_sweep(*SC.sweep_args(case))
    assert SC.same_bits(got, want)
    if (H, W) == (1, 1) or R == 0:
        assert not got.any()            # the patch does not fit, or (R = 0) its one tap has no variance: var_r == 0 > thr fails
    else:
        assert (got > 0).any()


NAMED = SC.named_cases()


@pytest.mark.parametrize("name", sorted(NAMED))
def test_named_case(name):
    case, check = NAMED[name]
    got = host_sweep(case)
    assert SC.same_bits(got, SC.brute_sweep(*SC.sweep_args(case)))
    check(got)


def test_nan_pose_equals_the_source_left_out():
    case, _ = NAMED["nan_pose"]
    without = dict(case, src=case["src"].copy())
    without["src"][0, 0] = -1
    assert SC.same_bits(host_sweep(case), host_sweep(without))
    assert (host_sweep(case)[0] > 0).any()


def test_cost_tie_and_den_edge_are_what_the_brute_force_sees():
    """The named cases' constructions, looked at from inside the brute force: equal costs at two hypotheses, and a
    winner whose later neighbour costs the same."""
    trace = {}
    case, _ = NAMED["cost_tie"]
    SC.brute_sweep(*SC.sweep_args(case), trace=trace)
    assert any(best == 0 and costs[0] == costs[1] == 0.0 for best, costs in trace.values())
    trace = {}
    case, _ = NAMED["den_edge"]
    SC.brute_sweep(*SC.sweep_args(case), trace=trace)
    assert any(best == 1 and costs[0] > costs[1] == costs[2] for best, costs in trace.values())


def test_exact_construction_stays_within_half_a_step():
    """A fronto-parallel value-noise plane at hypothesis k's depth, two cameras a sideways translation apart whose
    disparity there is 4 pixels: fx = 64, t = 1 / 8, inv[k] = 1 / 2, all exact in float64.  The winner is k wherever a
    depth is stored, so the clamp keeps the refined inverse depth within half a step of inv[k]; the map is float32, which
    adds its own rounding of the depth (2^-24 relative)."""
    H, W, D, k = 24, 40, 9, 4
    inv = np.linspace(0.75, 0.25, D)
    assert inv[k] == 0.5 and inv[1] - inv[0] == -0.0625
    ii, jj = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    plane = np.stack([jj / 64.0 * 2.0, ii / 64.0 * 2.0, np.full((H, W), 2.0)], -1)
    base = np.rint(255.0 * SS.value_noise(plane)).astype(np.uint8)
    gray = SC.shifted_views(base, (0, 4))
    K = np.tile(np.array([64.0, 64.0, 32.0, 24.0]), (2, 1))
    src = np.array([[1], [-1]], np.int32)
    rel = np.zeros((2, 1, 12))
    rel[0, 0] = np.concatenate([np.eye(3), np.array([[0.125], [0.0], [0.0]])], 1).reshape(12)
    out = SD.sweep(gray, K, np.tile(inv, (2, 1)), src, rel, 2, 1.0, 0.5, 1, backend="host").numpy()
    # interior: the patch fits and hypothesis k's footprints, 4 columns to the right, lie inside the source
    inner = out[0][2:H - 3, 2:W - 2 - 4 - 1]
    assert not out[1].any() and (inner > 0).sum() >= 1
    q = 1.0 / inner[inner > 0].astype(np.float64)
    assert (np.abs(q - inv[k]) <= 0.5 * 0.0625 + inv[k] * 2.0 ** -23).all()
    assert (np.abs(q - inv[k]) <= 0.25 * 0.0625).mean() > 0.9      # (not asserted by the issue: most sit far inside)


# ------------------------------------------------------------------------------------------------ consistency
def host_consistency(c, min_consistent):
    return SD.consistency(c["depth"], c["K"], c["src"], c["rel"], c["tol"], min_consistent, backend="host").numpy()


@pytest.mark.parametrize("V,H,W,S,mc", [(3, 5, 7, 3, 1), (3, 9, 11, 3, 2), (1, 1, 1, 1, 1), (4, 6, 5, 2, 0)])
def test_consistency_equals_brute_force(V, H, W, S, mc):
    c = SC.random_consistency_case(V, H, W, S, 40 + V + H)
    got = host_consistency(c, mc)
    assert SC.same_bits(got, SC.brute_consistency(c["depth"], c["K"], c["src"], c["rel"], c["tol"], mc))
    if V > 1 and mc > 0:
        assert (got > 0).any() and ((c["depth"] > 0) & (got == 0)).any()


def test_consistency_named_cases():
    c = SC.consistency_case()
    # view 1 at column 4: lands on columns 2 and 6 of views 0 and 2, both at depth 2 -> two agree
    both = host_consistency(c, 2)
    assert SC.same_bits(both, SC.brute_consistency(c["depth"], c["K"], c["src"], c["rel"], c["tol"], 2))
    assert both[1, 3, 4] == np.float32(2.0)
    assert both[1, 3, 0] == 0.0                                  # column -2 of view 0 is outside: one agrees, two are asked
    # exactly min_consistent agreeing sources: kept bit for bit
    odd = dict(c, depth=c["depth"].copy())
    odd["depth"][1, 3, 4] = np.float32(2.0000002)
    kept = host_consistency(odd, 2)
    assert kept[1, 3, 4].view(np.uint32) == odd["depth"][1, 3, 4].view(np.uint32)
    # a source with depth 0 never agrees, however large the tolerance
    zero = dict(c, depth=c["depth"].copy(), tol=np.full((3,), np.inf))
    zero["depth"][2] = 0.0
    got = host_consistency(zero, 2)
    assert SC.same_bits(got, SC.brute_consistency(zero["depth"], zero["K"], zero["src"], zero["rel"], zero["tol"], 2))
    assert not got.any()
    assert (host_consistency(zero, 1)[1] == np.float32(2.0)).any()
    # no agreeing source: every map at another depth
    apart = SC.consistency_case(zs=(2.0, 3.0, 4.0))
    assert not host_consistency(apart, 1).any()


# ------------------------------------------------------------------------------------------------ the Python layer
def test_luminance():
    rgb = np.array([[[255, 0, 0], [0, 255, 0], [0, 0, 255], [255, 255, 255], [12, 200, 99]]], np.uint8)
    want = [(299 * r + 587 * g + 114 * b + 500) // 1000 for r, g, b in rgb[0].tolist()]
    assert SD.luminance(rgb)[0].tolist() == want == [76, 150, 29, 255, 132]
    rgba = np.concatenate([rgb, np.full((1, 5, 1), 7, np.uint8)], 2)
    assert (SD.luminance(rgba) == SD.luminance(rgb)).all()
    grey = np.arange(12, dtype=np.uint8).reshape(3, 4)
    assert (SD.luminance(grey) == grey).all()
    with pytest.raises(ValueError):
        SD.luminance(grey.astype(np.float32))


def test_plan_views():
    cams = SS.emap_cameras_of(SS.arc_cameras(5, 12, 16))
    plan = SD.plan_views(cams, hypotheses=8, sources=2)
    assert [sorted(r) for r in plan.src.tolist()] == [[1, 2], [0, 2], [1, 3], [2, 4], [2, 3]]      # the nearest centres
    assert plan.src[0].tolist() == [1, 2] and plan.src[4].tolist() == [3, 2]                       # ... nearest first
    twin = SD.plan_views([cams[0], cams[3], cams[1], cams[1]], hypotheses=8, sources=2)
    assert twin.src[0].tolist() == [2, 3]                                                          # a tie: the lower index
    assert plan.usable.all() and plan.inv.shape == (5, 8)
    z = np.array([[x, y, zz] for x in (0, 1) for y in (0, 1) for zz in (0, 1)], np.float64) @ cams[0].R[2] + cams[0].T[2]
    assert plan.inv[0][0] == 1.0 / z.min() and plan.inv[0][-1] == 1.0 / z.max()
    assert np.allclose(plan.tol, 1.5 * np.abs(plan.inv[:, 1] - plan.inv[:, 0]), rtol=0, atol=0)
    # rel takes reference-camera coordinates to the source's
    X = np.array([0.4, 0.6, 0.5])
    ref, srcc = cams[0].R @ X + cams[0].T, cams[1].R @ X + cams[1].T
    M = plan.rel[0, 0].reshape(3, 4)
    assert np.allclose(M[:, :3] @ ref + M[:, 3], srcc, atol=1e-12)
    # a narrow angle leaves too few sources: the view is not swept; a camera inside the bounds is floored
    assert not SD.plan_views(cams, hypotheses=8, sources=2, max_angle_deg=1.0).usable.any()
    inside = SD.plan_views(cams, bounds=((-3, -3, -3), (3, 3, 3)), hypotheses=8, sources=2)
    assert (inside.inv[:, 0] == 1.0 / SD.STEREO_Z_FLOOR).all()


def test_mixed_sizes_and_unswept_views():
    small = SS.solid_scan("box", 3, 12, 16, backend="host", synth_cameras=SS.arc_cameras(3, 12, 16))
    large = SS.solid_scan("box", 1, 16, 12, backend="host", synth_cameras=SS.arc_cameras(1, 16, 12))
    cams = [small.cameras[0], large.cameras[0], small.cameras[1], small.cameras[2]]
    ph_s, ph_l = SS.photographs(small), SS.photographs(large)
    maps, info = SD.stereo_depth([ph_s[0], ph_l[0], ph_s[1], ph_s[2]], cams, hypotheses=8, patch_radius=1, sources=2,
                                 backend="host", return_info=True)
    assert [m.shape for m in maps] == [(12, 16), (16, 12), (12, 16), (12, 16)] and all(m.dtype == np.float32 for m in maps)
    assert info["swept"] == [True, False, True, True] and not maps[1].any()   # a lone view of its size has no source
    alone = SD.stereo_depth(list(ph_s), small.cameras, hypotheses=8, patch_radius=1, sources=2, backend="host")
    assert all(SC.same_bits(a, b) for a, b in zip(alone, [maps[0], maps[2], maps[3]]))
    with pytest.raises(ValueError):
        SD.stereo_depth([ph_l[0]], [small.cameras[0]], backend="host")
    with pytest.raises(ValueError):
        SD.stereo_depth(list(ph_s), small.cameras, patch_radius=SD.MAX_RADIUS + 1, backend="host")


# ------------------------------------------------------------------------------------------------ the purpose
def box_arc():
    scan = SS.solid_scan("box", 8, 48, 64, backend="host", synth_cameras=SS.arc_cameras(8, 48, 64))
    return scan, SS.photographs(scan)


def gate_pairs(scan, planes, slack):
    """(seen, hidden) bool [V,P] of the ground-truth samples under depth planes (already widened)."""
    from curve_gaussian_amd.edge_extraction.abc import pred_points_and_directions
    from curve_gaussian_amd.ops.view_chunks import camera_arrays
    K, M = camera_arrays(scan.cameras)
    M = np.asarray(M, np.float64).reshape(len(K), 12)
    pts = np.ascontiguousarray(pred_points_and_directions(scan.edges, SS.SAMPLE_RESOLUTION).points, np.float32).reshape(-1, 3)
    rows = [EO.gate_view_host(pts, K[v], M[v], planes[v], slack) for v in range(len(K))]
    return np.stack([r[2] | r[3] for r in rows]), np.stack([r[3] for r in rows])


def stereo_quality(scan, maps, hypotheses, sources):
    """The figures of profiles/stereo_depth.md against ``mesh_depth`` of the same solid (``scan.depth``)."""
    plan = SD.plan_views(scan.cameras, hypotheses=hypotheses, sources=sources)
    given = covered = in1 = in2 = near = stray = 0
    for v, m in enumerate(maps):
        mesh, has = np.isfinite(scan.depth[v]), m > 0
        both = has & mesh
        err = (1.0 / m[both].astype(np.float64) - 1.0 / scan.depth[v][both].astype(np.float64)) / abs(plan.inv[v][1] - plan.inv[v][0])
        given, covered, stray = given + int(both.sum()), covered + int(mesh.sum()), stray + int((has & ~mesh).sum())
        in1, in2, near = in1 + int((np.abs(err) <= 1).sum()), in2 + int((np.abs(err) <= 2).sum()), near + int((err > 2).sum())
    return {"coverage": given / max(covered, 1), "within_1_step": in1 / max(given, 1), "within_2_steps": in2 / max(given, 1),
            "too_near_by_more_than_2": near / max(given, 1), "depth_where_mesh_has_none": stray}


def test_stereo_gate_raises_the_precision_on_the_box():
    """The purpose, against the ungated behaviour: 8 views of the box on an arc 8 degrees apart, 48 x 64, D = 32, R = 2,
    S = 2.  Printed, not asserted (profiles/stereo_depth.md): the quality against the mesh's depth and the pairs each
    gate hides."""
    from curve_gaussian_amd.edge_extraction.reprojection import score_edges
    scan, photos = box_arc()
    maps, info = SD.stereo_depth(list(photos), scan.cameras, hypotheses=32, patch_radius=2, sources=2, backend="host",
                                 return_info=True)
    slack = info["recommended_slack"]
    plain = score_edges(scan.edges, scan.cameras, scan.maps, "PidiNet", backend="host")["aggregate"]
    gated = score_edges(scan.edges, scan.cameras, scan.maps, "PidiNet", backend="host", depth_maps=maps,
                        depth_slack=slack)["aggregate"]
    stereo_planes = EO.depth_window_max(np.stack(EO.check_depth_maps(scan.cameras, maps)), EO.DEPTH_WINDOW, backend="host").numpy()
    mesh_planes = EO.depth_window_max(scan.depth, EO.DEPTH_WINDOW, backend="host").numpy()
    seen, hid_s = gate_pairs(scan, stereo_planes, slack)
    _, hid_m = gate_pairs(scan, mesh_planes, EO.DEPTH_SLACK)
    mesh_sees = seen & ~hid_m
    share = float((mesh_sees & hid_s).sum()) / float(mesh_sees.sum())
    print("stereo quality:", json.dumps(stereo_quality(scan, maps, 32, 2)))
    print("pairs seen %d, hidden by both %d, by stereo only %d, by the mesh only %d; recommended_slack %.4f" % (
        seen.sum(), (hid_s & hid_m).sum(), (hid_s & ~hid_m).sum(), (hid_m & ~hid_s).sum(), slack))
    print("precision at 1 px %.4f -> %.4f, recall at 1 px %.4f -> %.4f (share %.4f)" % (
        plain["precision"][0], gated["precision"][0], plain["recall"][0], gated["recall"][0], share))
    assert gated["precision"][0] > plain["precision"][0]
    assert gated["recall"][0] >= plain["recall"][0] - share


# ------------------------------------------------------------------------------------------------ the fixture and the tool
def _files(root):
    return {os.path.relpath(os.path.join(d, f), root): open(os.path.join(d, f), "rb").read()
            for d, _, fs in os.walk(root) for f in fs}


def test_photographs_and_the_photos_flag(tmp_path):
    scan = SS.solid_scan("box", 3, 24, 32, backend="host", synth_cameras=SS.arc_cameras(3, 24, 32))
    ph = SS.photographs(scan)
    assert ph.dtype == np.uint8 and ph.shape == (3, 24, 32)
    assert ((ph == SS.PHOTO_BACKGROUND) | np.isfinite(scan.depth)).all() and ph[np.isfinite(scan.depth)].std() > 10
    assert (SS.photographs(scan) == ph).all()
    SS.write_solid_scan(str(tmp_path / "plain"), scan)
    SS.write_solid_scan(str(tmp_path / "photos"), scan, photos=True)
    plain, photos = _files(str(tmp_path / "plain")), _files(str(tmp_path / "photos"))
    assert not any(k.startswith("color") for k in plain)
    assert {k: v for k, v in photos.items() if not k.startswith("color")} == plain       # byte for byte what it was
    assert sorted(k for k in photos if k.startswith("color")) == [f"color/{i}_colors.png" for i in range(3)]
    from PIL import Image
    assert (np.array(Image.open(tmp_path / "photos" / "color" / "1_colors.png")) == ph[1]).all()


def test_tool(tmp_path):
    from curve_gaussian_amd import stereo_depth as TOOL
    from curve_gaussian_amd.edge_extraction import reprojection as RP
    scan_dir = str(tmp_path / "box")
    assert SS.main(["box", scan_dir, "--views", "4", "--height", "24", "--width", "32", "--backend", "host", "--photos",
                    "--arc"]) == 0
    args = ["--scan", scan_dir, "--backend", "host", "--hypotheses", "12", "--patch_radius", "1", "--sources", "2"]
    assert TOOL.main(args) == 0
    out = os.path.join(scan_dir, "depth_stereo")
    assert sorted(os.listdir(out)) == [f"{i}_colors.npy" for i in range(4)] + ["stereo.json"]
    report = json.load(open(os.path.join(out, "stereo.json")))
    for key, want in (("hypotheses", 12), ("patch_radius", 1), ("sources", 2), ("max_angle_deg", SD.MAX_ANGLE_DEG),
                      ("min_var", SD.MIN_VAR), ("max_cost", SD.MAX_COST), ("min_sources", SD.MIN_SOURCES),
                      ("consistency_steps", SD.CONSISTENCY_STEPS), ("min_consistent", SD.MIN_CONSISTENT),
                      ("bounds", [[0.0, 0.0, 0.0], [1.0, 1.0, 1.0]])):
        assert report[key] == want, key
    assert [r["name"] for r in report["views"]] == [f"{i}_colors.png" for i in range(4)]
    assert report["depth_step_max"] > 0 and report["recommended_slack"] == 2 * report["depth_step_max"]
    assert "0.001" in report["note"]
    cams, _ = RP.emap_cameras(scan_dir, "PidiNet")
    maps = EO.check_depth_maps(cams, RP.scan_depth_maps(out, cams))
    assert all(m.dtype == np.float32 and m.shape == (24, 32) and (m > 0).all() for m in maps)
    stored = [np.load(os.path.join(out, f"{i}_colors.npy")) for i in range(4)]
    assert all(s.dtype == np.float32 and (s >= 0).all() for s in stored) and any((s > 0).any() for s in stored)
    assert [r["coverage"] for r in report["views"]] == [float((s > 0).mean()) for s in stored]
    with pytest.raises(FileExistsError):
        TOOL.main(args)
    assert TOOL.main(args + ["--overwrite", "--out", out]) == 0
    from PIL import Image
    Image.fromarray(np.zeros((20, 32), np.uint8), mode="L").save(os.path.join(scan_dir, "color", "2_colors.png"))
    with pytest.raises(ValueError, match="2_colors.png"):
        TOOL.main(args + ["--out", str(tmp_path / "other")])
    assert not os.path.exists(tmp_path / "other")


# ------------------------------------------------------------------------------------------------ the ABI
def test_signatures_and_header():
    i, vp, d = ctypes.c_int, ctypes.c_void_p, ctypes.c_double
    assert _lib.SIGNATURES["cgs_stereo_sweep"] == (i, [i, i, i, vp, vp, i, vp, i, vp, vp, i, d, d, i, vp, vp])
    assert _lib.SIGNATURES["cgs_stereo_consistency"] == (i, [i, i, i, vp, vp, i, vp, vp, vp, i, vp, vp])
    header = open(os.path.join(ROOT, "include", "curvegs.h")).read()
    assert int(re.search(r"#define CGS_STEREO_MAX_RADIUS (\d+)", header).group(1)) == _lib.STEREO_MAX_RADIUS == SD.MAX_RADIUS
    lib = _lib.load()
    assert hasattr(lib, "cgs_stereo_sweep") and hasattr(lib, "cgs_stereo_consistency")


def test_entries_reject_before_any_launch():
    """Argument lists that must not pass validation (dummy pointers, never dereferenced)."""
    lib, A = _lib.load(), ctypes.c_void_p(64)
    good = [2, 8, 8, A, A, 4, A, 2, A, A, 1, 1.0, 0.5, 1, A, None]
    for pos, bad in ((0, -1), (1, 0), (2, _lib.EDT_MAX_SIZE + 1), (3, None), (5, 0), (7, 0), (10, -1),
                     (10, _lib.STEREO_MAX_RADIUS + 1), (11, -1.0), (11, float("nan")), (12, float("nan")), (13, 0), (14, None)):
        args = list(good)
        args[pos] = bad
        assert lib.cgs_stereo_sweep(*args) == -1, (pos, bad)
        assert _lib.last_error().startswith("cgs_stereo_sweep: invalid argument")
    good = [2, 8, 8, A, A, 2, A, A, A, 1, ctypes.c_void_p(64 + 4096), None]
    for pos, bad in ((0, -1), (1, 0), (3, None), (5, 0), (8, None), (9, -1), (10, None), (10, ctypes.c_void_p(64 + 256))):
        args = list(good)
        args[pos] = bad
        assert lib.cgs_stereo_consistency(*args) == -1, (pos, bad)
        assert _lib.last_error().startswith("cgs_stereo_consistency: invalid argument")
    assert "overlap" in _lib.last_error()
