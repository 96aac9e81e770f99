"""CPU: fusing the stereo depth maps across views (cgs_stereo_warp / cgs_stereo_fuse, include/curvegs.h) on the host back
end of ops.stereo_depth: against the brute force of stereo_fuse_cases.py bit for bit, one exact construction, the named
cases, the chunking, the purpose -- the fused maps cover and hide more than the filtered ones without hiding what the
unfiltered sweep does not -- the tool and the ABI."""
import ctypes
import functools
import json
import os
import re

import numpy as np
import pytest

import stereo_fuse_cases as FC
from curve_gaussian_amd import _lib
from curve_gaussian_amd.ops import edge_occlusion as EO
from curve_gaussian_amd.ops import stereo_depth as SD
from curve_gaussian_amd.scene import solid_scan as SS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32


def host_warp(c, v0, nv):
    return SD.warp(c["depth"], c["K"], c["fsrc"], c["into"], v0, nv, backend="host").numpy()


def host_fuse(c, warped, min_support, v0):
    out, sup = SD.fuse(c["depth"], warped, c["tol"], min_support, v0, backend="host", return_support=True)
    return out.numpy(), sup.numpy()


# ------------------------------------------------------------------------------------------------ the brute force
@pytest.mark.parametrize("F", [1, 3, 16])
@pytest.mark.parametrize("H,W", [(1, 1), (5, 7), (9, 11)])
@pytest.mark.parametrize("V", [1, 2, 5])
def test_host_equals_brute_force(V, H, W, F):
    c = FC.random_case(V, H, W, F, 10 * V + H + F)
    assert (c["fsrc"] == -1).any() or F == 1
    assert (c["fsrc"] >= V).any() == (F - (F >= 2) > V - 1)        # an index beyond the views wherever a slot is left for it
    filled = dropped = kept = 0
    for v0, nv in FC.ranges(V):
        warped = host_warp(c, v0, nv)
        assert warped.shape == (nv, F, H, W) and FC.same_bits(warped, FC.brute_warp(c["depth"], c["K"], c["fsrc"], c["into"], v0, nv))
        for min_support in (1, 2, 3, F + 1, F + 2):
            out, sup = host_fuse(c, warped, min_support, v0)
            want, want_sup = FC.brute_fuse(c["depth"], warped, c["tol"], min_support, v0)
            assert FC.same_bits(out, want) and sup.dtype == np.uint8 and (sup == want_sup).all()
            assert ((out > 0) == (sup >= min_support)).all() and ((out == 0) == (sup == 0)).all()
            if min_support == F + 2:
                assert not out.any()
            own = SD._is_depth(c["depth"])
            if min_support == min(2, F) and (v0, nv) == (0, V):         # (one source alone fills only at min_support = 1)
                filled = int((~own & (out > 0)).sum())
            if min_support == 2 and (v0, nv) == (0, V):
                dropped, kept = int((own & (out == 0)).sum()), int((own & (out > 0)).sum())
    if V == 5 and H * W > 1:                                       # the interesting cases hold all three kinds of pixel
        assert filled > 0 and dropped > 0 and kept > 0, (filled, dropped, kept)


# ------------------------------------------------------------------------------------------------ the exact construction
def test_exact_construction():
    """Three cameras a sideways translation apart, a plane at depth 2.0, integer disparities: source w's column c lands on
    column c + 2 (v - w) of target v."""
    c = FC.exact_case()
    warped = host_warp(c, 0, 3)
    assert (warped[1, 0, :, 2:] == F32(2.0)).all() and np.isinf(warped[1, 0, :, :2]).all()      # view 0 into view 1: + 2
    assert (warped[1, 1, :, :-2] == F32(2.0)).all() and np.isinf(warped[1, 1, :, -2:]).all()    # view 2 into view 1: - 2
    # a hole punched into the middle view comes back as exactly 2.0 (its two sources agree)
    hole = dict(c, depth=c["depth"].copy())
    hole["depth"][1, 3, 4] = 0.0
    out, sup = host_fuse(hole, host_warp(hole, 0, 3), 2, 0)
    assert out[1, 3, 4] == F32(2.0) and sup[1, 3, 4] == 2 and sup[1, 3, 5] == 3
    # a pixel set to depth 1.0 in one view comes back as 2.0 at min_support = 2: the pair outvotes it
    odd = dict(c, depth=c["depth"].copy())
    odd["depth"][1, 3, 4] = 1.0
    out, sup = host_fuse(odd, host_warp(odd, 0, 3), 2, 0)
    assert out[1, 3, 4] == F32(2.0) and sup[1, 3, 4] == 2
    assert (out[1][:, 2:-2] == F32(2.0)).all()
    # with every other view zeroed nothing survives min_support = 2, and everything min_support = 1
    alone = dict(c, depth=c["depth"].copy())
    alone["depth"][[0, 2]] = 0.0
    warped = host_warp(alone, 0, 3)
    assert not host_fuse(alone, warped, 2, 0)[0][1].any()
    assert (host_fuse(alone, warped, 1, 0)[0][1] == F32(2.0)).all()
    for case in (hole, odd, alone):
        w = host_warp(case, 0, 3)
        assert FC.same_bits(w, FC.brute_warp(case["depth"], case["K"], case["fsrc"], case["into"], 0, 3))
        assert FC.same_bits(host_fuse(case, w, 2, 0)[0], FC.brute_fuse(case["depth"], w, case["tol"], 2, 0)[0])


# ------------------------------------------------------------------------------------------------ the named cases
def fuse_pixel(own, others, tol, min_support=1):
    depth, warped, tol = FC.pixel_case(own, others, tol)
    out, sup = SD.fuse(depth, warped, tol, min_support, backend="host", return_support=True)
    want, want_sup = FC.brute_fuse(depth, warped, tol, min_support, 0)
    assert FC.same_bits(out.numpy(), want) and (sup.numpy() == want_sup).all()
    return out.numpy()[0, 0, 0], int(sup.numpy()[0, 0, 0])


def test_a_support_tie_goes_to_the_farther_pair():
    assert fuse_pixel(2.0, [2.0, 4.0, 4.0], 0.01) == (F32(4.0), 2)
    assert fuse_pixel(4.0, [2.0, 4.0, 2.0], 0.01) == (F32(4.0), 2)
    assert fuse_pixel(2.0, [2.0, 2.0, 4.0, 4.0], 0.01) == (F32(2.0), 3)      # no tie: the larger cluster
    assert fuse_pixel(0.0, [2.0, 4.0], 0.01) == (F32(4.0), 1)                # two lone candidates tie at support 1
    assert fuse_pixel(0.0, [2.0, 4.0], 0.01, min_support=2) == (F32(0.0), 0)


def test_tolerances():
    inf, nan = float("inf"), float("nan")
    # tol = 0: only equal inverse depths cluster
    assert fuse_pixel(2.0, [2.0, 2.0000002, 4.0], 0.0) == (F32(2.0), 2)
    # tol = inf: every present candidate is a member; the mean of 1/2, 1/4, 1/4 is 1/3
    got, sup = fuse_pixel(2.0, [4.0, 0.0, 4.0, inf, nan, -3.0], inf)
    assert sup == 3 and got == F32(1.0 / (((0.5 + 0.25) + 0.25) / 3.0))
    # tol = NaN (and a negative one): no candidate supports even itself
    assert fuse_pixel(2.0, [2.0, 2.0], nan) == (F32(0.0), 0)
    assert fuse_pixel(2.0, [2.0, 2.0], -1.0) == (F32(0.0), 0)
    # the own depth alone goes through (float)(1 / (1 / z)): two float64 roundings, far inside half a float32 step
    for z in (3.0, 0.1, 1.0000001, 1e-30, 3e38, 7.7):
        assert fuse_pixel(z, [inf], 0.01) == (F32(z), 1)


def test_support_saturates_at_nothing():
    assert SD.MAX_FUSE == 16
    assert fuse_pixel(2.0, [2.0] * 16, 0.0) == (F32(2.0), 17)
    assert fuse_pixel(2.0, [2.0] * 16, 0.0, min_support=17) == (F32(2.0), 17)
    assert fuse_pixel(2.0, [2.0] * 16, 0.0, min_support=18) == (F32(0.0), 0)
    with pytest.raises(ValueError):
        SD.fuse(*FC.pixel_case(2.0, [2.0] * 17, 0.0), backend="host")
    with pytest.raises(ValueError):
        SD.fuse(*FC.pixel_case(2.0, [2.0], 0.0), min_support=0, backend="host")


def test_return_support_changes_nothing():
    c = FC.random_case(5, 9, 11, 3, 77)
    warped = host_warp(c, 1, 4)
    plain = SD.fuse(c["depth"], warped, c["tol"], 2, 1, backend="host")
    assert FC.same_bits(plain.numpy(), host_fuse(c, warped, 2, 1)[0])


def test_two_source_pixels_on_one_target_pixel_keep_the_nearer():
    # column 0 at depth 2 lands at u = 0.25 with depth 4, column 1 at depth 1 at u = 0.5 with depth 3: both on column 0
    c = FC.two_views([2.0, 1.0, 0.0, 0.0], (0.0, 0.0, 2.0))
    warped = host_warp(c, 0, 1)
    assert FC.same_bits(warped, FC.brute_warp(c["depth"], c["K"], c["fsrc"], c["into"], 0, 1))
    assert warped[0, 0, 0, 0] == F32(3.0) and np.isinf(warped[0, 0, 0, 1:]).all()
    swapped = FC.two_views([1.0, 2.0, 0.0, 0.0], (0.0, 0.0, 2.0))      # u = 1 / 6 at depth 3 and u = 0.75 at depth 4
    assert host_warp(swapped, 0, 1)[0, 0, 0, 0] == F32(3.0)


def test_u_equal_to_the_width_is_rejected():
    # z = 2 and a shift of 1: column j lands at u = j + 1 exactly, the last one at u == width
    c = FC.two_views([2.0] * 5, (1.0, 0.0, 0.0))
    warped = host_warp(c, 0, 1)
    assert FC.same_bits(warped, FC.brute_warp(c["depth"], c["K"], c["fsrc"], c["into"], 0, 1))
    assert np.isinf(warped[0, 0, 0, 0]) and (warped[0, 0, 0, 1:] == F32(2.0)).all()


def test_a_point_behind_the_target_camera_is_rejected():
    c = FC.two_views([2.0] * 5, (0.0, 0.0, -5.0))
    warped = host_warp(c, 0, 1)
    assert FC.same_bits(warped, FC.brute_warp(c["depth"], c["K"], c["fsrc"], c["into"], 0, 1)) and np.isinf(warped).all()
    on_the_plane = FC.two_views([2.0] * 5, (0.0, 0.0, -2.0))           # c2 == 0
    assert np.isinf(host_warp(on_the_plane, 0, 1)).all()


def test_crowded_pixels():
    c = FC.crowded_case(3, 9, 11, 3)
    warped = host_warp(c, 0, 3)
    assert FC.same_bits(warped, FC.brute_warp(c["depth"], c["K"], c["fsrc"], c["into"], 0, 3))
    landed = np.isfinite(warped).sum()
    assert 0 < landed < 0.2 * (c["fsrc"] >= 0).sum() * 9 * 11           # many source pixels on few target pixels


def test_arguments_are_checked():
    c = FC.random_case(3, 5, 7, 3, 5)
    for v0, nv in ((-1, 1), (0, 4), (3, 1), (4, 0)):
        with pytest.raises(ValueError):
            host_warp(c, v0, nv)
    with pytest.raises(ValueError):
        SD.fuse(c["depth"], host_warp(c, 0, 2), c["tol"], 1, 2, backend="host")     # two targets from v0 = 2 on
    with pytest.raises(ValueError):
        SD.warp(c["depth"].astype(np.float64), c["K"], c["fsrc"], c["into"], backend="host")
    with pytest.raises(ValueError):
        SD.plan_fusion(SS.emap_cameras_of(SS.arc_cameras(3, 12, 16)), fuse_sources=17)


# ------------------------------------------------------------------------------------------------ the Python layer
def test_plan_fusion():
    cams = SS.emap_cameras_of(SS.arc_cameras(5, 12, 16))
    K, fsrc, into, tol = SD.plan_fusion(cams, hypotheses=8, fuse_sources=3)
    plan = SD.plan_views(cams, hypotheses=8, sources=3)
    assert fsrc.dtype == np.int32 and (fsrc == plan.src).all()          # chosen as plan_views chooses
    assert (K == plan.K).all() and (tol == plan.tol).all() and into.shape == (5, 3, 12)
    wide = SD.plan_fusion(cams, hypotheses=8, fuse_sources=7)[1]
    assert (wide[:, :4] >= 0).all() and (wide[:, 4:] == -1).all()
    # into takes the SOURCE's camera coordinates to the TARGET's: the other direction than rel
    X = np.array([0.4, 0.6, 0.5])
    w = int(fsrc[0, 0])
    M = into[0, 0].reshape(3, 4)
    assert np.allclose(M[:, :3] @ (cams[w].R @ X + cams[w].T) + M[:, 3], cams[0].R @ X + cams[0].T, atol=1e-12)
    assert (into[0, 0] == SD.relative_pose(cams[w].R, cams[w].T, cams[0].R, cams[0].T)).all()
    # a narrow angle leaves no source, and the plan is still made
    assert (SD.plan_fusion(cams, hypotheses=8, fuse_sources=3, max_angle_deg=1.0)[1] == -1).all()


@functools.lru_cache(maxsize=None)
def small_scan():
    scan = SS.solid_scan("box", 5, 24, 32, backend="host", synth_cameras=SS.arc_cameras(5, 24, 32))
    kw = dict(hypotheses=12, patch_radius=1, sources=2)
    return scan, SD.stereo_depth(list(SS.photographs(scan)), scan.cameras, backend="host", **kw), kw


def test_stereo_depth_with_fuse_is_fuse_depth_of_its_maps():
    scan, maps, kw = small_scan()
    fused, info = SD.stereo_depth(list(SS.photographs(scan)), scan.cameras, backend="host", return_info=True, fuse=True,
                                  fuse_sources=3, min_support=2, **kw)
    again, finfo = SD.fuse_depth(maps, scan.cameras, hypotheses=12, fuse_sources=3, min_support=2, backend="host",
                                 return_info=True)
    plain_info = SD.stereo_depth(list(SS.photographs(scan)), scan.cameras, backend="host", return_info=True, **kw)[1]
    assert all(FC.same_bits(a, b) for a, b in zip(fused, again)) and info["fusion"] == finfo
    assert info["recommended_slack"] == plain_info["recommended_slack"] and "fusion" not in plain_info
    assert finfo["coverage_before"] == plain_info["coverage"] and info["coverage"] == finfo["coverage"]
    assert finfo["coverage"] == [float((m > 0).mean()) for m in fused]
    assert len(finfo["support_histogram"]) == 5 and sum(finfo["support_histogram"]) == 5 * 24 * 32
    assert sum(finfo["support_histogram"][2:]) == sum(int((m > 0).sum()) for m in fused) and finfo["support_histogram"][1] == 0
    assert finfo["filled"] == sum(int(((a == 0) & (b > 0)).sum()) for a, b in zip(maps, fused)) > 0
    assert finfo["dropped"] == sum(int(((a > 0) & (b == 0)).sum()) for a, b in zip(maps, fused))


@pytest.mark.parametrize("targets", [1, 2, 5])
def test_chunking_changes_nothing(targets, monkeypatch):
    scan, maps, _ = small_scan()
    kw = dict(hypotheses=12, fuse_sources=3, min_support=2, backend="host", return_info=True)
    whole, info = SD.fuse_depth(maps, scan.cameras, **kw)
    calls = []
    real = SD.warp
    monkeypatch.setattr(SD, "warp", lambda *a, **k: calls.append(a[5]) or real(*a, **k))
    monkeypatch.setattr(SD, "FUSE_CHUNK_BYTES", targets * 3 * 24 * 32 * 4)
    parts, info_p = SD.fuse_depth(maps, scan.cameras, **kw)
    assert calls == [targets] * (5 // targets) + ([5 % targets] if 5 % targets else [])
    assert all(FC.same_bits(a, b) for a, b in zip(whole, parts)) and info == info_p


def test_mixed_sizes_and_foreign_maps():
    small = SS.solid_scan("box", 3, 12, 16, backend="host", synth_cameras=SS.arc_cameras(3, 12, 16))
    large = SS.solid_scan("box", 1, 16, 12, backend="host", synth_cameras=SS.arc_cameras(1, 16, 12))
    cams = [small.cameras[0], large.cameras[0], small.cameras[1], small.cameras[2]]
    mesh = lambda d: np.where(np.isfinite(d), d, 0.0)                   # the caller's own maps, float64 here
    maps = [mesh(small.depth[0]).astype(np.float64), mesh(large.depth[0]), mesh(small.depth[1]), mesh(small.depth[2])]
    fused = SD.fuse_depth(maps, cams, hypotheses=8, fuse_sources=2, min_support=2, backend="host")
    assert [m.shape for m in fused] == [(12, 16), (16, 12), (12, 16), (12, 16)] and all(m.dtype == np.float32 for m in fused)
    assert not fused[1].any() and all(fused[k].any() for k in (0, 2, 3))     # a lone view of its size has no source
    alone = SD.fuse_depth([maps[0], maps[2], maps[3]], small.cameras, hypotheses=8, fuse_sources=2, min_support=2, backend="host")
    assert all(FC.same_bits(a, b) for a, b in zip(alone, [fused[0], fused[2], fused[3]]))
    with pytest.raises(ValueError):
        SD.fuse_depth(maps[:3], cams, backend="host")
    with pytest.raises(ValueError):
        SD.fuse_depth([m.astype(np.int32) for m in maps], cams, backend="host")


# ------------------------------------------------------------------------------------------------ the purpose
def gate_pairs(scan, planes, slack):
    """(seen, hidden) bool [V,P] of the ground-truth samples under depth planes (already widened).  A copy of
    test_stereo_depth_cpu.py's helper."""
    from curve_gaussian_amd.edge_extraction.abc import pred_points_and_directions
    from curve_gaussian_amd.ops.view_chunks import camera_arrays
    K, M = camera_arrays(scan.cameras)
    M = np.asarray(M, np.float64).reshape(len(K), 12)
    pts = np.ascontiguousarray(pred_points_and_directions(scan.edges, SS.SAMPLE_RESOLUTION).points, np.float32).reshape(-1, 3)
    rows = [EO.gate_view_host(pts, K[v], M[v], planes[v], slack) for v in range(len(K))]
    return np.stack([r[2] | r[3] for r in rows]), np.stack([r[3] for r in rows])


def test_fusion_covers_and_hides_more_without_hiding_what_the_raw_sweep_does_not():
    """The purpose: the box arc of test_stereo_depth_cpu.py (8 views, 48 x 64, D = 32, R = 2, S = 2), one sweep, its
    filtered maps, the fused ones (the defaults: 7 sources, support >= 3) and the unfiltered sweep, each under the gate
    at the maps' recommended slack, against the mesh gate.  Figures of this rule (profiles/stereo_fuse.md): covered mesh
    pixels 4386 of 5724 unfused (76.6 %) and 5006 fused (87.5 %); of the 23341 pairs the mesh gate hides, hidden by both
    13336 -> 14096 (15812 by the unfiltered sweep); pairs the mesh gate sees that are hidden: 0 unfused, 0 fused, 125 by
    the unfiltered sweep."""
    scan = SS.solid_scan("box", 8, 48, 64, backend="host", synth_cameras=SS.arc_cameras(8, 48, 64))
    photos = SS.photographs(scan)
    plan = SD.plan_views(scan.cameras, hypotheses=32, sources=2)
    assert plan.usable.all()
    raw = SD.sweep(photos, plan.K, plan.inv, plan.src, plan.rel, 2, backend="host")
    filtered = SD.consistency(raw, plan.K, plan.src, plan.rel, plan.tol, backend="host").numpy()
    raw = raw.numpy()
    slack = 2.0 * max(float(plan.z_far[v] ** 2 * abs(plan.inv[v][1] - plan.inv[v][0])) for v in range(8))
    fused, info = SD.fuse_depth(list(filtered), scan.cameras, hypotheses=32, backend="host", return_info=True)
    mesh = np.isfinite(scan.depth)
    covered = {name: int(((np.stack(m) > 0) & mesh).sum()) for name, m in (("unfused", filtered), ("fused", fused), ("raw", raw))}
    seen, hid_m = gate_pairs(scan, EO.depth_window_max(scan.depth, EO.DEPTH_WINDOW, backend="host").numpy(), EO.DEPTH_SLACK)
    both, false = {}, {}
    for name, maps in (("unfused", filtered), ("fused", fused), ("raw", raw)):
        planes = EO.depth_window_max(np.stack(EO.check_depth_maps(scan.cameras, list(maps))), EO.DEPTH_WINDOW, backend="host").numpy()
        _, hid = gate_pairs(scan, planes, slack)
        both[name], false[name] = int((hid & hid_m).sum()), int((hid & seen & ~hid_m).sum())
    print("mesh pixels %d, covered %s; mesh gate hides %d pairs; hidden by both %s; hidden though the mesh gate sees them %s; "
          "recommended_slack %.4f" % (mesh.sum(), json.dumps(covered), hid_m.sum(), json.dumps(both), json.dumps(false), slack))
    print("fusion:", json.dumps(info))
    assert covered["fused"] > covered["unfused"]
    assert both["fused"] > both["unfused"]
    assert false["fused"] <= false["raw"]


# ------------------------------------------------------------------------------------------------ the tool
def _files(root):
    return {os.path.relpath(os.path.join(d, f), root): open(os.path.join(d, f), "rb").read()
            for d, _, fs in os.walk(root) for f in fs}


def test_tool(tmp_path):
    from curve_gaussian_amd import stereo_depth as TOOL
    from curve_gaussian_amd.edge_extraction import reprojection as RP
    scan_dir = str(tmp_path / "box")
    assert SS.main(["box", scan_dir, "--views", "4", "--height", "24", "--width", "32", "--backend", "host", "--photos",
                    "--arc"]) == 0
    args = ["--scan", scan_dir, "--backend", "host", "--hypotheses", "12", "--patch_radius", "1", "--sources", "2"]
    # without the new flags: the folder and the keys the existing tool test expects, nothing of the fusion
    assert TOOL.main(args) == 0
    plain_dir = os.path.join(scan_dir, "depth_stereo")
    plain = _files(plain_dir)
    assert sorted(plain) == [f"{i}_colors.npy" for i in range(4)] + ["stereo.json"]
    report = json.loads(plain["stereo.json"])
    assert sorted(report) == sorted(["method", "backend", "detector", "z_floor", "bounds", "hypotheses", "patch_radius", "sources",
                                     "max_angle_deg", "min_var", "max_cost", "min_sources", "consistency_steps", "min_consistent",
                                     "views", "depth_step_max", "recommended_slack", "note"])
    assert report["method"] == "plane_sweep" and all(sorted(v) == ["coverage", "name", "swept"] for v in report["views"])
    cams, _ = RP.emap_cameras(scan_dir, "PidiNet")
    from PIL import Image
    photos = [SD.luminance(np.array(Image.open(os.path.join(scan_dir, "color", f"{i}_colors.png")))) for i in range(4)]
    maps = SD.stereo_depth(photos, cams, hypotheses=12, patch_radius=1, sources=2, backend="host")
    assert all(np.load(os.path.join(plain_dir, f"{i}_colors.npy")).tobytes() == maps[i].tobytes() for i in range(4))
    # --fuse
    assert TOOL.main(args + ["--fuse", "--fuse_sources", "3", "--fuse_support", "2"]) == 0
    fused_dir = os.path.join(scan_dir, "depth_stereo_fused")
    assert sorted(os.listdir(fused_dir)) == [f"{i}_colors.npy" for i in range(4)] + ["stereo.json"]
    assert _files(plain_dir) == plain                                   # the unfused folder is left alone
    fused_report = json.load(open(os.path.join(fused_dir, "stereo.json")))
    assert fused_report["fused"] is True and fused_report["fuse_sources"] == 3 and fused_report["fuse_support"] == 2
    assert sorted(fused_report["fusion"]) == ["coverage", "coverage_before", "dropped", "filled", "support_histogram"]
    assert {k: v for k, v in fused_report.items() if k not in ("fused", "fuse_sources", "fuse_support", "fusion", "views")} == \
        {k: v for k, v in report.items() if k != "views"}
    assert fused_report["fusion"]["coverage_before"] == [v["coverage"] for v in report["views"]]
    assert [v["coverage"] for v in fused_report["views"]] == fused_report["fusion"]["coverage"]
    want = SD.fuse_depth(maps, cams, hypotheses=12, fuse_sources=3, min_support=2, backend="host")
    stored = RP.scan_depth_maps(fused_dir, cams)
    assert all(FC.same_bits(a, b) for a, b in zip(stored, want)) and fused_report["fusion"]["filled"] > 0
    checked = EO.check_depth_maps(cams, stored)                         # what --depth_dir depth_stereo_fused reads
    assert all(m.dtype == np.float32 and m.shape == (24, 32) and (m > 0).all() for m in checked)
    with pytest.raises(FileExistsError):
        TOOL.main(args + ["--fuse"])
    # --fuse_from: the caller's own maps, no sweep
    other = str(tmp_path / "from")
    assert TOOL.main(["--scan", scan_dir, "--backend", "host", "--hypotheses", "12", "--fuse_from", "depth_stereo", "--out", other,
                      "--fuse_sources", "3", "--fuse_support", "2"]) == 0
    assert all(FC.same_bits(np.load(os.path.join(other, f"{i}_colors.npy")), want[i]) for i in range(4))
    from_report = json.load(open(os.path.join(other, "stereo.json")))
    assert from_report["fused"] is True and from_report["fuse_from"] == "depth_stereo" and from_report["fusion"] == fused_report["fusion"]
    assert TOOL.main(["--scan", scan_dir, "--backend", "host", "--hypotheses", "12", "--fuse_from", plain_dir, "--out", other,
                      "--overwrite"]) == 0                               # an absolute folder, the default parameters
    assert json.load(open(os.path.join(other, "stereo.json")))["fuse_sources"] == SD.FUSE_SOURCES
    with pytest.raises(FileNotFoundError):
        TOOL.main(["--scan", scan_dir, "--backend", "host", "--fuse_from", "nowhere", "--out", str(tmp_path / "never")])


# ------------------------------------------------------------------------------------------------ the ABI
def test_signatures_and_header():
    i, vp = ctypes.c_int, ctypes.c_void_p
    assert _lib.SIGNATURES["cgs_stereo_warp"] == (i, [i, i, i, vp, vp, i, vp, vp, i, i, vp, vp])
    assert _lib.SIGNATURES["cgs_stereo_fuse"] == (i, [i, i, i, vp, i, vp, vp, i, i, i, vp, vp, vp])
    header = open(os.path.join(ROOT, "include", "curvegs.h")).read()
    assert int(re.search(r"#define CGS_STEREO_MAX_FUSE (\d+)", header).group(1)) == _lib.STEREO_MAX_FUSE == SD.MAX_FUSE
    lib = _lib.load()
    assert hasattr(lib, "cgs_stereo_warp") and hasattr(lib, "cgs_stereo_fuse")


def test_entries_reject_before_any_launch():
    """Argument lists that must not pass validation (dummy pointers, never dereferenced)."""
    lib, A, B, C, D = _lib.load(), ctypes.c_void_p(1 << 20), ctypes.c_void_p(2 << 20), ctypes.c_void_p(3 << 20), ctypes.c_void_p(4 << 20)
    inside = lambda p, n: ctypes.c_void_p(p.value + n)
    # (V, height, width, depth, intr, F, fsrc, into, v0, nv, warped, stream): depth is 3 * 8 * 8 * 4 = 768 bytes at A
    good = [3, 8, 8, A, D, 2, D, D, 1, 2, B, None]
    for pos, bad in ((0, -1), (1, 0), (2, _lib.EDT_MAX_SIZE + 1), (3, None), (4, None), (5, 0), (5, 17), (6, None), (7, None),
                     (8, -1), (8, 2), (8, 4), (9, -1), (9, 3), (10, None), (10, A), (10, inside(A, 764))):
        args = list(good)
        args[pos] = bad
        assert lib.cgs_stereo_warp(*args) == -1, (pos, bad)
        assert _lib.last_error().startswith("cgs_stereo_warp: invalid argument"), (pos, bad)
    assert "overlap" in _lib.last_error()
    args = list(good)
    args[3] = inside(B, 2 * 2 * 256 - 4)                                # depth begins in warped's last word
    assert lib.cgs_stereo_warp(*args) == -1 and "overlap" in _lib.last_error()
    # (V, height, width, depth, F, warped, tol, min_support, v0, nv, out, support, stream)
    good = [3, 8, 8, A, 2, B, D, 1, 1, 2, C, None, None]
    for pos, bad in ((0, -1), (1, 0), (2, 0), (3, None), (4, 0), (4, 17), (5, None), (6, None), (7, 0), (7, -2), (8, -1), (8, 2),
                     (9, -1), (9, 3), (10, None), (10, inside(A, 700)), (10, inside(B, 1020)), (11, inside(A, 767)),
                     (11, inside(B, 0)), (11, inside(C, 511))):
        args = list(good)
        args[pos] = bad
        assert lib.cgs_stereo_fuse(*args) == -1, (pos, bad)
        assert _lib.last_error().startswith("cgs_stereo_fuse: invalid argument"), (pos, bad)
    assert "overlap" in _lib.last_error()
    # with V = 0 the one range is (0, 0); every argument is still checked
    assert lib.cgs_stereo_warp(0, 8, 8, A, D, 2, D, D, 0, 1, B, None) == -1
    assert lib.cgs_stereo_warp(0, 8, 8, A, D, 0, D, D, 0, 0, B, None) == -1
    assert lib.cgs_stereo_fuse(0, 8, 8, A, 2, B, D, 0, 0, 0, C, None, None) == -1
    assert lib.cgs_stereo_warp(0, 8, 8, A, D, 2, D, D, 0, 0, B, None) == 0 and lib.cgs_stereo_warp(3, 8, 8, A, D, 2, D, D, 3, 0, B, None) == 0
    assert lib.cgs_stereo_fuse(3, 8, 8, A, 2, B, D, 1, 2, 0, C, C, None) == 0        # nv = 0: a no-op, nothing is launched
