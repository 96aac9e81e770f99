"""Host: rejoining cut edges at their junctions (ops.edge_join: end_attach, attachments, join_components, join_vertices,
move_ends, join_edges) on the numpy back end -- the chunked attachment against the all-pairs definition, every comparison
of the rule on its bound, the host rules on hand-written inputs, the drawn fixtures whose result is known, the command
line, the export, the driver's options and the C ABI's argument checks."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import edge_dedupe_cases as C
import edge_join_cases as J
import edge_score_cases as EC
from curve_gaussian_amd.ops import edge_join as EJ


def _host(pts, off, tol, reach):
    got = EJ.end_attach(pts, off, tol, reach, backend="host")
    assert got.dtype == torch.int64 and tuple(got.shape) == (2 * (len(off) - 1),) and not got.is_cuda
    return got.numpy()


# ------------------------------------------------------------------------------------------------ the attachment
@pytest.mark.parametrize("P,E", J.SHAPES)
def test_the_chunked_attachment_is_the_definition(P, E):
    pts, off = J.grid_case(P, E)
    assert len(pts) == P and len(off) == E + 1
    for tol, reach in ((J.GRID_TOL, J.GRID_REACH), (J.GRID_TOL, 2 * float(J.GRID)), (J.GRID_TOL, 0.0)):
        got = _host(pts, off, tol, reach)
        assert np.array_equal(got, J.attach_brute(pts, off, tol, reach)), (tol, reach)
        n = np.diff(off.astype(np.int64))
        assert (got[np.repeat(n == 0, 2)] == J.NO_ATTACH).all(), "an edge without samples has no end"
    if P >= 255 and E >= 2:
        assert (_host(pts, off, J.GRID_TOL, J.GRID_REACH) != J.NO_ATTACH).any()


def test_the_host_chunks_do_not_show():
    pts, off = J.grid_case(257, 129)
    want = J.attach_brute(pts, off, J.GRID_TOL, J.GRID_REACH)
    tol2, reach2 = EJ._squares(J.GRID_TOL, J.GRID_REACH)
    for chunk in (1, 7, 64, 1000):
        assert np.array_equal(EJ._attach_host(pts, off, tol2, reach2, chunk).view(np.int64), want)


@pytest.mark.parametrize("name", [row[0] for row in J.PLACED])
def test_every_comparison_on_its_bound(name):
    """NEAR, ENDS and the two sides of TUBE with equality, each next to the input one float32 below that fails; s == 0; a
    tie; the end's own edge; a one-sample edge; reach below the tolerance and no reach."""
    pts, off, tol, reach, key = J.placed_case(name)
    want = J.attach_brute(pts, off, tol, reach)
    assert want[1] == key, "the definition gives the hand-computed key"
    assert np.array_equal(_host(pts, off, tol, reach), want)


def test_coincident_points_and_the_splits():
    pts, off, want = J.coincident_case()
    assert np.array_equal(J.attach_brute(pts, off, J.GRID_TOL, J.GRID_REACH), want)
    assert np.array_equal(_host(pts, off, J.GRID_TOL, J.GRID_REACH), want)
    for swap in (False, True):
        pts, off, key = J.split_case(swap)
        got = _host(pts, off, J.GRID_TOL, J.GRID_REACH)
        assert got[1] == key and np.array_equal(got, J.attach_brute(pts, off, J.GRID_TOL, J.GRID_REACH))


def test_argument_errors():
    pts = np.zeros((4, 3), np.float32)
    call = lambda pts=pts, off=(0, 2, 4), tol=0.1, reach=0.4, **kw: EJ.end_attach(pts, off, tol, reach, **{"backend": "host", **kw})
    assert call().tolist() == [2, 2, 0, 0]
    with pytest.raises(ValueError, match="float32"):
        call(pts=pts.astype(np.float64))
    with pytest.raises(ValueError, match=r"\[P,3\]"):
        call(pts=np.zeros((4, 2), np.float32))
    for bad in (np.nan, np.inf, -np.inf):
        with pytest.raises(ValueError, match="finite"):
            call(pts=np.array([[0, 0, 0], [0, bad, 0], [0, 0, 0], [0, 0, 0]], np.float32))
    with pytest.raises(ValueError, match="offsets"):
        call(off=(0, 2, 5))
    with pytest.raises(ValueError, match="offsets"):
        call(off=(0.0, 2.0, 4.0))
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="tolerance"):
            call(tol=bad)
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="reach"):
            call(reach=bad)
    with pytest.raises(ValueError, match="backend"):
        call(backend="cuda")
    with pytest.raises(ValueError, match="keys"):
        EJ.attachments(np.zeros(3, np.int64), [0, 2, 4], 1)
    with pytest.raises(ValueError, match="keys"):
        EJ.attachments(np.zeros(4, np.int32), [0, 2, 4], 1)
    with pytest.raises(ValueError, match="does not exist"):
        EJ.attachments(np.array([4, -1, -1, -1], np.int64), [0, 2, 4], 1)
    with pytest.raises(ValueError, match="zone"):
        EJ.attachments(np.full(4, -1, np.int64), [0, 2, 4], -1)
    for kw in (dict(tolerance=0.0), dict(reach=-1.0), dict(zone=-1), dict(backend="cuda")):
        with pytest.raises(ValueError, match=next(iter(kw))):
            EJ.join_edges(EC.SCAN_EDGES, resolution=EC.SCAN_RESOLUTION, **{"backend": "host", **kw})
    if not torch.cuda.is_available():
        from curve_gaussian_amd import _lib
        with pytest.raises(_lib.CurveGSError, match="GPU"):
            call(backend="gpu")
        with pytest.raises(_lib.CurveGSError, match="GPU tensor"):
            call(pts=torch.from_numpy(pts), backend="gpu")


# ------------------------------------------------------------------------------------------------ host rules
def _keys(pairs, E):
    """int64 [2E] keys: {end: sample}, at a squared distance of 2^-12."""
    keys = np.full(2 * E, J.NO_ATTACH, np.int64)
    for end, j in pairs.items():
        keys[end] = J.key_of(1, j)
    return keys


def test_classification_at_the_edge_of_the_zone():
    """zone = 2.  On an edge of 10 samples k = 2 is still the first end and k = 3 a T, k = 7 the last end and k = 6 a T.
    On an edge of 4 samples (shorter than 2 zone) both zones cover everything: the nearer end wins and the tie of an edge
    of 5 samples at k = 2 goes to the first."""
    off = np.array([0, 1, 11, 15, 20])          # edge 0: the one sample whose ends ask; edges 1, 2, 3: 10, 4 and 5 samples
    for k, kind, target in ((0, 1, 2), (2, 1, 2), (3, 2, -1), (6, 2, -1), (7, 1, 3), (9, 1, 3)):
        a = EJ.attachments(_keys({0: 1 + k}, 4), off, 2)
        assert (a["sample"][0], a["edge"][0], a["local"][0], a["kind"][0], a["target"][0]) == (1 + k, 1, k, kind, target), k
        assert a["kind"][1:].tolist() == [0] * 7 and a["target"][1:].tolist() == [-1] * 7
        assert np.isnan(a["parameter"][0]) == (kind != 2) and (kind != 2 or a["parameter"][0] == k / 9)
        assert a["distance"][0] == 2.0 ** -6 and np.isnan(a["distance"][1])
    for k, target in ((0, 4), (1, 4), (2, 5), (3, 5)):
        a = EJ.attachments(_keys({0: 11 + k}, 4), off, 2)
        assert (a["edge"][0], a["local"][0], a["kind"][0], a["target"][0]) == (2, k, 1, target), k
    for k, target in ((1, 6), (2, 6), (3, 7)):
        a = EJ.attachments(_keys({0: 15 + k}, 4), off, 2)
        assert (a["edge"][0], a["local"][0], a["kind"][0], a["target"][0]) == (3, k, 1, target), k
    a = EJ.attachments(_keys({0: 4}, 4), off, 0)
    assert a["kind"][0] == 2, "zone 0: only the end samples themselves are ends"
    # an edge without samples between two others is stepped over
    a = EJ.attachments(_keys({0: 5}, 4), np.array([0, 5, 5, 5, 9]), 1)
    assert (a["edge"][0], a["local"][0], a["target"][0]) == (3, 0, 6)
    assert torch.is_tensor(EJ.end_attach(np.zeros((0, 3), np.float32), [0, 0], 1.0, 1.0, backend="host"))


def test_components():
    """Five edges of 10 samples.  End 1 attaches to end 2, end 3 to end 4 and end 5 onto the interior of edge 4 (a T): 1-2
    and 3-4 are components labelled by their least end, 5 is its own; where A attaches to B and B elsewhere -- 6 to 9, 9 to
    0 -- all three are one component.  An edge without samples has no label."""
    off = np.array([0, 10, 20, 30, 40, 50, 50])
    keys = _keys({1: 10, 3: 20, 5: 45, 6: 49, 9: 0}, 6)
    a = EJ.attachments(keys, off, 2)
    assert a["kind"].tolist() == [0, 1, 0, 1, 0, 2, 1, 0, 0, 1, 0, 0] and a["target"][[1, 3, 6, 9]].tolist() == [2, 4, 9, 0]
    labels = EJ.join_components(a, off)
    assert labels.tolist() == [0, 1, 1, 3, 3, 5, 0, 7, 8, 0, -1, -1]


def _fan_result(angles, gap, **kw):
    return EJ.join_edges(J.fan(angles, gap), resolution=0.01, backend="host", **{"tolerance": 0.02, "reach": 0.08, **kw})


def test_the_vertex_rules_in_their_order():
    centre = np.array([0.3, 0.2, 0.1])
    # least squares: two lines at 90 degrees that stop 3 and 4 samples short of their crossing meet IN it, not between
    # their ends; the bound is the 1e-5 of the shortened scan (same resolution scale, shorter lever)
    r = _fan_result([0, 90], [0.03, 0.04])
    assert r["rules"] == ["equal", "lsq", "equal"] and r["edge_vertices"].tolist() == [[0, 1], [2, 1]]
    assert np.linalg.norm(r["vertices"][1] - centre) < 1e-5
    assert np.allclose(r["moved"], [0, 0.03, 0, 0.04], atol=1e-5) and r["collapsed"] == [] and r["t_junctions"] == []
    lines = J.edge_arrays(r["edge_dict"])[1]
    given = J.edge_arrays(J.fan([0, 90], [0.03, 0.04]))[1]
    assert np.array_equal(lines[:, 0], given[:, 0]) and np.array_equal(lines[:, 1], r["vertices"][[1, 1]])
    # parallel members (10 degrees apart: the least eigenvalue is 1 - cos 10 deg < 0.1): the mean
    r = _fan_result([0, 10], 0.03)
    ends = J.edge_arrays(J.fan([0, 10], 0.03))[1][:, 1]
    assert r["rules"] == ["equal", "mean", "equal"] and np.array_equal(r["vertices"][1], ends.mean(0))
    # a least-squares point beyond reach: at 30 degrees the ends are 0.031 apart and both 0.06 from the crossing, so a
    # reach of 0.05 attaches them (ENDS) and refuses the crossing
    r = _fan_result([0, 30], 0.06, reach=0.05)
    ends = J.edge_arrays(J.fan([0, 30], 0.06))[1][:, 1]
    assert r["rules"] == ["equal", "mean", "equal"] and np.array_equal(r["vertices"][1], ends.mean(0))
    assert _fan_result([0, 30], 0.06)["rules"] == ["equal", "lsq", "equal"], "within reach it is taken"
    # bitwise equal before least squares: two lines that share their end point keep it, unchanged
    r = _fan_result([0, 90], 0.0)
    assert r["rules"] == ["equal"] * 3 and np.array_equal(r["vertices"][1], centre) and (r["moved"] == 0).all()
    # a T before everything: a third line passes through the crossing; the ends that stop short of it land on ITS sample
    fan = J.fan([0, 90], 0.01)
    fan["lines_end_pts"].append([0.3, 0.2, -0.1, 0.3, 0.2, 0.3])
    r = EJ.join_edges(fan, resolution=0.01, tolerance=0.02, reach=0.08, backend="host")
    assert [t["host"] for t in r["t_junctions"]] == [2, 2] and [t["end"] for t in r["t_junctions"]] == [1, 3]
    assert all(not t["host_moved"] and 0 < t["parameter"] < 1 for t in r["t_junctions"])
    pts = J.SP.sample_edges([], fan["lines_end_pts"], 0.01)[0]
    for t in r["t_junctions"]:
        assert np.array_equal(r["vertices"][t["vertex"]], pts[r["offsets"][2] + t["sample"]].astype(np.float64))
        assert r["rules"][t["vertex"]] == "t"
    assert np.array_equal(J.edge_arrays(r["edge_dict"])[1][2], J.edge_arrays(fan)[1][2]), "the host is not changed"


def test_no_end_moves_further_than_the_reach():
    """Three edges of two samples along x whose last ends, at x = x0, x1, x2, form one component (a chain: end 1 attached
    to end 3 and end 3 to end 5); the tangents are parallel, so the vertex is the mean.  At 0, 0.07 and 0.14 the mean lies
    0.07 from the outer ends, within a reach of 0.08, and nobody is released.  At 0, 0.075 and 0.16 it lies 0.0817 from
    end 5: that end is released and becomes a vertex of its own, unmoved, and the other two meet at their mean."""
    off = np.array([0, 2, 4, 6])
    attach = EJ.attachments(_keys({1: 3, 3: 5}, 3), off, 0)
    labels = EJ.join_components(attach, off)
    assert labels.tolist() == [0, 1, 2, 1, 4, 1]
    for xs, released, ids in (((0.0, 0.07, 0.14), [], [0, 1, 2, 1, 3, 1]), ((0.0, 0.075, 0.16), [5], [0, 1, 2, 1, 3, 4])):
        ends = np.array([[x + d, 0.0, 0.0] for x in xs for d in (-0.01, 0.0)])
        got = EJ.join_vertices(attach, labels, ends.astype(np.float32), off, ends, 0.08)
        assert got["released"] == released and got["vertex_of_end"].tolist() == ids
        moved = np.linalg.norm(got["vertices"][got["vertex_of_end"]] - ends, axis=1)
        assert (moved <= 0.08).all() and got["rule"][1] == "mean"
        kept = [x for k, x in enumerate(xs) if 2 * k + 1 not in released]
        assert got["vertices"][1].tolist() == [np.mean(kept), 0.0, 0.0]
        for end in released:
            assert np.array_equal(got["vertices"][got["vertex_of_end"][end]], ends[end]) and got["rule"][got["vertex_of_end"][end]] == "equal"


def test_an_edge_without_a_moved_end_comes_back_bit_for_bit_and_a_collapsed_edge_is_reported():
    given = J.fan([0, 90, 200], [0.03, 0.04, 0.5])
    r = EJ.join_edges(given, resolution=0.01, tolerance=0.02, reach=0.08, backend="host")
    assert np.array_equal(J.edge_arrays(r["edge_dict"])[1][2], J.edge_arrays(given)[1][2]) and (r["moved"][4:] == 0).all()
    # a line of 6 samples whose two ends both see the end of a long line beside its middle
    short = {"curves_ctl_pts": [], "lines_end_pts": [[0.0, 0.0, 0.0, 0.065, 0.0, 0.0], [0.0325, 0.5, 0.0, 0.0325, 0.04, 0.0]]}
    r = EJ.join_edges(short, resolution=0.01, tolerance=0.06, reach=0.08, zone=0, backend="host")
    assert r["attach"]["kind"].tolist() == [1, 1, 0, 2] and r["attach"]["target"][:2].tolist() == [3, 3]
    assert r["collapsed"] == [0] and r["edge_vertices"][0, 0] == r["edge_vertices"][0, 1]
    assert [(t["end"], t["host"], t["host_moved"]) for t in r["t_junctions"]] == [(3, 0, True)], "the host itself moved: reported"


def test_curves_move_only_their_end_control_points():
    g = J.shortened_scan(3)
    r = J.join_scan(g)
    curves, lines = J.edge_arrays(r["edge_dict"])
    given_c, given_l = J.edge_arrays(g)
    assert np.array_equal(curves, given_c), "the curve is free"
    moved = EJ.move_ends(given_c, given_l, np.array([0, 1, -1, -1, -1, -1, -1, -1]), np.array([[9.0, 9, 9], [8.0, 8, 8]]))
    assert np.array_equal(moved[0][0, [1, 2]], given_c[0, [1, 2]]) and moved[0][0, 0].tolist() == [9, 9, 9]
    assert moved[0][0, 3].tolist() == [8, 8, 8] and np.array_equal(moved[1], given_l) and (moved[2][2:] == 0).all()


# ------------------------------------------------------------------------------------------------ the drawn fixtures
@pytest.mark.parametrize("g", [0, 1, 3, 5, 7])
def test_the_shortened_scan_finds_its_corner(g):
    """EC.SCAN_EDGES with every edge cut by g samples at both ends, tolerance 2 and reach 8 resolutions.  For g = 1, 3, 5
    the ends of lines 0 and 1 join in one vertex within 1e-5 of the corner they shared: a float32 coordinate rounding of
    6e-8 on samples 0.004 apart is a direction error of about 2e-5 rad, over a lever of at most the reach, 0.032, about
    7e-7; the bound leaves more than 10 x on top.  Measured (host): 2.1e-8, 6.4e-8 and 2.2e-7; the mean of the two ends
    would be 2.7, 8.2 and 13.6 mm off.  The other six ends are free and their edges unchanged.  For g = 7 the ends are 9.9
    resolutions apart and nothing joins; for g = 0 the vertex is the shared point, bit for bit."""
    given = J.shortened_scan(g)
    r = J.join_scan(given)
    a, b = J.CORNER_ENDS
    ends = r["edge_vertices"].reshape(-1)
    kinds = r["attach"]["kind"]
    curves, lines = J.edge_arrays(r["edge_dict"])
    given_c, given_l = J.edge_arrays(given)
    assert np.array_equal(curves, given_c) and np.array_equal(lines[2], given_l[2]) and r["t_junctions"] == []
    assert r["collapsed"] == [] and r["released"] == []
    if g == 7:
        assert (kinds == 0).all() and len(r["vertices"]) == 8 and np.array_equal(lines, given_l) and (r["moved"] == 0).all()
        return
    assert kinds.tolist() == [0, 0, 0, 1, 1, 0, 0, 0] and r["attach"]["target"][[a, b]].tolist() == [b, a]
    assert ends[a] == ends[b] and len(r["vertices"]) == 7 and sorted(set(ends.tolist())) == list(range(7))
    vertex = r["vertices"][ends[a]]
    error = np.linalg.norm(vertex - J.CORNER)
    print(f"cut by {g} samples: the corner vertex is {error:.3g} off, the mean of the two ends would be "
          f"{np.linalg.norm((given_l[0, 1] + given_l[1, 0]) / 2 - J.CORNER):.3g}")
    assert np.array_equal(lines[0, 0], given_l[0, 0]) and np.array_equal(lines[1, 1], given_l[1, 1]), "the far ends stay"
    assert np.array_equal(lines[0, 1], vertex) and np.array_equal(lines[1, 0], vertex)
    if g == 0:
        assert vertex.tobytes() == J.CORNER.tobytes() and r["rules"][ends[a]] == "equal" and (r["moved"] == 0).all()
        assert np.array_equal(lines, given_l)
    else:
        assert error < 1e-5 and r["rules"][ends[a]] == "lsq"
        assert (r["moved"][[0, 1, 2, 5, 6, 7]] == 0).all() and (r["moved"][[a, b]] > 0.9 * g * EC.SCAN_RESOLUTION).all()


def test_the_constructed_scan_after_deduping():
    """The 7 pieces of C.constructed_dedupe(): the curve, the three drawn lines, the three leaving pieces that deduping cut
    11 or 12 samples short of their drawn line.  One end-to-end vertex, the corner of lines 0 and 1; three T-junctions, the
    first end of each leaving piece onto its own drawn line; nine free ends; the four drawn edges unchanged.  Measured
    (host, the same as the definition): the leaving pieces attach at samples 86, 95 and 100 of 152, 170 and 180, at 2.02,
    2.01 and 2.55 resolutions -- the last through the tube."""
    given = J.constructed_pieces()
    r = J.join_scan(given)
    n = np.diff(r["offsets"].astype(np.int64))
    assert n[:4].tolist() == C.DRAWN_SAMPLES and len(n) == 7
    pts = J.SP.sample_edges(given["curves_ctl_pts"], given["lines_end_pts"], EC.SCAN_RESOLUTION)[0]
    assert np.array_equal(r["keys"].numpy(), J.attach_brute(pts, r["offsets"], J.SCAN_TOLERANCE, J.SCAN_REACH))
    kinds = r["attach"]["kind"]
    assert kinds.tolist() == [0, 0, 0, 1, 1, 0, 0, 0, 2, 0, 2, 0, 2, 0] and (kinds == 0).sum() == 9
    assert r["attach"]["target"][[3, 4]].tolist() == [4, 3] and r["edge_vertices"][1, 1] == r["edge_vertices"][2, 0]
    assert np.array_equal(r["vertices"][r["edge_vertices"][1, 1]], J.CORNER) and len(r["vertices"]) == 13
    tees = r["t_junctions"]
    print("T-junctions:", [(t["edge"], t["host"], t["sample"], round(t["distance"] / EC.SCAN_RESOLUTION, 2)) for t in tees])
    assert [(t["end"], t["edge"], t["host"]) for t in tees] == [(8, 4, 1), (10, 5, 2), (12, 6, 3)]
    assert [t["sample"] for t in tees] == [86, 95, 100] and not any(t["host_moved"] for t in tees)
    assert [round(t["distance"] / EC.SCAN_RESOLUTION, 2) for t in tees] == [2.02, 2.01, 2.55]
    assert tees[2]["distance"] > J.SCAN_TOLERANCE, "through the tube: further than NEAR takes"
    for t in tees:
        assert t["parameter"] == t["sample"] / (n[t["host"]] - 1)
    curves, lines = J.edge_arrays(r["edge_dict"])
    given_c, given_l = J.edge_arrays(given)
    assert np.array_equal(curves, given_c) and np.array_equal(lines[:3], given_l[:3]), "the four drawn edges, bit for bit"
    assert np.array_equal(lines[3:, 1], given_l[3:, 1]), "a leaving piece keeps its far end"
    for t, line in zip(tees, lines[3:]):
        assert np.array_equal(line[0], pts[r["offsets"][t["host"]] + t["sample"]].astype(np.float64))
    assert r["collapsed"] == [] and r["released"] == []
    assert r["settings"] == {"resolution": EC.SCAN_RESOLUTION, "tolerance": J.SCAN_TOLERANCE, "reach": J.SCAN_REACH, "zone": 2,
                             "backend": "host", "points": int(n.sum())}


def test_the_trimmed_scan_keeps_the_invariants():
    """The 44 pieces that trimming leaves of the drawn scan, at the defaults.  Measured (host): 53 of 88 ends attach, 37 of
    them as T; one end of a chain of three is released (the rule without RELEASE would move it 10.7 resolutions).  Only
    the invariants are asserted: every displacement is at most the reach, every vertex id is in range."""
    r = EJ.join_edges(C.trimmed_scan_edges(), resolution=EC.SCAN_RESOLUTION, backend="host")
    assert r["settings"]["tolerance"] == J.SCAN_TOLERANCE and r["settings"]["reach"] == J.SCAN_REACH and r["settings"]["zone"] == 2
    print(f"88 ends: {(r['attach']['kind'] != 0).sum()} attach, {len(r['t_junctions'])} T-junctions, {len(r['vertices'])} "
          f"vertices, released {r['released']}, the furthest moves {r['moved'].max() / EC.SCAN_RESOLUTION:.2f} resolutions")
    assert len(r["moved"]) == 88 and (r["moved"] <= J.SCAN_REACH).all()
    assert r["edge_vertices"].shape == (44, 2) and r["edge_vertices"].min() >= 0 and r["edge_vertices"].max() < len(r["vertices"])
    assert sorted(set(r["edge_vertices"].reshape(-1).tolist())) == list(range(len(r["vertices"])))
    assert all(0 <= t["vertex"] < len(r["vertices"]) and 0 <= t["host"] < 44 for t in r["t_junctions"])


# ------------------------------------------------------------------------------------------------ files
def _listing(room):
    return {name: open(os.path.join(room, name), "rb").read() for name in sorted(os.listdir(room))}


def test_the_command_line_writes_its_two_files_and_no_other(tmp_path, capsys):
    from curve_gaussian_amd.edge_extraction import support as S
    base, data = EC.write_scan(tmp_path, "emap", "PidiNet")
    room = os.path.join(base, "room")
    with open(os.path.join(room, "parametric_edges.json"), "w") as f:
        json.dump(J.shortened_scan(3), f)
    argv = ["--base_dir", base, "--dataset_dir", data, "--detector", "PidiNet", "--backend", "host", "--frames_ratio", "0.5",
            "--sample_resolution", str(EC.SCAN_RESOLUTION), "--write_filtered"]
    assert S.main(argv) == 0
    before = _listing(room)
    plain_line = capsys.readouterr().out
    assert sorted(before) == sorted(["parametric_edges.json", S.SUPPORT_FILE, S.FILTERED_FILE]) and "joined" not in plain_line
    assert S.main(argv) == 0 and _listing(room) == before, "without --join a second run is the first, byte for byte"
    capsys.readouterr()
    assert S.main(argv + ["--join"]) == 0
    after = _listing(room)
    assert sorted(after) == sorted(list(before) + [S.GRAPH_FILE, S.JOINED_FILE])
    assert all(after[name] == before[name] for name in before), "every other file is byte-identical"
    want = J.join_scan(J.shortened_scan(3))
    assert json.loads(after[S.JOINED_FILE]) == want["edge_dict"]
    graph = json.loads(after[S.GRAPH_FILE])
    assert graph["scan"] == "room" and graph["input"] == "parametric_edges.json" and graph["settings"] == want["settings"]
    assert graph["vertices"] == want["vertices"].tolist() and graph["t_junctions"] == [] and graph["collapsed"] == []
    assert graph["edges"] == [{"kind": "curve", "index": 0, "vertices": [0, 1]}, {"kind": "line", "index": 0, "vertices": [2, 3]},
                              {"kind": "line", "index": 1, "vertices": [3, 4]}, {"kind": "line", "index": 2, "vertices": [5, 6]}]
    assert graph["moved"] == want["moved"].tolist() and graph["released"] == []
    assert graph["counts"] == {"edges": 4, "vertices": 7, "t_junctions": 0, "attached_ends": 2, "moved_ends": 2, "collapsed": 0,
                               "released": 0}
    line = capsys.readouterr().out
    assert line.strip() == plain_line.strip() + "; joined 4 edges at 7 vertices, 0 T-junctions, 2 ends moved"
    # the options reach join_edges
    assert S.main(argv + ["--join", "--join_tolerance", str(J.SCAN_TOLERANCE), "--join_reach", str(2 * EC.SCAN_RESOLUTION)]) == 0
    graph = json.loads(_listing(room)[S.GRAPH_FILE])
    assert graph["settings"]["reach"] == 2 * EC.SCAN_RESOLUTION and graph["counts"]["attached_ends"] == 0


def test_the_join_acts_on_the_last_product_of_the_chain(tmp_path):
    from curve_gaussian_amd.edge_extraction import support as S
    import edge_support_cases as SC
    base, data = SC.write_support_scan(tmp_path)
    room = os.path.join(base, "room")
    with open(os.path.join(room, "parametric_edges.json"), "w") as f:
        json.dump(C.constructed_edges(0.5), f)
    argv = ["--base_dir", base, "--dataset_dir", data, "--detector", "PidiNet", "--backend", "host", "--frames_ratio", "0.5",
            "--sample_resolution", str(EC.SCAN_RESOLUTION), "--min_visible", "0.5", "--keep_tolerance", "1"]
    trim = ["--trim", "--trim_max_gap", "3", "--trim_min_span", "10"]
    assert S.main(argv + trim + ["--dedupe"]) == 0
    before = _listing(room)
    assert S.main(argv + trim + ["--dedupe", "--join"]) == 0
    after = _listing(room)
    assert sorted(after) == sorted(list(before) + [S.GRAPH_FILE, S.JOINED_FILE])
    assert all(after[name] == before[name] for name in before)
    graph = json.loads(after[S.GRAPH_FILE])
    deduped = json.loads(after[S.DEDUPED_FILE])
    assert graph["input"] == S.DEDUPED_FILE and json.loads(after[S.JOINED_FILE]) == J.join_scan(deduped)["edge_dict"]
    for name in (S.GRAPH_FILE, S.JOINED_FILE, S.DEDUPE_FILE, S.DEDUPED_FILE):
        os.remove(os.path.join(room, name))
    assert S.main(argv + trim + ["--join"]) == 0
    assert json.loads(_listing(room)[S.GRAPH_FILE])["input"] == S.TRIMMED_FILE
    assert S.main(argv + ["--dedupe", "--join"]) == 0
    files = _listing(room)
    assert json.loads(files[S.GRAPH_FILE])["input"] == S.DEDUPED_FILE
    assert json.loads(files[S.JOINED_FILE]) == J.join_scan(J.constructed_pieces())["edge_dict"]


class _Model:
    """What write_parametric_edges reads of a model."""

    def __init__(self, curve_points, is_bezier):
        self.get_curve_points, self.is_bezier = curve_points, is_bezier


def test_the_export_with_the_flag_adds_two_files(tmp_path, capsys):
    from curve_gaussian_amd.edge_extraction import support as S
    from curve_gaussian_amd.scene import dataset_io as IO
    given = J.shortened_scan(3)
    curves, lines = J.edge_arrays(given)
    as_curves = np.stack([lines[:, 0], lines[:, 0], lines[:, 1], lines[:, 1]], 1)   # a line is its first and last point
    model = _Model(torch.from_numpy(np.concatenate([curves, as_curves])), torch.tensor([True] + [False] * 3))
    plain, flagged, both = tmp_path / "plain", tmp_path / "flagged", tmp_path / "both"
    IO.write_parametric_edges(model, str(plain))
    capsys.readouterr()
    options = dict(resolution=EC.SCAN_RESOLUTION, backend="host")
    d, _ = IO.write_parametric_edges(model, str(flagged), join=True, join_options=options)   # no cameras needed
    assert "joined:  4 edges,  7 vertices,  0 T-junctions,  2 ends moved" in capsys.readouterr().out
    assert sorted(os.listdir(plain)) == ["edge_points.ply", "parametric_edges.json"]
    assert sorted(os.listdir(flagged)) == sorted([S.GRAPH_FILE, "edge_points.ply", "parametric_edges.json", S.JOINED_FILE])
    for name in ("parametric_edges.json", "edge_points.ply"):
        assert open(flagged / name, "rb").read() == open(plain / name, "rb").read(), name
    assert json.load(open(flagged / S.JOINED_FILE)) == EJ.join_edges(d, **options)["edge_dict"]
    assert json.load(open(flagged / S.GRAPH_FILE))["input"] == "parametric_edges.json"
    IO.write_parametric_edges(model, str(both), dedupe=True, dedupe_options=options, join=True, join_options=options)
    assert sorted(os.listdir(both)) == sorted(["edge_points.ply", "parametric_edges.json", S.DEDUPE_FILE, S.DEDUPED_FILE,
                                               S.GRAPH_FILE, S.JOINED_FILE])
    assert json.load(open(both / S.GRAPH_FILE))["input"] == S.DEDUPED_FILE


def test_the_driver_parses_the_options():
    import inspect

    from curve_gaussian_amd import train as T
    _, _, args = T.parse_args(["-s", "scan", "-m", "out", "--join_edges", "--join_tolerance", "0.02", "--join_reach", "0.1"])
    assert args.join_edges and not args.dedupe_edges and not args.trim_edges
    assert T.join_options(args) == {"tolerance": 0.02, "reach": 0.1}
    assert set(T.join_options(args)) <= set(inspect.signature(EJ.join_edges).parameters)
    _, _, args = T.parse_args(["-s", "scan", "-m", "out"])
    assert not args.join_edges and T.join_options(args) == {}


# ------------------------------------------------------------------------------------------------ the C ABI
def test_abi_argument_checks_are_pinned():
    """Status and the exact text of cgs_last_error() for every rejection of cgs_end_attach; the pointers are dummies that
    are never dereferenced, and no row passes validation with work to do."""
    from curve_gaussian_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(64)
    fn = "cgs_end_attach: invalid argument "

    def call(P=5, points=p, E=2, offsets=p, tol2=0.25, reach2=4.0, keys=p, workspace=p):
        return lib.cgs_end_attach(P, points, E, offsets, tol2, reach2, keys, workspace, None)

    bounds = "; neither may be negative or NaN)"
    rows = [(dict(P=-1), "(P=-1, E=2)"), (dict(E=-1), "(P=5, E=-1)"), (dict(P=-2, E=-3, tol2=-1.0), "(P=-2, E=-3)"),
            (dict(P=0, E=-1), "(P=0, E=-1)"),
            (dict(tol2=-0.5), "(tol2=-0.5, reach2=4" + bounds), (dict(tol2=float("nan")), "(tol2=nan, reach2=4" + bounds),
            (dict(reach2=-0.25), "(tol2=0.25, reach2=-0.25" + bounds),
            (dict(reach2=float("nan"), points=None), "(tol2=0.25, reach2=nan" + bounds),
            (dict(E=0, tol2=-0.5), "(tol2=-0.5, reach2=4" + bounds)]
    rows += [({name: None}, "(NULL pointer; P=5, E=2)") for name in ("points", "offsets", "keys", "workspace")]
    rows += [(dict(P=0, offsets=None), "(NULL pointer; P=0, E=2)"), (dict(P=0, keys=None), "(NULL pointer; P=0, E=2)"),
             (dict(E=0, points=None), "(NULL pointer; P=5, E=0)"), (dict(P=0, E=0, workspace=None), "(NULL pointer; P=0, E=0)")]
    for kw, text in rows:
        assert call(**kw) == -1 and lib.cgs_last_error().decode() == fn + text, kw
    for kw in (dict(E=0), dict(E=0, keys=None), dict(P=0, E=0, points=None, keys=None), dict(E=0, tol2=0.0, reach2=0.0)):
        assert call(**kw) == 0, "no edge leaves no end to attach"
    assert _lib.SIGNATURES["cgs_end_attach"][1] == [ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_float,
                                                    ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    assert _lib.SIGNATURES["cgs_end_attach_workspace_bytes"] == (ctypes.c_size_t, [ctypes.c_int, ctypes.c_int])
    for P, E in ((0, 0), (1, 1), (256, 3), (257, 129), (2 ** 31 - 1, 2 ** 31 - 1)):
        assert lib.cgs_end_attach_workspace_bytes(P, E) == 4 * 128 + 16 * P + 2 * E * 40
