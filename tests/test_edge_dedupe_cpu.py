"""Host: dropping what a longer edge already covers (ops.edge_dedupe: edge_ranks, sample_cover, redundant_samples,
dedupe_edges) on the numpy back end -- the chunked cover against the all-pairs definition, the ranks and the run clearing on
hand-written inputs, the argument errors, the constructed scan whose result is known, the trimmed drawn scan, the command
line, the export, the driver's options and the C ABI's argument checks."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import edge_dedupe_cases as C
import edge_dir_cases as DC
import edge_score_cases as EC
import edge_support_cases as SC
from curve_gaussian_amd.ops import edge_dedupe as ED


# ------------------------------------------------------------------------------------------------ the cover
@pytest.mark.parametrize("P,E", C.SHAPES)
def test_the_chunked_cover_is_the_definition(P, E):
    pts, off, ranks = C.grid_case(P, E)
    assert len(pts) == P and len(ranks) == E
    for cos_min in (0.9, 0.0):
        got = ED.sample_cover(pts, off, ranks, C.GRID_TOL, cos_min, backend="host")
        assert got.dtype == torch.int32 and tuple(got.shape) == (P,)
        assert np.array_equal(got.numpy(), C.cover_brute(pts, off, ranks, C.GRID_TOL, cos_min))
    if P >= 256 and E >= 2:
        covered = got.numpy() != C.NO_COVER
        assert 0 < covered.sum() < P, "covered and free samples"


def test_the_grid_cases_sit_on_the_bound_of_the_distance_test():
    pts, off, ranks = C.grid_case(4161, 65)
    cells = np.round(pts / C.GRID).astype(np.int64)[:600]
    d2 = ((cells[:, None] - cells[None]) ** 2).sum(-1)
    assert (d2 == 25).any() and (d2 == 26).any() and (d2 == 24).any()


@pytest.mark.parametrize("cos_min", [0.0, 0.9, 1.0])
def test_equality_in_the_distance_and_in_the_direction_test_covers(cos_min):
    pts, off, ranks, want = C.equality_case()
    assert ranks.tolist() == [0, 1, 2, 3]
    got = ED.sample_cover(pts, off, ranks, C.GRID_TOL, cos_min, backend="host").numpy()
    assert np.array_equal(got, want) and np.array_equal(C.cover_brute(pts, off, ranks, C.GRID_TOL, cos_min), want)
    # a hair less tolerance: the pairs at exactly 5 cells go, B and D's coverers change
    less = ED.sample_cover(pts, off, ranks, np.nextafter(np.float32(C.GRID_TOL), np.float32(0)), cos_min, backend="host").numpy()
    assert (less[40:70] == C.NO_COVER).all() and (less[70:90] == 1).all() and (less[90:] == 0).all()


def test_the_direction_test_separates_crossing_edges():
    """Two lines through one point at 90 degrees: the shorter loses the samples near the crossing without the direction
    test and none with it; at 20 degrees it loses them either way (acos(0.9) is about 26 degrees)."""
    t = np.linspace(-1, 1, 41)[:, None]
    long_ = np.concatenate([t, 0 * t, 0 * t], 1)
    for degrees, cut in ((90, False), (20, True)):
        a = np.radians(degrees)
        short = np.concatenate([t[5:-5] * np.cos(a), t[5:-5] * np.sin(a), 0 * t[5:-5]], 1)
        pts = np.concatenate([long_, short]).astype(np.float32)
        off = np.array([0, 41, 72])
        ranks = ED.edge_ranks(off)
        free = ED.sample_cover(pts, off, ranks, 0.12, 0.0, backend="host").numpy() == C.NO_COVER
        assert free[:41].all() and not free[41:].all()
        free = ED.sample_cover(pts, off, ranks, 0.12, 0.9, backend="host").numpy() == C.NO_COVER
        assert free[:41].all() and free[41:].all() != cut


def test_coincident_points_and_zero_tangents():
    pts, off, ranks, want = C.coincident_case()
    for cos_min in (0.0, 1.0):
        assert np.array_equal(ED.sample_cover(pts, off, ranks, C.GRID_TOL, cos_min, backend="host").numpy(), want)
    # an edge of one sample has a zero tangent: 0 >= 0 passes, distance and rank decide
    pts = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [1, 0.5, 0]], np.float32)
    got = ED.sample_cover(pts, [0, 3, 4], [0, 1], 0.6, 1.0, backend="host")
    assert got.tolist() == [C.NO_COVER] * 3 + [0]


def test_the_clusters_touch_at_exactly_the_tolerance():
    pts, off, ranks = C.cluster_case()
    assert len(pts) == C.CLUSTER_LEAD + 128 * C.CLUSTERS
    got = ED.sample_cover(pts, off, ranks, C.GRID_TOL, 0.0, backend="host").numpy()
    for c in range(1, C.CLUSTERS):
        # the first sample of cluster c's short edge: only the far face of cluster c - 1 is within reach of it, and the
        # long edge of cluster c - 1 outranks everything of cluster c
        assert got[off[2 + 2 * c]] == ranks[1 + 2 * (c - 1)], c
    assert (got[:C.CLUSTER_LEAD] == C.NO_COVER).all()


def test_whole_tiles_exactly_a_tolerance_apart():
    """The input that puts the kernel's box cull on its bound (the host back end has no cull: it is the yardstick there).
    At a gap of 5 cells every pair of neighbouring tiles has fl(g*g) == tol2 and one pair of samples at d2 == tol2 decides
    a cover across it; one cell more and the tiles are out of reach and the same samples are covered from their own
    cluster, if at all."""
    pts, off, ranks, queries = C.tile_gap_case(5)
    assert len(pts) == C.GAP_CLUSTERS * C.TILE and C.tile_box_gaps(pts, C.GRID_TOL) == (2 * (C.GAP_CLUSTERS - 1), 20)
    assert C.tile_box_gaps(C.cluster_case()[0], C.GRID_TOL)[0] == 0, "the straddling clusters never sit on the bound"
    got = ED.sample_cover(pts, off, ranks, C.GRID_TOL, 0.0, backend="host").numpy()
    assert np.array_equal(got, C.cover_brute(pts, off, ranks, C.GRID_TOL, 0.0))
    assert [int(got[i]) for i, _ in queries] == [r for _, r in queries]
    wide, off6, ranks6, queries6 = C.tile_gap_case(6)
    assert C.tile_box_gaps(wide, C.GRID_TOL) == (0, C.GAP_CLUSTERS * (C.GAP_CLUSTERS - 1)) and queries6 == queries
    got = ED.sample_cover(wide, off6, ranks6, C.GRID_TOL, 0.0, backend="host").numpy()
    assert np.array_equal(got, C.cover_brute(wide, off6, ranks6, C.GRID_TOL, 0.0))
    assert all(int(got[i]) > r for i, r in queries6), "only the own cluster is left to cover them"


# ------------------------------------------------------------------------------------------------ ranks and runs
def test_ranks():
    assert ED.edge_ranks([0]).tolist() == [] and ED.edge_ranks([0, 5]).tolist() == [0]
    ranks = ED.edge_ranks(np.array([0, 3, 3, 8, 11, 11, 16, 17], np.int32))   # sizes 3, 0, 5, 3, 0, 5, 1
    assert ranks.dtype == np.int32 and ranks.tolist() == [2, 5, 0, 3, 6, 1, 4], "ties by edge index; empty edges last"
    assert ED.edge_ranks(torch.tensor([0, 2, 4])).tolist() == [0, 1]
    with pytest.raises(ValueError, match="offsets"):
        ED.edge_ranks([0, 3, 2])


def _cover(text):
    return np.array([0 if ch == "1" else C.NO_COVER for ch in text], np.int32)


def test_short_runs_of_covered_samples_are_cleared():
    flags = lambda text, off, m: "".join("1" if f else "0" for f in ED.redundant_samples(_cover(text), off, m))
    assert flags("", [0], 3) == "" and flags("0000", [0, 4], 2) == "0000"
    assert flags("0111011", [0, 7], 3) == "0111000", "a run of min_run stays, one of min_run - 1 goes"
    assert flags("0111011", [0, 7], 2) == "0111011" and flags("0111011", [0, 7], 4) == "0000000"
    assert flags("1110111", [0, 7], 3) == "1110111", "runs that touch both ends of the edge"
    assert flags("11011", [0, 5], 3) == "00000"
    # runs never join across edges: 2 + 2 covered samples on either side of an edge's end are two runs of 2
    assert flags("011110", [0, 3, 6], 3) == "000000" and flags("011110", [0, 6], 3) == "011110"
    assert flags("0111" + "1110", [0, 4, 4, 8], 3) == "01111110"
    got = ED.redundant_samples(torch.from_numpy(_cover("0111")), torch.tensor([0, 4]), 3)
    assert got.dtype == bool and got.tolist() == [False, True, True, True]
    mixed = np.array([C.NO_COVER, 7, 0, 3], np.int32)
    assert ED.redundant_samples(mixed, [0, 4], 3).tolist() == [False, True, True, True], "any rank is a cover"


def test_argument_errors():
    pts = np.zeros((4, 3), np.float32)
    call = lambda pts=pts, off=(0, 2, 4), ranks=(0, 1), tol=0.1, cos=0.9, **kw: ED.sample_cover(pts, off, ranks, tol, cos,
                                                                                               **{"backend": "host", **kw})
    assert call().tolist() == [C.NO_COVER] * 2 + [0, 0]
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
    for bad in (-0.1, 1.1, float("nan")):
        with pytest.raises(ValueError, match="cos_min"):
            call(cos=bad)
    for bad in ((0, 0), (0, 2), (1, 2), (-1, 0), (0,), (0, 1, 2)):
        with pytest.raises(ValueError, match="ranks"):
            call(ranks=bad)
    with pytest.raises(ValueError, match="ranks"):
        call(ranks=(0.0, 1.0))
    with pytest.raises(ValueError, match="backend"):
        call(backend="cuda")
    with pytest.raises(ValueError, match="min_run"):
        ED.redundant_samples(_cover("11"), [0, 2], 1)
    with pytest.raises(ValueError, match="cover"):
        ED.redundant_samples(np.zeros(2, np.int64), [0, 2], 2)
    with pytest.raises(ValueError, match="offsets"):
        ED.redundant_samples(_cover("11"), [0, 3], 2)
    for kw in (dict(min_run=1), dict(min_span=1), dict(tolerance=0.0), dict(tolerance=-1.0), dict(cos_min=1.5),
               dict(backend="cuda")):
        with pytest.raises(ValueError, match=next(iter(kw))):
            ED.dedupe_edges(EC.SCAN_EDGES, resolution=EC.SCAN_RESOLUTION, **{"backend": "host", **kw})
    if not torch.cuda.is_available():
        from curve_gaussian_amd import _lib
        with pytest.raises(_lib.CurveGSError, match="GPU"):
            call(backend="gpu")
        with pytest.raises(_lib.CurveGSError, match="GPU tensor"):
            call(pts=torch.from_numpy(pts), backend="gpu")


# ------------------------------------------------------------------------------------------------ the constructed scan
def _pieces(r):
    curves = np.array(r["edge_dict"]["curves_ctl_pts"]).reshape(-1, 4, 3)
    lines = np.array(r["edge_dict"]["lines_end_pts"]).reshape(-1, 2, 3)
    return curves, lines


@pytest.mark.parametrize("delta", [0.5, 1.0])
def test_the_constructed_scan_comes_out_as_built(delta):
    """The four drawn edges, a shifted copy of the range [0.2, 0.7] of each and one line per drawn line that leaves it at
    10 degrees: the drawn edges come back bit for bit, the copies yield nothing, and each leaving line keeps one piece from
    the sample at which it is a tolerance away from its drawn line, tolerance / (resolution sin 10 deg) = 11.5 samples at 2
    resolutions and 17.3 at 3, to its end.  Measured (host, both shifts): the pieces begin at samples 11, 11 and 12 at 2
    resolutions and at 17, 17 and 17 at 3.  The bound of +-2 samples is one sample of quantisation on the leaving line plus
    half a sample spacing to the nearest drawn sample, rounded up."""
    given = C.constructed_edges(delta)
    curves = np.array(given["curves_ctl_pts"]).reshape(-1, 4, 3)
    lines = np.array(given["lines_end_pts"]).reshape(-1, 2, 3)
    results = {}
    for tol in (2.0, 3.0):
        r = C.constructed_dedupe(delta, "host", tol)
        n = np.diff(r["offsets"].astype(np.int64))
        assert n.tolist() == [199, 93, 152, 170, 180, 76, 85, 90, 68, 76, 81]
        assert [n[e] for e in C.DRAWN] == C.DRAWN_SAMPLES and [n[e] for e in C.COPIES] == C.COPY_SAMPLES
        assert [n[e] for e in C.LEAVING] == C.LEAVE_SAMPLES
        starts = [r["spans"][e][0][0] for e in C.LEAVING]
        print(f"shift {delta}, tolerance {tol} resolutions: spans {r['spans']}, covered by {r['covered_by']}; the leaving "
              f"pieces begin at {starts}, expected about {C.leave_start(tol):.1f}")
        for e in C.DRAWN:
            assert r["spans"][e] == [(0, int(n[e]) - 1)] and r["covered_by"][e] == []
        for e, drawn in zip(C.COPIES, C.DRAWN):
            assert r["spans"][e] == [] and r["covered_by"][e] == [drawn]
            assert r["redundant"][r["offsets"][e]:r["offsets"][e + 1]].all()
        for e, start in zip(C.LEAVING, starts):
            assert r["spans"][e] == [(start, int(n[e]) - 1)], "one piece, to the end"
            assert abs(start - C.leave_start(tol)) <= 2.0
        assert r["source"].tolist() == [0, 2, 3, 4, 8, 9, 10]
        got_c, got_l = _pieces(r)
        assert np.array_equal(got_c, curves[:1]) and np.array_equal(got_l[:3], lines[:3]), "the drawn edges, bit for bit"
        assert np.array_equal(got_l[3:, 1], lines[6:, 1]), "a leaving piece ends where its line ends"
        assert r["ranks"].tolist() == ED.edge_ranks(r["offsets"]).tolist() and r["cover"].dtype == torch.int32
        assert r["settings"] == {"resolution": EC.SCAN_RESOLUTION, "tolerance": tol * EC.SCAN_RESOLUTION, "cos_min": 0.9,
                                 "min_run": 3, "min_span": 10, "backend": "host", "points": int(n.sum())}
        results[tol] = r
    other = C.constructed_dedupe(delta, "host", 2.0, 0.95, 2)
    assert other["spans"] == results[2.0]["spans"] and other["edge_dict"] == results[2.0]["edge_dict"]


def test_the_drawn_edges_survive_the_trimmed_scan():
    """The 44 pieces that trimming leaves of the drawn edges and the 72 bogus chords (scan_trim("bogus", max_gap 3, min_span
    10)) at the defaults: the four drawn edges are the four longest, only one another could cover them, and they do not.
    Measured: 27 pieces are left at a tolerance of 2 resolutions and 9 at 8 resolutions; the surviving stubs, 10 to 37
    samples long, leave the drawn edges obliquely and are no parallel duplicates.  Only the invariant is asserted."""
    edges = C.trimmed_scan_edges()
    assert len(edges["curves_ctl_pts"]) + len(edges["lines_end_pts"]) == 44
    r = ED.dedupe_edges(edges, resolution=EC.SCAN_RESOLUTION, backend="host")
    assert r["settings"]["tolerance"] == 2.0 * EC.SCAN_RESOLUTION and r["settings"]["cos_min"] == ED.COS_MIN == 0.9
    assert r["settings"]["min_run"] == ED.MIN_RUN == 3 and r["settings"]["min_span"] == ED.MIN_SPAN == 10
    wide = ED.dedupe_edges(edges, resolution=EC.SCAN_RESOLUTION, tolerance=8 * EC.SCAN_RESOLUTION, backend="host")
    print(f"44 pieces: {len(r['source'])} after deduping at 2 resolutions, {len(wide['source'])} at 8")
    drawn_c = np.array(EC.SCAN_EDGES["curves_ctl_pts"]).reshape(-1, 4, 3)
    drawn_l = np.array(EC.SCAN_EDGES["lines_end_pts"]).reshape(-1, 2, 3)
    given_c, given_l = _pieces({"edge_dict": edges})
    longest = np.argsort(r["ranks"])[:4]
    assert (longest < len(given_c)).sum() == 1 and np.array_equal(given_c[longest[longest < len(given_c)]], drawn_c)
    assert np.array_equal(given_l[np.sort(longest[longest >= len(given_c)]) - len(given_c)], drawn_l), "the four longest"
    got_c, got_l = _pieces(r)
    assert any(np.array_equal(c, drawn_c[0]) for c in got_c)
    for l in drawn_l:
        assert any(np.array_equal(l, g) for g in got_l)
    for e in longest:
        assert r["covered_by"][e] == [] and not r["redundant"][r["offsets"][e]:r["offsets"][e + 1]].any()
    assert len(wide["source"]) <= len(r["source"]) < 44


# ------------------------------------------------------------------------------------------------ files
DEDUPE_ARGS = ["--dedupe", "--dedupe_tolerance", str(2 * EC.SCAN_RESOLUTION), "--dedupe_min_run", "3", "--dedupe_min_span", "10",
               "--dedupe_cos_min", "0.9"]


def test_the_command_line_writes_its_two_files_and_no_other(tmp_path, capsys):
    from curve_gaussian_amd.edge_extraction import support as S
    base, data = SC.write_support_scan(tmp_path)
    room = os.path.join(base, "room")
    pred = os.path.join(room, "parametric_edges.json")
    given = C.constructed_edges(0.5)
    with open(pred, "w") as f:
        json.dump(given, f)
    argv = ["--base_dir", base, "--dataset_dir", data, "--detector", "PidiNet", "--backend", "host", "--frames_ratio", "0.5",
            "--sample_resolution", str(EC.SCAN_RESOLUTION), "--min_visible", "0.5", "--keep_tolerance", "1", "--write_filtered",
            "--trim", "--trim_max_gap", "3", "--trim_min_span", "10"]
    assert S.main(argv) == 0
    five = ["parametric_edges.json", S.SUPPORT_FILE, S.FILTERED_FILE, S.TRIM_FILE, S.TRIMMED_FILE]
    assert sorted(os.listdir(room)) == sorted(five)
    before = {name: open(os.path.join(room, name), "rb").read() for name in five}
    plain_line = capsys.readouterr().out
    assert "deduped" not in plain_line
    # with --trim the trimmed pieces are deduped
    assert S.main(argv + DEDUPE_ARGS) == 0
    assert sorted(os.listdir(room)) == sorted(five + [S.DEDUPE_FILE, S.DEDUPED_FILE])
    for name in five:
        assert open(os.path.join(room, name), "rb").read() == before[name], name
    trimmed = json.load(open(os.path.join(room, S.TRIMMED_FILE)))
    want = ED.dedupe_edges(trimmed, resolution=EC.SCAN_RESOLUTION, backend="host")
    assert json.load(open(os.path.join(room, S.DEDUPED_FILE))) == want["edge_dict"]
    out = json.load(open(os.path.join(room, S.DEDUPE_FILE)))
    n = np.diff(want["offsets"].astype(np.int64))
    total = len(trimmed["curves_ctl_pts"]) + len(trimmed["lines_end_pts"])
    assert out["scan"] == "room" and out["input"] == S.TRIMMED_FILE and out["total"] == total == len(n)
    assert out["pieces"] == len(want["source"]) and out["samples"] == n.sum()
    assert out["redundant_samples"] == int(want["redundant"].sum()) and out["settings"] == want["settings"]
    nc = len(trimmed["curves_ctl_pts"])
    for e, rec in enumerate(out["edges"]):
        assert sorted(rec) == ["covered_by", "index", "kind", "redundant_samples", "samples", "spans"]
        assert rec["kind"] == ("curve" if e < nc else "line") and rec["index"] == (e if e < nc else e - nc)
        assert rec["samples"] == n[e] and rec["spans"] == [list(s) for s in want["spans"][e]]
        assert rec["covered_by"] == want["covered_by"][e]
        assert rec["redundant_samples"] == int(want["redundant"][want["offsets"][e]:want["offsets"][e + 1]].sum())
    line = capsys.readouterr().out
    assert line.strip() == plain_line.strip() + f"; deduped to {out['pieces']} pieces, {out['redundant_samples']} of {n.sum()} " \
                                                "samples redundant"
    # without --trim the edges of parametric_edges.json are deduped
    for name in (S.TRIM_FILE, S.TRIMMED_FILE, S.DEDUPE_FILE, S.DEDUPED_FILE):
        os.remove(os.path.join(room, name))
    assert S.main(argv[:argv.index("--trim")] + DEDUPE_ARGS) == 0
    assert sorted(os.listdir(room)) == sorted(five[:3] + [S.DEDUPE_FILE, S.DEDUPED_FILE])
    for name in five[:3]:
        assert open(os.path.join(room, name), "rb").read() == before[name], name
    assert json.load(open(os.path.join(room, S.DEDUPED_FILE))) == C.constructed_dedupe(0.5, "host")["edge_dict"]
    out = json.load(open(os.path.join(room, S.DEDUPE_FILE)))
    assert out["input"] == "parametric_edges.json" and out["total"] == 11 and out["pieces"] == 7


class _Model:
    """What write_parametric_edges reads of a model."""

    def __init__(self, curve_points, is_bezier):
        self.get_curve_points, self.is_bezier = curve_points, is_bezier


def test_the_export_with_the_flag_adds_two_files(tmp_path, capsys):
    from curve_gaussian_amd.edge_extraction import support as S
    from curve_gaussian_amd.scene import dataset_io as IO
    given = C.constructed_edges(1.0)
    curves = np.array(given["curves_ctl_pts"]).reshape(-1, 4, 3)
    lines = np.array(given["lines_end_pts"]).reshape(-1, 2, 3)
    as_curves = np.stack([lines[:, 0], lines[:, 0], lines[:, 1], lines[:, 1]], 1)   # a line is its first and last point
    model = _Model(torch.from_numpy(np.concatenate([curves, as_curves])), torch.tensor([True] * 2 + [False] * 9))
    plain, flagged, both = tmp_path / "plain", tmp_path / "flagged", tmp_path / "both"
    IO.write_parametric_edges(model, str(plain))
    capsys.readouterr()
    options = dict(resolution=EC.SCAN_RESOLUTION, backend="host")
    d, _ = IO.write_parametric_edges(model, str(flagged), dedupe=True, dedupe_options=options)   # no cameras needed
    assert "before deduping:  11 edges, after deduping:  7 pieces" in capsys.readouterr().out
    assert sorted(os.listdir(plain)) == ["edge_points.ply", "parametric_edges.json"]
    assert sorted(os.listdir(flagged)) == [S.DEDUPE_FILE, "edge_points.ply", "parametric_edges.json", S.DEDUPED_FILE]
    for name in ("parametric_edges.json", "edge_points.ply"):
        assert open(flagged / name, "rb").read() == open(plain / name, "rb").read(), name
    assert json.load(open(flagged / S.DEDUPED_FILE)) == ED.dedupe_edges(d, resolution=EC.SCAN_RESOLUTION, backend="host")["edge_dict"]
    # after trim, the trimmed pieces are deduped
    cams, maps = DC.dir_novel_cameras()
    trim = dict(resolution=EC.SCAN_RESOLUTION, frames_ratio=0.5, backend="host")
    IO.write_parametric_edges(model, str(both), detector="PidiNet", trim=True, trim_options=trim, cameras=cams, edge_maps=maps,
                              dedupe=True, dedupe_options=options)
    assert sorted(os.listdir(both)) == sorted(["edge_points.ply", "parametric_edges.json", S.TRIM_FILE, S.TRIMMED_FILE,
                                               S.DEDUPE_FILE, S.DEDUPED_FILE])
    trimmed = json.load(open(both / S.TRIMMED_FILE))
    assert json.load(open(both / S.DEDUPED_FILE)) == ED.dedupe_edges(trimmed, resolution=EC.SCAN_RESOLUTION,
                                                                     backend="host")["edge_dict"]
    assert json.load(open(both / S.DEDUPE_FILE))["input"] == S.TRIMMED_FILE


def test_the_driver_parses_the_options():
    import inspect

    from curve_gaussian_amd import train as T
    _, _, args = T.parse_args(["-s", "scan", "-m", "out", "--dedupe_edges", "--dedupe_tolerance", "0.02", "--dedupe_cos_min",
                               "0.95", "--dedupe_min_run", "4", "--dedupe_min_span", "6"])
    assert args.dedupe_edges and not args.trim_edges
    assert T.dedupe_options(args) == {"tolerance": 0.02, "cos_min": 0.95, "min_run": 4, "min_span": 6}
    assert set(T.dedupe_options(args)) <= set(inspect.signature(ED.dedupe_edges).parameters)
    _, _, args = T.parse_args(["-s", "scan", "-m", "out"])
    assert not args.dedupe_edges and T.dedupe_options(args) == {}


# ------------------------------------------------------------------------------------------------ the C ABI
def test_abi_argument_checks_are_pinned():
    """Status and the exact text of cgs_last_error() for every rejection of cgs_sample_cover; the pointers are dummies
    that are never dereferenced, and no row passes validation with work to do."""
    from curve_gaussian_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(64)
    fn = "cgs_sample_cover: invalid argument "

    def call(P=5, points=p, E=2, offsets=p, rank=p, tol2=0.25, cos2=0.81, cover=p, workspace=p):
        return lib.cgs_sample_cover(P, points, E, offsets, rank, tol2, cos2, cover, workspace, None)

    bounds = "; tol2 >= 0 and cos2 lies in [0, 1])"
    rows = [(dict(P=-1), "(P=-1, E=2)"), (dict(E=-1), "(P=5, E=-1)"), (dict(P=-2, E=-3, tol2=-1.0), "(P=-2, E=-3)"),
            (dict(P=0, E=-1), "(P=0, E=-1)"),
            (dict(tol2=-0.5), "(tol2=-0.5, cos2=0.81" + bounds), (dict(tol2=float("nan")), "(tol2=nan, cos2=0.81" + bounds),
            (dict(cos2=-0.25), "(tol2=0.25, cos2=-0.25" + bounds), (dict(cos2=1.5), "(tol2=0.25, cos2=1.5" + bounds),
            (dict(cos2=float("nan"), points=None), "(tol2=0.25, cos2=nan" + bounds),
            (dict(P=0, tol2=-0.5), "(tol2=-0.5, cos2=0.81" + bounds), (dict(E=0, cos2=2.0), "(tol2=0.25, cos2=2" + bounds)]
    rows += [({name: None}, "(NULL pointer; P=5, E=2)") for name in ("points", "offsets", "rank", "cover", "workspace")]
    rows += [(dict(P=0, offsets=None), "(NULL pointer; P=0, E=2)"), (dict(E=0, rank=None), "(NULL pointer; P=5, E=0)"),
             (dict(E=0, cover=None), "(NULL pointer; P=5, E=0)"), (dict(P=0, E=0, workspace=None), "(NULL pointer; P=0, E=0)")]
    for kw, text in rows:
        assert call(**kw) == -1 and lib.cgs_last_error().decode() == fn + text, kw
    for kw in (dict(P=0), dict(E=0), dict(P=0, points=None, cover=None), dict(P=0, E=0, points=None, cover=None),
               dict(P=0, tol2=0.0, cos2=0.0), dict(E=0, cos2=1.0)):
        assert call(**kw) == 0, "no sample or no edge leaves nothing to cover"
    assert _lib.SIGNATURES["cgs_sample_cover"][1] == [ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                                                      ctypes.c_void_p, ctypes.c_float, ctypes.c_float, ctypes.c_void_p,
                                                      ctypes.c_void_p, ctypes.c_void_p]
    assert _lib.SIGNATURES["cgs_sample_cover_workspace_bytes"] == (ctypes.c_size_t, [ctypes.c_int])
    for P in (0, 1, 256, 257, 2 ** 31 - 1):
        tiles = (P + 255) // 256
        assert lib.cgs_sample_cover_workspace_bytes(P) == 4 * 128 + 32 * P + 32 * tiles
