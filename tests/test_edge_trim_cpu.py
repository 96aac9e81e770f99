"""Host: trimming extracted edges to their supported spans (ops.edge_trim: sample_tally, supported_samples, supported_spans,
trim_geometry, trim_edges) on the numpy back end -- the tally against a brute-force loop and against the per-edge counts of
ops.edge_support, the spans on hand-written flags, the pieces against their parent curves, the drawn scan with over-extended
edges and with bogus chords, the chunking, the command line, the export and the C ABI's argument checks."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import edge_dir_cases as DC
import edge_score_cases as EC
import edge_support_cases as SC
import edge_trim_cases as C
from curve_gaussian_amd.ops import edge_score as ES
from curve_gaussian_amd.ops import edge_support as SP
from curve_gaussian_amd.ops import edge_trim as ET


# ------------------------------------------------------------------------------------------------ the tally
@pytest.mark.parametrize("tol", SC.TOLERANCES, ids=["T1", "T4"])
def test_tally_against_the_brute_force_and_the_edge_counts(tol):
    V, W = 5, 33
    K, M = SC.support_cameras(V, W)
    d2 = SC.support_d2(V, W)
    sizes = np.array([0, 1, 2, 63, 64, 65, 0, 130, 9, 0])
    pts, off = SC.support_points(sizes, W)
    got = ET.sample_tally(pts, K, M, d2, tol, backend="host")
    assert got.dtype == torch.int32 and tuple(got.shape) == (len(pts), 1 + len(tol))
    want = C.tally_brute(pts, K, M, d2, ES.tolerances_squared(tol))
    assert np.array_equal(got.numpy(), want)
    assert 0 < want[:, 0].sum() < V * len(pts), "the case must hold points inside and outside the views"
    assert (want[:, 1:] <= want[:, :1]).all() and 0 < want[:, -1].sum() < want[:, 0].sum() and want[:, 0].max() == V
    # the existing kernel's numbers pin the new one: summed over an edge's samples and over the views they are the same
    counts = SP.support_counts(pts, off, K, M, d2, tol, backend="host").numpy()
    for e in range(len(sizes)):
        assert np.array_equal(want[off[e]:off[e + 1]].sum(0), counts[e].sum(0)), e


def test_the_tally_adds_to_the_one_handed_in():
    V, W = 5, 33
    K, M = SC.support_cameras(V, W)
    d2 = SC.support_d2(V, W)
    pts = C.tally_points(130, W)
    whole = ET.sample_tally(pts, K, M, d2, (1, 2.5), backend="host")
    out = torch.zeros((130, 3), dtype=torch.int32)
    assert ET.sample_tally(pts, K[:2], M[:2], d2[:2], (1, 2.5), backend="host", out=out) is out
    ET.sample_tally(pts, K[2:], M[2:], d2[2:], (1, 2.5), backend="host", out=out)
    assert torch.equal(out, whole) and whole.any()
    seven = torch.full((130, 3), 7, dtype=torch.int32)
    ET.sample_tally(pts, K, M, d2, (1, 2.5), backend="host", out=seven)
    assert torch.equal(seven, whole + 7)
    none = ET.sample_tally(pts, K[:0], M[:0], d2[:0], (1,), backend="host")
    assert tuple(none.shape) == (130, 2) and not none.any()
    assert tuple(ET.sample_tally(pts[:0], K, M, d2, (1,), backend="host").shape) == (0, 2)


def test_argument_errors():
    K, M = SC.support_cameras(1, 4)
    d2 = np.zeros((1, 3, 4), np.int32)
    pts = np.zeros((2, 3), np.float32)
    call = lambda pts=pts, K=K, M=M, d2=d2, tol=(1,), **kw: ET.sample_tally(pts, K, M, d2, tol, **{"backend": "host", **kw})
    assert call().tolist() == [[0, 0], [0, 0]]
    with pytest.raises(ValueError, match="float32"):
        call(pts=pts.astype(np.float64))
    with pytest.raises(ValueError, match=r"\[P,3\]"):
        call(pts=np.zeros((2, 4), np.float32))
    with pytest.raises(ValueError, match="int32"):
        call(d2=d2.astype(np.int64))
    with pytest.raises(ValueError, match="d2"):
        call(d2=np.zeros((2, 3, 4), np.int32))
    with pytest.raises(ValueError, match="tolerances"):
        call(tol=())
    with pytest.raises(ValueError, match="tolerances"):
        call(tol=(1, 2, 3, 4, 5))
    with pytest.raises(ValueError, match="backend"):
        call(backend="cuda")
    for bad in (torch.zeros((2, 3), dtype=torch.int32), torch.zeros((2, 2), dtype=torch.int64), np.zeros((2, 2), np.int32),
                torch.zeros((2, 4), dtype=torch.int32)[:, ::2]):
        with pytest.raises(ValueError, match="out must be"):
            call(out=bad)
    if not torch.cuda.is_available():
        from curve_gaussian_amd import _lib
        with pytest.raises(_lib.CurveGSError, match="GPU tensor"):
            call(backend="gpu")


def test_the_frame_rule_per_sample():
    tally = np.array([[12, 7], [12, 6], [3, 0], [7, 7]], np.int32)
    assert ET.supported_samples(tally, 12, 0.5).tolist() == [[True], [False], [False], [True]], "MORE than ceil(0.5 * 12) = 6"
    assert ET.supported_samples(torch.from_numpy(tally), 12, 0.05).tolist() == [[True], [True], [False], [True]], "more than 1"
    assert ET.supported_samples(tally, 13, 0.5).tolist() == [[False], [False], [False], [False]], "ceil(6.5) = 7"
    two = ET.supported_samples(np.array([[5, 5, 2]], np.int32), 4, 0.5)
    assert two.dtype == bool and two.tolist() == [[True, False]]
    with pytest.raises(ValueError, match="tally"):
        ET.supported_samples(tally[:, :1], 12, 0.5)
    with pytest.raises(ValueError, match="frames_ratio"):
        ET.supported_samples(tally, 12, 1.5)


# ------------------------------------------------------------------------------------------------ the spans
def _flags(text):
    return np.array([ch == "1" for ch in text], bool)


def test_spans_of_hand_written_flags():
    spans = lambda text, off, g, m: ET.supported_spans(_flags(text), off, g, m)
    assert spans("", [0], 0, 2) == [] and spans("", [0, 0, 0], 3, 10) == [[], []], "no edge; empty edges"
    assert spans("0000", [0, 4], 0, 2) == [[]] and spans("1111", [0, 4], 0, 2) == [[(0, 3)]]
    assert spans("1", [0, 1], 0, 2) == [[]] and spans("11", [0, 2], 0, 2) == [[(0, 1)]], "one sample is never a span"
    # a gap of exactly max_gap is bridged, one of max_gap + 1 is not
    assert spans("1110001111", [0, 10], 3, 2) == [[(0, 9)]]
    assert spans("11100001111", [0, 11], 3, 2) == [[(0, 2), (7, 10)]]
    assert spans("1101", [0, 4], 0, 2) == [[(0, 1)]], "max_gap 0 bridges nothing"
    # a run of exactly min_span stays, one of min_span - 1 goes
    assert spans("0111100111", [0, 10], 0, 4) == [[(1, 4)]]
    assert spans("0111100111", [0, 10], 0, 3) == [[(1, 4), (7, 9)]]
    # merging comes first: two runs of 2 and a gap of 1 make a span of 5, which min_span 4 keeps
    assert spans("0110110", [0, 7], 1, 4) == [[(1, 5)]] and spans("0110110", [0, 7], 0, 4) == [[]]
    assert spans("101010101", [0, 9], 1, 9) == [[(0, 8)]], "a chain of merges"
    # several edges in one call: runs do not cross an edge's end, gaps are not bridged across it, indices are local
    text, off = "111" + "11011" + "" + "0110" + "1", [0, 3, 8, 8, 12, 13]
    assert spans(text, off, 1, 2) == [[(0, 2)], [(0, 4)], [], [(1, 2)], []]
    assert spans(text, off, 0, 3) == [[(0, 2)], [], [], [], []]
    assert spans("1111", [0, 2, 4], 5, 2) == [[(0, 1)], [(0, 1)]]
    assert ET.supported_spans(torch.from_numpy(_flags("0110")), torch.tensor([0, 4]), 0, 2) == [[(1, 2)]]


def test_spans_against_a_loop():
    rng = np.random.default_rng(5)
    sizes = rng.integers(0, 40, 60)
    off = np.concatenate([[0], np.cumsum(sizes)])
    flags = rng.random(off[-1]) < 0.7
    several = []
    for max_gap, min_span in ((0, 2), (1, 3), (3, 10)):
        want = []
        for e in range(len(sizes)):
            f, runs = flags[off[e]:off[e + 1]], []
            for i in np.flatnonzero(f):
                if runs and i - runs[-1][1] - 1 <= max_gap:
                    runs[-1][1] = int(i)
                else:
                    runs.append([int(i), int(i)])
            want.append([(a, b) for a, b in runs if b - a + 1 >= min_span])
        assert ET.supported_spans(flags, off, max_gap, min_span) == want
        several.append(max(len(w) for w in want))
    assert several[0] > 2 and several[1] > 1 and min(several) >= 1, "edges with several spans, and spans at every setting"


def test_span_argument_errors():
    with pytest.raises(ValueError, match="min_span"):
        ET.supported_spans(_flags("11"), [0, 2], 0, 1)
    with pytest.raises(ValueError, match="max_gap"):
        ET.supported_spans(_flags("11"), [0, 2], -1, 2)
    with pytest.raises(ValueError, match="offsets"):
        ET.supported_spans(_flags("11"), [0, 3], 0, 2)
    with pytest.raises(ValueError, match="flags"):
        ET.supported_spans(np.array([1, 1]), [0, 2], 0, 2)


# ------------------------------------------------------------------------------------------------ the pieces
def _random_edges(seed=2):
    rng = np.random.default_rng(seed)
    return rng.uniform(0, 1, (3, 4, 3)), rng.uniform(0, 1, (2, 2, 3))


def test_a_full_span_returns_the_input_bits():
    curves, lines = _random_edges()
    off = np.array([0, 40, 47, 47, 60, 62])   # edge 2, a curve, has no samples
    spans = [[(0, 39)], [(0, 6)], [], [(0, 12)], [(0, 1)]]
    c, l, src = ET.trim_geometry(curves.reshape(3, 12), lines.reshape(2, 6), off, spans)
    assert c.dtype == np.float64 and l.dtype == np.float64 and src.tolist() == [0, 1, 3, 4]
    assert np.array_equal(c, curves[:2]) and np.array_equal(l, lines)
    c, l, src = ET.trim_geometry(curves, lines, off, [[], [], [], [], []])
    assert c.shape == (0, 4, 3) and l.shape == (0, 2, 3) and src.shape == (0,)
    c, l, src = ET.trim_geometry([], [], [0], [])
    assert c.shape == (0, 4, 3) and l.shape == (0, 2, 3) and src.shape == (0,)


def test_a_piece_matches_its_parent_over_the_span():
    curves, lines = _random_edges()
    off = np.array([0, 40, 47, 147, 160, 171])
    spans = [[(3, 17), (17, 39)], [(0, 5)], [(1, 99)], [(2, 9)], [(0, 4), (7, 10)]]
    c, l, src = ET.trim_geometry(curves, lines, off, spans)
    assert src.tolist() == [0, 0, 1, 2, 3, 4, 4] and c.shape == (4, 4, 3) and l.shape == (3, 2, 3)
    s = np.linspace(0, 1, 101)
    pieces = [(e, a, b) for e in range(5) for a, b in spans[e]]
    for k, (e, a, b) in enumerate(pieces):
        n = off[e + 1] - off[e]
        t = a / (n - 1) + (b / (n - 1) - a / (n - 1)) * s
        if e < 3:
            err = np.abs(C.bezier_points(c[k], s) - C.bezier_points(curves[e], t)).max()
        else:
            p = lines[e - 3]
            err = np.abs((l[k - 4, 0] + s[:, None] * (l[k - 4, 1] - l[k - 4, 0])) - (p[0] + t[:, None] * (p[1] - p[0]))).max()
        assert err <= 1e-12, (e, a, b, err)
    assert np.array_equal(c[0, 3], c[1, 0]), "two adjacent spans of a curve share their end point exactly"
    assert np.array_equal(c[1, 3], curves[0, 3]) and np.array_equal(c[2, 0], curves[1, 0]), "B(1,1,1) and B(0,0,0)"
    for bad in ([[(0, 40)], [], [], [], []], [[(5, 5)], [], [], [], []], [[(-1, 4)], [], [], [], []]):
        with pytest.raises(ValueError, match="span"):
            ET.trim_geometry(curves, lines, off, bad)
    with pytest.raises(ValueError, match="edges"):
        ET.trim_geometry(curves, lines, off, spans[:-1])


# ------------------------------------------------------------------------------------------------ the drawn scan
def test_the_drawn_scan_keeps_the_supported_part_of_an_over_extended_edge():
    """Twelve views of 96 x 128; the four drawn edges of EC.SCAN_EDGES, each over-extended at one end (the lines by 40 % of
    their length, the curve re-cut over [-0.3, 1]).  Measured (host back end, more than 6 of 12 views, the raw runs): the
    per-edge verdict of edge_support drops the three lines (curve, lines 0 to 2: pooled shares 0.827, 0.747, 0.746, 0.740 at
    1 px and 0.845, 0.768, 0.762, 0.754 at 2 px against min_near 0.8); trimming leaves exactly one span per edge, anchored at the
    untouched end, that overshoots the true end by 2.5, 5.6, 4.7 and 3.7 samples at 1 px and by 5.5, 8.6, 7.7 and 5.7 at 2 px
    (a sample is a quarter of a pixel).  The caps, 12 and 16 samples, are (tolerance + sqrt(2) px) / 0.25 px = 9.7 and
    13.7, rounded up for foreshortening."""
    edge_dict, true, at_end = C.extended_edges()
    cams, maps = DC.dir_novel_cameras()
    for tol in (1, 2):
        verdict = SP.edge_support(edge_dict, cams, maps, "PidiNet", resolution=EC.SCAN_RESOLUTION, keep_tolerance_px=tol,
                                  min_visible=0.5, min_near=0.8, frames_ratio=C.SCAN_FRAMES_RATIO, backend="host")
        t = verdict["settings"]["tolerances_px"].index(float(tol))
        r = C.scan_trim("extended", "host", tol)
        n = np.diff(r["offsets"].astype(np.int64))
        err = C.cut_errors(r) if all(len(s) == 1 for s in r["spans"]) else None
        print(f"{tol} px: the verdict keeps {verdict['kept'].tolist()} (pooled share {np.round(verdict['share'][:, t], 4).tolist()}); "
              f"samples {n.tolist()}, spans {r['spans']}, cut errors in samples {None if err is None else np.round(err, 2).tolist()}")
        assert not verdict["kept"].all(), "the per-edge verdict drops at least one over-extended edge whole"
        assert [len(s) for s in r["spans"]] == [1, 1, 1, 1] and r["source"].tolist() == [0, 1, 2, 3]
        for e, ((a, b),) in enumerate(r["spans"]):
            assert (a == 0) if at_end[e] else (b == n[e] - 1), "the run reaches the untouched end"
        assert (np.abs(err) <= C.CUT_CAP[tol]).all()
        assert len(r["edge_dict"]["curves_ctl_pts"]) == 1 and len(r["edge_dict"]["lines_end_pts"]) == 3
        assert r["settings"]["views"] == DC.DIR_VIEWS and r["settings"]["points"] == n.sum() == len(r["tally"])
        # the pieces end where the spans say: the untouched end of a line is the input's, bit for bit
        lines = np.array(r["edge_dict"]["lines_end_pts"]).reshape(3, 2, 3)
        given = np.array(edge_dict["lines_end_pts"]).reshape(3, 2, 3)
        assert np.array_equal(lines[0, 0], given[0, 0]) and np.array_equal(lines[2, 0], given[2, 0])
        assert np.abs(lines[1, 1] - given[1, 1]).max() <= 1e-15


def test_the_drawn_edges_come_back_whole():
    for tol in (1, 2):
        for gap, span in ((0, 2), (ET.MAX_GAP, ET.MIN_SPAN)):
            r = C.scan_trim("drawn", "host", tol, None, gap, span)
            n = np.diff(r["offsets"].astype(np.int64))
            assert r["spans"] == [[(0, int(k) - 1)] for k in n]
            assert np.array_equal(np.array(r["edge_dict"]["curves_ctl_pts"]).reshape(-1, 12),
                                  np.array(EC.SCAN_EDGES["curves_ctl_pts"]))
            assert np.array_equal(np.array(r["edge_dict"]["lines_end_pts"]), np.array(EC.SCAN_EDGES["lines_end_pts"]))
            assert np.array(r["edge_dict"]["curves_ctl_pts"]).shape == (1, 4, 3)


def test_what_survives_of_a_bogus_chord_runs_along_a_drawn_edge():
    """The 72 bogus chords of edge_support_cases.scan_edges at 1 px: 1562 of their 11727 samples are supported, and none of
    them lies further than 0.0380 from a drawn sample in 3D (ALONG, the bound of edge_support_cases for "runs along a drawn
    edge", is 0.03; at 2 px the worst is 0.195, a ghost).  The cap is 0.04."""
    edge_dict, drawn = SC.scan_edges()
    r = C.scan_trim("bogus", "host", 1)
    flags = ET.supported_samples(r["tally"], DC.DIR_VIEWS, C.SCAN_FRAMES_RATIO)[:, 0]
    pts, off = SP.sample_edges(edge_dict["curves_ctl_pts"], edge_dict["lines_end_pts"], EC.SCAN_RESOLUTION)
    assert np.array_equal(off, r["offsets"])
    bogus = np.repeat(~drawn, np.diff(off))
    kept = pts[bogus & flags].astype(np.float64)
    s = DC.dir_samples()[0]
    far = np.sqrt(((kept[:, None, :] - s[None, :, :]) ** 2).sum(-1).min(1))
    print(f"{len(kept)} of {bogus.sum()} samples of the bogus edges are supported; the worst lies {far.max():.4f} from a drawn "
          f"sample")
    assert 0 < len(kept) < bogus.sum() // 4 and flags[~bogus].all(), "every sample of a drawn edge is supported"
    assert far.max() <= 0.04


def test_chunking_the_views_changes_nothing():
    whole = C.scan_trim("extended", "host", 1)
    one = C.scan_trim("extended", "host", 1, 1)   # one view at a time
    five = C.scan_trim("extended", "host", 1, 5 * ET.BYTES_PER_PIXEL * DC.DIR_H * DC.DIR_W)   # 5 + 5 + 2 views
    for part in (one, five):
        assert torch.equal(part["tally"], whole["tally"]) and part["spans"] == whole["spans"]
        assert part["edge_dict"] == whole["edge_dict"]
    assert whole["tally"].dtype == torch.int32 and int(whole["tally"][:, 0].max()) == DC.DIR_VIEWS
    cams, maps = DC.dir_novel_cameras()
    with pytest.raises(ValueError, match="edge maps"):
        ET.trim_edges(EC.SCAN_EDGES, cams, maps[:-1], "PidiNet", backend="host")
    with pytest.raises(ValueError, match="min_span"):
        ET.trim_edges(EC.SCAN_EDGES, cams, maps, "PidiNet", min_span=1, backend="host")
    with pytest.raises(ValueError, match="Unknown detector"):
        ET.trim_edges(EC.SCAN_EDGES, cams, maps, "HED", backend="host")


# ------------------------------------------------------------------------------------------------ files
def test_the_command_line_writes_the_two_files(tmp_path, capsys):
    from curve_gaussian_amd.edge_extraction import support as S
    base, data = SC.write_support_scan(tmp_path)
    room = os.path.join(base, "room")
    pred = os.path.join(room, "parametric_edges.json")
    with open(pred, "w") as f:
        json.dump(C.extended_edges()[0], f)
    before = open(pred, "rb").read()
    argv = ["--base_dir", base, "--dataset_dir", data, "--detector", "PidiNet", "--backend", "host", "--frames_ratio", "0.5",
            "--sample_resolution", str(EC.SCAN_RESOLUTION), "--min_visible", "0.5", "--keep_tolerance", "1"]
    assert S.main(argv) == 0
    plain = open(os.path.join(room, S.SUPPORT_FILE), "rb").read()
    assert sorted(os.listdir(room)) == [S.SUPPORT_FILE, "parametric_edges.json"] and "trimmed" not in capsys.readouterr().out
    assert S.main(argv + ["--trim", "--trim_max_gap", "0", "--trim_min_span", "2"]) == 0
    want = C.scan_trim("extended", "host", 1)
    n = np.diff(want["offsets"].astype(np.int64))
    kept = sum(b - a + 1 for s in want["spans"] for a, b in s)
    assert f"room: views 12, edges 4, kept 1; trimmed to 4 pieces, {kept} of {n.sum()} samples" in capsys.readouterr().out
    assert sorted(os.listdir(room)) == [S.SUPPORT_FILE, S.TRIM_FILE, "parametric_edges.json", S.TRIMMED_FILE]
    assert open(pred, "rb").read() == before and open(os.path.join(room, S.SUPPORT_FILE), "rb").read() == plain
    assert json.load(open(os.path.join(room, S.TRIMMED_FILE))) == want["edge_dict"]
    out = json.load(open(os.path.join(room, S.TRIM_FILE)))
    assert out["scan"] == "room" and out["total"] == 4 and out["pieces"] == 4
    assert out["samples"] == n.sum() and out["kept_samples"] == kept
    assert out["settings"] == {**want["settings"], "layout": "emap", "undistort": False}
    assert out["settings"]["tolerance_px"] == 1.0 and out["settings"]["max_gap"] == 0 and out["settings"]["min_span"] == 2
    for e, rec in enumerate(out["edges"]):
        assert sorted(rec) == ["index", "kept_share", "kind", "samples", "spans"]
        assert rec["kind"] == ("curve" if e < 1 else "line") and rec["index"] == (e if e < 1 else e - 1)
        assert rec["samples"] == n[e] and rec["spans"] == [list(s) for s in want["spans"][e]]
        assert rec["kept_share"] == (want["spans"][e][0][1] - want["spans"][e][0][0] + 1) / n[e]
    # the defaults; an edge that nothing sees and one without samples have no span
    far = {"curves_ctl_pts": [], "lines_end_pts": [[50, 50, 50, 50, 50, 51], [0.5, 0.5, 0.5, 0.5, 0.5, 0.501]]}
    with open(pred, "w") as f:
        json.dump(far, f)
    assert S.main(argv + ["--trim"]) == 0
    out = json.load(open(os.path.join(room, S.TRIM_FILE)))
    assert [r["spans"] for r in out["edges"]] == [[], []] and [r["kept_share"] for r in out["edges"]] == [0.0, None]
    assert out["settings"]["max_gap"] == ET.MAX_GAP == 3 and out["settings"]["min_span"] == ET.MIN_SPAN == 10
    assert out["pieces"] == 0 and json.load(open(os.path.join(room, S.TRIMMED_FILE))) == {"curves_ctl_pts": [],
                                                                                          "lines_end_pts": []}


class _Model:
    """What write_parametric_edges reads of a model."""

    def __init__(self, curve_points, is_bezier):
        self.get_curve_points, self.is_bezier = curve_points, is_bezier


def test_the_export_with_the_flag_adds_two_files(tmp_path, capsys):
    from curve_gaussian_amd.edge_extraction import support as S
    from curve_gaussian_amd.scene import dataset_io as IO
    edge_dict = C.extended_edges()[0]
    curves = np.array(edge_dict["curves_ctl_pts"]).reshape(-1, 4, 3)
    lines = np.array(edge_dict["lines_end_pts"]).reshape(-1, 2, 3)
    as_curves = np.stack([lines[:, 0], lines[:, 0], lines[:, 1], lines[:, 1]], 1)   # a line is its first and last point
    model = _Model(torch.from_numpy(np.concatenate([curves, as_curves])), torch.tensor([True] + [False] * 3))
    cams, maps = DC.dir_novel_cameras()
    plain, flagged = tmp_path / "plain", tmp_path / "flagged"
    IO.write_parametric_edges(model, str(plain))
    capsys.readouterr()
    options = dict(resolution=EC.SCAN_RESOLUTION, frames_ratio=0.5, max_gap=0, min_span=2, backend="host")
    d, _ = IO.write_parametric_edges(model, str(flagged), detector="PidiNet", trim=True, trim_options=options, cameras=cams,
                                     edge_maps=maps)
    assert "before trimming:  4 edges, after trimming:  4 pieces" in capsys.readouterr().out
    assert sorted(os.listdir(plain)) == ["edge_points.ply", "parametric_edges.json"]
    assert sorted(os.listdir(flagged)) == ["edge_points.ply", S.TRIM_FILE, "parametric_edges.json", S.TRIMMED_FILE]
    for name in ("parametric_edges.json", "edge_points.ply"):
        assert open(flagged / name, "rb").read() == open(plain / name, "rb").read(), name
    assert json.load(open(flagged / S.TRIMMED_FILE)) == C.scan_trim("extended", "host", 1)["edge_dict"]
    assert json.load(open(flagged / "parametric_edges.json")) == d
    with pytest.raises(ValueError, match="cameras"):
        IO.write_parametric_edges(model, str(tmp_path / "none"), trim=True)


def test_the_driver_parses_the_options():
    import inspect

    from curve_gaussian_amd import train as T
    _, _, args = T.parse_args(["-s", "scan", "-m", "out", "--trim_edges", "--trim_tol_px", "1.5", "--trim_max_gap", "2",
                               "--trim_min_span", "6", "--thin_edge_maps"])
    assert args.trim_edges and not args.support_check
    assert T.trim_options(args) == {"tolerance_px": 1.5, "max_gap": 2, "min_span": 6, "thin": True}
    assert set(T.trim_options(args)) <= set(inspect.signature(ET.trim_edges).parameters)
    _, _, args = T.parse_args(["-s", "scan", "-m", "out"])
    assert not args.trim_edges and T.trim_options(args) == {}


# ------------------------------------------------------------------------------------------------ the C ABI
def test_abi_argument_checks_are_pinned():
    """Status and the exact text of cgs_last_error() for every rejection of cgs_sample_support; the pointers are dummies
    that are never dereferenced, and no row passes validation with work to do."""
    from curve_gaussian_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(64)
    fn = "cgs_sample_support: invalid argument "

    def call(P=5, points=p, V=2, intr=p, w2c=p, H=4, W=6, d2=p, T=1, tol2=p, tally=p):
        return lib.cgs_sample_support(P, points, V, intr, w2c, H, W, d2, T, tol2, tally, None)

    rows = [(dict(P=-1), "(P=-1, V=2, T=1; T lies in [1, 4])"), (dict(V=-1), "(P=5, V=-1, T=1; T lies in [1, 4])"),
            (dict(T=0), "(P=5, V=2, T=0; T lies in [1, 4])"), (dict(T=5), "(P=5, V=2, T=5; T lies in [1, 4])"),
            (dict(T=-1, H=0), "(P=5, V=2, T=-1; T lies in [1, 4])"),
            (dict(P=0, T=0), "(P=0, V=2, T=0; T lies in [1, 4])"),
            (dict(H=0), "(height=0, width=6; sizes lie in [1, 16384])"),
            (dict(H=16385), "(height=16385, width=6; sizes lie in [1, 16384])"),
            (dict(W=0), "(height=4, width=0; sizes lie in [1, 16384])"),
            (dict(W=-3, points=None), "(height=4, width=-3; sizes lie in [1, 16384])"),
            (dict(V=0, W=16385), "(height=4, width=16385; sizes lie in [1, 16384])")]
    rows += [({name: None}, "(NULL pointer; P=5, V=2)") for name in ("points", "intr", "w2c", "d2", "tol2", "tally")]
    rows += [(dict(P=0, intr=None), "(NULL pointer; P=0, V=2)"), (dict(V=0, tol2=None), "(NULL pointer; P=5, V=0)"),
             (dict(V=0, tally=None), "(NULL pointer; P=5, V=0)")]
    for kw, text in rows:
        assert call(**kw) == -1 and lib.cgs_last_error().decode() == fn + text, kw
    for kw in (dict(P=0), dict(V=0), dict(P=0, points=None, tally=None), dict(P=0, V=0, points=None, tally=None)):
        assert call(**kw) == 0, "no sample or no view leaves nothing to add"
    assert _lib.SIGNATURES["cgs_sample_support"][1] == [ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                                                        ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                                        ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
