"""Host: snapping extracted edges onto the detected edges (ops.edge_snap: snap_terms, snap_step, refit, snap_edges) on the
numpy back end -- the terms against the brute-force definition bit for bit, chunked calls, the drawn scan perturbed by a
pixel, the gate, the guard, shared ends, the files of the chain with and without the option, and the C ABI's argument
checks."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import edge_dir_cases as DC
import edge_score_cases as EC
import edge_snap_cases as C
import edge_support_cases as SC
from curve_gaussian_amd.ops import edge_snap as SN
from curve_gaussian_amd.ops import edge_support as SP


# ------------------------------------------------------------------------------------------------ the terms
@pytest.mark.parametrize("capture_px", C.CAPTURES)
@pytest.mark.parametrize("plane", C.PLANES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_terms_equal_the_brute_force_bit_for_bit(plane, capture_px):
    H, W = plane
    pts, K, M, d2, cap2, want = C.kernel_case(257, 5, H, W, capture_px)
    terms, views = SN.snap_terms(pts.copy(), K, M, d2.copy(), capture_px, backend="host")
    assert terms.dtype == torch.float64 and tuple(terms.shape) == (257, 10) and views.dtype == torch.int32
    assert C.same_bits((terms, views), want)
    if H < 2 or W < 2:
        assert not want[1].any(), "a plane without a 2 x 2 footprint never contributes"
    else:
        assert want[1].any() and (want[1] == 0).any(), "the case must both capture and skip"


def test_the_special_samples_do_what_they_are_there_for():
    """On the identity camera of the 37x70 plane with a transform of zeros and ones: exact-integer footprints take their
    value from one pixel, the samples within half a pixel of a border are skipped, the first pixel of the last footprint
    is kept."""
    H, W = 37, 70
    pts = C.snap_points(257, H, W)[C.SPECIAL:C.SPECIAL + 9]
    K, M = C.snap_cameras(1, H, W)
    d2 = np.zeros((1, H, W), np.int32)
    d2[0, 1, 1], d2[0, 2, 2] = 1, 4
    terms, views = (x.numpy() for x in SN.snap_terms(pts, K, M, d2, 2, backend="host"))
    assert views.tolist() == [1, 1, 1, 1, 0, 0, 0, 0, 1]
    assert terms[2, 9] == 1.0, "u - 0.5 = v - 0.5 = 1 exactly: r is the distance of pixel (1, 1) alone"
    assert 0.0 < terms[0, 9] < 1.0 and 0.0 < terms[1, 9] < 1.0 and terms[8, 9] == 0.0
    assert SN.snap_terms(pts, K, M, d2, 1, backend="host")[1].tolist() == [1, 1, 0, 1, 0, 0, 0, 0, 1], "d2 = 4 is past a capture of 1"


def test_an_all_infinite_plane_contributes_nothing():
    pts, K, M, d2, cap2, want = C.kernel_case(257, 2, 37, 70, 8, "inf")
    assert not want[1].any() and not want[0].any()
    assert C.same_bits(SN.snap_terms(pts.copy(), K, M, d2.copy(), 8, backend="host"), want)


def test_chunks_of_views_add_up_to_the_bits_of_one_call():
    pts, K, M, d2, cap2, want = C.kernel_case(257, 5, 37, 70, 3)
    pts, d2 = pts.copy(), d2.copy()
    out = (torch.zeros((257, 10), dtype=torch.float64), torch.zeros((257,), dtype=torch.int32))
    got = SN.snap_terms(pts, K[0:2], M[0:2], d2[0:2], 3, backend="host", out=out)
    assert got[0] is out[0] and got[1] is out[1]
    SN.snap_terms(pts, K[2:5], M[2:5], d2[2:5], 3, backend="host", out=out)
    assert C.same_bits(out, want)
    # a non-zero pair handed in is added to
    rng = np.random.default_rng(5)
    start = (rng.normal(size=(257, 10)), rng.integers(0, 9, 257).astype(np.int32))
    out = (torch.from_numpy(start[0].copy()), torch.from_numpy(start[1].copy()))
    SN.snap_terms(pts, K[:1], M[:1], d2[:1], 3, backend="host", out=out)
    one = C.snap_terms_brute(pts, K[:1], M[:1], d2[:1], cap2)
    assert np.array_equal(out[0].numpy().view(np.int64), (start[0] + one[0]).view(np.int64)), "one add per row and view"
    assert np.array_equal(out[1].numpy(), start[1] + one[1]) and one[1].any()


def test_no_sample_and_no_view():
    K, M = C.snap_cameras(2, 5, 33)
    d2 = C.snap_d2(2, 5, 33, 9)
    terms, views = SN.snap_terms(np.zeros((0, 3), np.float32), K, M, d2, 3, backend="host")
    assert tuple(terms.shape) == (0, 10) and tuple(views.shape) == (0,)
    terms, views = SN.snap_terms(C.snap_points(9, 5, 33), K[:0], M[:0], d2[:0], 3, backend="host")
    assert not terms.any() and not views.any()


def test_argument_errors():
    pts, K, M, d2, cap2, _ = C.kernel_case(65, 2, 37, 70, 3)
    pts, d2 = pts.copy(), d2.copy()
    for bad in (0, 0.9, 8.1, 9, -1, float("nan")):
        with pytest.raises(ValueError, match="capture_px must lie in"):
            SN.snap_terms(pts, K, M, d2, bad, backend="host")
    assert [SN.capture_squared(c) for c in (1, 1.5, 3, 8)] == [1, 2, 9, 64]
    assert np.array_equal(SN.distance_table(4), [0.0, 1.0, np.sqrt(2.0), np.sqrt(3.0), 2.0])
    with pytest.raises(ValueError, match="unknown edge support backend"):
        SN.snap_terms(pts, K, M, d2, 3, backend="cuda")
    with pytest.raises(ValueError, match="points must be float32"):
        SN.snap_terms(pts.astype(np.float64), K, M, d2, 3, backend="host")
    with pytest.raises(ValueError, match="d2 must be int32"):
        SN.snap_terms(pts, K, M, d2.astype(np.int64), 3, backend="host")
    with pytest.raises(ValueError, match="d2 must be"):
        SN.snap_terms(pts, K, M, d2[:1], 3, backend="host")
    good = (torch.zeros((65, 10), dtype=torch.float64), torch.zeros((65,), dtype=torch.int32))
    for out in (good[0], (good[0], good[1].long()), (good[0].float(), good[1]), (good[0][:, :9], good[1]),
                (good[0][:64], good[1]), (good[0].numpy(), good[1]), (good[0].t().contiguous().t(), good[1])):
        with pytest.raises(ValueError, match="snap_terms: out must be"):
            SN.snap_terms(pts, K, M, d2, 3, backend="host", out=out)
    with pytest.raises(SN.L.CurveGSError, match="d2"):
        SN.snap_terms(pts, K, M, d2, 3, backend="gpu")   # a host transform
    with pytest.raises(ValueError, match="frames_ratio"):
        SN.snap_step(np.zeros((2, 3)), np.zeros((2, 10)), np.zeros(2, np.int32), 12, frames_ratio=1.5)
    with pytest.raises(ValueError, match="damping"):
        SN.snap_step(np.zeros((2, 3)), np.zeros((2, 10)), np.zeros(2, np.int32), 12, damping=0.0)
    with pytest.raises(ValueError, match="snap_step: samples"):
        SN.snap_step(np.zeros((2, 3)), np.zeros((3, 10)), np.zeros(2, np.int32), 12)
    cams, maps = DC.dir_novel_cameras()
    for kw, text in ((dict(iterations=-1), "iterations"), (dict(capture_px=9), "capture_px"), (dict(min_constrained=1.5), "min_constrained"),
                     (dict(step_cap=0.0), "step_cap"), (dict(resolution=0.0), "resolution"), (dict(budget_bytes=0), "budget_bytes"),
                     (dict(backend="cuda"), "backend")):
        with pytest.raises(ValueError, match=text):
            SN.snap_edges(EC.SCAN_EDGES, cams, maps, "PidiNet", **{"backend": "host", **kw})
    with pytest.raises(ValueError, match="12 cameras and 11 edge maps"):
        SN.snap_edges(EC.SCAN_EDGES, cams, maps[:-1], "PidiNet", backend="host")


# ------------------------------------------------------------------------------------------------ step and refit
def test_the_step_solves_the_damped_equations_and_holds_the_rest():
    g = np.array([[1.0, 0.0, 0.0], [0.0, 2.0, 0.0]])
    r = np.array([0.5, 0.25])
    A, b = g.T @ g, g.T @ r
    row = np.array([A[0, 0], A[0, 1], A[0, 2], A[1, 1], A[1, 2], A[2, 2], b[0], b[1], b[2], (r * r).sum()])
    terms = np.stack([row, row, np.zeros(10), row * 100.0])
    views = np.array([7, 6, 7, 7], np.int32)
    delta, con = SN.snap_step(np.zeros((4, 3)), terms, views, 12, frames_ratio=0.5, damping=1e-2, step_cap=None)
    assert con.tolist() == [True, False, True, True], "more than ceil(0.5 * 12) = 6 views"
    lam = 1e-2 * 5.0 / 3.0
    assert np.allclose(delta[0], [-0.5 / (1 + lam), -0.5 / (4 + lam), 0.0], rtol=1e-14, atol=0) and delta[0, 2] == 0.0
    assert not delta[1].any() and not delta[2].any(), "unconstrained, and constrained without a gradient"
    capped, _ = SN.snap_step(np.zeros((4, 3)), terms, views, 12, frames_ratio=0.5, step_cap=0.1)
    assert np.isclose(np.linalg.norm(capped[0]), 0.1) and np.allclose(capped[0] / 0.1, delta[0] / np.linalg.norm(delta[0]))


def test_the_refit_moves_control_points_and_a_line_stays_a_line():
    c, l = C.drawn_arrays()
    pts, off = SP.sample_edges(c, l, EC.SCAN_RESOLUTION)
    shift = np.array([0.01, -0.02, 0.005])
    delta = np.tile(shift, (len(pts), 1))
    nc, nl = SN.refit(c, l, off, delta)
    assert np.allclose(nc, c + shift, atol=1e-12) and np.allclose(nl, l + shift, atol=1e-12)
    only, same = SN.refit(c, l, off, delta, edges=np.array([False, True, False, False]))
    assert only.tobytes() == c.tobytes() and same[1:].tobytes() == l[1:].tobytes() and np.allclose(same[0], l[0] + shift)
    rng = np.random.default_rng(1)
    nc, nl = SN.refit(c, l, off, rng.normal(0.0, 0.01, (len(pts), 3)))
    assert nl.shape == (3, 2, 3), "two end points per line whatever the steps: a line comes back as a line"
    with pytest.raises(ValueError, match="refit"):
        SN.refit(c, l, off[:-1], delta[:off[-2]])


# ------------------------------------------------------------------------------------------------ the drawn scan
def test_the_perturbed_scan_comes_back_onto_the_drawn_edges():
    """Four drawn edges, sigma = 1 px on every control point, seed C.SEED.  Mean distance of an edge's samples to its drawn
    edge, host run of this implementation: before 0.0059 0.0106 0.0113 0.0089, after 0.00102 0.00309 0.00420 0.00028 (the two
    lines that share a corner keep the along-edge part of their perturbation: a snap does not change an edge's length)."""
    given = C.perturbed_edges()
    res = C.scan_snap("perturbed")
    before, after = C.distance_to_drawn(given), C.distance_to_drawn(res["edge_dict"])
    print("before", before, "after", after, [(r["constrained_share"], r["rms_before"], r["rms_after"]) for r in res["edges"]])
    assert all(r["constrained_share"] >= 0.8 and r["moved"] and r["reason"] == "snapped" for r in res["edges"]), "the gate"
    assert (after < before).all()
    assert (after < np.array(C.AFTER_BOUND)).all()
    assert all(r["rms_after"] < r["rms_before"] for r in res["edges"])
    assert [r["kind"] for r in res["edges"]] == ["curve", "line", "line", "line"] and res["moved"].all()
    s = res["settings"]
    assert (s["views"], s["chunks"], s["capture_px"], s["iterations"], s["step_cap"]) == (12, 1, 3.0, 5, 4 * EC.SCAN_RESOLUTION)


def test_the_drawn_edges_stay_within_a_sample_spacing():
    res = C.scan_snap("drawn")
    moved = [r["mean_displacement"] for r in res["edges"]]
    print("mean displacement of the unperturbed edges", moved)
    assert all(m < EC.SCAN_RESOLUTION for m in moved)
    assert (C.distance_to_drawn(res["edge_dict"]) < EC.SCAN_RESOLUTION).all()


def test_chunked_views_give_the_same_edges():
    one = C.scan_snap("perturbed")
    many = C.scan_snap("perturbed", budget_bytes=1)   # one view per chunk: the transform is recomputed in every pass
    assert many["settings"]["chunks"] == 12 and one["settings"]["chunks"] == 1
    assert many["edge_dict"] == one["edge_dict"] and many["edges"] == one["edges"]


def test_an_edge_off_the_drawn_edges_comes_back_bit_for_bit():
    given = C.shifted_edge()
    res = C.scan_snap("shifted")
    assert res["edge_dict"] == given and not res["moved"].any()
    r = res["edges"][0]
    assert r["moved"] is False and r["reason"].startswith("gate:") and r["constrained_share"] < 0.8
    assert r["mean_displacement"] == 0.0 and r["max_displacement"] == 0.0 and r["rms_after"] is None


def test_the_guard_returns_an_edge_whose_residual_did_not_fall(monkeypatch):
    """A step in the wrong direction (the sign of the solve flipped) drives every edge off the detected edges: the residual
    rises, or the constraint is lost, and the guard hands the edges back bit for bit."""
    step = SN.snap_step
    monkeypatch.setattr(SN, "snap_step", lambda *a, **k: (lambda d, c: (-d, c))(*step(*a, **k)))
    cams, maps = DC.dir_novel_cameras()
    res = SN.snap_edges(EC.SCAN_EDGES, cams, maps, "PidiNet", resolution=EC.SCAN_RESOLUTION, frames_ratio=C.SCAN_FRAMES_RATIO,
                        backend="host", iterations=2)
    c, l = C.drawn_arrays()
    assert res["edge_dict"] == {"curves_ctl_pts": c.tolist(), "lines_end_pts": l.reshape(-1, 6).tolist()}
    assert all(r["reason"].startswith("guard:") and not r["moved"] and r["constrained_share"] >= 0.8 for r in res["edges"])


def test_an_edge_too_short_to_have_two_samples_and_no_iteration():
    cams, maps = DC.dir_novel_cameras()
    tiny = {"curves_ctl_pts": [], "lines_end_pts": [[0.2, 0.2, 0.2, 0.2 + 1.5 * EC.SCAN_RESOLUTION, 0.2, 0.2],
                                                     [0.2, 0.2, 0.2, 0.2 + 0.5 * EC.SCAN_RESOLUTION, 0.2, 0.2]]}
    res = SN.snap_edges(tiny, cams, maps, "PidiNet", resolution=EC.SCAN_RESOLUTION, frames_ratio=0.5, backend="host")
    assert res["edge_dict"] == tiny and [r["samples"] for r in res["edges"]] == [1, 0]
    assert all(r["reason"] == "fewer than two samples" for r in res["edges"])
    none = C.scan_snap("perturbed", iterations=0)
    assert none["edge_dict"]["lines_end_pts"] == C.perturbed_edges()["lines_end_pts"] and not none["moved"].any()
    empty = SN.snap_edges({"curves_ctl_pts": [], "lines_end_pts": []}, cams, maps, "PidiNet", backend="host")
    assert empty["edge_dict"] == {"curves_ctl_pts": [], "lines_end_pts": []} and empty["edges"] == []


def test_shared_ends_stay_shared():
    given = C.perturbed_edges()
    l0 = np.asarray(given["lines_end_pts"])
    assert l0[0, 3:].tobytes() == l0[1, :3].tobytes(), "the perturbed scan keeps the drawn corner"
    l = np.asarray(C.scan_snap("perturbed")["edge_dict"]["lines_end_pts"])
    assert l[0, 3:].tobytes() == l[1, :3].tobytes() and l[0, 3:].tobytes() != l0[0, 3:].tobytes()
    # a member that comes back unchanged holds the corner where it was
    cams, maps = DC.dir_novel_cameras()
    far = C.shifted_edge()["lines_end_pts"][0]
    mixed = {"curves_ctl_pts": [], "lines_end_pts": [given["lines_end_pts"][0], list(l0[0, 3:]) + far[3:]]}
    res = SN.snap_edges(mixed, cams, maps, "PidiNet", resolution=EC.SCAN_RESOLUTION, frames_ratio=0.5, backend="host")
    assert res["moved"].tolist() == [True, False]
    out = np.asarray(res["edge_dict"]["lines_end_pts"])
    assert out[1].tobytes() == np.asarray(mixed["lines_end_pts"][1]).tobytes()
    assert out[0, 3:].tobytes() == l0[0, 3:].tobytes() and out[0, :3].tobytes() != l0[0, :3].tobytes()


# ------------------------------------------------------------------------------------------------ files
def _listing(room):
    return {name: open(os.path.join(room, name), "rb").read() for name in sorted(os.listdir(room))}


def test_the_command_line_with_and_without_the_option(tmp_path, capsys):
    from curve_gaussian_amd.edge_extraction import support as S
    base, data = SC.write_support_scan(tmp_path)
    room = os.path.join(base, "room")
    with open(os.path.join(room, "parametric_edges.json"), "w") as f:
        json.dump(C.perturbed_edges(), f)
    given = open(os.path.join(room, "parametric_edges.json"), "rb").read()
    argv = ["--base_dir", base, "--dataset_dir", data, "--detector", "PidiNet", "--backend", "host", "--frames_ratio", "0.5",
            "--sample_resolution", str(EC.SCAN_RESOLUTION), "--trim", "--dedupe", "--join"]
    assert S.main(argv) == 0
    plain = _listing(room)
    plain_line = capsys.readouterr().out
    assert S.SNAP_FILE not in plain and S.SNAPPED_FILE not in plain and "snapped" not in plain_line
    assert "input" not in json.loads(plain[S.SUPPORT_FILE]) and "input" not in json.loads(plain[S.TRIM_FILE])
    assert S.main(argv + ["--snap"]) == 0
    line = capsys.readouterr().out
    snapped = _listing(room)
    assert sorted(snapped) == sorted(list(plain) + [S.SNAP_FILE, S.SNAPPED_FILE]) and snapped["parametric_edges.json"] == given
    assert "; snapped 4 of 4 edges first" in line
    from curve_gaussian_amd.edge_extraction.reprojection import emap_cameras
    cams, maps = emap_cameras(os.path.join(data, "room"), "PidiNet")   # the cameras as the scan's files round them
    want = SN.snap_edges(C.perturbed_edges(), cams, maps, "PidiNet", resolution=EC.SCAN_RESOLUTION, frames_ratio=0.5, backend="host")
    assert json.loads(snapped[S.SNAPPED_FILE]) == want["edge_dict"]
    record = json.loads(snapped[S.SNAP_FILE])
    assert record["input"] == "parametric_edges.json" and record["scan"] == "room" and record["moved"] == 4 and record["total"] == 4
    assert record["edges"] == want["edges"] and record["settings"]["capture_px"] == 3.0
    assert json.loads(snapped[S.SUPPORT_FILE])["input"] == S.SNAPPED_FILE
    assert json.loads(snapped[S.TRIM_FILE])["input"] == S.SNAPPED_FILE
    assert json.loads(snapped[S.DEDUPE_FILE])["input"] == S.TRIMMED_FILE
    # without trimming the deduping names the snapped file, and without either so does the joining
    assert S.main(argv[:-3] + ["--dedupe", "--snap", "--snap_capture", "2", "--snap_iterations", "1", "--snap_min_constrained", "0.5"]) == 0
    files = _listing(room)
    assert json.loads(files[S.DEDUPE_FILE])["input"] == S.SNAPPED_FILE
    s = json.loads(files[S.SNAP_FILE])["settings"]
    assert (s["capture_px"], s["iterations"], s["min_constrained"]) == (2.0, 1, 0.5)
    assert S.main(argv[:-3] + ["--join", "--snap"]) == 0
    assert json.loads(_listing(room)[S.GRAPH_FILE])["input"] == S.SNAPPED_FILE
    # a run that omits the option writes what the first run wrote, byte for byte
    for name in (S.SNAP_FILE, S.SNAPPED_FILE):
        os.remove(os.path.join(room, name))
    assert S.main(argv) == 0 and _listing(room) == plain


class _Model:
    """What write_parametric_edges reads of a model."""

    def __init__(self, curve_points, is_bezier):
        self.get_curve_points, self.is_bezier = curve_points, is_bezier


def test_the_export_with_and_without_the_option(tmp_path, capsys):
    from curve_gaussian_amd.edge_extraction import support as S
    from curve_gaussian_amd.scene import dataset_io as IO
    curves, lines = SP._edge_arrays(C.perturbed_edges()["curves_ctl_pts"], C.perturbed_edges()["lines_end_pts"])
    as_curves = np.stack([lines[:, 0], lines[:, 0], lines[:, 1], lines[:, 1]], 1)   # a line is its first and last point
    model = _Model(torch.from_numpy(np.concatenate([curves, as_curves])), torch.tensor([True] + [False] * 3))
    cams, maps = DC.dir_novel_cameras()
    options = dict(resolution=EC.SCAN_RESOLUTION, frames_ratio=0.5, backend="host")
    rest = dict(cameras=cams, edge_maps=maps, detector="PidiNet", support_checking=True, support_options=options, trim=True,
                trim_options=options, dedupe=True, dedupe_options=dict(resolution=EC.SCAN_RESOLUTION, backend="host"))
    plain, again, flagged = tmp_path / "plain", tmp_path / "again", tmp_path / "flagged"
    IO.write_parametric_edges(model, str(plain), **rest)
    IO.write_parametric_edges(model, str(again), snap=False, snap_options=options, **rest)
    assert _listing(plain) == _listing(again) and S.SNAP_FILE not in _listing(plain)
    capsys.readouterr()
    d, _ = IO.write_parametric_edges(model, str(flagged), snap=True, snap_options=options, **rest)
    assert "snapped:  4 of 4 edges moved" in capsys.readouterr().out
    files = _listing(flagged)
    assert sorted(files) == sorted(list(_listing(plain)) + [S.SNAP_FILE, S.SNAPPED_FILE])
    for name in ("parametric_edges.json", "edge_points.ply"):
        assert files[name] == _listing(plain)[name], name
    assert json.loads(files["parametric_edges.json"]) == d
    assert json.loads(files[S.SNAPPED_FILE]) == SN.snap_edges(d, cams, maps, "PidiNet", **options)["edge_dict"]
    assert json.loads(files[S.SNAP_FILE])["input"] == "parametric_edges.json"
    assert json.loads(files[S.SUPPORT_FILE])["input"] == S.SNAPPED_FILE and json.loads(files[S.TRIM_FILE])["input"] == S.SNAPPED_FILE
    with pytest.raises(ValueError, match="snap=True"):
        IO.write_parametric_edges(model, str(tmp_path / "bad"), snap=True)


def test_the_driver_parses_the_options_and_its_export_follows_them(tmp_path, capsys, monkeypatch):
    import inspect

    from curve_gaussian_amd import train as T
    from curve_gaussian_amd.edge_extraction import support as S
    _, _, args = T.parse_args(["-s", "scan", "-m", "out", "--snap_edges", "--snap_capture", "2", "--snap_iterations", "3",
                               "--snap_min_constrained", "0.7", "--thin_edge_maps"])
    assert T.snap_options(args) == {"capture_px": 2.0, "iterations": 3, "min_constrained": 0.7, "thin": True}
    assert set(T.snap_options(args)) <= set(inspect.signature(SN.snap_edges).parameters)
    _, _, args = T.parse_args(["-s", "scan", "-m", "out"])
    assert not args.snap_edges and T.snap_options(args) == {}
    # the export block, on the drawn cameras: the same files without the flag, two more and the new "input" with it
    cams, maps = DC.dir_novel_cameras()
    small = dict(resolution=EC.SCAN_RESOLUTION, frames_ratio=0.5, backend="host")   # the drawn scan's settings
    for module, fn in ((S.SN, "snap_edges"), (S.SP, "edge_support"), (S.ET, "trim_edges")):
        monkeypatch.setattr(module, fn, (lambda real: lambda *a, **k: real(*a, **{**small, **k}))(getattr(module, fn)))
    monkeypatch.setattr(S.EJ, "join_edges", (lambda real: lambda *a, **k: real(*a, **{"resolution": EC.SCAN_RESOLUTION,
                                                                                    "backend": "host", **k}))(S.EJ.join_edges))
    listings = {}
    for name, flags in (("plain", []), ("again", []), ("flagged", ["--snap_edges"])):
        model = tmp_path / name
        os.makedirs(model)
        with open(model / "parametric_edges.json", "w") as f:
            json.dump(C.perturbed_edges(), f)
        _, _, args = T.parse_args(["-s", "scan", "-m", str(model), "--trim_edges", "--join_edges", "--support_check"] + flags)
        T.export_checks(args, str(model), cams, "PidiNet", edge_maps=maps)
        listings[name] = _listing(model)
    capsys.readouterr()
    assert listings["plain"] == listings["again"] and S.SNAP_FILE not in listings["plain"]
    assert sorted(listings["flagged"]) == sorted(list(listings["plain"]) + [S.SNAP_FILE, S.SNAPPED_FILE])
    assert listings["flagged"]["parametric_edges.json"] == listings["plain"]["parametric_edges.json"]
    assert json.loads(listings["flagged"][S.TRIM_FILE])["input"] == S.SNAPPED_FILE
    assert json.loads(listings["flagged"][S.SUPPORT_FILE])["input"] == S.SNAPPED_FILE
    assert json.loads(listings["flagged"][S.GRAPH_FILE])["input"] == S.TRIMMED_FILE


# ------------------------------------------------------------------------------------------------ the C ABI
def test_abi_argument_checks_are_pinned():
    """Status and the exact text of cgs_last_error() for every rejection of cgs_sample_snap_terms; the pointers are dummies
    that are never dereferenced, and no row passes validation with work to do."""
    from curve_gaussian_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(1 << 20)
    head = "cgs_sample_snap_terms: invalid argument "

    def call(P=5, points=p, V=2, intr=p, w2c=p, H=4, W=6, d2=p, cap2=9, lut=p, terms=p, views=p):
        return lib.cgs_sample_snap_terms(P, points, V, intr, w2c, H, W, d2, cap2, lut, terms, views, None)

    rows = [(dict(P=-1), "(P=-1, V=2, cap2=9; cap2 lies in [1, 64])"),
            (dict(V=-1), "(P=5, V=-1, cap2=9; cap2 lies in [1, 64])"),
            (dict(cap2=0), "(P=5, V=2, cap2=0; cap2 lies in [1, 64])"),
            (dict(cap2=-3, H=0), "(P=5, V=2, cap2=-3; cap2 lies in [1, 64])"),
            (dict(cap2=65, lut=None), "(P=5, V=2, cap2=65; cap2 lies in [1, 64])"),
            (dict(P=0, cap2=65), "(P=0, V=2, cap2=65; cap2 lies in [1, 64])"),
            (dict(H=0), "(height=0, width=6; sizes lie in [1, 16384])"),
            (dict(H=16385), "(height=16385, width=6; sizes lie in [1, 16384])"),
            (dict(W=0, points=None), "(height=4, width=0; sizes lie in [1, 16384])"),
            (dict(V=0, W=16385), "(height=4, width=16385; sizes lie in [1, 16384])")]
    rows += [({name: None}, "(NULL pointer; P=5, V=2)") for name in ("points", "intr", "w2c", "d2", "lut", "terms", "views")]
    rows += [(dict(P=0, intr=None), "(NULL pointer; P=0, V=2)"), (dict(V=0, d2=None), "(NULL pointer; P=5, V=0)"),
             (dict(V=0, views=None), "(NULL pointer; P=5, V=0)"), (dict(P=0, V=0, lut=None), "(NULL pointer; P=0, V=0)")]
    for kw, text in rows:
        assert call(**kw) == -1 and lib.cgs_last_error().decode() == head + text, kw
    for kw in (dict(P=0), dict(V=0), dict(P=0, points=None, terms=None, views=None), dict(V=0, cap2=1), dict(V=0, cap2=64),
               dict(P=0, V=0, points=None, terms=None, views=None)):
        assert call(**kw) == 0, "no sample or no view leaves nothing to add"
    i, vp = ctypes.c_int, ctypes.c_void_p
    assert _lib.SIGNATURES["cgs_sample_snap_terms"] == (i, [i, vp, i, vp, vp, i, i, vp, i, vp, vp, vp, vp])


def test_the_constants_mirror_the_header():
    from curve_gaussian_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "curvegs.h")).read()
    for name, value in (("CGS_SNAP_MAX_CAP2", SN.MAX_CAP2), ("CGS_SNAP_TERMS", SN.TERMS)):
        assert f"#define {name} {value}\n" in header, name
    assert (SN.MAX_CAP2, SN.TERMS) == (_lib.SNAP_MAX_CAP2, _lib.SNAP_TERMS) == (64, 10)
    assert "int cgs_sample_snap_terms(int P, const float* points /*[P,3]*/, int V, const double* intr" in header
