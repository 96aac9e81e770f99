"""Host: the per-edge 2D support of ops.edge_support (sample_edges, support_counts, support_verdict, edge_support) on the
numpy back end -- the sampler against dataset_io's, the counts against a brute-force loop and a hand case, the verdict's
thresholds at their boundaries, the drawn scan with bogus chords, the command line, the export and the C ABI's argument
checks."""
import ctypes
import hashlib
import json
import os

import numpy as np
import pytest
import torch

import edge_dir_cases as DC
import edge_excl_cases as XC
import edge_score_cases as EC
import edge_support_cases as C
from curve_gaussian_amd.ops import edge_score as ES
from curve_gaussian_amd.ops import edge_support as SP
from curve_gaussian_amd.scene import dataset_io as IO


# ------------------------------------------------------------------------------------------------ the sampler
def test_sample_edges_equals_sample_edge_points():
    curves, lines = EC.SCAN_EDGES["curves_ctl_pts"], EC.SCAN_EDGES["lines_end_pts"]
    pts, off = SP.sample_edges(curves, lines, EC.SCAN_RESOLUTION)
    assert pts.dtype == np.float32 and off.dtype == np.int32 and off[0] == 0 and off[-1] == len(pts) and len(off) == 5
    assert np.array_equal(pts, IO.sample_edge_points(curves, lines, EC.SCAN_RESOLUTION))
    rng = np.random.default_rng(3)
    curves, lines = rng.uniform(0, 1, (9, 12)), rng.uniform(0, 1, (7, 6))
    for resolution in (0.005, 0.0371):
        pts, off = SP.sample_edges(curves, lines, resolution)
        assert np.array_equal(pts, IO.sample_edge_points(curves, lines, resolution))
        for e in range(16):   # every edge's own range is the sampler's result for that edge alone
            one = IO.sample_edge_points(curves[e:e + 1] if e < 9 else [], lines[e - 9:e - 8] if e >= 9 else [], resolution)
            assert np.array_equal(pts[off[e]:off[e + 1]], one), e


def test_an_edge_shorter_than_the_resolution_has_no_points():
    curves = [[0, 0, 0, 0.001, 0, 0, 0.002, 0, 0, 0.003, 0, 0], [0, 0, 0, 0.1, 0, 0, 0.2, 0, 0, 0.3, 0, 0]]
    lines = [[0, 0, 0, 0, 0.004, 0], [0, 0, 0, 0, 0.0101, 0], [1, 1, 1, 1, 1, 1]]
    pts, off = SP.sample_edges(curves, lines, 0.005)
    assert off.tolist() == [0, 0, 60, 60, 62, 62], "short curve, curve, short line, line of two samples, point"
    assert np.array_equal(pts, IO.sample_edge_points(curves, lines, 0.005))
    pts, off = SP.sample_edges([], [], 0.005)
    assert pts.shape == (0, 3) and off.tolist() == [0]


# ------------------------------------------------------------------------------------------------ the counts
@pytest.mark.parametrize("tol", C.TOLERANCES, ids=["T1", "T4"])
def test_counts_against_the_brute_force(tol):
    V, W = 5, 33
    K, M = C.support_cameras(V, W)
    d2 = C.support_d2(V, W)
    sizes = np.array([0, 1, 2, 63, 64, 65, 0, 130, 9, 0])
    pts, off = C.support_points(sizes, W)
    got = SP.support_counts(pts, off, K, M, d2, tol, backend="host")
    assert got.dtype == torch.int32 and tuple(got.shape) == (len(sizes), V, 1 + len(tol))
    want = C.counts_brute(pts, off, K, M, d2, ES.tolerances_squared(tol))
    assert np.array_equal(got.numpy(), want)
    seen = want[:, :, 0]
    assert 0 < seen.sum() < V * len(pts), "the case must hold points inside and outside the views"
    assert (want[:, :, 1:] <= seen[:, :, None]).all() and 0 < want[:, :, -1].sum() < seen.sum()
    assert not want[sizes == 0].any(), "an edge without points has a zero row"


def test_a_hand_case_under_the_identity_camera():
    """u = X / Z, v = Y / Z exactly; a 3 x 4 image whose transform is written out below."""
    K, M = XC.identity_camera()
    H, W = XC.HAND_H, XC.HAND_W
    d2 = np.array([[[0, 1, 4, 9], [1, 2, 5, 10], [4, 5, 8, EC.EDT_INF]]], np.int32)
    pts = np.array([
        # edge 0: pixels (0,0) d 0, (1,0) d 1, (2,1) d 5, (3,2) INF; then u = 4 = W (dropped) and a point behind
        [0.5, 0.5, 1.0], [3.0, 1.0, 2.0], [2.5, 1.5, 1.0], [7.0, 5.0, 2.0], [4.0, 1.0, 1.0], [1.0, 1.0, -1.0],
        # edge 2 (edge 1 is empty): u = 0 and v = 0 are kept, pixel (0,0); v = 3 = H is dropped; depth 0 is dropped
        [0.0, 0.0, 1.0], [1.0, 3.0, 1.0], [1.0, 1.0, 0.0],
        # edge 3: the last row and column, pixel (3,2) twice, and (1,1) d 2
        [3.999, 2.999, 1.0], [7.5, 5.5, 2.0], [1.5, 1.5, 1.0]], np.float32)
    off = np.array([0, 6, 6, 9, 12], np.int32)
    got = SP.support_counts(pts, off, K, M, d2, (0, 1, 2, 2.5), backend="host").numpy()
    # tolerances squared: 0, 1, 4, 6
    assert got.tolist() == [[[4, 1, 2, 2, 3]], [[0, 0, 0, 0, 0]], [[1, 1, 1, 1, 1]], [[3, 0, 0, 1, 1]]]
    assert np.array_equal(got, C.counts_brute(pts, off, K, M, d2, [0, 1, 4, 6]))
    none = SP.support_counts(pts, off, K[:0], M[:0], d2[:0], (1,), backend="host")
    assert tuple(none.shape) == (4, 0, 2)


def test_argument_errors():
    K, M = XC.identity_camera()
    d2 = np.zeros((1, 3, 4), np.int32)
    pts, off = np.zeros((2, 3), np.float32), np.array([0, 2], np.int32)
    call = lambda pts=pts, off=off, K=K, M=M, d2=d2, tol=(1,), **kw: SP.support_counts(pts, off, K, M, d2, tol,
                                                                                     **{"backend": "host", **kw})
    assert call().tolist() == [[[0, 0]]]
    with pytest.raises(ValueError, match="float32"):
        call(pts=pts.astype(np.float64))
    with pytest.raises(ValueError, match=r"\[P,3\]"):
        call(pts=np.zeros((2, 4), np.float32))
    for bad in ([0, 1], [1, 2], [0, 3, 2], [[0, 2]]):
        with pytest.raises(ValueError, match="offsets"):
            call(off=np.array(bad, np.int32))
    with pytest.raises(ValueError, match="offsets"):
        call(off=np.array([0.0, 2.0]))
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
    if not torch.cuda.is_available():
        from curve_gaussian_amd import _lib
        with pytest.raises(_lib.CurveGSError, match="GPU tensor"):
            call(backend="gpu")


class _OnGpu(torch.Tensor):
    """A CPU tensor that says it is on a GPU: what the placement checks ask, without a GPU."""
    is_cuda = property(lambda self: True)


def test_the_host_back_end_refuses_gpu_tensors_in_the_four_per_sample_operators():
    from curve_gaussian_amd.ops import edge_orient as OR
    from curve_gaussian_amd.ops import edge_snap as SN
    from curve_gaussian_amd.ops import edge_trim as ET
    K, M = XC.identity_camera()
    d2, near = np.zeros((1, 3, 4), np.int32), np.zeros((1, 3, 4), np.uint8)
    depth = np.full((1, 3, 4), np.inf, np.float32)
    pts, off, partner = np.zeros((2, 3), np.float32), np.array([0, 2], np.int32), np.array([1, 0], np.int32)
    gpu = lambda *shape, dtype=torch.int32: torch.zeros(shape, dtype=dtype).as_subclass(_OnGpu)
    cpu = lambda *shape, dtype=torch.int32: torch.zeros(shape, dtype=dtype)
    calls = {
        "support_counts": [lambda: SP.support_counts(gpu(2, 3, dtype=torch.float32), off, K, M, d2, (1,), backend="host"),
                           lambda: SP.support_counts(pts, off, K, M, gpu(1, 3, 4), (1,), backend="host", depth=depth)],
        "sample_tally": [lambda: ET.sample_tally(pts, K, M, d2, (1,), backend="host", out=gpu(2, 2)),
                         lambda: ET.sample_tally(pts, K, M, d2, (1,), backend="host", depth=depth, hidden_out=gpu(2)),
                         lambda: ET.sample_tally(gpu(2, 3, dtype=torch.float32), K, M, d2, (1,), backend="host")],
        "oriented_tally": [lambda: OR.oriented_tally(pts, partner, K, M, near, backend="host", out=gpu(2, 2)),
                           lambda: OR.oriented_tally(pts, partner, K, M, near, backend="host", depth=depth,
                                                     out=cpu(2, 2), hidden_out=gpu(2)),
                           lambda: OR.oriented_tally(pts, gpu(2), K, M, near, backend="host")],
        "snap_terms": [lambda: SN.snap_terms(pts, K, M, d2, 3, backend="host", out=(gpu(2, 10, dtype=torch.float64), cpu(2))),
                       lambda: SN.snap_terms(pts, K, M, d2, 3, backend="host", out=(cpu(2, 10, dtype=torch.float64), gpu(2))),
                       lambda: SN.snap_terms(pts, K, M, d2, 3, backend="host", depth=depth, hidden_out=gpu(2))],
    }
    for who, rows in calls.items():
        for row in rows:
            with pytest.raises(ValueError) as err:
                row()
            assert str(err.value) == f"{who}: backend='host' takes host arrays and CPU tensors"
    # the same calls with CPU tensors are taken
    assert ET.sample_tally(pts, K, M, d2, (1,), backend="host", out=cpu(2, 2)).shape == (2, 2)
    assert SN.snap_terms(pts, K, M, d2, 3, backend="host", out=(cpu(2, 10, dtype=torch.float64), cpu(2)))[1].shape == (2,)


# ------------------------------------------------------------------------------------------------ the verdict
def test_the_verdict_thresholds_at_their_boundaries():
    # one edge per row, V = 4 views, T = 1; n = 10 samples: sees iff seen >= ceil(0.5 * 10) = 5
    counts = np.zeros((6, 4, 2), np.int32)
    counts[0, :, 0], counts[0, :, 1] = [5, 4, 10, 0], [4, 4, 8, 0]          # sees views 0 and 2; near: ceil(.8*5)=4, ceil(8.0)=8
    counts[1, :, 0], counts[1, :, 1] = [5, 5, 10, 10], [3, 4, 7, 8]         # sees all; supports views 1 and 3
    counts[2, :, 0], counts[2, :, 1] = [10, 10, 10, 9], [8, 8, 8, 8]        # supports all four (ceil(.8*9) = 8)
    counts[3, :, 0], counts[3, :, 1] = [4, 4, 4, 4], [4, 4, 4, 4]           # seen by no view, every seen sample near
    n = np.array([10, 10, 10, 10, 0, 7])                                      # edge 4: no samples; edge 5: seen nowhere
    r = SP.support_verdict(counts, n, frames=4, min_visible=0.5, min_near=0.8, frames_ratio=0.5)
    assert r["seeing_views"].tolist() == [2, 4, 4, 0, 0, 0]
    assert r["supporting_views"].tolist() == [[2], [2], [4], [0], [0], [0]]
    assert r["kept"].tolist() == [False, False, True, False, False, False], "MORE than ceil(0.5 * 4) = 2 views"
    assert r["kept"].dtype == bool
    assert r["share"][:4, 0].tolist() == [16 / 19, 22 / 30, 32 / 39, 1.0] and np.isnan(r["share"][4:]).all()
    # frames_ratio 0.25: more than 1 view
    assert SP.support_verdict(counts, n, 4, 0.5, 0.8, 0.25)["kept"].tolist() == [True, True, True, False, False, False]
    # min_near 0.81: ceil(0.81 * 5) = 5, ceil(8.1) = 9, ceil(0.81 * 9) = 8
    assert SP.support_verdict(counts, n, 4, 0.5, 0.81, 0.5)["supporting_views"].tolist() == [[0], [0], [1], [0], [0], [0]]
    # min_visible 0.4: ceil(4.0) = 4 samples suffice -- exactly the threshold
    assert SP.support_verdict(counts, n, 4, 0.4, 0.8, 0.5)["seeing_views"].tolist() == [3, 4, 4, 4, 0, 0]
    assert SP.support_verdict(counts, n, 4, 0.41, 0.8, 0.5)["seeing_views"].tolist() == [2, 4, 4, 0, 0, 0]
    # min_visible 0 sees an edge with samples everywhere, never one without; 0 seen samples need 0 near ones
    r0 = SP.support_verdict(counts, n, 4, 0.0, 0.8, 0.5)
    assert r0["seeing_views"].tolist() == [4, 4, 4, 4, 0, 4] and r0["supporting_views"][5].tolist() == [4]
    assert np.isnan(r0["share"][5, 0]), "nothing seen: the share is NaN even where the verdict keeps the edge"
    # several tolerances, a chosen one, tensors
    c2 = np.concatenate([counts, counts[:, :, 1:] // 2], 2)
    r2 = SP.support_verdict(torch.from_numpy(c2), torch.from_numpy(n), 4, 0.5, 0.8, 0.5, keep_index=1)
    assert r2["supporting_views"].tolist() == [[2, 0], [2, 0], [4, 0], [0, 0], [0, 0], [0, 0]] and not r2["kept"].any()
    for kw in (dict(min_visible=1.5), dict(min_near=-0.1), dict(frames_ratio=2.0), dict(keep_index=1)):
        with pytest.raises(ValueError):
            SP.support_verdict(counts, n, 4, **kw)
    with pytest.raises(ValueError, match="counts"):
        SP.support_verdict(counts, n[:3], 4)
    empty = SP.support_verdict(np.zeros((0, 4, 2), np.int32), np.zeros(0, np.int64), 4)
    assert empty["kept"].shape == (0,) and empty["share"].shape == (0, 1)


# ------------------------------------------------------------------------------------------------ the drawn scan
def test_the_drawn_scan_drops_the_chords_that_the_control_point_rule_keeps():
    """Twelve views of 96 x 128, the four drawn edges of EC.SCAN_EDGES, 40 bogus curves and 32 bogus lines whose control /
    end points are samples of the drawn edges.  Measured (host back end, min_near 0.8, min_visible 0.5): every drawn edge
    is seen and supported by 12 of 12 views at 1, 2 and 4 px (pooled share 1.0); a bogus edge is supported by at most 4
    views at 1 px, 5 at 2 px and 11 at 4 px (pooled share at most 0.663, 0.760, 0.943).  The reference's control-point
    rule keeps all 76 edges.  The cap of 6 views is the verdict's own threshold, ceil(0.5 * 12)."""
    edge_dict, drawn = C.scan_edges()
    assert len(edge_dict["curves_ctl_pts"]) == 1 + 40 and len(edge_dict["lines_end_pts"]) == 3 + 32 and drawn.sum() == 4
    assert C.reference_rule_keeps().all(), "the control-point rule keeps every bogus edge"
    for tol in (1, 2):
        r = C.scan_support("host", tol)
        t = r["settings"]["tolerances_px"].index(float(tol))
        print(f"{tol} px: drawn supported by {r['supporting_views'][drawn, t].tolist()} of 12 views, bogus by at most "
              f"{r['supporting_views'][~drawn, t].max()}; pooled share drawn >= {r['share'][drawn, t].min():.4f}, bogus <= "
              f"{np.nanmax(r['share'][~drawn, t]):.4f}")
        assert np.array_equal(r["kept"], drawn), "exactly the four drawn edges are kept"
        assert (r["supporting_views"][drawn, t] == DC.DIR_VIEWS).all() and (r["seeing_views"][drawn] == DC.DIR_VIEWS).all()
        assert (r["supporting_views"][~drawn, t] <= 6).all()
        assert r["settings"]["views"] == DC.DIR_VIEWS and (r["n_points"] > 0).all()


def test_chunking_the_views_changes_nothing():
    whole = C.scan_support("host", 2)
    one = C.scan_support("host", 2, budget_bytes=1)   # one view at a time
    three = C.scan_support("host", 2, budget_bytes=3 * SP.BYTES_PER_PIXEL * DC.DIR_H * DC.DIR_W)
    for part in (one, three):
        assert torch.equal(part["counts"], whole["counts"]) and np.array_equal(part["kept"], whole["kept"])
    assert SP.BYTES_PER_PIXEL == 7
    cams, maps = DC.dir_novel_cameras()
    with pytest.raises(ValueError, match="keep_tolerance_px"):
        SP.edge_support(EC.SCAN_EDGES, cams, maps, "PidiNet", keep_tolerance_px=3, backend="host")
    with pytest.raises(ValueError, match="edge maps"):
        SP.edge_support(EC.SCAN_EDGES, cams, maps[:-1], "PidiNet", backend="host")
    with pytest.raises(ValueError, match="Unknown detector"):
        SP.edge_support(EC.SCAN_EDGES, cams, maps, "HED", backend="host")


def test_views_of_two_sizes_are_grouped():
    cams, maps = DC.dir_novel_cameras()
    small = cams[3]._replace(name="small", width=DC.DIR_W // 2, height=DC.DIR_H // 2, fx=cams[3].fx / 2, fy=cams[3].fy / 2,
                             cx=cams[3].cx / 2, cy=cams[3].cy / 2)
    kw = dict(resolution=EC.SCAN_RESOLUTION, backend="host")
    mixed = SP.edge_support(EC.SCAN_EDGES, [cams[0], small, cams[1]], [maps[0], maps[3][::2, ::2].copy(), maps[1]], "PidiNet", **kw)
    plain = SP.edge_support(EC.SCAN_EDGES, cams[:2], maps[:2], "PidiNet", **kw)
    assert torch.equal(mixed["counts"][:, [0, 2]], plain["counts"]) and mixed["counts"][:, 1, 0].sum() > 0


# ------------------------------------------------------------------------------------------------ files
def test_filter_edge_dict():
    from curve_gaussian_amd.edge_extraction import support as S
    edge_dict, drawn = C.scan_edges()
    got = S.filter_edge_dict(edge_dict, drawn)
    assert np.array_equal(np.array(got["curves_ctl_pts"]).reshape(-1, 12), np.array(EC.SCAN_EDGES["curves_ctl_pts"]))
    assert np.array_equal(np.array(got["lines_end_pts"]), np.array(EC.SCAN_EDGES["lines_end_pts"]))
    assert np.array(got["curves_ctl_pts"]).shape == (1, 4, 3)
    none = S.filter_edge_dict(edge_dict, np.zeros(len(drawn), bool))
    assert none == {"curves_ctl_pts": [], "lines_end_pts": []}
    with pytest.raises(ValueError, match="kept"):
        S.filter_edge_dict(edge_dict, drawn[:-1])
    with pytest.raises(ValueError, match="kept"):
        S.filter_edge_dict(edge_dict, drawn.astype(np.int64))


def test_the_command_line_writes_one_record_per_edge(tmp_path, capsys):
    from curve_gaussian_amd.edge_extraction import support as S
    base, data = C.write_support_scan(tmp_path)
    pred = os.path.join(base, "room", "parametric_edges.json")
    before = open(pred, "rb").read()
    edge_dict, drawn = C.scan_edges()
    argv = ["--base_dir", base, "--dataset_dir", data, "--detector", "PidiNet", "--backend", "host", "--frames_ratio", "0.5",
            "--sample_resolution", str(EC.SCAN_RESOLUTION)]
    assert S.main(argv) == 0
    assert f"room: views 12, edges {len(drawn)}, kept 4" in capsys.readouterr().out
    assert open(pred, "rb").read() == before and not os.path.exists(os.path.join(base, "room", S.FILTERED_FILE))
    out = json.load(open(os.path.join(base, "room", S.SUPPORT_FILE)))
    want = C.scan_support("host", 2)
    assert out["scan"] == "room" and out["total"] == len(drawn) and out["kept"] == 4 and len(out["edges"]) == len(drawn)
    assert out["settings"]["layout"] == "emap" and out["settings"]["tolerances_px"] == [1.0, 2.0, 4.0]
    for e, rec in enumerate(out["edges"]):
        assert sorted(rec) == ["index", "kept", "kind", "samples", "seeing_views", "share", "supporting_views"]
        assert rec["kind"] == ("curve" if e < 41 else "line") and rec["index"] == (e if e < 41 else e - 41)
        assert rec["samples"] == want["n_points"][e] and rec["seeing_views"] == want["seeing_views"][e]
        assert rec["supporting_views"] == want["supporting_views"][e].tolist() and rec["kept"] == bool(drawn[e])
        assert rec["share"] == want["share"][e].tolist()
    # --write_filtered; an edge that nothing sees has a null share
    far = {"curves_ctl_pts": [], "lines_end_pts": edge_dict["lines_end_pts"][:1] + [[50, 50, 50, 50, 50, 51]]}
    with open(pred, "w") as f:
        json.dump(far, f)
    before = open(pred, "rb").read()
    assert S.main(argv + ["--write_filtered"]) == 0
    out = json.load(open(os.path.join(base, "room", S.SUPPORT_FILE)))
    assert [r["kept"] for r in out["edges"]] == [True, False] and out["edges"][1]["share"] == [None, None, None]
    assert out["edges"][1]["samples"] > 0 and out["edges"][1]["seeing_views"] == 0
    assert json.load(open(os.path.join(base, "room", S.FILTERED_FILE))) == {"curves_ctl_pts": [],
                                                                           "lines_end_pts": far["lines_end_pts"][:1]}
    assert open(pred, "rb").read() == before
    assert S.score_scan(base, data, "absent", backend="host") is None
    with pytest.raises(ValueError, match="layout"):
        S.score_scan(base, data, "room", layout="nerf", backend="host")


class _Model:
    """What write_parametric_edges reads of a model."""

    def __init__(self, curve_points, is_bezier):
        self.get_curve_points, self.is_bezier = curve_points, is_bezier


def test_the_export_without_the_flag_writes_the_parents_bytes(tmp_path):
    """The model of test_dataset_io_cpu; the digests are those of the files the commit before this feature writes."""
    cp = torch.tensor([[[0, 0, 0], [0.1, 0, 0], [0.2, 0, 0], [0.3, 0, 0]], [[0, 0, 0], [0, 0.5, 0], [0, 0.5, 0], [0, 1.0, 0]],
                       [[0, 0, 0], [0.0, 0.1, 0], [0.1, 0.1, 0], [0.1, 0.0, 0]]], dtype=torch.float32)
    IO.write_parametric_edges(_Model(cp, torch.tensor([True, False, True])), str(tmp_path))
    assert sorted(os.listdir(tmp_path)) == ["edge_points.ply", "parametric_edges.json"]
    digest = lambda name: hashlib.sha256(open(tmp_path / name, "rb").read()).hexdigest()
    assert digest("parametric_edges.json") == "c7be59f71538e3fea413dff57f35559499a1fdc2f9d5fde104bf3a8c5f3545c4"
    assert digest("edge_points.ply") == "b37f79e893e080a8c1a786b1f40edf3c16f96f67e9636f30d78ed180de923716"


def test_the_export_with_the_flag_adds_two_files(tmp_path, capsys):
    from curve_gaussian_amd.edge_extraction import support as S
    edge_dict, drawn = C.scan_edges()
    curves = np.array(edge_dict["curves_ctl_pts"]).reshape(-1, 4, 3)
    lines = np.array(edge_dict["lines_end_pts"]).reshape(-1, 2, 3)
    as_curves = np.stack([lines[:, 0], lines[:, 0], lines[:, 1], lines[:, 1]], 1)   # a line is its first and last point
    model = _Model(torch.from_numpy(np.concatenate([curves, as_curves])),
                   torch.tensor([True] * len(curves) + [False] * len(lines)))
    cams, maps = DC.dir_novel_cameras()
    plain, flagged = tmp_path / "plain", tmp_path / "flagged"
    IO.write_parametric_edges(model, str(plain))
    capsys.readouterr()
    options = dict(resolution=EC.SCAN_RESOLUTION, frames_ratio=0.5, backend="host")
    d, _ = IO.write_parametric_edges(model, str(flagged), detector="PidiNet", support_checking=True, support_options=options,
                                     cameras=cams, edge_maps=maps)
    assert f"before support checking:  {len(drawn)} after support checking:  4" in capsys.readouterr().out
    assert sorted(os.listdir(flagged)) == ["edge_points.ply", S.SUPPORT_FILE, "parametric_edges.json", S.FILTERED_FILE]
    for name in ("parametric_edges.json", "edge_points.ply"):
        assert open(flagged / name, "rb").read() == open(plain / name, "rb").read(), name
    assert json.load(open(flagged / "parametric_edges.json")) == d and len(d["curves_ctl_pts"]) == 41
    assert json.load(open(flagged / S.FILTERED_FILE)) == S.filter_edge_dict(d, drawn)
    assert [r["kept"] for r in json.load(open(flagged / S.SUPPORT_FILE))["edges"]] == drawn.tolist()
    with pytest.raises(ValueError, match="cameras"):
        IO.write_parametric_edges(model, str(tmp_path / "none"), support_checking=True)


def test_the_driver_parses_the_options():
    from curve_gaussian_amd import train as T
    _, _, args = T.parse_args(["-s", "scan", "-m", "out", "--support_check", "--support_tol_px", "1.5", "--support_min_near",
                               "0.7", "--support_min_visible", "0.25", "--support_frames_ratio", "0.1"])
    assert args.support_check
    assert T.support_options(args) == {"tolerances_px": (1.5,), "keep_tolerance_px": 1.5, "min_near": 0.7, "min_visible": 0.25,
                                       "frames_ratio": 0.1}
    _, _, args = T.parse_args(["-s", "scan", "-m", "out"])
    assert not args.support_check and T.support_options(args) == {}
    import inspect
    assert set(T.support_options(T.parse_args(["-s", "s", "-m", "o", "--support_tol_px", "2"])[2])) <= \
        set(inspect.signature(SP.edge_support).parameters)


# ------------------------------------------------------------------------------------------------ the C ABI
def test_abi_rejections_without_a_gpu():
    from curve_gaussian_amd import _lib
    lib = _lib.load()
    assert _lib.EDGE_SUPPORT_MAX_TOL == SP.MAX_TOL == 4
    p = ctypes.c_void_p(64)   # never dereferenced: every call below is rejected before anything is launched

    def call(E=2, P=5, points=p, offsets=p, V=1, intr=p, w2c=p, H=4, W=4, d2=p, T=1, tol2=p, counts=p):
        return lib.cgs_edge_support(E, P, points, offsets, V, intr, w2c, H, W, d2, T, tol2, counts, None)

    for kw in [dict(E=-1), dict(P=-1), dict(V=-1), dict(T=0), dict(T=5), dict(T=-1), dict(H=0), dict(H=16385), dict(W=0),
               dict(W=-3), dict(points=None), dict(offsets=None), dict(intr=None), dict(w2c=None), dict(d2=None),
               dict(tol2=None), dict(counts=None)]:
        assert call(**kw) == -1 and b"cgs_edge_support: invalid argument" in lib.cgs_last_error(), kw
    assert call(T=5) == -1 and b"T=5" in lib.cgs_last_error()
    assert call(H=16385) == -1 and b"height=16385" in lib.cgs_last_error()
    assert call(points=None) == -1 and b"NULL pointer" in lib.cgs_last_error()
    for kw in [dict(E=0), dict(V=0), dict(E=0, V=0, P=0, points=None, offsets=None, intr=None, w2c=None, d2=None, tol2=None,
                                        counts=None)]:
        assert call(**kw) == 0, "no edge or no view leaves nothing to write"
    assert call(E=0, T=0) == -1, "T is checked first"
