"""Host: the depth gate on the four per-sample 2D operators of the extraction chain (ops.edge_support, ops.edge_trim,
ops.edge_orient, ops.edge_snap with ``depth=``; the occluder / depth_maps options of their scan-level functions, of the
support tool and of train.py) -- the numpy back ends against the per-(sample, view) loops of edge_gate_cases.py bit for bit,
the gate's identities, the solids' facts at 1 and 2 px, the independence of the chunking, the ungated output unchanged, and
the C ABI's rejections through the library."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import edge_gate_cases as G
import edge_occlusion_cases as OC
from curve_gaussian_amd.edge_extraction import support as SUP
from curve_gaussian_amd.ops import edge_occlusion as EO
from curve_gaussian_amd.ops import edge_orient as OR
from curve_gaussian_amd.ops import edge_score as ES
from curve_gaussian_amd.ops import edge_snap as SN
from curve_gaussian_amd.ops import edge_support as SP
from curve_gaussian_amd.ops import edge_trim as ET
from curve_gaussian_amd.scene import solid_scan as SS


# ------------------------------------------------------------------------------------------------ brute force
@pytest.mark.parametrize("W,V,P,E,slack", [(67, 5, 150, 4, 0.0), (33, 2, 97, 3, 0.01), (1, 1, 40, 1, 0.01)])
def test_host_back_ends_equal_the_per_pair_loops_bit_for_bit(W, V, P, E, slack):
    c = G.views_case(W, V)
    pts, off = OC.samples(P), G.offsets_for(E, P)
    tol2 = ES.tolerances_squared(G.TOLERANCES)
    got = G.run_operators(P, E, W, V, slack, "host")
    counts, ch = G.support_brute(pts, off, c["K"], c["M"], c["d2"], tol2, c["depth"], slack)
    tally, th = G.tally_brute(pts, c["K"], c["M"], c["d2"], tol2, c["depth"], slack)
    ot, oh = G.oriented_brute(pts, OR.sample_partners(off), c["K"], c["M"], c["near"], G.SPREAD, c["depth"], slack)
    terms, views, sh = G.snap_brute(pts, c["K"], c["M"], c["d2"], SN.capture_squared(G.CAPTURE_PX), c["depth"], slack)
    want = dict(counts=counts, counts_hidden=ch, tally=tally, tally_hidden=th, oriented=ot, oriented_hidden=oh, terms=terms,
                views=views, snap_hidden=sh)
    G.assert_same(got, want, f"W={W} V={V}")
    if W > 1:
        assert ch.sum() > 0 and counts[..., 0].sum() > 0, "the case has hidden and visible samples"
        assert th.sum() == ch.sum() == oh.sum() == sh.sum(), "every operator hides the same pairs"


# ------------------------------------------------------------------------------------------------ identities
def _ungated(P, E, W, V):
    return G.run_operators(P, E, W, V, 0.0, "host", depth=None)


def test_an_all_inf_depth_is_the_ungated_result_with_nothing_hidden():
    P, E, W, V = 130, 4, 67, 5
    plain = _ungated(P, E, W, V)
    got = G.run_operators(P, E, W, V, 0.0, "host", depth=np.full((V, G.HEIGHT, W), np.inf, np.float32))
    for k in ("counts", "tally", "oriented", "terms", "views"):
        assert G.same_bits(got[k], plain[k]), k
    for k in ("counts_hidden", "tally_hidden", "oriented_hidden", "snap_hidden"):
        assert not got[k].any(), k


def test_an_all_zero_depth_hides_everything_that_is_seen():
    P, E, W, V = 130, 4, 67, 5
    plain = _ungated(P, E, W, V)
    got = G.run_operators(P, E, W, V, 0.0, "host", depth=np.zeros((V, G.HEIGHT, W), np.float32))
    for k in ("counts", "tally", "oriented", "terms", "views"):
        assert not got[k].any(), k
    assert G.same_bits(got["counts_hidden"], plain["counts"][..., 0])
    for k in ("tally_hidden", "oriented_hidden", "snap_hidden"):
        assert G.same_bits(got[k], plain["tally"][:, 0]), k
    assert plain["tally"][:, 0].sum() > 0


@pytest.mark.parametrize("slack", G.SLACKS)
def test_seen_plus_hidden_is_the_ungated_seen(slack):
    P, E, W, V = 130, 5, 67, 5
    plain, got = _ungated(P, E, W, V), G.run_operators(P, E, W, V, slack, "host")
    assert G.same_bits(got["counts"][..., 0] + got["counts_hidden"], plain["counts"][..., 0])
    assert G.same_bits(got["tally"][:, 0] + got["tally_hidden"], plain["tally"][:, 0])
    assert G.same_bits(got["oriented"][:, 0] + got["oriented_hidden"], plain["oriented"][:, 0])
    assert (got["counts"] <= plain["counts"]).all() and (got["tally"] <= plain["tally"]).all()
    assert (got["views"] <= plain["views"]).all() and (got["views"] <= got["tally"][:, 0]).all()
    assert got["counts_hidden"].sum() > 0 and got["counts"][..., 0].sum() > 0
    # without the hidden outputs the others are the same
    quiet = G.run_operators(P, E, W, V, slack, "host", hidden=False)
    for k in ("counts", "tally", "oriented", "terms", "views"):
        assert G.same_bits(quiet[k], got[k]), k


def test_a_nan_depth_hides_nothing():
    P, E, W, V = 130, 4, 67, 5
    plain = _ungated(P, E, W, V)
    got = G.run_operators(P, E, W, V, 0.01, "host", depth=np.full((V, G.HEIGHT, W), np.nan, np.float32))
    for k in ("counts", "tally", "oriented", "terms", "views"):
        assert G.same_bits(got[k], plain[k]), k
    assert not got["counts_hidden"].any() and not got["snap_hidden"].any()


def test_the_adding_entries_add_and_any_split_of_the_views_gives_the_bits_of_one_call():
    P, W, V, slack = 130, 67, 5, 0.01
    c = G.views_case(W, V)
    pts, off = OC.samples(P), G.offsets_for(3, P)
    one = G.run_operators(P, 3, W, V, slack, "host")
    for cut in (1, 2, 4):
        terms, views, sh = torch.zeros(P, 10, dtype=torch.float64), torch.zeros(P, dtype=torch.int32), torch.zeros(P, dtype=torch.int32)
        tally, th = torch.zeros(P, 3, dtype=torch.int32), torch.zeros(P, dtype=torch.int32)
        ot, oh = torch.zeros(P, 2, dtype=torch.int32), torch.zeros(P, dtype=torch.int32)
        for sel in (slice(0, cut), slice(cut, V)):
            K, M, d2, near, depth = (np.array(c[k][sel]) for k in ("K", "M", "d2", "near", "depth"))
            kw = dict(depth=depth, slack=slack, backend="host")
            SN.snap_terms(pts, K, M, d2, G.CAPTURE_PX, out=(terms, views), hidden_out=sh, **kw)
            ET.sample_tally(pts, K, M, d2, G.TOLERANCES, out=tally, hidden_out=th, **kw)
            OR.oriented_tally(pts, OR.sample_partners(off), K, M, near, G.SPREAD, out=ot, hidden_out=oh, **kw)
        for k, v in dict(terms=terms, views=views, snap_hidden=sh, tally=tally, tally_hidden=th, oriented=ot,
                         oriented_hidden=oh).items():
            assert G.same_bits(v.numpy(), one[k]), (cut, k)
    # pre-filled outputs come back with the call's numbers added
    filled = G.run_operators(P, 3, W, V, slack, "host", prefill=7)
    for k in ("tally", "tally_hidden", "oriented", "oriented_hidden", "views", "snap_hidden"):
        assert G.same_bits(filled[k], one[k] + 7), k
    single = one["views"] <= 1   # one addition at most: exact; otherwise (7 + a) + b is not 7 + (a + b) to the bit
    assert single.any() and (~single).any()
    assert G.same_bits(filled["terms"][single], 7.0 + one["terms"][single])
    np.testing.assert_allclose(filled["terms"], 7.0 + one["terms"], rtol=1e-12)


def test_the_operators_check_their_new_arguments():
    c = {k: np.array(v) for k, v in G.views_case(33, 2).items()}
    pts, off = OC.samples(10), G.offsets_for(1, 10)
    d2 = torch.from_numpy(c["d2"])
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="slack must be finite and >= 0"):
            ET.sample_tally(pts, c["K"], c["M"], d2, (1,), backend="host", depth=c["depth"], slack=bad)
    with pytest.raises(ValueError, match=r"depth must be float32 \[2,5,33\]"):
        SP.support_counts(pts, off, c["K"], c["M"], d2, (1,), backend="host", depth=c["depth"][:1])
    with pytest.raises(ValueError, match="depth must be float32"):
        SN.snap_terms(pts, c["K"], c["M"], d2, 3, backend="host", depth=c["depth"].astype(np.float64))
    with pytest.raises(ValueError, match="return_hidden needs depth"):
        SP.support_counts(pts, off, c["K"], c["M"], d2, (1,), backend="host", return_hidden=True)
    with pytest.raises(ValueError, match="hidden_out needs depth"):
        OR.oriented_tally(pts, OR.sample_partners(off), c["K"], c["M"], c["near"], backend="host",
                          hidden_out=torch.zeros(10, dtype=torch.int32))
    with pytest.raises(ValueError, match=r"hidden_out must be a contiguous int32 \[10\] tensor"):
        ET.sample_tally(pts, c["K"], c["M"], d2, (1,), backend="host", depth=c["depth"], hidden_out=torch.zeros(9, dtype=torch.int32))


# ------------------------------------------------------------------------------------------------ solids
@pytest.mark.parametrize("shape,views,H,W", G.SOLIDS)
def test_a_solids_ground_truth_is_exact_with_the_gate_and_inflated_without(shape, views, H, W):
    G.check_solid_facts(shape, views, H, W, "host")


def _solid_operands(shape="box"):
    scan = G.solid(shape, 6, 48, 64)
    from curve_gaussian_amd.ops.view_chunks import camera_arrays
    intr, w2c = camera_arrays(scan.cameras)
    pts, off = SP.sample_edges(scan.edges["curves_ctl_pts"], scan.edges["lines_end_pts"], 0.0005)
    depth = EO.mesh_depth(scan.tris, intr, w2c, 48, 64, EO.DEPTH_WINDOW, backend="host")
    d2 = ES.edt_squared((scan.maps > 127).astype(np.uint8), backend="host")
    return scan, pts, off, intr, w2c, depth, d2


def test_snapping_takes_no_view_that_hides_the_sample():
    scan, pts, off, intr, w2c, depth, d2 = _solid_operands()
    hidden = torch.zeros(len(pts), dtype=torch.int32)
    terms, views = SN.snap_terms(pts, intr, w2c, d2, SN.CAPTURE_PX, backend="host", depth=depth, hidden_out=hidden)
    tally = ET.sample_tally(pts, intr, w2c, d2, (1,), backend="host", depth=depth)
    plain_views = SN.snap_terms(pts, intr, w2c, d2, SN.CAPTURE_PX, backend="host")[1]
    assert (views <= tally[:, 0]).all() and (views <= plain_views).all() and (views < plain_views).any()
    assert int(hidden.sum()) == int(scan.hidden.sum())
    # all six views leave no sample of the box unseen; the first two hide some samples in both
    sel = slice(0, 2)
    terms2, views2 = SN.snap_terms(pts, intr[sel], w2c[sel], d2[sel], SN.CAPTURE_PX, backend="host", depth=depth[sel])
    tally2 = ET.sample_tally(pts, intr[sel], w2c[sel], d2[sel], (1,), backend="host", depth=depth[sel])
    plain2 = SN.snap_terms(pts, intr[sel], w2c[sel], d2[sel], SN.CAPTURE_PX, backend="host")[1]
    unseen = ((tally2[:, 0] == 0) & (ET.sample_tally(pts, intr[sel], w2c[sel], d2[sel], (1,), backend="host")[:, 0] > 0)).numpy()
    assert unseen.any(), "two views of the box hide some samples in every view that keeps them"
    con = SN.constrained_samples(views2, 2)
    assert not con[unseen].any() and con.any() and not terms2.numpy()[unseen].any() and not views2.numpy()[unseen].any()
    assert SN.constrained_samples(plain2, 2)[unseen].any(), "without the gate such samples are pulled to front edges"
    # scan level: the ground truth stays where it is, the result names the gate
    res = SN.snap_edges(scan.edges, scan.cameras, scan.maps, "PidiNet", backend="host", occluder=scan.tris, iterations=1)
    assert G.same_bits(res["hidden"], hidden.numpy()) and res["settings"]["occluder"] is True
    assert sum(r["hidden_views"] for r in res["edges"]) == int(scan.hidden.sum())


# ------------------------------------------------------------------------------------------------ chunking
_scan_level, _drop_chunks = G.scan_level, G.comparable


def test_scan_level_results_do_not_depend_on_the_budget():
    scan = G.solid("l_bracket", 5, 48, 64)
    for gate in (dict(occluder=scan.tris), dict(depth_maps=list(scan.depth))):
        whole = _scan_level(scan, "host", None, **gate)
        assert whole["snap"]["settings"]["chunks"] == 1
        for budget, chunks in G.BUDGETS[1:]:
            cut = _scan_level(scan, "host", budget, **gate)
            assert cut["snap"]["settings"]["chunks"] == chunks
            assert _drop_chunks(cut) == _drop_chunks(whole), (sorted(gate), budget)
        assert whole["support"]["hidden"].shape == (18, 5) and whole["trim"]["hidden"].shape == whole["snap"]["hidden"].shape
        assert G.same_bits(whole["trim"]["hidden"].numpy(), whole["oriented"]["hidden"].numpy())
        off = whole["trim"]["offsets"].astype(np.int64)
        per_edge = np.array([int(whole["trim"]["hidden"][off[e]:off[e + 1]].sum()) for e in range(18)])
        assert (per_edge == whole["support"]["hidden"].numpy().sum(1)).all(), "the same pairs, tallied the other way round"
        assert int(whole["trim"]["hidden"].sum()) == int(whole["support"]["hidden"].sum()) == int(scan.hidden.sum())


# ------------------------------------------------------------------------------------------------ the ungated output
_SUPPORT_SETTINGS = {"detector", "resolution", "tolerances_px", "keep_tolerance_px", "min_visible", "min_near", "frames_ratio",
                     "edge_threshold", "backend", "views", "points"}


def test_without_the_new_arguments_results_and_files_are_what_they_were(tmp_path):
    scan = G.solid("box", 6, 48, 64)
    plain = _scan_level(scan, "host", None)
    named = _scan_level(scan, "host", None, occluder=None, depth_maps=None, depth_slack=0.5, depth_window=3)
    assert G.canon(plain) == G.canon(named), "without a depth source the slack and the window change nothing"
    assert set(plain["support"]["settings"]) == _SUPPORT_SETTINGS
    for k, r in plain.items():
        assert "hidden" not in r and not {"occluder", "depth_maps", "depth_slack", "depth_window"} & set(r["settings"]), k
    files = {}
    for tag, res in (("a", plain), ("b", named)):
        d = tmp_path / tag
        os.makedirs(d)
        SUP.write_support(str(d), scan.edges, res["support"])
        SUP.write_trim(str(d), scan.edges, res["trim"])
        SUP.write_snap(str(d), res["snap"])
        files[tag] = {n: (d / n).read_bytes() for n in (SUP.SUPPORT_FILE, SUP.TRIM_FILE, SUP.SNAP_FILE)}
    assert files["a"] == files["b"]
    for n, blob in files["a"].items():
        assert b"hidden" not in blob and b"depth" not in blob and b"occluder" not in blob, n
    # with the gate every file gains one hidden total per edge and the settings of the score
    gated = _scan_level(scan, "host", None, occluder=scan.tris)
    d = tmp_path / "g"
    os.makedirs(d)
    sup = SUP.write_support(str(d), scan.edges, gated["support"])
    trim = SUP.write_trim(str(d), scan.edges, gated["trim"])
    snap = SUP.write_snap(str(d), gated["snap"])
    total = int(scan.hidden.sum())
    assert sum(r["hidden_samples"] for r in sup["edges"]) == total == sum(r["hidden_views"] for r in trim["edges"])
    assert sum(r["hidden_views"] for r in snap["edges"]) == total
    for out in (sup, trim, snap):
        assert out["settings"]["occluder"] is True and out["settings"]["depth_slack"] == EO.DEPTH_SLACK
        assert out["settings"]["depth_window"] == EO.DEPTH_WINDOW
    json.loads((d / SUP.SUPPORT_FILE).read_text())


def test_scan_level_functions_reject_two_depth_sources_and_bad_parameters():
    scan = G.solid("box", 6, 48, 64)
    args = (scan.edges, scan.cameras, scan.maps, "PidiNet")
    for fn, name in ((SP.edge_support, "edge_support"), (ET.trim_edges, "trim_edges"), (SN.snap_edges, "snap_edges")):
        with pytest.raises(ValueError, match=f"{name}: give an occluder or depth_maps, not both"):
            fn(*args, backend="host", occluder=scan.tris, depth_maps=list(scan.depth))
        with pytest.raises(ValueError, match=f"{name}: the slack must be finite and >= 0"):
            fn(*args, backend="host", occluder=scan.tris, depth_slack=-1.0)
        with pytest.raises(ValueError, match=f"{name}: the window radius must lie in"):
            fn(*args, backend="host", occluder=scan.tris, depth_window=5)
        with pytest.raises(ValueError, match="6 cameras and 5 depth maps"):
            fn(*args, backend="host", depth_maps=list(scan.depth)[:5])


# ------------------------------------------------------------------------------------------------ the C ABI
def test_abi_symbols_and_argument_checks_are_pinned():
    """Status and the exact text of cgs_last_error() for every rejection of the four entries; the pointers are dummies that are
    never dereferenced, and no row passes validation with work to do."""
    from curve_gaussian_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(1 << 20)
    sizes = "(height=16385, width=6; sizes lie in [1, 16384])"
    slacks = [(dict(slack=-0.5), "(slack=-0.5; the slack is finite and >= 0)"),
              (dict(slack=float("nan")), "(slack=nan; the slack is finite and >= 0)"),
              (dict(slack=float("inf")), "(slack=inf; the slack is finite and >= 0)")]

    def pinned(fn, call, rows, noops):
        for kw, text in rows + slacks:
            assert call(**kw) == -1, (fn, kw)
            assert lib.cgs_last_error().decode() == f"{fn}: invalid argument {text}", (fn, kw, lib.cgs_last_error())
        for kw in noops:
            assert call(**kw) == 0, (fn, kw)

    def support(E=2, P=5, points=p, offsets=p, V=2, intr=p, w2c=p, H=4, W=6, d2=p, T=2, tol2=p, depth=p, slack=0.001, counts=p,
                hidden=p):
        return lib.cgs_edge_support_depth(E, P, points, offsets, V, intr, w2c, H, W, d2, T, tol2, depth, slack, counts, hidden,
                                          None)

    null = "(NULL pointer)"
    pinned("cgs_edge_support_depth", support,
           [(dict(E=-1), "(E=-1, P=5, V=2, T=2; T lies in [1, 4])"), (dict(T=5), "(E=2, P=5, V=2, T=5; T lies in [1, 4])"),
            (dict(T=0, slack=-1.0), "(E=2, P=5, V=2, T=0; T lies in [1, 4])"), (dict(H=16385), sizes),
            (dict(depth=None), null), (dict(d2=None), null), (dict(counts=None), null), (dict(points=None), null),
            (dict(offsets=None), null)],
           [dict(E=0), dict(V=0), dict(V=0, depth=None, hidden=None)])

    def tally(P=5, points=p, V=2, intr=p, w2c=p, H=4, W=6, d2=p, T=2, tol2=p, depth=p, slack=0.001, tally=p, hidden=p):
        return lib.cgs_sample_support_depth(P, points, V, intr, w2c, H, W, d2, T, tol2, depth, slack, tally, hidden, None)

    null = "(NULL pointer; P=5, V=2)"
    pinned("cgs_sample_support_depth", tally,
           [(dict(P=-1), "(P=-1, V=2, T=2; T lies in [1, 4])"), (dict(T=5), "(P=5, V=2, T=5; T lies in [1, 4])"),
            (dict(H=16385), sizes), (dict(depth=None), null), (dict(d2=None), null), (dict(tally=None), null),
            (dict(points=None), null), (dict(tol2=None), null)],
           [dict(P=0), dict(V=0), dict(P=0, points=None, tally=None, hidden=None)])

    def oriented(P=5, points=p, partner=p, V=2, intr=p, w2c=p, H=4, W=6, near=p, spread=1, depth=p, slack=0.001, tally=p,
                 hidden=p):
        return lib.cgs_sample_support_oriented_depth(P, points, partner, V, intr, w2c, H, W, near, spread, depth, slack, tally,
                                                     hidden, None)

    pinned("cgs_sample_support_oriented_depth", oriented,
           [(dict(P=-1), "(P=-1, V=2, spread=1; the spread lies in [0, 4])"),
            (dict(spread=5), "(P=5, V=2, spread=5; the spread lies in [0, 4])"), (dict(H=16385), sizes),
            (dict(depth=None), null), (dict(near=None), null), (dict(partner=None), null), (dict(tally=None), null)],
           [dict(P=0), dict(V=0), dict(V=0, hidden=None)])

    def snap(P=5, points=p, V=2, intr=p, w2c=p, H=4, W=6, d2=p, cap2=9, lut=p, depth=p, slack=0.001, terms=p, views=p, hidden=p):
        return lib.cgs_sample_snap_terms_depth(P, points, V, intr, w2c, H, W, d2, cap2, lut, depth, slack, terms, views, hidden,
                                               None)

    pinned("cgs_sample_snap_terms_depth", snap,
           [(dict(P=-1), "(P=-1, V=2, cap2=9; cap2 lies in [1, 64])"), (dict(cap2=65), "(P=5, V=2, cap2=65; cap2 lies in [1, 64])"),
            (dict(H=16385), sizes), (dict(depth=None), null), (dict(d2=None), null), (dict(lut=None), null),
            (dict(terms=None), null), (dict(views=None), null)],
           [dict(P=0), dict(V=0), dict(V=0, hidden=None)])
    i, vp, d = ctypes.c_int, ctypes.c_void_p, ctypes.c_double
    assert _lib.SIGNATURES["cgs_edge_support_depth"] == (i, [i, i, vp, vp, i, vp, vp, i, i, vp, i, vp, vp, d, vp, vp, vp])
    assert _lib.SIGNATURES["cgs_sample_support_depth"] == (i, [i, vp, i, vp, vp, i, i, vp, i, vp, vp, d, vp, vp, vp])
    assert _lib.SIGNATURES["cgs_sample_support_oriented_depth"] == (i, [i, vp, vp, i, vp, vp, i, i, vp, i, vp, d, vp, vp, vp])
    assert _lib.SIGNATURES["cgs_sample_snap_terms_depth"] == (i, [i, vp, i, vp, vp, i, i, vp, i, vp, vp, d, vp, vp, vp, vp])
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "curvegs.h")).read()
    for fn in ("cgs_edge_support_depth", "cgs_sample_support_depth", "cgs_sample_support_oriented_depth",
               "cgs_sample_snap_terms_depth"):
        assert hasattr(lib, fn) and f"int {fn}(" in header, fn
    assert "NEVER tested against depth" in header


# ------------------------------------------------------------------------------------------------ the tools
def test_the_support_tool_and_train_take_the_flags(tmp_path, capsys):
    scan = G.solid("box", 6, 48, 64)
    scan_dir = tmp_path / "data" / "box"
    SS.write_solid_scan(str(scan_dir), scan, depth=True)
    out = tmp_path / "out"
    os.makedirs(out / "box")
    with open(out / "box" / "parametric_edges.json", "w") as f:
        json.dump(scan.edges, f)
    args = SUP.parser().parse_args(["--dataset_dir", "x", "--occluder", "mesh.ply", "--depth_slack", "0.002"])
    assert (args.occluder, args.depth_dir, args.depth_slack, args.depth_window) == ("mesh.ply", None, 0.002, EO.DEPTH_WINDOW)
    common = ["--base_dir", str(out), "--dataset_dir", str(tmp_path / "data"), "--detector", "PidiNet", "--backend", "host",
              "--tolerances", "1", "2", "--keep_tolerance", "1", "--snap", "--snap_iterations", "1", "--trim"]
    names = (SUP.SUPPORT_FILE, SUP.TRIM_FILE, SUP.SNAP_FILE)
    assert SUP.main(common) == 0
    plain = {n: (out / "box" / n).read_bytes() for n in names}
    # without a depth source the two parameters change nothing: not a byte
    assert SUP.main(common + ["--depth_slack", "0.5", "--depth_window", "3"]) == 0
    assert {n: (out / "box" / n).read_bytes() for n in names} == plain
    assert all(b"hidden" not in blob and b"depth" not in blob for blob in plain.values())
    total = int(scan.hidden.sum())
    for flags, key in ((["--occluder", "mesh.ply"], "occluder"), (["--depth_dir", "depth"], "depth_maps")):
        assert SUP.main(common + flags) == 0
        sup, trim, snap = (json.loads((out / "box" / n).read_text()) for n in names)
        assert sup["kept"] == sup["total"] == 12 and trim["pieces"] == 12 and trim["kept_samples"] == trim["samples"]
        assert sum(r["hidden_views"] for r in snap["edges"]) == total
        for got in (sup, trim, snap):
            assert got["settings"][key] in (True, str(scan_dir / "mesh.ply")) and got["settings"]["depth_window"] == 1
    with pytest.raises(ValueError, match="an occluder or a depth_dir, not both"):
        SUP.main(common + ["--occluder", "mesh.ply", "--depth_dir", "depth"])
    capsys.readouterr()
    # train.py: one new flag, an argument error without a depth source
    from curve_gaussian_amd import train
    base = ["-s", str(scan_dir), "-m", str(out / "m"), "--support_check"]
    _, _, args = train.parse_args(base)
    assert args.gate_edge_checks is False
    _, _, args = train.parse_args(base + ["--gate_edge_checks", "--depth_dir", "depth"])
    assert args.gate_edge_checks is True and args.depth_dir == "depth"
    with pytest.raises(SystemExit):
        train.parse_args(base + ["--gate_edge_checks"])
    assert "--gate_edge_checks needs a depth source" in capsys.readouterr().err
    # the export's chain with the flag: the three 2D steps name the gate, and without it they do not
    from curve_gaussian_amd.edge_extraction.reprojection import emap_cameras
    cams, maps = emap_cameras(str(scan_dir), "PidiNet")
    model = out / "m"
    os.makedirs(model)
    with open(model / "parametric_edges.json", "w") as f:
        json.dump(scan.edges, f)
    flags = base + ["--snap_edges", "--snap_iterations", "0", "--trim_edges", "--detector", "PidiNet"]
    import unittest.mock as mock
    host = lambda fn: (lambda *a, **kw: fn(*a, **dict(kw, backend="host")))
    with mock.patch.object(SP, "edge_support", host(SP.edge_support)), mock.patch.object(ET, "trim_edges", host(ET.trim_edges)), \
            mock.patch.object(SN, "snap_edges", host(SN.snap_edges)):
        for extra, gated in (([], False), (["--gate_edge_checks", "--occluder", "mesh.ply"], True),
                             (["--gate_edge_checks", "--depth_dir", "depth"], True)):
            _, _, args = train.parse_args(flags + extra)
            train.export_checks(args, str(model), cams, "PidiNet", edge_maps=maps, source_path=str(scan_dir))
            for n in names:
                got = json.loads((model / n).read_text())
                assert ("depth_slack" in got["settings"]) == gated, (n, extra)
    capsys.readouterr()


class _Model:
    """What write_parametric_edges reads of a model."""

    def __init__(self, curve_points, is_bezier):
        self.get_curve_points, self.is_bezier = curve_points, is_bezier


def test_the_export_passes_depth_options_to_its_three_2d_steps(tmp_path, capsys):
    from curve_gaussian_amd.scene import dataset_io as IO
    scan = G.solid("box", 6, 48, 64)
    lines = np.asarray(scan.edges["lines_end_pts"], np.float64).reshape(-1, 2, 3)
    as_curves = np.stack([lines[:, 0], lines[:, 0], lines[:, 1], lines[:, 1]], 1)   # a line is its first and last point
    model = _Model(torch.from_numpy(as_curves), torch.tensor([False] * len(lines)))
    host = dict(backend="host")
    rest = dict(cameras=scan.cameras, edge_maps=list(scan.maps), detector="PidiNet", snap=True,
                snap_options=dict(host, iterations=0), support_checking=True, support_options=host, trim=True, trim_options=host)
    names = (SUP.SUPPORT_FILE, SUP.TRIM_FILE, SUP.SNAP_FILE)
    IO.write_parametric_edges(model, str(tmp_path / "plain"), **rest)
    IO.write_parametric_edges(model, str(tmp_path / "none"), depth_options=None, **rest)
    for n in names:
        blob = (tmp_path / "plain" / n).read_bytes()
        assert blob == (tmp_path / "none" / n).read_bytes() and b"depth" not in blob and b"hidden" not in blob, n
    IO.write_parametric_edges(model, str(tmp_path / "gated"), depth_options={"occluder": scan.tris, "depth_slack": 0.002}, **rest)
    for n in names:
        got = json.loads((tmp_path / "gated" / n).read_text())
        assert got["settings"]["occluder"] is True and got["settings"]["depth_slack"] == 0.002, n
        assert got["settings"]["depth_window"] == EO.DEPTH_WINDOW
        assert sum(r.get("hidden_samples", r.get("hidden_views")) for r in got["edges"]) > 0, n
    # an option of the same name in a step's own options wins for that step
    IO.write_parametric_edges(model, str(tmp_path / "own"), depth_options={"occluder": scan.tris, "depth_slack": 0.002},
                              **dict(rest, trim_options=dict(host, depth_slack=0.004)))
    assert json.loads((tmp_path / "own" / SUP.TRIM_FILE).read_text())["settings"]["depth_slack"] == 0.004
    assert json.loads((tmp_path / "own" / SUP.SUPPORT_FILE).read_text())["settings"]["depth_slack"] == 0.002
    capsys.readouterr()


def test_the_drivers_export_gates_a_scenes_own_cameras(tmp_path, capsys):
    """``export_checks`` as ``train.main`` calls it: a Scene's cameras with their maps inside (``edge_maps`` None), the depth
    maps found by the cameras' image names."""
    import types
    import unittest.mock as mock

    from curve_gaussian_amd import train
    from curve_gaussian_amd.edge_extraction.reprojection import scene_cameras
    scan = G.solid("box", 6, 48, 64)
    scan_dir = tmp_path / "data" / "box"
    SS.write_solid_scan(str(scan_dir), scan, depth=True)
    scene = [types.SimpleNamespace(image_name=c.name, image_height=c.height, image_width=c.width, R=np.ascontiguousarray(c.R.T),
                                   T=c.T, FoVx=s.FoVx, FoVy=s.FoVy,
                                   original_image=torch.from_numpy(m.astype(np.float32) / 255.0)[None])
             for c, s, m in zip(scan.cameras, scan.synth_cameras, scan.maps)]
    cams, maps = scene_cameras(scene)
    for a, b in zip(cams, scan.cameras):   # the stand-ins are the scan's cameras
        assert a.name == b.name and G.same_bits(a.R, b.R) and G.same_bits(a.T, b.T) and a[3:] == b[3:]
    assert G.same_bits(np.asarray(maps), scan.maps)
    names = (SUP.SUPPORT_FILE, SUP.TRIM_FILE, SUP.SNAP_FILE)
    flags = ["-s", str(scan_dir), "--detector", "PidiNet", "--support_check", "--snap_edges", "--snap_iterations", "0",
             "--trim_edges", "--gate_edge_checks"]
    host = lambda fn: (lambda *a, **kw: fn(*a, **dict(kw, backend="host")))
    written = {}
    with mock.patch.object(SP, "edge_support", host(SP.edge_support)), mock.patch.object(ET, "trim_edges", host(ET.trim_edges)), \
            mock.patch.object(SN, "snap_edges", host(SN.snap_edges)):
        for tag, source, given in (("maps_inside", ["--depth_dir", "depth"], None), ("maps_given", ["--depth_dir", "depth"], maps),
                                   ("mesh_inside", ["--occluder", "mesh.ply"], None)):
            model = tmp_path / tag
            os.makedirs(model)
            with open(model / "parametric_edges.json", "w") as f:
                json.dump(scan.edges, f)
            _, _, args = train.parse_args(flags + source + ["-m", str(model)])
            train.export_checks(args, str(model), scene if given is None else cams, "PidiNet", edge_maps=given,
                                source_path=str(scan_dir))
            written[tag] = {n: json.loads((model / n).read_text()) for n in names}
    capsys.readouterr()
    assert written["maps_inside"] == written["maps_given"]
    total = int(scan.hidden.sum())
    for tag in ("maps_inside", "mesh_inside"):
        sup, trim, snap = (written[tag][n] for n in names)
        assert sup["kept"] == sup["total"] == 12 and trim["kept_samples"] == trim["samples"]
        assert sum(r["hidden_samples"] for r in sup["edges"]) == total == sum(r["hidden_views"] for r in snap["edges"])
        assert sup["settings"]["depth_window"] == EO.DEPTH_WINDOW
    assert written["maps_inside"][SUP.SUPPORT_FILE]["settings"]["depth_maps"] is True
    assert written["mesh_inside"][SUP.SUPPORT_FILE]["settings"]["occluder"] == str(scan_dir / "mesh.ply")
    # two sources with the flag: an argument error, before any work
    with pytest.raises(SystemExit):
        train.parse_args(flags + ["--occluder", "mesh.ply", "--depth_dir", "depth", "-m", str(tmp_path / "m")])
    assert "takes one depth source" in capsys.readouterr().err
