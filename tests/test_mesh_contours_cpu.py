"""Host: occluding contours (ops.mesh_contours, the ``contours`` option of scene.solid_scan, ``ignore_contours`` of
edge_extraction.reprojection) -- the edge tables and contour counts of the solids, the hand-made tents of
mesh_contours_cases.py, the numpy back end against the brute force bit for bit, drawn contours without a gap, the C ABI's
rejections through the library, and the point of the feature: contours in the maps cost the ground truth recall, and the
don't-care zone gives it back exactly."""
import ctypes

import numpy as np
import pytest

import mesh_contours_cases as C
from curve_gaussian_amd import synthetic
from curve_gaussian_amd.edge_extraction import reprojection as R
from curve_gaussian_amd.ops import edge_occlusion as EO
from curve_gaussian_amd.ops import edge_score as ES
from curve_gaussian_amd.ops import mesh_contours as MC
from curve_gaussian_amd.ops.view_chunks import camera_arrays
from curve_gaussian_amd.scene import solid_scan as SS

SCAN_VIEWS, SCAN_H, SCAN_W = 12, 96, 128


# ------------------------------------------------------------------------------------------------ the edge table
@pytest.mark.parametrize("shape, two, flat, smooth", [("box", 18, 6, 6), ("l_bracket", 30, 12, 12), ("cylinder", 378, 186, 250)])
def test_edge_tables_of_the_solids(shape, two, flat, smooth):
    tris, _ = SS.solid_geometry(shape)
    e = MC.mesh_edges(tris)
    assert e.rows.shape == (two, 4, 3) and e.rows.dtype == np.float32 and e.cos.shape == (two,) and e.cos.dtype == np.float64
    assert (e.boundary, e.non_manifold) == (0, 0)
    assert int(MC.smooth(e.cos, 0.01).sum()) == flat and int(MC.smooth(e.cos, 30).sum()) == smooth
    assert MC.edge_rows(tris, "all").shape[0] == two and MC.edge_rows(tris, "smooth").shape[0] == smooth
    assert C.same_bits(MC.edge_rows(tris, "smooth"), e.rows[MC.smooth(e.cos)])


def test_edge_table_order_counts_and_fold():
    a, b, c, d, far = (0, 0, 0), (0, 1, 0), (1, 0, 0), (-1, 0, 0), (0, 0, 1)
    flat = np.array([(a, b, c), (b, a, d)], np.float32)
    e = MC.mesh_edges(flat)
    assert e.rows.shape[0] == 1 and e.boundary == 4 and e.non_manifold == 0 and e.cos[0] == 1.0
    for t1 in ((a, b, c), (a, c, b)):          # a flat pair is flat whatever the winding
        for t2 in ((b, a, d), (a, b, d)):
            assert MC.mesh_edges(np.array([t1, t2], np.float32)).cos[0] == 1.0
    # the ordered bit patterns give d = (-1, 0, 0) the highest index (sign bit), so a < b by index within the row
    bits = lambda row: [tuple(v.view(np.uint32).tolist()) for v in row]
    row = bits(e.rows[0])
    assert row[0] < row[1] and {tuple(e.rows[0, 0]), tuple(e.rows[0, 1])} == {a, b}
    assert tuple(e.rows[0, 2]) == c and tuple(e.rows[0, 3]) == d, "c belongs to the earlier triangle"
    three = MC.mesh_edges(np.array([(a, b, c), (b, a, d), (a, b, far)], np.float32))
    assert three.rows.shape[0] == 0 and three.non_manifold == 1 and three.boundary == 6
    # rows are ordered by (a, b); -0.0 and 0.0 are different vertices
    box = MC.mesh_edges(SS.solid_geometry("box")[0])
    keys = [bits(r)[:2] for r in box.rows]
    assert keys == sorted(keys) and all(k[0] < k[1] for k in keys)
    assert MC.mesh_edges(np.array([(a, b, c), (b, (-0.0, 0, 0), d)], np.float32)).rows.shape[0] == 0
    # a degenerate triangle: NaN, never smooth; a right-angle fold: cos 0
    deg = MC.mesh_edges(np.array([(a, b, c), (b, a, (0, 2, 0))], np.float32))
    assert np.isnan(deg.cos[0]) and not MC.smooth(deg.cos, 180)[0]
    fold = MC.mesh_edges(np.array([(a, b, c), (b, a, far)], np.float32))
    assert fold.cos[0] == 0.0 and not MC.smooth(fold.cos)[0] and MC.smooth(fold.cos, 91)[0]
    assert MC.mesh_edges(np.zeros((0, 3, 3), np.float32)).rows.shape == (0, 4, 3)
    with pytest.raises(ValueError, match="tris must be"):
        MC.mesh_edges(np.zeros((2, 3), np.float32))
    with pytest.raises(ValueError, match="unknown contour kind"):
        MC.edge_rows(flat, "sharp")
    assert MC.CREASE_DEG == 30 and MC.CONTOUR_RADIUS_PX == 2


@pytest.mark.parametrize("n_views, H, W", [(12, 96, 128), (24, 240, 320)])
def test_contour_counts_of_the_solids(n_views, H, W):
    intr, w2c = camera_arrays(SS.emap_cameras_of(synthetic.fibonacci_cameras(n_views, H, W)))
    for shape, smooth_per_view in (("box", 0), ("l_bracket", 0), ("cylinder", 2)):
        e = MC.mesh_edges(SS.solid_geometry(shape)[0])
        flags = MC.contour_flags(e.rows, intr, w2c)
        assert flags.shape == (n_views, e.rows.shape[0])
        assert (flags[:, MC.smooth(e.cos)].sum(1) == smooth_per_view).all(), shape
        assert not flags[:, MC.smooth(e.cos, 0.01)].any(), "a flat edge is never a contour"
        if shape == "box":
            assert (flags.sum(1) == 6).all(), "the hexagonal outline"


# ------------------------------------------------------------------------------------------------ the hand-made cases
@pytest.mark.parametrize("name", sorted(C.HAND_CASES))
def test_hand_made_cases(name):
    row, eye, want = C.HAND_CASES[name]
    K, M = C.camera(eye)
    got = MC.row_masks(row, K, M, C.H, C.W, backend="host").numpy()
    assert C.same_bits(got[0], want), (name, np.argwhere(got[0]).tolist())
    assert C.same_bits(C.contours_brute(row, K, M, C.H, C.W)[0], want), name


def test_a_ridge_behind_a_nearer_quad_is_hidden_with_the_plane_only():
    K, M = C.camera(C.EYE_SIDE)
    plane = EO.mesh_depth(C.QUAD, K, M, C.H, C.W, window=0, backend="host")
    assert float(plane[0, 7, 18]) == 1.0 and np.isinf(float(plane[0, 8, 18]))
    gated = MC.row_masks(C.tent_row(), K, M, C.H, C.W, depth=plane, slack=0.001, backend="host").numpy()
    assert C.same_bits(gated[0], C.BEHIND_QUAD_WITH_PLANE)
    assert C.same_bits(MC.row_masks(C.tent_row(), K, M, C.H, C.W, backend="host").numpy()[0], C.BEHIND_QUAD_WITHOUT)
    far = MC.row_masks(C.tent_row(), K, M, C.H, C.W, depth=plane, slack=1.0, backend="host").numpy()   # 2 > 1 + 1 is false
    assert C.same_bits(far[0], C.BEHIND_QUAD_WITHOUT)
    with pytest.raises(ValueError, match="slack must be finite"):
        MC.row_masks(C.tent_row(), K, M, C.H, C.W, depth=plane, slack=float("nan"), backend="host")


def test_winding_changes_nothing():
    K, M = C.cameras([C.EYE_SIDE, C.EYE_FRONT, C.EYE_EDGE_ON])
    want = MC.contour_masks(C.tent_tris(), K, M, C.H, C.W, kind="all", backend="host").numpy()
    assert C.same_bits(want[0], C.HAND_CASES["side"][2]) and not want[1:].any()
    for flip_c in (False, True):
        for flip_d in (False, True):
            got = MC.contour_masks(C.tent_tris(flip_c, flip_d), K, M, C.H, C.W, kind="all", backend="host").numpy()
            assert C.same_bits(got, want), (flip_c, flip_d)
    assert not MC.contour_masks(C.tent_tris(), K, M, C.H, C.W, kind="smooth", backend="host").numpy().any(), "a fold of 90 deg"


# ------------------------------------------------------------------------------------------------ drawing
@pytest.mark.parametrize("E", [0, 1, 65])
def test_host_equals_the_brute_force_bit_for_bit(E):
    H, W, V = 24, 32, 3
    K, M = C.cube_cameras(V, H, W)
    rows = C.random_rows(E)
    plane = EO.mesh_depth(SS.solid_geometry("box")[0], K, M, H, W, backend="host").numpy()
    free = MC.row_masks(rows, K, M, H, W, backend="host").numpy()
    gated = MC.row_masks(rows, K, M, H, W, depth=plane, slack=0.001, backend="host").numpy()
    assert free.dtype == np.uint8 and set(np.unique(free)) <= {0, 1}
    assert C.same_bits(free, C.contours_brute(rows, K, M, H, W))
    assert C.same_bits(gated, C.contours_brute(rows, K, M, H, W, plane, 0.001))
    if E == 65:
        assert 0 < gated.sum() < free.sum() and (gated <= free).all()
        assert free[:, 0, :].any() or free[:, -1, :].any() or free[:, :, 0].any() or free[:, :, -1].any(), "some row is clipped"
    assert MC.row_masks(rows, K[:0], M[:0], H, W, backend="host").shape == (0, H, W)


def test_fans_on_the_host():
    K, M = C.camera(C.EYE_SIDE)
    for E, contour in ((64, lambda i: True), (64, lambda i: False), (65, lambda i: i % 3 == 0)):
        rows = C.fan(E, contour)
        assert MC.contour_flags(rows, K, M)[0].tolist() == [contour(i) for i in range(E)]
        assert C.same_bits(MC.row_masks(rows, K, M, C.H, C.W, backend="host").numpy(), C.contours_brute(rows, K, M, C.H, C.W))


def test_a_drawn_contour_has_no_gap():
    intr, w2c = camera_arrays(SS.emap_cameras_of(synthetic.fibonacci_cameras(SCAN_VIEWS, SCAN_H, SCAN_W)))
    rows = MC.edge_rows(SS.solid_geometry("cylinder")[0], "smooth")
    flags = MC.contour_flags(rows, intr, w2c)
    seen = 0
    for e in np.flatnonzero(flags.any(0)):
        masks = MC.row_masks(rows[e:e + 1], intr, w2c, SCAN_H, SCAN_W, backend="host").numpy()
        for v in range(SCAN_VIEWS):
            assert (masks[v].any()) == bool(flags[v, e]), "the cylinder is inside every image"
            if flags[v, e]:
                assert C.components(masks[v]) == 1, (e, v)
                seen += 1
    assert seen == 2 * SCAN_VIEWS


# ------------------------------------------------------------------------------------------------ fixtures and the score
@pytest.fixture(scope="module")
def scans():
    return {(shape, contours): SS.solid_scan(shape, SCAN_VIEWS, SCAN_H, SCAN_W, backend="host", contours=contours)
            for shape in ("cylinder", "box") for contours in (False, True)}


def test_solid_scan_with_contours(scans):
    plain, drawn = scans["cylinder", False], scans["cylinder", True]
    assert plain.contours is None and drawn.contours.shape == plain.maps.shape and drawn.contours.dtype == np.uint8
    assert (drawn.contours.reshape(SCAN_VIEWS, -1).sum(1) > 0).all()
    assert C.same_bits(drawn.maps, plain.maps | drawn.contours * np.uint8(255))
    assert (drawn.maps != plain.maps).any() and C.same_bits(drawn.depth, plain.depth) and C.same_bits(drawn.hidden, plain.hidden)
    box, box_drawn = scans["box", False], scans["box", True]
    assert C.same_bits(box_drawn.maps, box.maps) and not box_drawn.contours.any()
    old = SS.SolidScan(plain.tris, plain.edges, plain.synth_cameras, plain.cameras, plain.maps, plain.depth, plain.hidden)
    assert old.contours is None, "every existing construction keeps working"


def check_contour_scores(scans, backend):
    """The point of the feature, shared with the GPU tests."""
    plain, drawn, box = scans["cylinder", False], scans["cylinder", True], scans["box", True]
    score = lambda s, **kw: R.score_edges(s.edges, s.cameras, s.maps, "PidiNet", backend=backend, occluder=s.tris, **kw)
    clean = score(plain)
    agg = clean["aggregate"]
    assert agg["precision"] == [1.0, 1.0, 1.0] and agg["recall"] == [1.0, 1.0, 1.0]
    assert agg["accuracy_px"] == 0.0 and agg["completeness_px"] == 0.0 and agg["chamfer_views"] == SCAN_VIEWS
    assert "contour_pixels" not in clean["views"][0] and "ignore_contours" not in clean["settings"]
    blind = score(drawn)["aggregate"]
    assert blind["precision"] == [1.0, 1.0, 1.0], "the ground truth still explains every pixel it predicts"
    assert blind["recall"][0] < agg["recall"][0], "no 3D edge explains a contour: it costs recall"
    assert blind["completeness_px"] > 0.0
    fixed = score(drawn, ignore_contours=True)
    for row, contour in zip(fixed["views"], drawn.contours):
        assert row["contour_pixels"] == int(contour.sum()) > 0
        assert row["n_pred"] > 0 and row["n_det"] > 0
        assert row["det_hits"] == [row["n_det"]] * 3, "every detected pixel left is a ground-truth pixel"
        assert row["pred_hits"] == [row["n_pred"]] * 3, "every predicted pixel left is a detected one"
        assert row["accuracy_px"] == 0.0 and row["completeness_px"] == 0.0
    assert fixed["settings"]["ignore_contours"] is True and fixed["settings"]["contour_radius_px"] == 2.0
    assert fixed["settings"]["crease_deg"] == 30.0
    assert fixed["aggregate"]["n_pred"] < clean["aggregate"]["n_pred"], "the zone also takes predicted pixels"
    a, b = score(box), score(box, ignore_contours=True)
    assert a["aggregate"] == b["aggregate"] and all(r["contour_pixels"] == 0 for r in b["views"])
    for ra, rb in zip(a["views"], b["views"]):
        assert ra == {k: v for k, v in rb.items() if k != "contour_pixels"}
    return fixed


def test_contours_cost_recall_and_the_zone_gives_it_back(scans):
    check_contour_scores(scans, "host")


def test_ignore_contours_needs_a_mesh_and_does_not_depend_on_the_chunking(scans):
    s = scans["cylinder", True]
    with pytest.raises(ValueError, match="ignore_contours needs an occluder.*depth_maps have no mesh edges"):
        R.score_edges(s.edges, s.cameras, s.maps, "PidiNet", backend="host", depth_maps=list(s.depth), ignore_contours=True)
    with pytest.raises(ValueError, match="ignore_contours needs an occluder"):
        R.score_edges(s.edges, s.cameras, s.maps, "PidiNet", backend="host", ignore_contours=True)
    with pytest.raises(ValueError, match="contour radius"):
        R.score_edges(s.edges, s.cameras, s.maps, "PidiNet", backend="host", occluder=s.tris, ignore_contours=True,
                      contour_radius_px=-1)
    kw = dict(backend="host", occluder=s.tris, ignore_contours=True)
    whole = R.score_edges(s.edges, s.cameras[:4], s.maps[:4], "PidiNet", **kw)
    single = R.score_edges(s.edges, s.cameras[:4], s.maps[:4], "PidiNet", budget_bytes=1, **kw)
    assert whole["views"] == single["views"] and whole["aggregate"] == single["aggregate"]
    wide = R.score_edges(s.edges, s.cameras[:4], s.maps[:4], "PidiNet", contour_radius_px=0, **kw)
    assert wide["aggregate"]["n_det"] > whole["aggregate"]["n_det"], "radius 0 removes the contour pixels alone"
    assert ES.CONTOUR_BYTES_PER_PIXEL == 8
    args = R.parser().parse_args(["--dataset_dir", "x", "--occluder", "mesh.ply", "--ignore_contours"])
    assert args.ignore_contours and args.contour_radius_px == 2 and args.crease_deg == 30
    assert R.contour_options(False) == {} and R.contour_options(True, 3, 20) == {
        "ignore_contours": True, "contour_radius_px": 3, "crease_deg": 20}


def test_ignore_zone_is_the_distance_transform():
    m = np.zeros((1, 9, 9), np.uint8)
    m[0, 4, 4] = 1
    zone = MC.ignore_zone(m, 2, backend="host").numpy()[0]
    yy, xx = np.mgrid[:9, :9]
    assert ((zone != 0) == ((yy - 4) ** 2 + (xx - 4) ** 2 <= 4)).all()
    assert MC.ignore_zone(m, 0, backend="host").numpy().sum() == 1
    assert not MC.ignore_zone(np.zeros((1, 9, 9), np.uint8), 2, backend="host").numpy().any(), "no contour, no zone"


# ------------------------------------------------------------------------------------------------ the C ABI
def test_abi_argument_checks_are_pinned():
    """Status and the exact text of cgs_last_error() for every rejection of cgs_mesh_contours; the pointers are dummies that
    are never dereferenced, and no row passes validation with work to do (V = 0 is the only accepted call)."""
    from curve_gaussian_amd import _lib
    lib = _lib.load()
    p, q = ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 24)
    head = "cgs_mesh_contours: invalid argument "

    def call(E=3, edges=p, V=2, intr=p, w2c=p, H=4, W=6, depth=None, slack=0.0, mask=q):
        return lib.cgs_mesh_contours(E, edges, V, intr, w2c, H, W, depth, slack, mask, None)

    slack = "; with a depth plane the slack is finite and >= 0)"
    for kw, text in [(dict(E=-1), "(E=-1, V=2)"), (dict(V=-1, H=0), "(E=3, V=-1)"),
                     (dict(H=0), "(height=0, width=6; sizes lie in [1, 16384])"),
                     (dict(W=16385, V=0), "(height=4, width=16385; sizes lie in [1, 16384])"),
                     (dict(depth=p, slack=-1e-3), "(slack=-0.001" + slack),
                     (dict(depth=p, slack=float("nan"), V=0), "(slack=nan" + slack),
                     (dict(depth=p, slack=float("inf")), "(slack=inf" + slack),
                     (dict(edges=None), "(NULL pointer; E=3)"), (dict(intr=None), "(NULL pointer; E=3)"),
                     (dict(w2c=None, V=0), "(NULL pointer; E=3)"), (dict(mask=None, E=0), "(NULL pointer; E=0)")]:
        assert call(**kw) == -1 and lib.cgs_last_error().decode() == head + text, (kw, lib.cgs_last_error())
    for kw in (dict(V=0), dict(V=0, E=0, edges=None), dict(V=0, depth=p, slack=0.0),
               dict(V=0, slack=float("nan"))):   # without a plane the slack is not read
        assert call(**kw) == 0, kw
    i, vp = ctypes.c_int, ctypes.c_void_p
    assert _lib.SIGNATURES["cgs_mesh_contours"] == (i, [i, vp, i, vp, vp, i, i, vp, ctypes.c_double, vp, vp])
