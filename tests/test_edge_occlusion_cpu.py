"""Host: occlusion for the 2D score (ops.edge_occlusion, scene.solid_scan, the occluder / depth_maps options of
edge_extraction.reprojection) -- the numpy back end against the brute-force restatements of edge_occlusion_cases.py bit for
bit, the gate at its threshold, the C ABI's rejections through the library, the mesh readers, and the point of the feature:
a solid's ground truth scores 1.0 with the occluder and below 1.0 without."""
import ctypes
import itertools
import json
import os

import numpy as np
import pytest
import torch

import edge_occlusion_cases as C
import edge_score_cases as SC
from curve_gaussian_amd.edge_extraction import reprojection as R
from curve_gaussian_amd.ops import edge_occlusion as EO
from curve_gaussian_amd.ops import edge_score as ES
from curve_gaussian_amd.scene import solid_scan as SS


# ------------------------------------------------------------------------------------------------ z-buffer and window
def test_host_zbuffer_and_window_equal_the_brute_force_bit_for_bit():
    for F, W, V in itertools.product(C.FACES, C.WIDTHS, C.VIEWS):
        K, M = C.cameras(V, C.HEIGHT, W)
        want = C.reference_zbuffer(F, W, V)
        got = EO.mesh_depth(C.triangles(F), K, M, C.HEIGHT, W, window=0, backend="host").numpy()
        assert C.same_bits(got, want), (F, W, V)
        for r in C.WINDOWS:
            win = EO.mesh_depth(C.triangles(F), K, M, C.HEIGHT, W, window=r, backend="host").numpy()
            assert C.same_bits(win, C.window_max_brute(want, r)), (F, W, V, r)
            assert C.same_bits(win, EO.depth_window_max(want, r, backend="host").numpy()), (F, W, V, r)


def test_the_special_triangles_do_what_the_rule_says():
    W = 33
    K, M = C.cameras(1, C.HEIGHT, W)
    sp = C.special_triangles()
    depth = lambda t: EO.mesh_depth(t, K, M, C.HEIGHT, W, window=0, backend="host").numpy()[0]
    for name in ("zero_area", "nan_vertex", "all_behind", "one_behind", "off_screen"):
        assert np.isinf(depth(sp[[C.SPECIAL[name]]])).all(), name
    cover = depth(sp[[C.SPECIAL["whole_image"]]])
    assert np.isfinite(cover).all() and np.allclose(cover, C.COVER_DEPTH, rtol=1e-6)
    # two triangles sharing a side: every pixel centre ON the side is covered, by each of them alone and by both
    diag = np.arange(5)
    for idx in (["shared_a"], ["shared_b"], ["shared_a", "shared_b"]):
        d = depth(sp[[C.SPECIAL[n] for n in idx]])
        assert np.allclose(d[diag, diag], C.SHARED_DEPTH, rtol=1e-6), idx
    both = depth(sp[[C.SPECIAL["shared_a"], C.SPECIAL["shared_b"]]])
    assert np.isfinite(both[:5, :5]).all(), "the square of the two halves has no hole"
    # stacked triangles: the nearer wins in either order, and the order of the whole list does not matter
    full = depth(sp)
    assert np.allclose(full[1, 8], C.STACK_NEAR, rtol=1e-6) and np.allclose(full[1, 14], C.STACK_NEAR, rtol=1e-6)
    assert np.allclose(depth(sp[[C.SPECIAL["stack_far_first"]]])[1, 14], C.STACK_FAR, rtol=1e-6)
    assert C.same_bits(depth(sp[::-1].copy()), full)
    rng = np.random.default_rng(0)
    many = C.triangles(257)
    K5, M5 = C.cameras(5, C.HEIGHT, 67)
    a = EO.mesh_depth(many, K5, M5, C.HEIGHT, 67, window=0, backend="host").numpy()
    b = EO.mesh_depth(many[rng.permutation(257)], K5, M5, C.HEIGHT, 67, window=0, backend="host").numpy()
    assert C.same_bits(a, b)
    # a vertex exactly on a pixel centre covers that pixel (two edge functions are zero there) with the vertex's depth
    tip = depth(sp[[C.SPECIAL["vertex_on_centre"]]])
    assert tip[2, 20] == np.float32(C.CENTRE_DEPTH) and np.isinf(tip[2, 19])


def test_the_window_maximum_keeps_inf():
    d = np.full((2, 7, 9), 3.0, np.float32)
    d[0, 3, 4] = np.inf
    d[1, 0, 0] = np.inf
    for r in (1, 2, 4):
        out = EO.depth_window_max(d, r, backend="host").numpy()
        want = np.full_like(d, 3.0)
        want[0, max(3 - r, 0):3 + r + 1, max(4 - r, 0):4 + r + 1] = np.inf
        want[1, :r + 1, :r + 1] = np.inf
        assert C.same_bits(out, want), r
    assert C.same_bits(EO.depth_window_max(d, 0, backend="host").numpy(), d)
    small = np.array([[[1.0, 5.0], [2.0, 0.5]]], np.float32)   # a plane smaller than the window: clipped, not padded
    assert (EO.depth_window_max(small, 4, backend="host").numpy() == 5.0).all()
    with pytest.raises(ValueError, match=r"window radius must lie in \[0, 4\]"):
        EO.depth_window_max(d, 5, backend="host")
    with pytest.raises(ValueError, match="float32"):
        EO.depth_window_max(d.astype(np.float64), 1, backend="host")


# ------------------------------------------------------------------------------------------------ the gate
def test_the_gate_at_its_threshold():
    H, W = 4, 6
    K = np.array([[1.0, 1.0, 0.0, 0.0]] * 2)
    M = np.stack([np.eye(4)[:3, :4]] * 2)
    M[1, 2, 3] = 2.0 ** -51                         # view 1: c2 = 2.25 + one ulp of 2.25
    pts = np.array([[2.5 * 2.25, 1.5 * 2.25, 2.25]], np.float32)
    depth = np.full((2, H, W), 2.0, np.float32)
    slack = 0.25                                    # depth + slack = 2.25 exactly
    mask, kept, hidden = EO.point_masks_depth(pts, K, M, depth, slack, backend="host", return_counts=True)
    assert kept.tolist() == [1, 0] and hidden.tolist() == [0, 1], "c2 == depth + slack is not hidden, one ulp above is"
    assert mask[0, 1, 2] == 1 and int(mask.sum()) == 1
    for got, want in zip((mask, kept, hidden), C.gate_brute(pts, K, M, depth, slack)):
        assert C.same_bits(got.numpy(), want)
    # no surface: never hidden, whatever the slack
    inf = np.full((2, H, W), np.inf, np.float32)
    mask, kept, hidden = EO.point_masks_depth(pts, K, M, inf, 0.0, backend="host", return_counts=True)
    assert kept.tolist() == [1, 1] and hidden.tolist() == [0, 0]
    for bad in (-1e-9, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="slack must be finite and >= 0"):
            EO.point_masks_depth(pts, K, M, depth, bad, backend="host")
    with pytest.raises(ValueError, match=r"depth must be float32 \[2,4,6\]"):
        EO.point_masks_depth(pts, K, M, depth[:1], slack, backend="host")


def test_host_gate_equals_the_brute_force_and_splits_the_plain_count():
    W, V = 67, 5
    K, M = C.cameras(V, C.HEIGHT, W)
    depth = EO.depth_window_max(C.reference_zbuffer(257, W, V), 1, backend="host").numpy()
    pts = C.samples(600)
    got = EO.point_masks_depth(pts, K, M, depth, 0.01, backend="host", return_counts=True)
    for g, w in zip(got, C.gate_brute(pts, K, M, depth, 0.01)):
        assert C.same_bits(g.numpy(), w)
    mask, kept, hidden = (x.numpy() for x in got)
    plain, plain_kept = ES.point_masks(pts, K, M, C.HEIGHT, W, backend="host", return_kept=True)
    assert (kept + hidden == plain_kept.numpy()).all() and hidden.sum() > 0 and kept.sum() > 0
    assert ((mask == 1) <= (plain.numpy() == 1)).all()
    open_, k, h = EO.point_masks_depth(pts, K, M, np.full_like(depth, np.inf), 0.0, backend="host", return_counts=True)
    assert C.same_bits(open_.numpy(), plain.numpy()) and C.same_bits(k.numpy(), plain_kept.numpy()) and h.sum() == 0
    none = EO.point_masks_depth(pts[:0], K, M, depth, 0.01, backend="host", return_counts=True)
    assert int(none[0].sum()) == 0 and none[1].tolist() == [0] * V and none[2].tolist() == [0] * V


def test_check_depth_maps():
    cams = SS.solid_scan("box", 2, 6, 8, backend="host").cameras
    d = np.full((6, 8), 2.0, np.float64)
    d[0, 0], d[1, 1], d[2, 2] = np.nan, 0.0, -3.0
    out = EO.check_depth_maps(cams, [d, torch.from_numpy(d.astype(np.float32))])
    for m in out:
        assert m.dtype == np.float32 and np.isinf(m[[0, 1, 2], [0, 1, 2]]).all() and (m > 0).all() and (m == 2.0).sum() == 45
    with pytest.raises(ValueError, match="2 cameras and 1 depth maps"):
        EO.check_depth_maps(cams, [d])
    with pytest.raises(ValueError, match=r"must be a float \[6,8\] array"):
        EO.check_depth_maps(cams, [d, d[:5]])
    with pytest.raises(ValueError, match=r"must be a float \[6,8\] array"):
        EO.check_depth_maps(cams, [d, np.full((6, 8), 2, np.int32)])


# ------------------------------------------------------------------------------------------------ the C ABI
def _pinned(lib, fn, head, call, rows, noops):
    for kw, text in rows:
        assert call(**kw) == -1 and lib.cgs_last_error().decode() == head + text, (fn, kw, lib.cgs_last_error())
    for kw in noops:
        assert call(**kw) == 0, (fn, kw)


def test_abi_argument_checks_are_pinned():
    """Status and the exact text of cgs_last_error() for every rejection of the three entries; the pointers are dummies that
    are never dereferenced, and no row passes validation with work to do (V = 0 is the only accepted call)."""
    from curve_gaussian_amd import _lib
    lib = _lib.load()
    p, q = ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 24)

    def mesh(F=3, tris=p, V=2, intr=p, w2c=p, H=4, W=6, depth=p):
        return lib.cgs_mesh_depth(F, tris, V, intr, w2c, H, W, depth, None)

    _pinned(lib, "cgs_mesh_depth", "cgs_mesh_depth: invalid argument ", mesh,
            [(dict(F=-1), "(F=-1, V=2)"), (dict(V=-1, H=0), "(F=3, V=-1)"),
             (dict(H=0), "(height=0, width=6; sizes lie in [1, 16384])"),
             (dict(W=16385, V=0), "(height=4, width=16385; sizes lie in [1, 16384])"),
             (dict(tris=None), "(NULL pointer; F=3)"), (dict(intr=None), "(NULL pointer; F=3)"),
             (dict(w2c=None, V=0), "(NULL pointer; F=3)"), (dict(depth=None, F=0), "(NULL pointer; F=0)")],
            [dict(V=0), dict(V=0, F=0, tris=None)])

    def window(V=2, H=4, W=6, radius=1, depth=p, out=q):
        return lib.cgs_depth_window_max(V, H, W, radius, depth, out, None)

    size = "sizes lie in [1, 16384])"
    _pinned(lib, "cgs_depth_window_max", "cgs_depth_window_max: invalid argument ", window,
            [(dict(V=-1), f"(V=-1, height=4, width=6; {size}"), (dict(H=0, radius=9), f"(V=2, height=0, width=6; {size}"),
             (dict(W=16385, V=0), f"(V=0, height=4, width=16385; {size}"),
             (dict(radius=-1), "(radius=-1; the radius lies in [0, 4])"),
             (dict(radius=5, V=0), "(radius=5; the radius lies in [0, 4])"),
             (dict(depth=None), "(NULL pointer)"), (dict(out=None, V=0), "(NULL pointer)"),
             (dict(out=p), "(depth and out overlap)"),
             (dict(out=ctypes.c_void_p((1 << 20) + 4 * (2 * 4 * 6 - 1))), "(depth and out overlap)"),
             (dict(depth=ctypes.c_void_p((1 << 24) + 4)), "(depth and out overlap)")],
            [dict(V=0), dict(V=0, radius=0), dict(V=0, radius=4, out=p)])   # (V = 0: no byte, no overlap)

    def gate(P=5, points=p, V=2, intr=p, w2c=p, H=4, W=6, depth=p, slack=0.001, mask=q, kept=q, hidden=q):
        return lib.cgs_point_mask_depth(P, points, V, intr, w2c, H, W, depth, slack, mask, kept, hidden, None)

    _pinned(lib, "cgs_point_mask_depth", "cgs_point_mask_depth: invalid argument ", gate,
            [(dict(P=-1), "(P=-1, V=2)"), (dict(V=-1, W=0), "(P=5, V=-1)"),
             (dict(H=16385), "(height=16385, width=6; sizes lie in [1, 16384])"),
             (dict(W=0, V=0), "(height=4, width=0; sizes lie in [1, 16384])"),
             (dict(slack=-1e-3), "(slack=-0.001; the slack is finite and >= 0)"),
             (dict(slack=float("nan"), V=0), "(slack=nan; the slack is finite and >= 0)"),
             (dict(slack=float("inf")), "(slack=inf; the slack is finite and >= 0)"),
             (dict(points=None), "(NULL pointer; P=5)"), (dict(intr=None), "(NULL pointer; P=5)"),
             (dict(w2c=None), "(NULL pointer; P=5)"), (dict(depth=None, V=0), "(NULL pointer; P=5)"),
             (dict(mask=None, P=0), "(NULL pointer; P=0)")],
            [dict(V=0), dict(V=0, P=0, points=None, kept=None, hidden=None), dict(V=0, slack=0.0)])
    i, vp = ctypes.c_int, ctypes.c_void_p
    assert _lib.SIGNATURES["cgs_mesh_depth"] == (i, [i, vp, i, vp, vp, i, i, vp, vp])
    assert _lib.SIGNATURES["cgs_depth_window_max"] == (i, [i, i, i, i, vp, vp, vp])
    assert _lib.SIGNATURES["cgs_point_mask_depth"] == (i, [i, vp, i, vp, vp, i, i, vp, ctypes.c_double, vp, vp, vp, vp])
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "curvegs.h")).read()
    assert f"#define CGS_DEPTH_MAX_WINDOW {EO.MAX_WINDOW}\n" in header and EO.MAX_WINDOW == _lib.DEPTH_MAX_WINDOW == 4
    assert EO.DEPTH_WINDOW == 1 and EO.DEPTH_SLACK == 2 * R.SAMPLE_RESOLUTION == 2 * SS.SAMPLE_RESOLUTION


# ------------------------------------------------------------------------------------------------ mesh files
_QUAD = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0.5], [0, 1, 0]], np.float32)
_QUAD_TRIS = np.stack([_QUAD[[0, 1, 2]], _QUAD[[0, 2, 3]]])


def _ply(fmt, coord="float", count="uchar", index="int", name="vertex_indices", extra=b""):
    import struct
    head = (f"ply\nformat {fmt} 1.0\ncomment hand-written\nelement vertex 4\nproperty {coord} x\nproperty {coord} y\n"
            f"property {coord} z\nproperty uchar red\nelement face 2\nproperty list {count} {index} {name}\n"
            "end_header\n").encode()
    faces = [(3, [0, 1, 2]), (4, [0, 1, 2, 3])]
    if fmt == "ascii":
        body = "".join(f"{x} {y} {z} 7\n" for x, y, z in _QUAD.tolist())
        body += "".join(f"{n} {' '.join(map(str, idx))}\n" for n, idx in faces)
        return head + body.encode() + extra
    c = {"float": "f", "double": "d"}[coord]
    k = {"uchar": "B", "int": "i", "ushort": "H", "uint": "I", "short": "h"}
    body = b"".join(struct.pack("<3" + c + "B", *row, 7) for row in _QUAD.tolist())
    body += b"".join(struct.pack("<" + k[count] + str(n) + k[index], n, *idx) for n, idx in faces)
    return head + body + extra


def test_read_triangle_mesh_reads_every_accepted_form(tmp_path):
    def read(name, data):
        path = tmp_path / name
        path.write_bytes(data if isinstance(data, bytes) else data.encode())
        return EO.read_triangle_mesh(str(path))

    v = "".join(f"v {x} {y} {z}\n" for x, y, z in _QUAD.tolist())
    for k, faces in enumerate(("f 1 2 3 4\n", "f 1/1 2/2 3/3 4/4\n", "f 1/1/1 2/2/2 3/3/3 4/4/4\n", "f 1//1 2//2 3//3 4//4\n",
                               "f -4 -3 -2 -1\n", "f 1 2 3\nf 1 3 4\n")):
        got = read(f"q{k}.obj", "# a quad\nvn 0 0 1\n" + v + "vt 0 0\n" + faces)
        assert C.same_bits(got, _QUAD_TRIS), faces
    pent = read("p.obj", v + "v 0.5 2 0\nf 1 2 3 5 4\n")   # a polygon is fanned from its first vertex
    assert pent.shape == (3, 3, 3) and C.same_bits(pent[2], np.array([[0, 0, 0], [0.5, 2, 0], [0, 1, 0]], np.float32))
    want = np.concatenate([_QUAD_TRIS[:1], _QUAD_TRIS])   # the files hold a triangle and a quad
    for k, kw in enumerate((dict(fmt="ascii"), dict(fmt="ascii", coord="double", name="vertex_index"),
                            dict(fmt="binary_little_endian"), dict(fmt="binary_little_endian", coord="double"),
                            dict(fmt="binary_little_endian", count="ushort", index="uint", name="vertex_index"),
                            dict(fmt="binary_little_endian", count="int", index="short"))):
        assert C.same_bits(read(f"m{k}.ply", _ply(**kw)), want), kw
    out = tmp_path / "w.ply"
    EO.write_triangle_ply(str(out), want)
    assert C.same_bits(EO.read_triangle_mesh(str(out)), want)
    assert read("empty.obj", "# nothing\n").shape == (0, 3, 3)


def test_read_triangle_mesh_rejects_what_it_cannot_read(tmp_path):
    def fails(name, data, match):
        path = tmp_path / name
        path.write_bytes(data if isinstance(data, bytes) else data.encode())
        with pytest.raises(ValueError, match=match):
            EO.read_triangle_mesh(str(path))

    v = "v 0 0 0\nv 1 0 0\nv 0 1 0\n"
    fails("a.stl", "solid", "unknown mesh format '.stl'")
    fails("a.obj", v + "f 1 2 4\n", "refers to vertex 3 of 3")
    fails("b.obj", v + "f 1 2 0\n", "b.obj:4: vertex index 0")
    fails("c.obj", v + "f 1 2\n", "c.obj:4: a face needs at least three vertices")
    fails("d.obj", "v 0 0\n", "d.obj:1: a vertex needs x y z")
    fails("e.obj", v + "f 1 2 x\n", "e.obj:4")
    fails("f.obj", "f -1 -2 -3\n", "refers to vertex -3 of 0")
    fails("a.ply", b"plx\nend_header\n", "not a PLY file")
    fails("b.ply", b"no header at all", "not a PLY file")
    fails("c.ply", _ply("binary_big_endian"), "unsupported PLY format binary_big_endian")
    fails("d.ply", _ply("binary_little_endian")[:-3], "shorter than the header says")
    fails("e.ply", _ply("ascii")[:-9], "shorter than the header says")
    fails("f.ply", _ply("ascii", name="indices"), "no integer list vertex_indices / vertex_index")
    fails("g.ply", _ply("ascii", coord="int"), "x, y, z must be float or double")
    fails("h.ply", _ply("ascii", index="float"), "no integer list")
    fails("i.ply", b"ply\nformat ascii 1.0\nelement vertex 0\nproperty float x\nproperty float y\nproperty float z\n"
                   b"end_header\n", "needs a vertex and a face element")
    fails("j.ply", _ply("ascii", coord="quad"), "bad header line")


# ------------------------------------------------------------------------------------------------ solids and the score
SCAN_VIEWS, SCAN_H, SCAN_W = 12, 96, 128


def check_solid_score(shape, backend):
    """The point of the feature, shared with the GPU tests."""
    s = SS.solid_scan(shape, SCAN_VIEWS, SCAN_H, SCAN_W, backend=backend)
    assert (s.hidden > 0).all(), "every view hides part of a closed solid's edges"
    with_occluder = R.score_edges(s.edges, s.cameras, s.maps, "PidiNet", backend=backend, occluder=s.tris)
    with_depth = R.score_edges(s.edges, s.cameras, s.maps, "PidiNet", backend=backend, depth_maps=list(s.depth))
    for res in (with_occluder, with_depth):
        agg = res["aggregate"]
        assert agg["precision"] == [1.0, 1.0, 1.0] and agg["recall"] == [1.0, 1.0, 1.0], agg
        assert agg["accuracy_px"] == 0.0 and agg["completeness_px"] == 0.0 and agg["chamfer_views"] == SCAN_VIEWS
        assert agg["n_pred"] == agg["n_det"] == int((s.maps != 0).sum()), "the masks are the drawn maps"
        for row, hidden in zip(res["views"], s.hidden):
            assert row["hidden_points"] == hidden > 0 and row["n_pred"] == row["n_det"] == row["pred_hits"][0]
    assert with_occluder["settings"]["occluder"] is True and "depth_maps" not in with_occluder["settings"]
    assert with_depth["settings"]["depth_maps"] is True and "occluder" not in with_depth["settings"]
    for res in (with_occluder, with_depth):
        assert res["settings"]["depth_slack"] == EO.DEPTH_SLACK and res["settings"]["depth_window"] == EO.DEPTH_WINDOW
    assert with_depth["views"] == with_occluder["views"]
    plain = R.score_edges(s.edges, s.cameras, s.maps, "PidiNet", backend=backend)
    assert plain["aggregate"]["recall"] == [1.0, 1.0, 1.0]
    assert plain["aggregate"]["precision"][0] < 1.0, "the hidden edges project inside the silhouette, away from every drawn one"
    assert all("hidden_points" not in row for row in plain["views"]) and "occluder" not in plain["settings"]
    for row, gated in zip(plain["views"], with_occluder["views"]):
        assert row["kept_points"] == gated["kept_points"] + gated["hidden_points"]
    return s


def test_solid_scans_have_their_ground_truth():
    box = SS.solid_scan("box", 4, 24, 32, backend="host")
    assert len(box.edges["lines_end_pts"]) == 12 and box.edges["curves_ctl_pts"] == [] and box.tris.shape == (12, 3, 3)
    assert (box.hidden > 0).all() and box.maps.dtype == np.uint8 and set(np.unique(box.maps)) == {0, 255}
    assert box.depth.shape == (4, 24, 32) and np.isinf(box.depth).any() and np.isfinite(box.depth).any()
    tris, edges = SS.solid_geometry("l_bracket")
    assert len(edges["lines_end_pts"]) == 18 and tris.shape == (20, 3, 3)
    tris, edges = SS.solid_geometry("cylinder")
    assert edges["lines_end_pts"] == [] and len(edges["curves_ctl_pts"]) == 8 and tris.shape == (4 * 64 - 4, 3, 3)
    from curve_gaussian_amd.edge_extraction.abc import pred_points_and_directions
    rim = pred_points_and_directions(edges, 0.005).points
    radial = np.hypot(rim[:, 0] - 0.5, rim[:, 1] - 0.5) / 0.3 - 1.0
    assert np.abs(radial).max() < 2.8e-4, "a quarter arc with the handle 0.5523 leaves the circle by 2.7e-4 r"
    with pytest.raises(ValueError, match="unknown solid 'cone'"):
        SS.solid_geometry("cone")
    # every triangle side is shared by exactly two triangles: the solids are closed
    for shape in SS.SHAPES:
        tris, _ = SS.solid_geometry(shape)
        sides = {}
        for t in tris:
            for a, b in ((0, 1), (1, 2), (2, 0)):
                key = tuple(sorted((tuple(t[a]), tuple(t[b]))))
                sides[key] = sides.get(key, 0) + 1
        assert set(sides.values()) == {2}, shape


@pytest.mark.parametrize("shape", ["box", "l_bracket"])
def test_a_solids_ground_truth_scores_one_with_the_occluder_and_less_without(shape):
    check_solid_score(shape, "host")


def test_score_edges_rejects_two_depth_sources_and_bad_parameters():
    s = SS.solid_scan("box", 2, 12, 16, backend="host")
    with pytest.raises(ValueError, match="an occluder or depth_maps, not both"):
        R.score_edges(s.edges, s.cameras, s.maps, "PidiNet", backend="host", occluder=s.tris, depth_maps=list(s.depth))
    with pytest.raises(ValueError, match="slack must be finite"):
        R.score_edges(s.edges, s.cameras, s.maps, "PidiNet", backend="host", occluder=s.tris, depth_slack=-1.0)
    with pytest.raises(ValueError, match="window radius"):
        R.score_edges(s.edges, s.cameras, s.maps, "PidiNet", backend="host", occluder=s.tris, depth_window=5)
    with pytest.raises(ValueError, match=r"tris must be \[F,3,3\]"):
        R.score_edges(s.edges, s.cameras, s.maps, "PidiNet", backend="host", occluder=np.zeros((4, 3), np.float32))
    # the chunking does not change the result
    a = R.score_edges(s.edges, s.cameras, s.maps, "PidiNet", backend="host", occluder=s.tris)
    b = R.score_edges(s.edges, s.cameras, s.maps, "PidiNet", backend="host", occluder=s.tris, budget_bytes=1)
    assert a == b and ES.DEPTH_BYTES_PER_PIXEL == 8


_LEGACY_SETTINGS = {"detector", "tolerances_px", "edge_threshold", "sample_resolution", "backend", "points"}
_LEGACY_ROW = {"name", "width", "height", "kept_points", "n_pred", "n_det", "pred_hits", "det_hits", "accuracy_px",
               "completeness_px", "both_nonempty"}


def test_without_the_new_arguments_score_edges_is_what_it_was(tmp_path):
    base, data = SC.write_scan(tmp_path, "emap", "DexiNed")
    cams, maps = R.emap_cameras(os.path.join(data, "room"), "DexiNed")
    res = R.score_edges(SC.SCAN_EDGES, cams, maps, "DexiNed", sample_resolution=SC.SCAN_RESOLUTION, backend="host")
    assert set(res["settings"]) == _LEGACY_SETTINGS and all(set(row) == _LEGACY_ROW for row in res["views"])
    # the unchanged path, step by step: point_masks -> detected masks -> score_masks
    from curve_gaussian_amd.ops.view_chunks import camera_arrays, detected_lut, detected_masks
    intr, w2c = camera_arrays(cams)
    pts = R._pred_points(SC.SCAN_EDGES, SC.SCAN_RESOLUTION)
    pm, kept = ES.point_masks(pts, intr, w2c, SC.SCAN_H, SC.SCAN_W, backend="host", return_kept=True)
    det = detected_masks(detected_lut("DexiNed", R.EDGE_MAX_THRESHOLD), list(maps), list(range(len(cams))))
    want = ES.score_masks(pm, det, (1, 2, 4), backend="host")
    assert res["aggregate"] == want["aggregate"]
    assert [row["kept_points"] for row in res["views"]] == kept.tolist()
    assert [row["n_pred"] for row in res["views"]] == want["n_pred"].tolist()
    assert [row["pred_hits"] for row in res["views"]] == want["pred_hits"].tolist()


def test_command_lines(tmp_path, capsys):
    scan_dir = tmp_path / "data" / "box"
    assert SS.main(["box", str(scan_dir), "--views", "3", "--height", "24", "--width", "32", "--depth", "--backend", "host"]) == 0
    assert "box: 3 views of 32x24, 12 triangles, 12 lines, 0 curves" in capsys.readouterr().out
    names = sorted(os.listdir(scan_dir))
    assert names == ["depth", "edge_PidiNet", "gt_edges.json", "mesh.ply", "meta_data.json"], names
    assert sorted(os.listdir(scan_dir / "depth")) == ["0_colors.npy", "1_colors.npy", "2_colors.npy"]
    scan = SS.solid_scan("box", 3, 24, 32, backend="host")
    assert C.same_bits(EO.read_triangle_mesh(str(scan_dir / "mesh.ply")), scan.tris)
    assert json.load(open(scan_dir / "gt_edges.json")) == scan.edges
    assert C.same_bits(np.load(scan_dir / "depth" / "1_colors.npy"), scan.depth[1])
    cams, maps = R.emap_cameras(str(scan_dir), "PidiNet")
    assert C.same_bits(np.asarray(maps), scan.maps), "the written maps are the drawn ones"
    for a, b in zip(cams, scan.cameras):
        assert a.name == b.name and C.same_bits(a.R, b.R) and C.same_bits(a.T, b.T) and a[3:] == b[3:]
    # the ground truth as the prediction: from disk, the gated score is exact with either depth source
    out = tmp_path / "out"
    os.makedirs(out / "box")
    with open(out / "box" / "parametric_edges.json", "w") as f:
        json.dump(scan.edges, f)
    score = out / "box" / R.SCORE_FILE
    common = ["--base_dir", str(out), "--dataset_dir", str(tmp_path / "data"), "--detector", "PidiNet", "--backend", "host"]
    assert R.main(common) == 0
    plain = score.read_bytes()
    assert json.loads(plain)["aggregate"]["precision"][0] < 1.0 and set(json.loads(plain)["settings"]) == \
        _LEGACY_SETTINGS | {"layout", "undistort"}
    # without a depth source the two parameters change nothing: not a byte
    assert R.main(common + ["--depth_slack", "0.5", "--depth_window", "3"]) == 0 and score.read_bytes() == plain
    R.score_scan(str(out), str(tmp_path / "data"), "box", detector="PidiNet", backend="host")
    assert score.read_bytes() == plain
    for flags, key in ((["--occluder", "mesh.ply"], "occluder"), (["--depth_dir", "depth"], "depth_maps")):
        assert R.main(common + flags) == 0
        got = json.loads(score.read_bytes())
        assert got["aggregate"]["precision"] == [1.0, 1.0, 1.0] == got["aggregate"]["recall"]
        assert got["settings"][key] in (True, str(scan_dir / "mesh.ply")) and got["settings"]["depth_window"] == 1
        assert all(row["hidden_points"] > 0 for row in got["views"])
    with pytest.raises(ValueError, match="an occluder or a depth_dir, not both"):
        R.main(common + ["--occluder", "mesh.ply", "--depth_dir", "depth"])
    with pytest.raises(FileNotFoundError, match="no depth map for 0_colors.png"):
        R.main(common + ["--depth_dir", "nowhere"])
    capsys.readouterr()
    # train.py takes the same four options
    from curve_gaussian_amd import train
    _, _, args = train.parse_args(["-s", str(scan_dir), "-m", str(out / "m"), "--reprojection_score", "--occluder", "mesh.ply"])
    assert (args.occluder, args.depth_dir, args.depth_slack, args.depth_window) == ("mesh.ply", None, EO.DEPTH_SLACK, 1)
