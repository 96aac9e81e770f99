"""CPU: the host back end of ops.tsdf (the distance field and its marching-tetrahedra surface; include/curvegs.h,
cgs_tsdf_integrate / cgs_tsdf_mesh_count / cgs_tsdf_mesh_emit) against the brute force of tsdf_cases.py bit for bit, the
derived cases and the winding against ``mesh_edges`` on closed fields, the box end to end on the host back end, the tool,
and the header's constants."""
import json
import os
import re

import numpy as np
import pytest
import torch

import tsdf_cases as TC
from curve_gaussian_amd import _lib
from curve_gaussian_amd.ops import edge_occlusion as EO
from curve_gaussian_amd.ops import mesh_contours as MC
from curve_gaussian_amd.ops import tsdf as TS
from curve_gaussian_amd.scene import solid_scan as SS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def integrate(c, backend="host", state=None):
    s, w = TS.integrate(c["depth"], c["K"], c["M"], c["dims"], c["bounds"], c["trunc"], state=state, backend=backend)
    return s.cpu().numpy(), w.cpu().numpy()


def extract(total, weight, dims, bounds, min_weight, backend="host"):
    tris, counts = TS.extract(torch.from_numpy(np.ascontiguousarray(total, np.float64)),
                              torch.from_numpy(np.ascontiguousarray(weight, np.uint16)), dims, bounds, min_weight,
                              backend=backend, return_counts=True)
    return counts.cpu().numpy(), tris.cpu().numpy()


def same_state(a, b):
    return (a[0].view(np.uint64) == b[0].view(np.uint64)).all() and (a[1] == b[1]).all()


def check_extract(total, weight, dims, bounds, min_weight):
    counts, tris = extract(total, weight, dims, bounds, min_weight)
    want_counts, want = TC.brute_extract(total, weight, dims, bounds, min_weight)
    assert counts.dtype == np.uint8 and (counts == want_counts).all() and TC.same_bits(tris, want)
    return counts, tris


# ------------------------------------------------------------------------------------------------ integration
@pytest.mark.parametrize("H,W", [(1, 1), (5, 7), (9, 11)])
@pytest.mark.parametrize("V", [1, 3])
@pytest.mark.parametrize("dims", [(1, 1, 1), (2, 2, 2), (3, 4, 5), (5, 13, 5)])
def test_integration_equals_the_brute_force(dims, V, H, W):
    c = TC.random_case(dims, V, H, W, 7 * V + H + dims[1])
    got = integrate(c)
    assert got[0].dtype == np.float64 and got[1].dtype == np.uint16
    assert same_state(got, TC.brute_integrate(c["depth"], c["K"], c["M"], dims, c["bounds"], c["trunc"]))
    if H > 1 and dims[0] > 1:
        assert 0 < int((got[1] > 0).sum()) and int(got[1].max()) <= V    # something is observed, and not by magic


@pytest.mark.parametrize("name,case,total,weight", [
    ("behind the camera", TC.one_point(2.0, tz=-5.0), 0.0, 0),
    ("u == width", TC.one_point(2.0, cx=0.5), 0.0, 0),
    ("inside the image", TC.one_point(2.0), 0.0, 1),
    ("sdf == -trunc", TC.one_point(1.75), -1.0, 1),
    ("sdf just beyond -trunc", TC.one_point(float(np.nextafter(np.float32(1.75), np.float32(0.0)))), 0.0, 0),
    ("sdf == trunc", TC.one_point(2.25), 1.0, 1),
    ("sdf beyond trunc", TC.one_point(5.0), 1.0, 1),
    ("half way", TC.one_point(2.125), 0.5, 1),
    ("depth 0", TC.one_point(0.0), 0.0, 0),
    ("negative depth", TC.one_point(-2.0), 0.0, 0),
    ("NaN depth", TC.one_point(TC.NAN), 0.0, 0),
    ("+inf depth", TC.one_point(TC.INF), 0.0, 0),
])
def test_named_integration_cases(name, case, total, weight):
    got = integrate(case)
    assert same_state(got, TC.brute_integrate(case["depth"], case["K"], case["M"], case["dims"], case["bounds"], case["trunc"]))
    assert got[0][0] == total and got[1][0] == weight, name


def test_chunked_views_give_the_bits_of_one_call():
    c = TC.random_case((5, 13, 5), 3, 9, 11, 5)
    whole = integrate(c)
    state = TS.integrate(c["depth"][:1], c["K"][:1], c["M"][:1], c["dims"], c["bounds"], c["trunc"], backend="host")
    back = TS.integrate(c["depth"][1:], c["K"][1:], c["M"][1:], c["dims"], c["bounds"], c["trunc"], state=state, backend="host")
    assert back[0] is state[0] and back[1] is state[1]
    assert same_state((state[0].numpy(), state[1].numpy()), whole) and int(whole[1].max()) > 1
    brute = TC.brute_integrate(c["depth"][1:], c["K"][1:], c["M"][1:], c["dims"], c["bounds"], c["trunc"],
                               state=TC.brute_integrate(c["depth"][:1], c["K"][:1], c["M"][:1], c["dims"], c["bounds"], c["trunc"]))
    assert same_state(brute, whole)
    empty = TS.integrate(c["depth"][:0], c["K"][:0], c["M"][:0], c["dims"], c["bounds"], c["trunc"], state=state, backend="host")
    assert same_state((empty[0].numpy(), empty[1].numpy()), whole)        # V = 0 adds nothing


def test_the_weight_saturates():
    one = TC.one_point(2.125)
    c = dict(one, depth=np.repeat(one["depth"], 3, 0), K=np.repeat(one["K"], 3, 0), M=np.repeat(one["M"], 3, 0))
    state = (torch.tensor([7.25], dtype=torch.float64), torch.tensor([TC.MAX_WEIGHT - 1], dtype=torch.uint16))
    want = TC.brute_integrate(c["depth"], c["K"], c["M"], c["dims"], c["bounds"], c["trunc"],
                              state=(state[0].numpy().copy(), state[1].numpy().copy()))
    got = integrate(c, state=state)
    assert same_state(got, want) and got[0][0] == 7.75 and got[1][0] == TC.MAX_WEIGHT == TS.MAX_WEIGHT


def test_integration_argument_checks():
    c = TC.random_case((2, 2, 2), 1, 5, 7, 1)
    for bad in (0.0, -1.0, TC.INF, TC.NAN):
        with pytest.raises(ValueError, match="trunc"):
            integrate(dict(c, trunc=bad))
    with pytest.raises(ValueError, match="depth must be float32"):
        integrate(dict(c, depth=c["depth"].astype(np.float64)))
    with pytest.raises(ValueError, match="state"):
        integrate(c, state=(torch.zeros(8, dtype=torch.float32), torch.zeros(8, dtype=torch.uint16)))
    with pytest.raises(ValueError, match="min_weight"):
        extract(np.zeros(8), np.zeros(8, np.uint16), (2, 2, 2), TC.UNIT, 0)


# ------------------------------------------------------------------------------------------------ extraction
def test_every_corner_pattern_of_a_cell():
    rng = np.random.default_rng(11)
    tets = TC.tetrahedra()
    for pattern in range(256):
        for mags in (None, rng.uniform(0.25, 4.0, 8)):
            total, weight = TC.pattern_state(pattern, mags)
            counts, tris = check_extract(total, weight, (2, 2, 2), TC.CELL_BOUNDS, 2)
            crossed = sum(0 < sum((pattern >> c) & 1 for c in q) < 4 for q, _ in tets)
            assert crossed <= counts[0] <= min(2 * crossed, TS.CELL_MAX_TRIS) and (pattern in (0, 255)) == (counts[0] == 0)


def test_normals_point_from_inside_to_outside():
    """In a tetrahedron the field is linear: a triangle's normal must have a positive product with its gradient.  Checked
    on the trilinear sign of every cell pattern through the cell's own corner values."""
    lo, step = TC.lattice(TC.CELL_BOUNDS, (2, 2, 2))
    P = np.array([[TC.centre(lo, step, a, (c >> a) & 1) for a in range(3)] for c in range(8)])
    rng = np.random.default_rng(3)
    for pattern in range(1, 255):
        total, weight = TC.pattern_state(pattern, rng.uniform(0.25, 4.0, 8))
        f = total / weight
        _, tris = extract(total, weight, (2, 2, 2), TC.CELL_BOUNDS, 2)
        at = 0
        for q, odd in TC.tetrahedra():
            n = len(TC.case_triangles([f[c] < 0.0 for c in q], odd))
            A = np.array([P[q[x]] - P[q[0]] for x in (1, 2, 3)])
            grad = np.linalg.solve(A, np.array([f[q[x]] - f[q[0]] for x in (1, 2, 3)]))
            for t in tris[at:at + n].astype(np.float64):
                assert np.cross(t[1] - t[0], t[2] - t[0]) @ grad > 0.0, (pattern, q)
            at += n
        assert at == len(tris)


def test_zero_corner_min_weight_and_flat_grids():
    total, weight = TC.pattern_state(0b00001010)                  # corners 1 and 3 inside: a quad in tetrahedron (0, 1, 3, 7)
    total[0] = 0.0                                                # exactly 0.0: outside, and its vertices sit ON the corner
    counts, tris = check_extract(total, weight, (2, 2, 2), TC.CELL_BOUNDS, 2)
    kept, dropped = TS.drop_degenerate(tris)
    assert counts[0] > 0 and dropped > 0 and len(kept) + dropped == len(tris)
    total[0] = -0.0
    assert (check_extract(total, weight, (2, 2, 2), TC.CELL_BOUNDS, 2)[0] == counts).all()
    total, weight = TC.pattern_state(0b00010110)
    weight[5] = 1                                                 # one corner under min_weight: the cell emits nothing
    counts, tris = check_extract(total, weight, (2, 2, 2), TC.CELL_BOUNDS, 2)
    assert counts.tolist() == [0] and tris.shape == (0, 3, 3)
    assert check_extract(total, weight, (2, 2, 2), TC.CELL_BOUNDS, 1)[0][0] > 0
    for dims in ((1, 3, 3), (3, 1, 3), (3, 3, 1), (1, 1, 1)):     # a dimension of 1: no cells
        total, weight = TC.shell_field(dims, 1, True)
        counts, tris = check_extract(-total, weight, dims, TC.UNIT, 1)
        assert counts.shape == (0,) and tris.shape == (0, 3, 3)


@pytest.mark.parametrize("unit", [True, False])
@pytest.mark.parametrize("dims", [(6, 6, 6), (7, 5, 4)])
def test_random_closed_fields_are_closed_oriented_manifolds(dims, unit):
    for seed in range(3):
        total, weight = TC.shell_field(dims, 10 * seed + dims[0], unit)
        counts, raw = check_extract(total, weight, dims, TC.BOUNDS, 2)
        tris, dropped = TS.drop_degenerate(raw)
        edges = MC.mesh_edges(tris)
        assert len(tris) > 0 and dropped == 0 and edges.boundary == 0 and edges.non_manifold == 0
        assert TC.closed_and_oriented(tris) and TC.signed_volume(tris) > 0.0
        assert int(counts.max()) <= TS.CELL_MAX_TRIS


def test_sphere():
    n = 17
    total, weight = TC.sphere_field(n)
    _, raw = check_extract(total, weight, (n, n, n), TC.UNIT, 1)
    tris, dropped = TS.drop_degenerate(raw)
    edges = MC.mesh_edges(tris)
    assert dropped == 0 and edges.boundary == 0 and edges.non_manifold == 0 and TC.closed_and_oriented(tris)
    assert TC.euler_characteristic(tris) == 2
    # a vertex lies on a lattice edge (a cell's side, face diagonal or diagonal) whose ends straddle the sphere
    dist = np.abs(np.linalg.norm(tris.reshape(-1, 3).astype(np.float64) - np.array(TC.SPHERE_CENTRE), axis=1) - TC.SPHERE_RADIUS)
    assert dist.max() <= np.sqrt(3.0) / n
    volume = TC.signed_volume(tris)
    assert 0.0 < volume < 4.0 / 3.0 * np.pi * (TC.SPHERE_RADIUS + np.sqrt(3.0) / n) ** 3


# ------------------------------------------------------------------------------------------------ end to end
def test_box_end_to_end_on_the_host(tmp_path):
    tris, info, _, scan = TC.box_end_to_end("host", tmp_path)
    again, info2 = TS.tsdf_mesh(list(scan.depth), scan.cameras, grid=48, backend="host",
                                budget_bytes=5 * 60 * 80 * 4)              # chunks of 5, 5 and 2 views
    assert TC.same_bits(again, tris) and info2 == info


def test_mixed_sizes_and_bad_maps_on_the_host():
    small, large = SS.solid_scan("box", 3, 24, 32, backend="host"), SS.solid_scan("box", 2, 33, 65, backend="host")
    cams = [small.cameras[0], large.cameras[0], small.cameras[1], large.cameras[1], small.cameras[2]]
    maps = [small.depth[0], large.depth[0], small.depth[1], large.depth[1], small.depth[2]]
    tris, info = TS.tsdf_mesh(maps, cams, grid=12, min_weight=1, backend="host")
    ordered, info_o = TS.tsdf_mesh([maps[k] for k in (0, 2, 4, 1, 3)], [cams[k] for k in (0, 2, 4, 1, 3)], grid=12, min_weight=1,
                                   backend="host")
    assert len(tris) > 0 and TC.same_bits(tris, ordered) and info == info_o    # grouped by size, sizes in first-seen order
    with pytest.raises(ValueError, match="cameras and"):
        TS.tsdf_mesh(maps[:4], cams, backend="host")
    with pytest.raises(ValueError, match="must be a float"):
        TS.tsdf_mesh([np.ones(m.shape, np.int32) for m in maps], cams, backend="host")
    with pytest.raises(ValueError, match="must be a float"):
        TS.tsdf_mesh(maps[1:] + maps[:1], cams, backend="host")       # a map of another camera's size


# ------------------------------------------------------------------------------------------------ the tool and the header
def test_tool_writes_the_mesh_and_its_record(tmp_path):
    from curve_gaussian_amd import tsdf_mesh as TOOL
    scan = SS.solid_scan("box", 6, 30, 40, backend="host")
    root = str(tmp_path / "scan")
    SS.write_solid_scan(root, scan, depth=True)
    depth_dir = "depth"
    assert TOOL.main(["--scan", root, "--depth_dir", depth_dir, "--grid", "16", "--backend", "host", "--min_weight", "1"]) == 0
    ply, record = os.path.join(root, "tsdf_mesh.ply"), os.path.join(root, "tsdf_mesh.json")
    tris = EO.read_occluder(ply)
    report = json.load(open(record))
    want, info = TS.tsdf_mesh(list(scan.depth), scan.cameras, grid=16, min_weight=1, backend="host")
    assert isinstance(tris, np.ndarray) and TC.same_bits(tris, want) and report["info"] == json.loads(json.dumps(info))
    assert report["recommended_slack"] == info["recommended_slack"] and report["grid"] == 16 and report["min_weight"] == 1
    assert report["trunc"] == 4.0 / 16 and report["depth_dir"] == depth_dir and report["backend"] == "host"
    with pytest.raises(FileExistsError):
        TOOL.main(["--scan", root, "--depth_dir", depth_dir, "--grid", "16", "--backend", "host"])
    out = str(tmp_path / "other" / "m.ply")
    assert TOOL.main(["--scan", root, "--depth_dir", depth_dir, "--grid", "8", "--trunc", "0.3", "--backend", "host", "--out", out,
                      "--bounds", "0", "0", "0", "1", "1", "2"]) == 0
    other = json.load(open(os.path.splitext(out)[0] + ".json"))
    assert other["trunc"] == 0.3 and other["info"]["dims"] == [4, 4, 8] and other["bounds"] == [[0, 0, 0], [1, 1, 2]]


def test_header_library_and_layer_agree():
    header = open(os.path.join(ROOT, "include", "curvegs.h")).read()
    assert int(re.search(r"#define CGS_TSDF_MAX_WEIGHT (\d+)", header).group(1)) == _lib.TSDF_MAX_WEIGHT == TS.MAX_WEIGHT
    lib = _lib.load()
    for name, nargs in (("cgs_tsdf_integrate", 16), ("cgs_tsdf_mesh_count", 8), ("cgs_tsdf_mesh_emit", 12)):
        assert hasattr(lib, name) and len(_lib.SIGNATURES[name][1]) == nargs
    # the derived cases of the layer and of the brute force say the same, and a quad is split along E(i,k) -- E(j,l)
    for m in range(16):
        inside = [bool((m >> x) & 1) for x in range(4)]
        assert [tuple(t) for t in TC.case_triangles(inside, False)] == [tuple(t) for t in TS.CASES[m]]
    assert TS.CASES[0b0011] == [((0, 2), (0, 3), (1, 3)), ((0, 2), (1, 3), (1, 2))]
    assert [q for q, _ in TS.TETS] == [q for q, _ in TC.tetrahedra()] and [o for _, o in TS.TETS] == [False, True, True, False, False, True]
