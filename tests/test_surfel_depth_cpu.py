"""CPU: the surfel z-buffer (cgs_surfel_depth, include/curvegs.h) on the host back end of ops.edge_occlusion against the brute
force of surfel_cases.py, bit for bit -- one case per branch of the rule --, the readers and writers of point-cloud
occluders, what ChunkDepth does with one, and the surfel gate held against the mesh gate on the sampled box and cylinder.

The gate comparison (profiles/surfel_depth.md has the same counts): 6 views of 60 x 80, surfel_cloud at spacing 0.01, radii
from surfel_radii with the shipped factor.  No pixel the mesh covers is empty in the cloud's z-buffer, and no (sample, view)
that the mesh gate hides is seen by the surfel gate: those two are conditions.  The surplus -- pairs only the surfel gate
hides, because a disk overhangs a silhouette by up to its radius -- is a measurement of a deterministic pipeline and is
asserted exactly: 207 of 71,952 seen pairs on the box, 226 of 45,216 on the cylinder."""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest
import torch

import surfel_cases as C
from curve_gaussian_amd.edge_extraction import reprojection as R
from curve_gaussian_amd.edge_extraction import support as SUP
from curve_gaussian_amd.ops import edge_occlusion as EO
from curve_gaussian_amd.scene import solid_scan as SS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SURPLUS = {"box": (207, 71952), "cylinder": (226, 45216)}     # (pairs only the surfel gate hides, seen pairs)


def host(pts, nrm, rad, K, M, H, W, window=0):
    return EO.surfel_depth(EO.Surfels(pts, nrm, rad), K, M, H, W, window=window, backend="host").numpy()


# ------------------------------------------------------------------------------------------------ the rule
@pytest.mark.parametrize("normals", [True, False], ids=["normals", "normals_none"])
@pytest.mark.parametrize("H, W", C.SIZES)
def test_host_back_end_equals_the_brute_force(H, W, normals):
    pts, nrm, rad = C.special(normals=normals)
    K, M = C.cameras(C.VIEWS, H, W)
    want = C.zbuffer_brute(pts, nrm, rad, K, M, H, W)
    got = host(pts, nrm, rad, K, M, H, W)
    assert got.dtype == np.float32 and C.same_bits(got, want)
    assert np.isfinite(want[0]).all(), "whole_image covers camera 0's image"
    if (H, W) == C.SIZES[-1]:
        assert np.isfinite(want[2]).any() and not np.isfinite(want[2]).all(), "a view with and without surface"


@pytest.mark.parametrize("name", list(C.SPECIAL))
def test_every_branch_on_its_own(name):
    H, W = C.SIZES[-1]
    K, M = C.cameras(C.VIEWS, H, W)
    pts, nrm, rad = C.special([name])
    want = C.zbuffer_brute(pts, nrm, rad, K, M, H, W)
    assert C.same_bits(host(pts, nrm, rad, K, M, H, W), want)
    covered = int(np.isfinite(want[0]).sum())
    if name in C.STORES_NOTHING:
        assert covered == 0, name            # (camera 0, which the case is built in; the others see it as they see it)
    elif name == "sub_pixel_one":
        assert covered == 1 and want[0, 4, 28] == 1.0
    elif name in ("whole_image", "just_in_front"):
        assert covered == H * W
    elif name.startswith("over_"):
        assert 0 < covered < 16, "partly outside the image"
    else:
        assert covered > 1


def test_two_sided_scale_free_and_coincident():
    H, W = C.SIZES[-1]
    K, M = C.cameras(C.VIEWS, H, W)
    pts, nrm, rad = C.special()
    base = host(pts, nrm, rad, K, M, H, W)
    assert C.same_bits(base, host(pts, -nrm, rad, K, M, H, W)), "the disk is two-sided: -n gives -num / -den"
    # a normal of length 7 (times its own length): the surfels whose normals are small integers, so that 7 n is exact in
    # float32 and the DIRECTION is the same; num and den then round on their own, which never reaches the float32 depth here
    names = [n for n, (_, normal, _) in C.SPECIAL.items() if all(float(x) == int(x) for x in normal if x == x)]
    assert len(names) >= 15 and "tilted" in names and "just_in_front" in names
    pts, nrm, rad = C.special(names)
    assert C.same_bits(host(pts, nrm, rad, K, M, H, W), host(pts, nrm * np.float32(7.0), rad, K, M, H, W))
    # two coincident surfels are one
    one, two = C.special(["coincident_a"]), C.special(["coincident_a", "coincident_b"])
    assert C.same_bits(host(*one, K, M, H, W), host(*two, K, M, H, W))
    # c2 - r == 0 is dropped, one float32 step less is drawn
    assert not np.isfinite(host(*C.special(["touches_plane"]), K, M, H, W)[0]).any()
    assert np.isfinite(host(*C.special(["just_in_front"]), K, M, H, W)[0]).all()


def test_no_surfels_and_no_views():
    K, M = C.cameras(C.VIEWS, 5, 7)
    empty = EO.Surfels(np.zeros((0, 3), np.float32), None, np.zeros((0,), np.float32))
    out = EO.surfel_depth(empty, K, M, 5, 7, backend="host")
    assert tuple(out.shape) == (C.VIEWS, 5, 7) and out.dtype == torch.float32 and bool(torch.isposinf(out).all())
    pts, nrm, rad = C.special()
    out = EO.surfel_depth(EO.Surfels(pts, nrm, rad), K[:0], M[:0], 5, 7, backend="host")
    assert tuple(out.shape) == (0, 5, 7)
    with pytest.raises(ValueError, match=r"radii \[26\]"):
        EO.surfel_depth(EO.Surfels(pts, nrm, rad[:-1]), K, M, 5, 7, backend="host")
    with pytest.raises(ValueError, match="height and width"):
        EO.surfel_depth(EO.Surfels(pts, nrm, rad), K, M, 0, 7, backend="host")


def test_the_order_of_the_points_does_not_show():
    H, W = C.WAVE_SIZE
    K, M = C.cameras(C.VIEWS, H, W)
    pts, nrm, rad = C.wave_cloud(257)
    perm = np.random.default_rng(3).permutation(len(pts))
    a = host(pts, nrm, rad, K, M, H, W)
    assert C.same_bits(a, host(pts[perm], nrm[perm], rad[perm], K, M, H, W))
    assert C.same_bits(a, C.zbuffer_brute(pts, nrm, rad, K, M, H, W)), "small and large disks mixed: the GPU test's cloud"
    # the window maximum behind it is depth_window_max's
    assert C.same_bits(host(pts, nrm, rad, K, M, H, W, window=1), EO.depth_window_max(a, 1, backend="host").numpy())


def test_the_host_back_end_works_in_runs(monkeypatch):
    """The host back end holds SURFEL_HOST_PAIRS (surfel, pixel) pairs at a time: the runs do not show."""
    H, W = C.SIZES[-1]
    K, M = C.cameras(C.VIEWS, H, W)
    pts, nrm, rad = C.special()
    whole = host(pts, nrm, rad, K, M, H, W)
    monkeypatch.setattr(EO, "SURFEL_HOST_PAIRS", 7)
    assert C.same_bits(whole, host(pts, nrm, rad, K, M, H, W))


# ------------------------------------------------------------------------------------------------ readers and writers
def _write_ply(path, fmt, cols, faces=None):
    """A vertex table {name: array} as an ascii or binary little-endian PLY; faces: None (no element), or a count of 0."""
    names = list(cols)
    n = len(cols[names[0]])
    head = f"ply\nformat {fmt} 1.0\nelement vertex {n}\n" + "".join(f"property float {k}\n" for k in names)
    if faces is not None:
        head += f"element face {faces}\nproperty list uchar int vertex_indices\n"
    table = np.stack([np.asarray(cols[k], np.float32) for k in names], 1)
    with open(path, "wb") as f:
        f.write((head + "end_header\n").encode("ascii"))
        if fmt == "ascii":
            f.write("".join(" ".join(repr(float(x)) for x in row) + "\n" for row in table).encode("ascii"))
        else:
            f.write(np.ascontiguousarray(table, "<f4").tobytes())


@pytest.mark.parametrize("fmt", ["ascii", "binary_little_endian"])
@pytest.mark.parametrize("with_normals", [True, False])
@pytest.mark.parametrize("with_radius", [True, False])
def test_read_occluder_on_a_point_cloud(tmp_path, fmt, with_normals, with_radius):
    pts, nrm, rad = C.wave_cloud(65)
    rad = np.abs(rad)
    cols = {"x": pts[:, 0], "y": pts[:, 1], "z": pts[:, 2]}
    if with_normals:
        cols.update({"nx": nrm[:, 0], "ny": nrm[:, 1], "nz": nrm[:, 2]})
    if with_radius:
        cols["radius"] = rad
    path = str(tmp_path / "cloud.ply")
    _write_ply(path, fmt, cols)
    got = EO.read_occluder(path)
    assert isinstance(got, EO.Surfels) and C.same_bits(got.points, pts)
    assert (got.normals is None) if not with_normals else C.same_bits(got.normals, nrm)
    want = rad if with_radius else EO.surfel_radii(pts, backend="host")
    assert C.same_bits(got.radii, want) and got.radii.dtype == np.float32
    if not with_radius:
        assert EO.read_occluder(path, derive_radii=False).radii is None
        assert C.same_bits(EO.read_occluder(path, factor=0.5).radii, EO.surfel_radii(pts, 0.5, backend="host"))
    with pytest.raises(ValueError, match="needs a vertex and a face element"):
        EO.read_triangle_mesh(path)                                       # unchanged: a mesh reader reads meshes


def test_read_occluder_on_face_zero_and_on_meshes(tmp_path):
    pts, nrm, rad = C.wave_cloud(9)
    path = str(tmp_path / "no_faces.ply")
    _write_ply(path, "binary_little_endian", {"x": pts[:, 0], "y": pts[:, 1], "z": pts[:, 2], "radius": rad}, faces=0)
    got = EO.read_occluder(path)
    assert isinstance(got, EO.Surfels) and C.same_bits(got.points, pts) and got.normals is None and C.same_bits(got.radii, rad)
    tris, _ = SS.solid_geometry("box")
    mesh = str(tmp_path / "mesh.ply")
    EO.write_triangle_ply(mesh, tris)
    got = EO.read_occluder(mesh)
    assert isinstance(got, np.ndarray) and C.same_bits(got, tris)
    obj = str(tmp_path / "mesh.obj")
    with open(obj, "w") as f:
        f.write("v 0 0 0\nv 1 0 0\nv 0 1 0\nf 1 2 3\n")
    assert C.same_bits(EO.read_occluder(obj), EO.read_triangle_mesh(obj))
    with pytest.raises(ValueError, match="unknown mesh format"):
        EO.read_occluder(str(tmp_path / "cloud.xyz"))


def test_surfel_cloud_round_trips_through_a_file(tmp_path):
    tris, _ = SS.solid_geometry("box")
    pts, nrm = SS.surfel_cloud(tris, 0.05)
    again = SS.surfel_cloud(tris, 0.05)
    assert C.same_bits(pts, again[0]) and C.same_bits(nrm, again[1]), "deterministic"
    assert pts.dtype == np.float32 and pts.shape == nrm.shape and 400 < len(pts) < 1200
    assert np.allclose(np.linalg.norm(nrm, axis=1), 1.0, atol=1e-6)
    lo, hi = tris.reshape(-1, 3).min(0), tris.reshape(-1, 3).max(0)
    assert (pts >= lo).all() and (pts <= hi).all() and ((pts == lo) | (pts == hi)).any(1).all(), "on the box's faces"
    gaps = np.linalg.norm(pts[:, None, :] - pts[None, :, :], axis=2) + np.eye(len(pts))
    assert gaps.min() >= SS.CLOUD_MIN_GAP * 0.05 * (1 - 1e-6)
    rad = EO.surfel_radii(pts, backend="host")
    path = str(tmp_path / "cloud.ply")
    EO.write_surfel_ply(path, EO.Surfels(pts, nrm, rad))
    got = EO.read_occluder(path)
    assert C.same_bits(got.points, pts) and C.same_bits(got.normals, nrm) and C.same_bits(got.radii, rad)
    assert len(SS.surfel_cloud(np.zeros((2, 3, 3), np.float32), 0.05)[0]) == 0, "no area, no sample"
    with pytest.raises(ValueError, match="spacing"):
        SS.surfel_cloud(tris, 0.0)


def test_surfel_radii_on_the_host():
    rng = np.random.default_rng(5)
    pts = rng.uniform(0, 1, (300, 3)).astype(np.float32)
    pts[7] = (40.0, 40.0, 40.0)                                            # a lone outlier
    r = EO.surfel_radii(pts, backend="host")
    d2 = ((pts[:, None, :].astype(np.float64) - pts[None, :, :].astype(np.float64)) ** 2).sum(2)
    np.fill_diagonal(d2, np.inf)
    exact = np.sqrt(np.sort(d2, 1)[:, :3].mean(1))
    cap = EO.SURFEL_RADIUS_CAP * np.median(exact)
    assert exact[7] > 10 * cap, "the outlier's own neighbours are far"
    assert r.dtype == np.float32 and np.allclose(r, np.minimum(exact, cap), rtol=1e-6, atol=0.0) and abs(r[7] - cap) <= 1e-6 * cap
    assert np.allclose(EO.surfel_radii(pts, 0.5, backend="host"), 0.5 * r.astype(np.float64), rtol=1e-6)
    assert np.isposinf(EO.surfel_radii(pts[:3], backend="host")).all(), "fewer than 4 points have no 3 neighbours"
    with pytest.raises(ValueError, match="factor"):
        EO.surfel_radii(pts, 0.0, backend="host")
    assert EO.SURFEL_RADIUS_FACTOR == 1.0 and EO.SURFEL_RADIUS_CAP == 4.0


# ------------------------------------------------------------------------------------------------ ChunkDepth
def test_chunk_depth_takes_surfels_and_rejects_what_needs_a_mesh(tmp_path):
    s = SS.solid_scan("box", 2, 12, 16, backend="host")
    pts, nrm = SS.surfel_cloud(s.tris, 0.05)
    cloud = EO.Surfels(pts, nrm, EO.surfel_radii(pts, backend="host"))
    from curve_gaussian_amd.ops.view_chunks import camera_arrays
    K, M = camera_arrays(s.cameras)
    gate = EO.ChunkDepth("t", s.cameras, occluder=cloud)
    assert gate.gated and gate.tris is None and gate.bytes_per_pixel == 8
    assert gate.settings() == {"occluder": True, "depth_slack": EO.DEPTH_SLACK, "depth_window": EO.DEPTH_WINDOW,
                               "occluder_kind": "surfels", "surfels": len(pts)}
    planes = gate.to("host").planes(12, 16, [0, 1], K, M)
    assert C.same_bits(planes.numpy(), EO.surfel_depth(cloud, K, M, 12, 16, backend="host").numpy())
    # a file with radii, and one without: the factor is recorded when the radii were derived
    with_r, without = str(tmp_path / "with.ply"), str(tmp_path / "without.ply")
    EO.write_surfel_ply(with_r, cloud)
    _write_ply(without, "ascii", {"x": pts[:, 0], "y": pts[:, 1], "z": pts[:, 2], "nx": nrm[:, 0], "ny": nrm[:, 1], "nz": nrm[:, 2]})
    g1, g2 = EO.ChunkDepth("t", s.cameras, occluder=with_r), EO.ChunkDepth("t", s.cameras, occluder=without)
    assert g1.settings()["occluder"] == with_r and "surfel_radius_factor" not in g1.settings()
    assert g2.settings() == {"occluder": without, "depth_slack": EO.DEPTH_SLACK, "depth_window": EO.DEPTH_WINDOW,
                             "occluder_kind": "surfels", "surfels": len(pts), "surfel_radius_factor": EO.SURFEL_RADIUS_FACTOR}
    for g in (g1, g2):
        assert C.same_bits(g.to("host").planes(12, 16, [0, 1], K, M).numpy(), planes.numpy())
    for occluder in (cloud, with_r):
        with pytest.raises(ValueError, match="near_clip takes a mesh"):
            EO.ChunkDepth("t", s.cameras, occluder=occluder, near_clip=EO.NEAR_CLIP)
        with pytest.raises(ValueError, match="ignore_contours takes a mesh"):
            R.score_edges(s.edges, s.cameras, s.maps, "PidiNet", backend="host", occluder=occluder, ignore_contours=True)
    with pytest.raises(ValueError, match="surfels must be a Surfels"):
        EO.surfel_depth((pts, nrm, cloud.radii), K, M, 12, 16, backend="host")


def test_a_meshs_settings_are_what_they_were(tmp_path):
    s = SS.solid_scan("box", 2, 12, 16, backend="host")
    assert EO.ChunkDepth("t", s.cameras, occluder=s.tris).settings() == {"occluder": True, "depth_slack": 0.001, "depth_window": 1}
    mesh = str(tmp_path / "mesh.ply")
    EO.write_triangle_ply(mesh, s.tris)
    g = EO.ChunkDepth("t", s.cameras, occluder=mesh, depth_slack=0.002, depth_window=2, near_clip=0.02)
    assert g.settings() == {"occluder": mesh, "depth_slack": 0.002, "depth_window": 2, "near_clip": 0.02}
    assert list(g.settings()) == ["occluder", "depth_slack", "depth_window", "near_clip"] and g.surfels is None
    assert EO.ChunkDepth("t", s.cameras, depth_maps=list(s.depth)).settings() == {"depth_maps": True, "depth_slack": 0.001,
                                                                                 "depth_window": 1}
    assert EO.ChunkDepth("t", s.cameras).settings() == {}


# ------------------------------------------------------------------------------------------------ against the mesh gate
@pytest.mark.parametrize("shape", ["box", "cylinder"])
def test_the_surfel_gate_hides_what_the_mesh_gate_hides(shape):
    g = C.gate_fixture(shape)
    holes = np.isfinite(g["raw_mesh"]) & ~np.isfinite(g["raw_cloud"])
    mesh_only = g["hidden_mesh"] & ~g["hidden_cloud"]
    surplus = g["hidden_cloud"] & ~g["hidden_mesh"]
    print(f"\n   {shape}: {len(g['cloud'][0])} surfels, median radius {float(np.median(g['cloud'][2])):.5f}, holes "
          f"{int(holes.sum())}, seen pairs {int(g['seen'].sum())}, mesh hides {int(g['hidden_mesh'].sum())}, surfels hide "
          f"{int(g['hidden_cloud'].sum())}, mesh-only {int(mesh_only.sum())}, surplus {int(surplus.sum())}")
    assert int(g["hidden_mesh"].sum()) > 10000, "the fixture hides something"
    assert not holes.any(), "(a) no pixel the mesh covers is empty"
    assert not mesh_only.any(), "(b) nothing the mesh gate hides is seen by the surfel gate"
    assert (int(surplus.sum()), int(g["seen"].sum())) == SURPLUS[shape]
    assert not (g["hidden_cloud"] & ~g["seen"]).any()


def test_the_shipped_factor_is_the_smallest_of_its_list_without_a_hole():
    """SURFEL_RADIUS_FACTOR = 1.0: the next smaller of (0.6, 0.8, 1.0, 1.2) leaves a hole in the box."""
    g = C.gate_fixture("box")
    pts, nrm, _ = g["cloud"]
    H, W = C.GATE_SIZE
    smaller = EO.Surfels(pts, nrm, EO.surfel_radii(pts, 0.8, backend="host"))
    raw = EO.surfel_depth(smaller, g["K"], g["M"], H, W, window=0, backend="host").numpy()
    assert (np.isfinite(g["raw_mesh"]) & ~np.isfinite(raw)).any()


def test_a_written_scan_scores_with_its_cloud_as_with_its_mesh(tmp_path, capsys):
    """write_solid_scan(cloud=) -> score_scan / the support tool with --occluder cloud.ply on the ground truth."""
    H, W = C.GATE_SIZE
    scan = SS.solid_scan("box", C.GATE_VIEWS, H, W, backend="host")
    plain, with_cloud = tmp_path / "plain" / "box", tmp_path / "data" / "box"
    SS.write_solid_scan(str(plain), scan)
    SS.write_solid_scan(str(with_cloud), scan, cloud=C.GATE_SPACING)
    assert sorted(os.listdir(with_cloud)) == sorted(os.listdir(plain) + ["cloud.ply"])
    for name in os.listdir(plain):
        if os.path.isfile(plain / name):
            assert (plain / name).read_bytes() == (with_cloud / name).read_bytes(), name
    cloud = EO.read_occluder(str(with_cloud / "cloud.ply"))
    want = C.gate_fixture("box")["cloud"]
    assert all(C.same_bits(a, b) for a, b in zip(cloud, want))
    out = tmp_path / "out"
    os.makedirs(out / "box")
    with open(out / "box" / "parametric_edges.json", "w") as f:
        json.dump(scan.edges, f)
    res = {}
    for occluder in ("mesh.ply", "cloud.ply"):
        res[occluder] = R.score_scan(str(out), str(tmp_path / "data"), "box", detector="PidiNet", backend="host", occluder=occluder)
    mesh, cl = res["mesh.ply"]["aggregate"], res["cloud.ply"]["aggregate"]
    settings = json.loads((out / "box" / R.SCORE_FILE).read_text())["settings"]
    assert settings["occluder_kind"] == "surfels" and settings["surfels"] == len(want[0]) and "surfel_radius_factor" not in settings
    assert "occluder_kind" not in res["mesh.ply"]["settings"]
    surplus, seen = SURPLUS["box"]
    print(f"\n   box, 1 px: mesh precision {mesh['precision'][0]:.6f} recall {mesh['recall'][0]:.6f}; cloud precision "
          f"{cl['precision'][0]:.6f} recall {cl['recall'][0]:.6f}; surplus share {surplus / seen:.6f}")
    assert mesh["precision"][0] == 1.0 == mesh["recall"][0], "the maps were drawn with the mesh"
    assert cl["precision"][0] >= mesh["precision"][0]
    assert abs(cl["recall"][0] - mesh["recall"][0]) <= surplus / seen
    hidden = [sum(row["hidden_points"] for row in r["views"]) for r in (res["mesh.ply"], res["cloud.ply"])]
    assert hidden[1] - hidden[0] == surplus
    # the command lines take the cloud as they take the mesh
    common = ["--base_dir", str(out), "--dataset_dir", str(tmp_path / "data"), "--detector", "PidiNet", "--backend", "host",
              "--occluder", "cloud.ply"]
    assert R.main(common) == 0
    assert json.loads((out / "box" / R.SCORE_FILE).read_text())["settings"]["surfels"] == len(want[0])
    assert SUP.main(common + ["--tolerances", "1", "2", "--keep_tolerance", "1", "--trim"]) == 0
    for n in (SUP.SUPPORT_FILE, SUP.TRIM_FILE):
        got = json.loads((out / "box" / n).read_text())["settings"]
        assert got["occluder_kind"] == "surfels" and got["surfels"] == len(want[0]), n
    with pytest.raises(ValueError, match="near_clip takes a mesh"):
        R.main(common + ["--near_clip"])
    with pytest.raises(ValueError, match="ignore_contours takes a mesh"):
        R.main(common + ["--ignore_contours"])
    capsys.readouterr()


def test_command_lines_write_clouds(tmp_path, capsys):
    from curve_gaussian_amd import surfel_cloud as CLI
    scan_dir = tmp_path / "box"
    assert SS.main(["box", str(scan_dir), "--views", "2", "--height", "12", "--width", "16", "--cloud", "0.05", "--backend", "host"]) == 0
    assert sorted(os.listdir(scan_dir)) == ["cloud.ply", "edge_PidiNet", "gt_edges.json", "mesh.ply", "meta_data.json"]
    cloud = EO.read_occluder(str(scan_dir / "cloud.ply"))
    bare = str(tmp_path / "bare.ply")
    _write_ply(bare, "binary_little_endian", {"x": cloud.points[:, 0], "y": cloud.points[:, 1], "z": cloud.points[:, 2],
                                             "nx": cloud.normals[:, 0], "ny": cloud.normals[:, 1], "nz": cloud.normals[:, 2]})
    out = str(tmp_path / "out.ply")
    assert CLI.main([bare, out, "--backend", "host"]) == 0 and f"{len(cloud.points)} surfels, with normals" in capsys.readouterr().out
    got = EO.read_occluder(out)
    assert all(C.same_bits(a, b) for a, b in zip(got, cloud))
    assert CLI.main([bare, out, "--backend", "host", "--factor", "0.5"]) == 0
    assert C.same_bits(EO.read_occluder(out).radii, EO.surfel_radii(cloud.points, 0.5, backend="host"))
    assert CLI.main([bare, out, "--radius", "0.25"]) == 0
    got = EO.read_occluder(out)
    assert (got.radii == np.float32(0.25)).all() and C.same_bits(got.normals, cloud.normals)
    for bad in ([bare, out, "--radius", "0.1", "--factor", "1"], [bare, out, "--radius", "-1"], [str(scan_dir / "mesh.ply"), out]):
        with pytest.raises(SystemExit):
            CLI.main(bad)
    capsys.readouterr()
    ap = R.parser()
    assert "mesh or point cloud" in ap.format_help()


# ------------------------------------------------------------------------------------------------ the C ABI and the code object
def test_abi_argument_checks_are_pinned():
    """Status and the exact text of cgs_last_error() for every rejection of cgs_surfel_depth; the pointers are dummies that
    are never dereferenced, and no row passes validation with work to do (V = 0 is the only accepted call)."""
    from curve_gaussian_amd import _lib
    from test_edge_occlusion_cpu import _pinned
    lib = _lib.load()
    p = ctypes.c_void_p(1 << 20)

    def surfel(P=3, points=p, normals=p, radii=p, V=2, intr=p, w2c=p, H=4, W=6, depth=p):
        return lib.cgs_surfel_depth(P, points, normals, radii, V, intr, w2c, H, W, depth, None)

    _pinned(lib, "cgs_surfel_depth", "cgs_surfel_depth: invalid argument ", surfel,
            [(dict(P=-1), "(P=-1, V=2)"), (dict(V=-1, H=0), "(P=3, V=-1)"),
             (dict(H=0), "(height=0, width=6; sizes lie in [1, 16384])"),
             (dict(W=16385, V=0), "(height=4, width=16385; sizes lie in [1, 16384])"),
             (dict(points=None), "(NULL pointer; P=3)"), (dict(radii=None, normals=None), "(NULL pointer; P=3)"),
             (dict(intr=None), "(NULL pointer; P=3)"), (dict(w2c=None, V=0), "(NULL pointer; P=3)"),
             (dict(depth=None, P=0), "(NULL pointer; P=0)")],
            [dict(V=0), dict(V=0, normals=None), dict(V=0, P=0, points=None, radii=None, normals=None)])
    i, vp = ctypes.c_int, ctypes.c_void_p
    assert _lib.SIGNATURES["cgs_surfel_depth"] == (i, [i, vp, vp, vp, i, vp, vp, i, i, vp, vp])
    header = open(os.path.join(ROOT, "include", "curvegs.h")).read()
    assert "COVERED iff d2 <= r * r" in header and "The disk is two-sided" in header


def test_the_kernel_uses_no_scratch_memory(tmp_path):
    """k_surfel_depth's metadata record in the device assembly, compiled with the Makefile's flags: no scratch (private
    segment), no spilled register, no LDS."""
    import shutil
    from test_compositor_resources_cpu import CSRC, HIPCC, _makefile_hipflags, _metadata
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("hipcc is not installed here")
    asm = str(tmp_path / "surfel_depth.s")
    subprocess.run([HIPCC, *_makefile_hipflags(), "-S", "--cuda-device-only", "-w", os.path.join(CSRC, "surfel_depth.hip"), "-o", asm],
                   check=True, cwd=str(tmp_path), capture_output=True)
    records = _metadata(open(asm).read())
    for prefix in ("_ZN3cgs14k_surfel_depthE",):
        match = [v for k, v in records.items() if k.startswith(prefix)]
        assert len(match) == 1, prefix
        print(f"\n   {prefix}: {match[0]}")
        assert match[0]["private_segment_fixed_size"] == 0 and match[0]["vgpr_spill_count"] == 0
        assert match[0]["group_segment_fixed_size"] == 0 and match[0]["vgpr_count"] <= 64, "eight waves per SIMD"
