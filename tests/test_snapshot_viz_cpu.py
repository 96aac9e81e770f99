"""CPU: the inspection files of a snapshot (scene/snapshot_viz.py; the reference's draw_curve / draw_ellipsoids).  The
sphere template's invariants, the colours and sample points against tests/golden/snapshot_viz.npz (made by running the
reference's own code, make_snapshot_viz_golden.py), the layout of both PLY writers read back, and the training driver's
``draw`` option on the recording fakes."""
import json
import math
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

import ellipsoid_ref64 as E
import train_fakes as TF

HERE = os.path.dirname(os.path.abspath(__file__))
G = np.load(os.path.join(HERE, "golden", "snapshot_viz.npz"))


# ------------------------------------------------------------------------------------------------ sphere template
@pytest.mark.parametrize("res", [2, 3, 5, 10, 17])
@pytest.mark.parametrize("radius", [1.2, 0.5])
def test_sphere_template_is_a_closed_outward_sphere(res, radius):
    from curve_gaussian_amd.scene.snapshot_viz import sphere_template
    v, f = sphere_template(radius, res)
    assert v.dtype == np.float64 and f.dtype == np.int32
    assert v.shape == (2 + 2 * res * (res - 1), 3) and f.shape == (4 * res * (res - 1), 3)
    assert tuple(v[0]) == (0.0, 0.0, radius) and tuple(v[1]) == (0.0, 0.0, -radius)
    np.testing.assert_allclose(np.linalg.norm(v, axis=1), radius, rtol=1e-15, atol=0)
    assert f.min() == 0 and f.max() == len(v) - 1 and len(np.unique(f)) == len(v)
    assert all(len(set(t)) == 3 for t in f.tolist())
    # every directed edge once, and its reverse once: closed, two triangles per edge, consistent winding
    directed = [(int(t[a]), int(t[(a + 1) % 3])) for t in f for a in range(3)]
    assert len(set(directed)) == len(directed)
    assert set(directed) == {(b, a) for a, b in directed}
    # outward: every normal points away from the centre, and the enclosed volume is positive
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    n = np.cross(b - a, c - a)
    assert (np.einsum("ij,ij->i", n, (a + b + c) / 3) > 0).all()
    vol = np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6
    assert 0 < vol < 4 / 3 * math.pi * radius ** 3
    assert len(v) - len(f) / 2 == 2                              # Euler: V - E + F = 2 with E = 3F/2


def test_resolution_ten_has_the_issue_record_sizes():
    from curve_gaussian_amd.scene.snapshot_viz import FACE_RECORD, VERTEX_RECORD, sphere_template
    v, f = sphere_template()
    assert (len(v), len(f)) == (182, 360)
    assert len(v) * VERTEX_RECORD + len(f) * FACE_RECORD == 9594


# ------------------------------------------------------------------------------------------------ the fixture
def _cpu_model():
    from curve_gaussian_amd.scene import GaussianCurveModel
    g = object.__new__(GaussianCurveModel)
    g._curve_points = torch.from_numpy(G["curve_points"])
    g.is_bezier = torch.from_numpy(G["is_bezier"])
    return g


def test_fixture_file_names_and_counts():
    step = int(G["step"])
    assert list(G["files"]) == [f"curve_step{step}.ply", f"ellipsoids_step{step}.ply"]
    P = G["is_bezier"].shape[0] * int(G["n_gaussians"])
    assert tuple(G["mesh_counts"]) == (182 * P, 360 * P)


def test_curve_sample_points_equal_the_reference():
    from curve_gaussian_amd.scene.snapshot_viz import curve_sample_points
    pts = curve_sample_points(_cpu_model(), int(G["num_sample"])).numpy()
    assert pts.dtype == G["curve_sample_points"].dtype
    assert np.array_equal(pts, G["curve_sample_points"])


def test_curve_colours_equal_the_reference():
    from curve_gaussian_amd.scene.snapshot_viz import curve_colors
    cols = curve_colors(G["is_bezier"].shape[0], seed=0).repeat_interleave(int(G["num_sample"]), 0).numpy()
    assert np.array_equal(cols, G["curve_point_colors"])


def test_splat_colours_equal_the_reference():
    from curve_gaussian_amd.scene.snapshot_viz import splat_colors
    cols = splat_colors(torch.from_numpy(G["is_bezier"]), torch.from_numpy(G["mask"]), int(G["n_gaussians"]), 0).numpy()
    assert np.array_equal(np.clip(cols, 0, 1), G["splat_color"])
    m = int(G["n_gaussians"])
    lines = np.repeat(~G["is_bezier"], m)
    off = (1 / (1 + np.exp(-G["mask"].reshape(-1).astype(np.float64)))) < 0.01
    assert off.any() and (lines & ~off).any() and (lines & off).any()
    assert (G["splat_color"][off] == 1).all() and (G["splat_color"][lines & ~off] == 0).all()


def test_splat_inputs_are_the_reference_accessors():
    """The reference hands Open3D get_xyz / get_rotation as they are, and scales the template by get_scaling: the
    kernel's first arithmetic step (p = template * (double)s) is the reference's product, bit for bit."""
    from curve_gaussian_amd.scene.snapshot_viz import sphere_template
    assert np.array_equal(G["splat_center"], G["xyz"])
    assert np.array_equal(G["splat_quaternion"], G["rotation"])
    tv, _ = sphere_template(float(G["radius"]), int(G["resolution"]))
    want = tv[None] * G["scaling"].astype(np.float64)[:, None, :]
    assert np.array_equal(G["splat_scaled_vertices"], want)


def test_ref64_positions_rotate_and_move_the_scaled_template():
    from curve_gaussian_amd.scene.snapshot_viz import sphere_template
    tv, _ = sphere_template()
    pos = E.vertex_positions(G["xyz"], G["rotation"], G["scaling"], tv)
    q = G["rotation"].astype(np.float64)
    w, x, y, z = q.T
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                  2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                  2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1).reshape(-1, 3, 3)
    want = np.einsum("pij,pkj->pki", R, G["splat_scaled_vertices"]) + G["xyz"].astype(np.float64)[:, None]
    np.testing.assert_allclose(pos, want, rtol=0, atol=1e-15)


def _exact_u8(c):
    if c != c:
        return 0
    f = Fraction(min(1.0, max(0.0, float(c)))) * 255
    fl = f.numerator // f.denominator
    return fl + (f - fl >= Fraction(1, 2))


def test_colour_bytes_round_half_away_from_zero():
    from curve_gaussian_amd.scene.snapshot_viz import _color_u8
    half = [np.float32((k + 0.5) / 255) for k in range(255)]
    edge = [np.nextafter(h, np.float32(-1)) for h in half] + [np.nextafter(h, np.float32(2)) for h in half]
    c = np.array(half + edge + [-1.0, -0.0, 0.0, 1.0, 1.5, np.inf, -np.inf, np.nan] + list(G["splat_color"].ravel())
                 + list(G["curve_point_colors"].ravel()), np.float32)
    want = np.array([_exact_u8(v) for v in c], np.uint8)
    assert np.array_equal(_color_u8(c), want)
    assert np.array_equal(E.color_u8(c), want)


# ------------------------------------------------------------------------------------------------ writers
def test_curve_point_writer_layout(tmp_path):
    from curve_gaussian_amd.scene.snapshot_viz import write_curve_points
    p, c = G["curve_sample_points"], G["curve_point_colors"]
    path = tmp_path / "curve.ply"
    write_curve_points(str(path), torch.from_numpy(p), torch.from_numpy(c))
    lines, el, body = E.read_ply(str(path))
    assert lines == ["ply", "format ascii 1.0", f"element vertex {len(p)}", "property double x", "property double y",
                     "property double z", "property uchar red", "property uchar green", "property uchar blue",
                     "end_header"]
    rows = body.decode("ascii").splitlines()
    assert len(rows) == len(p) and body.endswith(b"\n")
    vals = np.array([r.split() for r in rows])
    assert np.array_equal(vals[:, :3].astype(np.float64).astype(np.float32), p)      # %.9g reads back exactly
    assert np.array_equal(vals[:, 3:].astype(np.int64), E.color_u8(c).astype(np.int64))


def test_curve_point_writer_empty(tmp_path):
    from curve_gaussian_amd.scene.snapshot_viz import write_curve_points
    path = tmp_path / "empty.ply"
    write_curve_points(str(path), np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32))
    lines, el, body = E.read_ply(str(path))
    assert el["vertex"][0] == 0 and body == b""


def test_mesh_header_and_body_layout(tmp_path):
    """The header write_ellipsoid_mesh writes, followed by a body of the restated records, reads back as the records."""
    from curve_gaussian_amd.scene.snapshot_viz import _header, sphere_template
    tv, tf = sphere_template()
    P = G["xyz"].shape[0]
    head = _header("binary_little_endian", P * 182, P * 360)
    assert head.decode().splitlines() == [
        "ply", "format binary_little_endian 1.0", f"element vertex {P * 182}", "property double x", "property double y",
        "property double z", "property uchar red", "property uchar green", "property uchar blue",
        f"element face {P * 360}", "property list uchar int vertex_indices", "end_header"]
    body = E.mesh_body(G["xyz"], G["rotation"], G["scaling"], G["splat_color"], tv, tf)
    assert len(body) == P * 9594
    f = tmp_path / "layout.ply"
    f.write_bytes(head + body)
    v, fc = E.read_mesh(str(f))
    assert (fc["n"] == 3).all()
    tri = np.stack([fc["a"], fc["b"], fc["c"]], 1).reshape(P, 360, 3)
    assert np.array_equal(tri - (np.arange(P) * 182)[:, None, None], np.broadcast_to(tf, (P, 360, 3)))
    x = v["x"].reshape(P, 182)
    assert np.array_equal(x[:, 0], E.vertex_positions(G["xyz"], G["rotation"], G["scaling"], tv)[:, 0, 0])


def test_mesh_writer_refuses_cpu_tensors(tmp_path):
    from curve_gaussian_amd import _lib as L
    from curve_gaussian_amd.scene.snapshot_viz import write_ellipsoid_mesh
    z = torch.zeros(2, 3)
    with pytest.raises(L.CurveGSError, match="GPU tensor"):
        write_ellipsoid_mesh(str(tmp_path / "m.ply"), z, torch.zeros(2, 4), z, z)


# ------------------------------------------------------------------------------------------------ the driver
SCHEDULE = json.load(open(os.path.join(HERE, "golden", "train_schedule.json")))
GPU_OVERRIDES = dict(iterations=5000, densify_from_iter=100, densification_interval=200, densify_until_iter=1000,
                     opacity_reset_interval=500)


def _run(opt, lists, tmp_path, draw):
    from curve_gaussian_amd import train as T
    rec = TF.Recorder()
    model = TF.FakeModel(rec)
    scene = TF.FakeScene(rec, model)
    step = TF.FakeStep(rec, model, opt.densify_until_iter)
    dataset = T.ModelParams(source_path="scan", model_path=str(tmp_path / "out"))
    saves = list(lists["save"]) + [opt.iterations]
    out = T.training(dataset, opt, lists["test"], saves, lists["checkpoint"], None, quiet=True, scene=(scene, model),
                     step=step, report=lambda it, tests, sc, bg: rec.add("report"),
                     save_ply=lambda g, path, it: rec.add("save"), save_checkpoint=lambda obj, path: rec.add("checkpoint"),
                     export=lambda g, d, o: rec.add("export"), draw=draw)
    return rec.log, out, saves


@pytest.mark.parametrize("run", ["defaults", "gpu_options"])
def test_driver_draws_after_every_save(run, tmp_path):
    from curve_gaussian_amd import train as T
    opt = T.OptimizationParams(**(GPU_OVERRIDES if run == "gpu_options" else {}))
    g = SCHEDULE["runs"][run]
    log, out, saves = _run(opt, g["lists"], tmp_path, draw=True)
    draws = [(i, e) for i, e in enumerate(log) if e[1].startswith("draw_")]
    saved = sorted({e[0] for e in log if e[1] == "save"})
    assert saved == sorted(set(saves))
    assert [e for _, e in draws] == [[it, name] for it in saved for name in ("draw_curve", "draw_ellipsoids")]
    for i, e in draws:
        prev = log[i - 1] if e[1] == "draw_curve" else log[i - 2]
        assert prev == [e[0], "save"]
    # the schedule and the driver's own events are those of a run without drawing
    norm = TF.compress(TF.normalise(log))
    assert norm["events"] == g["log"]["events"] and norm["plain_steps"] == g["log"]["plain_steps"]
    log0, out0, _ = _run(opt, g["lists"], tmp_path, draw=False)
    assert not any(e[1].startswith("draw_") for e in log0)
    assert out["events"] == out0["events"]


def test_command_line_option():
    from curve_gaussian_amd import train as T
    assert T.parse_args(["-s", "x", "-m", "y", "--draw_snapshots"])[2].draw_snapshots is True
    assert T.parse_args(["-s", "x", "-m", "y"])[2].draw_snapshots is False
