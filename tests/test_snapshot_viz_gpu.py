"""GPU: the ellipsoid mesh kernels (csrc/mesh.hip) byte for byte against the float64 restatement tests/ellipsoid_ref64.py,
chunking, a chunk past 2^31 bytes, the argument checks, draw_curve / draw_ellipsoids on the fixture's model
(tests/golden/snapshot_viz.npz) and ``python -m curve_gaussian_amd.train --draw_snapshots`` end to end."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import ellipsoid_ref64 as E
from test_train_driver_gpu import scan  # noqa: F401  (the synthetic COLMAP scan fixture)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = np.load(os.path.join(ROOT, "tests", "golden", "snapshot_viz.npz"))


def _splats(P, seed):
    """Random splats with planted edge cases: zero, tiny and huge scales; quaternions at and next to +-1, one
    un-normalised and one zero; colours outside [0, 1], NaN and on the rounding boundaries (k + 0.5) / 255."""
    rng = np.random.default_rng(seed)
    xyz = rng.uniform(-3, 3, (P, 3)).astype(np.float32)
    rot = rng.normal(size=(P, 4))
    rot = (rot / np.linalg.norm(rot, axis=1, keepdims=True)).astype(np.float32)
    scale = np.exp(rng.normal(-4, 1.5, (P, 3))).astype(np.float32)
    rgb = rng.uniform(-0.2, 1.2, (P, 3)).astype(np.float32)
    near = lambda *q: np.asarray(q, np.float64) / np.linalg.norm(q)
    planted_rot = [(1, 0, 0, 0), (-1, 0, 0, 0), (0, 0, 0, 1), near(1, 1e-4, -2e-4, 3e-4), near(-1, 3e-7, 0, -1e-7),
                   near(1, 0, 0, 1e-3), (2, 0.5, -1, 0.25), (0, 0, 0, 0)]
    planted_scale = [(0, 0, 0), (1e-30, 1e-38, 1e-45), (1e30, 1, 1e-30), (0, 1, 0), (1, 1, 1)]
    for k, q in enumerate(planted_rot):
        rot[k % P] = q
    for k, s in enumerate(planted_scale):
        scale[(3 * k + 1) % P] = s
    halves = (np.arange(255, dtype=np.float64) + 0.5) / 255
    n = min(P * 3, 255)
    rgb.reshape(-1)[:n] = halves[:n].astype(np.float32)
    rgb[-1] = (np.nan, -0.0, 1.0)
    return xyz, rot, scale, rgb


def _gpu(*a):
    return [torch.from_numpy(np.ascontiguousarray(x)).to(DEV) for x in a]


def _template():
    from curve_gaussian_amd.scene.snapshot_viz import sphere_template
    return sphere_template(1.2, 10)


def _write(path, arrays, **kw):
    from curve_gaussian_amd.scene.snapshot_viz import write_ellipsoid_mesh
    return write_ellipsoid_mesh(str(path), *_gpu(*arrays), **kw)


def test_kernel_bytes_equal_the_float64_restatement(tmp_path):
    arrays = _splats(997, 1)
    tv, tf = _template()
    assert _write(tmp_path / "m.ply", arrays) == (997 * 182, 997 * 360)
    lines, el, body = E.read_ply(str(tmp_path / "m.ply"))
    assert el["vertex"][0] == 997 * 182 and el["face"][0] == 997 * 360
    want = E.mesh_body(*arrays, tv, tf)
    if body != want:
        v, f = E.read_mesh(str(tmp_path / "m.ply"))
        wv = np.frombuffer(want, E.VERTEX, 997 * 182)
        bad = np.nonzero(v != wv)[0]
        pytest.fail(f"{len(bad)} vertex records differ, first {bad[:5]}: {v[bad[:3]]} vs {wv[bad[:3]]}")
    v, f = E.read_mesh(str(tmp_path / "m.ply"))
    assert (v["red"][-182:] == 0).all() and (v["green"][-182:] == 0).all() and (v["blue"][-182:] == 255).all()


@pytest.mark.parametrize("per_pass", [1, 7, None])
def test_every_chunking_writes_the_same_file(tmp_path, per_pass):
    from curve_gaussian_amd.scene.snapshot_viz import EllipsoidMesh
    P = 23
    arrays = _splats(P, 2)
    tv, tf = _template()
    ws = 1 << 30 if per_pass is None else 2 * EllipsoidMesh.chunk_bytes(per_pass, 182 * 27)
    _write(tmp_path / "m.ply", arrays, workspace_bytes=ws)
    _, _, body = E.read_ply(str(tmp_path / "m.ply"))
    assert body == E.mesh_body(*arrays, tv, tf)


def test_too_small_a_workspace_is_refused(tmp_path):
    from curve_gaussian_amd import _lib as L
    with pytest.raises(L.CurveGSError, match="holds no splat"):
        _write(tmp_path / "m.ply", _splats(3, 3), workspace_bytes=4096)


def test_empty_mesh(tmp_path):
    z3 = np.zeros((0, 3), np.float32)
    assert _write(tmp_path / "e.ply", (z3, np.zeros((0, 4), np.float32), z3, z3)) == (0, 0)
    lines, el, body = E.read_ply(str(tmp_path / "e.ply"))
    assert el["vertex"][0] == 0 and el["face"][0] == 0 and body == b""
    assert "property list uchar int vertex_indices" in lines


def test_a_chunk_past_two_gigabytes():
    """One vertex pass of 440 000 splats: 2 162 160 000 bytes, records on both sides of byte 2^31 checked."""
    from curve_gaussian_amd.scene.snapshot_viz import EllipsoidMesh
    P = 440_000
    arrays = _splats(P, 4)
    tv, _ = _template()
    m = EllipsoidMesh(*_gpu(*arrays))
    size = m.chunk_bytes(P, 182 * 27)
    assert size > 2 ** 31
    out = torch.full((size,), 0xAB, dtype=torch.uint8, device=DEV)
    m.vertices_into(out, 0, P)
    r0 = 2 ** 31 // 27
    recs = np.unique(np.concatenate([np.arange(r0 - 40, r0 + 40), np.arange(P * 182 - 40, P * 182),
                                     np.arange(0, 40), np.random.default_rng(5).integers(0, P * 182, 2000)]))
    idx = torch.from_numpy(recs[:, None] * 27 + np.arange(27)[None]).to(DEV)
    got = out[idx.reshape(-1)].cpu().numpy().tobytes()
    splats = np.unique(recs // 182)
    sel = [a[splats] for a in arrays]
    ref = E.vertex_records(*sel, tv).reshape(len(splats), 182)
    pos = {s: i for i, s in enumerate(splats)}
    want = b"".join(ref[pos[r // 182], r % 182].tobytes() for r in recs)
    assert got == want
    assert (out[P * 182 * 27:].cpu().numpy() == 0).all()                      # the last word's padding


def test_argument_checks():
    from curve_gaussian_amd import _lib as L
    lib = L.load()
    vb, fb = ctypes.c_int64(), ctypes.c_int64()
    assert lib.cgs_ellipsoid_mesh_body_bytes(3, 10, ctypes.byref(vb), ctypes.byref(fb)) == 3 * 9594
    assert (vb.value, fb.value) == (3 * 4914, 3 * 4680)
    assert lib.cgs_ellipsoid_mesh_body_bytes(0, 10, None, None) == 0
    for P, res in ((-1, 10), (5, 1), (5, 0)):
        assert lib.cgs_ellipsoid_mesh_body_bytes(P, res, None, None) == -1
    # vertex indices: (first + count) * 182 <= 2^31
    top = 2 ** 31 // 182
    assert lib.cgs_ellipsoid_mesh_body_bytes(top, 10, None, None) > 0
    assert lib.cgs_ellipsoid_mesh_body_bytes(top + 1, 10, None, None) == -1
    assert "int" in L.last_error()
    buf = torch.zeros(8192, dtype=torch.uint8, device=DEV)
    tv, tf = _template()
    xyz, rot, scale, rgb, tvd, tfd = _gpu(*_splats(4, 6), tv, tf)
    s = L.raw_stream(DEV)
    faces = lambda first, count, out=L.ptr(buf), t=L.ptr(tfd): lib.cgs_ellipsoid_mesh_faces(first, count, 182, 360, t,
                                                                                             out, s)
    verts = lambda first, count, out=L.ptr(buf), x=L.ptr(xyz): lib.cgs_ellipsoid_mesh_vertices(
        first, count, x, L.ptr(rot), L.ptr(scale), L.ptr(rgb), 182, L.ptr(tvd), out, s)
    assert faces(top, 0) == 0 and verts(0, 0) == 0                  # count 0: no-op
    assert faces(top, 1) == -1 and "int" in L.last_error()
    assert faces(top - 1, 2) == -1
    assert verts(top, 1) == -1
    assert faces(-1, 1) == -1 and faces(0, -1) == -1 and verts(-1, 1) == -1
    assert faces(0, 1, out=None) == -1 and faces(0, 1, t=None) == -1 and verts(0, 1, x=None) == -1
    assert faces(0, 1, out=ctypes.c_void_p(buf.data_ptr() + 4)) == -1 and "aligned" in L.last_error()
    assert lib.cgs_ellipsoid_mesh_faces(0, 1, 0, 360, L.ptr(tfd), L.ptr(buf), s) == -1
    assert faces(0, 1) == 0 and verts(0, 1) == 0
    torch.cuda.synchronize()
    b = buf.cpu().numpy()
    assert np.array_equal(b[:4914].view(np.uint8), np.frombuffer(E.vertex_records(*[a[:1] for a in _splats(4, 6)], tv)
                                                                 .tobytes(), np.uint8))


# ------------------------------------------------------------------------------------------------ the model
def _model():
    from curve_gaussian_amd.scene import GaussianCurveModel
    t = lambda k: torch.from_numpy(G[k])
    return GaussianCurveModel(0, int(G["n_gaussians"]), device=DEV).create_from_curves(
        t("curve_points"), t("width"), t("opacity"), t("mask"), t("is_bezier"))


def test_draw_ellipsoids_and_draw_curve_match_the_reference(tmp_path):
    g = _model()
    step = int(G["step"])
    fc = g.draw_curve(str(tmp_path), step)
    fe = g.draw_ellipsoids(str(tmp_path), step)
    assert [os.path.basename(fc), os.path.basename(fe)] == list(G["files"])
    # the per-splat inputs: the HIP sampling kernel against the reference's torch expressions, float32 rounding apart
    np.testing.assert_allclose(g.get_xyz.detach().cpu().numpy(), G["xyz"], rtol=0, atol=1e-6)
    np.testing.assert_allclose(g.get_rotation.detach().cpu().numpy(), G["rotation"], rtol=0, atol=1e-5)
    np.testing.assert_allclose(g.get_scaling.detach().cpu().numpy(), G["scaling"], rtol=1e-5, atol=0)
    # the mesh: counts and faces exact, colours exact, positions as the float64 restatement of the fixture's inputs
    v, f = E.read_mesh(fe)
    P = G["xyz"].shape[0]
    assert (len(v), len(f)) == tuple(G["mesh_counts"])
    tv, tf = _template()
    assert f.tobytes() == E.face_records(P, tf, 182).tobytes()
    u8 = np.repeat(E.color_u8(G["splat_color"]), 182, axis=0)
    assert np.array_equal(np.stack([v["red"], v["green"], v["blue"]], 1), u8)
    want = E.vertex_positions(G["splat_center"], G["splat_quaternion"], G["scaling"], tv).reshape(-1, 3)
    got = np.stack([v["x"], v["y"], v["z"]], 1)
    np.testing.assert_allclose(got, want, rtol=0, atol=4e-6)
    # and bit for bit the restatement of the model's own (GPU-sampled) inputs
    rgb = np.clip(G["splat_color"], 0, 1)
    assert v.tobytes() == E.vertex_records(g.get_xyz.detach().cpu().numpy(), g.get_rotation.detach().cpu().numpy(),
                                           g.get_scaling.detach().cpu().numpy(), rgb, tv).tobytes()
    # the curve samples
    lines, el, body = E.read_ply(fc)
    rows = np.array([r.split() for r in body.decode().splitlines()])
    assert len(rows) == len(G["curve_sample_points"])
    np.testing.assert_allclose(rows[:, :3].astype(np.float64), G["curve_sample_points"], rtol=0, atol=2e-6)
    assert np.array_equal(rows[:, 3:].astype(np.int64), E.color_u8(G["curve_point_colors"]).astype(np.int64))


def test_draw_reads_deferred_derived_tensors(tmp_path):
    """With lazy_derived, the accessors run the deferred sampling first: the mesh equals the eager model's."""
    g0, g1 = _model(), _model()
    g1.lazy_derived = True
    with torch.no_grad():
        g1._curve_points.add_(0.01)
        g0._curve_points.add_(0.01)
    g0.prepare_scaling_rot()
    g1.prepare_scaling_rot()
    assert g1._derived_pending is not None
    a = open(g0.draw_ellipsoids(str(tmp_path / "a"), 1), "rb").read()
    b = open(g1.draw_ellipsoids(str(tmp_path / "b"), 1), "rb").read()
    assert a == b


def test_command_line_run_draws_every_snapshot(scan, tmp_path):  # noqa: F811
    out = tmp_path / "cli"
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-m", "curve_gaussian_amd.train", "-s", scan[0], "-m", str(out), "--iterations",
                        "400", "--test_iterations", "400", "--save_iterations", "200", "--quiet",
                        "--draw_snapshots"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    for it in (200, 400):
        d = out / "point_cloud" / f"iteration_{it}"
        _, el, _ = E.read_ply(str(d / "point_cloud.ply"))
        P = el["vertex"][0]
        assert P > 0 and P % 12 == 0
        v, f = E.read_mesh(str(d / f"ellipsoids_step{it}.ply"))
        assert (len(v), len(f)) == (182 * P, 360 * P)
        assert int(f["c"].max()) == 182 * P - 1
        _, el, body = E.read_ply(str(d / f"curve_step{it}.ply"))
        assert el["vertex"][0] == 200 * (P // 12) == len(body.decode().splitlines())
