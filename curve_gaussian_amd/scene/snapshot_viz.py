"""The two inspection files train.py writes next to every snapshot (train.py:213-220): the reference's
``GaussianCurveModel.draw_curve`` (scene/gaussian_curve_model.py:712-727) and ``draw_ellipsoids`` (:634-709).

* ``curve_step{N}.ply``: ``num_sample`` points of every curve, one colour per curve, ASCII PLY (host side: 200 points per
  curve is not a hot path).
* ``ellipsoids_step{N}.ply``: every splat as a sphere of radius 1.2 and resolution 10, scaled by ``get_scaling``,
  rotated by ``get_rotation`` and moved to ``get_xyz``; lines black, splats with ``sigmoid(_mask) < 0.01`` white, every
  other splat its curve's colour; one binary PLY triangle mesh.  The HIP kernels ``cgs_ellipsoid_mesh_vertices`` /
  ``cgs_ellipsoid_mesh_faces`` write the bytes of the file body in chunks; the host copies each chunk to pinned memory
  (the copy of one chunk overlaps the next chunk's kernel) and writes it unchanged.

Deviations: the sphere template restates Open3D's ``TriangleMesh.create_sphere``, whose vertex and triangle
order could not be checked against Open3D; the PLY writers restate Open3D's record layout (no Open3D header comment, ASCII
coordinates printed with ``%.9g``); the colour permutation is seeded."""
import ctypes
import itertools
import math
import os

import numpy as np
import torch

from .. import _lib as L

VERTEX_RECORD = 27     # double x, y, z; uchar red, green, blue
FACE_RECORD = 13       # uchar 3; int a, b, c
WORKSPACE_BUDGET = 1 << 30
_ASCII_ROWS = 1 << 16  # rows formatted per string operation in write_curve_points


# ------------------------------------------------------------------------------------------------ sphere template
def sphere_template(radius=1.2, resolution=10):
    """Open3D's TriangleMesh.create_sphere(radius, resolution), restated: float64 vertices [2 + 2r(r-1), 3] and int32
    triangles [4r(r-1), 3].  Vertices: the poles (0, 0, +radius) and (0, 0, -radius), then r - 1 rings of 2r vertices,
    (sin a cos t, sin a sin t, cos a) * radius at a = pi i / r, t = pi j / r.  Triangles: for every j the north and the
    south fan triangle, then two triangles per quad between neighbouring rings; every triangle winds outward."""
    r = int(resolution)
    if r < 2:
        raise L.CurveGSError(f"sphere_template: resolution must be >= 2 (got {resolution})")
    n = 2 * r
    v = np.zeros((2 + n * (r - 1), 3), np.float64)
    v[0] = (0.0, 0.0, radius)
    v[1] = (0.0, 0.0, -radius)
    step = math.pi / r
    for i in range(1, r):
        a = step * i
        base = 2 + n * (i - 1)
        for j in range(n):
            t = step * j
            v[base + j] = (math.sin(a) * math.cos(t) * radius, math.sin(a) * math.sin(t) * radius, math.cos(a) * radius)
    f = []
    south = 2 + n * (r - 2)
    for j in range(n):
        j1 = (j + 1) % n
        f.append((0, 2 + j, 2 + j1))
        f.append((1, south + j1, south + j))
    for i in range(1, r - 1):
        b1 = 2 + n * (i - 1)
        b2 = b1 + n
        for j in range(n):
            j1 = (j + 1) % n
            f.append((b2 + j, b1 + j1, b1 + j))
            f.append((b2 + j, b2 + j1, b1 + j1))
    return v, np.asarray(f, np.int32)


# ------------------------------------------------------------------------------------------------ colours and samples
def curve_colors(n_curves, seed=0):
    """get_fancy_color(n + 1)[torch.randperm(n)] (:691-692, :714-715), float32 [n,3]; the permutation is drawn from a
    generator seeded with `seed` (the reference's is unseeded)."""
    from ..edge_extraction.novel_view import fancy_colors
    g = torch.Generator().manual_seed(int(seed))
    return fancy_colors(n_curves + 1)[torch.randperm(n_curves, generator=g)]


def splat_colors(is_bezier, mask, n_gaussians, seed=0):
    """draw_ellipsoids' colours (:691-697), float32 [B*m,3] on mask's device: the curve's colour, black for the splats of
    a line (is_bezier False), white for a splat with sigmoid(_mask) < 0.01 (after the lines)."""
    B = int(is_bezier.shape[0])
    cols = curve_colors(B, seed).to(mask.device).repeat_interleave(int(n_gaussians), 0)
    lines = (~is_bezier.to(mask.device).bool()).repeat_interleave(int(n_gaussians), 0)
    cols[lines] = 0.0
    cols[(torch.sigmoid(mask) < 0.01).reshape(-1)] = 1.0
    return cols


def curve_sample_points(g, num_sample=200):
    """draw_curve's points (:717-720): get_curve_gaussians at linspace(0, 1, num_sample), curve-major ('m b c -> b m c'),
    [B*num_sample, 3] on the model's device."""
    t = torch.linspace(0, 1, int(num_sample), device=g._curve_points.device)[:, None, None]
    return g.get_curve_gaussians(t).transpose(0, 1).reshape(-1, 3)


# ------------------------------------------------------------------------------------------------ writers
def _color_u8(c):
    """Open3D's ColorToUint8: round(min(1, max(0, c)) * 255), half away from zero, NaN -> 0."""
    c = np.asarray(c, np.float64)
    c = np.where(0.0 < c, c, 0.0)
    c = np.where(c < 1.0, c, 1.0) * 255.0
    r = np.floor(c)
    return (r + (c - r >= 0.5)).astype(np.uint8)      # c >= 0: round half away from zero (c - floor(c) is exact)


def _header(fmt, n_vertices, n_faces=None):
    h = [f"ply\nformat {fmt} 1.0\nelement vertex {n_vertices}\n",
         "property double x\nproperty double y\nproperty double z\n",
         "property uchar red\nproperty uchar green\nproperty uchar blue\n"]
    if n_faces is not None:
        h.append(f"element face {n_faces}\nproperty list uchar int vertex_indices\n")
    h.append("end_header\n")
    return "".join(h).encode("ascii")


def write_curve_points(path, points, colors):
    """ASCII PLY of points [N,3] (double x y z, printed with %.9g: a float32 value reads back exactly) and colours
    [N,3] in [0, 1] (uchar, Open3D's ColorToUint8), as o3d.io.write_point_cloud(..., write_ascii=True) writes them."""
    def host(x):
        return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    p = host(points).astype(np.float64).reshape(-1, 3)
    c = _color_u8(host(colors).reshape(-1, 3))
    if c.shape[0] != p.shape[0]:
        raise L.CurveGSError(f"write_curve_points: {p.shape[0]} points but {c.shape[0]} colours")
    with open(path, "wb") as fh:
        fh.write(_header("ascii", p.shape[0]))
        for s in range(0, p.shape[0], _ASCII_ROWS):
            pp, cc = p[s:s + _ASCII_ROWS].tolist(), c[s:s + _ASCII_ROWS].tolist()
            row = "%.9g %.9g %.9g %d %d %d\n"
            fh.write((row * len(pp) % tuple(itertools.chain.from_iterable(a + b for a, b in zip(pp, cc)))).encode())


def _splat_input(t, cols, name, dev):
    L.require_gpu_tensor(t, name)
    if t.dim() != 2 or t.shape[1] != cols or t.device != dev:
        raise L.CurveGSError(f"{name} must be [P,{cols}] on {dev} (got {tuple(t.shape)} on {t.device})")
    return t.detach().to(torch.float32).contiguous()


class EllipsoidMesh:
    """The splat inputs and the sphere template on the device, and launchers of the two record kernels."""

    def __init__(self, xyz, rot, scale, rgb, radius=1.2, resolution=10):
        L.require_gpu_tensor(xyz, "xyz")
        self.dev = xyz.device
        self.xyz = _splat_input(xyz, 3, "xyz", self.dev)
        self.P = int(self.xyz.shape[0])
        self.rot, self.scale, self.rgb = (_splat_input(t, c, n, self.dev) for t, c, n in
                                          ((rot, 4, "rot"), (scale, 3, "scale"), (rgb, 3, "rgb")))
        if not (self.rot.shape[0] == self.scale.shape[0] == self.rgb.shape[0] == self.P):
            raise L.CurveGSError("xyz, rot, scale and rgb must have the same number of rows")
        self.lib = L.load()
        vb, fb = ctypes.c_int64(), ctypes.c_int64()
        if self.lib.cgs_ellipsoid_mesh_body_bytes(self.P, int(resolution), ctypes.byref(vb), ctypes.byref(fb)) < 0:
            raise L.CurveGSError(f"cgs_ellipsoid_mesh_body_bytes failed: {L.last_error()}")
        self.vertex_bytes, self.face_bytes = vb.value, fb.value
        tv, tf = sphere_template(radius, resolution)
        self.V0, self.F0 = tv.shape[0], tf.shape[0]
        self.tv = torch.from_numpy(np.ascontiguousarray(tv)).to(self.dev)
        self.tf = torch.from_numpy(np.ascontiguousarray(tf)).to(self.dev)

    @staticmethod
    def chunk_bytes(count, per_splat):
        return -(-count * per_splat // 16) * 16

    def vertices_into(self, out, first, count):
        """Vertex records of splats [first, first + count) into the uint8 device tensor `out` (>= chunk_bytes)."""
        with L.device_guard(self.dev):
            rc = self.lib.cgs_ellipsoid_mesh_vertices(first, count, L.ptr(self.xyz), L.ptr(self.rot), L.ptr(self.scale),
                                                      L.ptr(self.rgb), self.V0, L.ptr(self.tv), L.ptr(out),
                                                      L.raw_stream(self.dev))
        L.check(rc, "cgs_ellipsoid_mesh_vertices")

    def faces_into(self, out, first, count):
        with L.device_guard(self.dev):
            rc = self.lib.cgs_ellipsoid_mesh_faces(first, count, self.V0, self.F0, L.ptr(self.tf), L.ptr(out),
                                                   L.raw_stream(self.dev))
        L.check(rc, "cgs_ellipsoid_mesh_faces")


def write_ellipsoid_mesh(path, xyz, rot, scale, rgb, radius=1.2, resolution=10, workspace_bytes=WORKSPACE_BUDGET):
    """Binary little-endian PLY of every splat's sphere (vertex records, then face records).  xyz [P,3],
    rot [P,4] (w, x, y, z, used as given), scale [P,3] and rgb [P,3] are GPU tensors on one device.  `workspace_bytes` of
    device memory hold two chunk buffers, and as much pinned host memory is used; the file does not depend on it.  Returns
    (number of vertices, number of faces)."""
    m = EllipsoidMesh(xyz, rot, scale, rgb, radius, resolution)
    P, V0, F0 = m.P, m.V0, m.F0
    with open(path, "wb") as fh:
        fh.write(_header("binary_little_endian", P * V0, P * F0))
        if P == 0:
            return 0, 0
        half = int(workspace_bytes) // 2 // 16 * 16
        per_v, per_f = half // (V0 * VERTEX_RECORD), half // (F0 * FACE_RECORD)
        if per_v < 1 or per_f < 1:
            need = 2 * m.chunk_bytes(1, max(V0 * VERTEX_RECORD, F0 * FACE_RECORD))
            raise L.CurveGSError(f"write_ellipsoid_mesh: a workspace of {workspace_bytes} bytes holds no splat (need {need})")
        jobs = []
        for launch, per, rec in ((m.vertices_into, per_v, V0 * VERTEX_RECORD), (m.faces_into, per_f, F0 * FACE_RECORD)):
            for first in range(0, P, per):
                count = min(per, P - first)
                jobs.append((launch, first, count, m.chunk_bytes(count, rec), count * rec))
        size = max(j[3] for j in jobs)
        nbuf = min(2, len(jobs))
        dev_buf = [torch.empty(size, dtype=torch.uint8, device=m.dev) for _ in range(nbuf)]
        pin_buf = [torch.empty(size, dtype=torch.uint8, pin_memory=True) for _ in range(nbuf)]
        main = torch.cuda.current_stream(m.dev)
        copy = torch.cuda.Stream(m.dev)
        pending = []

        def flush():
            ev, b, n = pending.pop(0)
            ev.synchronize()
            fh.write(memoryview(pin_buf[b].numpy())[:n])

        for k, (launch, first, count, nbytes, n_valid) in enumerate(jobs):
            b = k % nbuf
            if len(pending) == nbuf:
                flush()                 # the chunk that last used buffer b is on disk: dev_buf[b] / pin_buf[b] are free
            launch(dev_buf[b], first, count)
            copy.wait_stream(main)
            with torch.cuda.stream(copy):
                pin_buf[b][:nbytes].copy_(dev_buf[b][:nbytes], non_blocking=True)
                done = torch.cuda.Event()
                done.record(copy)
            pending.append((done, b, n_valid))
        while pending:
            flush()
    return P * V0, P * F0


# ------------------------------------------------------------------------------------------------ model methods
@torch.no_grad()
def draw_curve(g, path, step, num_sample=200, seed=0):
    """GaussianCurveModel.draw_curve (:712-727): ``{path}/curve_step{step}.ply``."""
    os.makedirs(path, exist_ok=True)
    n = int(g.get_curve_points.shape[0])
    cols = curve_colors(n, seed).repeat_interleave(int(num_sample), 0)
    out = os.path.join(path, f"curve_step{step}.ply")
    write_curve_points(out, curve_sample_points(g, num_sample), cols)
    return out


@torch.no_grad()
def draw_ellipsoids(g, path, step, radius=1.2, seed=0, resolution=10, workspace_bytes=WORKSPACE_BUDGET):
    """GaussianCurveModel.draw_ellipsoids (:634-709): ``{path}/ellipsoids_step{step}.ply``.  The per-splat tensors are read
    through the accessors (a deferred sampling runs first)."""
    os.makedirs(path, exist_ok=True)
    xyz, rot, scale = g.get_xyz, g.get_rotation, g.get_scaling
    rgb = splat_colors(g.is_bezier, g._mask, g.n_gaussians, seed)
    out = os.path.join(path, f"ellipsoids_step{step}.ply")
    write_ellipsoid_mesh(out, xyz, rot, scale, rgb, radius, resolution, workspace_bytes)
    return out
