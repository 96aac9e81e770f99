"""float64 numpy restatement of the ellipsoid mesh kernels (csrc/mesh.hip, cgs_ellipsoid_mesh_vertices / _faces) and a
reader of the PLY files scene/snapshot_viz.py writes.  Every operation is one IEEE float64 operation in the kernel's order
(numpy does not contract into FMAs), so the bytes must match the kernel's bit for bit."""
import numpy as np

VERTEX = np.dtype([("x", "<f8"), ("y", "<f8"), ("z", "<f8"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])
FACE = np.dtype([("n", "u1"), ("a", "<i4"), ("b", "<i4"), ("c", "<i4")])
assert VERTEX.itemsize == 27 and FACE.itemsize == 13


def color_u8(c):
    """Open3D's ColorToUint8: round(min(1, max(0, c)) * 255), half away from zero; NaN -> 0."""
    c = np.asarray(c, np.float32).astype(np.float64)
    c = np.where(0.0 < c, c, 0.0)
    c = np.where(c < 1.0, c, 1.0) * 255.0
    r = np.floor(c)
    return (r + (c - r >= 0.5)).astype(np.uint8)


def rotation_rows(q):
    """Eigen's toRotationMatrix of float32 quaternions [P,4] (w, x, y, z), float64 [P,3,3]."""
    q = np.asarray(q, np.float32).astype(np.float64)
    w, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return np.stack([np.stack([1.0 - (tyy + tzz), txy - twz, txz + twy], -1),
                     np.stack([txy + twz, 1.0 - (txx + tzz), tyz - twx], -1),
                     np.stack([txz - twy, tyz + twx, 1.0 - (txx + tyy)], -1)], 1)


def vertex_positions(xyz, rot, scale, template):
    """float64 [P,V0,3]: p = template * (double)scale, every row ((r0*p0 + r1*p1) + r2*p2) + (double)xyz."""
    s = np.asarray(scale, np.float32).astype(np.float64)
    c = np.asarray(xyz, np.float32).astype(np.float64)
    p = np.asarray(template, np.float64)[None] * s[:, None, :]
    R = rotation_rows(rot)
    out = np.empty(p.shape, np.float64)
    for j in range(3):
        out[..., j] = ((R[:, j, 0, None] * p[..., 0] + R[:, j, 1, None] * p[..., 1]) + R[:, j, 2, None] * p[..., 2]) \
            + c[:, j, None]
    return out


def vertex_records(xyz, rot, scale, rgb, template):
    pos = vertex_positions(xyz, rot, scale, template)
    P, V0 = pos.shape[:2]
    rec = np.empty(P * V0, VERTEX)
    rec["x"], rec["y"], rec["z"] = (pos[..., j].reshape(-1) for j in range(3))
    u8 = np.repeat(color_u8(np.asarray(rgb).reshape(P, 3)), V0, axis=0)
    rec["red"], rec["green"], rec["blue"] = u8[:, 0], u8[:, 1], u8[:, 2]
    return rec


def face_records(P, triangles, V0, first=0):
    tri = np.asarray(triangles, np.int64)
    idx = (tri[None] + (np.arange(first, first + P, dtype=np.int64) * V0)[:, None, None]).reshape(-1, 3)
    rec = np.empty(idx.shape[0], FACE)
    rec["n"] = 3
    rec["a"], rec["b"], rec["c"] = idx[:, 0], idx[:, 1], idx[:, 2]
    return rec


def mesh_body(xyz, rot, scale, rgb, template, triangles):
    P = np.asarray(xyz).shape[0]
    return vertex_records(xyz, rot, scale, rgb, template).tobytes() + \
        face_records(P, triangles, len(template)).tobytes()


def read_ply(path):
    """(header lines, {element: (count, [property lines])}, body bytes) of a PLY file."""
    with open(path, "rb") as fh:
        data = fh.read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").splitlines()
    elements, cur = {}, None
    for ln in lines:
        w = ln.split()
        if w[0] == "element":
            cur = w[1]
            elements[cur] = (int(w[2]), [])
        elif w[0] == "property":
            elements[cur][1].append(ln)
    return lines, elements, data[end:]


def read_mesh(path):
    """(vertex records, face records) of a binary little-endian ellipsoid mesh written by write_ellipsoid_mesh."""
    lines, el, body = read_ply(path)
    assert lines[:2] == ["ply", "format binary_little_endian 1.0"], lines[:2]
    nv, nf = el["vertex"][0], el["face"][0]
    assert len(body) == nv * VERTEX.itemsize + nf * FACE.itemsize, (len(body), nv, nf)
    v = np.frombuffer(body, VERTEX, nv)
    f = np.frombuffer(body, FACE, nf, offset=nv * VERTEX.itemsize)
    return v, f
