"""Rejoining the extracted edges at their junctions (cgs_end_attach, include/curvegs.h; csrc/edge_join.hip).  Trimming
(ops/edge_trim.py) and deduping (ops/edge_dedupe.py) cut edges short of the points where they met, and the reference's
``merge_endpoints`` -- end point against end point inside one ball, before any cut -- never joins an end to the interior of
another edge.  This module tests every end of every edge against every sample of every OTHER edge in 3D -- near, or ahead
along the end's outward tangent --, groups the ends that found each other into vertices, records where an end lands on
the interior of an edge (a T-junction), and moves the end control points onto their vertices.  Opt-in.

  end_attach       int64 [2E]: per end the key of the nearest accepted sample, NO_ATTACH when there is none
  attachments      the keys decoded and classified: none, onto an end, or onto the interior of an edge (T)
  join_components  the ends that attached to one another, grouped
  join_vertices    one point per group
  move_ends        the end control points replaced by their vertices
  join_edges       all of it on an edge dict

Definitions, frozen.  "float32" is IEEE single precision, one rounded operation at a time in the written
order, nothing contracted into an FMA: numpy float32 arrays and the kernel agree bit for bit.
  SAMPLES     pts, off = ``sample_edges(curves, lines, resolution)``; n[e] = off[e+1] - off[e]
  ENDS        edge e with n >= 1 has end 2e at its first sample and end 2e+1 at its last; an edge with n = 0 has none and
              its two keys stay NO_ATTACH
  TANGENT     of an end at sample i, OUTWARD: t = pts[i] - pts[inner], inner = i + min(1, n-1) for the first end and
              i - min(1, n-1) for the last; q = (t.x*t.x + t.y*t.y) + t.z*t.z.  An edge of one sample has t = 0, q = 0
  ACCEPTS     sample j of edge b is accepted by an end of edge a with point p iff b != a and, with w = pts[j] - p,
              w2 = (w.x*w.x + w.y*w.y) + w.z*w.z and s = (w.x*t.x + w.y*t.y) + w.z*t.z, at least one of
                NEAR  w2 <= tol2                                  the ball of ``merge_endpoints``, any direction
                TUBE  s > 0 and s*s <= rq and (w2*q) - (s*s) <= tq    rq = reach2*q, tq = tol2*q: ahead of the end, at
                                                                  most reach along its tangent, at most tolerance beside
                ENDS  j is the first or the last sample of b and s > 0 and w2 <= reach2: another edge's end that lies
                                                                  ahead within reach, however far beside the ray
              tol2 = float32(tolerance)^2, reach2 = float32(reach)^2.  With q = 0 only NEAR can hold
  ATTACH      key[end] = the minimum over the accepted samples of (uint64(bits(w2)) << 32) | uint32(j); w2 >= +0, so its
              bits order like its value: the nearest accepted sample, the lowest index among equals.  NO_ATTACH = 2^64 - 1,
              -1 as an int64
Host rules, integers and float64, the same code for both back ends:
  CLASSIFY    k = j - off[b].  Onto end 2b when k <= zone, onto end 2b+1 when k >= n[b] - 1 - zone; when both hold the
              nearer end wins and a tie goes to 2b.  Otherwise a T-attachment onto edge b at sample k, parameter
              k / (n[b] - 1).  zone defaults to ceil(tolerance / resolution)
  COMPONENTS  union-find over the end-to-end attachments (one direction suffices), each labelled by its least end; an
              unattached end that nobody attaches to is its own component
  VERTEX      of a component: 1. when a member has a T-attachment, the host's sample point pts[j] of the member
              T-attachment with the least key; 2. else, when all member end points are bitwise equal, that point,
              unchanged; 3. else the least-squares point nearest to the members' tangent lines -- A = sum(I - u u^T),
              A x = sum((I - u u^T) p) in float64, u the normalised tangent, a member with q = 0 contributes I -- taken
              only when the least eigenvalue of A is at least 1 - COS_MIN (0.1: two lines nearer than about 26 degrees
              count as parallel, the line the dedupe draws) and x lies within reach of every member; 4. otherwise the
              float64 mean of the member points, as ``merge_endpoints`` does.  The member points are the end control
              points of the edges in float64, not their float32 samples
  RELEASE     no end moves further than reach.  While a member lies further than reach from its component's vertex, the
              furthest member (the least end among equals) leaves the component and becomes a component of its own, with
              its own point as the vertex, and the vertex of the rest is formed again.  This happens to the far end of a
              chain -- A attaches to B within reach, B to C or onto a T within reach, and the common vertex lies further
              than reach from A -- and to an end whose T-attachment sits in the far corner of the tube, up to
              sqrt(reach^2 + tolerance^2) away.  Released ends are reported (``released``) and their T-attachment, if
              any, is not a T-junction
  MOVE        the first or last control point of a curve, or the end point of a line, is replaced by its vertex; the
              middle control points stay, as in ``merge_endpoints``; an edge none of whose ends moves comes back bit for
              bit; the host of a T-attachment is neither changed nor split
  REPORTED, NOT REPAIRED: an edge whose two ends land in one vertex (``collapsed``), and a T-attachment whose host itself
              moved (``host_moved``)

KNOWN LIMITS.  This is 3D only, there is no image evidence for a junction.  The host of a T-junction is not split.  An
end joins at most one thing: the nearest accepted sample.  A parallel edge that continues past an end within ``tolerance``
of its ray attracts that end.  An edge of one sample has both ends on its first point.  One pass: the join is not iterated.
Whether joined edges score better on ABC has not been measured.  THE DEFAULTS ARE UNTUNED: only drawn fixtures
(tests/edge_join_cases.py) have been looked at, no real scan.

Two back ends: ``"gpu"``, HIP, and ``"host"``, numpy in chunks of ends, so memory stays O(chunk x P)."""
import math

import numpy as np
import torch

from .. import _lib as L
from ..edge_extraction.reprojection import SAMPLE_RESOLUTION
from . import edge_dedupe as ED
from . import edge_score as ES
from . import edge_support as SP

JOIN_BACKENDS = SP.SUPPORT_BACKENDS
NO_ATTACH = -1                # 2^64 - 1 as an int64
KIND_NONE, KIND_END, KIND_T = 0, 1, 2
# UNTUNED: drawn fixtures only
TOLERANCE_RESOLUTIONS = ED.TOLERANCE_RESOLUTIONS   # the default tolerance, in units of the sampling resolution
REACH_RESOLUTIONS = 8.0                            # the default reach
MIN_EIGENVALUE = 1.0 - ED.COS_MIN                  # of the least-squares vertex's normal matrix
HOST_CHUNK = 64               # ends per step of the host back end


def _check_backend(backend):
    if backend not in JOIN_BACKENDS:
        raise ValueError(f"unknown edge join backend {backend!r}: expected one of {JOIN_BACKENDS}")


def _squares(tolerance, reach):
    """(tol2, reach2) as float32, formed once: float32(x) * float32(x)."""
    tolerance, reach = float(tolerance), float(reach)
    if not tolerance > 0.0 or not np.isfinite(tolerance):
        raise ValueError(f"tolerance must be a positive number (got {tolerance})")
    if not reach >= 0.0 or not np.isfinite(reach):
        raise ValueError(f"reach must be a non-negative number (got {reach})")
    return np.float32(tolerance) * np.float32(tolerance), np.float32(reach) * np.float32(reach)


def _end_samples(off):
    """(exists bool [2E], at int64 [2E], inner int64 [2E]): the sample of every end and the one its tangent starts from; 0
    where the end does not exist."""
    off = off.astype(np.int64)
    n = np.diff(off)
    step = np.clip(n - 1, 0, 1)
    at = np.stack([off[:-1], off[1:] - 1], 1)
    inner = np.stack([off[:-1] + step, off[1:] - 1 - step], 1)
    exists = np.repeat(n > 0, 2)
    return exists, np.where(exists, at.reshape(-1), 0), np.where(exists, inner.reshape(-1), 0)


def end_tangents(points, offsets):
    """(t float32 [2E,3], q float32 [2E]) of the ends, outward; 0 for an end that does not exist."""
    pts = np.asarray(points, np.float32).reshape(-1, 3)
    exists, at, inner = _end_samples(np.asarray(offsets))
    t = np.zeros((exists.size, 3), np.float32)
    if pts.shape[0]:
        t = np.where(exists[:, None], pts[at] - pts[inner], np.float32(0))
    return t, (t[:, 0] * t[:, 0] + t[:, 1] * t[:, 1]) + t[:, 2] * t[:, 2]


def _attach_host(pts, off, tol2, reach2, chunk=HOST_CHUNK):
    P, E = pts.shape[0], off.size - 1
    keys = np.full(2 * E, np.iinfo(np.uint64).max, np.uint64)
    if P == 0:
        return keys
    exists, at, _ = _end_samples(off)
    t, q = end_tangents(pts, off)
    n = np.diff(off.astype(np.int64))
    edge = np.repeat(np.arange(E, dtype=np.int64), n)       # [P]: the edge of every sample
    is_end = np.zeros(P, bool)
    is_end[at[exists]] = True
    index = np.arange(P, dtype=np.uint64)
    ends = np.nonzero(exists)[0]
    with np.errstate(over="ignore", invalid="ignore"):
        for c0 in range(0, ends.size, chunk):
            c = ends[c0:c0 + chunk]
            p = pts[at[c]]
            wx, wy, wz = (pts[None, :, a] - p[:, a, None] for a in range(3))
            w2 = (wx * wx + wy * wy) + wz * wz
            s = (wx * t[c, 0, None] + wy * t[c, 1, None]) + wz * t[c, 2, None]
            ss = s * s
            qc = q[c, None]
            near = w2 <= tol2
            tube = (ss <= reach2 * qc) & ((w2 * qc - ss) <= tol2 * qc)
            other_end = is_end[None, :] & (w2 <= reach2)
            ok = (edge[None, :] != (c >> 1)[:, None]) & (near | ((s > 0) & (tube | other_end)))
            key = (w2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | index[None, :]
            keys[c] = np.where(ok, key, np.iinfo(np.uint64).max).min(1)
    return keys


def end_attach(points, offsets, tolerance, reach, backend="gpu", device=None):
    """int64 [2E]: key[end] as the module docstring defines it, the uint64 reinterpreted: NO_ATTACH is -1 and every other
    key is non-negative, (bits(w2) << 32) | j.  points float32 [P,3], finite (ValueError otherwise: the kernel never sees
    a NaN); offsets int [E+1] as ``sample_edges`` gives them; tolerance > 0 and reach >= 0 in the units of the points.

    ``backend="gpu"``: ``cgs_end_attach``.  points may be a host array, which is uploaded to ``device`` (default: the
    current GPU), or a tensor, which must then be a contiguous GPU tensor (CurveGSError otherwise); ``device``, when given,
    and offsets that are a GPU tensor must be on that GPU (CurveGSError).  The result stays on the device.  The call is
    NOT asynchronous: offsets are checked on the host (a GPU tensor is copied back for that, which synchronises, and
    uploaded again), and so is the finiteness of the points (one reduction read back).
    ``backend="host"``: numpy, ``HOST_CHUNK`` ends at a time; host arrays and CPU tensors; a CPU tensor comes back."""
    _check_backend(backend)
    tol2, reach2 = _squares(tolerance, reach)
    pts = SP._points(points)
    P = int(pts.shape[0])
    off = SP._offsets(offsets, P)
    E = off.size - 1
    if P > np.iinfo(np.int32).max:
        raise ValueError(f"end_attach: {P} samples: at most 2^31 - 1")
    if not bool(torch.isfinite(pts).all()):
        raise ValueError("end_attach: points must be finite")
    if backend == "host":
        if pts.is_cuda:
            raise ValueError("end_attach: backend='host' takes host arrays and CPU tensors")
        return torch.from_numpy(_attach_host(np.ascontiguousarray(pts.numpy()), off, tol2, reach2).view(np.int64))
    if torch.is_tensor(points):
        L.require_gpu_tensor(pts, "end_attach: points")
        if not pts.is_contiguous():
            raise L.CurveGSError("end_attach: points must be contiguous")
    dev = ES._device_for([pts], "end_attach", None if pts.is_cuda else device)
    if device is not None and torch.device(device) != dev and torch.device(device) != torch.device(dev.type):
        raise L.CurveGSError(f"end_attach: points are on {dev}, device={device}: all tensors must be on one device")
    if torch.is_tensor(offsets) and offsets.is_cuda and offsets.device != dev:
        raise L.CurveGSError(f"end_attach: offsets are on {offsets.device}, points on {dev}: all tensors must be on one device")
    with L.device_guard(dev):
        keys = torch.empty((2 * E,), dtype=torch.int64, device=dev)   # the kernel writes every key
        if E > 0:
            lib = L.load()
            pts = pts.to(dev)
            off_d = torch.from_numpy(off).to(dev)
            work = torch.empty(int(lib.cgs_end_attach_workspace_bytes(P, E)), dtype=torch.uint8, device=dev)
            rc = lib.cgs_end_attach(P, L.ptr(pts), E, L.ptr(off_d), float(tol2), float(reach2), L.ptr(keys), L.ptr(work),
                                    L.raw_stream(dev))
            L.check(rc, "cgs_end_attach")
    return keys


# ------------------------------------------------------------------------------------------------ host rules
def _keys(keys, E):
    k = ES._host(keys)
    if k.ndim != 1 or k.dtype != np.int64 or k.size != 2 * E:
        raise ValueError(f"keys must be int64 [2E] with E = {E} edges (got {k.dtype} {k.shape})")
    return k


def attachments(keys, offsets, zone):
    """The keys of ``end_attach`` decoded and classified (CLASSIFY in the module docstring); host integers for either back
    end's keys.  Returns a dict of [2E] arrays: "key" int64, "sample" j, "edge" b, "local" k = j - off[b] (int64, -1 where
    there is none), "kind" int8 (KIND_NONE, KIND_END, KIND_T), "target" int64, the end 2b or 2b+1 of an end attachment (-1
    otherwise), "parameter" float64, k / (n[b] - 1) of a T-attachment (nan otherwise), and "distance" float64, the root of
    the float32 w2 (nan where there is none)."""
    zone = int(zone)
    if zone < 0:
        raise ValueError(f"zone must be >= 0 (got {zone})")
    off = ES._host(offsets)
    off = SP._offsets(off, int(off[-1]) if off.ndim == 1 and off.size else 0).astype(np.int64)
    E = off.size - 1
    key = _keys(keys, E)
    found = key != NO_ATTACH
    j = np.where(found, key & 0xffffffff, -1)
    if (key < NO_ATTACH).any() or (j >= off[-1]).any():
        raise ValueError("keys name a sample that does not exist")
    b = np.where(found, np.searchsorted(off, np.maximum(j, 0), side="right") - 1, -1)   # the last e with off[e] <= j
    n = np.diff(off)
    nb = np.where(found, n[np.maximum(b, 0)] if E else 0, 0)
    k = np.where(found, j - off[np.maximum(b, 0)] if E else 0, -1)
    to_first, to_last = found & (k <= zone), found & (k >= nb - 1 - zone)
    first_wins = to_first & (~to_last | (k <= nb - 1 - k))
    kind = np.where(found, np.where(to_first | to_last, KIND_END, KIND_T), KIND_NONE).astype(np.int8)
    target = np.where(kind == KIND_END, 2 * b + np.where(first_wins, 0, 1), -1)
    with np.errstate(invalid="ignore", divide="ignore"):
        parameter = np.where(kind == KIND_T, k / np.maximum(nb - 1, 1), np.nan)
    w2 = (np.where(found, key, 0) >> 32).astype(np.uint32).view(np.float32)
    distance = np.where(found, np.sqrt(w2.astype(np.float64)), np.nan)
    return {"key": key, "sample": j, "edge": b, "local": k, "kind": kind, "target": target, "parameter": parameter,
            "distance": distance}


def join_components(attach, offsets):
    """int64 [2E]: per end the least end of its component (COMPONENTS in the module docstring), -1 for an end that does
    not exist.  ``attach``: the dict of ``attachments``."""
    off = ES._host(offsets).astype(np.int64)
    exists = np.repeat(np.diff(off) > 0, 2)
    parent = np.arange(exists.size, dtype=np.int64)

    def root(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for end in np.nonzero(attach["kind"] == KIND_END)[0]:
        a, b = root(end), root(attach["target"][end])
        parent[max(a, b)] = min(a, b)          # the root of a set is its least member
    labels = np.array([root(x) for x in range(exists.size)], np.int64).reshape(-1)
    return np.where(exists, labels, -1)


def end_points(curves, lines):
    """float64 [2E,3]: the first and the last control point of every curve, then the two end points of every line."""
    curves, lines = SP._edge_arrays(curves, lines)
    return np.concatenate([curves[:, [0, 3]].reshape(-1, 3), lines.reshape(-1, 3)])


def join_vertices(attach, labels, points, offsets, ends, reach):
    """One vertex per component (VERTEX in the module docstring).  ``points``, ``offsets``: the samples; ``ends``: float64
    [2E,3], ``end_points``.  Returns {"vertices": float64 [Nv,3], in the order of the components' labels, "vertex_of_end":
    int64 [2E], -1 for an end that does not exist, "rule": per vertex which of "t", "equal", "lsq", "mean" gave it,
    "released": the ends that RELEASE took out of their component, ascending}."""
    pts = np.asarray(ES._host(points), np.float32).reshape(-1, 3)
    ends = np.asarray(ends, np.float64).reshape(-1, 3)
    reach = float(reach)
    t, q = end_tangents(pts, ES._host(offsets))
    t, q = t.astype(np.float64), q.astype(np.float64)
    labels = np.asarray(labels, np.int64)

    def vertex(members):
        p = ends[members]
        tees = members[attach["kind"][members] == KIND_T]
        if tees.size:
            best = tees[np.argmin(attach["key"][tees])]
            return pts[attach["sample"][best]].astype(np.float64), "t"
        if all(p[m].tobytes() == p[0].tobytes() for m in range(len(p))):
            return p[0], "equal"
        A, rhs = np.zeros((3, 3)), np.zeros(3)
        for m, point in zip(members, p):
            M = np.eye(3)
            if q[m] > 0.0:
                u = t[m] / math.sqrt(q[m])
                M = M - np.outer(u, u)
            A += M
            rhs += M @ point
        if np.linalg.eigvalsh(A)[0] >= MIN_EIGENVALUE:
            x = np.linalg.solve(A, rhs)
            if (np.linalg.norm(p - x, axis=1) <= reach).all():
                return x, "lsq"
        return p.mean(0), "mean"

    groups, released = [], []
    for root in np.unique(labels[labels >= 0]):
        members = np.nonzero(labels == root)[0]
        while members.size:
            x, rule = vertex(members)
            far = np.linalg.norm(ends[members] - x, axis=1)
            worst = int(np.argmax(far))          # the first of equals: the least end
            if far[worst] <= reach:
                groups.append((members, x, rule))
                break
            released.append(int(members[worst]))
            groups.append((members[worst:worst + 1], ends[members[worst]], "equal"))
            members = np.delete(members, worst)
    groups.sort(key=lambda g: int(g[0][0]))       # by the least member: np.nonzero and np.delete keep them ascending
    vertex_of_end = np.full(labels.size, -1, np.int64)
    for v, (members, _, _) in enumerate(groups):
        vertex_of_end[members] = v
    vertices = np.array([g[1] for g in groups], np.float64).reshape(-1, 3)
    return {"vertices": vertices, "vertex_of_end": vertex_of_end, "rule": [g[2] for g in groups],
            "released": sorted(released)}


def move_ends(curves, lines, vertex_of_end, vertices):
    """(curves float64 [Nc,4,3], lines float64 [Nl,2,3], moved float64 [2E]): copies of the edges (curves [Nc,4,3] or
    [Nc,12], lines [Nl,2,3] or [Nl,6]) with every end control point replaced by its vertex (MOVE in the module docstring)
    and the length of every end's displacement, 0 for an end without a vertex."""
    curves, lines = SP._edge_arrays(curves, lines)
    curves, lines = curves.copy(), lines.copy()
    old = end_points(curves, lines)
    vertex_of_end = np.asarray(vertex_of_end, np.int64)
    if vertex_of_end.shape != (old.shape[0],):
        raise ValueError(f"move_ends: {old.shape[0] // 2} edges and {vertex_of_end.shape} vertex ids")
    has = vertex_of_end >= 0
    new = old.copy()
    new[has] = np.asarray(vertices, np.float64).reshape(-1, 3)[vertex_of_end[has]]
    Nc = len(curves)
    curves[:, [0, 3]] = new[:2 * Nc].reshape(-1, 2, 3)
    lines[:] = new[2 * Nc:].reshape(-1, 2, 3)
    return curves, lines, np.linalg.norm(new - old, axis=1)


def join_edges(edge_dict, resolution=SAMPLE_RESOLUTION, tolerance=None, reach=None, zone=None, backend="gpu", device=None):
    """The edges of ``edge_dict`` (the layout of ``get_parametric_edge``) rejoined at their junctions: ``sample_edges`` at
    ``resolution``, ``end_attach``, ``attachments``, ``join_components``, ``join_vertices``, ``move_ends``.  ``tolerance``
    and ``reach``: in the units of the edges, defaults ``TOLERANCE_RESOLUTIONS`` (2) and ``REACH_RESOLUTIONS`` (8) x
    resolution; ``zone``: in samples, default ceil(tolerance / resolution).  THE DEFAULTS ARE UNTUNED and the limits are
    those of the module docstring.

    Returns {"edge_dict": the joined edges (curves [Nc,4,3], lines [Nl,6], as lists; the same edges in the same order),
    "vertices": float64 [Nv,3], "edge_vertices": int64 [E,2], the vertex of each edge's first and last end (curves first,
    then lines; -1 for an edge without samples), "t_junctions": one dict per T-attachment -- "end", "edge" (the end's),
    "host" (edge), "sample" (k on the host), "parameter", "distance", "vertex", "host_moved" (the host itself moved: reported,
    not repaired) --, "moved": float64 [2E], the length of every end's displacement, "collapsed": the edges whose two ends
    land in one vertex, "released": the ends that attached but stay where they are (RELEASE), "rules": per vertex which
    rule gave it, "attach": the dict of ``attachments``, "keys": int64 [2E] CPU tensor, "offsets": int32 [E+1],
    "settings"}."""
    _check_backend(backend)
    resolution = float(resolution)
    tolerance = TOLERANCE_RESOLUTIONS * resolution if tolerance is None else float(tolerance)
    reach = REACH_RESOLUTIONS * resolution if reach is None else float(reach)
    _squares(tolerance, reach)
    zone = int(math.ceil(tolerance / resolution)) if zone is None else int(zone)
    if zone < 0:
        raise ValueError(f"zone must be >= 0 (got {zone})")
    curves, lines = SP._edge_arrays(edge_dict["curves_ctl_pts"], edge_dict["lines_end_pts"])
    pts, off = SP.sample_edges(curves, lines, resolution)
    keys = end_attach(pts, off, tolerance, reach, backend=backend, device=device).cpu()
    attach = attachments(keys, off, zone)
    labels = join_components(attach, off)
    found = join_vertices(attach, labels, pts, off, end_points(curves, lines), reach)
    out_c, out_l, moved = move_ends(curves, lines, found["vertex_of_end"], found["vertices"])
    edge_vertices = found["vertex_of_end"].reshape(-1, 2)
    tees = [{"end": int(end), "edge": int(end >> 1), "host": int(attach["edge"][end]), "sample": int(attach["local"][end]),
             "parameter": float(attach["parameter"][end]), "distance": float(attach["distance"][end]),
             "vertex": int(found["vertex_of_end"][end]),
             "host_moved": bool(moved[2 * attach["edge"][end]] > 0 or moved[2 * attach["edge"][end] + 1] > 0)}
            for end in np.nonzero(attach["kind"] == KIND_T)[0] if end not in found["released"]]
    collapsed = [int(e) for e in np.nonzero((edge_vertices[:, 0] >= 0) & (edge_vertices[:, 0] == edge_vertices[:, 1]))[0]]
    settings = {"resolution": resolution, "tolerance": tolerance, "reach": reach, "zone": zone, "backend": backend,
                "points": int(pts.shape[0])}
    return {"edge_dict": {"curves_ctl_pts": out_c.tolist(), "lines_end_pts": out_l.reshape(-1, 6).tolist()},
            "vertices": found["vertices"], "edge_vertices": edge_vertices, "t_junctions": tees, "moved": moved,
            "collapsed": collapsed, "released": found["released"], "rules": found["rule"], "attach": attach, "keys": keys,
            "offsets": off, "settings": settings}
