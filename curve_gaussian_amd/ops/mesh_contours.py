"""Occluding contours of a triangle mesh: where a view sees a smooth surface turn away from it (cgs_mesh_contours,
include/curvegs.h; csrc/mesh_contours.hip).  A contour is an edge in every image and an edge nowhere in 3D -- the main
view-dependent nuisance of comparing 3D edges with 2D edge maps: no 3D edge explains it.  The reference has no counterpart.

  mesh_edges      the mesh's edge table: every edge shared by exactly two triangles as a row (a, b, c, d) -- the edge and
                  the two triangles' third vertices -- with the cosine of its fold; the other edges counted
  smooth          which rows are smooth: cos >= cos(crease_deg).  A smooth edge is no feature edge, so where it is drawn
                  it is a view-dependent contour
  edge_rows       the rows a ``kind`` selects: "smooth" (the contours of curved surfaces) or "all" (every two-triangle
                  edge: the outline with the hidden lines removed, feature edges included)
  contour_flags   bool [V,E]: the contour test alone, on the host
  row_masks       uint8 [V,H,W]: the rows that are contours of each view, drawn, optionally behind a depth gate
  contour_masks   edge_rows + row_masks
  ignore_zone     the masks widened to a radius with the distance transform of ops.edge_score: the don't-care zone of the
                  2D score (edge_extraction.reprojection.score_edges, ``ignore_contours``)

A row is a contour of a view iff both triangles lie on the same side of the plane through the eye and the edge.  The rule,
the clip and the stepping are frozen in include/curvegs.h -- float64, one rounded operation at a time.  Two back ends:
``"gpu"``, HIP, and ``"host"``, numpy written operation for operation, so the two agree BIT FOR BIT, and so does the
brute-force restatement of tests/mesh_contours_cases.py.  The selection of the rows happens on the host either way: the
kernel sees only the selected rows.

WHAT THIS IS NOT.  Boundary edges of an open mesh (one triangle) are never rows.  By default no near-plane clipping: a row
with an end at or behind the camera plane is skipped whole; ``near_clip=`` (``cgs_mesh_contours_clipped``) cuts it at the
plane instead, for cameras inside the mesh -- off unless asked for.  The silhouette edges of a general, noisy triangulation zigzag across
its facets; the radius of ``ignore_zone`` is meant to absorb that and this is UNMEASURED -- only the drawn solids of
scene/solid_scan.py have been checked.  The zone is known to the 2D score only: the support check, trimming, snapping and
the edge vote do not take it (their per-sample tallies would need a third verdict).  ``CREASE_DEG`` AND ``CONTOUR_RADIUS_PX``
ARE UNTUNED."""
from typing import NamedTuple

import numpy as np
import torch

from .. import _lib as L
from . import edge_occlusion as EO
from . import edge_score as ES

KINDS = ("smooth", "all")
CREASE_DEG = 30.0        # UNTUNED: a fold of up to this angle is smooth
CONTOUR_RADIUS_PX = 2    # UNTUNED: the radius of the score's don't-care zone around a predicted contour


class MeshEdges(NamedTuple):
    rows: np.ndarray        # float32 [E,4,3]: (a, b, c, d) of every edge with exactly two triangles
    cos: np.ndarray         # float64 [E]: the cosine of the fold, 1 = flat; NaN where a triangle is degenerate
    boundary: int           # edges with one triangle (left out)
    non_manifold: int       # edges with more than two triangles (left out)


def mesh_edges(tris):
    """The edge table of float32 [F,3,3] triangles (``read_triangle_mesh``), a ``MeshEdges``.  Vertices are matched by the
    BITS of their three floats (0.0 and -0.0 differ; no tolerance).  A vertex's index is its rank among the distinct vertices
    ordered by those bits as unsigned integers, x then y then z.  Within a row a < b by vertex index, the rows are ordered
    by (a, b), and c belongs to the earlier triangle of the input (d to the later).  The side of a triangle that joins a
    vertex to itself is no edge.  The fold: n1 = (b-a) x (c-a), n2 = (d-a) x (b-a), cos = n1.n2 / (|n1| |n2|) in float64 --
    a flat pair gives 1 whatever the triangles' winding."""
    t = np.ascontiguousarray(ES._host(tris), np.float32)
    if t.ndim != 3 or t.shape[1:] != (3, 3):
        raise ValueError(f"mesh_edges: tris must be [F,3,3] (got {t.shape})")
    F = t.shape[0]
    if F == 0:
        return MeshEdges(np.zeros((0, 4, 3), np.float32), np.zeros((0,), np.float64), 0, 0)
    verts, idx = np.unique(t.reshape(-1, 3).view(np.uint32), axis=0, return_inverse=True)
    idx = idx.reshape(F, 3).astype(np.int64)
    N = verts.shape[0]
    p = idx[:, [0, 1, 2]].reshape(-1)       # the three sides of a triangle, in corner order ...
    q = idx[:, [1, 2, 0]].reshape(-1)
    o = idx[:, [2, 0, 1]].reshape(-1)       # ... and the vertex opposite each
    real = p != q
    p, q, o = p[real], q[real], o[real]
    key = np.minimum(p, q) * N + np.maximum(p, q)
    order = np.argsort(key, kind="stable")  # ties stay in input order: triangle, then corner
    key, o = key[order], o[order]
    uniq, first, count = np.unique(key, return_index=True, return_counts=True)
    two = count == 2
    a, b = uniq[two] // N, uniq[two] % N
    c, d = o[first[two]], o[first[two] + 1]
    xyz = verts.view(np.float32)
    rows = np.ascontiguousarray(np.stack([xyz[a], xyz[b], xyz[c], xyz[d]], 1).reshape(-1, 4, 3))
    A, B, C, D = (rows[:, k].astype(np.float64) for k in range(4))
    n1, n2 = np.cross(B - A, C - A), np.cross(D - A, B - A)
    with np.errstate(all="ignore"):
        cos = (n1 * n2).sum(1) / (np.sqrt((n1 * n1).sum(1)) * np.sqrt((n2 * n2).sum(1)))
    return MeshEdges(rows, cos, int((count == 1).sum()), int((count > 2).sum()))


def smooth(cos, crease_deg=CREASE_DEG):
    """bool [E]: cos >= cos(crease_deg).  A NaN (a degenerate triangle) is never smooth."""
    crease_deg = float(crease_deg)
    if not 0.0 <= crease_deg <= 180.0:
        raise ValueError(f"crease_deg must lie in [0, 180] (got {crease_deg})")
    with np.errstate(invalid="ignore"):
        return np.asarray(cos, np.float64) >= np.cos(np.radians(crease_deg))


def edge_rows(tris, kind="smooth", crease_deg=CREASE_DEG):
    """float32 [E,4,3]: the rows of ``mesh_edges`` that ``kind`` selects, in its order."""
    if kind not in KINDS:
        raise ValueError(f"unknown contour kind {kind!r}: expected one of {KINDS}")
    edges = mesh_edges(tris)
    return edges.rows if kind == "all" else np.ascontiguousarray(edges.rows[smooth(edges.cos, crease_deg)])


# ------------------------------------------------------------------------------------------------ the rule on the host
def _clip_side(p, q, t0, t1, alive):
    """One boundary of the clip for all rows at once: the branches of cgs_mesh_contours as masks."""
    with np.errstate(all="ignore"):
        zero, neg = p == 0.0, p < 0.0
        pos = ~zero & ~neg          # p > 0, and a NaN p: every comparison below then fails
        r = q / p
        alive = alive & ~(zero & (q < 0.0)) & ~(neg & (r > t1)) & ~(pos & (r < t0))
        return np.where(neg & (r > t0), r, t0), np.where(pos & (r < t1), r, t1), alive


def _classify_host(rows64, M, near=None):
    """The contour test of one view for all rows at once: (bool [E], c0, c1, c2 [E,4] -- the camera-space vertices).  With
    ``near`` (cgs_mesh_contours_clipped) a row needs one end with c2 >= near instead of both ends in front of the camera."""
    X, Y, Z = rows64[..., 0], rows64[..., 1], rows64[..., 2]   # [E,4] each
    with np.errstate(all="ignore"):
        c0 = ((M[0] * X + M[1] * Y) + M[2] * Z) + M[3]
        c1 = ((M[4] * X + M[5] * Y) + M[6] * Z) + M[7]
        z = ((M[8] * X + M[9] * Y) + M[10] * Z) + M[11]
        A0, A1, A2, B0, B1, B2 = c0[:, 0], c1[:, 0], z[:, 0], c0[:, 1], c1[:, 1], z[:, 1]
        m0 = A1 * B2 - A2 * B1
        m1 = A2 * B0 - A0 * B2
        m2 = A0 * B1 - A1 * B0
        sc = (m0 * c0[:, 2] + m1 * c1[:, 2]) + m2 * z[:, 2]
        sd = (m0 * c0[:, 3] + m1 * c1[:, 3]) + m2 * z[:, 3]
        ends = (A2 > 0.0) & (B2 > 0.0) if near is None else (A2 >= near) | (B2 >= near)
        return ends & (sc * sd > 0.0), c0, c1, z


def contour_flags(rows, intrinsics, w2c):
    """bool [V,E]: which rows are contours of which view -- the contour test of cgs_mesh_contours alone (both ends in front
    of the camera, both triangles on one side), whether or not anything of the row falls into an image.  numpy."""
    V, _, M = ES._cameras(intrinsics, w2c)
    rows64 = _as_rows(rows).cpu().numpy().astype(np.float64)
    return np.stack([_classify_host(rows64, M[i])[0] for i in range(V)]) if V else np.zeros((0, rows64.shape[0]), bool)


def _contours_view_host(rows64, K, M, height, width, plane, slack, out, near=None):
    """One view of cgs_mesh_contours (near None) or cgs_mesh_contours_clipped in numpy: rows64 float64 [E,4,3] (widened
    float32); plane float32 [H,W] or None; out uint8 [H,W], cleared.  The classification and the clip for all rows at once,
    then one contour at a time."""
    if rows64.shape[0] == 0:
        return
    alive, c0, c1, z = _classify_host(rows64, M, near)
    A0, A1, A2, B0, B1, B2 = c0[:, 0], c1[:, 0], z[:, 0], c0[:, 1], c1[:, 1], z[:, 1]
    if near is not None:   # an OUT end becomes the cut from the IN end toward it (EO.near_cut_host, the z-buffer's)
        with np.errstate(all="ignore"):
            in_a, in_b = A2 >= near, B2 >= near
        A, B = (A0, A1, A2), (B0, B1, B2)
        cut_b, cut_a = EO.near_cut_host(A, B, near), EO.near_cut_host(B, A, near)
        A0, A1, A2 = (np.where(in_a, x, q) for x, q in zip(A, cut_a))
        B0, B1, B2 = (np.where(in_b, x, q) for x, q in zip(B, cut_b))
    with np.errstate(all="ignore"):
        ua, va = K[0] * (A0 / A2) + K[2], K[1] * (A1 / A2) + K[3]
        ub, vb = K[0] * (B0 / B2) + K[2], K[1] * (B1 / B2) + K[3]
        du, dv = ub - ua, vb - va
        wd, hd = float(width), float(height)
        t0, t1 = np.zeros_like(ua), np.ones_like(ua)
        t0, t1, alive = _clip_side(-du, ua, t0, t1, alive)
        t0, t1, alive = _clip_side(du, wd - ua, t0, t1, alive)
        t0, t1, alive = _clip_side(-dv, va, t0, t1, alive)
        t0, t1, alive = _clip_side(dv, hd - va, t0, t1, alive)
        dt = t1 - t0
        length = np.fmax(np.abs(dt * du), np.abs(dt * dv))   # fmax, as the kernel: a NaN operand loses
        alive &= length <= wd + hd
    for e in np.flatnonzero(alive):
        n = int(np.ceil(2.0 * length[e]))
        k = np.arange(n + 1, dtype=np.float64)
        with np.errstate(all="ignore"):
            f = k / float(n) if n > 0 else np.zeros(1, np.float64)
            t = t0[e] + dt[e] * f
            u = ua[e] + t * du[e]
            v = va[e] + t * dv[e]
            keep = (u >= 0.0) & (u < wd) & (v >= 0.0) & (v < hd)
            if plane is not None:
                depth = 1.0 / ((1.0 - t) / A2[e] + t / B2[e])
                keep &= ~EO.hidden_host(depth, u, v, keep, plane, slack)
        out[np.floor(v[keep]).astype(np.int64), np.floor(u[keep]).astype(np.int64)] = 1


# ------------------------------------------------------------------------------------------------ the operators
def _as_rows(rows):
    r = rows if torch.is_tensor(rows) else torch.from_numpy(np.ascontiguousarray(rows, np.float32))
    if r.dim() != 3 or tuple(r.shape[1:]) != (4, 3):
        raise ValueError(f"rows must be [E,4,3] (got {tuple(r.shape)})")
    return r.detach().to(torch.float32).contiguous()


def row_masks(rows, intrinsics, w2c, height, width, depth=None, slack=EO.DEPTH_SLACK, backend="gpu", device=None,
              near_clip=None):
    """uint8 [V,height,width]: 1 on every step of every row (float32 [E,4,3], ``edge_rows``) that is a contour of the view.
    ``depth``: float32 [V,height,width] planes (camera z, +inf = no surface; usually ``mesh_depth`` of the same mesh) --
    a step behind them by more than ``slack`` is dropped --, or None: nothing is hidden and the slack is not read.
    ``backend="gpu"``: ``cgs_mesh_contours``, rows and planes are uploaded when they are not on a GPU, the result stays on the
    device; ``"host"``: numpy, a CPU tensor.  ``near_clip``: None -- a row with an end at or behind the camera plane is
    skipped whole --, or the near plane (finite, > 0): such a row is cut at c2 == near_clip
    (``cgs_mesh_contours_clipped``), as ``mesh_depth`` cuts the triangles."""
    ES._check_backend(backend)
    height, width = ES._check_size("row_masks", height, width)
    near = EO._check_near("row_masks", near_clip)
    V, K, M = ES._cameras(intrinsics, w2c)
    r = _as_rows(rows)
    if backend == "host":
        planes = None
        if depth is not None:
            planes, slack = EO.operator_depth("row_masks", depth, slack, V, height, width, "host")
        rows64 = r.cpu().numpy().astype(np.float64)
        mask = np.zeros((V, height, width), np.uint8)
        for i in range(V):
            _contours_view_host(rows64, K[i], M[i], height, width, None if planes is None else planes[i], slack, mask[i],
                                near)
        return torch.from_numpy(mask)
    dev = ES._device_for([r] + ([depth] if torch.is_tensor(depth) else []), "row_masks", device)
    with L.device_guard(dev):
        d = None
        if depth is not None:
            d, slack = EO.operator_depth("row_masks", depth, slack, V, height, width, "gpu", dev)
        r = r.to(dev)
        mask = torch.empty((V, height, width), dtype=torch.uint8, device=dev)
        if V > 0:
            Kd, Md = ES.cameras_on(dev, K, M)
            sl = float(slack) if d is not None else 0.0
            if near is None:
                rc = L.load().cgs_mesh_contours(int(r.shape[0]), L.ptr(r), V, L.ptr(Kd), L.ptr(Md), height, width, L.ptr(d),
                                                sl, L.ptr(mask), L.raw_stream(dev))
                L.check(rc, "cgs_mesh_contours")
            else:
                rc = L.load().cgs_mesh_contours_clipped(int(r.shape[0]), L.ptr(r), V, L.ptr(Kd), L.ptr(Md), height, width,
                                                        L.ptr(d), sl, near, L.ptr(mask), L.raw_stream(dev))
                L.check(rc, "cgs_mesh_contours_clipped")
    return mask


def contour_masks(tris, intrinsics, w2c, height, width, depth=None, slack=EO.DEPTH_SLACK, kind="smooth",
                  crease_deg=CREASE_DEG, backend="gpu", device=None, near_clip=None):
    """uint8 [V,height,width]: the contours of the mesh (float32 [F,3,3] triangles) in every view -- ``row_masks`` of
    ``edge_rows(tris, kind, crease_deg)``.  ``kind="smooth"``: the view-dependent contours of curved surfaces;
    ``"all"``: the outline of every two-triangle edge, with ``depth`` the hidden-line-removed outline."""
    return row_masks(edge_rows(tris, kind, crease_deg), intrinsics, w2c, height, width, depth, slack, backend, device,
                     near_clip)


def _check_radius(what, radius_px):
    r = float(radius_px)
    if not 0.0 <= r <= L.EDT_MAX_SIZE:
        raise ValueError(f"{what}: the contour radius must lie in [0, {L.EDT_MAX_SIZE}] pixels (got {radius_px})")
    return r


def ignore_zone(masks, radius_px=CONTOUR_RADIUS_PX, backend="gpu", device=None):
    """bool [V,H,W]: the pixels within ``radius_px`` (Euclidean, dist^2 <= radius^2) of a set pixel of ``masks`` -- the
    distance transform of ``ops.edge_score.edt_squared``, so integers on both back ends.  Stays where the back end works."""
    r2 = int(np.floor(_check_radius("ignore_zone", radius_px) ** 2))
    return ES.edt_squared(masks, backend=backend, device=device) <= r2
