"""Occlusion for the 2D operators: depth planes from a triangle mesh or from the user, and the prediction mask gated by
them (cgs_mesh_depth / cgs_depth_window_max / cgs_point_mask_depth, include/curvegs.h; csrc/edge_occlusion.hip).  The
reference has no counterpart.

  mesh_depth          the mesh rendered into one camera-z plane per view -- a z-buffer, +inf where no triangle covers the
                      pixel centre -- followed by the window maximum
  surfel_depth        the same planes from an ORIENTED POINT CLOUD, a ``Surfels(points, normals, radii)``: every point a
                      disk around it, normal to its normal (cgs_surfel_depth; csrc/surfel_depth.hip) -- for a scan made
                      from photographs, which has COLMAP's fused.ply and neither a mesh nor depth maps.  A disk overhangs
                      a silhouette by up to its radius, so a cloud hides slightly MORE than the surface it samples
  surfel_radii        a cloud's radii from its 3 nearest neighbours (cgs_knn_mean_dist2): ``SURFEL_RADIUS_FACTOR`` x the
                      root of their mean squared distance, capped at ``SURFEL_RADIUS_CAP`` median radii; BOTH UNTUNED
  read_occluder       what an occluder file holds: triangles (``read_triangle_mesh``), or the ``Surfels`` of a PLY that
                      has vertices and no faces; write_surfel_ply writes one
  depth_window_max    the maximum over a (2r+1)^2 window clipped to the image: +inf (no surface) wins
  point_masks_depth   ``ops.edge_score.point_masks`` with the gate: a sample the projection keeps is HIDDEN iff
                          c2 > float64(depth[v][floor(v_px)][floor(u_px)]) + slack
                      with c2 its camera-space depth; a hidden sample marks no pixel and counts in ``hidden``
  check_depth_maps    the user's own depth maps (camera z, one float [H,W] array per camera) made ready: NaN and <= 0
                      become +inf
  read_triangle_mesh  float32 [F,3,3] from an .obj or .ply file, without trimesh or open3d
  hidden_host         the rule for one view in numpy, the host back ends' one statement of it; gate_view_host: the
                      projection and the rule together, what the gated 2D operators' host back ends call per view
  ChunkDepth          a scan's depth source -- an occluder or the user's maps -- asked per chunk of views, with the
                      settings a result records and the bytes per pixel it adds

The rules are frozen in include/curvegs.h -- float64, one rounded operation at a time -- and the one occlusion rule is the
device function ``nv_hidden`` of csrc/point_projection.h.  Two back ends: ``"gpu"``, HIP, and ``"host"``, numpy written
operation for operation (numpy evaluates one rounded operation per ufunc call), so the two agree BIT FOR BIT, and so do the
brute-force restatements of tests/edge_occlusion_cases.py.

Why the window: a sample on a visible edge lies somewhere inside its pixel while the plane holds the surface's depth at the
pixel CENTRE, which on a slanted face differs by far more than any sensible slack.  On a convex solid the depth is a convex
function of the image point and the sample lies inside the hull of the nine centres around it, so the maximum over them is
at least the sample's own depth; at a silhouette one of the nine has no surface and the sample is never hidden.

WHAT THIS IS NOT.  By default no clipping: a triangle with a vertex at or behind the camera plane is dropped whole, which
is right for a solid seen from outside and wrong for a camera INSIDE its occluder (a room, a coarse proxy mesh): there
``near_clip=`` (``mesh_depth``, ``ChunkDepth``; ``cgs_mesh_depth_clipped``) cuts such a triangle at the plane c2 == near_clip
and keeps what is in front.  It stays off unless asked for; ``NEAR_CLIP`` IS UNTUNED and only the drawn room of
scene/solid_scan.py has been checked.  A sample nearer than the plane is still seen and can only be hidden by a surface at
or beyond it.  The rule has
five consumers: the score's prediction mask (``point_masks_depth``) and, opt-in, the support check, trimming, oriented
trimming and snapping (``support_counts``, ``sample_tally``, ``oriented_tally`` and ``snap_terms`` with ``depth=``; DESIGN.md
4.8u), which share ``hidden_host`` / ``gate_view_host`` on the host and ``ChunkDepth`` for a scan's planes.  The edge vote
(ops/edge_seed.py) takes it the same way, opt-in, for a voxel's centre; the control-point visibility check
(``edge_extraction.para_edge``) is ungated unless ``get_parametric_edge`` is given ``occluder=`` / ``depth_maps=``, and the
drawn views (``edge_extraction.novel_view``) unless their drivers are (opt-in, like the others).  Along a CONCAVE edge the surface's depth is a local maximum, so samples of a visible concave edge can be
hidden by their own faces where the faces are steep; a larger slack trades that against hiding less behind thin parts.
``DEPTH_WINDOW`` AND ``DEPTH_SLACK`` ARE UNTUNED: only the drawn solids of scene/solid_scan.py have been checked, no real
scan."""
import os
from typing import NamedTuple

import numpy as np
import torch

from .. import _lib as L
from . import edge_score as ES

SURFEL_RADIUS_FACTOR = 1.0       # UNTUNED: a disk's radius over the root of its point's mean squared 3-NN distance; the
                                 # smallest of (0.6, 0.8, 1.0, 1.2) that leaves no hole in the sampled box and cylinder of
                                 # tests/test_surfel_depth_cpu.py (profiles/surfel_depth.md)
SURFEL_RADIUS_CAP = 4.0          # UNTUNED: no radius above this many median radii (a lone outlier has far neighbours)
MAX_WINDOW = L.DEPTH_MAX_WINDOW
DEPTH_WINDOW = 1                 # UNTUNED
DEPTH_SLACK = 2 * 0.0005         # UNTUNED: 2 x edge_extraction.reprojection.SAMPLE_RESOLUTION, in world units
NEAR_CLIP = 0.01                 # UNTUNED: the near plane of the clipped z-buffer, in world units, for scenes in the unit cube;
                                 # synthetic.make_camera's znear


def _check_window(what, window):
    window = int(window)
    if not 0 <= window <= MAX_WINDOW:
        raise ValueError(f"{what}: the window radius must lie in [0, {MAX_WINDOW}] (got {window})")
    return window


def _check_slack(what, slack):
    slack = float(slack)
    if not (slack >= 0.0 and np.isfinite(slack)):
        raise ValueError(f"{what}: the slack must be finite and >= 0 (got {slack})")
    return slack


def _check_near(what, near_clip):
    """None (no clipping), or the near plane as a float: finite and > 0."""
    if near_clip is None:
        return None
    near = float(near_clip)
    if not (near > 0.0 and np.isfinite(near)):
        raise ValueError(f"{what}: near_clip must be finite and > 0 (got {near_clip})")
    return near


def _as_tris(tris):
    """float32 [F,3,3] as a contiguous float32 tensor (on the device it is on)."""
    t = tris if torch.is_tensor(tris) else torch.from_numpy(np.ascontiguousarray(tris, np.float32))
    if t.dim() != 3 or tuple(t.shape[1:]) != (3, 3):
        raise ValueError(f"tris must be [F,3,3] (got {tuple(t.shape)})")
    return t.detach().to(torch.float32).contiguous()


def _as_depth(depth, V, height, width, what):
    if not torch.is_tensor(depth):
        a = np.ascontiguousarray(depth)
        depth = torch.from_numpy(a if a.flags.writeable else a.copy())   # (a tensor cannot share a read-only array)
    d = depth
    if d.dtype != torch.float32 or tuple(d.shape) != (V, height, width):
        raise ValueError(f"{what}: depth must be float32 [{V},{height},{width}] (got {d.dtype} {tuple(d.shape)})")
    return d.detach().contiguous()


# ------------------------------------------------------------------------------------------------ z-buffer
def _camera_points_host(P, K, M):
    """(c2, u, v) of float64 points P [...,3] in one camera (K [4], M [12]): the operation order of cgs_project_points."""
    X, Y, Z = P[..., 0], P[..., 1], P[..., 2]
    with np.errstate(all="ignore"):
        c0 = ((M[0] * X + M[1] * Y) + M[2] * Z) + M[3]
        c1 = ((M[4] * X + M[5] * Y) + M[6] * Z) + M[7]
        c2 = ((M[8] * X + M[9] * Y) + M[10] * Z) + M[11]
        u = K[0] * (c0 / c2) + K[2]
        v = K[1] * (c1 / c2) + K[3]
    return c2, u, v


def near_cut_host(a, b, near):
    """THE cut of cgs_mesh_depth_clipped in numpy, from the IN ends a toward the OUT ends b: (c0, c1, c2) float64 [N] each of
    a, b -> the cut points, c2 assigned.  The host back ends' one statement of it (the contours share it)."""
    with np.errstate(all="ignore"):
        t = (a[2] - near) / (a[2] - b[2])
        return a[0] + t * (b[0] - a[0]), a[1] + t * (b[1] - a[1]), np.full_like(t, near)


def _clip_host(T, M, near):
    """The pieces of cgs_mesh_depth_clipped in one view: camera-space (c0, c1, c2), float64 [G,3] each.  T float64 [F,3,3]."""
    X, Y, Z = T[..., 0], T[..., 1], T[..., 2]
    with np.errstate(all="ignore"):
        c = np.stack([((M[0] * X + M[1] * Y) + M[2] * Z) + M[3], ((M[4] * X + M[5] * Y) + M[6] * Z) + M[7],
                      ((M[8] * X + M[9] * Y) + M[10] * Z) + M[11]])          # [3 (coordinate), F, 3 (vertex)]
        c = c[:, ~np.isnan(c).any(axis=(0, 2))]
        inn = c[2] >= near
    nin = inn.sum(1)
    pieces = [c[:, nin == 3]]
    for count in (1, 2):
        sel = nin == count
        if not sel.any():
            continue
        cs, ins = c[:, sel], inn[sel]
        i = np.argmax(ins, 1) if count == 1 else np.argmin(ins, 1)   # the one IN, or the one OUT
        rows = np.arange(cs.shape[1])
        r0, r1, r2 = (tuple(cs[k][rows, (i + d) % 3] for k in range(3)) for d in range(3))
        if count == 1:       # a = r0, b = r1, c = r2: (a, cut(a,b), cut(a,c))
            tri = [(r0, near_cut_host(r0, r1, near), near_cut_host(r0, r2, near))]
        else:                # c = r0, a = r1, b = r2: (a, b, cut(b,c)), (a, cut(b,c), cut(a,c))
            qb, qa = near_cut_host(r2, r0, near), near_cut_host(r1, r0, near)
            tri = [(r1, r2, qb), (r1, qb, qa)]
        for verts in tri:
            pieces.append(np.stack([np.stack([vtx[k] for vtx in verts], 1) for k in range(3)]))
    c = np.concatenate(pieces, 1)
    return c[0], c[1], c[2]


def _zbuffer_host(T, K, M, height, width, near=None):
    """One view of cgs_mesh_depth (near None) or cgs_mesh_depth_clipped in numpy: T float64 [F,3,3] (widened float32),
    float32 [height,width]."""
    plane = np.full((height, width), np.inf, np.float32)
    if T.shape[0] == 0:
        return plane
    if near is None:
        z, u, v = _camera_points_host(T, K, M)   # [F,3] each
    else:
        c0, c1, z = _clip_host(T, M, near)       # [G,3] each: the pieces' camera-space vertices
        if z.shape[0] == 0:
            return plane
        with np.errstate(all="ignore"):
            u = K[0] * (c0 / z) + K[2]
            v = K[1] * (c1 / z) + K[3]
    with np.errstate(all="ignore"):
        ok = (z > 0.0).all(1) & ~np.isnan(u).any(1) & ~np.isnan(v).any(1)
        area = (u[:, 1] - u[:, 0]) * (v[:, 2] - v[:, 0]) - (v[:, 1] - v[:, 0]) * (u[:, 2] - u[:, 0])
        ok &= (area != 0.0) & ~np.isnan(area)
        wd, hd = float(width), float(height)
        umin, umax = np.minimum(np.minimum(u[:, 0], u[:, 1]), u[:, 2]), np.maximum(np.maximum(u[:, 0], u[:, 1]), u[:, 2])
        vmin, vmax = np.minimum(np.minimum(v[:, 0], v[:, 1]), v[:, 2]), np.maximum(np.maximum(v[:, 0], v[:, 1]), v[:, 2])
        jlo = np.minimum(np.maximum(np.ceil(umin - 0.5), 0.0), wd)
        jhi = np.maximum(np.minimum(np.floor(umax - 0.5), wd - 1.0), -1.0)
        ilo = np.minimum(np.maximum(np.ceil(vmin - 0.5), 0.0), hd)
        ihi = np.maximum(np.minimum(np.floor(vmax - 0.5), hd - 1.0), -1.0)
        ok &= (jlo <= jhi) & (ilo <= ihi)
    for t in np.nonzero(ok)[0]:
        j0, j1, i0, i1 = int(jlo[t]), int(jhi[t]), int(ilo[t]), int(ihi[t])
        px = (np.arange(j0, j1 + 1, dtype=np.float64) + 0.5)[None, :]
        py = (np.arange(i0, i1 + 1, dtype=np.float64) + 0.5)[:, None]
        (u0, u1, u2), (v0, v1, v2), (z0, z1, z2), a = u[t], v[t], z[t], area[t]
        with np.errstate(all="ignore"):
            e0 = (u2 - u1) * (py - v1) - (v2 - v1) * (px - u1)
            e1 = (u0 - u2) * (py - v2) - (v0 - v2) * (px - u2)
            e2 = (u1 - u0) * (py - v0) - (v1 - v0) * (px - u0)
            covered = ((e0 >= 0.0) & (e1 >= 0.0) & (e2 >= 0.0)) | ((e0 <= 0.0) & (e1 <= 0.0) & (e2 <= 0.0))
            invz = ((e0 / a) / z0 + (e1 / a) / z1) + (e2 / a) / z2
            zf = (1.0 / invz).astype(np.float32)
            store = covered & (zf > 0.0) & np.isfinite(zf)
        sub = plane[i0:i1 + 1, j0:j1 + 1]
        np.minimum(sub, np.where(store, zf, np.float32(np.inf)), out=sub)
    return plane


def _window_max_host(depth, radius):
    """cgs_depth_window_max in numpy on float32 [V,H,W]: a NaN never wins."""
    d = np.asarray(depth, np.float32)
    if radius == 0 or d.size == 0:
        return np.where(d > -np.inf, d, np.float32(-np.inf)).astype(np.float32)
    for axis in (2, 1):
        pad = [(0, 0)] * 3
        pad[axis] = (radius, radius)
        p = np.pad(d, pad, constant_values=-np.inf)
        n = d.shape[axis]
        m = np.full(d.shape, -np.inf, np.float32)
        for k in range(2 * radius + 1):
            a = np.take(p, range(k, k + n), axis=axis)
            m = np.where(a > m, a, m)
        d = m
    return d


def depth_window_max(depth, radius, backend="gpu", device=None):
    """float32 [V,H,W] -> float32 [V,H,W]: the maximum over the (2 radius + 1)^2 window clipped to the image, 0 <= radius <=
    MAX_WINDOW.  ``backend="gpu"``: ``cgs_depth_window_max``, the result stays on the device; ``"host"``: numpy."""
    ES._check_backend(backend)
    radius = _check_window("depth_window_max", radius)
    d = depth if torch.is_tensor(depth) else torch.from_numpy(np.array(depth, order="C"))   # (a copy: may be read-only)
    if d.dtype != torch.float32 or d.dim() != 3:
        raise ValueError(f"depth_window_max: depth must be float32 [V,H,W] (got {d.dtype} {tuple(d.shape)})")
    V, H, W = (int(s) for s in d.shape)
    if V > 0:
        ES._check_size("depth_window_max", H, W)
    if backend == "host":
        return torch.from_numpy(_window_max_host(ES._host(d), radius))
    dev = ES._device_for([d], "depth_window_max", device)
    with L.device_guard(dev):
        d = d.detach().to(dev).contiguous()
        out = torch.empty_like(d)
        if V > 0:
            rc = L.load().cgs_depth_window_max(V, H, W, radius, L.ptr(d), L.ptr(out), L.raw_stream(dev))
            L.check(rc, "cgs_depth_window_max")
    return out


def mesh_depth(tris, intrinsics, w2c, height, width, window=DEPTH_WINDOW, backend="gpu", device=None, near_clip=None):
    """float32 [V,height,width]: the camera-z of the nearest triangle at every pixel centre (+inf where there is none), then
    the window maximum of radius ``window`` (0: the plain z-buffer).  tris float32 [F,3,3] (tensor or array); intrinsics
    [V,4] and w2c [V,3,4] as ``point_masks``.  ``backend="gpu"``: ``cgs_mesh_depth`` and ``cgs_depth_window_max``, the
    triangles are uploaded when they are not on a GPU, the result stays on the device; ``"host"``: numpy, a CPU tensor.
    ``near_clip``: None -- a triangle with a vertex at or behind the camera plane is dropped whole --, or the near plane
    (world units, finite, > 0; ``NEAR_CLIP``): such a triangle is clipped at c2 == near_clip (``cgs_mesh_depth_clipped``),
    which a camera INSIDE its occluder needs; with every vertex in front of the plane the bits are the same."""
    ES._check_backend(backend)
    height, width = ES._check_size("mesh_depth", height, width)
    window = _check_window("mesh_depth", window)
    near = _check_near("mesh_depth", near_clip)
    V, K, M = ES._cameras(intrinsics, w2c)
    t = _as_tris(tris)
    if backend == "host":
        T = t.cpu().numpy().astype(np.float64)
        raw = np.empty((V, height, width), np.float32)
        for i in range(V):
            raw[i] = _zbuffer_host(T, K[i], M[i], height, width, near)
        return torch.from_numpy(_window_max_host(raw, window) if window else raw)
    dev = ES._device_for([t], "mesh_depth", device)
    with L.device_guard(dev):
        t = t.to(dev)
        raw = torch.empty((V, height, width), dtype=torch.float32, device=dev)
        if V > 0:
            Kd, Md = ES.cameras_on(dev, K, M)
            if near is None:
                rc = L.load().cgs_mesh_depth(int(t.shape[0]), L.ptr(t), V, L.ptr(Kd), L.ptr(Md), height, width, L.ptr(raw),
                                             L.raw_stream(dev))
                L.check(rc, "cgs_mesh_depth")
            else:
                rc = L.load().cgs_mesh_depth_clipped(int(t.shape[0]), L.ptr(t), V, L.ptr(Kd), L.ptr(Md), height, width, near,
                                                     L.ptr(raw), L.raw_stream(dev))
                L.check(rc, "cgs_mesh_depth_clipped")
    return depth_window_max(raw, window, "gpu", dev) if window else raw


# ------------------------------------------------------------------------------------------------ surfel z-buffer
class Surfels(NamedTuple):
    """An oriented point cloud as an occluder: every point a disk of its own radius around it, normal to its normal."""
    points: object            # float32 [P,3]
    normals: object           # float32 [P,3], or None: every disk faces the camera plane of the view that draws it
    radii: object             # float32 [P], world units


def _as_surfels(surfels):
    """A ``Surfels`` as contiguous float32 tensors (each on the device it is on): (points [P,3], normals [P,3] or None,
    radii [P])."""
    def tensor(x):
        t = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x, np.float32))
        return t.detach().to(torch.float32).contiguous()
    if not isinstance(surfels, Surfels):
        raise ValueError(f"surfels must be a Surfels(points, normals, radii) (got {type(surfels).__name__})")
    pts, rad = tensor(surfels.points), tensor(surfels.radii)
    nrm = None if surfels.normals is None else tensor(surfels.normals)
    if pts.dim() != 2 or pts.shape[1] != 3:
        raise ValueError(f"surfels: points must be [P,3] (got {tuple(pts.shape)})")
    P = int(pts.shape[0])
    if tuple(rad.shape) != (P,) or (nrm is not None and tuple(nrm.shape) != (P, 3)):
        raise ValueError(f"surfels: normals must be [{P},3] or None and radii [{P}] (got "
                         f"{None if nrm is None else tuple(nrm.shape)}, {tuple(rad.shape)})")
    return pts, nrm, rad


SURFEL_HOST_PAIRS = 1 << 21      # (surfel, candidate pixel) pairs the host back end holds at a time


def _surfel_zbuffer_host(X, N, R, K, M, height, width):
    """One view of cgs_surfel_depth in numpy: X float64 [P,3], N float64 [P,3] or None, R float64 [P] (all widened float32);
    float32 [height,width].  The set-up is vectorised over the surfels and the pixel rule over the (surfel, candidate pixel)
    pairs of a run of surfels; every operation is elementwise, so the grouping does not show in the bits."""
    plane = np.full((height, width), np.inf, np.float32)
    if X.shape[0] == 0:
        return plane
    with np.errstate(all="ignore"):
        c0 = ((M[0] * X[:, 0] + M[1] * X[:, 1]) + M[2] * X[:, 2]) + M[3]
        c1 = ((M[4] * X[:, 0] + M[5] * X[:, 1]) + M[6] * X[:, 2]) + M[7]
        c2 = ((M[8] * X[:, 0] + M[9] * X[:, 1]) + M[10] * X[:, 2]) + M[11]
        if N is None:
            n0, n1, n2 = np.zeros_like(c0), np.zeros_like(c0), np.ones_like(c0)
        else:
            n0 = (M[0] * N[:, 0] + M[1] * N[:, 1]) + M[2] * N[:, 2]
            n1 = (M[4] * N[:, 0] + M[5] * N[:, 1]) + M[6] * N[:, 2]
            n2 = (M[8] * N[:, 0] + M[9] * N[:, 1]) + M[10] * N[:, 2]
        zlo, zhi = c2 - R, c2 + R
        ok = (R > 0.0) & (zlo > 0.0)
        a0, b0, a1, b1 = c0 - R, c0 + R, c1 - R, c1 + R
        ulo = K[0] * np.fmin(a0 / zlo, a0 / zhi) + K[2]      # fmin / fmax: a NaN operand loses, as the device's
        uhi = K[0] * np.fmax(b0 / zlo, b0 / zhi) + K[2]
        vlo = K[1] * np.fmin(a1 / zlo, a1 / zhi) + K[3]
        vhi = K[1] * np.fmax(b1 / zlo, b1 / zhi) + K[3]
        ok &= ~(np.isnan(ulo) | np.isnan(uhi) | np.isnan(vlo) | np.isnan(vhi))
        wd, hd = float(width), float(height)
        jlo = np.fmin(np.fmax(np.ceil(ulo - 0.5), 0.0), wd)
        jhi = np.fmax(np.fmin(np.floor(uhi - 0.5), wd - 1.0), -1.0)
        ilo = np.fmin(np.fmax(np.ceil(vlo - 0.5), 0.0), hd)
        ihi = np.fmax(np.fmin(np.floor(vhi - 0.5), hd - 1.0), -1.0)
        ok &= (jlo <= jhi) & (ilo <= ihi)
        num = (n0 * c0 + n1 * c1) + n2 * c2
        r2 = R * R
    live = np.flatnonzero(ok)
    if live.size == 0:
        return plane
    j0, i0 = jlo[live].astype(np.int64), ilo[live].astype(np.int64)
    bw = jhi[live].astype(np.int64) - j0 + 1
    count = bw * (ihi[live].astype(np.int64) - i0 + 1)
    flat = plane.reshape(-1)
    ends = np.cumsum(count)
    at = 0
    while at < live.size:
        # a run of surfels whose boxes hold about SURFEL_HOST_PAIRS pixels together (one surfel at least)
        stop = max(at + 1, int(np.searchsorted(ends, (ends[at - 1] if at else 0) + SURFEL_HOST_PAIRS, side="right")))
        n = count[at:stop]
        rep = np.repeat(np.arange(at, stop), n)
        local = np.arange(int(n.sum()), dtype=np.int64) - np.repeat(np.cumsum(n) - n, n)
        row = local // bw[rep]
        i, j = i0[rep] + row, j0[rep] + (local - row * bw[rep])
        s_ = live[rep]
        with np.errstate(all="ignore"):
            px, py = j.astype(np.float64) + 0.5, i.astype(np.float64) + 0.5
            dx, dy = (px - K[2]) / K[0], (py - K[3]) / K[1]
            den = (n0[s_] * dx + n1[s_] * dy) + n2[s_]
            s = num[s_] / den
            qx, qy, qz = s * dx - c0[s_], s * dy - c1[s_], s - c2[s_]
            d2 = (qx * qx + qy * qy) + qz * qz
            zf = s.astype(np.float32)
            store = (d2 <= r2[s_]) & (zf > 0.0) & np.isfinite(zf)
        pix, zf = (i * width + j)[store], zf[store]
        if pix.size:
            order = np.argsort(pix, kind="stable")
            pix, zf = pix[order], zf[order]
            first = np.flatnonzero(np.r_[True, pix[1:] != pix[:-1]])
            flat[pix[first]] = np.minimum(flat[pix[first]], np.minimum.reduceat(zf, first))
        at = stop
    return plane


def surfel_depth(surfels, intrinsics, w2c, height, width, window=DEPTH_WINDOW, backend="gpu", device=None):
    """``mesh_depth`` for an oriented point cloud: float32 [V,height,width], the camera-z of the nearest disk at every pixel
    centre (+inf where there is none), then the window maximum of radius ``window`` (0: the plain z-buffer).  ``surfels``: a
    ``Surfels`` (tensors or arrays); intrinsics [V,4] and w2c [V,3,4] as ``point_masks``.  ``backend="gpu"``:
    ``cgs_surfel_depth`` and ``cgs_depth_window_max``, the cloud is uploaded when it is not on a GPU, the result stays on the
    device; ``"host"``: numpy, a CPU tensor, the same bits.  A disk that could reach the camera plane (c2 - r <= 0) is
    dropped whole: there is no near-plane clipping of disks."""
    ES._check_backend(backend)
    height, width = ES._check_size("surfel_depth", height, width)
    window = _check_window("surfel_depth", window)
    V, K, M = ES._cameras(intrinsics, w2c)
    pts, nrm, rad = _as_surfels(surfels)
    if backend == "host":
        X = pts.cpu().numpy().astype(np.float64)
        N = None if nrm is None else nrm.cpu().numpy().astype(np.float64)
        R = rad.cpu().numpy().astype(np.float64)
        raw = np.empty((V, height, width), np.float32)
        for i in range(V):
            raw[i] = _surfel_zbuffer_host(X, N, R, K[i], M[i], height, width)
        return torch.from_numpy(_window_max_host(raw, window) if window else raw)
    dev = ES._device_for([pts, nrm, rad], "surfel_depth", device)
    with L.device_guard(dev):
        pts, rad = pts.to(dev), rad.to(dev)
        nrm = None if nrm is None else nrm.to(dev)
        raw = torch.empty((V, height, width), dtype=torch.float32, device=dev)
        if V > 0:
            Kd, Md = ES.cameras_on(dev, K, M)
            rc = L.load().cgs_surfel_depth(int(pts.shape[0]), L.ptr(pts), L.ptr(nrm), L.ptr(rad), V, L.ptr(Kd), L.ptr(Md),
                                           height, width, L.ptr(raw), L.raw_stream(dev))
            L.check(rc, "cgs_surfel_depth")
    return depth_window_max(raw, window, "gpu", dev) if window else raw


def _knn_mean_dist2_host(pts):
    """The mean squared distance to the 3 nearest other points, float64 from float32 points, as float32 [P]; +inf with
    fewer than 4 points, as ``cgs_knn_mean_dist2``.  scipy's k-d tree where there is one, else brute force."""
    X = np.asarray(pts, np.float32).reshape(-1, 3).astype(np.float64)
    P = X.shape[0]
    if P < 4:
        return np.full((P,), np.inf, np.float32)
    try:
        from scipy.spatial import cKDTree
        d = cKDTree(X).query(X, k=4)[0][:, 1:]             # (itself first, at 0; with exact copies a copy stands in for it)
        return (d * d).mean(1).astype(np.float32)
    except ImportError:
        out = np.empty((P,), np.float32)
        for a in range(0, P, 1024):
            d2 = ((X[a:a + 1024, None, :] - X[None, :, :]) ** 2).sum(2)
            d2[np.arange(d2.shape[0]), np.arange(a, a + d2.shape[0])] = np.inf
            out[a:a + 1024] = np.sort(d2, 1)[:, :3].mean(1).astype(np.float32)
        return out


def surfel_radii(points, factor=SURFEL_RADIUS_FACTOR, backend="gpu", device=None):
    """float32 [P] (a host array): ``factor * sqrt(mean_dist2)`` of every point, with mean_dist2 the mean squared distance to
    its 3 nearest neighbours -- ``cgs_knn_mean_dist2``, the initialiser's kernel, for ``backend="gpu"``; an exact host 3-NN
    for ``"host"`` --, capped at ``SURFEL_RADIUS_CAP`` x the cloud's median radius: a lone outlier has far neighbours and
    would otherwise get a giant disk.  The two back ends agree to float32 rounding of mean_dist2, not to the bit.  Fewer than
    4 points have no 3 neighbours: their radii are +inf, which ``surfel_depth`` skips."""
    ES._check_backend(backend)
    factor = float(factor)
    if not (factor > 0.0 and np.isfinite(factor)):
        raise ValueError(f"surfel_radii: the factor must be finite and > 0 (got {factor})")
    pts = points if torch.is_tensor(points) else torch.from_numpy(np.ascontiguousarray(points, np.float32).reshape(-1, 3))
    if pts.dim() != 2 or pts.shape[1] != 3:
        raise ValueError(f"points must be [P,3] (got {tuple(pts.shape)})")
    pts = pts.detach().to(torch.float32)
    if backend == "host":
        md2 = _knn_mean_dist2_host(pts.cpu().numpy())
    else:
        from ..simple_knn import distCUDA2
        md2 = distCUDA2(pts.to(ES._device_for([pts], "surfel_radii", device))).cpu().numpy()
    with np.errstate(all="ignore"):
        r = factor * np.sqrt(md2.astype(np.float64))
    finite = r[np.isfinite(r)]
    if finite.size:
        r = np.minimum(r, SURFEL_RADIUS_CAP * float(np.median(finite)))
    return r.astype(np.float32)


# ------------------------------------------------------------------------------------------------ the rule on the host
def hidden_host(c2, u, v, keep, plane, slack):
    """``nv_hidden`` in numpy for one view, the host back ends' one statement of the rule: bool [P], True where a sample that
    the projection keeps (``keep`` bool [P]; only those are looked up) has c2 > float64(plane[floor(v)][floor(u)]) + slack.
    c2, u, v float64 [P] as the projection forms them; plane float32 [H,W].  A NaN depth hides nothing."""
    hid = np.zeros(keep.shape, bool)
    idx = np.flatnonzero(keep)
    row, col = np.floor(v[idx]).astype(np.int64), np.floor(u[idx]).astype(np.int64)
    with np.errstate(all="ignore"):
        hid[idx] = c2[idx] > plane[row, col].astype(np.float64) + slack
    return hid


def gate_view_host(points, K, M, plane, slack):
    """One view of a gated operator on the host: (u, v, seen, hidden), float64 [P] and bool [P].  points float32 [P,3]; K [4],
    M [12]; plane float32 [H,W].  The projection is ``cgs_project_points`` operation for operation; ``seen`` are the samples
    it keeps that ``hidden_host`` does not hide, ``hidden`` those it does: seen | hidden is the ungated operators' keep."""
    H, W = plane.shape
    c2, u, v = _camera_points_host(np.asarray(points, np.float32).reshape(-1, 3).astype(np.float64), K, M)
    with np.errstate(all="ignore"):
        keep = ~(c2 <= 0.0) & (u >= 0.0) & (u < float(W)) & (v >= 0.0) & (v < float(H))   # NaN fails the image test
    hid = hidden_host(c2, u, v, keep, plane, slack)
    return u, v, keep & ~hid, hid


def operator_depth(what, depth, slack, V, height, width, backend, dev=None):
    """The ``depth`` and ``slack`` arguments of a gated operator, checked: (float32 [V,height,width] -- a numpy array for
    ``backend="host"``, a tensor on ``dev`` otherwise --, the slack as a float)."""
    slack = _check_slack(what, slack)
    d = _as_depth(depth, V, height, width, what)
    if backend == "host":
        if d.is_cuda:
            raise ValueError(f"{what}: backend='host' takes host arrays and CPU tensors")
        return d.numpy(), slack
    if d.is_cuda and d.device != dev:
        raise L.CurveGSError(f"{what}: depth is on {d.device}, the other tensors on {dev}: all tensors must be on one device")
    return d.to(dev), slack


def check_hidden_out(what, hidden_out, depth, P):
    """The ``hidden_out`` argument of a per-sample gated operator: None, or a contiguous int32 [P] tensor (needs ``depth``)."""
    if hidden_out is None:
        return
    if depth is None:
        raise ValueError(f"{what}: hidden_out needs depth")
    if (not torch.is_tensor(hidden_out) or hidden_out.dtype != torch.int32 or tuple(hidden_out.shape) != (P,)
            or not hidden_out.is_contiguous()):
        raise ValueError(f"{what}: hidden_out must be a contiguous int32 [{P}] tensor")


# ------------------------------------------------------------------------------------------------ the gated mask
def point_masks_depth(points, intrinsics, w2c, depth, slack=DEPTH_SLACK, backend="gpu", device=None, return_counts=False):
    """uint8 [V,H,W]: ``point_masks`` of the samples that are not hidden behind ``depth`` (float32 [V,H,W], camera z, +inf =
    no surface; its size is the views' size).  With return_counts, also (kept, hidden) int32 [V]: the seen samples that are
    not hidden and those that are; kept + hidden is ``point_masks``'s kept.  ``backend="gpu"``: ``cgs_point_mask_depth``,
    points and planes are uploaded when they are not on a GPU, the results stay on the device; ``"host"``: numpy."""
    ES._check_backend(backend)
    slack = _check_slack("point_masks_depth", slack)
    V, K, M = ES._cameras(intrinsics, w2c)
    d = depth if torch.is_tensor(depth) else torch.from_numpy(np.array(depth, order="C"))   # (a copy: may be read-only)
    if d.dim() != 3:
        raise ValueError(f"point_masks_depth: depth must be float32 [V,H,W] (got {tuple(d.shape)})")
    height, width = ES._check_size("point_masks_depth", d.shape[1], d.shape[2])
    d = _as_depth(d, V, height, width, "point_masks_depth")
    pts = points if torch.is_tensor(points) else torch.from_numpy(np.ascontiguousarray(points, np.float32).reshape(-1, 3))
    if pts.dim() != 2 or pts.shape[1] != 3:
        raise ValueError(f"points must be [P,3] (got {tuple(pts.shape)})")
    pts = pts.detach().to(torch.float32)
    if backend == "host":
        mask = np.zeros((V, height, width), np.uint8)
        kept, hidden = np.zeros((V,), np.int32), np.zeros((V,), np.int32)
        P64 = pts.cpu().numpy().astype(np.float64)
        planes = ES._host(d)
        for i in range(V):
            c2, u, v = _camera_points_host(P64, K[i], M[i])
            with np.errstate(all="ignore"):
                seen = ~(c2 <= 0.0) & (u >= 0.0) & (u < float(width)) & (v >= 0.0) & (v < float(height))
            hid = hidden_host(c2, u, v, seen, planes[i], slack)
            vis = seen & ~hid
            mask[i, np.floor(v[vis]).astype(np.int64), np.floor(u[vis]).astype(np.int64)] = 1
            kept[i], hidden[i] = np.count_nonzero(vis), np.count_nonzero(hid)
        mask = torch.from_numpy(mask)
        return (mask, torch.from_numpy(kept), torch.from_numpy(hidden)) if return_counts else mask
    dev = ES._device_for([pts, d], "point_masks_depth", device)
    with L.device_guard(dev):
        pts, d = pts.to(dev).contiguous(), d.to(dev)
        mask = torch.empty((V, height, width), dtype=torch.uint8, device=dev)
        kept = torch.empty((V,), dtype=torch.int32, device=dev)
        hidden = torch.empty((V,), dtype=torch.int32, device=dev)
        if V > 0:
            Kd, Md = ES.cameras_on(dev, K, M)
            rc = L.load().cgs_point_mask_depth(int(pts.shape[0]), L.ptr(pts), V, L.ptr(Kd), L.ptr(Md), height, width,
                                               L.ptr(d), slack, L.ptr(mask), L.ptr(kept), L.ptr(hidden), L.raw_stream(dev))
            L.check(rc, "cgs_point_mask_depth")
    return (mask, kept, hidden) if return_counts else mask


# ------------------------------------------------------------------------------------------------ the user's depth
def check_depth_maps(cameras, depth_maps):
    """One depth map per camera -- a floating-point [H,W] array of camera z, of its camera's size -- as a list of float32
    arrays in which every entry that is NaN or <= 0 (no measurement) is +inf (no surface: it hides nothing).  ValueError
    for a wrong count, type or size."""
    cameras, maps = list(cameras), list(depth_maps)
    if len(maps) != len(cameras):
        raise ValueError(f"check_depth_maps: {len(cameras)} cameras and {len(maps)} depth maps")
    out = []
    for c, m in zip(cameras, maps):
        m = ES._host(m)
        if m.dtype.kind != "f" or m.shape != (c.height, c.width):
            raise ValueError(f"check_depth_maps: the depth map of {c.name} must be a float [{c.height},{c.width}] array "
                             f"(got {m.dtype} {m.shape})")
        m = m.astype(np.float32)
        with np.errstate(invalid="ignore"):
            m[~(m > 0.0)] = np.inf
        out.append(m)
    return out


# ------------------------------------------------------------------------------------------------ a scan's depth source
def check_one_depth_source(what, occluder, depth_maps):
    if occluder is not None and depth_maps is not None:
        raise ValueError(f"{what}: give an occluder or depth_maps, not both")


class ChunkDepth:
    """The depth source of a scan-level operator (``score_edges``, ``edge_support``, ``trim_edges``, ``snap_edges``), built
    once and asked per chunk of views.  ``occluder``: float32 [F,3,3] triangles or the path of an .obj / .ply mesh, rendered
    into every chunk's planes by ``mesh_depth``; ``depth_maps``: one float [H,W] array of camera z per camera
    (``check_depth_maps``).  At most one of the two; with neither ``gated`` is False and nothing else may be asked.  Either
    way a chunk's planes go through the window maximum of radius ``depth_window``; ``depth_slack`` is what the operators
    then hold a sample's depth against.  Nothing is kept between chunks: ``planes`` builds what one chunk needs.

      gated             whether there is a depth source
      bytes_per_pixel   what a chunk's working set grows by: ``edge_score.DEPTH_BYTES_PER_PIXEL`` (the float32 plane and
                        its window maximum), 0 when not gated
      slack, window     the checked settings
      to(backend, dev)  where the planes are built; uploads the triangles once
      planes(...)       float32 [len(sel),H,W] of a chunk of ``view_chunks``, on the back end's device
      settings()        the keys a result records: "occluder" (the path, or true) or "depth_maps": true, "depth_slack",
                        "depth_window", and "near_clip" only when it was given; {} when not gated

    ``near_clip``: the near plane of ``mesh_depth`` for an occluder the cameras stand INSIDE (None: no clipping, the
    default); rejected without an occluder.

    The occluder may also be a point cloud: a ``Surfels``, or the path of a PLY with vertices and no faces
    (``read_occluder``), rendered by ``surfel_depth``.  ``to`` then uploads its three arrays once; radii that the file does
    not hold are derived once by ``surfel_radii`` on the back end the planes are built on; ``settings()`` also records
    "occluder_kind": "surfels", "surfels" (the count) and, when the radii were derived, "surfel_radius_factor" -- for a
    mesh the keys are what they were.  ``near_clip`` with a cloud is a ValueError: a disk is dropped, not cut."""

    def __init__(self, what, cameras, occluder=None, depth_maps=None, depth_slack=DEPTH_SLACK, depth_window=DEPTH_WINDOW,
                 near_clip=None):
        check_one_depth_source(what, occluder, depth_maps)
        if near_clip is not None and occluder is None:
            raise ValueError(f"{what}: near_clip needs an occluder (the caller's depth maps need no clipping)")
        self.near = _check_near(what, near_clip)
        self.what = what
        self.gated = occluder is not None or depth_maps is not None
        self.bytes_per_pixel = ES.DEPTH_BYTES_PER_PIXEL if self.gated else 0
        self.slack, self.window = depth_slack, depth_window
        self.occluder, self.tris, self.maps = occluder, None, None
        self.surfels, self.radius_factor = None, None   # a point-cloud occluder: (points, normals or None, radii) tensors
        self.backend, self.device = "host", None
        if self.gated:
            self.slack = _check_slack(what, depth_slack)
            self.window = _check_window(what, depth_window)
        if occluder is not None:
            geometry = occluder
            if isinstance(occluder, (str, os.PathLike)):
                geometry = read_occluder(occluder, derive_radii=False)   # (radii the file lacks: on the back end of to())
            if isinstance(geometry, Surfels):
                if self.near is not None:
                    raise ValueError(f"{what}: near_clip takes a mesh (a disk that reaches the camera plane is dropped, not cut)")
                if geometry.radii is None:
                    self.radius_factor = SURFEL_RADIUS_FACTOR
                    geometry = geometry._replace(radii=np.zeros((len(geometry.points),), np.float32))
                self.surfels = _as_surfels(geometry)
                self._radii_ready = self.radius_factor is None
            else:
                self.tris = _as_tris(geometry)
        if depth_maps is not None:
            self.maps = check_depth_maps(cameras, depth_maps)

    def to(self, backend, device=None):
        self.backend, self.device = backend, device
        if self.tris is not None and backend == "gpu":
            self.tris = self.tris.to(device)
        if self.surfels is not None and backend == "gpu":
            self.surfels = tuple(None if t is None else t.to(device) for t in self.surfels)
        return self

    def planes(self, H, W, sel, intr, w2c):
        if self.tris is not None:
            return mesh_depth(self.tris, intr, w2c, H, W, self.window, backend=self.backend, device=self.device,
                              near_clip=self.near)
        if self.surfels is not None:
            if not self._radii_ready:   # a cloud file without radii: derived once, on the back end the planes are built on
                pts, nrm, _ = self.surfels
                rad = torch.from_numpy(surfel_radii(pts, self.radius_factor, backend=self.backend, device=self.device))
                self.surfels, self._radii_ready = (pts, nrm, rad.to(pts.device)), True
            return surfel_depth(Surfels(*self.surfels), intr, w2c, H, W, self.window, backend=self.backend, device=self.device)
        return depth_window_max(np.stack([self.maps[v] for v in sel]), self.window, backend=self.backend, device=self.device)

    def settings(self):
        if not self.gated:
            return {}
        if self.occluder is not None:
            out = {"occluder": os.fspath(self.occluder) if isinstance(self.occluder, (str, os.PathLike)) else True}
        else:
            out = {"depth_maps": True}
        out.update({"depth_slack": self.slack, "depth_window": self.window})
        if self.near is not None:
            out["near_clip"] = self.near
        if self.surfels is not None:
            out.update({"occluder_kind": "surfels", "surfels": int(self.surfels[0].shape[0])})
            if self.radius_factor is not None:
                out["surfel_radius_factor"] = self.radius_factor
        return out


# ------------------------------------------------------------------------------------------------ mesh files
def _fan(faces):
    """Index lists of polygons -> int64 [F,3]: polygon (a, b, c, d, ...) as the fan (a, b, c), (a, c, d), ..."""
    tris = [(f[0], f[k], f[k + 1]) for f in faces for k in range(1, len(f) - 1)]
    return np.asarray(tris, np.int64).reshape(-1, 3)


def _gather(path, xyz, tri_idx):
    xyz = np.asarray(xyz, np.float64).reshape(-1, 3)
    if tri_idx.size and (tri_idx.min() < 0 or tri_idx.max() >= xyz.shape[0]):
        raise ValueError(f"{path}: a face refers to vertex {int(tri_idx.max() if tri_idx.max() >= xyz.shape[0] else tri_idx.min())}"
                         f" of {xyz.shape[0]}")
    return np.ascontiguousarray(xyz[tri_idx].astype(np.float32)).reshape(-1, 3, 3)


def _read_obj(path):
    xyz, faces = [], []
    with open(path, "r") as f:
        for n, ln in enumerate(f, 1):
            tok = ln.split("#", 1)[0].split()
            if not tok:
                continue
            try:
                if tok[0] == "v":
                    if len(tok) < 4:
                        raise ValueError("a vertex needs x y z")
                    xyz.append([float(t) for t in tok[1:4]])
                elif tok[0] == "f":
                    if len(tok) < 4:
                        raise ValueError("a face needs at least three vertices")
                    idx = [int(t.split("/")[0]) for t in tok[1:]]   # a, a/b, a/b/c, a//c
                    if any(i == 0 for i in idx):
                        raise ValueError("vertex index 0")
                    # a negative index counts back from the vertices read so far
                    faces.append([i - 1 if i > 0 else len(xyz) + i for i in idx])
            except ValueError as e:
                raise ValueError(f"{path}:{n}: {e}") from None
    return _gather(path, xyz, _fan(faces))


def _read_ply(path):
    from ..scene.dataset_io import _PLY_TYPES
    with open(path, "rb") as f:
        blob = f.read()
    if b"end_header" not in blob:
        raise ValueError(f"{path}: not a PLY file (no end_header)")
    head, body = blob.split(b"end_header", 1)
    body = body[body.index(b"\n") + 1:] if b"\n" in body else b""
    lines = head.decode("ascii", "replace").splitlines()
    if not lines or lines[0].strip() != "ply":
        raise ValueError(f"{path}: not a PLY file")
    fmt, elements = None, []   # (name, count, [(property, type, list count type or None)])
    for ln in lines[1:]:
        tok = ln.split()
        if not tok:
            continue
        try:
            if tok[0] == "format":
                fmt = tok[1]
            elif tok[0] == "element":
                elements.append((tok[1], int(tok[2]), []))
            elif tok[0] == "property":
                if tok[1] == "list":
                    elements[-1][2].append((tok[4], _PLY_TYPES[tok[3]], _PLY_TYPES[tok[2]]))
                else:
                    elements[-1][2].append((tok[2], _PLY_TYPES[tok[1]], None))
        except (IndexError, KeyError, ValueError):
            raise ValueError(f"{path}: bad header line {ln!r}") from None
    if fmt not in ("ascii", "binary_little_endian"):
        raise ValueError(f"{path}: unsupported PLY format {fmt} (ascii and binary_little_endian are read)")
    xyz, faces = None, None
    text = body.decode("ascii", "replace").split() if fmt == "ascii" else None
    at = 0   # token index (ascii) or byte offset (binary)
    try:
        for name, count, props in elements:
            rows = []
            scalar_only = all(lt is None for _, _, lt in props)
            if fmt != "ascii" and scalar_only:   # a table: one frombuffer
                dt = np.dtype([(p, "<" + t) for p, t, _ in props])
                tab = np.frombuffer(body, dtype=dt, count=count, offset=at)
                at += dt.itemsize * count
                rows = {p: tab[p] for p, _, _ in props}
            else:
                cols = {p: [] for p, _, _ in props}
                for _ in range(count):
                    for p, t, lt in props:
                        if fmt == "ascii":
                            if lt is None:
                                cols[p].append(float(text[at]))
                                at += 1
                            else:
                                n = int(text[at])
                                cols[p].append([int(x) for x in text[at + 1:at + 1 + n]])
                                if len(cols[p][-1]) != n:
                                    raise IndexError
                                at += 1 + n
                        elif lt is None:
                            cols[p].append(np.frombuffer(body, "<" + t, 1, at)[0])
                            at += np.dtype(t).itemsize
                        else:
                            n = int(np.frombuffer(body, "<" + lt, 1, at)[0])
                            at += np.dtype(lt).itemsize
                            cols[p].append(np.frombuffer(body, "<" + t, n, at).astype(np.int64).tolist())
                            at += n * np.dtype(t).itemsize
                rows = cols
            if name == "vertex":
                if not all(k in rows for k in "xyz"):
                    raise ValueError(f"{path}: the vertex element has no x, y, z")
                for k in "xyz":
                    if dict((p, t) for p, t, _ in props)[k] not in ("f4", "f8"):
                        raise ValueError(f"{path}: x, y, z must be float or double")
                xyz = np.stack([np.asarray(rows[k], np.float64) for k in "xyz"], 1)
            elif name == "face":
                key = next((k for k in ("vertex_indices", "vertex_index") if k in rows), None)
                lt = {p: (t, l) for p, t, l in props}.get(key)
                if key is None or lt[1] is None or lt[0][0] not in "iu":
                    raise ValueError(f"{path}: the face element has no integer list vertex_indices / vertex_index")
                faces = rows[key]
    except (IndexError, ValueError) as e:
        if isinstance(e, ValueError) and str(e).startswith(str(path)):
            raise
        raise ValueError(f"{path}: the body is shorter than the header says") from None
    if xyz is None or faces is None:
        raise ValueError(f"{path}: needs a vertex and a face element")
    if any(len(f) < 3 for f in faces):
        raise ValueError(f"{path}: a face needs at least three vertices")
    return _gather(path, xyz, _fan(faces))


def read_triangle_mesh(path):
    """float32 [F,3,3] of a mesh file.  ``.obj``: ``v`` and ``f`` records (``a``, ``a/b``, ``a/b/c``, ``a//c``; negative
    indices count back from the last vertex read); ``.ply``: ascii or binary_little_endian, float or double ``x y z``, a
    face list property ``vertex_indices`` or ``vertex_index`` of any integer types.  Polygons are fan-triangulated.
    Anything else is a ValueError."""
    ext = os.path.splitext(str(path))[1].lower()
    if ext == ".obj":
        return _read_obj(path)
    if ext == ".ply":
        return _read_ply(path)
    raise ValueError(f"{path}: unknown mesh format {ext!r} (.obj and .ply are read)")


def _ply_element_counts(path):
    """{element name: count} of a PLY file's header."""
    counts = {}
    with open(path, "rb") as f:
        if f.readline().strip() != b"ply":
            raise ValueError(f"{path}: not a PLY file")
        for raw in f:
            tok = raw.decode("ascii", "replace").split()
            if tok[:1] == ["end_header"]:
                return counts
            if tok[:1] == ["element"]:
                try:
                    counts[tok[1]] = int(tok[2])
                except (IndexError, ValueError):
                    raise ValueError(f"{path}: bad header line {raw!r}") from None
    raise ValueError(f"{path}: not a PLY file (no end_header)")


def read_occluder(path, factor=SURFEL_RADIUS_FACTOR, backend="host", device=None, derive_radii=True):
    """An occluder file as what ``ChunkDepth`` takes: float32 [F,3,3] triangles of an ``.obj`` or of a ``.ply`` that has
    faces (``read_triangle_mesh``), or the ``Surfels`` of a ``.ply`` with a vertex element and no face (none, or ``element
    face 0``) -- a point cloud such as COLMAP's fused.ply: positions from ``x y z``, normals from ``nx ny nz`` when all three
    are there (else None), radii from a scalar ``radius`` property when there is one, else ``surfel_radii(points, factor,
    backend, device)`` -- or None with ``derive_radii=False``, for a caller that derives them later."""
    ext = os.path.splitext(str(path))[1].lower()
    if ext != ".ply":
        return read_triangle_mesh(path)
    counts = _ply_element_counts(path)
    if "vertex" not in counts or counts.get("face", 0) > 0:
        return read_triangle_mesh(path)
    from ..scene.dataset_io import read_ply_table
    tab = read_ply_table(path)
    if not all(k in tab and tab[k].dtype.kind == "f" for k in "xyz"):
        raise ValueError(f"{path}: the vertex element needs float or double x, y, z")
    column = lambda names: np.ascontiguousarray(np.stack([np.asarray(tab[k], np.float32) for k in names], 1))
    pts = column("xyz")
    nrm = column(("nx", "ny", "nz")) if all(k in tab for k in ("nx", "ny", "nz")) else None
    if "radius" in tab:
        rad = np.ascontiguousarray(tab["radius"], np.float32)
    else:
        rad = surfel_radii(pts, factor, backend=backend, device=device) if derive_radii else None
    return Surfels(pts, nrm, rad)


def write_surfel_ply(path, surfels):
    """A ``Surfels`` as a binary little-endian PLY of P float vertices -- ``x y z``, ``nx ny nz`` when there are normals,
    ``radius`` -- and no face element; ``read_occluder`` returns the same float32 bits."""
    pts, nrm, rad = _as_surfels(surfels)
    cols = [pts.cpu().numpy()] + ([] if nrm is None else [nrm.cpu().numpy()]) + [rad.cpu().numpy()[:, None]]
    names = ["x", "y", "z"] + ([] if nrm is None else ["nx", "ny", "nz"]) + ["radius"]
    head = (f"ply\nformat binary_little_endian 1.0\nelement vertex {pts.shape[0]}\n"
            + "".join(f"property float {n}\n" for n in names) + "end_header\n")
    with open(path, "wb") as f:
        f.write(head.encode("ascii"))
        f.write(np.ascontiguousarray(np.concatenate(cols, 1), "<f4").tobytes())


def write_triangle_ply(path, tris):
    """tris [F,3,3] as a binary little-endian PLY of 3 F float vertices and F ``vertex_indices`` faces (no vertex is
    shared); ``read_triangle_mesh`` returns the same float32 triangles."""
    t = np.ascontiguousarray(ES._host(tris), "<f4").reshape(-1, 3, 3)
    F = t.shape[0]
    head = (f"ply\nformat binary_little_endian 1.0\nelement vertex {3 * F}\nproperty float x\nproperty float y\n"
            f"property float z\nelement face {F}\nproperty list uchar int vertex_indices\nend_header\n")
    faces = np.zeros(F, np.dtype([("n", "u1"), ("i", "<i4", (3,))]))
    faces["n"] = 3
    faces["i"] = np.arange(3 * F, dtype=np.int32).reshape(F, 3)
    with open(path, "wb") as f:
        f.write(head.encode("ascii"))
        f.write(t.tobytes())
        f.write(faces.tobytes())
