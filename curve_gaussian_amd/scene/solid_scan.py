"""Solid synthetic scans with ground truth: a closed triangle mesh, its feature edges as a ``parametric_edges.json`` dict,
cameras around it and edge maps with the HIDDEN LINES REMOVED -- the first scans of this project in which occlusion exists
(every drawn scan of tests/*_cases.py is a wireframe with nothing to hide behind).

The maps are drawn by the operators that the score uses: the ground-truth edges sampled as the score samples them
(``abc.pred_points_and_directions`` at ``reprojection.SAMPLE_RESOLUTION``), gated by ``ops.edge_occlusion.point_masks_depth``
against ``mesh_depth`` of the solid with the defaults of the score.  Scoring the ground truth with the solid as the
occluder therefore reproduces the maps exactly, and scoring it without shows what the missing depth costs.  The cameras
are ``synthetic.fibonacci_cameras`` as a scan in the EMAP layout stores and reads them back (camtoworld = inv(w2c) in the
file, w2c = inv(camtoworld) on reading), so a scan written by ``write_solid_scan`` scores the same from disk.

Shapes (inside the unit cube, around its centre):
  box         12 lines
  l_bracket   an L-shaped prism: concave, 18 lines, one solid hiding part of itself
  cylinder    a 64-gon side with two caps; the ground truth is its two rims, four cubic quarter arcs each with the usual
              handle 0.5523 r.  Such an arc leaves the circle by at most 2.7e-4 r, below the sampling resolution; the
              64-gon's sides lie up to 1.2e-3 r inside the circle, so a rim sample is never behind its own cap.

One shape is seen from INSIDE (``INDOOR_SHAPES``; it is not among ``SHAPES``, whose scans stay byte for byte what they were):
  room        an inward box of 12 large triangles (walls, floor, ceiling) with one free-standing box pillar on its floor,
              12 triangles; the ground truth is the 12 lines of the room and the 12 of the pillar.  The cameras are
              ``synthetic.make_camera`` s on a ring inside the room, each looking across it at the far side of the ring --
              every eye at least 0.1 from every surface.  Every wall reaches behind the camera plane of most views, so the
              planes are drawn with near-plane clipping (``near_clip = EO.NEAR_CLIP``, ``cgs_mesh_depth_clipped``); without
              it most of the room's triangles are dropped and the gate sees through the walls.

``surfel_cloud`` samples a solid's surface as an oriented point cloud, and ``write_solid_scan(..., cloud=SPACING)`` writes it
as ``cloud.ply`` beside ``mesh.ply``: the occluder of a scan that has no mesh (``ops.edge_occlusion.read_occluder``).

``photographs`` shades every view from the depth planes with a fixed 3D value-noise texture, and
``write_solid_scan(..., photos=True)`` writes them as ``color/<rgb_path>``: the input of a scan that has photographs and
poses only (``edge_detect``, ``stereo_depth``).

LIMITS.  By default the maps hold feature edges only (the cylinder's side draws nothing).  With ``contours=True`` they also
hold the occluding contours of the curved surfaces -- the smooth mesh edges along which a view sees the surface turn away
(``ops.mesh_contours.contour_masks``, gated by the same planes and slack) -- as a detector would: edges of the image that
no 3D edge explains.  They are the contours of the MESH (the 64-gon's side edges), one pixel wide.  No detector noise, no
line width beyond the pixel a sample falls into.  Along a concave edge (the bracket's inner corner) the
gate can hide samples of a visible edge behind their own faces (ops/edge_occlusion.py says why); the maps then miss them,
consistently with the score."""
import json
import math
import os
from typing import NamedTuple

import numpy as np
import torch

from .. import synthetic
from ..ops import edge_occlusion as EO
from ..ops import mesh_contours as MC
from ..ops.view_chunks import camera_arrays
from .dataset_io import fov2focal

SHAPES = ("box", "l_bracket", "cylinder")
INDOOR_SHAPES = ("room",)    # seen from inside: their own cameras, planes drawn with near-plane clipping
ROOM_BOX = ((0.05, 0.05), (0.95, 0.95), 0.25, 0.75)       # (x0, y0), (x1, y1), floor, ceiling
ROOM_PILLAR = ((0.50, 0.40), (0.62, 0.52), 0.25, 0.60)    # stands on the floor, ends below the ceiling
ROOM_RING = (0.5, 0.5, 0.5, 0.3)                          # the eyes: centre x, y, height, radius
ROOM_LOOK_DOWN = 0.08                                     # the target lies this far below the eyes' height
CYLINDER_SIDES = 64
ARC_HANDLE = 0.5523
CLOUD_SPACING = 0.01         # the --cloud flag's spacing: the density the surfel gate is checked at (profiles/surfel_depth.md)
CLOUD_MIN_GAP = 0.75         # surfel_cloud: no two samples nearer than this many spacings
PHOTO_BACKGROUND = 128       # photographs: the grey value where a view sees no surface
PHOTO_OCTAVES = ((12, 4.0), (29, 2.0), (67, 1.0))   # photographs: (lattice cells per world unit, weight) of the value noise
SAMPLE_RESOLUTION = 0.0005   # edge_extraction.reprojection.SAMPLE_RESOLUTION (that module imports the ops; not imported here)


class SolidScan(NamedTuple):
    tris: np.ndarray        # float32 [F,3,3]
    edges: dict             # the ground truth: {"lines_end_pts": [[6]], "curves_ctl_pts": [[12]]}
    synth_cameras: list     # synthetic.SynthCamera s, what dataset_io.write_emap takes
    cameras: list           # NovelViewCamera s, what score_edges takes
    maps: np.ndarray        # uint8 [V,H,W], 255 on an edge: PidiNet bytes
    depth: np.ndarray       # float32 [V,H,W], the plain z-buffer (+inf: no surface)
    hidden: np.ndarray      # int32 [V]: the ground-truth samples each view hides
    contours: np.ndarray = None   # uint8 [V,H,W], 1 on a drawn contour (already OR-ed into maps); None without contours=True


def _prism(poly, z0, z1):
    """A polygon [(x, y)] that is star-shaped from its first vertex, extruded from z0 to z1: (triangles, lines).  The caps
    are fans over the polygon's own vertices, so no side of a triangle ends inside another's (no T-junction)."""
    n = len(poly)
    lo = [(x, y, z0) for x, y in poly]
    hi = [(x, y, z1) for x, y in poly]
    tris, lines = [], []
    for k in range(1, n - 1):
        tris += [(lo[0], lo[k + 1], lo[k]), (hi[0], hi[k], hi[k + 1])]
    for k in range(n):
        j = (k + 1) % n
        tris += [(lo[k], lo[j], hi[j]), (lo[k], hi[j], hi[k])]
        lines += [lo[k] + lo[j], hi[k] + hi[j], lo[k] + hi[k]]
    return tris, lines


def _ring(cx, cy, r, z):
    """The circle of radius r around (cx, cy) at height z as four cubic quarter arcs, 12 numbers each."""
    h = ARC_HANDLE * r
    out = []
    for q in range(4):
        a, b = q * math.pi / 2.0, (q + 1) * math.pi / 2.0
        p0 = (cx + r * math.cos(a), cy + r * math.sin(a))
        p3 = (cx + r * math.cos(b), cy + r * math.sin(b))
        p1 = (p0[0] - h * math.sin(a), p0[1] + h * math.cos(a))
        p2 = (p3[0] + h * math.sin(b), p3[1] - h * math.cos(b))
        out.append([c for p in (p0, p1, p2, p3) for c in (p[0], p[1], z)])
    return out


def solid_geometry(shape):
    """(tris float32 [F,3,3], edge dict) of a shape."""
    curves = []
    if shape == "box":
        tris, lines = _prism([(0.2, 0.25), (0.8, 0.25), (0.8, 0.75), (0.2, 0.75)], 0.3, 0.7)
    elif shape == "l_bracket":
        tris, lines = _prism([(0.2, 0.2), (0.8, 0.2), (0.8, 0.45), (0.45, 0.45), (0.45, 0.8), (0.2, 0.8)], 0.3, 0.7)
    elif shape == "cylinder":
        r, n = 0.3, CYLINDER_SIDES
        poly = [(0.5 + r * math.cos(2.0 * math.pi * k / n), 0.5 + r * math.sin(2.0 * math.pi * k / n)) for k in range(n)]
        tris, lines = _prism(poly, 0.25, 0.75)
        lines, curves = [], _ring(0.5, 0.5, r, 0.25) + _ring(0.5, 0.5, r, 0.75)
    elif shape == "room":
        tris, lines = [], []
        for k, ((x0, y0), (x1, y1), z0, z1) in enumerate((ROOM_BOX, ROOM_PILLAR)):
            t, ln = _prism([(x0, y0), (x1, y0), (x1, y1), (x0, y1)], z0, z1)
            tris += [tri[::-1] for tri in t] if k == 0 else t   # the room faces inward
            lines += ln
    else:
        raise ValueError(f"unknown solid {shape!r}: expected one of {SHAPES + INDOOR_SHAPES}")
    return (np.asarray(tris, np.float32).reshape(-1, 3, 3),
            {"lines_end_pts": [list(map(float, ln)) for ln in lines], "curves_ctl_pts": curves})


def emap_cameras_of(synth_cams):
    """NovelViewCamera s of synthetic cameras, formed as ``write_emap`` stores and ``reprojection.emap_cameras`` reads them."""
    from ..edge_extraction.novel_view import NovelViewCamera
    out = []
    for i, c in enumerate(synth_cams):
        H, W = int(c.image_height), int(c.image_width)
        stored = np.linalg.inv(c.world_view_transform.detach().cpu().double().numpy().T)   # camtoworld, as written
        w2c = np.linalg.inv(np.asarray(stored, np.float64))
        out.append(NovelViewCamera(f"{i}_colors.png", np.ascontiguousarray(w2c[:3, :3]), w2c[:3, 3].copy(),
                                   float(fov2focal(c.FoVx, W)), float(fov2focal(c.FoVy, H)), W / 2.0, H / 2.0, W, H))
    return out


def room_cameras(n_views, H, W):
    """``n_views`` ``synthetic.make_camera`` s on the ring ``ROOM_RING`` inside the room, each looking at the opposite point
    of the ring, ``ROOM_LOOK_DOWN`` lower; z is up."""
    cx, cy, cz, r = ROOM_RING
    cams = []
    for k in range(int(n_views)):
        a = 2.0 * math.pi * k / max(int(n_views), 1)
        eye = (cx + r * math.cos(a), cy + r * math.sin(a), cz)
        target = (cx - r * math.cos(a), cy - r * math.sin(a), cz - ROOM_LOOK_DOWN)
        cams.append(synthetic.make_camera(eye, target, (0.0, 0.0, 1.0), int(H), int(W)))
    return cams


def solid_scan(shape, n_views, H, W, backend="gpu", device=None, slack=EO.DEPTH_SLACK, window=EO.DEPTH_WINDOW,
               sample_resolution=SAMPLE_RESOLUTION, contours=False, crease_deg=MC.CREASE_DEG, near_clip=None, clip=True,
               synth_cameras=None):
    """A ``SolidScan`` of ``shape`` seen from ``n_views`` ``synthetic.fibonacci_cameras`` of H x W pixels; ``backend`` as the
    ops (both give the same bytes).  ``contours``: the smooth contours of the mesh (folds up to ``crease_deg``, UNTUNED) are
    OR-ed into the maps as 255, gated by the planes and the slack that gate the feature edges, and kept in ``.contours``;
    without it every byte is what it was.  ``near_clip``: the near plane of the planes and contours, as
    ``mesh_depth`` takes it (None: no clipping for ``SHAPES``, whose cameras stand outside; ``EO.NEAR_CLIP`` for
    ``INDOOR_SHAPES``, whose cameras stand inside).  ``clip=False`` draws an indoor scan WITHOUT clipping, to see what that
    costs; it is an error with a ``near_clip``.  ``synth_cameras``: ``synthetic.make_camera`` s of H x W pixels to use instead
    (``n_views`` is then ignored): neighbouring views a few degrees apart, which the default cameras are not."""
    from ..edge_extraction.abc import pred_points_and_directions
    tris, edges = solid_geometry(shape)
    if synth_cameras is not None:
        synth = list(synth_cameras)
        if shape in INDOOR_SHAPES and clip and near_clip is None:
            near_clip = EO.NEAR_CLIP
    elif shape in INDOOR_SHAPES:
        synth = room_cameras(n_views, H, W)
        if not clip and near_clip is not None:
            raise ValueError("solid_scan: clip=False takes no near_clip")
        if clip and near_clip is None:
            near_clip = EO.NEAR_CLIP
    else:
        synth = synthetic.fibonacci_cameras(int(n_views), int(H), int(W))
    cams = emap_cameras_of(synth)
    intr, w2c = camera_arrays(cams)
    pts = np.ascontiguousarray(pred_points_and_directions(edges, sample_resolution).points, np.float32).reshape(-1, 3)
    raw = EO.mesh_depth(tris, intr, w2c, H, W, window=0, backend=backend, device=device, near_clip=near_clip)
    planes = EO.depth_window_max(raw, window, backend=backend, device=device)
    mask, _, hidden = EO.point_masks_depth(pts, intr, w2c, planes, slack, backend=backend, device=device, return_counts=True)
    maps, drawn = mask.cpu().numpy() * np.uint8(255), None
    if contours:
        drawn = MC.contour_masks(tris, intr, w2c, H, W, planes, slack, "smooth", crease_deg, backend=backend,
                                 device=device, near_clip=near_clip).cpu().numpy()
        maps |= drawn * np.uint8(255)
    return SolidScan(tris, edges, synth, cams, maps, raw.cpu().numpy(), hidden.cpu().numpy(), drawn)


def surfel_cloud(tris, spacing):
    """A mesh's surface as an oriented point cloud, what a dense reconstruction would give: (points float32 [P,3], normals
    float32 [P,3]).  Deterministic, no randomness, in two steps.  CANDIDATES: a grid in barycentric coordinates per
    triangle -- with a the vertex between the longest side ab and the shortest side ac, the points a + u (b - a) + v (c - a) for
    u = (i + 0.5) / n1, v = (j + 0.5) / n2, u + v < 1, n1 and n2 the sides' lengths over a third of the spacing, rounded up --
    each with the face's unit normal (b - a) x (c - a); none lies on a side.  THINNING: the candidates are taken in their
    order (triangle by triangle, row by row) and one is kept unless a kept one lies nearer than ``CLOUD_MIN_GAP * spacing``.
    A grid alone is as skewed as its triangle: on the thin triangles of a cylinder's caps and sides it leaves lines of
    points many times as dense along one direction as along the other, and disks sized by the nearest neighbours
    (``EO.surfel_radii``) then leave gaps between the lines.  After the thinning no two samples are nearer than that
    distance and no point of the surface is farther than it, plus a candidate cell, from a sample, whatever the
    triangulation.  A triangle without area gives nothing."""
    T = np.asarray(tris, np.float64).reshape(-1, 3, 3)
    spacing = float(spacing)
    if not (spacing > 0.0 and math.isfinite(spacing)):
        raise ValueError(f"surfel_cloud: the spacing must be finite and > 0 (got {spacing})")
    pts, nrm = [], []
    for tri in T:
        normal = np.cross(tri[1] - tri[0], tri[2] - tri[0])
        length = float(np.linalg.norm(normal))
        if not length > 0.0:
            continue
        sides = [float(np.linalg.norm(tri[(s + 1) % 3] - tri[s])) for s in range(3)]   # side s: vertex s -> vertex s + 1
        lo, hi = int(np.argmin(sides)), int(np.argmax(sides))
        if lo == hi:
            lo = (hi + 2) % 3
        # a: the vertex the longest and the shortest side share, so that the grid's cells are about as long as wide
        a = tri[hi] if (hi + 2) % 3 == lo else tri[(hi + 1) % 3]
        b = tri[(hi + 1) % 3] if (hi + 2) % 3 == lo else tri[hi]
        c = tri[lo] if (hi + 2) % 3 == lo else tri[(lo + 1) % 3]
        n1 = max(1, int(math.ceil(3.0 * np.linalg.norm(b - a) / spacing)))
        n2 = max(1, int(math.ceil(3.0 * np.linalg.norm(c - a) / spacing)))
        u, v = np.meshgrid((np.arange(n1) + 0.5) / n1, (np.arange(n2) + 0.5) / n2, indexing="ij")
        inside = (u + v) < 1.0
        pts.append(a + u[inside][:, None] * (b - a) + v[inside][:, None] * (c - a))
        nrm.append(np.broadcast_to(normal / length, (pts[-1].shape[0], 3)))
    if not pts:
        return np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32)
    pts, nrm = np.concatenate(pts), np.concatenate(nrm)
    gap = CLOUD_MIN_GAP * spacing
    cell = np.floor(pts / gap).astype(np.int64)
    kept, grid = [], {}
    around = [(i, j, k) for i in (-1, 0, 1) for j in (-1, 0, 1) for k in (-1, 0, 1)]
    rows, cells, gap2 = pts.tolist(), cell.tolist(), gap * gap
    for n, ((x, y, z), (ci, cj, ck)) in enumerate(zip(rows, cells)):
        for di, dj, dk in around:
            for (qx, qy, qz) in grid.get((ci + di, cj + dj, ck + dk), ()):
                if (x - qx) * (x - qx) + (y - qy) * (y - qy) + (z - qz) * (z - qz) < gap2:
                    break
            else:
                continue
            break
        else:
            grid.setdefault((ci, cj, ck), []).append((x, y, z))
            kept.append(n)
    return np.ascontiguousarray(pts[kept], np.float32), np.ascontiguousarray(nrm[kept], np.float32)


def arc_cameras(n_views, H, W, step_deg=8.0, radius=1.8, elevation_deg=25.0, centre=(0.5, 0.5, 0.5)):
    """``n_views`` ``synthetic.make_camera`` s on an arc around ``centre``, ``step_deg`` apart in azimuth at one elevation, all
    looking at the centre; z is up.  Neighbours a few degrees apart: what stereo needs and ``fibonacci_cameras`` do not give."""
    c, el = np.asarray(centre, np.float64), math.radians(float(elevation_deg))
    cams = []
    for k in range(int(n_views)):
        az = math.radians(float(step_deg)) * (k - 0.5 * (int(n_views) - 1)) + math.radians(30.0)
        eye = c + float(radius) * np.array([math.cos(el) * math.cos(az), math.cos(el) * math.sin(az), math.sin(el)])
        cams.append(synthetic.make_camera(eye, c, (0.0, 0.0, 1.0), int(H), int(W)))
    return cams


def value_noise(points):
    """A fixed 3D value-noise texture at float64 world points [...,3], in [0, 1]: per octave of ``PHOTO_OCTAVES`` an integer
    lattice whose nodes carry a hashed value, interpolated trilinearly; the octaves' weighted mean.  Not periodic within
    any scene, which sines are: a periodic texture gives plane-sweep stereo false matches."""
    P = np.asarray(points, np.float64)
    total, weight = np.zeros(P.shape[:-1]), 0.0
    for cells, wgt in PHOTO_OCTAVES:
        q = P * float(cells)
        q0 = np.floor(q)
        t = q - q0
        q0 = q0.astype(np.int64)
        acc = np.zeros(P.shape[:-1])
        for dx in (0, 1):
            for dy in (0, 1):
                for dz in (0, 1):
                    h = ((q0[..., 0] + dx) * 73856093) ^ ((q0[..., 1] + dy) * 19349663) ^ ((q0[..., 2] + dz) * 83492791)
                    h = (h ^ (cells * 2654435761)) & 0xFFFFFFFF
                    h = ((h ^ (h >> 16)) * 0x45D9F3B) & 0xFFFFFFFF
                    h = ((h ^ (h >> 16)) * 0x45D9F3B) & 0xFFFFFFFF
                    h = h ^ (h >> 16)
                    wx = t[..., 0] if dx else 1.0 - t[..., 0]
                    wy = t[..., 1] if dy else 1.0 - t[..., 1]
                    wz = t[..., 2] if dz else 1.0 - t[..., 2]
                    acc += (h & 0xFFFF).astype(np.float64) / 65535.0 * wx * wy * wz
        total += wgt * acc
        weight += wgt
    return total / weight


def photographs(scan):
    """uint8 [V,H,W]: what a camera would photograph of the textured solid.  A pixel whose depth plane holds a surface is
    un-projected at its centre to its world point and takes round(255 * ``value_noise``) there; every other pixel is
    ``PHOTO_BACKGROUND``.  No lighting: a surface point has the same grey value in every view.  Host numpy."""
    depth = np.asarray(scan.depth, np.float32)
    V, H, W = depth.shape
    out = np.full((V, H, W), PHOTO_BACKGROUND, np.uint8)
    for v, c in enumerate(scan.cameras):
        z = depth[v].astype(np.float64)
        hit = np.isfinite(z) & (z > 0.0)
        i, j = np.nonzero(hit)
        zc = z[i, j]
        cam = np.stack([((j + 0.5) - c.cx) / c.fx * zc, ((i + 0.5) - c.cy) / c.fy * zc, zc], 1)
        world = (cam - np.asarray(c.T, np.float64)) @ np.asarray(c.R, np.float64)   # R^T (c - T), row vectors
        out[v, i, j] = np.rint(255.0 * np.clip(value_noise(world), 0.0, 1.0)).astype(np.uint8)
    return out


def write_solid_scan(path, scan, depth=False, cloud=None, photos=False):
    """The scan in the EMAP layout (``dataset_io.write_emap``, PidiNet maps) plus ``mesh.ply``, ``gt_edges.json`` and, with
    ``depth``, ``depth/<image stem>.npy`` (the plain z-buffer, float32 camera z, +inf where there is no surface).  ``cloud``:
    a spacing in world units; ``cloud.ply`` is then written beside ``mesh.ply`` -- ``surfel_cloud`` of the mesh at that
    spacing, with normals and the radii ``EO.surfel_radii`` derives (host back end) --, the occluder a scan without a mesh
    has.  None (the default) writes no such file, and every other file is the same either way.  ``photos``: also
    ``color/<rgb_path>``, the view's ``photographs`` as an 8-bit grey PNG; without it no such folder is written and every
    other file is the same either way."""
    from .dataset_io import write_emap
    write_emap(path, scan.synth_cameras, [torch.from_numpy(m.astype(np.float32) / 255.0) for m in scan.maps], detector="PidiNet")
    EO.write_triangle_ply(os.path.join(path, "mesh.ply"), scan.tris)
    if cloud is not None:
        pts, nrm = surfel_cloud(scan.tris, cloud)
        EO.write_surfel_ply(os.path.join(path, "cloud.ply"), EO.Surfels(pts, nrm, EO.surfel_radii(pts, backend="host")))
    with open(os.path.join(path, "gt_edges.json"), "w") as f:
        json.dump(scan.edges, f)
    if photos:
        from PIL import Image
        os.makedirs(os.path.join(path, "color"), exist_ok=True)
        for c, p in zip(scan.cameras, photographs(scan)):
            Image.fromarray(p, mode="L").save(os.path.join(path, "color", c.name))
    if depth:
        os.makedirs(os.path.join(path, "depth"), exist_ok=True)
        for c, d in zip(scan.cameras, scan.depth):
            np.save(os.path.join(path, "depth", os.path.splitext(c.name)[0] + ".npy"), d)


def main(argv=None):
    import argparse
    ap = argparse.ArgumentParser(prog="python -m curve_gaussian_amd.solid_scan",
                                 description="Write a solid synthetic scan with ground truth and hidden lines removed.")
    ap.add_argument("shape", choices=SHAPES + INDOOR_SHAPES)
    ap.add_argument("out_dir", help="the scan directory to write (EMAP layout)")
    ap.add_argument("--views", type=int, default=24)
    ap.add_argument("--height", type=int, default=240)
    ap.add_argument("--width", type=int, default=320)
    ap.add_argument("--depth", action="store_true", help="also write depth/<image stem>.npy")
    ap.add_argument("--contours", action="store_true",
                    help="also draw the occluding contours of the curved surfaces into the maps (no 3D edge explains them)")
    ap.add_argument("--cloud", nargs="?", type=float, const=CLOUD_SPACING, default=None, metavar="SPACING",
                    help="also write cloud.ply, the solid's surface sampled as an oriented point cloud with radii: the "
                         f"occluder of a scan that has no mesh (bare flag: a spacing of {CLOUD_SPACING}, world units)")
    ap.add_argument("--photos", action="store_true",
                    help="also write color/<rgb_path>: photographs of the solid under a fixed value-noise texture")
    ap.add_argument("--arc", nargs="?", type=float, const=8.0, default=None, metavar="DEGREES",
                    help="cameras on an arc this many degrees apart instead of spread over the sphere (bare flag: 8): "
                         "neighbouring views close enough for stereo")
    ap.add_argument("--backend", choices=("gpu", "host"), default="gpu")
    args = ap.parse_args(argv)
    arc = None if args.arc is None else arc_cameras(args.views, args.height, args.width, args.arc)
    scan = solid_scan(args.shape, args.views, args.height, args.width, backend=args.backend, contours=args.contours,
                      synth_cameras=arc)
    write_solid_scan(args.out_dir, scan, depth=args.depth, cloud=args.cloud, photos=args.photos)
    print(f"{args.shape}: {len(scan.cameras)} views of {args.width}x{args.height}, {scan.tris.shape[0]} triangles, "
          f"{len(scan.edges['lines_end_pts'])} lines, {len(scan.edges['curves_ctl_pts'])} curves, "
          f"{int(scan.hidden.sum())} hidden samples"
          + (f", {int(scan.contours.sum())} contour pixels" if scan.contours is not None else "") + f" -> {args.out_dir}")
    return 0
