"""Cases for the depth gate on the control-point visibility check and on the drawn views (tests/test_edge_visgate_*.py,
tests/test_novel_view_gate_*.py): a per-point Python restatement of the rule that shares nothing with
``ops.edge_occlusion.hidden_host``, the planted scene with its counts written out by hand, random scenes in which both
verdicts are common, and the box with 200 segments inside it."""
import math

import numpy as np

H, W = 12, 16   # the planted and the small random scenes


# ------------------------------------------------------------------------------------------------ brute force
def visibility_brute(curves, lines, maps_u8, K, c2w, detector, depth, slack):
    """``cgs_edge_visibility_depth`` one point at a time in Python floats (IEEE float64, one operation per expression):
    (counts int32 [E,2], kept_cells) -- kept_cells: the (edge, frame) cells in which rounding keeps at least one point."""
    c = np.asarray(curves, np.float64).reshape(-1, 4, 3)
    ln = np.asarray(lines, np.float64).reshape(-1, 2, 3)
    edges = [list(map(tuple, e)) for e in c.tolist()] + [list(map(tuple, e)) for e in ln.tolist()]
    F, h, w = maps_u8.shape
    counts = np.zeros((len(edges), 2), np.int32)
    kept_cells = 0
    for f in range(F):
        k = np.asarray(K[f], np.float64)[:3, :3].tolist()
        m = np.linalg.inv(np.asarray(c2w[f], np.float64)[:4, :4])[:3, :4].tolist()
        for e, pts in enumerate(edges):
            total, mx, nv, dropped, any_kept = 0.0, 0.0, 0, False, False
            for X, Y, Z in pts:
                cc = [((m[r][0] * X + m[r][1] * Y) + m[r][2] * Z) + m[r][3] for r in range(3)]
                x = [(k[r][0] * cc[0] + k[r][1] * cc[1]) + k[r][2] * cc[2] for r in range(3)]
                if x[2] == 0.0 or not all(math.isfinite(t) for t in x):
                    continue   # inf or NaN after the division: dropped (the scenes have no other source of them)
                ur, vr = x[0] / x[2], x[1] / x[2]
                u, v = float(np.rint(ur)), float(np.rint(vr))
                if not (0.0 <= u < w and 0.0 <= v < h):
                    continue
                any_kept = True
                if ur >= 0.0 and vr >= 0.0:
                    d = float(depth[f][int(math.floor(vr))][int(math.floor(ur))])   # float32 widened exactly
                    if cc[2] > d + slack:   # False for a NaN d
                        dropped = True
                        continue
                raw = int(maps_u8[f][int(v)][int(u)]) / 255.0
                val = 1.0 - raw if detector == "DexiNed" else raw
                total = total + val
                mx = val if nv == 0 else max(mx, val)
                nv += 1
            kept_cells += any_kept
            if nv > 0 and total / nv > 0.1 and mx > 0.5:
                counts[e, 0] += 1
            if dropped:
                counts[e, 1] += 1
    return counts, kept_cells


def hidden_brute(points, K, M, planes, slack):
    """(seen, hidden) bool [V,P] of ``cgs_project_points_depth`` one (point, view) pair at a time.  points float32 [P,3];
    K [V,4]; M [V,12]; planes float32 [V,H,W]."""
    pts = np.asarray(points, np.float32).astype(np.float64).tolist()
    V, h, w = planes.shape
    seen, hidden = np.zeros((V, len(pts)), bool), np.zeros((V, len(pts)), bool)
    for i in range(V):
        m, (fx, fy, cx, cy) = np.asarray(M[i], np.float64).reshape(12).tolist(), np.asarray(K[i], np.float64).tolist()
        for j, (X, Y, Z) in enumerate(pts):
            c0 = ((m[0] * X + m[1] * Y) + m[2] * Z) + m[3]
            c1 = ((m[4] * X + m[5] * Y) + m[6] * Z) + m[7]
            c2 = ((m[8] * X + m[9] * Y) + m[10] * Z) + m[11]
            if not c2 > 0.0:
                continue
            u, v = fx * (c0 / c2) + cx, fy * (c1 / c2) + cy
            if not (0.0 <= u < w and 0.0 <= v < h):
                continue
            d = float(planes[i][int(math.floor(v))][int(math.floor(u))])
            if c2 > d + slack:
                hidden[i, j] = True
            else:
                seen[i, j] = True
    return seen, hidden


# ------------------------------------------------------------------------------------------------ the planted scene
def planted_scene():
    """12x16 images, 3 frames, 5 curves and 4 lines, PidiNet maps that are 255 everywhere (a cell is visible iff a point
    survives), slack 0.  Frames 0 and 1: the identity camera, K = [[4,0,8],[0,4,6],[0,0,1]] -- a point (X, Y, 2) has c2 == 2.0
    exactly and lands on (u, v) = (2 X + 8, 2 Y + 6), every value a dyadic rational, nothing rounded.  Frame 2: the same
    camera two units further back (c2 == 4), an all-+inf plane.
    Plane of frame 0, by column: 0..3 hold 1.0 (hide c2 = 2), 4 NaN, 5 +inf, 6 exactly 2.0 (c2 > 2.0 + 0 is false: NOT hidden),
    7 nextafter(float32(2), 0) (hidden), 8..15 +inf.  Plane of frame 1: 1.0 everywhere."""
    def P(u, v, z=2.0):   # the point of depth z that frames 0 and 1 see at the raw coordinates (u, v)
        return [(u - 8.0) * z / 4.0, (v - 6.0) * z / 4.0, z]
    curves = np.array([
        [P(1.5, 3.5), P(9.5, 3.5), P(10.5, 3.5), P(11.5, 3.5)],     # 1 of 4 hidden in frame 0
        [P(1.5, 4.5), P(2.5, 4.5), P(9.5, 4.5), P(10.5, 4.5)],      # 2 of 4
        [P(1.5, 5.5), P(2.5, 5.5), P(3.25, 5.5), P(9.5, 5.5)],      # 3 of 4
        [P(0.5, 6.5), P(1.5, 6.5), P(2.5, 6.5), P(3.25, 6.5)],      # all 4
        [P(4.5, 7.5), P(5.5, 7.5), P(6.5, 7.5), P(7.5, 7.5)],       # NaN, +inf, the boundary (not hidden), one ulp nearer (hidden)
    ])
    lines = np.array([
        [P(9.5, 8.5), P(2.0, 4.0, -2.0)],       # one end behind the camera: mirrored onto a 1.0 pixel, c2 = -2, never hidden
        [P(-0.25, 2.5), P(-0.25, 3.5)],         # raw u in [-0.5, 0): rint keeps it at pixel 0, no plane pixel, not gated
        [P(1.5, 9.5), P(2.5, 9.5)],             # both ends hidden in frame 0
        [P(20.0, 3.5), P(30.0, 3.5)],           # outside frames 0 and 1; frame 2 sees the first end at u = 14
    ])
    K = np.tile(np.array([[4.0, 0, 8.0], [0, 4.0, 6.0], [0, 0, 1.0]]), (3, 1, 1))
    c2w = np.tile(np.eye(4), (3, 1, 1))
    c2w[2, 2, 3] = -2.0
    maps = np.full((3, H, W), 255, np.uint8)
    depth = np.full((3, H, W), np.inf, np.float32)
    depth[0, :, 0:4] = 1.0
    depth[0, :, 4] = np.nan
    depth[0, :, 6] = 2.0
    depth[0, :, 7] = np.nextafter(np.float32(2), np.float32(0))
    depth[1] = 1.0
    # [visible frames, frames the gate touched], by hand:
    #   frame 0: C0 C1 C2 C4 L0 L1 visible; C0..C4 and L2 touched
    #   frame 1: every gated point is hidden: only L0 (its mirrored end) and L1 (not gated) stay visible; C0..C4, L0, L2 touched
    #   frame 2: everything in the image is visible (L0 through its first end: the other has x2 == 0; L3 through u = 14)
    want = np.array([[2, 2], [2, 2], [2, 2], [1, 2], [2, 2], [3, 1], [3, 0], [1, 2], [1, 0]], np.int32)
    return dict(curves=curves, lines=lines, K=K, c2w=c2w, maps=maps, depth=depth, slack=0.0, detector="PidiNet", want=want)


# ------------------------------------------------------------------------------------------------ random scenes
def _look_at(eye, target):
    f = (target - eye) / np.linalg.norm(target - eye)
    r = np.cross(f, [0.0, 0.0, 1.0])
    r /= np.linalg.norm(r)
    d = np.cross(f, r)
    c2w = np.eye(4)
    c2w[:3, 0], c2w[:3, 1], c2w[:3, 2], c2w[:3, 3] = r, d, f, eye
    return c2w


def random_scene(n_curves, n_lines, F, h=H, w=W, seed=0):
    """Cameras on a ring round the unit cube of random control points; PidiNet bytes, a third of them 0 / 255 / random;
    planes that are +inf on half of the pixels and on the other half a slanted surface through the middle of the point cloud,
    so that both verdicts are common."""
    g = np.random.default_rng(seed)
    K, c2w = np.zeros((F, 3, 3)), np.zeros((F, 4, 4))
    centre = np.array([0.5, 0.5, 0.5])
    for f in range(F):
        a = 2.0 * math.pi * f / F + 0.1
        eye = centre + 2.2 * np.array([math.cos(a), math.sin(a), 0.35 * math.sin(3 * a)])
        c2w[f] = _look_at(eye, centre + g.uniform(-0.1, 0.1, 3))
        K[f] = [[0.9 * w, 0, w / 2 + g.uniform(-1, 1)], [0, 0.9 * w, h / 2 + g.uniform(-1, 1)], [0, 0, 1]]
    curves = g.uniform(-0.1, 1.1, (n_curves, 4, 3))
    lines = g.uniform(-0.1, 1.1, (n_lines, 2, 3))
    kind = g.integers(0, 3, (F, h, w))
    maps = np.where(kind == 0, 0, np.where(kind == 1, 255, g.integers(0, 256, (F, h, w)))).astype(np.uint8)
    jj, ii = np.meshgrid(np.arange(w), np.arange(h))
    surface = 2.2 + 0.5 * (jj / w - 0.5)[None] * g.uniform(-1, 1, (F, 1, 1)) + 0.5 * (ii / h - 0.5)[None] * g.uniform(-1, 1, (F, 1, 1))
    depth = np.where(g.random((F, h, w)) < 0.5, np.inf, surface).astype(np.float32)
    return dict(curves=curves, lines=lines, K=K, c2w=c2w, maps=maps, depth=depth, slack=0.001)


# (n_curves, n_lines, F): empty; two workgroups, the second almost empty; lines only; frames sliced over grid.y
RANDOM_SHAPES = [(0, 0, 1), (257, 3, 1), (0, 900, 3), (300, 300, 65)]
RANDOM_SIZES = [(12, 16), (48, 64)]


# ------------------------------------------------------------------------------------------------ the box
BOX_VIEWS, BOX_H, BOX_W = 24, 60, 80


def interior_segments(tris, n=200, shrink=0.15, seed=0):
    """n segments [n,2,3] with both ends uniform in the bounding box of ``tris`` shrunk by ``shrink`` of its extent per side:
    for the box every such point lies well inside the solid, where no camera can see it."""
    v = np.asarray(tris, np.float64).reshape(-1, 3)
    lo, hi = v.min(0), v.max(0)
    lo, hi = lo + shrink * (hi - lo), hi - shrink * (hi - lo)
    return np.random.default_rng(seed).uniform(lo, hi, (n, 2, 3))


def view_cameras(V, h=H, w=W, seed=0):
    """(intr [V,4], w2c [V,3,4]) of V pinhole cameras on a ring round the unit cube, for the drawn views."""
    g = np.random.default_rng(seed)
    intr, w2c = np.zeros((V, 4)), np.zeros((V, 3, 4))
    centre = np.array([0.5, 0.5, 0.5])
    for i in range(V):
        a = 2.0 * math.pi * i / V + 0.3
        eye = centre + 2.0 * np.array([math.cos(a), math.sin(a), 0.3])
        w2c[i] = np.linalg.inv(_look_at(eye, centre))[:3, :4]
        intr[i] = [0.9 * w, 0.9 * w, w / 2 + g.uniform(-1, 1), h / 2 + g.uniform(-1, 1)]
    return intr, w2c


def view_planes(V, h=H, w=W, seed=0):
    """float32 [V,h,w]: half +inf, half a slanted surface through the middle of the unit cube as ``view_cameras`` sees it
    (the cameras stand 2.09 from the centre)."""
    g = np.random.default_rng(seed + 1)
    jj, ii = np.meshgrid(np.arange(w), np.arange(h))
    surface = 2.09 + 0.6 * (jj / w - 0.5)[None] * g.uniform(-1, 1, (V, 1, 1)) + 0.6 * (ii / h - 0.5)[None] * g.uniform(-1, 1, (V, 1, 1))
    return np.where(g.random((V, h, w)) < 0.5, np.inf, surface).astype(np.float32)


def view_points(P, seed=0):
    """float32 [P,3] in a slightly enlarged unit cube (some fall outside the views) and float32 colours."""
    g = np.random.default_rng(seed + 2)
    return g.uniform(-0.2, 1.2, (P, 3)).astype(np.float32), g.uniform(0, 1, (P, 3)).astype(np.float32)


def crowded_points(P, seed=0):
    """``view_points`` with 60 % of the points in a ball of radius 0.12 round the cube's centre, which the planes' surfaces cut:
    the few pixels it lands on hold far more than the compositor's K = 25 newest points, hidden and visible ones interleaved."""
    pts, col = view_points(P, seed)
    g = np.random.default_rng(seed + 3)
    n = (6 * P) // 10
    d = g.normal(size=(n, 3))
    pts[:n] = (0.5 + 0.12 * g.random((n, 1)) ** (1 / 3) * d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    order = g.permutation(P)
    return pts[order], col[order]
