"""Shared inputs of the near-plane clipping tests (test_edge_clip_cpu.py, test_edge_clip_gpu.py): brute-force float64
restatements of the frozen rules of cgs_mesh_depth_clipped and cgs_mesh_contours_clipped (include/curvegs.h), written with
Python floats one operation at a time and independently of the host back ends of ops.edge_occlusion / ops.mesh_contours -- a
per-triangle cut, then a per-pixel loop over all pieces; a loop over views, rows and steps for the contours --, an
independent truth (a float64 Moeller-Trumbore ray cast against the UNCLIPPED triangles), and the cases they run on.

Camera 0 of ``edge_occlusion_cases.cameras`` is the identity pose with fx = fy = 1, cx = cy = 0: camera space is world
space, u = X / Z, v = Y / Z, and a vertex's c2 is its float32 Z exactly.  NEAR = 0.25 is exact in float32."""
import functools
import math

import numpy as np

import edge_occlusion_cases as OC
import mesh_contours_cases as MC

NEAR = 0.25
SIZES = [(1, 1), (5, 33), (5, 67)]   # (height, width): one pixel, and two rows of more than one wave's stride
WIDTHS = [w for _, w in SIZES]


def height(W):
    """The height of the test image of width W."""
    return dict((w, h) for h, w in SIZES)[W]


VIEWS = [1, 2, 5]
FACES = [0, 1, 63, 64, 65, 257]
ROWS = [0, 1, 63, 64, 65, 257]
ULP2 = 2.0 ** -22               # 2 float32 ulps, relative: 2.4e-7
BORDER_CAP = 0.001              # the share of the pixels the ray cast may leave out as border cases (a cap)

same_bits = OC.same_bits
cameras = OC.cameras


# ------------------------------------------------------------------------------------------------ triangles
def _on_plane(xy):
    """Points of the plane 0.01 X + 0.1 Y + Z = 1 above (X, Y): every ray of camera 0 through a pixel of the test images
    (1 x 1, 5 x 33, 5 x 67: u in [0, 67], v in [0, 5]) meets it, at X in [0, 41], Y in [0, 3.4], Z in [0.46, 1]."""
    return [[x, y, 1.0 - 0.01 * x - 0.1 * y] for x, y in xy]


_BELOW = float(np.nextafter(np.float32(NEAR), np.float32(0.0)))   # one float32 ulp below the plane
# The floor: one triangle of the plane above, two vertices IN (Z = 111, 71) and one far behind the camera (Z = -289); its
# clipped pieces cover every pixel of every test image of camera 0.
FLOOR = _on_plane([(-1000.0, -1000.0), (3000.0, -1000.0), (-1000.0, 3000.0)])
# The pair: the quadrilateral A B C D of the same plane cut along A-C.  A (Z = 3.5) and B (Z = 1) are IN, C (Z = -7) and D
# (Z = -4.5) OUT, so the shared edge A-C straddles; it crosses the images between (12.5, 0) and (21.9, 3) in (X, Y).
QUAD_XY = [(-50.0, -20.0), (200.0, -20.0), (200.0, 60.0), (-50.0, 60.0)]
_A, _B, _C, _D = _on_plane(QUAD_XY)
PAIRS = {   # both orders of the triangles, the shared edge's vertices listed in both directions
    "abc_acd": [[_A, _B, _C], [_A, _C, _D]],
    "acd_abc": [[_A, _C, _D], [_A, _B, _C]],
    "cab_acd": [[_C, _A, _B], [_A, _C, _D]],
    "abc_cad": [[_A, _B, _C], [_C, _A, _D]],
    "bca_dca": [[_B, _C, _A], [_D, _C, _A]],
}
nan = float("nan")
SINGLES = {   # name -> one triangle in camera 0's space
    "three_in": [[0.0, 0.0, 1.0], [40.0, 0.0, 1.0], [0.0, 6.0, 1.0]],
    "none_in_front": [[0.0, 0.0, 0.125], [4.0, 0.0, 0.125], [0.0, 1.0, 0.125]],          # 0 < c2 < near: all OUT
    "none_in_behind": [[0.0, 0.0, -1.0], [4.0, 0.0, -1.0], [0.0, 4.0, -1.0]],
    "one_in_0": [[1.0, 1.0, 2.0], [30.0, 0.0, 0.125], [0.0, 9.0, -1.0]],
    "one_in_1": [[0.0, 9.0, -1.0], [1.0, 1.0, 2.0], [30.0, 0.0, 0.125]],
    "one_in_2": [[30.0, 0.0, 0.125], [0.0, 9.0, -1.0], [1.0, 1.0, 2.0]],
    "two_in_0": [[4.0, 8.0, -1.0], [1.0, 1.0, 2.0], [90.0, 2.0, 3.0]],
    "two_in_1": [[90.0, 2.0, 3.0], [4.0, 8.0, -1.0], [1.0, 1.0, 2.0]],
    "two_in_2": [[1.0, 1.0, 2.0], [90.0, 2.0, 3.0], [4.0, 8.0, -1.0]],
    "vertex_at_near": [[0.0, 0.0, NEAR], [20.0, 0.0, 2.0], [0.0, 9.0, 2.0]],               # c2 == near is IN: unclipped
    "vertex_ulp_below": [[0.0, 0.0, _BELOW], [20.0, 0.0, 2.0], [0.0, 9.0, 2.0]],          # one ulp below: OUT, two pieces
    "in_the_plane": [[0.0, 0.0, NEAR], [10.0, 0.0, NEAR], [0.0, 1.5, NEAR]],              # all three at c2 == near: IN
    "sliver_zero_area": [[1.0, 1.0, NEAR], [5.0, 1.0, 0.125], [1.0, 3.0, -2.0]],          # the one IN vertex ON the plane:
                                                                                         # t = 0 twice, the piece is a point
    "nan_vertex": [[nan, 0.0, 1.0], [40.0, 0.0, 1.0], [0.0, 6.0, -1.0]],
    "nan_depth": [[0.0, 0.0, nan], [40.0, 0.0, 1.0], [0.0, 6.0, 1.0]],
    "far_behind": [[1.0, 1.0, 2.0], [90.0, 2.0, 3.0], [4.0, 8.0, -1.0e6]],
    "floor": FLOOR,
}
EXPECT_EMPTY = ("none_in_front", "none_in_behind", "sliver_zero_area", "nan_vertex", "nan_depth")


def single(name):
    return np.array([SINGLES[name]], np.float32)


def pair(name):
    return np.array(PAIRS[name], np.float32)


@functools.lru_cache(maxsize=None)
def _cloud(F, seed):
    rng = np.random.default_rng(seed)
    centre = rng.uniform(-2.0, 2.0, (F, 1, 3))
    t = centre + rng.uniform(-1.5, 1.5, (F, 3, 3))   # large triangles all around camera 0, most of which straddle a plane
    specials = np.concatenate([single(n) for n in SINGLES] + [pair("abc_acd")])
    return np.concatenate([specials, t.astype(np.float32)])[:F].copy() if F else np.zeros((0, 3, 3), np.float32)


def cloud(F, seed=17):
    """float32 [F,3,3]: the special triangles first (all of them from F = 63 on), then random triangles around camera 0,
    which stands inside their cloud; the cameras 1 .. 4 (radius 1.8 around the unit cube) stand inside it too."""
    return _cloud(F, seed).copy()


# ------------------------------------------------------------------------------------------------ brute force: z-buffer
def _camera_xyz(M, X, Y, Z):
    m = [float(x) for x in np.asarray(M, np.float64).reshape(12)]
    return (((m[0] * X + m[1] * Y) + m[2] * Z) + m[3], ((m[4] * X + m[5] * Y) + m[6] * Z) + m[7],
            ((m[8] * X + m[9] * Y) + m[10] * Z) + m[11])


def cut(a, b, near):
    """THE cut, from the IN end a toward the OUT end b (a[2] >= near > b[2], so the divisor is positive)."""
    t = (a[2] - near) / (a[2] - b[2])
    return (a[0] + t * (b[0] - a[0]), a[1] + t * (b[1] - a[1]), near)


def pieces_of(C, near):
    """The pieces of a camera-space triangle C = [c_0, c_1, c_2]: a list of 0, 1 or 2 vertex triples."""
    if any(x != x for c in C for x in c):
        return []
    ins = [c[2] >= near for c in C]
    if sum(ins) == 3:
        return [tuple(C)]
    if sum(ins) == 0:
        return []
    if sum(ins) == 1:
        i = ins.index(True)
        a, b, c = C[i], C[(i + 1) % 3], C[(i + 2) % 3]
        return [(a, cut(a, b, near), cut(a, c, near))]
    i = ins.index(False)
    c, a, b = C[i], C[(i + 1) % 3], C[(i + 2) % 3]
    return [(a, b, cut(b, c, near)), (a, cut(b, c, near), cut(a, c, near))]


def _prepare_piece(piece, K, H, W):
    """The set-up of cgs_mesh_depth from three camera-space vertices: None for a skipped piece."""
    fx, fy, cx, cy = (float(x) for x in K)
    u, v, z = [], [], []
    for c0, c1, c2 in piece:
        if not c2 > 0.0:
            return None
        uu, vv = fx * (c0 / c2) + cx, fy * (c1 / c2) + cy
        if uu != uu or vv != vv:
            return None
        u.append(uu), v.append(vv), z.append(c2)
    area = (u[1] - u[0]) * (v[2] - v[0]) - (v[1] - v[0]) * (u[2] - u[0])
    if area == 0.0 or area != area:
        return None
    return (u, v, z, area, OC._clamped(math.ceil, min(u) - 0.5, 0, W), OC._clamped(math.floor, max(u) - 0.5, -1, W - 1),
            OC._clamped(math.ceil, min(v) - 0.5, 0, H), OC._clamped(math.floor, max(v) - 0.5, -1, H - 1))


def _pixel(prepared, i, j):
    """float32 depth of the pixel under the prepared pieces, +inf where none stores."""
    px, py = j + 0.5, i + 0.5
    best = np.float32(np.inf)
    for u, v, z, area, jlo, jhi, ilo, ihi in prepared:
        if not (jlo <= j <= jhi and ilo <= i <= ihi):
            continue
        e0 = (u[2] - u[1]) * (py - v[1]) - (v[2] - v[1]) * (px - u[1])
        e1 = (u[0] - u[2]) * (py - v[2]) - (v[0] - v[2]) * (px - u[2])
        e2 = (u[1] - u[0]) * (py - v[0]) - (v[1] - v[0]) * (px - u[0])
        if not ((e0 >= 0 and e1 >= 0 and e2 >= 0) or (e0 <= 0 and e1 <= 0 and e2 <= 0)):
            continue
        invz = ((e0 / area) / z[0] + (e1 / area) / z[1]) + (e2 / area) / z[2]
        if invz == 0.0 or invz != invz:
            continue
        with np.errstate(over="ignore"):
            zf = np.float32(1.0 / invz)
        if zf > 0 and np.isfinite(zf) and zf < best:
            best = zf
    return best


def zbuffer_clipped_brute(tris, K, M, H, W, near=NEAR):
    """cgs_mesh_depth_clipped: float32 [V,H,W], triangle by triangle for the cut and pixel by pixel over ALL pieces."""
    tris = np.asarray(tris, np.float32).reshape(-1, 3, 3)
    out = np.full((len(K), H, W), np.inf, np.float32)
    for view in range(len(K)):
        prepared = []
        for t in tris:
            C = [_camera_xyz(M[view], float(X), float(Y), float(Z)) for X, Y, Z in t]
            prepared += [p for p in (_prepare_piece(q, K[view], H, W) for q in pieces_of(C, near)) if p is not None]
        for i in range(H):
            for j in range(W):
                out[view, i, j] = _pixel(prepared, i, j)
    return out


@functools.lru_cache(maxsize=None)
def reference_cloud(F, W, V):
    """The brute-force clipped z-buffer of cloud(F) in cameras(V, height(W), W): computed once, shared, read-only."""
    K, M = cameras(V, height(W), W)
    out = zbuffer_clipped_brute(cloud(F), K, M, height(W), W)
    out.setflags(write=False)
    return out


# ------------------------------------------------------------------------------------------------ the independent truth
def ray_cast(tris, K, M, H, W, near):
    """float64 [V,H,W]: the camera depth of the nearest hit with depth >= near of the ray through every pixel centre with
    the UNCLIPPED triangles (Moeller-Trumbore, vectorised over the pixels), +inf where there is none.  In camera space the ray
    is s * (x, y, 1) from the origin, so a hit's parameter s IS its camera depth."""
    T = np.asarray(tris, np.float32).astype(np.float64).reshape(-1, 3, 3)
    out = np.full((len(K), H, W), np.inf)
    jj, ii = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
    for view in range(len(K)):
        R, t = np.asarray(M[view], np.float64).reshape(3, 4)[:, :3], np.asarray(M[view], np.float64).reshape(3, 4)[:, 3]
        fx, fy, cx, cy = (float(x) for x in K[view])
        d = np.stack([(jj - cx) / fx, (ii - cy) / fy, np.ones_like(jj)], -1)   # [H,W,3]
        for tri in T:
            if np.isnan(tri).any():
                continue
            v0, v1, v2 = (R @ p + t for p in tri)
            e1, e2 = v1 - v0, v2 - v0
            with np.errstate(all="ignore"):
                p = np.cross(d, e2)
                det = p @ e1
                s = -v0   # the origin minus v0
                uu = (p @ s) / det
                q = np.cross(s, e1)
                vv = (d @ q) / det
                depth = (q @ e2) / det
                hit = (det != 0.0) & (uu >= 0.0) & (vv >= 0.0) & (uu + vv <= 1.0) & (depth >= near)
            out[view] = np.where(hit & (depth < out[view]), depth, out[view])
    return out


def against_ray_cast(planes, truth):
    """(border pixels, largest relative error where both are finite) of float32 planes against ``ray_cast``."""
    planes = np.asarray(planes, np.float64)
    both = np.isfinite(planes) & np.isfinite(truth)
    border = int((np.isfinite(planes) != np.isfinite(truth)).sum())
    rel = np.abs(planes[both] - truth[both]) / truth[both]
    return border, float(rel.max()) if rel.size else 0.0


# ------------------------------------------------------------------------------------------------ the crack property
def clipped_polygon(quad_xyz, near):
    """The part of a planar convex polygon (camera space, float64) with c2 >= near: Sutherland-Hodgman, independent of THE cut."""
    out = []
    n = len(quad_xyz)
    for k in range(n):
        a, b = np.asarray(quad_xyz[k], np.float64), np.asarray(quad_xyz[(k + 1) % n], np.float64)
        if a[2] >= near:
            out.append(a)
        if (a[2] >= near) != (b[2] >= near):
            s = (near - a[2]) / (b[2] - a[2])
            out.append(a + s * (b - a))
    return out


def centres_inside(poly_uv, H, W, margin):
    """bool [H,W]: the pixel centres inside the convex image polygon by more than ``margin`` pixels (so that no rounding of
    a coverage test can matter)."""
    jj, ii = np.meshgrid(np.arange(W) + 0.5, np.arange(H) + 0.5)
    inside_pos, inside_neg = np.ones((H, W), bool), np.ones((H, W), bool)
    n = len(poly_uv)
    for k in range(n):
        (u0, v0), (u1, v1) = poly_uv[k], poly_uv[(k + 1) % n]
        length = math.hypot(u1 - u0, v1 - v0)
        dist = ((u1 - u0) * (ii - v0) - (v1 - v0) * (jj - u0)) / length
        inside_pos &= dist > margin
        inside_neg &= dist < -margin
    return inside_pos | inside_neg


# ------------------------------------------------------------------------------------------------ brute force: contours
def _draw_row_clipped(row, K, M, height, width, plane, slack, near, out):
    f64 = np.float64
    fx, fy, cx, cy = (f64(x) for x in K)
    P = [tuple(f64(x) for x in _camera_xyz(M, f64(X), f64(Y), f64(Z))) for X, Y, Z in
         np.asarray(row, np.float32).astype(np.float64)]
    A, B, C, D = P
    in_a, in_b = bool(A[2] >= near), bool(B[2] >= near)
    if not in_a and not in_b:
        return
    m0 = A[1] * B[2] - A[2] * B[1]
    m1 = A[2] * B[0] - A[0] * B[2]
    m2 = A[0] * B[1] - A[1] * B[0]
    sc = (m0 * C[0] + m1 * C[1]) + m2 * C[2]
    sd = (m0 * D[0] + m1 * D[1]) + m2 * D[2]
    if not sc * sd > 0.0:
        return
    if not in_b:
        B = tuple(f64(x) for x in cut(A, B, f64(near)))
    elif not in_a:
        A = tuple(f64(x) for x in cut(B, A, f64(near)))
    ua, va = fx * (A[0] / A[2]) + cx, fy * (A[1] / A[2]) + cy
    ub, vb = fx * (B[0] / B[2]) + cx, fy * (B[1] / B[2]) + cy
    du, dv = ub - ua, vb - va
    wd, hd = f64(width), f64(height)
    t0, t1 = f64(0.0), f64(1.0)
    for p, q in ((-du, ua), (du, wd - ua), (-dv, va), (dv, hd - va)):
        if p == 0.0:
            if q < 0.0:
                return
            continue
        r = q / p
        if p < 0.0:
            if r > t1:
                return
            if r > t0:
                t0 = r
        else:
            if r < t0:
                return
            if r < t1:
                t1 = r
    dt = t1 - t0
    length = MC._fmax(abs(dt * du), abs(dt * dv))
    if not length <= wd + hd:
        return
    n = int(math.ceil(2.0 * length))
    for k in range(n + 1):
        f = f64(k) / f64(n) if n > 0 else f64(0.0)
        t = t0 + dt * f
        u = ua + t * du
        v = va + t * dv
        if not (u >= 0.0 and u < wd and v >= 0.0 and v < hd):
            continue
        i, j = int(math.floor(v)), int(math.floor(u))
        if plane is not None:
            z = 1.0 / ((1.0 - t) / A[2] + t / B[2])
            if z > f64(plane[i, j]) + f64(slack):
                continue
        out[i, j] = 1


def contours_clipped_brute(rows, intr, w2c, height, width, depth=None, slack=0.0, near=NEAR):
    """cgs_mesh_contours_clipped: uint8 [V,height,width], step by step."""
    V = len(intr)
    out = np.zeros((V, height, width), np.uint8)
    with np.errstate(all="ignore"):
        for v in range(V):
            for row in rows:
                _draw_row_clipped(row, intr[v], w2c[v], height, width, None if depth is None else depth[v], slack, near,
                                  out[v])
    return out


# The hand-made tent of mesh_contours_cases.py seen from the eye at x = -3 (camera z = world z): name -> (row, ends IN).
#   b_behind   B2 = -1: skipped whole without clipping, with it the ridge is cut at c2 = 0.25 and drawn from A toward the cut
#   b_at_near  B2 == near exactly: IN, unclipped
TENT_ROWS = {
    "both_in": (MC.tent_row(), 2),
    "b_behind": (MC.tent_row(b=(0.0, 1.5, -1.0)), 1),
    "a_behind": (MC.tent_row(a=(0.0, -1.5, -1.0)), 1),
    "b_in_front_of_near": (MC.tent_row(b=(0.0, 1.5, 0.125)), 1),
    "b_at_near": (MC.tent_row(b=(0.0, 1.5, NEAR)), 2),
    "both_out": (MC.tent_row(a=(0.0, -1.5, 0.125), b=(0.0, 1.5, -1.0)), 0),
    "nan_end": (MC.tent_row(b=(0.0, float("nan"), 2.0)), 1),
}


def cloud_rows(E, seed=23):
    """float32 [E,4,3]: the tent rows first, then random rows around camera 0 of ``cameras`` -- it stands inside them."""
    rng = np.random.default_rng(seed)
    rnd = (rng.uniform(-1.0, 1.0, (E, 1, 3)) + rng.uniform(-1.2, 1.2, (E, 4, 3))).astype(np.float32)
    tents = np.concatenate([r for r, _ in TENT_ROWS.values()])
    return np.concatenate([tents, rnd])[:E].copy() if E else np.zeros((0, 4, 3), np.float32)
