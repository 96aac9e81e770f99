"""Shared inputs of the contour tests (test_mesh_contours_cpu.py, test_mesh_contours_gpu.py): a brute-force float64
restatement of the frozen rule of cgs_mesh_contours (include/curvegs.h), written with scalars one operation at a time and
independently of the host back end of ops.mesh_contours -- a loop over views, rows and steps --, the hand-made tents whose
expected pixels are worked out below by hand, fans of tents around a wave and a workgroup, and random rows."""
import functools
import math

import numpy as np

# ------------------------------------------------------------------------------------------------ the hand-made tent
# Cameras without rotation: w2c = [I | T], eye at -T.  fx = fy = 4, cx = 12, cy = 8 in an image of 24 x 16, so that
# u = 4 X / Z + 12 and v = 4 Y / Z + 8 are exact for the numbers below.
H, W = 16, 24
K1 = [4.0, 4.0, 12.0, 8.0]


def camera(eye_x):
    """(intrinsics [1,4], w2c [1,3,4]) of the eye (eye_x, 0, 0) looking along +z."""
    return np.array([K1], np.float64), np.array([[[1.0, 0, 0, -eye_x], [0, 1.0, 0, 0], [0, 0, 1.0, 0]]], np.float64)


def cameras(eyes):
    K, M = zip(*(camera(x) for x in eyes))
    return np.concatenate(K), np.concatenate(M)


# The tent, seen from above (x to the right, z away from the eyes): the ridge at x = 0, z = 2 runs along y; the wings fall
# back to c = (-1, ., 3) and d = (+1, ., 3).
#   eye x =  0: the ridge lies on the z axis, c is left of it and d right: both faces are seen, NO contour.
#   eye x = -3: in camera space A = (3, -1.5, 2), B = (3, 1.5, 2), so m = A x B = (-6, 0, 9); C = (2, 0, 3), D = (4, 0, 3) give
#               sc = -12 + 27 = 15 and sd = -24 + 27 = 3: the same side, a CONTOUR.  u = 4 * 3 / 2 + 12 = 18 at both ends,
#               v = 4 * (-+1.5) / 2 + 8 = 5 and 11: column 18, rows 5 .. 11 (v = 11.0 is row 11).
#   eye x = -2: A = (2, -1.5, 2), B = (2, 1.5, 2), m = (-6, 0, 6); D = (3, 0, 3): sd = -18 + 18 = 0 exactly -- the d face is
#               seen EDGE-ON: a zero product, no contour.
RIDGE_A, RIDGE_B = (0.0, -1.5, 2.0), (0.0, 1.5, 2.0)
WING_C, WING_D = (-1.0, 0.0, 3.0), (1.0, 0.0, 3.0)
EYE_FRONT, EYE_SIDE, EYE_EDGE_ON = 0.0, -3.0, -2.0


def tent_row(a=RIDGE_A, b=RIDGE_B, c=WING_C, d=WING_D):
    return np.array([[a, b, c, d]], np.float32)


def tent_tris(flip_c=False, flip_d=False, a=RIDGE_A, b=RIDGE_B):
    """The tent as two triangles; a flip reverses that triangle's winding."""
    t1 = (a, WING_C, b) if flip_c else (a, b, WING_C)
    t2 = (a, b, WING_D) if flip_d else (b, a, WING_D)
    return np.array([t1, t2], np.float32)


def pixels(col, rows):
    m = np.zeros((H, W), np.uint8)
    m[list(rows), col] = 1
    return m


# name -> (row, eye, expected uint8 [H,W]); every expectation computed by hand:
#   long_ridge   a = (0, -6, 2): v = 4 * (-6) / 2 + 8 = -4, outside: the clip cuts at v = 0, rows 0 .. 11
#   one_pixel    v = 4 * (-0.375) / 2 + 8 = 7.25 and 4 * (-0.125) / 2 + 8 = 7.75: both ends in pixel (18, 7); the segment is
#                half a pixel long, a single step apart
#   behind_zero / behind_negative   B2 = 0 and B2 = -1: the row is skipped, not clipped
HAND_CASES = {
    "side": (tent_row(), EYE_SIDE, pixels(18, range(5, 12))),
    "front": (tent_row(), EYE_FRONT, pixels(0, [])),
    "edge_on": (tent_row(), EYE_EDGE_ON, pixels(0, [])),
    "swapped_wings": (tent_row(c=WING_D, d=WING_C), EYE_SIDE, pixels(18, range(5, 12))),
    "swapped_ends": (tent_row(a=RIDGE_B, b=RIDGE_A), EYE_SIDE, pixels(18, range(5, 12))),
    "long_ridge": (tent_row(a=(0.0, -6.0, 2.0)), EYE_SIDE, pixels(18, range(0, 12))),
    "one_pixel": (tent_row(a=(0.0, -0.375, 2.0), b=(0.0, -0.125, 2.0)), EYE_SIDE, pixels(18, [7])),
    "behind_zero": (tent_row(b=(0.0, 1.5, 0.0)), EYE_SIDE, pixels(0, [])),
    "behind_negative": (tent_row(b=(0.0, 1.5, -1.0)), EYE_SIDE, pixels(0, [])),
    "nan_wing": (tent_row(c=(float("nan"), 0.0, 3.0)), EYE_SIDE, pixels(0, [])),
}

# A quad in front of the ridge for the eye at x = -3, at z = 1: camera X in [1, 2.25] is u in [16, 21], Y in [-1.25, 0] is
# v in [3, 8].  Its z-buffer covers the pixel centres of rows 3 .. 7 (7.5 <= 8 < 8.5) at depth 1, so with the plane the
# ridge (depth 2) keeps rows 8 .. 11 of its 5 .. 11; without the plane it keeps them all.
QUAD = np.array([[(-2.0, -1.25, 1.0), (-0.75, -1.25, 1.0), (-0.75, 0.0, 1.0)],
                 [(-2.0, -1.25, 1.0), (-0.75, 0.0, 1.0), (-2.0, 0.0, 1.0)]], np.float32)
BEHIND_QUAD_WITH_PLANE, BEHIND_QUAD_WITHOUT = pixels(18, range(8, 12)), pixels(18, range(5, 12))


# ------------------------------------------------------------------------------------------------ fans of tents
def fan(E, contour):
    """float32 [E,4,3]: E tents side by side for the eye at x = -3, ridges at world x = 0.04 i (i = 0 .. E-1: image column
    18 + 0.08 i, so those from i = 75 on lie outside the tent image) and slightly different lengths.  contour(i) says whether
    tent i is to be a contour there.  For the ridge at x the sign of a wing (x + s, ., 3) is that of (x + 3) - 2 s: c at s = -1
    is positive, d at s = +1 positive (a contour), d at s = x + 4 negative (none)."""
    rows = []
    for i in range(E):
        x = 0.04 * i
        a, b = (x, -1.5 + 0.001 * i, 2.0), (x, 1.5, 2.0)
        d = (x + 1.0, 0.0, 3.0) if contour(i) else (2.0 * x + 4.0, 0.0, 3.0)
        rows.append([a, b, (x - 1.0, 0.0, 3.0), d])
    return np.array(rows, np.float32).reshape(E, 4, 3)


@functools.lru_cache(maxsize=None)
def _random_rows(E, seed):
    rng = np.random.default_rng(seed)
    return (rng.uniform(0.1, 0.9, (E, 1, 3)) + rng.uniform(-0.3, 0.3, (E, 4, 3))).astype(np.float32)


def random_rows(E, seed=11):
    """float32 [E,4,3]: rows around the unit cube; about half are contours of a camera that looks at the cube, and some
    leave its image."""
    return _random_rows(E, seed).copy()


def cube_cameras(V, height, width):
    """(intrinsics [V,4], w2c [V,3,4]) float64: V different cameras that look at the unit cube."""
    from curve_gaussian_amd import synthetic as S
    intr, w2c = [], []
    for c in S.fibonacci_cameras(max(V, 1), height, width)[:V]:
        intr.append([width / (2 * math.tan(c.FoVx / 2)), height / (2 * math.tan(c.FoVy / 2)), width / 2.0, height / 2.0])
        w2c.append(c.world_view_transform.double().numpy().T[:3, :4])
    return np.array(intr, np.float64).reshape(-1, 4), np.array(w2c, np.float64).reshape(-1, 3, 4)


# ------------------------------------------------------------------------------------------------ brute force
def _fmax(x, y):
    """C's fmax: a NaN operand loses."""
    if x != x:
        return y
    if y != y:
        return x
    return x if x > y else y


def _draw_row(row, K, M, height, width, plane, slack, out):
    f64 = np.float64
    m = [f64(x) for x in np.asarray(M, np.float64).reshape(12)]
    fx, fy, cx, cy = (f64(x) for x in K)
    P = []
    for X, Y, Z in np.asarray(row, np.float32).astype(np.float64):
        P.append((((m[0] * X + m[1] * Y) + m[2] * Z) + m[3], ((m[4] * X + m[5] * Y) + m[6] * Z) + m[7],
                  ((m[8] * X + m[9] * Y) + m[10] * Z) + m[11]))
    A, B, C, D = P
    if not A[2] > 0.0 or not B[2] > 0.0:
        return
    m0 = A[1] * B[2] - A[2] * B[1]
    m1 = A[2] * B[0] - A[0] * B[2]
    m2 = A[0] * B[1] - A[1] * B[0]
    sc = (m0 * C[0] + m1 * C[1]) + m2 * C[2]
    sd = (m0 * D[0] + m1 * D[1]) + m2 * D[2]
    if not sc * sd > 0.0:
        return
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
    length = _fmax(abs(dt * du), abs(dt * dv))
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


def contours_brute(rows, intr, w2c, height, width, depth=None, slack=0.0):
    """cgs_mesh_contours: uint8 [V,height,width], step by step."""
    V = len(intr)
    out = np.zeros((V, height, width), np.uint8)
    with np.errstate(all="ignore"):
        for v in range(V):
            for row in rows:
                _draw_row(row, intr[v], w2c[v], height, width, None if depth is None else depth[v], slack, out[v])
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def components(mask):
    """The number of 8-connected components of the set pixels of a [H,W] mask, by flood fill."""
    todo = {(int(i), int(j)) for i, j in zip(*np.nonzero(mask))}
    n = 0
    while todo:
        n += 1
        stack = [todo.pop()]
        while stack:
            i, j = stack.pop()
            for di in (-1, 0, 1):
                for dj in (-1, 0, 1):
                    if (i + di, j + dj) in todo:
                        todo.remove((i + di, j + dj))
                        stack.append((i + di, j + dj))
    return n
