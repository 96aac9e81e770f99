"""Shared inputs of the orientation tests (test_edge_orient_cpu.py, test_edge_orient_gpu.py): the three brute-force
definitions of ops/edge_orient.py's rule -- pixel by pixel in Python ints, point by point in Python floats --, random and
hand-placed masks, random partners, and the drawn scans of edge_trim_cases trimmed with and without orientation."""
import functools
import math

import numpy as np

import edge_dir_cases as DC
import edge_score_cases as EC
import edge_support_cases as SC
import edge_trim_cases as TC
from curve_gaussian_amd.ops import edge_orient as OR
from curve_gaussian_amd.ops import edge_trim as ET

R = 3
TOL2S = [0, 1, 2, 4, 5, 8, 9, 10, 13, 16]
TOL_PX = {t2: math.sqrt(t2) + 1e-9 for t2 in TOL2S}   # a tolerance whose floored square is t2
TH, TW = OR.TILE_HEIGHT, OR.TILE_WIDTH
PLANE_SIZES = [(1, 1), (1, 7), (7, 1), (3, 3), (8, 8), (63, 65), (64, 64), (65, 63),
               (TH - 1, TW + 1), (TH, TW), (TH + 1, TW - 1)]
DENSITIES = [0.0, 0.02, 0.3, 1.0]


# ------------------------------------------------------------------------------------------------ brute force
def octant(a, b):
    """The table of the rule, for Python ints or floats, (a, b) != (0, 0)."""
    assert a != 0 or b != 0
    if a > 0 and b >= 0:
        return 0 if abs(b) < abs(a) else 1
    if a <= 0 and b > 0:
        return 2 if abs(b) > abs(a) else 3
    if a < 0 and b <= 0:
        return 4 if abs(b) < abs(a) else 5
    assert a >= 0 and b < 0
    return 6 if abs(b) > abs(a) else 7


def moments(mask, y, x):
    """(N, Sx, Sy, Sxx, Syy, Sxy) of the window of pixel (y, x) of one view's mask, in Python ints."""
    H, W = mask.shape
    N = Sx = Sy = Sxx = Syy = Sxy = 0
    for dy in range(-R, R + 1):
        for dx in range(-R, R + 1):
            if 0 <= y + dy < H and 0 <= x + dx < W and mask[y + dy, x + dx]:
                N, Sx, Sy, Sxx, Syy, Sxy = N + 1, Sx + dx, Sy + dy, Sxx + dx * dx, Syy + dy * dy, Sxy + dx * dy
    return N, Sx, Sy, Sxx, Syy, Sxy


def derived(m):
    """(A, B, C, a, b) of the moments m."""
    N, Sx, Sy, Sxx, Syy, Sxy = m
    A, B, C = N * Sxx - Sx * Sx, N * Sxy - Sx * Sy, N * Syy - Sy * Sy
    return A, B, C, A - C, 2 * B


def code_of(m):
    """The code of a SET pixel with the moments m."""
    A, B, C, a, b = derived(m)
    if m[0] >= 3 and (a, b) != (0, 0) and 4 * (a * a + b * b) >= (A + C) * (A + C):
        return 1 << octant(a, b)
    return 0xFF


def codes_brute(masks):
    """uint8 [V,H,W]: the definition of cgs_mask_orientation, pixel by pixel."""
    masks = np.asarray(masks)
    out = np.zeros(masks.shape, np.uint8)
    for v in range(masks.shape[0]):
        for y, x in zip(*np.nonzero(masks[v])):
            out[v, y, x] = code_of(moments(masks[v], y, x))
    return out


def near_brute(codes, tol2):
    """uint8 [V,H,W]: the definition of cgs_oriented_near, pixel by pixel."""
    codes = np.asarray(codes)
    V, H, W = codes.shape
    r = math.isqrt(tol2)
    disk = [(dy, dx) for dy in range(-r, r + 1) for dx in range(-r, r + 1) if dx * dx + dy * dy <= tol2]
    out = np.zeros(codes.shape, np.uint8)
    for v in range(V):
        for y in range(H):
            for x in range(W):
                acc = 0
                for dy, dx in disk:
                    if 0 <= y + dy < H and 0 <= x + dx < W:
                        acc |= int(codes[v, y + dy, x + dx])
                out[v, y, x] = acc
    return out


def accept_bits(a, b, spread):
    """acc for the step (a, b) between a sample and its seen partner."""
    if a == 0 and b == 0:
        return 0xFF
    o = octant(a, b)
    acc = 0
    for s in range(-spread, spread + 1):
        acc |= 1 << ((o + s) % 8)
    return acc


def _project(m, k, p, H, W):
    X, Y, Z = p
    c0 = ((m[0] * X + m[1] * Y) + m[2] * Z) + m[3]
    c1 = ((m[4] * X + m[5] * Y) + m[6] * Z) + m[7]
    c2 = ((m[8] * X + m[9] * Y) + m[10] * Z) + m[11]
    if not c2 > 0.0:
        return None
    u, w = k[0] * (c0 / c2) + k[2], k[1] * (c1 / c2) + k[3]
    return (u, w) if 0.0 <= u < W and 0.0 <= w < H else None


def oriented_tally_brute(points, partner, K, M, near, spread):
    """int32 [P,2], point by point in Python floats (IEEE float64, one rounded operation at a time): the definition of
    cgs_sample_support_oriented on a zeroed tally."""
    V, H, W = near.shape
    pts = [[float(x) for x in p] for p in np.asarray(points, np.float32).astype(np.float64)]
    P = len(pts)
    out = np.zeros((P, 2), np.int32)
    for v in range(V):
        m = [float(x) for x in np.asarray(M[v], np.float64).reshape(12)]
        k = [float(x) for x in K[v]]
        for i in range(P):
            uv = _project(m, k, pts[i], H, W)
            if uv is None:
                continue
            out[i, 0] += 1
            j = int(partner[i])
            acc = 0xFF
            if j != i and 0 <= j < P:
                q = _project(m, k, pts[j], H, W)
                if q is not None:
                    dx, dy = q[0] - uv[0], q[1] - uv[1]
                    acc = accept_bits(dx * dx - dy * dy, 2.0 * (dx * dy), spread)
            out[i, 1] += (int(near[v, int(math.floor(uv[1])), int(math.floor(uv[0]))]) & acc) != 0
    return out


# ------------------------------------------------------------------------------------------------ inputs for the kernels
def random_masks(V, H, W, density, seed=0):
    """uint8 [V,H,W] of 0 and nonzero bytes (a set pixel is not always 1)."""
    rng = np.random.default_rng([seed, V, H, W, int(density * 1000)])
    return ((rng.random((V, H, W)) < density) * rng.integers(1, 256, (V, H, W))).astype(np.uint8)


def random_near(V, H, W, seed=0):
    """uint8 [V,H,W] of random bytes: every bit pattern meets every octant."""
    return np.random.default_rng([seed, V, H, W]).integers(0, 256, (V, H, W)).astype(np.uint8)


def random_partners(P, seed=0):
    """(partner int32 [P], offsets int32 [E+1]): sample_partners of random offsets with empty, one-sample and two-sample
    edges among them."""
    rng = np.random.default_rng([seed, P])
    sizes = []
    while sum(sizes) < P:
        sizes.append(int(rng.choice([0, 1, 2, 3, 17, 64, 100])))
    if sizes:
        sizes[-1] -= sum(sizes) - P
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    return OR.sample_partners(off), off


def line_mask(H, W, kind, at=None):
    """uint8 [H,W]: a one-pixel line -- "h" (row ``at``), "v" (column ``at``), "d" (y = x + at) or "a" (y = -x + at)."""
    m = np.zeros((H, W), np.uint8)
    if kind == "h":
        m[at, :] = 1
    elif kind == "v":
        m[:, at] = 1
    else:
        for x in range(W):
            y = x + at if kind == "d" else -x + at
            if 0 <= y < H:
                m[y, x] = 1
    return m


# ------------------------------------------------------------------------------------------------ hand cases for the tally
HAND_SIZE = 8                 # the views are 8 x 8 pixels
STEP = 2.0 ** -50             # one float64 step of a coordinate in [4, 8)
# A direction with dx dx - dy dy == 2 (dx dy) exactly in float64, every operation rounded (found by a search over multiples
# of STEP next to dx tan 22.5 degrees): fl(dx dx) - fl(dy dy) rounds to the very double that 2 fl(dx dy) is
TIE = (float.fromhex("0x1.b03e0b80d71e8p+0"), float.fromhex("0x1.6614cff206e08p-1"))


def hand_directions():
    """[(dx, dy, octant)]: the eight octant boundaries of the doubled angle and one float64 step to either side of each.
    Boundary k lies at a line orientation of 22.5 k degrees; the table gives it to the octant that begins there."""
    tx, ty = TIE
    on = [(1.0, 0.0), (tx, ty), (1.0, 1.0), (ty, tx), (0.0, 1.0), (-ty, tx), (-1.0, 1.0), (-tx, ty)]

    def turn(dx, dy, s):
        """(dx, dy) turned towards larger (s = 1) or smaller (s = -1) angles -- along (-dy, dx) -- by one step of the
        coordinate that moves more."""
        if abs(dx) >= abs(dy):
            return dx, dy + s * math.copysign(STEP, dx)
        return dx - s * math.copysign(STEP, dy), dy

    out = []
    for k, (dx, dy) in enumerate(on):
        out += [(dx, dy, k), turn(dx, dy, 1) + (k,), turn(dx, dy, -1) + ((k - 1) % 8,)]
    return out


def hand_tally_case():
    """(points [2,3], partner [2], K [V,4], M [V,3,4], octants [V]): the camera R = I, T = 0 and two points at Z = 1, (0, 0)
    and (1, 1), partners of each other.  View v has (fx, fy, cx, cy) = (dx, dy, 4, 4) for direction v of hand_directions:
    the first point lands on (4, 4) and the second on (4 + dx, 4 + dy), both exactly, so the step between them is (dx, dy)
    to the bit -- and (-dx, -dy), the same doubled angle, the other way round."""
    dirs = hand_directions()
    pts = np.array([[0, 0, 1], [1, 1, 1]], np.float32)
    K = np.array([[dx, dy, 4.0, 4.0] for dx, dy, _ in dirs], np.float64)
    M = np.tile(np.eye(4)[None, :3, :4], (len(dirs), 1, 1))
    return pts, np.array([1, 0], np.int32), K, M, np.array([o for _, _, o in dirs])


# ------------------------------------------------------------------------------------------------ the drawn scans
def _dilated_maps(maps, width):
    """The stored maps with every detected pixel grown to a square of ``width`` pixels (PidiNet: a bright byte is an edge)."""
    r = width // 2
    out = []
    for m in maps:
        p = np.pad(m, r)
        out.append(np.max([p[r + dy:r + dy + m.shape[0], r + dx:r + dx + m.shape[1]]
                           for dy in range(-r, r + 1) for dx in range(-r, r + 1)], axis=0).astype(np.uint8))
    return out


@functools.lru_cache(maxsize=None)
def scan_trim(which="bogus", backend="host", tolerance_px=1, max_gap=3, min_span=10, oriented=True, spread=1,
              budget_bytes=None, thin=False, dilate=0):
    """trim_edges on the drawn scan of edge_trim_cases.scan_trim, with the orientation options; ``dilate``: the width the
    drawn strokes are grown to first (0: as drawn)."""
    edges = {"extended": lambda: TC.extended_edges()[0], "drawn": lambda: EC.SCAN_EDGES, "bogus": lambda: SC.scan_edges()[0]}
    cams, maps = DC.dir_novel_cameras()
    if dilate:
        maps = _dilated_maps(maps, dilate)
    return ET.trim_edges(edges[which](), cams, maps, "PidiNet", resolution=EC.SCAN_RESOLUTION, tolerance_px=tolerance_px,
                         frames_ratio=TC.SCAN_FRAMES_RATIO, max_gap=max_gap, min_span=min_span, backend=backend,
                         budget_bytes=budget_bytes, thin=thin, oriented=oriented, spread=spread)


DRAWN_EDGES = (0, 41, 42, 43)   # the drawn edges among the 76 of the "bogus" scan


def bogus_counts(result):
    """(pieces, kept samples) on the 72 bogus chords of a "bogus" result, and whether the four drawn edges came back whole."""
    n = np.diff(result["offsets"].astype(np.int64))
    bogus = [e for e in range(len(n)) if e not in DRAWN_EDGES]
    pieces = sum(len(result["spans"][e]) for e in bogus)
    kept = sum(b - a + 1 for e in bogus for a, b in result["spans"][e])
    whole = all(result["spans"][e] == [(0, int(n[e]) - 1)] for e in DRAWN_EDGES)
    return pieces, kept, whole
