"""Shared inputs of the edge-dedupe tests (test_edge_dedupe_cpu.py, test_edge_dedupe_gpu.py): the definition of the cover as
a brute-force all-pairs numpy expression, point sets on a dyadic grid (so that distances and direction tests hit their
bounds EXACTLY), clusters that exercise the kernel's cull, and the constructed scan whose result is known."""
import functools
import math

import numpy as np

import edge_score_cases as EC
import edge_trim_cases as TC
from curve_gaussian_amd.ops import edge_dedupe as ED

NO_COVER = np.iinfo(np.int32).max
GRID = np.float32(2.0 ** -6)            # the points are integers times this: every difference and square below is exact
GRID_TOL = 5.0 * 2.0 ** -6              # tol2 = 25 * 2^-12: the offset (3, 4, 0) * 2^-6 lies exactly on it
assert np.float32(GRID_TOL) * np.float32(GRID_TOL) == np.float32(25.0 * 2.0 ** -12)


# ------------------------------------------------------------------------------------------------ the definition
def cover_brute(points, offsets, ranks, tolerance, cos_min):
    """int32 [P]: the definition of ``sample_cover`` -- numpy float32, all pairs at once, the expressions of the rule as
    they are written (every numpy operation rounds once, nothing is contracted)."""
    p = np.asarray(points, np.float32)
    off = np.asarray(offsets, np.int64)
    P, E = len(p), len(off) - 1
    tol2 = np.float32(tolerance) * np.float32(tolerance)
    cos2 = np.float32(cos_min) * np.float32(cos_min)
    t = np.zeros((P, 3), np.float32)
    r = np.zeros(P, np.int64)
    for e in range(E):
        n = off[e + 1] - off[e]
        for k in range(n):
            t[off[e] + k] = p[off[e] + min(k + 1, n - 1)] - p[off[e] + max(k - 1, 0)]
        r[off[e]:off[e + 1]] = ranks[e]
    q = (t[:, 0] * t[:, 0] + t[:, 1] * t[:, 1]) + t[:, 2] * t[:, 2]
    dx, dy, dz = (p[:, None, a] - p[None, :, a] for a in range(3))           # [i, j]
    d2 = (dx * dx + dy * dy) + dz * dz
    dot = (t[:, None, 0] * t[None, :, 0] + t[:, None, 1] * t[None, :, 1]) + t[:, None, 2] * t[None, :, 2]
    covers = (r[None, :] < r[:, None]) & (d2 <= tol2) & (dot * dot >= (cos2 * q[:, None]) * q[None, :])
    out = np.full(P, NO_COVER, np.int64)
    if P:
        out = np.where(covers, r[None, :], NO_COVER).min(1)
    return out.astype(np.int32)


# ------------------------------------------------------------------------------------------------ sample and edge counts
POINT_COUNTS = [0, 1, 2, 63, 64, 65, 255, 256, 257, 4161]   # around a wave and a tile; 4161 = 16 tiles and a tail of 65
EDGE_COUNTS = [1, 2, 3, 65]
SHAPES = [(P, EDGE_COUNTS[k % 4]) for k, P in enumerate(POINT_COUNTS)] + [(257, 2), (257, 65), (4161, 1), (4161, 3), (4161, 65),
                                                                          (65, 65), (2, 2)]
assert len(set(SHAPES)) == len(SHAPES)


def edge_sizes(P, E):
    """int64 [E] summing to P.  Two or three edges: two halves (a rank tie when P is even), for three with an edge without
    samples between them.  More: an edge without samples and one of a single sample, the rest of equal length (rank ties)
    with the remainder in the last."""
    if E == 1:
        return np.array([P], np.int64)
    if E <= 3:
        return np.array([P // 2] + [0] * (E - 2) + [P - P // 2], np.int64)
    sizes = np.zeros(E, np.int64)
    sizes[1] = min(1, P)
    sizes[2:] = (P - sizes[1]) // (E - 2)
    sizes[-1] += P - sizes.sum()
    return sizes


@functools.lru_cache(maxsize=None)
def grid_case(P, E, seed=0):
    """(points float32 [P,3], offsets int32 [E+1], ranks int32 [E]): every edge a walk on the dyadic grid inside a box of 24
    cells, steps of 0 to 2 cells per axis -- short enough that consecutive samples, and samples of different edges, lie
    within GRID_TOL of one another; squared distances are small integers times 2^-12, so d2 == tol2 holds exactly for
    some pairs and fails by one unit for others."""
    rng = np.random.default_rng(1000 * E + P + seed)
    sizes = edge_sizes(P, E)
    parts = []
    for n in sizes:
        start = rng.integers(0, 24, 3)
        steps = rng.integers(0, 3, (int(n), 3)) * rng.choice([-1, 1], 3)
        walk = start + np.cumsum(steps, 0)
        parts.append(np.abs((walk + 24) % 48 - 24))      # folded back into [0, 24]
    cells = np.concatenate(parts) if parts else np.zeros((0, 3))
    pts = cells.reshape(-1, 3).astype(np.float32) * GRID
    off = np.zeros(E + 1, np.int32)
    off[1:] = np.cumsum(sizes)
    return pts, off, ED.edge_ranks(off)


@functools.lru_cache(maxsize=None)
def equality_case():
    """Four parallel edges on the grid, 8 cells between consecutive samples.  A, 40 samples at (8k, 0, 0); B, 30 samples
    at (8k + 3, 4, 0): 5 cells from A's sample k, d2 == tol2 exactly, and sqrt(41) from sample k + 1; C, 20 samples at
    (8k + 3, 4, 1): d2 = 26 > 25; D, 10 samples at (8k + 2, 4, 0): d2 = 20.  Every tangent is (16, 0, 0) or (8, 0, 0) cells,
    so dot*dot == q_i * q_j exactly and the direction test at cos_min = 1 is an equality that holds.
    -> (points, offsets, ranks, expected cover)."""
    k = np.arange(40)
    line = lambda n, x, y, z: np.stack([8 * k[:n] + x, np.full(n, y), np.full(n, z)], 1)
    pts = np.concatenate([line(40, 0, 0, 0), line(30, 3, 4, 0), line(20, 3, 4, 1), line(10, 2, 4, 0)]).astype(np.float32) * GRID
    off = np.array([0, 40, 70, 90, 100], np.int32)
    want = np.concatenate([np.full(40, NO_COVER), np.zeros(30), np.ones(20), np.zeros(10)]).astype(np.int32)
    # C is one cell above B: B covers it (rank 1); D lies sqrt(20) from A (rank 0) -- and one cell from B, which ranks behind A
    return pts, off, ED.edge_ranks(off), want


@functools.lru_cache(maxsize=None)
def coincident_case():
    """600 samples in five edges, all at one point: every box is degenerate, every tangent is zero (0 >= 0 passes), and
    every sample but those of the rank-0 edge is covered by rank 0."""
    off = np.array([0, 100, 300, 300, 301, 600], np.int32)
    pts = np.tile(np.array([[3, 5, 7]], np.float32) * GRID, (600, 1))
    ranks = ED.edge_ranks(off)
    return pts, off, ranks, np.where(np.repeat(ranks, np.diff(off)) == 0, NO_COVER, 0).astype(np.int32)


CLUSTERS, CLUSTER_LONG, CLUSTER_SHORT, CLUSTER_LEAD = 64, 70, 58, 64
CLUSTER_PITCH, CLUSTER_WIDTH = 13, 8   # cells: the gap between neighbouring clusters is 13 - 8 = 5 cells = GRID_TOL


@functools.lru_cache(maxsize=None)
def cluster_case():
    """64 clusters of 128 samples (two edges of 70 and 58) in a row along x behind a leading edge of 64 samples, so that
    cluster c owns samples [64 + 128 c, 192 + 128 c) and every second cluster straddles a boundary between two 256-sample
    tiles.  A cluster fills x in [13 c, 13 c + 8] cells: the centres are 13 cells apart, more than the tolerance of 5, so
    whole tiles lie out of reach of one another, and the GAP between neighbouring clusters is exactly the tolerance.  The
    first sample of a cluster's long edge lies on its far face at (13 c + 8, 0, 0), the first of the next cluster's short
    edge on the near face at (13 (c + 1), 0, 0): d2 == tol2 between clusters.  A tile holds half a cluster, a whole one and
    half of the next, so neighbouring tiles' boxes overlap and the next but one lies 18 cells away: this case tells "far
    tiles may be skipped" from "overlapping tiles may not"; the boundary of the box cull itself is ``tile_gap_case``."""
    rng = np.random.default_rng(64)
    parts, sizes = [np.stack([np.full(CLUSTER_LEAD, -40), np.arange(CLUSTER_LEAD) % 5, np.zeros(CLUSTER_LEAD, np.int64)], 1)], \
        [CLUSTER_LEAD]
    for c in range(CLUSTERS):
        for n, face in ((CLUSTER_LONG, CLUSTER_WIDTH), (CLUSTER_SHORT, 0)):
            cells = np.stack([rng.integers(0, CLUSTER_WIDTH + 1, n), rng.integers(0, 4, n), rng.integers(0, 4, n)], 1)
            cells[0] = (face, 0, 0)
            cells[:, 0] += CLUSTER_PITCH * c
            parts.append(cells)
            sizes.append(n)
    pts = np.concatenate(parts).astype(np.float32) * GRID
    off = np.zeros(len(sizes) + 1, np.int32)
    off[1:] = np.cumsum(sizes)
    return pts, off, ED.edge_ranks(off)


TILE = 256                    # samples per tile of the kernel
GAP_CLUSTERS = 6
GAP_LONG = (140, 141)         # the long edge of an even and of an odd cluster: an odd cluster's outranks its neighbours'


@functools.lru_cache(maxsize=None)
def tile_gap_case(gap):
    """(points, offsets, ranks, queries): 6 clusters of exactly 256 samples, aligned with the kernel's tiles, in a row along
    x, cluster c in x = [c (8 + gap), c (8 + gap) + 8] cells: the boxes of neighbouring TILES are ``gap`` cells apart on x
    and overlap on y and z, so at gap = 5 the cull's g satisfies fl(g*g) == tol2 and the tile must NOT be skipped, and at
    gap = 6 it may be.  A cluster is a long edge (140 samples in an even cluster, 141 in an odd one) and a short one (the
    rest); every long edge outranks every short one, and an odd cluster's long edge outranks those of its two neighbours.
    Only four samples of a cluster lie on its faces: long[0] = (8, 0, 0) and short[1] = (8, 3, 3) on the far face, long[1] =
    (0, 3, 3) and short[0] = (0, 0, 0) on the near one; the others have 1 <= x <= 7.  So between neighbouring clusters
    exactly two pairs lie ``gap`` cells apart and every other pair further.

    ``queries``: rows (sample, the rank that covers it at gap = 5 and cos_min = 0).  For an even c, short_c[1] on the far
    face is covered by long_{c+1} -- the candidate tile lies at higher x than the queries' --, and for an odd c,
    short_{c+1}[0] on the near face by long_c -- the candidate tile at lower x, the mirrored gap.  The own cluster's long edge
    ranks behind that coverer, so the pair at exactly the tolerance decides cover[sample]."""
    rng = np.random.default_rng(256 + gap)
    pitch = CLUSTER_WIDTH + gap
    parts, sizes = [], []
    for c in range(GAP_CLUSTERS):
        for n, faces in ((GAP_LONG[c % 2], ((CLUSTER_WIDTH, 0, 0), (0, 3, 3))), (TILE - GAP_LONG[c % 2], ((0, 0, 0), (CLUSTER_WIDTH, 3, 3)))):
            cells = np.stack([rng.integers(1, CLUSTER_WIDTH, n), rng.integers(0, 4, n), rng.integers(0, 4, n)], 1)
            cells[:2] = faces
            cells[:, 0] += pitch * c
            parts.append(cells)
            sizes.append(n)
    pts = np.concatenate(parts).astype(np.float32) * GRID
    off = np.zeros(len(sizes) + 1, np.int32)
    off[1:] = np.cumsum(sizes)
    ranks = ED.edge_ranks(off)
    queries = []
    for c in range(GAP_CLUSTERS - 1):
        if c % 2 == 0:
            queries.append((int(off[2 * c + 1]) + 1, int(ranks[2 * (c + 1)])))       # short_c[1] <- long_{c+1}
        else:
            queries.append((int(off[2 * (c + 1) + 1]), int(ranks[2 * c])))            # short_{c+1}[0] <- long_c
    return pts, off, ranks, queries


def tile_box_gaps(points, tolerance):
    """(on, beyond): the ordered pairs of 256-sample tiles whose boxes the kernel's cull finds EXACTLY on its bound -- on
    some axis g = fl(lo_a - hi_b) > 0 with fl(g*g) == tol2, and on no axis beyond it -- and those it skips, in float32 as the
    kernel computes them."""
    p = np.asarray(points, np.float32)
    tol2 = np.float32(tolerance) * np.float32(tolerance)
    tiles = [p[k:k + TILE] for k in range(0, len(p), TILE)]
    lo, hi = np.stack([t.min(0) for t in tiles]), np.stack([t.max(0) for t in tiles])
    g = lo[:, None, :] - hi[None, :, :]                      # [a, b, axis]
    g = np.maximum(g, np.swapaxes(g, 0, 1))                   # the gap or the mirrored one: at most one is positive
    sq = np.where(g > 0, g * g, np.float32(0))
    beyond = (sq > tol2).any(-1)
    on = (sq == tol2).any(-1) & ~beyond
    return int(on.sum()), int(beyond.sum())


# ------------------------------------------------------------------------------------------------ the constructed scan
LEAVE_DEGREES = 10.0
LEAVE_AT, LEAVE_LENGTH = 0.5, 0.45
COPY_RANGE = (0.2, 0.7)
DRAWN_SAMPLES = [199, 152, 170, 180]      # the curve, then the three lines, at EC.SCAN_RESOLUTION
COPY_SAMPLES = [93, 76, 85, 90]
LEAVE_SAMPLES = [68, 76, 81]


def _frame(u):
    """Two unit vectors (v, w) that complete the unit vector u to a right-handed orthonormal frame."""
    v = np.cross(u, [0.0, 0.0, 1.0] if abs(u[2]) < 0.9 else [1.0, 0.0, 0.0])
    v /= np.linalg.norm(v)
    return v, np.cross(u, v)


@functools.lru_cache(maxsize=None)
def constructed_edges(delta):
    """The edge dict of the constructed scan; ``delta``: the sideways shift of the copies in units of the resolution.
    Curves: the drawn curve, its copy over COPY_RANGE (cut by the blossom).  Lines: the three drawn lines, their copies
    over COPY_RANGE (interpolation), then per drawn line one that starts on it at LEAVE_AT, leaves it at LEAVE_DEGREES in
    the plane of (u, v) and is LEAVE_LENGTH of it long.  A copy is shifted by delta * resolution along w, out of that
    plane, so that it lies no nearer to the leaving line than the drawn line itself."""
    shift = float(delta) * EC.SCAN_RESOLUTION
    l = np.asarray(EC.SCAN_EDGES["lines_end_pts"], np.float64).reshape(3, 2, 3)
    c = np.asarray(EC.SCAN_EDGES["curves_ctl_pts"], np.float64).reshape(4, 3)
    a, b = COPY_RANGE
    chord = TC.bezier_blossom(c, b, b, b) - TC.bezier_blossom(c, a, a, a)
    _, w = _frame(chord / np.linalg.norm(chord))
    copy_c = np.stack([TC.bezier_blossom(c, a, a, a), TC.bezier_blossom(c, a, a, b), TC.bezier_blossom(c, a, b, b),
                       TC.bezier_blossom(c, b, b, b)]) + shift * w
    copies, leaving = [], []
    rad = math.radians(LEAVE_DEGREES)
    for p0, p1 in l:
        d = p1 - p0
        u = d / np.linalg.norm(d)
        v, w = _frame(u)
        copies.append(np.stack([p0 + a * d, p0 + b * d]) + shift * w)
        start = p0 + LEAVE_AT * d
        leaving.append(np.stack([start, start + LEAVE_LENGTH * np.linalg.norm(d) * (math.cos(rad) * u + math.sin(rad) * v)]))
    return {"curves_ctl_pts": np.stack([c, copy_c]).reshape(2, 12).tolist(),
            "lines_end_pts": np.concatenate([l, np.stack(copies), np.stack(leaving)]).reshape(9, 6).tolist()}


DRAWN = [0, 2, 3, 4]        # edge indices of the constructed scan (curves first, then lines)
COPIES = [1, 5, 6, 7]
LEAVING = [8, 9, 10]


@functools.lru_cache(maxsize=None)
def constructed_dedupe(delta=0.5, backend="host", tolerance=2.0, cos_min=0.9, min_run=3, min_span=10):
    """``dedupe_edges`` on the constructed scan; the tolerance in units of the resolution."""
    return ED.dedupe_edges(constructed_edges(delta), resolution=EC.SCAN_RESOLUTION, tolerance=tolerance * EC.SCAN_RESOLUTION,
                           cos_min=cos_min, min_run=min_run, min_span=min_span, backend=backend)


def leave_start(tolerance):
    """The sample of a leaving line at which it is a tolerance (in resolutions) away from its drawn line."""
    return tolerance / math.sin(math.radians(LEAVE_DEGREES))


# ------------------------------------------------------------------------------------------------ the trimmed drawn scan
@functools.lru_cache(maxsize=None)
def trimmed_scan_edges():
    """The 44 pieces that trimming leaves of the drawn edges and the bogus chords (edge_trim_cases.scan_trim)."""
    return TC.scan_trim("bogus", "host", 1, None, 3, 10)["edge_dict"]
