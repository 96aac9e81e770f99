"""Shared inputs of the edge-join tests (test_edge_join_cpu.py, test_edge_join_gpu.py): the definition of the end attachment
as a brute-force all-pairs numpy expression, point sets on a dyadic grid (so that every test of the rule hits its bound
EXACTLY), hand-placed cases with a known answer, and the drawn fixtures: the shortened scan, the constructed scan after
deduping and the trimmed scan."""
import functools

import numpy as np

import edge_dedupe_cases as C
import edge_score_cases as EC
from curve_gaussian_amd.ops import edge_join as EJ
from curve_gaussian_amd.ops import edge_support as SP
from curve_gaussian_amd.ops import edge_trim as ET

NO_ATTACH = -1
GRID = C.GRID                          # 2^-6: the points are integers times this, every product below is exact
GRID_TOL = C.GRID_TOL                  # 5 cells: tol2 = 25 * 2^-12, the offset (3, 4, 0) lies exactly on it
GRID_REACH = 10.0 * 2.0 ** -6          # 10 cells: reach2 = 100 * 2^-12, the offset (6, 8, 0) lies exactly on it
assert np.float32(GRID_REACH) * np.float32(GRID_REACH) == np.float32(100.0 * 2.0 ** -12)


def below(x):
    """The float32 just below x: squared, it is below x^2 too."""
    return float(np.nextafter(np.float32(x), np.float32(0)))


# ------------------------------------------------------------------------------------------------ the definition
def attach_brute(points, offsets, tolerance, reach):
    """int64 [2E]: the definition of ``end_attach`` -- numpy float32, all pairs at once, the expressions of the rule as
    they are written (every numpy operation rounds once, nothing is contracted)."""
    p = np.asarray(points, np.float32).reshape(-1, 3)
    off = np.asarray(offsets, np.int64)
    P, E = len(p), len(off) - 1
    tol2 = np.float32(tolerance) * np.float32(tolerance)
    reach2 = np.float32(reach) * np.float32(reach)
    keys = np.full(2 * E, NO_ATTACH, np.int64)
    edge = np.zeros(P, np.int64)
    end_sample = np.zeros(P, bool)
    for e in range(E):
        edge[off[e]:off[e + 1]] = e
        if off[e + 1] > off[e]:
            end_sample[off[e]] = end_sample[off[e + 1] - 1] = True
    j = np.arange(P, dtype=np.uint64)
    for e in range(E):
        n = off[e + 1] - off[e]
        if n < 1:
            continue
        for end, i, inner in ((2 * e, off[e], off[e] + min(1, n - 1)), (2 * e + 1, off[e + 1] - 1, off[e + 1] - 1 - min(1, n - 1))):
            t = p[i] - p[inner]
            q = (t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]
            w = p - p[i]
            w2 = (w[:, 0] * w[:, 0] + w[:, 1] * w[:, 1]) + w[:, 2] * w[:, 2]
            s = (w[:, 0] * t[0] + w[:, 1] * t[1]) + w[:, 2] * t[2]
            rq, tq = reach2 * q, tol2 * q
            a, b = w2 * q, s * s
            near = w2 <= tol2
            tube = (s > 0) & (s * s <= rq) & ((a - b) <= tq)
            ends = end_sample & (s > 0) & (w2 <= reach2)
            ok = (edge != e) & (near | tube | ends)
            if ok.any():
                key = (w2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | j
                keys[end] = int(key[ok].min())
    return keys


def key_of(w2_cells, j):
    """The key of sample j at a squared distance of ``w2_cells`` cells^2."""
    return (int(np.float32(w2_cells * 2.0 ** -12).view(np.uint32)) << 32) | int(j)


# ------------------------------------------------------------------------------------------------ sample and edge counts
POINT_COUNTS = [0, 1, 2, 63, 64, 65, 255, 256, 257, 4161]   # around a wave and a tile; 4161 = 16 tiles and a tail of 65
EDGE_COUNTS = [1, 2, 3, 65, 129]                            # 129: 258 ends, a second tile of queries with a tail of 2
SHAPES = [(P, EDGE_COUNTS[k % 5]) for k, P in enumerate(POINT_COUNTS)] + [(0, 129), (2, 2), (65, 65), (257, 129), (4161, 1),
                                                                          (4161, 3), (4161, 65), (256, 129)]
assert len(set(SHAPES)) == len(SHAPES)


def edge_sizes(P, E):
    """int64 [E] summing to P.  Two or three edges: two halves, for three with an edge without samples between them.
    More: an edge without samples, one of a single sample and one of two samples (its ``inner`` sample is its other end),
    the rest of equal length with the remainder in the last."""
    if E == 1:
        return np.array([P], np.int64)
    if E <= 3:
        return np.array([P // 2] + [0] * (E - 2) + [P - P // 2], np.int64)
    sizes = np.zeros(E, np.int64)
    sizes[1] = min(1, P)
    sizes[3] = min(2, P - sizes[1])
    rest = [e for e in range(E) if e not in (0, 1, 3)]
    sizes[rest] = (P - sizes[1] - sizes[3]) // len(rest)
    sizes[-1] += P - sizes.sum()
    return sizes


@functools.lru_cache(maxsize=None)
def grid_case(P, E, seed=0):
    """(points float32 [P,3], offsets int32 [E+1]): every edge a walk on the dyadic grid as ``edge_dedupe_cases.grid_case``
    draws it -- inside a box of 24 cells, steps of 0 to 2 cells per axis --, so that squared distances, dot products and
    the two sides of the tube test are small integers times a power of two: each comparison of the rule holds with
    equality for some pairs and fails by one unit for others.  A step of 0 cells gives ends with a zero tangent."""
    rng = np.random.default_rng(7000 * E + P + seed)
    sizes = edge_sizes(P, E)
    parts = []
    for n in sizes:
        start = rng.integers(0, 24, 3)
        steps = rng.integers(0, 3, (int(n), 3)) * rng.choice([-1, 1], 3)
        walk = start + np.cumsum(steps, 0)
        parts.append(np.abs((walk + 24) % 48 - 24))
    cells = np.concatenate(parts) if parts else np.zeros((0, 3))
    off = np.zeros(E + 1, np.int32)
    off[1:] = np.cumsum(sizes)
    return cells.reshape(-1, 3).astype(np.float32) * GRID, off


def _case(*edges):
    pts = np.concatenate([np.asarray(e, np.float32).reshape(-1, 3) for e in edges]) * GRID
    off = np.zeros(len(edges) + 1, np.int32)
    off[1:] = np.cumsum([len(e) for e in edges])
    return pts, off


# Edge A of the hand-placed cases: three samples along x that end in the origin, so that end 1 (its last) sits at the
# origin with the outward tangent (1, 0, 0) cells: q = 1 cell^2, rq = 100 and tq = 25 cells^4 at GRID_TOL and GRID_REACH.
_A = [(-2, 0, 0), (-1, 0, 0), (0, 0, 0)]
FAR = 4000     # cells: out of every reach

# (name, edges, tolerance, reach, the sample end 1 attaches to or None, its w2 in cells^2)
PLACED = [
    # NEAR on its bound: B's only sample lies behind the end (s < 0), 5 cells away
    ("near_equal", [_A, [(-3, 4, 0)]], GRID_TOL, GRID_REACH, 3, 25),
    ("near_below", [_A, [(-3, 4, 0)]], below(GRID_TOL), GRID_REACH, None, 0),
    # ENDS on its bound: B's first sample lies ahead, 10 cells away and 8 beside the ray (outside the tube)
    ("ends_equal", [_A, [(6, 8, 0), (7, 9, 0), (8, 10, 0)]], GRID_TOL, GRID_REACH, 3, 100),
    ("ends_below", [_A, [(6, 8, 0), (7, 9, 0), (8, 10, 0)]], GRID_TOL, below(GRID_REACH), None, 0),
    ("ends_interior", [_A, [(5, 9, 0), (6, 8, 0), (7, 9, 0)]], GRID_TOL, GRID_REACH, None, 0),   # the same point, no end sample
    # TUBE, s*s == rq: an interior sample 10 cells ahead and 3 beside (w2 = 109 > reach2: ENDS could not take it either)
    ("tube_reach_equal", [_A, [(12, 5, 0), (10, 3, 0), (12, 1, 0)]], GRID_TOL, GRID_REACH, 4, 109),
    ("tube_reach_below", [_A, [(12, 5, 0), (10, 3, 0), (12, 1, 0)]], GRID_TOL, below(GRID_REACH), None, 0),
    # TUBE, w2*q - s*s == tq: an interior sample 4 cells ahead and 5 beside
    ("tube_side_equal", [_A, [(4, 12, 0), (4, 5, 0), (12, 5, 0)]], GRID_TOL, GRID_REACH, 4, 41),
    ("tube_side_below", [_A, [(4, 12, 0), (4, 5, 0), (12, 5, 0)]], below(GRID_TOL), GRID_REACH, None, 0),
    # s == 0 exactly: an end sample abreast of the end, 6 cells beside, passes neither TUBE nor ENDS; one cell ahead it does
    ("abreast", [_A, [(0, 6, 0), (-2, 8, 0)]], GRID_TOL, GRID_REACH, None, 0),
    ("abreast_ahead", [_A, [(1, 6, 0), (-2, 8, 0)]], GRID_TOL, GRID_REACH, 3, 37),
    # two samples at the same distance: the lower index wins, whichever edge it is on
    ("tie", [_A, [(FAR, 0, 0), (4, 3, 0)], [(3, 4, 0)], [(0, 5, 0)]], GRID_TOL, GRID_REACH, 4, 25),
    # the nearest accepted-looking samples are the end's own edge, folded back in front of it: excluded
    ("own_edge", [[(2, 1, 0), (1, 0, 0), (-1, 0, 0), (0, 0, 0)], [(3, 0, 0), (3, FAR, 0)]], GRID_TOL, GRID_REACH, 4, 9),
    # a one-sample edge has q = 0: only NEAR
    ("one_sample_far", [[(0, 0, 0)], [(6, 0, 0), (7, 0, 0)]], GRID_TOL, GRID_REACH, None, 0),
    ("one_sample_near", [[(0, 0, 0)], [(5, 0, 0), (7, 0, 0)]], GRID_TOL, GRID_REACH, 1, 25),
    # reach below the tolerance, and no reach at all: NEAR still holds
    ("short_reach", [_A, [(3, 4, 0), (6, 0, 0)]], GRID_TOL, 2 * float(GRID), 3, 25),
    ("no_reach", [_A, [(3, 4, 0), (6, 0, 0)]], GRID_TOL, 0.0, 3, 25),
]


def placed_case(name):
    """(points, offsets, tolerance, reach, the int64 key that end 1 must get)."""
    _, edges, tol, reach, j, w2 = next(row for row in PLACED if row[0] == name)
    pts, off = _case(*edges)
    return pts, off, tol, reach, (NO_ATTACH if j is None else key_of(w2, j))


@functools.lru_cache(maxsize=None)
def coincident_case():
    """600 samples in five edges (one without samples, one of a single sample), all at one point: every tangent is zero and
    every end attaches at distance 0 to the lowest sample that is not on its own edge."""
    off = np.array([0, 100, 300, 300, 301, 600], np.int32)
    pts = np.tile(np.array([[3, 5, 7]], np.float32) * GRID, (600, 1))
    want = np.array([100, 100, 0, 0, NO_ATTACH, NO_ATTACH, 0, 0, 0, 0], np.int64)
    return pts, off, want


TILE = 256


@functools.lru_cache(maxsize=None)
def split_case(swap):
    """4161 samples, 17 candidate tiles, each its own grid.y split when the ends fill one query tile.  Edge A (samples 0..2)
    ends in the origin; edge B (samples 3..4159) lies far away except for its sample 5, 4 cells ahead of that end in tile 0;
    edge C is the single sample 4160, the last lane of the last, partial tile, 3 cells ahead.  ``swap`` exchanges the two
    distances.  -> (points, offsets, the key of end 1): sample 4160 at w2 = 9, or with ``swap`` sample 5 at w2 = 9."""
    b = np.stack([FAR + np.arange(4157), np.zeros(4157, np.int64), np.zeros(4157, np.int64)], 1)
    b[2] = (3, 0, 0) if swap else (4, 0, 0)
    pts, off = _case(_A, b, [(4, 0, 0) if swap else (3, 0, 0)])
    assert len(pts) == 4161 and len(pts) % TILE == 65
    return pts, off, key_of(9, 5 if swap else 4160)


# ------------------------------------------------------------------------------------------------ host rules
def fan(angles_deg, gap, resolution=0.01, samples=20, centre=(0.3, 0.2, 0.1)):
    """An edge dict of lines in the plane z = centre.z that point AT ``centre`` from the directions ``angles_deg`` and stop
    ``gap`` short of it (a number, or one per line): line k runs from centre + (gap + samples * resolution) d_k to centre +
    gap d_k, so that its LAST end is the one near the centre."""
    c = np.asarray(centre, np.float64)
    gaps = np.broadcast_to(np.asarray(gap, np.float64), (len(angles_deg),))
    lines = []
    for a, g in zip(np.radians(angles_deg), gaps):
        d = np.array([np.cos(a), np.sin(a), 0.0])
        lines.append(np.concatenate([c + (g + samples * resolution) * d, c + g * d]))
    return {"curves_ctl_pts": [], "lines_end_pts": np.array(lines).tolist()}


# ------------------------------------------------------------------------------------------------ the drawn fixtures
CORNER = np.array([0.8, 0.25, 0.3])     # lines 0 and 1 of EC.SCAN_EDGES share it, at about 90 degrees
CORNER_ENDS = (3, 4)                     # edge 1 = line 0, its last end; edge 2 = line 1, its first end (the curve is edge 0)
SCAN_TOLERANCE, SCAN_REACH = 2.0 * EC.SCAN_RESOLUTION, 8.0 * EC.SCAN_RESOLUTION


@functools.lru_cache(maxsize=None)
def shortened_scan(g):
    """EC.SCAN_EDGES with every edge cut by ``g`` samples at both ends (``trim_geometry``; g = 0: the edges themselves)."""
    curves, lines = SP._edge_arrays(EC.SCAN_EDGES["curves_ctl_pts"], EC.SCAN_EDGES["lines_end_pts"])
    _, off = SP.sample_edges(curves, lines, EC.SCAN_RESOLUTION)
    spans = [[(g, int(n) - 1 - g)] for n in np.diff(off.astype(np.int64))]
    out_c, out_l, _ = ET.trim_geometry(curves, lines, off, spans)
    return {"curves_ctl_pts": out_c.tolist(), "lines_end_pts": out_l.reshape(-1, 6).tolist()}


def join_scan(edges, backend="host", **kw):
    return EJ.join_edges(edges, resolution=EC.SCAN_RESOLUTION, **{"tolerance": SCAN_TOLERANCE, "reach": SCAN_REACH, **kw},
                         backend=backend)


def edge_arrays(edge_dict):
    return SP._edge_arrays(edge_dict["curves_ctl_pts"], edge_dict["lines_end_pts"])


def constructed_pieces():
    """The 7 pieces that deduping leaves of the constructed scan: the curve, the three drawn lines, the three leaving lines
    cut to where they are a tolerance away from their drawn line."""
    return C.constructed_dedupe()["edge_dict"]


def same_result(a, b):
    """Two ``join_edges`` results agree in everything but the back end's name."""
    assert sorted(a) == sorted(b)
    assert np.array_equal(a["keys"].numpy(), b["keys"].numpy()) and a["edge_dict"] == b["edge_dict"]
    assert a["vertices"].tobytes() == b["vertices"].tobytes() and np.array_equal(a["edge_vertices"], b["edge_vertices"])
    assert a["t_junctions"] == b["t_junctions"] and a["collapsed"] == b["collapsed"] and a["rules"] == b["rules"]
    assert a["released"] == b["released"]
    assert np.array_equal(a["moved"], b["moved"]) and np.array_equal(a["offsets"], b["offsets"])
    assert {**a["settings"], "backend": b["settings"]["backend"]} == b["settings"]
