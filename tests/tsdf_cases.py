"""Inputs and brute-force restatements for the distance-field tests (include/curvegs.h: cgs_tsdf_integrate,
cgs_tsdf_mesh_count, cgs_tsdf_mesh_emit), shared by test_tsdf_cpu.py and test_tsdf_gpu.py.  The brute force is written from
the header's text in Python floats -- every lattice point x view, every cell x tetrahedron, one operation a line, the 16
cases derived from the header's sentences -- and shares no code with ops/tsdf.py."""
import itertools
import json
import math

import numpy as np

from stereo_cases import _div, _f32, same_bits  # noqa: F401  (same_bits is re-exported to the tests)

INF = float("inf")
NAN = float("nan")
MAX_WEIGHT = 65535


def lattice(bounds, dims):
    """(lo, step) as lists of Python floats: step = (hi - lo) / dims per axis, one division."""
    lo, hi = (np.asarray(b, np.float64) for b in bounds)
    return lo.tolist(), ((hi - lo) / np.asarray(dims, np.float64)).tolist()


def centre(lo, step, axis, i):
    return float(_f32(lo[axis] + (i + 0.5) * step[axis]))


# ------------------------------------------------------------------------------------------------ the brute force
def brute_integrate(depth, K, M, dims, bounds, trunc, state=None):
    """(sum float64 [n], weight uint16 [n])."""
    depth = np.asarray(depth, np.float32)
    V, H, W = depth.shape
    K, M = np.asarray(K, np.float64).reshape(V, 4).tolist(), np.asarray(M, np.float64).reshape(V, 12).tolist()
    lo, step = lattice(bounds, dims)
    nx, ny, nz = dims
    n = nx * ny * nz
    total = [0.0] * n if state is None else np.asarray(state[0], np.float64).tolist()
    weight = [0] * n if state is None else np.asarray(state[1]).astype(np.int64).tolist()
    for g in range(n):
        X, Y, Z = centre(lo, step, 0, g % nx), centre(lo, step, 1, (g // nx) % ny), centre(lo, step, 2, g // (nx * ny))
        for v in range(V):
            m = M[v]
            fx, fy, cx, cy = K[v]
            c0 = ((m[0] * X + m[1] * Y) + m[2] * Z) + m[3]
            c1 = ((m[4] * X + m[5] * Y) + m[6] * Z) + m[7]
            c2 = ((m[8] * X + m[9] * Y) + m[10] * Z) + m[11]
            if c2 <= 0.0:
                continue
            u = fx * _div(c0, c2) + cx
            vv = fy * _div(c1, c2) + cy
            if not (0.0 <= u < W and 0.0 <= vv < H):
                continue
            d = float(depth[v, int(math.floor(vv)), int(math.floor(u))])
            if not (d > 0.0 and d < INF):
                continue
            sdf = d - c2
            if sdf < -trunc:
                continue
            if weight[g] == MAX_WEIGHT:
                continue
            t = _div(sdf, trunc)
            if t > 1.0:
                t = 1.0
            total[g] = total[g] + t
            weight[g] += 1
    return np.array(total, np.float64), np.array(weight, np.int64).astype(np.uint16)


def tetrahedra():
    """[(corners (q0, q1, q2, q3), odd)]: one per order of the axes, lexicographic."""
    out = []
    for order in itertools.permutations((0, 1, 2)):
        a, b, _ = order
        inversions = sum(order[x] > order[y] for x in range(3) for y in range(x + 1, 3))
        out.append(((0, 1 << a, (1 << a) | (1 << b), 7), inversions % 2 == 1))
    return out


def case_triangles(inside, odd):
    """The triangles of a tetrahedron whose corners x with inside[x] are inside: triples of (x, y) edges, x < y."""
    ins = [x for x in range(4) if inside[x]]
    outs = [x for x in range(4) if not inside[x]]
    E = lambda x, y: (x, y) if x < y else (y, x)
    if len(ins) == 1:
        x, (p, q, r) = ins[0], outs
        tris, turned = [[E(x, p), E(x, q), E(x, r)]], x % 2 == 1
    elif len(ins) == 3:
        x, (p, q, r) = outs[0], ins
        tris, turned = [[E(x, p), E(x, q), E(x, r)]], x % 2 == 0
    elif len(ins) == 2:
        (i, j), (k, l) = ins, outs
        perm = (i, j, k, l)
        turned = sum(perm[x] > perm[y] for x in range(4) for y in range(x + 1, 4)) % 2 == 1
        tris = [[E(i, k), E(i, l), E(j, l)], [E(i, k), E(j, l), E(j, k)]]
    else:
        return []
    if odd:
        turned = not turned
    return [[t[0], t[2], t[1]] if turned else t for t in tris]


def brute_extract(total, weight, dims, bounds, min_weight):
    """(counts uint8 [cells], tris float32 [T,3,3]) in the header's order."""
    total, weight = np.asarray(total, np.float64).tolist(), np.asarray(weight).astype(np.int64).tolist()
    lo, step = lattice(bounds, dims)
    nx, ny, nz = dims
    tets = tetrahedra()
    counts, tris = [], []
    for k in range(nz - 1):
        for j in range(ny - 1):
            for i in range(nx - 1):
                ids = [(i + (c & 1)) + nx * ((j + ((c >> 1) & 1)) + ny * (k + (c >> 2))) for c in range(8)]
                if any(weight[g] < min_weight for g in ids):
                    counts.append(0)
                    continue
                f = [_div(total[g], float(weight[g])) for g in ids]
                P = [(centre(lo, step, 0, i + (c & 1)), centre(lo, step, 1, j + ((c >> 1) & 1)), centre(lo, step, 2, k + (c >> 2)))
                     for c in range(8)]
                before = len(tris)
                for q, odd in tets:
                    for tri in case_triangles([f[c] < 0.0 for c in q], odd):
                        out = []
                        for x, y in tri:
                            a, b = q[x], q[y]          # a < b: ascending corner number is ascending lattice index
                            w = _div(f[a], f[a] - f[b])
                            out.append([float(_f32(P[a][axis] + w * (P[b][axis] - P[a][axis]))) for axis in range(3)])
                        tris.append(out)
                counts.append(len(tris) - before)
    return np.array(counts, np.uint8).reshape(-1), np.array(tris, np.float32).reshape(-1, 3, 3)


# ------------------------------------------------------------------------------------------------ cameras and maps
def look_at(eye, target, up=(0.0, 0.0, 1.0)):
    """[R | T] (12 doubles, row-major), world -> camera, z forward, y down."""
    eye, target, up = (np.asarray(x, np.float64) for x in (eye, target, up))
    fwd = (target - eye) / np.linalg.norm(target - eye)
    right = np.cross(fwd, up)
    right /= np.linalg.norm(right)
    down = np.cross(fwd, right)
    R = np.stack([right, down, fwd])
    return np.concatenate([R, (-R @ eye)[:, None]], 1).reshape(12)


BOUNDS = ((0.1, 0.2, 0.3), (0.9, 1.0, 0.8))


def random_case(dims, V, H, W, seed, bounds=BOUNDS, trunc=0.15):
    """Cameras on a ring around the box whose images the lattice overflows on every side, and maps that hold ordinary
    depths on both sides of the lattice's, 0, negative depths, NaN and +inf."""
    rng = np.random.default_rng(seed)
    mid = 0.5 * (np.asarray(bounds[0]) + np.asarray(bounds[1]))
    K, M = np.zeros((V, 4)), np.zeros((V, 12))
    for v in range(V):
        a = 2.0 * math.pi * (v + rng.uniform(0.0, 0.5)) / V
        eye = mid + np.array([1.6 * math.cos(a), 1.6 * math.sin(a), rng.uniform(-0.4, 0.6)])
        M[v] = look_at(eye, mid + rng.uniform(-0.05, 0.05, 3))
        K[v] = (1.7 * W, 1.9 * H, 0.5 * W + rng.uniform(-0.3, 0.3), 0.5 * H + rng.uniform(-0.3, 0.3))
    depth = rng.uniform(1.2, 2.0, (V, H, W)).astype(np.float32)
    kind = rng.integers(0, 12, (V, H, W))
    for code, value in ((0, 0.0), (1, -1.5), (2, NAN), (3, INF)):
        depth[kind == code] = value
    return dict(depth=depth, K=K, M=M, dims=tuple(dims), bounds=bounds, trunc=trunc)


def one_point(d, trunc=0.25, cx=0.0, tz=0.0, width=1):
    """A 1 x 1 x 1 lattice whose point (0.5, 0.5, 2.0) an axis-aligned camera sees at u = 0.5 + cx, depth 2.0 + tz, in a
    1 x ``width`` map filled with ``d``: every number is exact in binary."""
    M = np.array([1.0, 0, 0, 0, 0, 1.0, 0, 0, 0, 0, 1.0, tz], np.float64)
    return dict(depth=np.full((1, 1, width), d, np.float32), K=np.array([[2.0, 2.0, cx, 0.0]]), M=M[None], dims=(1, 1, 1),
                bounds=((0.0, 0.0, 1.5), (1.0, 1.0, 2.5)), trunc=trunc)


def views(case, v0, v1):
    return dict(case, depth=case["depth"][v0:v1], K=case["K"][v0:v1], M=case["M"][v0:v1])


# ------------------------------------------------------------------------------------------------ fields
CELL_BOUNDS = ((0.25, -0.5, 1.0), (1.25, 1.5, 4.0))   # one cell of a 2 x 2 x 2 lattice, a different step per axis


def pattern_state(pattern, magnitudes=None, weight=2):
    """(sum, weight) of a 2 x 2 x 2 lattice whose corner c is inside iff bit c of ``pattern`` is set: f = -+magnitude."""
    mag = np.ones(8) if magnitudes is None else np.asarray(magnitudes, np.float64)
    f = np.where([(pattern >> c) & 1 for c in range(8)], -mag, mag)
    return f * weight, np.full(8, weight, np.uint16)


def shell_field(dims, seed, unit):
    """(sum, weight) with weight 2 everywhere: a positive outer shell, random signs inside; unit or random magnitudes."""
    rng = np.random.default_rng(seed)
    nx, ny, nz = dims
    sign = np.where(rng.random((nz, ny, nx)) < 0.5, -1.0, 1.0)
    sign[[0, -1]] = sign[:, [0, -1]] = sign[:, :, [0, -1]] = 1.0
    f = sign * (1.0 if unit else rng.uniform(0.25, 1.0, (nz, ny, nx)))
    return (f * 2.0).reshape(-1), np.full(nx * ny * nz, 2, np.uint16)


SPHERE_CENTRE, SPHERE_RADIUS = (0.4873, 0.5219, 0.5102), 0.3
UNIT = ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))


def sphere_field(n):
    """(sum, weight 1) of the analytic distance to the sphere on the n^3 lattice of the unit cube."""
    lo, step = lattice(UNIT, (n, n, n))
    ax = [np.array([centre(lo, step, a, i) for i in range(n)]) for a in range(3)]
    Z, Y, X = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    c = SPHERE_CENTRE
    f = np.sqrt((X - c[0]) ** 2 + (Y - c[1]) ** 2 + (Z - c[2]) ** 2) - SPHERE_RADIUS
    return f.reshape(-1), np.ones(n * n * n, np.uint16)


# ------------------------------------------------------------------------------------------------ the welded mesh
def weld(tris):
    """(vertex count, {directed edge (a, b): times traversed}) of a soup welded by the bits of its vertices."""
    t = np.ascontiguousarray(tris, np.float32).reshape(-1, 3)
    _, idx = np.unique(t.view(np.uint32), axis=0, return_inverse=True)
    idx = idx.reshape(-1, 3)
    edges = {}
    for a, b, c in idx.tolist():
        for e in ((a, b), (b, c), (c, a)):
            edges[e] = edges.get(e, 0) + 1
    return int(idx.max()) + 1 if idx.size else 0, edges


def closed_and_oriented(tris):
    """Every welded edge is traversed exactly once in each direction."""
    _, edges = weld(tris)
    return all(n == 1 and edges.get((b, a), 0) == 1 for (a, b), n in edges.items())


def euler_characteristic(tris):
    nv, edges = weld(tris)
    return nv - len({(min(a, b), max(a, b)) for a, b in edges}) + len(tris)


def signed_volume(tris):
    t = np.asarray(tris, np.float64)
    return float((t[:, 0] * np.cross(t[:, 1], t[:, 2])).sum() / 6.0)


# ------------------------------------------------------------------------------------------------ end to end
def box_end_to_end(backend, tmp_path):
    """The drawn box, 12 views of 80 x 60, exact maps, lattice 48^3: shared with the GPU suite."""
    from curve_gaussian_amd.edge_extraction.reprojection import score_edges
    from curve_gaussian_amd.ops import edge_occlusion as EO
    from curve_gaussian_amd.ops import tsdf as TS
    from curve_gaussian_amd.ops.view_chunks import camera_arrays
    from curve_gaussian_amd.scene import solid_scan as SS
    scan = SS.solid_scan("box", 12, 60, 80, backend=backend)
    tris, info = TS.tsdf_mesh(list(scan.depth), scan.cameras, grid=48, backend=backend)
    assert len(tris) > 0 and info["triangles"] == len(tris) and info["dims"] == [48, 48, 48] and info["views"] == 12
    assert info["trunc"] == 4.0 / 48 and info["min_weight"] == 2 and info["observed"] > 0 and info["live_cells"] > 0
    assert info["recommended_slack"] == 2.0 * info["voxel_diagonal"] and abs(info["voxel_diagonal"] - np.sqrt(3.0) / 48) < 1e-12
    path = str(tmp_path / "tsdf_mesh.ply")
    EO.write_triangle_ply(path, tris)
    assert same_bits(EO.read_triangle_mesh(path), tris)
    occluder = EO.read_occluder(path)
    assert isinstance(occluder, np.ndarray) and same_bits(occluder, tris)          # a mesh, not surfels
    intr, w2c = camera_arrays(scan.cameras)
    drawn = EO.mesh_depth(tris, intr, w2c, 60, 80, window=0, backend=backend).cpu().numpy()
    both = np.isfinite(drawn) & np.isfinite(scan.depth)
    diff = np.abs(drawn[both].astype(np.float64) - scan.depth[both].astype(np.float64))
    figures = dict(pixels=int(both.sum()), median=float(np.median(diff)), p95=float(np.percentile(diff, 95)), max=float(diff.max()))
    print("tsdf box depth error:", json.dumps(figures), "bound", info["trunc"] + info["voxel_diagonal"])
    assert both.sum() > 0.5 * np.isfinite(scan.depth).sum()
    assert figures["p95"] <= info["trunc"] + info["voxel_diagonal"]
    # the options that --depth_dir users lacked, in one call (the host z-buffer of 30 000 triangles takes seconds a call)
    res = score_edges(scan.edges, scan.cameras, scan.maps, "PidiNet", backend=backend, occluder=path,
                      depth_slack=info["recommended_slack"], ignore_contours=True, near_clip=EO.NEAR_CLIP)
    assert res["settings"]["ignore_contours"] is True and res["settings"]["near_clip"] == EO.NEAR_CLIP
    assert res["settings"]["occluder"] == path and sum(r["hidden_points"] for r in res["views"]) > 0
    return tris, info, figures, scan
