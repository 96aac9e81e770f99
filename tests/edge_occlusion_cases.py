"""Shared inputs of the occlusion tests (test_edge_occlusion_cpu.py, test_edge_occlusion_gpu.py): brute-force float64
restatements of the frozen rules of include/curvegs.h (cgs_mesh_depth, cgs_depth_window_max, cgs_point_mask_depth), written
with Python floats one operation at a time and independently of the host back end of ops.edge_occlusion -- a per-pixel loop
over all triangles for the z-buffer, a per-(sample, view) loop for the gate --, and the cameras, triangle sets and samples
they run on."""
import functools
import math

import numpy as np

INF = float("inf")
HEIGHT = 5
WIDTHS = [1, 33, 67]
VIEWS = [1, 2, 5]
FACES = [0, 1, 2, 63, 64, 65, 257]
WINDOWS = [0, 1, 4]
POINT_COUNTS = [0, 1, 63, 64, 65, 4096]


# ------------------------------------------------------------------------------------------------ cameras
def cameras(V, H, W):
    """(intrinsics [V,4], w2c [V,3,4]) float64.  Camera 0 is the identity pose with fx = fy = 1, cx = cy = 0, so that
    u = X / Z and v = Y / Z exactly and a vertex can be put ON a pixel centre; the others look at the unit cube."""
    from curve_gaussian_amd import synthetic as S
    intr, w2c = [[1.0, 1.0, 0.0, 0.0]], [np.eye(4)[:3, :4]]
    for c in S.fibonacci_cameras(max(V - 1, 1), H, W)[:V - 1]:
        intr.append([W / (2 * math.tan(c.FoVx / 2)), H / (2 * math.tan(c.FoVy / 2)), W / 2.0, H / 2.0])
        w2c.append(c.world_view_transform.double().numpy().T[:3, :4])
    return np.array(intr, np.float64), np.array(w2c, np.float64)


# ------------------------------------------------------------------------------------------------ triangles
def _image_tri(uv, z):
    """A triangle of camera 0 with the image points uv [(u, v)] at the depth z (one number, or one per vertex)."""
    zs = [z] * 3 if np.isscalar(z) else list(z)
    return [[u * d, v * d, d] for (u, v), d in zip(uv, zs)]


SPECIAL = {   # name -> index into special_triangles()
    "zero_area": 0, "nan_vertex": 1, "all_behind": 2, "one_behind": 3, "off_screen": 4, "whole_image": 5, "shared_a": 6,
    "shared_b": 7, "stack_near_first": 8, "stack_far_second": 9, "stack_far_first": 10, "stack_near_second": 11,
    "vertex_on_centre": 12}
SHARED_DEPTH, STACK_NEAR, STACK_FAR, COVER_DEPTH, CENTRE_DEPTH = 4.0, 2.0, 3.0, 8.0, 1.5


def special_triangles():
    """float32 [13,3,3], in camera 0's image (every number below is exact in float32 and survives u = X / Z)."""
    nan = float("nan")
    t = [
        _image_tri([(0, 0), (1, 1), (2, 2)], 1.0),                                    # zero area
        [[nan, 0.0, 1.0], [1.0, 0.0, 1.0], [0.0, 1.0, 1.0]],                         # a NaN vertex
        _image_tri([(0, 0), (4, 0), (0, 4)], -1.0),                                   # all three behind the camera
        [[0.0, 0.0, 1.0], [4.0, 0.0, 1.0], [0.0, 4.0, -1.0]],                        # one behind: skipped, not clipped
        _image_tri([(-30, 0), (-20, 0), (-25, 4)], 1.0),                              # wholly off screen
        _image_tri([(-16, -16), (512, -16), (-16, 64)], COVER_DEPTH),                 # covers every image of the tests
        _image_tri([(0.5, 0.5), (4.5, 4.5), (4.5, 0.5)], SHARED_DEPTH),               # two sharing the side through the
        _image_tri([(0.5, 0.5), (0.5, 4.5), (4.5, 4.5)], SHARED_DEPTH),               # centres (0.5, 0.5) ... (4.5, 4.5)
        _image_tri([(6, 0), (10, 0), (8, 5)], STACK_NEAR),                            # stacked, the nearer first
        _image_tri([(6, 0), (10, 0), (8, 5)], STACK_FAR),
        _image_tri([(12, 0), (16, 0), (14, 5)], STACK_FAR),                           # stacked, the farther first
        _image_tri([(12, 0), (16, 0), (14, 5)], STACK_NEAR),
        _image_tri([(20.5, 2.5), (26, 0), (26, 5)], CENTRE_DEPTH),                    # a vertex exactly on a pixel centre
    ]
    return np.array(t, np.float32)


@functools.lru_cache(maxsize=None)
def _triangles(F, seed):
    rng = np.random.default_rng(seed)
    sp = special_triangles()
    n = max(F - len(sp), 0)
    small = rng.uniform(-0.3, 1.3, (n, 1, 3)) + rng.uniform(-0.25, 0.25, (n, 3, 3))       # around the unit cube
    z = rng.uniform(0.5, 6.0, (n, 3))
    wide = np.stack([rng.uniform(-8, 75, (n, 3)) * z, rng.uniform(-3, 8, (n, 3)) * z, z], 2)   # across camera 0's image
    rnd = np.where((np.arange(n) % 2 == 0)[:, None, None], small, wide).astype(np.float32)
    return np.concatenate([sp, rnd])[:F].copy()


def triangles(F, seed=5):
    """float32 [F,3,3]: the special triangles first (all of them from F = 63 on), then random ones -- small ones around the
    unit cube and ones that span camera 0's image with a different depth at every vertex."""
    return _triangles(F, seed).copy()


# ------------------------------------------------------------------------------------------------ brute force
def _project(K, M, X, Y, Z):
    """(c2, u, v) in Python floats, the operation order of cgs_project_points; u, v are None unless c2 > 0."""
    m = [float(x) for x in np.asarray(M, np.float64).reshape(12)]
    fx, fy, cx, cy = (float(x) for x in K)
    c0 = ((m[0] * X + m[1] * Y) + m[2] * Z) + m[3]
    c1 = ((m[4] * X + m[5] * Y) + m[6] * Z) + m[7]
    c2 = ((m[8] * X + m[9] * Y) + m[10] * Z) + m[11]
    if not c2 > 0.0:
        return c2, None, None
    return c2, fx * (c0 / c2) + cx, fy * (c1 / c2) + cy


def _clamped(fn, x, lo, hi):
    """min(max(fn(x), lo), hi) for fn = floor or ceil without converting a huge or infinite x."""
    return lo if x <= lo else hi if x >= hi else int(fn(x))


def _prepare(tri, K, M, H, W):
    """None for a skipped triangle, else (u, v, z, area, jlo, jhi, ilo, ihi)."""
    u, v, z = [], [], []
    for X, Y, Z in tri:
        c2, uu, vv = _project(K, M, float(X), float(Y), float(Z))
        if uu is None or uu != uu or vv != vv:
            return None
        u.append(uu), v.append(vv), z.append(c2)
    area = (u[1] - u[0]) * (v[2] - v[0]) - (v[1] - v[0]) * (u[2] - u[0])
    if area == 0.0 or area != area:
        return None
    return (u, v, z, area, _clamped(math.ceil, min(u) - 0.5, 0, W), _clamped(math.floor, max(u) - 0.5, -1, W - 1),
            _clamped(math.ceil, min(v) - 0.5, 0, H), _clamped(math.floor, max(v) - 0.5, -1, H - 1))


def zbuffer_brute(tris, K, M, H, W):
    """cgs_mesh_depth: float32 [V,H,W], pixel by pixel over ALL triangles."""
    tris = np.asarray(tris, np.float32).reshape(-1, 3, 3)
    out = np.full((len(K), H, W), np.inf, np.float32)
    for view in range(len(K)):
        prepared = [p for p in (_prepare(t, K[view], M[view], H, W) for t in tris) if p is not None]
        for i in range(H):
            for j in range(W):
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
                        continue   # 1 / invz is no positive finite float
                    with np.errstate(over="ignore"):
                        zf = np.float32(1.0 / invz)
                    if zf > 0 and np.isfinite(zf) and zf < best:
                        best = zf
                out[view, i, j] = best
    return out


def window_max_brute(depth, radius):
    d = np.asarray(depth, np.float32)
    V, H, W = d.shape
    out = np.empty_like(d)
    for v in range(V):
        for i in range(H):
            for j in range(W):
                out[v, i, j] = d[v, max(i - radius, 0):i + radius + 1, max(j - radius, 0):j + radius + 1].max()
    return out


def gate_brute(points, K, M, depth, slack):
    """cgs_point_mask_depth: (mask uint8 [V,H,W], kept int32 [V], hidden int32 [V]), sample by sample and view by view."""
    depth = np.asarray(depth, np.float32)
    V, H, W = depth.shape
    mask, kept, hidden = np.zeros((V, H, W), np.uint8), np.zeros(V, np.int32), np.zeros(V, np.int32)
    for view in range(V):
        for X, Y, Z in np.asarray(points, np.float32).reshape(-1, 3):
            c2, u, v = _project(K[view], M[view], float(X), float(Y), float(Z))
            if u is None or not (0.0 <= u < W and 0.0 <= v < H):
                continue
            i, j = int(math.floor(v)), int(math.floor(u))
            if c2 > float(depth[view, i, j]) + slack:
                hidden[view] += 1
            else:
                mask[view, i, j] = 1
                kept[view] += 1
    return mask, kept, hidden


# ------------------------------------------------------------------------------------------------ shared references
@functools.lru_cache(maxsize=None)
def reference_zbuffer(F, W, V):
    """The brute-force z-buffer of triangles(F) in cameras(V, HEIGHT, W): computed once, shared, read-only."""
    K, M = cameras(V, HEIGHT, W)
    out = zbuffer_brute(triangles(F), K, M, HEIGHT, W)
    out.setflags(write=False)
    return out


def samples(P, seed=3):
    """float32 [P,3]: points around the unit cube and along camera 0's axis, in front of and behind the test triangles."""
    rng = np.random.default_rng(seed)
    cube = rng.uniform(-0.4, 1.4, (P, 3))
    z = rng.uniform(0.2, 9.0, P)
    img = np.stack([rng.uniform(-2, 70, P) * z, rng.uniform(-1, 6, P) * z, z], 1)
    return np.where((np.arange(P) % 2 == 0)[:, None], cube, img).astype(np.float32)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
