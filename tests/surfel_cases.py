"""Shared inputs of the surfel z-buffer tests (test_surfel_depth_cpu.py, test_surfel_depth_gpu.py): a brute-force float64
restatement of the frozen rule of cgs_surfel_depth (include/curvegs.h), written with Python floats one operation at a time
and independently of the host back end of ops.edge_occlusion -- every pixel x every surfel, the candidates test included
--, the cameras, the named special surfels (one per branch of the rule), the mixed clouds of the wave-shape tests and the
sampled solids of the gate comparison."""
import functools
import math

import numpy as np

INF, NAN = float("inf"), float("nan")
SIZES = [(1, 1), (5, 7), (24, 32)]      # (height, width)
VIEWS = 3
FOCAL0 = 64.0                           # camera 0: identity pose, fx = fy = 64, cx = cy = 0 -- u = 64 X / Z exactly
WAVE_COUNTS = [1, 63, 64, 65, 257]      # surfels: one, and around 64 and 256 (workgroups of 4 surfels: full, and one surfel in the last)
WAVE_SIZE = (33, 65)


# ------------------------------------------------------------------------------------------------ cameras
def cameras(V, H, W):
    """(intrinsics [V,4], w2c [V,3,4]) float64.  Camera 0 is the identity pose with fx = fy = FOCAL0 and cx = cy = 0, so that
    a surfel can be put ON a pixel centre or a pixel corner exactly; the others look at the unit cube."""
    from curve_gaussian_amd import synthetic as S
    intr, w2c = [[FOCAL0, FOCAL0, 0.0, 0.0]], [np.eye(4)[:3, :4]]
    for c in S.fibonacci_cameras(max(V - 1, 1), H, W)[:V - 1]:
        intr.append([W / (2 * math.tan(c.FoVx / 2)), H / (2 * math.tan(c.FoVy / 2)), W / 2.0, H / 2.0])
        w2c.append(c.world_view_transform.double().numpy().T[:3, :4])
    return np.array(intr[:V], np.float64).reshape(-1, 4), np.array(w2c[:V], np.float64).reshape(-1, 3, 4)


# ------------------------------------------------------------------------------------------------ special surfels
def _at(u, v, z):
    """The point of camera 0 that projects to the image point (u, v) at depth z (exact for the numbers used below)."""
    return [u / FOCAL0 * z, v / FOCAL0 * z, z]


def _px(r_px, z):
    """The world radius that spans r_px pixels at depth z in camera 0."""
    return r_px / FOCAL0 * z


# name -> (point, normal, radius), in camera 0's image.  Depths are powers of two and image points multiples of 1/2, so the
# float32 inputs hold the intended numbers exactly.
SPECIAL = {
    "facing":          (_at(10.5, 8.5, 2.0), [0.0, 0.0, -1.0], _px(3.0, 2.0)),
    "from_behind":     (_at(20.5, 8.5, 2.0), [0.0, 0.0, 1.0], _px(3.0, 2.0)),           # the same bits as facing, shifted
    "tilted":          (_at(10.5, 16.5, 2.0), [1.0, 0.0, -1.0], _px(4.0, 2.0)),
    "grazing":         (_at(2.75, 3.5, 2.0), [1.0, 0.0, -2.5 / FOCAL0], _px(3.0, 2.0)),  # den == 0 exactly at j = 2
    "centre_behind":   (_at(10.5, 8.5, -2.0), [0.0, 0.0, 1.0], _px(3.0, 2.0)),
    "touches_plane":   (_at(16.5, 16.5, 2.0), [0.0, 0.0, 1.0], 2.0),                     # c2 - r == 0: skipped
    "just_in_front":   (_at(16.5, 16.5, 2.0), [1.0, 1.0, 1.0], float(np.nextafter(np.float32(2.0), np.float32(0.0)))),
    "over_left":       (_at(0.0, 10.5, 4.0), [0.0, 0.0, 1.0], _px(2.25, 4.0)),
    "over_right":      (_at(32.0, 10.5, 4.0), [0.0, 0.0, 1.0], _px(2.25, 4.0)),
    "over_top":        (_at(14.5, 0.0, 4.0), [0.0, 0.0, 1.0], _px(2.25, 4.0)),
    "over_bottom":     (_at(14.5, 24.0, 4.0), [0.0, 0.0, 1.0], _px(2.25, 4.0)),
    "sub_pixel_none":  (_at(26.0, 4.0, 1.0), [0.0, 0.0, 1.0], _px(0.25, 1.0)),           # on a pixel corner: no centre
    "sub_pixel_one":   (_at(28.5, 4.5, 1.0), [0.0, 0.0, 1.0], _px(0.25, 1.0)),           # on a pixel centre: that one
    "whole_image":     (_at(16.0, 12.0, 8.0), [0.0, 0.0, 1.0], _px(40.0, 8.0)),           # r = 5 < c2 = 8
    "radius_zero":     (_at(5.5, 20.5, 2.0), [0.0, 0.0, 1.0], 0.0),
    "radius_negative": (_at(5.5, 20.5, 2.0), [0.0, 0.0, 1.0], -_px(3.0, 2.0)),
    "radius_nan":      (_at(5.5, 20.5, 2.0), [0.0, 0.0, 1.0], NAN),
    "radius_inf":      (_at(5.5, 20.5, 2.0), [0.0, 0.0, 1.0], INF),
    "nan_coordinate":  ([NAN, 0.25, 2.0], [0.0, 0.0, 1.0], _px(3.0, 2.0)),
    "nan_normal":      (_at(5.5, 20.5, 2.0), [0.0, NAN, 1.0], _px(3.0, 2.0)),
    "zero_normal":     (_at(5.5, 20.5, 2.0), [0.0, 0.0, 0.0], _px(3.0, 2.0)),
    "unit_normal":     (_at(5.5, 12.5, 2.0), [0.0, 0.6, -0.8], _px(3.0, 2.0)),
    "long_normal":     (_at(25.5, 12.5, 2.0), [0.0, 4.2, -5.6], _px(3.0, 2.0)),          # 7 x unit_normal, 20 pixels along
    "coincident_a":    (_at(22.5, 20.5, 2.0), [0.0, 1.0, -1.0], _px(2.0, 2.0)),
    "coincident_b":    (_at(22.5, 20.5, 2.0), [0.0, 1.0, -1.0], _px(2.0, 2.0)),
    "in_front_of_all": (_at(16.0, 12.0, 1.0), [0.0, 0.0, 1.0], _px(1.75, 1.0)),          # nearer than whole_image: wins
}
STORES_NOTHING = ("grazing", "centre_behind", "touches_plane", "sub_pixel_none", "radius_zero", "radius_negative",
                  "radius_nan", "radius_inf", "nan_coordinate", "nan_normal", "zero_normal")


def special(names=None, normals=True):
    """(points float32 [P,3], normals float32 [P,3] or None, radii float32 [P]) of the named special surfels (all)."""
    rows = [SPECIAL[n] for n in (SPECIAL if names is None else names)]
    pts = np.array([r[0] for r in rows], np.float32).reshape(-1, 3)
    nrm = np.array([r[1] for r in rows], np.float32).reshape(-1, 3) if normals else None
    return pts, nrm, np.array([r[2] for r in rows], np.float32).reshape(-1)


@functools.lru_cache(maxsize=None)
def _wave_cloud(P, seed):
    rng = np.random.default_rng(seed)
    H, W = WAVE_SIZE
    z = rng.uniform(1.0, 6.0, P)
    pts = np.stack([rng.uniform(-2, W + 2, P) / FOCAL0 * z, rng.uniform(-2, H + 2, P) / FOCAL0 * z, z], 1)
    cube = rng.uniform(0.1, 0.9, (P, 3))
    pts = np.where((np.arange(P) % 3 == 2)[:, None], cube, pts)
    nrm = rng.normal(0, 1, (P, 3))
    k = np.arange(P)
    large = (k % 7 == 3) | (k == P - 1)
    large &= ~((k >= 64) & (k < 128))                       # the second wave has no large disk
    if P - 1 >= 64 and P - 1 < 128:
        large[P - 1] = True                                 # ... unless it is the last, partial one
    r_px = np.where(large, rng.uniform(6.0, 30.0, P), np.exp(rng.uniform(np.log(0.2), np.log(4.5), P)))
    rad = r_px / FOCAL0 * z
    rad = np.where((np.arange(P) % 3 == 2), r_px / 33.0 * 0.4, rad)   # the cube's: the other cameras see them about as large
    return pts.astype(np.float32), nrm.astype(np.float32), rad.astype(np.float32)


def wave_cloud(P, seed=11):
    """(points, normals, radii) of P surfels across WAVE_SIZE images: disks of a fraction of a pixel up to 30 pixels mixed
    inside every wave (every 7th surfel and the last are large), except the second wave of 64, which has small ones only."""
    return tuple(a.copy() for a in _wave_cloud(P, seed))


# ------------------------------------------------------------------------------------------------ brute force
def _div(a, b):
    """IEEE a / b for Python floats."""
    try:
        return a / b
    except ZeroDivisionError:
        if a != a or a == 0.0:
            return NAN
        return math.copysign(INF, a) * math.copysign(1.0, b)


def _fmin(a, b):
    return b if a != a else a if b != b else min(a, b)


def _fmax(a, b):
    return b if a != a else a if b != b else max(a, b)


def _clamped(fn, x, lo, hi):
    """min(max(fn(x), lo), hi) for fn = floor or ceil without converting a huge or infinite x."""
    return lo if x <= lo else hi if x >= hi else int(fn(x))


def _prepare(p, n, r, K, M, H, W):
    """None for a surfel the view skips, else (c0, c1, c2, n0, n1, n2, num, r2, jlo, jhi, ilo, ihi)."""
    m = [float(x) for x in np.asarray(M, np.float64).reshape(12)]
    fx, fy, cx, cy = (float(x) for x in K)
    X, Y, Z = (float(x) for x in p)
    c0 = ((m[0] * X + m[1] * Y) + m[2] * Z) + m[3]
    c1 = ((m[4] * X + m[5] * Y) + m[6] * Z) + m[7]
    c2 = ((m[8] * X + m[9] * Y) + m[10] * Z) + m[11]
    if n is None:
        n0, n1, n2 = 0.0, 0.0, 1.0
    else:
        A, B, C = (float(x) for x in n)
        n0 = (m[0] * A + m[1] * B) + m[2] * C
        n1 = (m[4] * A + m[5] * B) + m[6] * C
        n2 = (m[8] * A + m[9] * B) + m[10] * C
    r = float(r)
    if not r > 0.0 or not c2 - r > 0.0:
        return None
    zlo, zhi = c2 - r, c2 + r
    a, b = c0 - r, c0 + r
    ulo = fx * _fmin(_div(a, zlo), _div(a, zhi)) + cx
    uhi = fx * _fmax(_div(b, zlo), _div(b, zhi)) + cx
    a, b = c1 - r, c1 + r
    vlo = fy * _fmin(_div(a, zlo), _div(a, zhi)) + cy
    vhi = fy * _fmax(_div(b, zlo), _div(b, zhi)) + cy
    if ulo != ulo or uhi != uhi or vlo != vlo or vhi != vhi:
        return None
    num = (n0 * c0 + n1 * c1) + n2 * c2
    return (c0, c1, c2, n0, n1, n2, num, r * r, _clamped(math.ceil, ulo - 0.5, 0, W), _clamped(math.floor, uhi - 0.5, -1, W - 1),
            _clamped(math.ceil, vlo - 0.5, 0, H), _clamped(math.floor, vhi - 0.5, -1, H - 1))


def zbuffer_brute(points, normals, radii, K, M, H, W):
    """cgs_surfel_depth: float32 [V,H,W], pixel by pixel over ALL surfels."""
    points = np.asarray(points, np.float32).reshape(-1, 3)
    out = np.full((len(K), H, W), np.inf, np.float32)
    for view in range(len(K)):
        fx, fy, cx, cy = (float(x) for x in K[view])
        prepared = [q for q in (_prepare(points[k], None if normals is None else normals[k], radii[k], K[view], M[view], H, W)
                                for k in range(len(points))) if q is not None]
        for i in range(H):
            for j in range(W):
                px, py = j + 0.5, i + 0.5
                dx, dy = _div(px - cx, fx), _div(py - cy, fy)
                best = np.float32(np.inf)
                for c0, c1, c2, n0, n1, n2, num, r2, jlo, jhi, ilo, ihi in prepared:
                    if not (jlo <= j <= jhi and ilo <= i <= ihi):
                        continue
                    den = (n0 * dx + n1 * dy) + n2
                    s = _div(num, den)
                    qx, qy, qz = s * dx - c0, s * dy - c1, s - c2
                    d2 = (qx * qx + qy * qy) + qz * qz
                    if not d2 <= r2:
                        continue
                    with np.errstate(over="ignore"):
                        zf = np.float32(s)
                    if zf > 0 and np.isfinite(zf) and zf < best:
                        best = zf
                out[view, i, j] = best
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------------------ the sampled solids
GATE_VIEWS, GATE_SIZE, GATE_SPACING = 6, (60, 80), 0.01


@functools.lru_cache(maxsize=None)
def gate_fixture(shape):
    """The comparison of the surfel gate with the mesh gate on one solid, host back ends, computed once and shared: a dict
    with the solid's triangles, cameras (K, M), the ground-truth samples, the cloud (points, normals, radii -- derived with
    the shipped factor), the plain z-buffers of both and, per (sample, view), seen / hidden by the mesh / hidden by the cloud."""
    from curve_gaussian_amd.edge_extraction.abc import pred_points_and_directions
    from curve_gaussian_amd.ops import edge_occlusion as EO
    from curve_gaussian_amd.ops.view_chunks import camera_arrays
    from curve_gaussian_amd.scene import solid_scan as SS
    from curve_gaussian_amd import synthetic
    H, W = GATE_SIZE
    tris, edges = SS.solid_geometry(shape)
    K, M = camera_arrays(SS.emap_cameras_of(synthetic.fibonacci_cameras(GATE_VIEWS, H, W)))
    pts, nrm = SS.surfel_cloud(tris, GATE_SPACING)
    rad = EO.surfel_radii(pts, backend="host")
    samples = np.ascontiguousarray(pred_points_and_directions(edges, SS.SAMPLE_RESOLUTION).points, np.float32).reshape(-1, 3)
    raw_mesh = EO.mesh_depth(tris, K, M, H, W, window=0, backend="host").numpy()
    raw_cloud = EO.surfel_depth(EO.Surfels(pts, nrm, rad), K, M, H, W, window=0, backend="host").numpy()
    out = {"tris": tris, "edges": edges, "K": K, "M": M, "samples": samples, "cloud": (pts, nrm, rad), "raw_mesh": raw_mesh,
           "raw_cloud": raw_cloud}
    Md = np.asarray(M, np.float64).reshape(len(K), 12)
    for name, raw in (("mesh", raw_mesh), ("cloud", raw_cloud)):
        planes = EO.depth_window_max(raw, EO.DEPTH_WINDOW, backend="host").numpy()
        seen, hid = [], []
        for v in range(len(K)):
            _, _, s, h = EO.gate_view_host(samples, K[v], Md[v], planes[v], EO.DEPTH_SLACK)
            seen.append(s | h), hid.append(h)
        out["seen"], out["hidden_" + name] = np.stack(seen), np.stack(hid)
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out
