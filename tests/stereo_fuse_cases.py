"""Inputs and brute-force restatements for the map-fusion tests (include/curvegs.h: cgs_stereo_warp, cgs_stereo_fuse),
shared by test_stereo_fuse_cpu.py and test_stereo_fuse_gpu.py.  The brute force is written from the header's text in
Python floats -- every target x slot x source pixel, every pixel x candidate x candidate, one operation a line -- and
shares no code with ops/stereo_depth.py."""
import math

import numpy as np

import stereo_cases as SC
from stereo_cases import _div, _f32, same_bits  # noqa: F401  (same_bits is re-exported to the tests)

INF = float("inf")


def _is_depth(x):
    """A positive finite float32, given as a Python float."""
    return x > 0.0 and math.isfinite(x)


# ------------------------------------------------------------------------------------------------ the brute force
def brute_warp(depth, K, fsrc, into, v0, nv):
    depth = np.asarray(depth, np.float32)
    V, H, W = depth.shape
    K = np.asarray(K, np.float64).tolist()
    fsrc = np.asarray(fsrc).tolist()
    F = len(fsrc[0])
    into = np.asarray(into, np.float64).reshape(V, F, 12).tolist()
    out = np.full((nv, F, H, W), np.inf, np.float32)
    for v in range(v0, v0 + nv):
        fxv, fyv, cxv, cyv = K[v]
        for s in range(F):
            w = fsrc[v][s]
            if not 0 <= w < V:
                continue
            fxw, fyw, cxw, cyw = K[w]
            M = into[v][s]
            for i in range(H):
                for j in range(W):
                    z = float(depth[w, i, j])
                    if not _is_depth(z):
                        continue
                    X = _div((j + 0.5) - cxw, fxw) * z
                    Y = _div((i + 0.5) - cyw, fyw) * z
                    c0 = ((M[0] * X + M[1] * Y) + M[2] * z) + M[3]
                    c1 = ((M[4] * X + M[5] * Y) + M[6] * z) + M[7]
                    c2 = ((M[8] * X + M[9] * Y) + M[10] * z) + M[11]
                    if not c2 > 0.0:
                        continue
                    u = fxv * _div(c0, c2) + cxv
                    vv = fyv * _div(c1, c2) + cyv
                    if not (0.0 <= u < W and 0.0 <= vv < H):
                        continue
                    zf = _f32(c2)
                    if not _is_depth(float(zf)):
                        continue
                    at = (v - v0, s, int(math.floor(vv)), int(math.floor(u)))
                    if zf < out[at]:
                        out[at] = zf
    return out


def brute_fuse(depth, warped, tol, min_support, v0):
    """(out float32 [nv,H,W], support uint8 [nv,H,W])."""
    depth, warped = np.asarray(depth, np.float32), np.asarray(warped, np.float32)
    nv, F, H, W = warped.shape
    tol = np.asarray(tol, np.float64).tolist()
    out, sup = np.zeros((nv, H, W), np.float32), np.zeros((nv, H, W), np.uint8)
    for t in range(nv):
        v = v0 + t
        for i in range(H):
            for j in range(W):
                values = [float(depth[v, i, j])] + [float(warped[t, s, i, j]) for s in range(F)]
                q = [_div(1.0, x) if _is_depth(x) else None for x in values]
                best, support_best, q_best = None, None, None
                for k in range(F + 1):
                    if q[k] is None:
                        continue
                    support_k = 0
                    for m in range(F + 1):
                        if q[m] is not None and abs(q[m] - q[k]) <= tol[v]:
                            support_k += 1
                    if best is None or support_k > support_best or (support_k == support_best and q[k] < q_best):
                        best, support_best, q_best = k, support_k, q[k]
                if best is None or support_best < min_support:
                    continue
                total, count = 0.0, 0
                for m in range(F + 1):
                    if q[m] is not None and abs(q[m] - q_best) <= tol[v]:
                        total = total + q[m]
                        count += 1
                mean = total / float(count)
                out[t, i, j] = _f32(_div(1.0, mean))
                sup[t, i, j] = count
    return out, sup


# ------------------------------------------------------------------------------------------------ inputs
def into_pose(R_w, T_w, R_v, T_v):
    """[R | T] taking the SOURCE w's camera coordinates to the TARGET v's."""
    Rel = R_v @ R_w.T
    return np.concatenate([Rel, (T_v - Rel @ T_w)[:, None]], 1).reshape(12)


def random_case(V, H, W, F, seed, spoil=True):
    """V views looking along +z with small turns and sideways shifts at the world plane z = 2: every map holds the plane's
    depth with a little noise, holes (0), a few outliers and -- when ``spoil`` -- a NaN, an infinity and a negative depth.
    fsrc: target v's sources are the next views in turn, with a -1 pad in the middle of the row and one index >= V behind
    the sources where F allows."""
    rng = np.random.default_rng(2000 + seed)
    K = np.array([[1.3 * W + 0.1 * v, 1.2 * W - 0.2 * v, 0.5 * W + 0.3, 0.5 * H - 0.2] for v in range(V)], np.float64)
    Rs = [SC._rot(*rng.uniform(-0.02, 0.02, 3)) for _ in range(V)]
    Ts = [np.array([0.05 * v, 0.01 * v, 0.0]) + rng.uniform(-0.01, 0.01, 3) for v in range(V)]
    depth = np.zeros((V, H, W), np.float32)
    for v in range(V):
        d = np.stack(np.broadcast_arrays(((np.arange(W) + 0.5 - K[v][2]) / K[v][0])[None, :],
                                         ((np.arange(H) + 0.5 - K[v][3]) / K[v][1])[:, None], np.ones((H, W))), -1)
        z = (2.0 + (Rs[v].T @ Ts[v])[2]) / (d @ Rs[v])[..., 2]          # the ray z * d meets the world plane z = 2
        depth[v] = (z * (1.0 + rng.normal(0.0, 0.002, (H, W)))).astype(np.float32)
    depth[rng.random((V, H, W)) < 0.25] = 0.0
    wild = rng.random((V, H, W)) < 0.1
    depth[wild] = rng.uniform(1.0, 4.0, int(wild.sum())).astype(np.float32)
    if spoil:
        flat = depth.reshape(V, -1)
        flat[0, 0] = np.nan
        if H * W > 2:
            flat[0, 1], flat[0, 2] = -1.0, np.inf
    fsrc, into = np.full((V, F), -1, np.int32), np.zeros((V, F, 12), np.float64)
    for v in range(V):
        slots = list(range(F))
        if F >= 2:
            slots.pop(F // 2)
        others = [(v + k) % V for k in range(1, V)]
        for s, w in zip(slots, others):
            fsrc[v, s] = w
            into[v, s] = into_pose(Rs[w], Ts[w], Rs[v], Ts[v])
        if len(slots) > len(others):
            fsrc[v, slots[len(others)]] = V + 2
    return dict(depth=depth, K=K, fsrc=fsrc, into=into, tol=np.full((V,), 0.01) + 0.001 * np.arange(V))


def ranges(V):
    """(v0, nv): all, all but the first, the last alone, none."""
    return sorted({(0, V), (1, V - 1), (V - 1, 1), (0, 0)})


def exact_case(H=6, W=10, zs=(2.0, 2.0, 2.0)):
    """``stereo_cases.consistency_case`` for the fusion: three views shifted by 4 along x, maps constant at depth 2 -> source
    w's pixel at column c lands on column c + 2 (v - w) of target v at depth 2, all exact."""
    c = SC.consistency_case(3, H, W, zs)
    into = np.zeros((3, 2, 12))
    for v in range(3):
        for s, w in enumerate(c["src"][v].tolist()):
            into[v, s] = np.concatenate([np.eye(3), np.array([[(v - w) * 4.0], [0.0], [0.0]])], 1).reshape(12)
    return dict(depth=c["depth"], K=c["K"], fsrc=c["src"], into=into, tol=c["tol"])


def two_views(depth_row, T, W=None):
    """View 1 warped into view 0: fx = fy = 1, cx = cy = 0, no rotation, into = [I | T]; view 1 holds ``depth_row`` in its
    one row, view 0 nothing."""
    row = np.asarray(depth_row, np.float32)
    depth = np.stack([np.zeros_like(row), row])[:, None, :]
    into = np.zeros((2, 1, 12))
    into[0, 0] = np.concatenate([np.eye(3), np.asarray(T, np.float64)[:, None]], 1).reshape(12)
    return dict(depth=depth, K=np.tile(np.array([1.0, 1.0, 0.0, 0.0]), (2, 1)), fsrc=np.array([[1], [-1]], np.int32), into=into,
                tol=np.zeros(2))


def crowded_case(V=3, H=24, W=32, F=3, seed=9):
    """Sources much farther from the scene than the target sees them: every into pushes the points 10 units away, so a
    whole map shrinks onto a few target pixels and many source pixels collide on each."""
    c = random_case(V, H, W, F, seed, spoil=False)
    c["depth"] = np.random.default_rng(seed).uniform(1.5, 2.5, c["depth"].shape).astype(np.float32)
    c["into"] = c["into"].copy()
    c["into"][:, :, 11] += 10.0
    return c


def pixel_case(own, others, tol):
    """One target pixel by hand: depth [1,1,1], warped [1,F,1,1], tol [1]."""
    return (np.array(own, np.float32).reshape(1, 1, 1), np.array(others, np.float32).reshape(1, -1, 1, 1),
            np.array([tol], np.float64))
