"""Inputs and brute-force restatements for the plane-sweep stereo tests (include/curvegs.h: cgs_stereo_sweep,
cgs_stereo_consistency), shared by test_stereo_depth_cpu.py and test_stereo_depth_gpu.py.  The brute force is written from
the header's text in Python floats -- every pixel x hypothesis x source x tap, one operation a line -- and shares no code
with ops/stereo_depth.py."""
import math

import numpy as np

INF = float("inf")


# ------------------------------------------------------------------------------------------------ IEEE helpers
def _div(a, b):
    try:
        return a / b
    except ZeroDivisionError:
        with np.errstate(all="ignore"):
            return float(np.float64(a) / np.float64(b))


def _floor(x):
    return float(math.floor(x)) if math.isfinite(x) else x


def _f32(x):
    with np.errstate(all="ignore"):
        return np.float32(x)


# ------------------------------------------------------------------------------------------------ the brute force
def brute_sweep(gray, K, inv, src, rel, R, min_var, max_cost, min_sources, trace=None):
    """float32 [V,H,W].  ``trace``: a dict that receives {(v, i, j): (best, costs)} of every pixel that reaches the sweep."""
    g = np.asarray(gray).astype(np.float64).tolist()
    V, H, W = np.asarray(gray).shape
    K, inv, rel = np.asarray(K, np.float64).tolist(), np.asarray(inv, np.float64).tolist(), np.asarray(rel, np.float64)
    rel = rel.reshape(V, -1, 12).tolist()
    src = np.asarray(src).tolist()
    D, S = len(inv[0]) if V else 0, len(src[0]) if V else 0
    n = float((2 * R + 1) * (2 * R + 1))
    thr = (min_var * n) * n
    out = np.zeros((V, H, W), np.float32)
    taps = [(di, dj) for di in range(-R, R + 1) for dj in range(-R, R + 1)]
    for v in range(V):
        fx, fy, cx, cy = K[v]
        for i in range(H):
            for j in range(W):
                if not (i - R >= 0 and i + R <= H - 1 and j - R >= 0 and j + R <= W - 1):
                    continue
                sr = srr = 0.0
                for di, dj in taps:
                    r = g[v][i + di][j + dj]
                    sr = sr + r
                    srr = srr + r * r
                var_r = n * srr - sr * sr
                if not var_r > thr:
                    continue
                cost = []
                for d in range(D):
                    z = _div(1.0, inv[v][d])
                    total, count = 0.0, 0
                    for s in range(S):
                        w = src[v][s]
                        if not 0 <= w < V:
                            continue
                        M = rel[v][s]
                        fxs, fys, cxs, cys = K[w]
                        ss = sss = srs = 0.0
                        valid = True
                        for di, dj in taps:
                            px = (j + dj) + 0.5
                            py = (i + di) + 0.5
                            X = _div(px - cx, fx) * z
                            Y = _div(py - cy, fy) * z
                            c0 = ((M[0] * X + M[1] * Y) + M[2] * z) + M[3]
                            c1 = ((M[4] * X + M[5] * Y) + M[6] * z) + M[7]
                            c2 = ((M[8] * X + M[9] * Y) + M[10] * z) + M[11]
                            if not c2 > 0.0:
                                valid = False
                                break
                            u = fxs * _div(c0, c2) + cxs
                            vv = fys * _div(c1, c2) + cys
                            x = u - 0.5
                            y = vv - 0.5
                            x0 = _floor(x)
                            y0 = _floor(y)
                            if not (0.0 <= x0 and x0 + 1.0 <= W - 1 and 0.0 <= y0 and y0 + 1.0 <= H - 1):
                                valid = False
                                break
                            a = x - x0
                            b = y - y0
                            xi, yi = int(x0), int(y0)
                            g00, g01, g10, g11 = g[w][yi][xi], g[w][yi][xi + 1], g[w][yi + 1][xi], g[w][yi + 1][xi + 1]
                            top = g00 * (1.0 - a) + g01 * a
                            bot = g10 * (1.0 - a) + g11 * a
                            val = top * (1.0 - b) + bot * b
                            ss = ss + val
                            sss = sss + val * val
                            srs = srs + g[v][i + di][j + dj] * val
                        if not valid:
                            continue
                        var_s = n * sss - ss * ss
                        if not var_s > thr:
                            continue
                        cov = n * srs - sr * ss
                        score = _div(cov * abs(cov), var_r * var_s)
                        total = total + (1.0 - score)
                        count += 1
                    cost.append(total / float(count) if count >= min_sources else INF)
                best = 0
                for d in range(1, D):
                    if cost[d] < cost[best]:
                        best = d
                if trace is not None:
                    trace[(v, i, j)] = (best, list(cost))
                cb = cost[best]
                if not (math.isfinite(cb) and cb <= max_cost):
                    continue
                o = 0.0
                if 0 < best < D - 1:
                    cm, cp = cost[best - 1], cost[best + 1]
                    if math.isfinite(cm) and math.isfinite(cp):
                        den = (cm - 2.0 * cb) + cp
                        if den > 0.0:
                            o = _div(0.5 * (cm - cp), den)
                            o = min(max(o, -0.5), 0.5)
                q = inv[v][best]
                if o != 0.0:
                    q = inv[v][best] + o * ((inv[v][best + 1] - inv[v][best]) if o >= 0.0 else (inv[v][best] - inv[v][best - 1]))
                out[v, i, j] = _f32(_div(1.0, q))
    return out


def brute_consistency(depth, K, src, rel, tol, min_consistent):
    depth = np.asarray(depth, np.float32)
    V, H, W = depth.shape
    K, tol = np.asarray(K, np.float64).tolist(), np.asarray(tol, np.float64).tolist()
    rel = np.asarray(rel, np.float64).reshape(V, -1, 12).tolist()
    src = np.asarray(src).tolist()
    out = np.zeros((V, H, W), np.float32)
    for v in range(V):
        fx, fy, cx, cy = K[v]
        for i in range(H):
            for j in range(W):
                z = float(depth[v, i, j])
                if not z > 0.0:
                    continue
                X = _div((j + 0.5) - cx, fx) * z
                Y = _div((i + 0.5) - cy, fy) * z
                agree = 0
                for s in range(len(src[v])):
                    w = src[v][s]
                    if not 0 <= w < V:
                        continue
                    M = rel[v][s]
                    fxs, fys, cxs, cys = K[w]
                    c0 = ((M[0] * X + M[1] * Y) + M[2] * z) + M[3]
                    c1 = ((M[4] * X + M[5] * Y) + M[6] * z) + M[7]
                    c2 = ((M[8] * X + M[9] * Y) + M[10] * z) + M[11]
                    if not c2 > 0.0:
                        continue
                    u = fxs * _div(c0, c2) + cxs
                    vv = fys * _div(c1, c2) + cys
                    if not (0.0 <= u < W and 0.0 <= vv < H):
                        continue
                    ds = float(depth[w, int(math.floor(vv)), int(math.floor(u))])
                    if not ds > 0.0:
                        continue
                    if abs(_div(1.0, ds) - _div(1.0, c2)) <= tol[v]:
                        agree += 1
                if agree >= min_consistent:
                    out[v, i, j] = depth[v, i, j]
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and bool((a.view(np.uint32) == b.view(np.uint32)).all())


# ------------------------------------------------------------------------------------------------ inputs
def texture(V, H, W, seed):
    """uint8 [V,H,W]: one smooth random surface seen with small shifts, so that patches correlate between the views, plus
    a little noise, so that nothing is exact."""
    rng = np.random.default_rng(seed)
    coarse = rng.uniform(30.0, 225.0, (H // 3 + 4, W // 3 + 6))
    ys, xs = np.arange(H) / 3.0, np.arange(W) / 3.0
    out = np.zeros((V, H, W), np.uint8)
    for v in range(V):
        x = xs + 0.4 * v + 1.0
        y0, x0 = np.floor(ys).astype(int), np.floor(x).astype(int)
        b, a = (ys - y0)[:, None], (x - x0)[None, :]
        val = (coarse[y0][:, x0] * (1 - a) + coarse[y0][:, x0 + 1] * a) * (1 - b) \
            + (coarse[y0 + 1][:, x0] * (1 - a) + coarse[y0 + 1][:, x0 + 1] * a) * b
        out[v] = np.clip(np.rint(val + rng.normal(0.0, 2.0, (H, W))), 0, 255).astype(np.uint8)
    return out


def _rot(ax, ay, az):
    cx, sx, cy, sy, cz, sz = math.cos(ax), math.sin(ax), math.cos(ay), math.sin(ay), math.cos(az), math.sin(az)
    Rx = np.array([[1, 0, 0], [0, cx, -sx], [0, sx, cx]])
    Ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    Rz = np.array([[cz, -sz, 0], [sz, cz, 0], [0, 0, 1]])
    return Rz @ Ry @ Rx


def random_case(V, H, W, D, S, R, seed, pads=True):
    """A group of V views looking along +z at depths around 2 with small turns and sideways shifts.  src: view v's sources
    are the next views in turn, with a -1 pad in the middle of every row when ``pads`` and S allows."""
    rng = np.random.default_rng(1000 + seed)
    K = np.array([[1.3 * W + 0.1 * v, 1.2 * W - 0.2 * v, 0.5 * W + 0.3, 0.5 * H - 0.2] for v in range(V)], np.float64)
    Rs = [_rot(*rng.uniform(-0.02, 0.02, 3)) for _ in range(V)]
    Ts = [np.array([0.05 * v, 0.01 * v, 0.0]) + rng.uniform(-0.01, 0.01, 3) for v in range(V)]
    inv = np.stack([np.linspace(1.0 / (1.2 + 0.01 * v), 1.0 / 3.5, D) if D > 1 else np.array([0.5 + 0.01 * v])
                    for v in range(V)])
    src, rel = np.full((V, S), -1, np.int32), np.zeros((V, S, 12), np.float64)
    others = lambda v: [(v + k) % V for k in range(1, V)]
    for v in range(V):
        slots = list(range(S))
        if pads and S >= 2:
            slots.pop(S // 2)
        for s, w in zip(slots, others(v)):
            Rel = Rs[w] @ Rs[v].T
            src[v, s] = w
            rel[v, s] = np.concatenate([Rel, (Ts[w] - Rel @ Ts[v])[:, None]], 1).reshape(12)
    return dict(gray=texture(V, H, W, seed), K=K, inv=inv, src=src, rel=rel, R=R, min_var=1.0, max_cost=1.5, min_sources=1)


def exact_case(H=12, W=20, inv=(0.5, 0.25), t=8.0, V=2, seed=3):
    """Arithmetic without rounding: fx = fy = 1, cx = cy = 0, identity rotations, view w shifted by w * t along x, inverse
    depths that are powers of two.  A tap at column c of view v lands at column c + (w - v) * t * inv exactly (a = b = 0)."""
    rng = np.random.default_rng(seed)
    gray = rng.integers(0, 256, (V, H, W)).astype(np.uint8)
    K = np.tile(np.array([1.0, 1.0, 0.0, 0.0]), (V, 1))
    src, rel = np.full((V, max(V - 1, 1)), -1, np.int32), np.zeros((V, max(V - 1, 1), 12))
    for v in range(V):
        for s, w in enumerate([w for w in range(V) if w != v]):
            src[v, s] = w
            rel[v, s] = np.concatenate([np.eye(3), np.array([[(w - v) * t], [0.0], [0.0]])], 1).reshape(12)
    return dict(gray=gray, K=K, inv=np.tile(np.asarray(inv, np.float64), (V, 1)), src=src, rel=rel, R=1, min_var=0.0,
                max_cost=0.5, min_sources=1)


def shifted_views(base, shifts):
    """uint8 [V,H,W]: view w holds ``base`` moved right by shifts[w] columns (wrapped around)."""
    return np.stack([np.roll(base, int(s), axis=1) for s in shifts]).astype(np.uint8)


def sweep_args(case):
    return (case["gray"], case["K"], case["inv"], case["src"], case["rel"], case["R"], case["min_var"], case["max_cost"],
            case["min_sources"])


# ------------------------------------------------------------------------------------------------ the named cases
def named_cases():
    """name -> (case, check) where check(out float32 [V,H,W]) asserts what the case is about.  Every case is also held to
    the brute force bit for bit by the tests."""
    cases = {}
    rng = np.random.default_rng(11)

    # a patch over each border: the frame of width R stores 0, the inside stores something
    c = random_case(3, 9, 11, 4, 3, 1, 21)

    def check_border(out, R=1):
        assert not out[:, :R].any() and not out[:, -R:].any() and not out[:, :, :R].any() and not out[:, :, -R:].any()
        assert (out[:, R:-R, R:-R] > 0).any()
    cases["border"] = (c, check_border)

    # a flat reference patch: var_r == 0 everywhere in view 0
    c = random_case(3, 9, 11, 4, 3, 1, 22)
    c["gray"] = c["gray"].copy()
    c["gray"][0] = 77
    c["min_var"] = 0.0

    def check_flat_reference(out):
        assert not out[0].any()
    cases["flat_reference"] = (c, check_flat_reference)

    # a flat source patch: view 0's only source is constant
    c = random_case(2, 9, 11, 4, 1, 1, 23)
    c["gray"] = c["gray"].copy()
    c["gray"][1] = 200
    c["min_var"] = 0.0

    def check_flat_source(out):
        assert not out[0].any()
    cases["flat_source"] = (c, check_flat_source)

    # a source behind the camera: the relative pose turns the scene behind the source (c2 < 0 at every tap)
    c = random_case(2, 9, 11, 4, 1, 1, 24)
    c["rel"] = c["rel"].copy()
    c["rel"][:, 0] = np.concatenate([np.diag([-1.0, 1.0, -1.0]), np.zeros((3, 1))], 1).reshape(12)

    def check_behind(out):
        assert not out.any()
    cases["source_behind"] = (c, check_behind)

    # a bilinear footprint that touches the last row / column exactly: no shift, the tap at column c lands on column c with
    # a = 0, and x0 + 1 <= W - 1 holds up to c = W - 2.  With R = 1 the pixels up to column W - 3 and row H - 3 store the
    # depth 2 (the two views are the same picture: cost 0) and column W - 2 and row H - 2, whose patches fit, store 0.
    c = exact_case(inv=(0.5,), t=0.0)
    c["gray"] = shifted_views(c["gray"][0], (0, 0))

    def check_last(out):
        H, W = out.shape[1:]
        assert (out[:, 1:H - 2, 1:W - 2] == np.float32(2.0)).all()
        assert not out[:, H - 2].any() and not out[:, :, W - 2].any()
    cases["footprint_last_row_col"] = (c, check_last)

    # a cost tie: a picture of period 2 along x matches at the disparities 4 (d = 0) and 2 (d = 1) alike -- cost 0 both
    c = exact_case(inv=(0.5, 0.25), t=8.0)
    base = np.tile(rng.integers(0, 256, (12, 2)), (1, 10))
    c["gray"] = shifted_views(base, (0, 0))

    def check_tie(out):   # up to column 13 both disparities land inside view 1: 1 / inv[0] = 2 there, never 4
        assert (out[0][:, :14] == np.float32(2.0)).any() and set(np.unique(out[0][:, :14])) <= {np.float32(0.0), np.float32(2.0)}
    cases["cost_tie"] = (c, check_tie)

    # the best hypothesis at d = 0 and at d = D - 1: view 1 is view 0 moved by the disparity of that hypothesis; the end
    # hypothesis is stored unrefined, 1 / inv to the bit
    for name, k in (("best_first", 0), ("best_last", 2)):
        invs = (0.5, 0.375, 0.25)
        c = exact_case(inv=invs, t=8.0, seed=5)
        c["gray"] = shifted_views(c["gray"][0], (0, int(8.0 * invs[k])))

        def check_end(out, z=np.float32(1.0 / invs[k])):
            assert (out[0] == z).any() and set(np.unique(out[0])) <= {np.float32(0.0), z}
        cases[name] = (c, check_end)

    # den <= 0.  den = (cm - cb) + (cp - cb) with cb the strict minimum before it and the minimum after it: from finite
    # costs it is > 0 unless cm == cb, which the strict < excludes, so the guard only ever sees its edge: cp == cb (a tie
    # AFTER the winner), where den = cm - cb and o is 0.5 exactly, the clamp's end.  View 1 matches at d = 1 and d = 2.
    c = exact_case(inv=(0.5, 0.25, 0.125), t=16.0, seed=6)
    base = np.tile(rng.integers(0, 256, (12, 2)), (1, 10))        # period 2: disparities 4 (d = 1) and 2 (d = 2) match
    base[:, 13] ^= 0x55                                           # ... and 8 (d = 0) does not, left of this mark
    c["gray"] = shifted_views(base, (0, 0))
    c["max_cost"] = 1.5

    def check_den(out):
        z = np.float32(1.0 / (0.25 + 0.5 * (0.125 - 0.25)))
        assert (out[0] == z).any()
    cases["den_edge"] = (c, check_den)

    for D in (1, 2):
        cases[f"D{D}"] = (random_case(3, 9, 11, D, 3, 1, 30 + D), lambda out: None)

    # min_sources above the valid count: two sources, three asked for
    c = random_case(3, 9, 11, 4, 3, 1, 25)
    c["min_sources"] = 3
    cases["min_sources_above"] = (c, check_behind)

    # every source -1
    c = random_case(3, 9, 11, 4, 3, 1, 26)
    c["src"] = np.full_like(c["src"], -1)
    cases["no_sources"] = (c, check_behind)

    # a NaN pose: the source never counts, the others are what they were
    c = random_case(3, 9, 11, 4, 3, 1, 27)
    c["rel"] = c["rel"].copy()
    c["rel"][0, 0, 5] = float("nan")
    cases["nan_pose"] = (c, lambda out: None)
    return cases


def consistency_case(V=3, H=6, W=10, zs=(2.0, 2.0, 2.0)):
    """Exact arithmetic again: three views shifted by 4 along x, every map constant at depth 2 -> a pixel at column c of
    view v lands on column c + 2 (w - v) of view w at depth 2."""
    K = np.tile(np.array([1.0, 1.0, 0.0, 0.0]), (V, 1))
    src, rel = np.zeros((V, V - 1), np.int32), np.zeros((V, V - 1, 12))
    for v in range(V):
        for s, w in enumerate([w for w in range(V) if w != v]):
            src[v, s] = w
            rel[v, s] = np.concatenate([np.eye(3), np.array([[(w - v) * 4.0], [0.0], [0.0]])], 1).reshape(12)
    depth = np.stack([np.full((H, W), z, np.float32) for z in zs])
    return dict(depth=depth, K=K, src=src, rel=rel, tol=np.full((V,), 0.01))


def random_consistency_case(V, H, W, S, seed):
    c = random_case(V, H, W, 4, S, 1, seed)
    rng = np.random.default_rng(seed)
    depth = rng.uniform(1.8, 2.2, (V, H, W)).astype(np.float32)
    depth[rng.random((V, H, W)) < 0.2] = 0.0
    depth[0, 0, 0] = np.nan
    if H * W > 1:
        depth[0].reshape(-1)[1] = -1.0
    return dict(depth=depth, K=c["K"], src=c["src"], rel=c["rel"], tol=np.full((V,), 0.04))
