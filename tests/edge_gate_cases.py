"""Shared inputs of the depth-gate tests (test_edge_gate_cpu.py, test_edge_gate_gpu.py): the four gated 2D operators
(include/curvegs.h: cgs_edge_support_depth, cgs_sample_support_depth, cgs_sample_support_oriented_depth,
cgs_sample_snap_terms_depth) restated as plain per-(sample, view) loops over Python floats, one operation at a time, from
the header's rule and independently of the host back ends; the cameras, samples and z-buffers of edge_occlusion_cases.py they
run on; and the solid scans whose facts the tests assert."""
import functools
import math

import numpy as np
import torch

import edge_occlusion_cases as OC
from curve_gaussian_amd.ops import edge_occlusion as EO
from curve_gaussian_amd.ops import edge_orient as OR
from curve_gaussian_amd.ops import edge_score as ES
from curve_gaussian_amd.ops import edge_snap as SN

HEIGHT = OC.HEIGHT
WIDTHS = OC.WIDTHS                # 1, 33, 67
VIEWS = OC.VIEWS                  # 1, 2, 5
POINT_COUNTS = OC.POINT_COUNTS    # 0, 1, 63, 64, 65, 4096: around a wave and a workgroup
EDGE_COUNTS = [0, 1, 3, 4, 5]     # around the four waves of a workgroup
SLACKS = [0.0, 0.01]
FACES = 257
TOLERANCES = (1, 2)
CAPTURE_PX = 3
SPREAD = 1
same_bits = OC.same_bits


# ------------------------------------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def views_case(W, V, seed=11):
    """The per-view inputs at width W and V views, computed once, shared, read-only: cameras, the windowed reference z-buffer
    (hidden and visible samples both occur), random detected masks and what the ungated operators derive from them."""
    K, M = OC.cameras(V, HEIGHT, W)
    depth = EO.depth_window_max(OC.reference_zbuffer(FACES, W, V), 1, backend="host").numpy()
    rng = np.random.default_rng(seed + 100 * W + V)
    masks = (rng.random((V, HEIGHT, W)) < 0.2).astype(np.uint8)
    d2 = ES.edt_squared(masks, backend="host").numpy()
    near = OR.oriented_near(OR.mask_orientation(masks, backend="host"), TOLERANCES[0], backend="host").numpy()
    out = dict(K=K, M=M, depth=depth, masks=masks, d2=d2, near=near)
    for a in out.values():
        a.setflags(write=False)
    return out


def offsets_for(E, P):
    """int32 [E+1] from 0 to P: edge 1 (when there is one) has no samples, the others split P unevenly, so that with P > 64
    ranges start and end off the 64-lane stride."""
    if E == 0:
        return np.zeros(1, np.int32)   # (P must be 0)
    cuts = [0] + sorted(int(round(P * f)) for f in np.linspace(0.13, 0.87, E - 1)) + [P] if E > 1 else [0, P]
    if E > 1:
        cuts[2] = cuts[1]              # edge 1 is empty
    return np.asarray(cuts, np.int32)


# ------------------------------------------------------------------------------------------------ the rule, one pair at a time
def _verdict(K, M, X, Y, Z, depth_plane, slack, H, W):
    """None when the view does not keep the sample, else (u, v, c2, hidden): the projection of cgs_project_points, then
    c2 > (double)depth[floor(v)][floor(u)] + slack."""
    c2, u, v = OC._project(K, M, X, Y, Z)
    if u is None or not (0.0 <= u < W and 0.0 <= v < H):
        return None
    d = float(depth_plane[int(math.floor(v)), int(math.floor(u))])
    return u, v, c2, c2 > d + slack


def _pts(points):
    return [(float(X), float(Y), float(Z)) for X, Y, Z in np.asarray(points, np.float32).reshape(-1, 3)]


def support_brute(points, offsets, K, M, d2, tol2, depth, slack):
    """cgs_edge_support_depth: (counts int32 [E,V,1+T], hidden int32 [E,V])."""
    V, H, W = d2.shape
    E, pts = len(offsets) - 1, _pts(points)
    counts, hidden = np.zeros((E, V, 1 + len(tol2)), np.int32), np.zeros((E, V), np.int32)
    for e in range(E):
        for view in range(V):
            for X, Y, Z in pts[offsets[e]:offsets[e + 1]]:
                r = _verdict(K[view], M[view], X, Y, Z, depth[view], slack, H, W)
                if r is None:
                    continue
                if r[3]:
                    hidden[e, view] += 1
                    continue
                d = int(d2[view, int(math.floor(r[1])), int(math.floor(r[0]))])
                counts[e, view, 0] += 1
                for t, t2 in enumerate(tol2):
                    counts[e, view, 1 + t] += d <= t2
    return counts, hidden


def tally_brute(points, K, M, d2, tol2, depth, slack):
    """cgs_sample_support_depth from zero: (tally int32 [P,1+T], hidden int32 [P])."""
    V, H, W = d2.shape
    pts = _pts(points)
    tally, hidden = np.zeros((len(pts), 1 + len(tol2)), np.int32), np.zeros(len(pts), np.int32)
    for i, (X, Y, Z) in enumerate(pts):
        for view in range(V):
            r = _verdict(K[view], M[view], X, Y, Z, depth[view], slack, H, W)
            if r is None:
                continue
            if r[3]:
                hidden[i] += 1
                continue
            d = int(d2[view, int(math.floor(r[1])), int(math.floor(r[0]))])
            tally[i, 0] += 1
            for t, t2 in enumerate(tol2):
                tally[i, 1 + t] += d <= t2
    return tally, hidden


def _octant(a, b):
    ma, mb = abs(a), abs(b)
    if a > 0 and b >= 0:
        return 0 if mb < ma else 1
    if a <= 0 and b > 0:
        return 2 if mb > ma else 3
    if a < 0 and b <= 0:
        return 4 if mb < ma else 5
    return 6 if mb > ma else 7


def oriented_brute(points, partner, K, M, near, spread, depth, slack):
    """cgs_sample_support_oriented_depth from zero: (tally int32 [P,2], hidden int32 [P]).  The sample is gated; the partner is
    projected by the projection rule alone and never held against the depth."""
    V, H, W = near.shape
    pts = _pts(points)
    P = len(pts)
    tally, hidden = np.zeros((P, 2), np.int32), np.zeros(P, np.int32)
    for i, (X, Y, Z) in enumerate(pts):
        j = int(partner[i])
        paired = j != i and 0 <= j < P
        for view in range(V):
            r = _verdict(K[view], M[view], X, Y, Z, depth[view], slack, H, W)
            if r is None:
                continue
            if r[3]:
                hidden[i] += 1
                continue
            u, v = r[0], r[1]
            acc = 0xFF
            if paired:
                _, up, vp = OC._project(K[view], M[view], *pts[j])
                if up is not None and 0.0 <= up < W and 0.0 <= vp < H:
                    dx, dy = up - u, vp - v
                    a, b = dx * dx - dy * dy, 2.0 * (dx * dy)
                    if a != 0.0 or b != 0.0:
                        acc = 0
                        for s in range(-spread, spread + 1):
                            acc |= 1 << ((_octant(a, b) + s) % 8)
            tally[i, 0] += 1
            tally[i, 1] += (int(near[view, int(math.floor(v)), int(math.floor(u))]) & acc) != 0
    return tally, hidden


def snap_brute(points, K, M, d2, cap2, depth, slack):
    """cgs_sample_snap_terms_depth from zero: (terms float64 [P,10], views int32 [P], hidden int32 [P]).  A hidden pair leaves
    right after the projection's verdict, before the footprint test."""
    V, H, W = d2.shape
    pts = _pts(points)
    lut = [float(x) for x in SN.distance_table(cap2)]
    terms, views, hidden = np.zeros((len(pts), 10), np.float64), np.zeros(len(pts), np.int32), np.zeros(len(pts), np.int32)
    for i, (X, Y, Z) in enumerate(pts):
        row = [0.0] * 10
        for view in range(V):
            m = [float(x) for x in np.asarray(M[view]).reshape(12)]
            fx, fy = float(K[view][0]), float(K[view][1])
            r = _verdict(K[view], M[view], X, Y, Z, depth[view], slack, H, W)
            if r is None:
                continue
            if r[3]:
                hidden[i] += 1
                continue
            u, v, c2 = r[0], r[1], r[2]
            c0 = ((m[0] * X + m[1] * Y) + m[2] * Z) + m[3]
            c1 = ((m[4] * X + m[5] * Y) + m[6] * Z) + m[7]
            x, y = c0 / c2, c1 / c2
            a, b = u - 0.5, v - 0.5
            fj, fi = math.floor(a), math.floor(b)
            j0, i0 = int(fj), int(fi)
            if j0 < 0 or j0 + 1 > W - 1 or i0 < 0 or i0 + 1 > H - 1:
                continue
            k = [int(d2[view, i0, j0]), int(d2[view, i0, j0 + 1]), int(d2[view, i0 + 1, j0]), int(d2[view, i0 + 1, j0 + 1])]
            if any(q < 0 or q > cap2 for q in k):
                continue
            d00, d01, d10, d11 = (lut[q] for q in k)
            fa, fb = a - fj, b - fi
            ga, gb = 1.0 - fa, 1.0 - fb
            res = gb * (ga * d00 + fa * d01) + fb * (ga * d10 + fa * d11)
            gu = gb * (d01 - d00) + fb * (d11 - d10)
            gv = ga * (d10 - d00) + fa * (d11 - d01)
            su, sv = (gu * fx) / c2, (gv * fy) / c2
            gc = -(su * x + sv * y)
            gx = (m[0] * su + m[4] * sv) + m[8] * gc
            gy = (m[1] * su + m[5] * sv) + m[9] * gc
            gz = (m[2] * su + m[6] * sv) + m[10] * gc
            for c, val in enumerate((gx * gx, gx * gy, gx * gz, gy * gy, gy * gz, gz * gz, gx * res, gy * res, gz * res,
                                     res * res)):
                row[c] += val
            views[i] += 1
        terms[i] = row
    return terms, views, hidden


# ------------------------------------------------------------------------------------------------ the operators, one call
def run_operators(P, E, W, V, slack, backend, device=None, depth="case", hidden=True, prefill=0):
    """The four gated operators on samples(P) cut into E edges, at width W and V views, on one back end.  ``depth``: "case"
    (the windowed reference z-buffer), None (ungated) or an array.  ``hidden``: whether the hidden outputs are asked for.
    ``prefill``: the value the outputs handed in are filled with first (the ADDING entries add to it, the WRITING one must
    overwrite it).  Returns a dict of numpy arrays."""
    from curve_gaussian_amd.ops import edge_support as SP
    from curve_gaussian_amd.ops import edge_trim as ET
    c = views_case(W, V)
    pts, off = OC.samples(P), offsets_for(E, P)
    partner = OR.sample_partners(off)
    if isinstance(depth, str):
        depth = c["depth"]
    gated = depth is not None
    dev = device if backend == "gpu" else None
    on = (lambda a: torch.from_numpy(np.array(a)).to(dev)) if backend == "gpu" else (lambda a: torch.from_numpy(np.array(a)))
    d2, near = on(c["d2"]), on(c["near"])
    full = lambda shape, dtype: torch.full(shape, prefill, dtype=dtype, device=dev)
    kw = dict(depth=np.array(depth), slack=slack) if gated else {}
    c = dict(c, K=np.array(c["K"]), M=np.array(c["M"]))   # (the shared arrays are read-only)
    out = {}
    r = SP.support_counts(pts, off, c["K"], c["M"], d2, TOLERANCES, backend=backend, **kw,
                          **({"return_hidden": True} if gated and hidden else {}))
    out["counts"], out["counts_hidden"] = (r if isinstance(r, tuple) else (r, None))
    tally, th = full((P, 1 + len(TOLERANCES)), torch.int32), full((P,), torch.int32) if gated and hidden else None
    ET.sample_tally(pts, c["K"], c["M"], d2, TOLERANCES, backend=backend, out=tally, **kw,
                    **({"hidden_out": th} if th is not None else {}))
    out["tally"], out["tally_hidden"] = tally, th
    ot, oh = full((P, 2), torch.int32), full((P,), torch.int32) if gated and hidden else None
    OR.oriented_tally(pts, partner, c["K"], c["M"], near, SPREAD, backend=backend, out=ot, **kw,
                      **({"hidden_out": oh} if oh is not None else {}))
    out["oriented"], out["oriented_hidden"] = ot, oh
    terms, views = full((P, 10), torch.float64), full((P,), torch.int32)
    sh = full((P,), torch.int32) if gated and hidden else None
    SN.snap_terms(pts, c["K"], c["M"], d2, CAPTURE_PX, backend=backend, out=(terms, views), **kw,
                  **({"hidden_out": sh} if sh is not None else {}))
    out["terms"], out["views"], out["snap_hidden"] = terms, views, sh
    return {k: (None if v is None else v.cpu().numpy()) for k, v in out.items()}


def assert_same(got, want, what):
    assert set(got) == set(want), what
    for k in want:
        assert (got[k] is None) == (want[k] is None), (what, k)
        if want[k] is not None:
            assert same_bits(got[k], want[k]), f"{what}: {k} differs"


# ------------------------------------------------------------------------------------------------ solids
SOLIDS = [("box", 6, 48, 64), ("l_bracket", 6, 48, 64), ("cylinder", 6, 48, 64), ("l_bracket", 12, 96, 128)]
# the (edge, view) cells with seen > 0 without the gate, those of them with near < seen at 1 px, and the cells with the gate
SOLID_CELLS = {("box", 6): (72, 22, 70), ("l_bracket", 6): (108, 37, 100), ("cylinder", 6): (48, 15, 45),
               ("l_bracket", 12): (216, 70, 202)}
SOLID_OPTIONS = dict(resolution=0.0005, tolerances_px=(1, 2))


@functools.lru_cache(maxsize=None)
def solid(shape, views, H, W):
    """A solid scan drawn on the host (both back ends give the same bytes): computed once, shared."""
    from curve_gaussian_amd.scene.solid_scan import solid_scan
    return solid_scan(shape, views, H, W, backend="host")


def check_solid_facts(shape, views, H, W, backend):
    """The facts of a solid's ground truth at 1 and 2 px: exact with the gate, inflated without."""
    from curve_gaussian_amd.ops import edge_support as SP
    from curve_gaussian_amd.ops import edge_trim as ET
    scan = solid(shape, views, H, W)
    plain_cells, plain_short, gated_cells = SOLID_CELLS[(shape, views)]
    run = lambda keep, **kw: SP.edge_support(scan.edges, scan.cameras, scan.maps, "PidiNet", keep_tolerance_px=keep,
                                             backend=backend, **SOLID_OPTIONS, **kw)
    plain = run(1)
    c = plain["counts"].numpy()
    assert "hidden" not in plain
    assert int((c[..., 0] > 0).sum()) == plain_cells and int(((c[..., 0] > 0) & (c[..., 1] < c[..., 0])).sum()) == plain_short
    assert plain_short >= 1 and (plain["seeing_views"] == views).all(), "without depth every view sees every edge"
    for keep in (1, 2):
        gated = run(keep, occluder=scan.tris)
        g = gated["counts"].numpy()
        seen = g[..., 0] > 0
        assert int(seen.sum()) == gated_cells
        assert (g[..., 1][seen] == g[..., 0][seen]).all() and (g[..., 2][seen] == g[..., 0][seen]).all(), "near == seen"
        assert (gated["supporting_views"] == gated["seeing_views"][:, None]).all()
        assert gated["kept"].all(), "every edge is kept"
        assert (gated["hidden"].numpy().sum(0) == scan.hidden).all(), "hidden per view is the scan's"
        assert same_bits(g[..., 0] + gated["hidden"].numpy(), c[..., 0]), "seen + hidden is the plain seen"
        assert gated["settings"]["occluder"] is True and gated["settings"]["depth_window"] == EO.DEPTH_WINDOW
        maps = run(keep, depth_maps=list(scan.depth))
        assert same_bits(maps["counts"].numpy(), g) and same_bits(maps["hidden"].numpy(), gated["hidden"].numpy())
        assert maps["settings"]["depth_maps"] is True and "occluder" not in maps["settings"]
    if (shape, views) == ("box", 6):
        assert int(plain["supporting_views"][3, 0]) == 5 and int(gated["seeing_views"][3]) == 4, \
            "edge 3 collects support it cannot have"
    # trimming the gated ground truth returns every edge whole, bit for bit
    trim = ET.trim_edges(scan.edges, scan.cameras, scan.maps, "PidiNet", backend=backend, resolution=0.0005,
                         occluder=scan.tris)
    lines = np.asarray(scan.edges["lines_end_pts"], np.float64).reshape(-1, 6)
    curves = np.asarray(scan.edges["curves_ctl_pts"], np.float64).reshape(-1, 4, 3)
    assert same_bits(np.asarray(trim["edge_dict"]["lines_end_pts"], np.float64).reshape(-1, 6), lines)
    assert same_bits(np.asarray(trim["edge_dict"]["curves_ctl_pts"], np.float64).reshape(-1, 4, 3), curves)
    assert list(trim["source"]) == list(range(len(lines) + len(curves)))
    assert (trim["hidden"].numpy().sum() == scan.hidden.sum()) and trim["settings"]["occluder"] is True


BUDGETS = [(None, 1), (2 * 15 * 48 * 64, 3), (1, 5)]   # (budget_bytes, chunks) for 5 views of 48 x 64 at 7 + 8 bytes per pixel


def scan_level(scan, backend, budget, **gate):
    """The four scan-level functions on a solid scan's ground truth."""
    from curve_gaussian_amd.ops import edge_support as SP
    from curve_gaussian_amd.ops import edge_trim as ET
    common = dict(backend=backend, budget_bytes=budget, resolution=0.0005, **gate)
    args = (scan.edges, scan.cameras, scan.maps, "PidiNet")
    return {"support": SP.edge_support(*args, tolerances_px=(1, 2), keep_tolerance_px=1, **common),
            "trim": ET.trim_edges(*args, **common), "oriented": ET.trim_edges(*args, oriented=True, **common),
            "snap": SN.snap_edges(*args, iterations=1, **common)}


def comparable(results):
    """``canon`` of scan-level results without what names the run and not its outcome: the back end and the chunk count."""
    out = {k: dict(v) for k, v in results.items()}
    for r in out.values():
        r["settings"] = {k: v for k, v in r["settings"].items() if k not in ("chunks", "backend")}
    return canon(out)


def canon(x):
    """A result dict as nested tuples of plain values, with arrays and tensors as (dtype, shape, bytes): equal iff the two
    results hold the same keys and the same bits."""
    if torch.is_tensor(x):
        x = x.cpu().numpy()
    if isinstance(x, np.ndarray):
        return ("array", str(x.dtype), x.shape, np.ascontiguousarray(x).tobytes())
    if isinstance(x, dict):
        return tuple((k, canon(v)) for k, v in sorted(x.items()))
    if isinstance(x, (list, tuple)):
        return tuple(canon(v) for v in x)
    if isinstance(x, (float, np.floating)):
        return ("float", np.float64(x).tobytes())
    return x
