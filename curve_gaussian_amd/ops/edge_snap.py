"""Snapping extracted edges onto the detected edges (cgs_sample_snap_terms, include/curvegs.h; csrc/edge_snap.hip).  The
chain of ops/edge_support.py, ops/edge_trim.py, ops/edge_dedupe.py and ops/edge_join.py can check, cut, drop and rejoin an
edge; none of them can MOVE one, so an edge that training left a pixel or two beside the detected edge stays there, and
every later tool pays for it.  The evidence that corrects it is the one those tools already hold on the device: the exact
squared distance transform of every view's detected mask.  Opt-in; the reference has no counterpart.

  snap_terms   per sample, over the views, the 3x3 normal equations of "move me onto the nearest detected edge in every
               image": float64 [P,10] = (Axx, Axy, Axz, Ayy, Ayz, Azz, bx, by, bz, rr) and int32 [P] views; ADDS to an
               ``out`` handed in
  snap_step    the damped step of every constrained sample, on the host
  refit        each edge's own control points (4 for a curve, 2 for a line) fitted to its moved samples
  snap_edges   the three, iterated, on a scan's cameras and stored edge maps, with a gate, a guard and shared ends

The rule of the terms, frozen (include/curvegs.h writes it out operation by operation; the point-by-point
``snap_terms_brute`` of tests/edge_snap_cases.py is its definition): for every view whose projection keeps the sample
(``cgs_project_points``, to the letter) the four pixel centres around its image point must lie inside the plane and all
within ``capture_px`` of a detected pixel (d2 <= floor(capture_px^2), compared before anything is looked up); r is the
bilinear interpolation of their distances sqrt(d2) -- a table computed on the host, no square root on the device -- and g
the gradient of r with respect to the world point; A += g g^T, b += g r, rr += r r, views += 1.  Float64, one rounded
operation at a time, view by view in view order into the sample's own row: however the views are cut into calls, a row
is the same floating-point sequence, so chunking cannot change a bit, and the two back ends agree on every bit.

The step, frozen: a sample is CONSTRAINED iff views > ceil(frames_ratio * frames) (the frame rule of
``edge_trim.supported_samples``).  A constrained sample moves by delta = -(A + lambda I)^-1 b with lambda = damping *
trace(A) / 3, clipped to the length ``step_cap``; any other sample gets delta = 0 and holds its edge in place.  The images
pull across an edge, never along it, and the damping leaves the direction without pull at zero: a snap does not change an
edge's length -- that is trimming's job.  The refit is a linear least-squares fit of the edge's control points to the
targets B(t) P + delta at the fixed parameters np.linspace(0, 1, n) of ``sample_edges`` (Bernstein basis for a curve,
(1 - t, t) for a line: a line stays a line).

DEPTH (opt-in).  Without a depth source a sample hidden behind a surface is pulled onto whatever front
edge it projects within ``capture_px`` of.  With ``depth`` (``snap_terms``) or ``occluder`` / ``depth_maps``
(``snap_edges``) a view whose depth plane hides the sample -- the one rule of ops/edge_occlusion.py -- contributes no term
and no view: it is left right after the projection's verdict, before the footprint test, and for every other view the
floating-point sequence is unchanged.  Limits as ops/edge_occlusion.py states them: untuned, drawn solids only, concave
edges, no near-plane clipping unless ``near_clip`` is given.

KNOWN LIMITS.  A sample inside the capture radius of the WRONG edge is pulled
to it: at crossings, and along a parallel edge closer than ``capture_px``.  Snapping is not a filter: a bogus chord that
passes the gate is moved too (the gate asks that 0.8 of an edge's samples be constrained; see DESIGN.md 4.8s for what the
drawn scan's chords read).  A shared end with a member that came back unchanged stays at the old point, off the moved
member's own fit; ``join_edges`` remains the tool for corners.  The drawn maps are quantised to pixels, so the evidence itself is off by up to half a pixel.  EVERY
DEFAULT OF ``snap_edges`` IS UNTUNED: only the drawn test scan (tests/edge_snap_cases.py) has been checked, no real scan.

Two back ends: ``"gpu"``, HIP, and ``"host"``, numpy -- the same rule in the same order, so the terms agree bit for bit;
the step, the refit and everything after them are host arithmetic for both."""
import math

import numpy as np
import torch

from .. import _lib as L
from ..edge_extraction.para_edge import EDGE_MAX_THRESHOLD, EDGE_VISIBILITY_FRAMES_RATIO
from ..edge_extraction.reprojection import SAMPLE_RESOLUTION
from . import edge_occlusion as EO
from . import edge_score as ES
from . import edge_support as SP
from .edge_thin import thin_masks
from .view_chunks import check_budget, check_edge_maps, detected_lut, detected_masks, view_chunks

SNAP_BACKENDS = SP.SUPPORT_BACKENDS
BYTE_BUDGET = SP.BYTE_BUDGET
BYTES_PER_PIXEL = SP.BYTES_PER_PIXEL   # the working set of edge_support: one uint8 mask, one uint16 pass, one int32 transform
MAX_CAP2 = L.SNAP_MAX_CAP2
TERMS = L.SNAP_TERMS
# UNTUNED, like the defaults of ops/edge_trim.py: the drawn test scan only, no real scan
CAPTURE_PX = 3
ITERATIONS = 5
MIN_CONSTRAINED = 0.8
DAMPING = 1e-2
STEP_CAP_RESOLUTIONS = 4   # step_cap = None: this many sampling resolutions


# ------------------------------------------------------------------------------------------------ terms
def capture_squared(capture_px):
    """cap2 = floor(capture_px^2), which must lie in [1, MAX_CAP2]: for an integer d2, d2 <= capture_px^2 iff d2 <= cap2."""
    c = float(capture_px)
    cap2 = int(math.floor(c * c)) if c == c and 0.0 <= c <= L.EDT_MAX_SIZE else -1
    if not (1 <= cap2 <= MAX_CAP2):
        raise ValueError(f"capture_px must lie in [1, {math.isqrt(MAX_CAP2)}] pixels (got {capture_px})")
    return cap2


def distance_table(cap2):
    """float64 [cap2 + 1]: sqrt(k), correctly rounded, on the host -- the one table both back ends read."""
    return np.sqrt(np.arange(cap2 + 1, dtype=np.float64))


def _terms_host(pts, K, M, d2, cap2, lut, terms, views, depth=None, slack=0.0, hidden=None):
    """``depth`` float32 [V,H,W] or None; ``hidden`` int32 [P] or None, added to when there is a depth."""
    H, W = d2.shape[1], d2.shape[2]
    P64 = pts.astype(np.float64)
    X, Y, Z = P64[:, 0], P64[:, 1], P64[:, 2]
    for v in range(K.shape[0]):   # one view at a time, in view order: [P] temporaries
        m, (fx, fy, cx, cy) = M[v], K[v]
        with np.errstate(all="ignore"):
            c0 = ((m[0] * X + m[1] * Y) + m[2] * Z) + m[3]
            c1 = ((m[4] * X + m[5] * Y) + m[6] * Z) + m[7]
            c2 = ((m[8] * X + m[9] * Y) + m[10] * Z) + m[11]
            x, y = c0 / c2, c1 / c2
            u, w = fx * x + cx, fy * y + cy
            keep = ~(c2 <= 0.0) & (u >= 0.0) & (u < float(W)) & (w >= 0.0) & (w < float(H))   # NaN fails the image test
            if depth is not None:   # right after the projection's verdict: a hidden pair gives no term and no view
                hid = EO.hidden_host(c2, u, w, keep, depth[v], slack)
                keep &= ~hid
                if hidden is not None:
                    hidden += hid
            a, b = u - 0.5, w - 0.5
            fj, fi = np.floor(a), np.floor(b)
            keep &= (fj >= 0.0) & (fj + 1.0 <= W - 1.0) & (fi >= 0.0) & (fi + 1.0 <= H - 1.0)
        idx = np.flatnonzero(keep)
        j0, i0 = fj[idx].astype(np.int64), fi[idx].astype(np.int64)
        k = np.stack([d2[v][i0, j0], d2[v][i0, j0 + 1], d2[v][i0 + 1, j0], d2[v][i0 + 1, j0 + 1]]).astype(np.int64)
        near = ((k >= 0) & (k <= cap2)).all(0)   # the capture, before the table is indexed
        idx, k = idx[near], k[:, near]
        d00, d01, d10, d11 = lut[k[0]], lut[k[1]], lut[k[2]], lut[k[3]]
        fa, fb = a[idx] - fj[idx], b[idx] - fi[idx]
        ga, gb = 1.0 - fa, 1.0 - fb
        r = gb * (ga * d00 + fa * d01) + fb * (ga * d10 + fa * d11)
        gu = gb * (d01 - d00) + fb * (d11 - d10)
        gv = ga * (d10 - d00) + fa * (d11 - d01)
        su, sv = (gu * fx) / c2[idx], (gv * fy) / c2[idx]
        gc = -(su * x[idx] + sv * y[idx])
        gx = (m[0] * su + m[4] * sv) + m[8] * gc
        gy = (m[1] * su + m[5] * sv) + m[9] * gc
        gz = (m[2] * su + m[6] * sv) + m[10] * gc
        for col, val in enumerate((gx * gx, gx * gy, gx * gz, gy * gy, gy * gz, gz * gz, gx * r, gy * r, gz * r, r * r)):
            terms[idx, col] += val   # idx has no repeats: one add per row and view
        views[idx] += 1


def _check_out(out, P):
    if (not isinstance(out, (tuple, list)) or len(out) != 2 or not all(torch.is_tensor(t) and t.is_contiguous() for t in out)
            or out[0].dtype != torch.float64 or tuple(out[0].shape) != (P, TERMS) or out[1].dtype != torch.int32
            or tuple(out[1].shape) != (P,)):
        raise ValueError(f"snap_terms: out must be (a contiguous float64 [{P},{TERMS}] tensor, a contiguous int32 [{P}] "
                         "tensor)")
    return out[0], out[1]


def snap_terms(points, intrinsics, w2c, d2, capture_px, backend="gpu", device=None, out=None, depth=None,
               slack=EO.DEPTH_SLACK, hidden_out=None):
    """(terms float64 [P,10], views int32 [P]).  points float32 [P,3]; intrinsics [V,4] = (fx, fy, cx, cy) and w2c [V,3,4]
    float64 host arrays or tensors; d2 int32 [V,H,W], ``edt_squared`` of every view's detected mask -- the arguments of
    ``sample_tally`` -- and ``capture_px``, whose square, rounded down, lies in [1, 64].  A row of terms is (Axx, Axy, Axz,
    Ayy, Ayz, Azz, bx, by, bz, rr) of the module docstring, summed over the views that capture the sample; views counts them.

    ``out``: a pair (terms, views) of contiguous tensors that the sums are ADDED to, view by view in view order, and that
    is returned -- one call per chunk of views into the same pair gives the bits of one call over all of them; without it
    the sums of this call alone, in new tensors.

    ``backend="gpu"``: ``cgs_sample_snap_terms``.  d2 must be on a GPU (CurveGSError otherwise), ``device``, when given, must
    be that GPU, and so must the device of ``out`` and of points that are on a GPU; points on the host are uploaded.  The
    result stays on the device.  ``backend="host"``: numpy, CPU tensors.

    ``depth`` (None: no gate, the call above and nothing else), ``slack`` and ``hidden_out`` as ``edge_trim.sample_tally``
    takes them (``cgs_sample_snap_terms_depth``): a view that keeps sample i and whose depth plane hides it adds no term and
    no view and is ADDED to hidden_out[i], whether or not its footprint would have captured the sample; the sums of the other
    views are bit for bit what they are without the gate."""
    SP._check_backend(backend)
    cap2 = capture_squared(capture_px)
    pts = SP._points(points)
    V, K, M = ES._cameras(intrinsics, w2c)
    d2 = SP._d2(d2, V)
    P = int(pts.shape[0])
    if out is not None:
        terms, views = _check_out(out, P)
    lut = distance_table(cap2)
    EO.check_hidden_out("snap_terms", hidden_out, depth, P)
    if backend == "host":
        SP._host_only("snap_terms", d2, pts, *(out or ()), hidden_out)
        if out is None:
            terms, views = torch.zeros((P, TERMS), dtype=torch.float64), torch.zeros((P,), dtype=torch.int32)
        if depth is not None:
            depth, slack = EO.operator_depth("snap_terms", depth, slack, V, int(d2.shape[1]), int(d2.shape[2]), "host")
        _terms_host(pts.numpy(), K, M, d2.numpy(), cap2, lut, terms.numpy(), views.numpy(), depth, slack,
                    None if hidden_out is None else hidden_out.numpy())
        return terms, views
    dev = SP._one_device("snap_terms", "d2", d2, device, uploaded=[("points", pts)],
                         resident=[("out", out or ()), ("hidden_out", [hidden_out])])
    with L.device_guard(dev):
        pts = pts.to(dev).contiguous()
        if out is None:
            terms = torch.zeros((P, TERMS), dtype=torch.float64, device=dev)
            views = torch.zeros((P,), dtype=torch.int32, device=dev)
        if depth is not None:
            depth, slack = EO.operator_depth("snap_terms", depth, slack, V, int(d2.shape[1]), int(d2.shape[2]), "gpu", dev)
        if P > 0 and V > 0:
            lut_d = torch.from_numpy(lut).to(dev)
            Kd, Md = ES.cameras_on(dev, K, M)
            args = [P, L.ptr(pts), V, L.ptr(Kd), L.ptr(Md), int(d2.shape[1]), int(d2.shape[2]), L.ptr(d2), cap2, L.ptr(lut_d)]
            if depth is None:
                L.check(L.load().cgs_sample_snap_terms(*args, L.ptr(terms), L.ptr(views), L.raw_stream(dev)),
                        "cgs_sample_snap_terms")
            else:
                L.check(L.load().cgs_sample_snap_terms_depth(*args, L.ptr(depth), slack, L.ptr(terms), L.ptr(views),
                                                             L.ptr(hidden_out), L.raw_stream(dev)),
                        "cgs_sample_snap_terms_depth")
    return terms, views


# ------------------------------------------------------------------------------------------------ step and refit
def _positive(name, x):
    x = float(x)
    if not (x > 0.0 and math.isfinite(x)):
        raise ValueError(f"{name} must be positive and finite (got {x})")
    return x


def constrained_samples(views, frames, frames_ratio=EDGE_VISIBILITY_FRAMES_RATIO):
    """bool [P] (numpy): views > ceil(frames_ratio * frames), the frame rule of ``supported_samples``."""
    n = ES._host(views)
    if n.ndim != 1 or not np.issubdtype(n.dtype, np.integer):
        raise ValueError(f"views must be an integer [P] array (got {n.dtype} {n.shape})")
    return n.astype(np.int64) > math.ceil(SP._ratio01("frames_ratio", frames_ratio) * int(frames))


def snap_step(samples64, terms, views, frames, frames_ratio=EDGE_VISIBILITY_FRAMES_RATIO, damping=DAMPING, step_cap=None):
    """(delta float64 [P,3], constrained bool [P]): the step of every sample, host arithmetic for either back end's terms.
    A constrained sample (``constrained_samples``) moves by -(A + lambda I)^-1 b, lambda = damping * trace(A) / 3, clipped
    to the length ``step_cap`` (None: no clip); a sample whose A is zero, and every unconstrained one, gets 0.  ``samples64``
    [P,3] fixes the shape only: the step does not depend on where the sample is."""
    s = np.asarray(ES._host(samples64), np.float64)
    t = np.asarray(ES._host(terms), np.float64)
    if s.ndim != 2 or s.shape[1] != 3 or t.shape != (s.shape[0], TERMS):
        raise ValueError(f"snap_step: samples must be [P,3] and terms [P,{TERMS}] (got {s.shape}, {t.shape})")
    damping = _positive("damping", damping)
    con = constrained_samples(views, frames, frames_ratio)
    if con.shape != (s.shape[0],):
        raise ValueError(f"snap_step: views must be [{s.shape[0]}] (got {con.shape})")
    delta = np.zeros_like(s)
    trace = (t[:, 0] + t[:, 3]) + t[:, 5]
    idx = np.flatnonzero(con & (trace > 0.0))
    if idx.size:
        q = t[idx]
        A = np.stack([q[:, 0], q[:, 1], q[:, 2], q[:, 1], q[:, 3], q[:, 4], q[:, 2], q[:, 4], q[:, 5]], 1).reshape(-1, 3, 3)
        A = A + ((damping * trace[idx]) / 3.0)[:, None, None] * np.eye(3)
        d = -np.linalg.solve(A, q[:, 6:9, None])[:, :, 0]
        if step_cap is not None:
            cap = _positive("step_cap", step_cap)
            norm = np.sqrt((d * d).sum(1))
            long = norm > cap
            d[long] *= (cap / norm[long])[:, None]
        delta[idx] = d
    return delta, con


def _basis(n, curve):
    t = np.linspace(0, 1, n)
    if curve:
        return np.stack([(1 - t) ** 3, 3 * (1 - t) ** 2 * t, 3 * (1 - t) * t ** 2, t ** 3], 1)
    return np.stack([1 - t, t], 1)


def _positions(curves, lines, sizes):
    """float64 [P,3]: n samples of every edge at np.linspace(0, 1, n), by the expressions of ``sample_edges`` (so that the
    first pass projects exactly its points), with the sizes held fixed while the control points move."""
    parts = []
    for curve, n in zip(curves, sizes[:len(curves)]):
        t = np.linspace(0, 1, n)
        U = np.array([t ** 3, t ** 2, t, np.ones_like(t)])
        parts.append(U.T.dot(SP._BEZIER).dot(curve))
    for line, n in zip(lines, sizes[len(curves):]):
        t = np.linspace(0, 1, n)
        parts.append(np.outer(t, line[1] - line[0]) + line[0])
    return np.concatenate(parts).reshape(-1, 3) if parts else np.zeros((0, 3))


def refit(curves, lines, offsets, delta, edges=None):
    """(curves float64 [Nc,4,3], lines float64 [Nl,2,3]): every edge's own control points fitted, by linear least squares, to
    the targets B(t) P + delta at the parameters np.linspace(0, 1, n) of its n samples (offsets int [E+1] of
    ``sample_edges``; delta float64 [P,3]); Bernstein basis for a curve, (1 - t, t) for a line.  ``edges``: bool [E], the
    edges to fit (None: all); the others, and an edge of fewer than two samples, come back as they are."""
    curves, lines = SP._edge_arrays(curves, lines)
    delta = np.asarray(delta, np.float64)
    off = SP._offsets(offsets, delta.shape[0]).astype(np.int64)
    E, Nc = len(curves) + len(lines), len(curves)
    if off.size != E + 1 or delta.ndim != 2 or delta.shape[1] != 3:
        raise ValueError(f"refit: {E} edges, {off.size - 1} ranges of samples and steps of shape {delta.shape}")
    out_c, out_l = curves.copy(), lines.copy()
    for e in range(E):
        n = int(off[e + 1] - off[e])
        if n < 2 or (edges is not None and not edges[e]):
            continue
        ctl = curves[e] if e < Nc else lines[e - Nc]
        B = _basis(n, e < Nc)
        fit = np.linalg.lstsq(B, B.dot(ctl) + delta[off[e]:off[e + 1]], rcond=None)[0]
        if e < Nc:
            out_c[e] = fit
        else:
            out_l[e - Nc] = fit
    return out_c, out_l


# ------------------------------------------------------------------------------------------------ a scan
def _edge_sums(x, off):
    run = np.concatenate([[0.0], np.cumsum(np.asarray(x, np.float64))])
    return run[off[1:]] - run[off[:-1]]


def _edge_rms(terms, views, con, off):
    """float64 [E]: sqrt(sum rr / sum views) over the constrained samples of every edge, in pixels; NaN for an edge with none."""
    rr = _edge_sums(np.where(con, terms[:, 9], 0.0), off)
    n = _edge_sums(np.where(con, views, 0), off)
    with np.errstate(all="ignore"):
        return np.where(n > 0, np.sqrt(rr / n), np.nan)


def _share_ends(old_c, old_l, new_c, new_l, moved):
    """End control points that were bitwise equal before are made bitwise equal after: the mean of the members' snapped
    ends, or the old point when the edge of any member came back unchanged."""
    Nc = len(old_c)
    ends = [(e, k) for e in range(Nc) for k in (0, 3)] + [(Nc + e, k) for e in range(len(old_l)) for k in (0, 1)]
    point = lambda c, l, e, k: c[e][k] if e < Nc else l[e - Nc][k]
    groups = {}
    for e, k in ends:
        groups.setdefault(point(old_c, old_l, e, k).tobytes(), []).append((e, k))
    for members in groups.values():
        if len(members) < 2:
            continue
        if all(moved[e] for e, _ in members):
            total = np.zeros(3)
            for e, k in members:
                total = total + point(new_c, new_l, e, k)
            target = total / len(members)
        else:
            target = point(old_c, old_l, *members[0]).copy()
        for e, k in members:
            if moved[e]:
                point(new_c, new_l, e, k)[:] = target


def _number(x):
    return None if x is None or not math.isfinite(float(x)) else float(x)


def snap_edges(edge_dict, cameras, edge_maps_u8, detector, resolution=SAMPLE_RESOLUTION, capture_px=CAPTURE_PX,
               iterations=ITERATIONS, frames_ratio=EDGE_VISIBILITY_FRAMES_RATIO, min_constrained=MIN_CONSTRAINED,
               damping=DAMPING, step_cap=None, edge_threshold=EDGE_MAX_THRESHOLD, backend="gpu", device=None,
               budget_bytes=None, thin=False, occluder=None, depth_maps=None, depth_slack=EO.DEPTH_SLACK,
               depth_window=EO.DEPTH_WINDOW, near_clip=None):
    """edge_dict, cameras, edge_maps_u8, detector, resolution, edge_threshold, budget_bytes and thin as ``trim_edges`` takes
    them, and the same walk over the views: ``view_chunks``, ``detected_masks``, the optional ``thin_masks``, ``edt_squared``
    (the same seven bytes per pixel), then one ``snap_terms`` call per chunk into one pair of sums.  When all views fit one
    chunk the transform is computed once and kept over the iterations; otherwise it is RECOMPUTED in every pass, chunk by
    chunk -- the price of a budget that does not hold the scan.  The sums are bit for bit the same either way.

    ``iterations + 1`` passes: each of the first ``iterations`` takes a ``snap_step`` (``step_cap`` None: 4 x resolution) and
    a ``refit`` of the edges that take part; the last one only measures.  The samples keep the count and the parameters that
    ``sample_edges`` gives the edge as it came in.
      GATE   an edge takes part only if at least ``min_constrained`` of its samples are constrained in the first pass, and
             it has at least two samples; every other edge is returned bit for bit.
      GUARD  a snapped edge is accepted only if its rms residual -- sqrt(sum rr / sum views) over its constrained samples,
             in pixels -- is lower in the last pass than in the first; one that fails is returned bit for bit.
      SHARED ENDS  end control points that were bitwise equal before are bitwise equal after: the mean of their members'
             snapped ends, or the old point if any member's edge came back unchanged.
    THE DEFAULTS ARE UNTUNED (the drawn test scan only), a sample within ``capture_px`` of the wrong edge is pulled to it,
    and this is not a filter: see the module docstring.

    Depth (opt-in; ``occluder``, ``depth_maps``, ``depth_slack`` and ``depth_window`` with the meaning and the checks of
    ``score_edges`` and ``edge_support``, at most one of the first two): a view whose depth plane hides a sample gives it
    no term and no view (``snap_terms(depth=...)``).  The planes are built PER CHUNK inside the walk over the views, like
    the transform, in every pass (``edge_occlusion.ChunkDepth``, 8 bytes per pixel more); only when all views fit one chunk
    are they, like the transform, built once and kept.  The result then also holds "hidden": int32 [P] numpy array, the
    views that hide every sample of the edges AS THEY CAME IN (the first pass), every record of "edges" holds
    "hidden_views", their sum over the edge's samples, and "settings" the keys ``score_edges`` records.  With neither,
    nothing changes: no key is added.  Untuned, drawn solids only, concave edges can be hidden by their own faces, no
    near-plane clipping unless ``near_clip`` is given (ops/edge_occlusion.py).

    Returns {"edge_dict": the edges in the layout of ``get_parametric_edge`` (curves [Nc,4,3], lines [Nl,6], as lists; an
    unmoved edge holds the floats it came with), "edges": one record per edge -- kind, index within its kind, samples,
    constrained_share, moved, reason, rms_before and rms_after in pixels, mean_displacement and max_displacement of its
    samples --, "moved": bool [E], "settings"}."""
    SP._check_backend(backend)
    resolution, frames_ratio = _positive("resolution", resolution), SP._ratio01("frames_ratio", frames_ratio)
    min_constrained, damping = SP._ratio01("min_constrained", min_constrained), _positive("damping", damping)
    cap2 = capture_squared(capture_px)
    iterations = int(iterations)
    if iterations < 0:
        raise ValueError(f"iterations must be >= 0 (got {iterations})")
    step_cap = STEP_CAP_RESOLUTIONS * resolution if step_cap is None else _positive("step_cap", step_cap)
    lut = detected_lut(detector, edge_threshold)
    cameras, maps = check_edge_maps("snap_edges", cameras, edge_maps_u8)
    budget = check_budget("snap_edges", budget_bytes, BYTE_BUDGET)
    source = EO.ChunkDepth("snap_edges", cameras, occluder, depth_maps, depth_slack, depth_window, near_clip)
    old_c, old_l = SP._edge_arrays(edge_dict["curves_ctl_pts"], edge_dict["lines_end_pts"])
    pts0, off = SP.sample_edges(old_c, old_l, resolution)
    off = off.astype(np.int64)
    sizes = np.diff(off)
    E, Nc, P, V = len(sizes), len(old_c), int(off[-1]), len(cameras)
    if backend == "gpu":
        device = ES._device_for([], "snap_edges", device)
    source.to(backend, device)
    chunks = list(view_chunks(cameras, BYTES_PER_PIXEL + source.bytes_per_pixel, budget))

    def transform(sel):
        det = detected_masks(lut, maps, sel)
        if thin:
            det = thin_masks(det, backend=backend, device=device)
        return ES.edt_squared(det, backend=backend, device=device)

    kept = transform(chunks[0][2]) if len(chunks) == 1 else None   # one chunk: the transform is computed once
    kept_depth = source.planes(*chunks[0]) if source.gated and len(chunks) == 1 else None   # and so are the depth planes
    hidden_first = []   # the hidden counts of the first pass

    def measure(pts32):
        pts_b = torch.from_numpy(pts32).to(device) if backend == "gpu" else pts32
        out = (torch.zeros((P, TERMS), dtype=torch.float64, device=device if backend == "gpu" else None),
               torch.zeros((P,), dtype=torch.int32, device=device if backend == "gpu" else None))
        hid = torch.zeros((P,), dtype=torch.int32, device=out[1].device) if source.gated and not hidden_first else None
        for H, W, sel, intr, w2c in chunks:
            d2 = kept if kept is not None else transform(sel)
            if source.gated:   # the planes of this chunk, built inside the walk like the transform
                depth = kept_depth if kept_depth is not None else source.planes(H, W, sel, intr, w2c)
                snap_terms(pts_b, intr, w2c, d2, capture_px, backend=backend, out=out, depth=depth, slack=source.slack,
                           hidden_out=hid)
                del depth
            else:
                snap_terms(pts_b, intr, w2c, d2, capture_px, backend=backend, out=out)
            del d2
        if hid is not None:
            hidden_first.append(hid.cpu().numpy())
        return out[0].cpu().numpy(), out[1].cpu().numpy()

    cur_c, cur_l = old_c.copy(), old_l.copy()
    gate = np.zeros(E, bool)
    share = np.full(E, np.nan)
    rms_before = rms_after = np.full(E, np.nan)
    for it in range(iterations + 1):
        pos = _positions(cur_c, cur_l, sizes)
        terms, views = measure(pts0 if it == 0 else pos.astype(np.float32))
        delta, con = snap_step(pos, terms, views, V, frames_ratio, damping, step_cap)
        rms = _edge_rms(terms, views, con, off)
        if it == 0:
            with np.errstate(all="ignore"):
                share = np.where(sizes > 0, _edge_sums(con, off) / sizes, np.nan)
            gate = (sizes >= 2) & (share >= min_constrained)
            rms_before = rms
        if it == iterations:
            rms_after = rms
            break
        delta[~np.repeat(gate, sizes)] = 0.0
        cur_c, cur_l = refit(cur_c, cur_l, off, delta, edges=gate)
    with np.errstate(all="ignore"):
        moved = gate & (rms_after < rms_before) if iterations > 0 else np.zeros(E, bool)
    new_c, new_l = old_c.copy(), old_l.copy()
    new_c[moved[:Nc]], new_l[moved[Nc:]] = cur_c[moved[:Nc]], cur_l[moved[Nc:]]
    _share_ends(old_c, old_l, new_c, new_l, moved)
    shift = np.sqrt(((_positions(new_c, new_l, sizes) - _positions(old_c, old_l, sizes)) ** 2).sum(1))
    records = []
    for e in range(E):
        if moved[e]:
            reason = "snapped"
        elif sizes[e] < 2:
            reason = "fewer than two samples"
        elif not gate[e]:
            reason = f"gate: fewer than {min_constrained:g} of the samples are constrained"
        elif iterations == 0:
            reason = "no iteration"
        else:
            reason = "guard: the rms residual did not fall"
        seg = shift[off[e]:off[e + 1]]
        records.append({"kind": "curve" if e < Nc else "line", "index": int(e if e < Nc else e - Nc), "samples": int(sizes[e]),
                        "constrained_share": _number(share[e]), "moved": bool(moved[e]), "reason": reason,
                        "rms_before": _number(rms_before[e]), "rms_after": _number(rms_after[e]) if gate[e] else None,
                        "mean_displacement": float(seg.mean()) if seg.size else 0.0,
                        "max_displacement": float(seg.max()) if seg.size else 0.0})
        if source.gated:
            records[-1]["hidden_views"] = int(hidden_first[0][off[e]:off[e + 1]].sum())
    settings = {"detector": detector, "resolution": resolution, "capture_px": float(capture_px), "iterations": iterations,
                "frames_ratio": frames_ratio, "min_constrained": min_constrained, "damping": damping, "step_cap": step_cap,
                "edge_threshold": float(edge_threshold), "backend": backend, "views": V, "points": P,
                "chunks": len(chunks)}
    if thin:
        settings["thin"] = True
    settings.update(source.settings())
    out = {"edge_dict": {"curves_ctl_pts": new_c.tolist(), "lines_end_pts": new_l.reshape(-1, 6).tolist()},
           "edges": records, "moved": moved, "settings": settings}
    if source.gated:
        out["hidden"] = hidden_first[0]
    return out
