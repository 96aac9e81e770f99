"""Trimming extracted edges to the spans of their length that the images show (cgs_sample_support, include/curvegs.h;
csrc/edge_trim.hip).  The support check (ops/edge_support.py) gives one verdict per edge -- it removes, it never repairs:
an edge that overshoots a corner loses its whole length to the part that runs on, and so does a merged chord that runs
along a real edge for half its length.  This module tallies the same evidence per SAMPLE over the views, where
``support_counts`` tallies per (edge, view) over the samples, and cuts every edge down to its supported runs.  Opt-in;
the reference has no counterpart.

  sample_tally       int32 [P,1+T]: per sample the views that see it (the projection rule of ``cgs_project_points``, to
                     the letter) and, per tolerance, those of them in which its pixel (floor(u), floor(v)) lies within the
                     tolerance of a detected pixel (``edt_squared`` of the detected mask); ADDS to a tally handed in
  supported_samples  the frame rule per sample
  supported_spans    the supported runs of every edge, small gaps bridged, short runs dropped
  trim_geometry      the pieces of the edges over their spans: Bezier subdivision by the blossom, lines by interpolation
  trim_edges         the four on a scan's cameras and stored edge maps

Definitions, frozen; n = the samples of edge e, ``sample_edges`` places them at np.linspace(0, 1, n):
  sample i is SUPPORTED at t   iff tally[i,1+t] > ceil(frames_ratio * frames)   (the reference's frame rule,
                               ``para_edge.edge_visibility_frames``, the one ``support_verdict`` uses)
  a RUN                        a maximal range of consecutive supported samples of one edge
  the SPANS of an edge         its runs, two runs merged when at most max_gap unsupported samples separate them, and THEN
                               the runs of fewer than min_span samples dropped; inclusive index pairs (a, b) local to the edge
  the PIECE of a span (a, b)   the edge over [ta, tb] = [a / (n - 1), b / (n - 1)]: for a curve the control points
                               B(ta,ta,ta), B(ta,ta,tb), B(ta,tb,tb), B(tb,tb,tb) of its blossom B, for a line
                               p0 + t (p1 - p0) at ta and tb; a span (0, n - 1) is the edge itself, bit for bit

DEPTH (opt-in).  Without a depth source a stretch hidden behind a surface in most views is cut away,
and a hidden stretch collects hits it cannot have from the front edges it projects behind.  With ``depth``
(``sample_tally``) or ``occluder`` / ``depth_maps`` (``trim_edges``) a view whose depth plane hides the sample -- the one
rule of ops/edge_occlusion.py -- counts as not seeing it and is tallied in "hidden" instead; the frame rule itself does not
change.  Limits as ops/edge_occlusion.py states them: untuned, drawn solids only, concave edges, no near-plane clipping unless ``near_clip`` is given.

KNOWN LIMITS.  The pieces of a chord that runs along a real edge duplicate that edge; this module does not merge them
(ops/edge_dedupe.py, opt-in, drops what a longer edge already covers).  The tally asks how near a detected pixel is, not
which way the detected edge runs there, so a chord collects support where it crosses a real edge (``oriented=True``,
ops/edge_orient.py, opt-in, holds the edge's direction against the pixels' orientations).  The cut lands up to the tolerance plus a pixel
diagonal beyond the true end, because a sample just past the end still falls on a pixel near the drawn one.  THE
DEFAULTS OF ``trim_edges`` ARE UNTUNED: only the drawn test scan (tests/edge_trim_cases.py) has been checked, no real
scan.

Two back ends: ``"gpu"``, HIP, and ``"host"``, numpy -- the same rules in integers, so the tallies agree exactly; the
spans and the pieces are host arithmetic for both."""
import math

import numpy as np
import torch

from .. import _lib as L
from ..edge_extraction.para_edge import EDGE_MAX_THRESHOLD, EDGE_VISIBILITY_FRAMES_RATIO
from ..edge_extraction.reprojection import SAMPLE_RESOLUTION
from . import edge_occlusion as EO
from . import edge_orient as OR
from . import edge_score as ES
from . import edge_support as SP
from .edge_thin import thin_masks
from .view_chunks import check_budget, check_edge_maps, detected_lut, detected_masks, view_chunks

TRIM_BACKENDS = SP.SUPPORT_BACKENDS
BYTE_BUDGET = SP.BYTE_BUDGET
BYTES_PER_PIXEL = SP.BYTES_PER_PIXEL   # the working set of edge_support: one uint8 mask, one uint16 pass, one int32 transform
# UNTUNED, like the defaults of ops/edge_support.py: the drawn test scan only, no real scan
TOLERANCE_PX = 1
MAX_GAP = 3
MIN_SPAN = 10


# ------------------------------------------------------------------------------------------------ tally
def _tally_host(pts, K, M, d2, tol2, out, depth=None, slack=0.0, hidden=None):
    """``depth`` float32 [V,H,W] or None; ``hidden`` int32 [P] or None, added to when there is a depth."""
    H, W = d2.shape[1], d2.shape[2]
    for v in range(K.shape[0]):   # one view at a time: [P] temporaries
        if depth is None:
            u, w, keep = (x[0] for x in ES.project_points_host(pts, K[v:v + 1], M[v:v + 1], H, W))
        else:   # a view that hides the sample does not see it
            u, w, keep, hid = EO.gate_view_host(pts, K[v], M[v], depth[v], slack)
            if hidden is not None:
                hidden += hid
        d = np.full(pts.shape[0], ES.EDT_INF, np.int64)
        d[keep] = d2[v][np.floor(w[keep]).astype(np.int64), np.floor(u[keep]).astype(np.int64)]
        out[:, 0] += keep
        for t, t2 in enumerate(tol2):
            out[:, 1 + t] += keep & (d <= t2)
    return out


def sample_tally(points, intrinsics, w2c, d2, tolerances_px, backend="gpu", device=None, out=None, depth=None,
                 slack=EO.DEPTH_SLACK, hidden_out=None):
    """int32 [P,1+T].  points float32 [P,3]; intrinsics [V,4] = (fx, fy, cx, cy) and w2c [V,3,4] float64 host arrays or
    tensors; d2 int32 [V,H,W], ``edt_squared`` of every view's detected mask; 1 to 4 pixel tolerances, squared by
    ``edge_score.tolerances_squared`` -- the arguments of ``support_counts`` without the offsets.  tally[i,0] = the views in
    which ``cgs_project_points`` keeps point i; tally[i,1+t] = those of them with d2[v][floor(v)][floor(u)] <= floor(t^2).

    ``out``: a contiguous int32 [P,1+T] tensor that the counts are ADDED to and that is returned -- one call per chunk of
    views into the same tally; without it the counts of this call alone, in a new tensor.

    ``backend="gpu"``: ``cgs_sample_support``.  d2 must be on a GPU (CurveGSError otherwise), ``device``, when given, must
    be that GPU, and so must the device of ``out`` and of points that are on a GPU; points on the host are uploaded.  The
    result stays on the device.  ``backend="host"``: numpy, CPU tensors.

    ``depth`` (None: no gate, the call above and nothing else): float32 [V,H,W] of d2's size, camera z, +inf where there is
    no surface.  A view that keeps sample i HIDES it iff c2 > float64(depth[v][floor(v)][floor(u)]) + ``slack`` (finite,
    >= 0; ``cgs_sample_support_depth``): it counts in no column of the tally.  ``hidden_out`` (needs ``depth``): a contiguous
    int32 [P] tensor, on ``out``'s device, that the hiding views of every sample are ADDED to, as the tally is; tally[i,0] +
    hidden is the ungated tally[i,0].  depth on the host is uploaded for ``backend="gpu"``."""
    SP._check_backend(backend)
    tol2 = SP._tolerances(tolerances_px)
    pts = SP._points(points)
    V, K, M = ES._cameras(intrinsics, w2c)
    d2 = SP._d2(d2, V)
    P, T = int(pts.shape[0]), len(tol2)
    if out is not None:
        if not torch.is_tensor(out) or out.dtype != torch.int32 or tuple(out.shape) != (P, 1 + T) or not out.is_contiguous():
            raise ValueError(f"sample_tally: out must be a contiguous int32 [{P},{1 + T}] tensor")
    EO.check_hidden_out("sample_tally", hidden_out, depth, P)
    if backend == "host":
        SP._host_only("sample_tally", d2, pts, out, hidden_out)
        if out is None:
            out = torch.zeros((P, 1 + T), dtype=torch.int32)
        if depth is not None:
            depth, slack = EO.operator_depth("sample_tally", depth, slack, V, int(d2.shape[1]), int(d2.shape[2]), "host")
        _tally_host(pts.numpy(), K, M, d2.numpy(), tol2, out.numpy(), depth, slack,
                    None if hidden_out is None else hidden_out.numpy())
        return out
    dev = SP._one_device("sample_tally", "d2", d2, device, uploaded=[("points", pts)],
                         resident=[("out", [out]), ("hidden_out", [hidden_out])])
    with L.device_guard(dev):
        pts = pts.to(dev).contiguous()
        if out is None:
            out = torch.zeros((P, 1 + T), dtype=torch.int32, device=dev)
        if depth is not None:
            depth, slack = EO.operator_depth("sample_tally", depth, slack, V, int(d2.shape[1]), int(d2.shape[2]), "gpu", dev)
        if P > 0 and V > 0:
            tol_d = torch.tensor(tol2, dtype=torch.int32).to(dev)
            Kd, Md = ES.cameras_on(dev, K, M)
            args = [P, L.ptr(pts), V, L.ptr(Kd), L.ptr(Md), int(d2.shape[1]), int(d2.shape[2]), L.ptr(d2), T, L.ptr(tol_d)]
            if depth is None:
                L.check(L.load().cgs_sample_support(*args, L.ptr(out), L.raw_stream(dev)), "cgs_sample_support")
            else:
                L.check(L.load().cgs_sample_support_depth(*args, L.ptr(depth), slack, L.ptr(out), L.ptr(hidden_out),
                                                          L.raw_stream(dev)), "cgs_sample_support_depth")
    return out


# ------------------------------------------------------------------------------------------------ spans
def supported_samples(tally, frames, frames_ratio=EDGE_VISIBILITY_FRAMES_RATIO):
    """bool [P,T] (numpy): sample i is supported at tolerance t iff tally[i,1+t] > ceil(frames_ratio * frames); ``frames`` is
    the number of views the frame rule speaks of (V for a whole scan).  Host integers for either back end's tally."""
    c = ES._host(tally)
    if c.ndim != 2 or c.shape[1] < 2 or not np.issubdtype(c.dtype, np.integer):
        raise ValueError(f"tally must be an integer [P,1+T] array (got {c.dtype} {c.shape})")
    return c[:, 1:].astype(np.int64) > math.ceil(SP._ratio01("frames_ratio", frames_ratio) * int(frames))


def _span_options(max_gap, min_span):
    max_gap, min_span = int(max_gap), int(min_span)
    if max_gap < 0 or min_span < 2:
        raise ValueError(f"max_gap must be >= 0 and min_span >= 2 (got {max_gap}, {min_span})")
    return max_gap, min_span


def supported_spans(flags, offsets, max_gap=MAX_GAP, min_span=MIN_SPAN):
    """Per edge the list of its spans (a, b), inclusive sample indices local to the edge, ascending.  flags bool [P], one
    tolerance's column of ``supported_samples``; offsets int [E+1] as ``sample_edges`` gives them.  Maximal runs of supported
    samples; two runs of an edge that at most ``max_gap`` unsupported samples separate are merged; THEN runs of fewer than
    ``min_span`` samples are dropped.  Vectorised numpy."""
    max_gap, min_span = _span_options(max_gap, min_span)
    f = ES._host(flags)
    if f.ndim != 1 or f.dtype != bool:
        raise ValueError(f"flags must be bool [P] (got {f.dtype} {f.shape})")
    off = SP._offsets(offsets, f.size).astype(np.int64)
    E = off.size - 1
    edge = np.repeat(np.arange(E), np.diff(off))            # [P]: the edge of every sample
    cut = np.ones(f.size + 1, bool)                          # cut[i]: samples i - 1 and i do not belong to one run
    cut[1:-1] = (edge[1:] != edge[:-1]) | ~f[1:] | ~f[:-1]
    first = np.flatnonzero(f & cut[:-1])                     # [R]: the runs, in order
    last = np.flatnonzero(f & cut[1:])
    run_edge = edge[first]
    # run r and run r + 1 are merged when they belong to one edge and the gap between them is small
    joined = (run_edge[1:] == run_edge[:-1]) & (first[1:] - last[:-1] - 1 <= max_gap)
    head = np.concatenate([[True], ~joined]) if first.size else np.zeros(0, bool)
    tail = np.concatenate([~joined, [True]]) if first.size else np.zeros(0, bool)
    a, b, e = first[head], last[tail], run_edge[head]
    keep = b - a + 1 >= min_span
    a, b, e = a[keep] - off[e[keep]], b[keep] - off[e[keep]], e[keep]
    bounds = np.searchsorted(e, np.arange(E + 1))
    return [list(zip(a[bounds[k]:bounds[k + 1]].tolist(), b[bounds[k]:bounds[k + 1]].tolist())) for k in range(E)]


# ------------------------------------------------------------------------------------------------ geometry
def _blossom(c, t1, t2, t3):
    """B(t1, t2, t3) of the cubic Bezier curves c [k,4,3] at parameters [k]: de Casteljau with one parameter per level."""
    t1, t2, t3 = (t[:, None, None] for t in (t1, t2, t3))
    q = (1.0 - t1) * c[:, :-1] + t1 * c[:, 1:]
    r = (1.0 - t2) * q[:, :-1] + t2 * q[:, 1:]
    return ((1.0 - t3) * r[:, :-1] + t3 * r[:, 1:])[:, 0]


def trim_geometry(curves, lines, offsets, spans):
    """(curves float64 [k,4,3], lines float64 [m,2,3], source int64 [k+m]): the pieces of the edges (curves [Nc,4,3] or
    [Nc,12], then lines [Nl,2,3] or [Nl,6]; offsets int [E+1] of ``sample_edges``) over ``spans``, one list of (a, b) per
    edge as ``supported_spans`` gives them.  Pieces keep the order of their edges and then of a; ``source`` is the edge
    (curves first, then lines) each piece came from.  A span (0, n - 1) returns the edge unchanged, bit for bit -- it is not
    passed through the subdivision; an edge without a span yields nothing."""
    curves, lines = SP._edge_arrays(curves, lines)
    n = np.diff(ES._host(offsets).astype(np.int64))
    E, Nc = len(curves) + len(lines), len(curves)
    if n.size != E or len(spans) != E:
        raise ValueError(f"trim_geometry: {E} edges, {n.size} ranges of samples and {len(spans)} lists of spans")
    src = np.array([e for e in range(E) for _ in spans[e]], np.int64)
    ab = np.array([s for e in range(E) for s in spans[e]], np.int64).reshape(-1, 2)
    if (ab[:, 0] < 0).any() or (ab[:, 0] >= ab[:, 1]).any() or (ab[:, 1] >= n[src]).any():
        raise ValueError("trim_geometry: a span (a, b) needs 0 <= a < b <= n - 1")
    ta, tb = ab[:, 0] / (n[src] - 1), ab[:, 1] / (n[src] - 1)
    whole = (ab[:, 0] == 0) & (ab[:, 1] == n[src] - 1)
    k = int(np.count_nonzero(src < Nc))
    c, (a, b) = curves[src[:k]], (ta[:k], tb[:k])
    out_c = np.stack([_blossom(c, a, a, a), _blossom(c, a, a, b), _blossom(c, a, b, b), _blossom(c, b, b, b)], 1).reshape(-1, 4, 3)
    out_c[whole[:k]] = c[whole[:k]]
    l, (a, b) = lines[src[k:] - Nc], (ta[k:, None], tb[k:, None])
    d = l[:, 1] - l[:, 0]
    out_l = np.stack([l[:, 0] + a * d, l[:, 0] + b * d], 1).reshape(-1, 2, 3)
    out_l[whole[k:]] = l[whole[k:]]
    return out_c, out_l, src


# ------------------------------------------------------------------------------------------------ a scan
def trim_edges(edge_dict, cameras, edge_maps_u8, detector, resolution=SAMPLE_RESOLUTION, tolerance_px=TOLERANCE_PX,
               frames_ratio=EDGE_VISIBILITY_FRAMES_RATIO, max_gap=MAX_GAP, min_span=MIN_SPAN,
               edge_threshold=EDGE_MAX_THRESHOLD, backend="gpu", device=None, budget_bytes=None, thin=False, oriented=False,
               spread=OR.SPREAD, occluder=None, depth_maps=None, depth_slack=EO.DEPTH_SLACK, depth_window=EO.DEPTH_WINDOW,
               near_clip=None):
    """edge_dict, cameras, edge_maps_u8, detector, resolution, edge_threshold, budget_bytes and thin as ``edge_support``
    takes them, and the same walk over the views: ``view_chunks``, ``detected_masks``, the optional ``thin_masks``,
    ``edt_squared``, then one ``sample_tally`` call per chunk into one tally -- integers, so the chunking cannot change a bit.
    EVERY edge of edge_dict is trimmed, whatever ``edge_support`` says of it: the verdict drops over-long true edges whole,
    and those are the ones trimming exists for.  ``tolerance_px``: the one pixel tolerance; the frame rule counts all
    cameras.  THE DEFAULTS ARE UNTUNED (the drawn test scan only): see the module docstring.

    Depth (opt-in; ``occluder``, ``depth_maps``, ``depth_slack`` and ``depth_window`` with the meaning and the checks of
    ``score_edges`` and ``edge_support``, at most one of the first two): every chunk gets its depth planes
    (``edge_occlusion.ChunkDepth``, 8 bytes per pixel more) and ``sample_tally`` / ``oriented_tally`` hold every sample
    against them: a view that hides a sample does not see it -- with ``oriented`` the sample alone is gated, its partner
    gives a direction only.  The frame rule is the frozen one; only the tally changes.  The result then also holds "hidden":
    int32 [P] CPU tensor, the hiding views of every sample, and "settings" the keys ``score_edges`` records.  With neither,
    nothing changes: no key is added.  Untuned, drawn solids only, concave edges can be hidden by their own faces, no
    near-plane clipping unless ``near_clip`` is given (ops/edge_occlusion.py).

    ``oriented=True`` (off by default; ops/edge_orient.py freezes the rule and states its limits) counts a sample as near
    only where a detected pixel within the tolerance runs the way the sample's edge does, to within ``spread`` octants of
    22.5 degrees: the walk is ``detected_masks``, the optional ``thin_masks``, ``mask_orientation``, ``oriented_near`` (a
    tolerance of at most 4 pixels) and one ``oriented_tally`` call per chunk -- no distance transform, three bytes per pixel.
    "settings" then records "oriented" and "spread".  With oriented=False nothing changes by a byte.

    Returns {"tally": int32 [P,2] CPU tensor, "offsets": int32 [E+1], "spans": per edge its list of (a, b), "edge_dict": the
    pieces in the layout of ``get_parametric_edge`` (curves [k,4,3], lines [m,6], as lists), "source": int64 [k+m], the
    edge each piece came from (curves first, then lines), "settings"}."""
    SP._check_backend(backend)
    resolution, tolerance_px, frames_ratio = float(resolution), float(tolerance_px), SP._ratio01("frames_ratio", frames_ratio)
    SP._tolerances([tolerance_px])
    max_gap, min_span = _span_options(max_gap, min_span)
    lut = detected_lut(detector, edge_threshold)
    cameras, maps = check_edge_maps("trim_edges", cameras, edge_maps_u8)
    budget = check_budget("trim_edges", budget_bytes, BYTE_BUDGET)
    gate = EO.ChunkDepth("trim_edges", cameras, occluder, depth_maps, depth_slack, depth_window, near_clip)
    curves, lines = SP._edge_arrays(edge_dict["curves_ctl_pts"], edge_dict["lines_end_pts"])
    pts, off = SP.sample_edges(curves, lines, resolution)
    V = len(cameras)
    if backend == "gpu":
        device = ES._device_for([], "trim_edges", device)
        pts_b = torch.from_numpy(pts).to(device)
    else:
        pts_b = pts
    gate.to(backend, device)
    tally = torch.zeros((pts.shape[0], 2), dtype=torch.int32, device=device if backend == "gpu" else None)
    hidden = torch.zeros((pts.shape[0],), dtype=torch.int32, device=tally.device) if gate.gated else None
    if oriented:
        spread = OR._spread(spread)
        OR._tol2(tolerance_px)
        partner = OR.sample_partners(off)
        partner_b = torch.from_numpy(partner).to(device) if backend == "gpu" else partner
    per_pixel = (OR.BYTES_PER_PIXEL if oriented else BYTES_PER_PIXEL) + gate.bytes_per_pixel
    for H, W, sel, intr, w2c in view_chunks(cameras, per_pixel, budget):
        gated = dict(depth=gate.planes(H, W, sel, intr, w2c), slack=gate.slack, hidden_out=hidden) if gate.gated else {}
        det = detected_masks(lut, maps, sel)
        if thin:
            det = thin_masks(det, backend=backend, device=device)
        if oriented:
            near = OR.oriented_near(OR.mask_orientation(det, backend=backend, device=device), tolerance_px, backend=backend,
                                    device=device)
            del det
            OR.oriented_tally(pts_b, partner_b, intr, w2c, near, spread, backend=backend, out=tally, **gated)
            del near, gated
            continue
        d2 = ES.edt_squared(det, backend=backend, device=device)
        del det
        sample_tally(pts_b, intr, w2c, d2, [tolerance_px], backend=backend, out=tally, **gated)
        del d2, gated
    tally = tally.cpu()
    spans = supported_spans(supported_samples(tally, V, frames_ratio)[:, 0], off, max_gap, min_span)
    out_c, out_l, source = trim_geometry(curves, lines, off, spans)
    settings = {"detector": detector, "resolution": resolution, "tolerance_px": tolerance_px, "frames_ratio": frames_ratio,
                "max_gap": max_gap, "min_span": min_span, "edge_threshold": float(edge_threshold), "backend": backend,
                "views": V, "points": int(pts.shape[0])}
    if thin:
        settings["thin"] = True
    if oriented:
        settings.update({"oriented": True, "spread": spread})
    settings.update(gate.settings())
    out = {"tally": tally, "offsets": off, "spans": spans,
           "edge_dict": {"curves_ctl_pts": out_c.tolist(), "lines_end_pts": out_l.reshape(-1, 6).tolist()},
           "source": source, "settings": settings}
    if gate.gated:
        out["hidden"] = hidden.cpu()
    return out
