"""Dropping the extracted edges, or the parts of them, that a longer edge already covers (cgs_sample_cover,
include/curvegs.h; csrc/edge_dedupe.hip).  After trimming (ops/edge_trim.py) the pieces of a chord that runs along a real
edge describe that edge a second or third time, and every copy counts against precision in the ABC metrics and in the
reprojection score.  This module tests every sample of the edges against every sample of every LONGER edge in 3D -- near
and running the same way -- and cuts each edge down to the runs of its samples that no longer edge covers.  Opt-in; the
reference has no counterpart: its ``merge_endpoints`` only snaps end points, and the training-time ``merge_curves`` works
on the model, not on an exported edge file.

  edge_ranks         the priority of every edge: the longest edge has rank 0
  sample_cover       int32 [P]: per sample the best rank among the samples that cover it, NO_COVER when there is none
  redundant_samples  the covered samples, short runs of them cleared
  dedupe_edges       the three on an edge dict, and the pieces of what is left (``edge_trim.trim_geometry``)

Definitions, frozen.  "float32" is IEEE single precision, one rounded operation at a time in the written
order, nothing contracted into an FMA: numpy float32 arrays and the kernel agree bit for bit.
  SAMPLES     pts, off = ``sample_edges(curves, lines, resolution)``; n[e] = off[e+1] - off[e]
  RANK        a permutation of 0..E-1: the edges by descending n[e], ties by ascending edge index; rank 0 is the longest
  TANGENT     of sample i, the k-th of edge e:  t_i = pts[off[e] + min(k+1, n-1)] - pts[off[e] + max(k-1, 0)] and
              q_i = (t.x*t.x + t.y*t.y) + t.z*t.z.  An edge of ONE sample has t = 0: the direction test below then reads
              0 >= 0 and passes, so such a sample covers, and is covered, on distance and rank alone
  COVERS      sample j of edge b covers sample i of edge a iff
                1. rank[b] < rank[a]                      (strict: an edge never covers itself)
                2. (dx*dx + dy*dy) + dz*dz <= tol2        dx = p_i.x - p_j.x ...; tol2 = float32(tolerance)^2
                3. dot*dot >= (cos2 * q_i) * q_j          dot = (t_i.x*t_j.x + t_i.y*t_j.y) + t_i.z*t_j.z;
                                                          cos2 = float32(cos_min)^2
  COVER       cover[i] = the least rank[b] over the samples that cover i, NO_COVER = INT32_MAX when there is none
  REDUNDANT   cover[i] != NO_COVER, and then the maximal runs of such samples of one edge that are shorter than min_run
              are cleared: ``supported_spans(raw, off, 0, min_run)`` painted back onto the samples
  PIECES      spans = ``supported_spans(~redundant, off, 0, min_span)``, cut by ``trim_geometry``, unchanged: an edge
              without a redundant sample comes back bit for bit, one whose free runs are all shorter than min_span disappears

Without the direction test a lower-ranked edge loses its end at every junction (two lines that share an end point at 90
degrees overlap by tolerance / resolution samples); with cos_min = 0.9, junctions at 90, 60 and 30 degrees lose no sample.

KNOWN LIMITS.  A longer duplicate always wins, even when the shorter edge is the true one.  Coverage is one pass: a coverer
that is itself cut still covers.  Edges that meet at less than acos(cos_min) (about 26 degrees at 0.9) cut each other near
the junction: a 15 degree junction loses 8 samples at a tolerance of 2 x the resolution and 31 at 8 x.  There is no image
evidence here, this is 3D only.  Whether deduped edges score better on ABC has not been measured.  THE DEFAULTS ARE UNTUNED:
only drawn fixtures (tests/edge_dedupe_cases.py) have been looked at, no real scan.

Two back ends: ``"gpu"``, HIP, and ``"host"``, numpy in chunks of queries, so memory stays O(chunk x P)."""
import numpy as np
import torch

from .. import _lib as L
from ..edge_extraction.reprojection import SAMPLE_RESOLUTION
from . import edge_score as ES
from . import edge_support as SP
from . import edge_trim as ET

DEDUPE_BACKENDS = SP.SUPPORT_BACKENDS
NO_COVER = int(np.iinfo(np.int32).max)
# UNTUNED: drawn fixtures only
TOLERANCE_RESOLUTIONS = 2.0   # the default tolerance, in units of the sampling resolution
COS_MIN = 0.9
MIN_RUN = 3
MIN_SPAN = ET.MIN_SPAN
HOST_CHUNK = 256              # queries per step of the host back end


def _check_backend(backend):
    if backend not in DEDUPE_BACKENDS:
        raise ValueError(f"unknown edge dedupe backend {backend!r}: expected one of {DEDUPE_BACKENDS}")


def _squares(tolerance, cos_min):
    """(tol2, cos2) as float32, formed once: float32(x) * float32(x)."""
    tolerance, cos_min = float(tolerance), float(cos_min)
    if not tolerance > 0.0 or not np.isfinite(tolerance):
        raise ValueError(f"tolerance must be a positive number (got {tolerance})")
    if not 0.0 <= cos_min <= 1.0:
        raise ValueError(f"cos_min must lie in [0, 1] (got {cos_min})")
    return np.float32(tolerance) * np.float32(tolerance), np.float32(cos_min) * np.float32(cos_min)


def _run_options(min_run, min_span):
    min_run, min_span = int(min_run), int(min_span)
    if min_run < 2 or min_span < 2:
        raise ValueError(f"min_run and min_span must be >= 2 (got {min_run}, {min_span})")
    return min_run, min_span


def edge_ranks(offsets):
    """int32 [E]: rank[e] of every edge, from offsets int [E+1] as ``sample_edges`` gives them.  The edges ordered by
    descending sample count, ties by ascending edge index (``np.lexsort((arange(E), -n))``); rank 0 is the longest edge, an
    edge without samples ranks behind every edge that has some."""
    off = ES._host(offsets)
    off = SP._offsets(off, int(off[-1]) if off.ndim == 1 and off.size else 0).astype(np.int64)
    n = np.diff(off)
    order = np.lexsort((np.arange(n.size), -n))
    ranks = np.empty(n.size, np.int32)
    ranks[order] = np.arange(n.size, dtype=np.int32)
    return ranks


def _ranks(ranks, E):
    r = ES._host(ranks)
    if r.ndim != 1 or r.size != E or not np.issubdtype(r.dtype, np.integer):
        raise ValueError(f"ranks must be an integer [E] array with E = {E} edges (got {r.dtype} {r.shape})")
    if not np.array_equal(np.sort(r.astype(np.int64)), np.arange(E)):
        raise ValueError(f"ranks must be a permutation of 0 .. {E - 1}")
    return np.ascontiguousarray(r.astype(np.int32))


def _tangents(pts, off):
    """(t float32 [P,3], q float32 [P]) of the samples."""
    P = pts.shape[0]
    n = np.diff(off.astype(np.int64))
    first = np.repeat(off[:-1].astype(np.int64), n)
    count = np.repeat(n, n)
    k = np.arange(P, dtype=np.int64) - first
    t = pts[first + np.minimum(k + 1, count - 1)] - pts[first + np.maximum(k - 1, 0)]
    return t, (t[:, 0] * t[:, 0] + t[:, 1] * t[:, 1]) + t[:, 2] * t[:, 2]


def _cover_host(pts, off, ranks, tol2, cos2, chunk=HOST_CHUNK):
    P = pts.shape[0]
    t, q = _tangents(pts, off)
    r = np.repeat(ranks, np.diff(off.astype(np.int64)))   # [P]: the rank of every sample's edge
    cover = np.full(P, NO_COVER, np.int32)
    for c0 in range(0, P, chunk):
        c = slice(c0, min(P, c0 + chunk))
        dx, dy, dz = (pts[c, a, None] - pts[None, :, a] for a in range(3))
        d2 = (dx * dx + dy * dy) + dz * dz
        dot = (t[c, 0, None] * t[None, :, 0] + t[c, 1, None] * t[None, :, 1]) + t[c, 2, None] * t[None, :, 2]
        covers = (r[None, :] < r[c, None]) & (d2 <= tol2) & (dot * dot >= (cos2 * q[c, None]) * q[None, :])
        cover[c] = np.where(covers, r[None, :], NO_COVER).min(1)
    return cover


def sample_cover(points, offsets, ranks, tolerance, cos_min, backend="gpu", device=None):
    """int32 [P]: cover[i] as the module docstring defines it.  points float32 [P,3], finite (ValueError otherwise: the
    kernel never sees a NaN); offsets int [E+1] as ``sample_edges`` gives them; ranks int [E], a permutation of 0..E-1
    (``edge_ranks``); tolerance > 0 in the units of the points; cos_min in [0, 1].

    ``backend="gpu"``: ``cgs_sample_cover``.  points may be a host array, which is uploaded to ``device`` (default: the
    current GPU), or a tensor, which must then be a contiguous GPU tensor (CurveGSError otherwise); ``device``, when given,
    and offsets or ranks that are GPU tensors must be on that GPU (CurveGSError).  The result stays on the device.  The call
    is NOT asynchronous: offsets and ranks are checked on the host (GPU tensors are copied back for that, which
    synchronises, and uploaded again), and so is the finiteness of the points (one reduction read back).
    ``backend="host"``: numpy, ``HOST_CHUNK`` queries at a time; host arrays and CPU tensors; a CPU tensor comes back."""
    _check_backend(backend)
    tol2, cos2 = _squares(tolerance, cos_min)
    pts = SP._points(points)
    P = int(pts.shape[0])
    off = SP._offsets(offsets, P)
    rk = _ranks(ranks, off.size - 1)
    if P > np.iinfo(np.int32).max:
        raise ValueError(f"sample_cover: {P} samples: at most 2^31 - 1")
    if not bool(torch.isfinite(pts).all()):
        raise ValueError("sample_cover: points must be finite")
    if backend == "host":
        if pts.is_cuda:
            raise ValueError("sample_cover: backend='host' takes host arrays and CPU tensors")
        return torch.from_numpy(_cover_host(np.ascontiguousarray(pts.numpy()), off, rk, tol2, cos2))
    if torch.is_tensor(points):
        L.require_gpu_tensor(pts, "sample_cover: points")
        if not pts.is_contiguous():
            raise L.CurveGSError("sample_cover: points must be contiguous")
    dev = ES._device_for([pts], "sample_cover", None if pts.is_cuda else device)
    if device is not None and torch.device(device) != dev and torch.device(device) != torch.device(dev.type):
        raise L.CurveGSError(f"sample_cover: points are on {dev}, device={device}: all tensors must be on one device")
    for name, x in (("offsets", offsets), ("ranks", ranks)):
        if torch.is_tensor(x) and x.is_cuda and x.device != dev:
            raise L.CurveGSError(f"sample_cover: {name} are on {x.device}, points on {dev}: all tensors must be on one device")
    with L.device_guard(dev):
        cover = torch.full((P,), NO_COVER, dtype=torch.int32, device=dev)
        if P > 0:
            lib = L.load()
            pts = pts.to(dev)
            off_d, rk_d = torch.from_numpy(off).to(dev), torch.from_numpy(rk).to(dev)
            work = torch.empty(int(lib.cgs_sample_cover_workspace_bytes(P)), dtype=torch.uint8, device=dev)
            rc = lib.cgs_sample_cover(P, L.ptr(pts), int(rk.size), L.ptr(off_d), L.ptr(rk_d), float(tol2), float(cos2),
                                      L.ptr(cover), L.ptr(work), L.raw_stream(dev))
            L.check(rc, "cgs_sample_cover")
    return cover


def redundant_samples(cover, offsets, min_run=MIN_RUN):
    """bool [P] (numpy): sample i is redundant iff cover[i] != NO_COVER and it belongs to a maximal run of at least
    ``min_run`` (>= 2) such samples of its edge; runs never join across edges.  Host integers for either back end's cover."""
    min_run, _ = _run_options(min_run, 2)
    c = ES._host(cover)
    if c.ndim != 1 or c.dtype != np.int32:
        raise ValueError(f"cover must be int32 [P] (got {c.dtype} {c.shape})")
    off = SP._offsets(offsets, c.size).astype(np.int64)
    out = np.zeros(c.size, bool)
    for e, spans in enumerate(ET.supported_spans(c != NO_COVER, off, 0, min_run)):
        for a, b in spans:
            out[off[e] + a:off[e] + b + 1] = True
    return out


def dedupe_edges(edge_dict, resolution=SAMPLE_RESOLUTION, tolerance=None, cos_min=COS_MIN, min_run=MIN_RUN,
                 min_span=MIN_SPAN, backend="gpu", device=None):
    """Every edge of ``edge_dict`` (the layout of ``get_parametric_edge``) cut down to the runs of its samples that no longer
    edge covers: ``sample_edges`` at ``resolution``, ``edge_ranks``, ``sample_cover``, ``redundant_samples``, then the free
    runs of at least ``min_span`` samples (``supported_spans`` with max_gap 0) cut by ``trim_geometry``.  ``tolerance``: in
    the units of the edges, default ``TOLERANCE_RESOLUTIONS`` x resolution.  THE DEFAULTS ARE UNTUNED and the limits are
    those of the module docstring.

    Returns {"cover": int32 [P] CPU tensor, "offsets": int32 [E+1], "ranks": int32 [E], "redundant": bool [P], "spans": per
    edge its list of (a, b), "edge_dict": the pieces (curves [k,4,3], lines [m,6], as lists), "source": int64 [k+m], the
    edge each piece came from (curves first, then lines), "covered_by": per edge the sorted indices of the edges that
    ``cover`` names for its redundant samples -- the best-ranked coverer of each; a second, lower-ranked coverer of a sample
    is not listed --, "settings"}."""
    _check_backend(backend)
    resolution = float(resolution)
    tolerance = TOLERANCE_RESOLUTIONS * resolution if tolerance is None else float(tolerance)
    _squares(tolerance, cos_min)
    min_run, min_span = _run_options(min_run, min_span)
    curves, lines = SP._edge_arrays(edge_dict["curves_ctl_pts"], edge_dict["lines_end_pts"])
    pts, off = SP.sample_edges(curves, lines, resolution)
    ranks = edge_ranks(off)
    cover = sample_cover(pts, off, ranks, tolerance, cos_min, backend=backend, device=device).cpu()
    redundant = redundant_samples(cover, off, min_run)
    spans = ET.supported_spans(~redundant, off, 0, min_span)
    out_c, out_l, source = ET.trim_geometry(curves, lines, off, spans)
    edge_of_rank = np.argsort(ranks)
    c = cover.numpy()
    covered_by = [sorted({int(x) for x in edge_of_rank[c[off[e]:off[e + 1]][redundant[off[e]:off[e + 1]]]]})
                  for e in range(len(ranks))]
    settings = {"resolution": resolution, "tolerance": tolerance, "cos_min": float(cos_min), "min_run": min_run,
                "min_span": min_span, "backend": backend, "points": int(pts.shape[0])}
    return {"cover": cover, "offsets": off, "ranks": ranks, "redundant": redundant, "spans": spans,
            "edge_dict": {"curves_ctl_pts": out_c.tolist(), "lines_end_pts": out_l.reshape(-1, 6).tolist()},
            "source": source, "covered_by": covered_by, "settings": settings}
