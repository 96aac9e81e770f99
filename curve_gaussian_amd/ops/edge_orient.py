"""Orientation-aware 2D support (cgs_mask_orientation, cgs_oriented_near, cgs_sample_support_oriented, include/curvegs.h;
csrc/edge_orient.hip).  Every 2D check of the extraction chain asks whether a projected sample lies within a few pixels of a
detected pixel; none asks whether the edge runs the way the detected edge runs, so a bogus chord that crosses a real edge
collects full support near the crossing and trimming leaves a stub there.  This module gives every detected pixel an
orientation code and tallies per sample with the direction of the sample's own edge held against the codes nearby.  Opt-in
(``trim_edges(oriented=True)``); the reference has no counterpart.

  mask_orientation   uint8 [V,H,W]: the orientation code of every pixel of the detected masks
  oriented_near      uint8 [V,H,W]: the OR of the codes over the tolerance disk -- which orientations lie within reach
  sample_partners    int32 [P]: per sample the neighbour on its edge that gives it a direction
  oriented_tally     int32 [P,2]: per sample the views that see it and those in which an orientation within reach agrees
                     with the direction to its partner; ADDS to a tally handed in

The rule, frozen; x runs to the right and y down.

octant(a, b) for (a, b) != (0, 0), the half-open octant of the doubled angle, by signs and one comparison of magnitudes:
  a >  0, b >= 0:  0 if |b| < |a| else 1          a <  0, b <= 0:  4 if |b| < |a| else 5
  a <= 0, b >  0:  2 if |b| > |a| else 3          a >= 0, b <  0:  6 if |b| > |a| else 7
Bin k is a line orientation in [22.5 k, 22.5 (k + 1)) degrees: a horizontal line gives 0, the line y = x gives 2, a vertical
line 4, the line y = -x gives 6.

The CODE of a pixel, from its view's detected mask (nonzero = set, pixels outside the image are unset): 0 for an unset
pixel.  For a set pixel, over the set pixels of its window (dx, dy) in [-R, R]^2, R = 3, in integers:
  N = sum 1, Sx = sum dx, Sy = sum dy, Sxx = sum dx dx, Syy = sum dy dy, Sxy = sum dx dy
  A = N Sxx - Sx Sx,  B = N Sxy - Sx Sy,  C = N Syy - Sy Sy,  a = A - C,  b = 2 B
  the pixel is ORIENTED iff N >= 3 and (a, b) != (0, 0) and 4 (a a + b b) >= (A + C)(A + C)   (a coherence of at least 0.5)
  code = 1 << octant(a, b) when oriented, else 0xFF: it accepts every direction
A + C <= 49 * 392 and a a + b b <= (A + C)^2 (B B <= A C), so 4 (a a + b b) < 2^31: the kernel computes in 32 bits.

NEAR: near[v][y][x] = the OR of code[v][y + dy][x + dx] over dx dx + dy dy <= tol2, tol2 = floor(tolerance_px^2) as
``edge_score.tolerances_squared`` gives it, 0 <= tol2 <= 16.  near != 0 iff ``edt_squared`` of the mask is <= tol2: the
oriented path needs no distance transform.

The PARTNER of sample i is i + 1, or i - 1 when i is the last sample of its edge; an edge of one sample has partner[i] = i,
which means none.

The TALLY: SEEN is the rule of ``cgs_project_points`` (float64, nothing contracted).  For a sample seen at (u, v), pixel
(floor(u), floor(v)), the accepted orientations are acc = 0xFF when partner[i] == i, when the partner lies outside [0, P) or
when the partner is not seen in this view.  Otherwise dx = u_p - u, dy = v_p - v, a = dx dx - dy dy, b = 2 (dx dy) in float64,
one rounded operation at a time, in this order; (a, b) == (0, 0) gives acc = 0xFF and any other (a, b) the bits
(octant(a, b) + s) mod 8 for s = -spread .. spread, 0 <= spread <= 4 (4: all bits).  spread = 1 accepts every pair of
orientations nearer than 22.5 degrees and refuses every pair further than 45.
  tally[i][0] += the views that see sample i,   tally[i][1] += those of them with (near[v][pixel] & acc) != 0

KNOWN LIMITS.  The orientation comes from a BINARY MASK in a 7 x 7 window: a stroke wider than about 3 pixels is isotropic
there, its pixels get 0xFF and the test falls back to the plain distance test -- thin such maps first (``thin=True``,
ops/edge_thin.py).  Corners and junctions accept everything, so a chord still collects support where it crosses one.  There
is no depth unless the caller gives one: ``oriented_tally(depth=...)`` (``trim_edges(oriented=True, occluder=...)``) gates THE
SAMPLE by the one rule of ops/edge_occlusion.py -- a view that hides it does not see it -- while its partner gives a
direction only and is never held against the depth (``cgs_sample_support_oriented_depth``).  THE DEFAULTS (R = 3, coherence 0.5, spread 1) ARE UNTUNED: drawn fixtures only
(tests/edge_orient_cases.py), unmeasured on ABC or any real detector output.

Two back ends: ``"gpu"``, HIP, and ``"host"``, numpy -- the same rule, so they agree on every bit."""
import numpy as np
import torch

from .. import _lib as L
from . import edge_occlusion as EO
from . import edge_score as ES
from . import edge_support as SP

ORIENT_BACKENDS = ES.SCORE_BACKENDS
RADIUS = L.ORIENT_RADIUS
MAX_TOL2 = L.ORIENT_MAX_TOL2
MAX_SPREAD = L.ORIENT_MAX_SPREAD
TILE_HEIGHT, TILE_WIDTH = L.ORIENT_TILE_HEIGHT, L.ORIENT_TILE_WIDTH   # the kernels' tile
SPREAD = 1               # UNTUNED: see the module docstring
BYTES_PER_PIXEL = 3      # the working set of the oriented walk: one uint8 mask, one uint8 code, one uint8 near


def _check_backend(backend):
    if backend not in ORIENT_BACKENDS:
        raise ValueError(f"unknown edge orientation backend {backend!r}: expected one of {ORIENT_BACKENDS}")


def _spread(spread):
    s = int(spread)
    if s != spread or not (0 <= s <= MAX_SPREAD):
        raise ValueError(f"spread must be an integer in [0, {MAX_SPREAD}] (got {spread})")
    return s


def _tol2(tolerance_px):
    tol2 = ES.tolerances_squared([tolerance_px])[0]
    if tol2 > MAX_TOL2:
        raise ValueError(f"oriented_near: a tolerance of at most {int(np.sqrt(MAX_TOL2))} pixels (got {tolerance_px})")
    return tol2


# ------------------------------------------------------------------------------------------------ the rule on the host
def octant_host(a, b):
    """The octant of the module docstring for arrays a, b (integers or float64); where (a, b) == (0, 0) the value is 7 and
    means nothing."""
    a, b = np.asarray(a), np.asarray(b)
    ma, mb = np.abs(a), np.abs(b)
    return np.where((a > 0) & (b >= 0), np.where(mb < ma, 0, 1),
                    np.where((a <= 0) & (b > 0), np.where(mb > ma, 2, 3),
                             np.where((a < 0) & (b <= 0), np.where(mb < ma, 4, 5), np.where(mb > ma, 6, 7))))


def accept_bits_host(o, spread):
    """uint8: the bits (o + s) mod 8 for s = -spread .. spread, for an array of octants."""
    band = 0xFF if spread >= 4 else (1 << (2 * spread + 1)) - 1
    sh = (np.asarray(o, np.int64) - spread) & 7
    return (((band << sh) | (band >> (8 - sh))) & 0xFF).astype(np.uint8)


def mask_orientation_host(mask):
    """One view, numpy int64: uint8 [H,W]."""
    m = np.asarray(mask) != 0
    H, W = m.shape
    p = np.pad(m, RADIUS).astype(np.int64)
    N, Sx, Sy, Sxx, Syy, Sxy = (np.zeros((H, W), np.int64) for _ in range(6))
    for dy in range(-RADIUS, RADIUS + 1):
        for dx in range(-RADIUS, RADIUS + 1):
            s = p[RADIUS + dy:RADIUS + dy + H, RADIUS + dx:RADIUS + dx + W]
            N += s
            Sx += dx * s
            Sy += dy * s
            Sxx += dx * dx * s
            Syy += dy * dy * s
            Sxy += dx * dy * s
    A, B, C = N * Sxx - Sx * Sx, N * Sxy - Sx * Sy, N * Syy - Sy * Sy
    a, b = A - C, 2 * B
    oriented = (N >= 3) & ((a != 0) | (b != 0)) & (4 * (a * a + b * b) >= (A + C) * (A + C))
    code = np.where(oriented, 1 << octant_host(a, b), 0xFF)
    return np.where(m, code, 0).astype(np.uint8)


def oriented_near_host(code, tol2):
    """One view, numpy: uint8 [H,W]."""
    code = np.asarray(code, np.uint8)
    H, W = code.shape
    r = int(np.floor(np.sqrt(tol2)))
    p = np.pad(code, r)
    out = np.zeros((H, W), np.uint8)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            if dx * dx + dy * dy <= tol2:
                out |= p[r + dy:r + dy + H, r + dx:r + dx + W]
    return out


def _tally_host(pts, partner, K, M, near, spread, out, depth=None, slack=0.0, hidden=None):
    """``depth`` float32 [V,H,W] or None; ``hidden`` int32 [P] or None, added to when there is a depth."""
    P = pts.shape[0]
    H, W = near.shape[1], near.shape[2]
    i = np.arange(P, dtype=np.int64)
    j = partner.astype(np.int64)
    paired = (j != i) & (j >= 0) & (j < P)
    other = pts[np.where(paired, j, i)]
    for v in range(K.shape[0]):   # one view at a time: [P] temporaries
        if depth is None:
            u, w, keep = (x[0] for x in ES.project_points_host(pts, K[v:v + 1], M[v:v + 1], H, W))
        else:   # the sample is gated; the partner below is not
            u, w, keep, hid = EO.gate_view_host(pts, K[v], M[v], depth[v], slack)
            if hidden is not None:
                hidden += hid
        up, wp, keep_p = (x[0] for x in ES.project_points_host(other, K[v:v + 1], M[v:v + 1], H, W))
        with np.errstate(all="ignore"):   # a sample or a partner that is not seen may project to anything
            dx, dy = up - u, wp - w
            a, b = dx * dx - dy * dy, 2.0 * (dx * dy)
        directed = keep & paired & keep_p & ((a != 0.0) | (b != 0.0))
        acc = np.full(P, 0xFF, np.uint8)
        acc[directed] = accept_bits_host(octant_host(a[directed], b[directed]), spread)
        n = np.zeros(P, np.uint8)
        n[keep] = near[v][np.floor(w[keep]).astype(np.int64), np.floor(u[keep]).astype(np.int64)]
        out[:, 0] += keep
        out[:, 1] += keep & ((n & acc) != 0)
    return out


# ------------------------------------------------------------------------------------------------ the planes
def _planes(name, planes, backend, device, host_fn, entry):
    V, H, W = (int(s) for s in planes.shape)
    if backend == "host":
        m = ES._host(planes)
        out = np.empty((V, H, W), np.uint8)
        for v in range(V):   # the views are independent
            out[v] = host_fn(m[v])
        return torch.from_numpy(out)
    dev = ES._device_for([planes], name, device)
    with L.device_guard(dev):
        planes = planes.to(dev)
        out = torch.empty((V, H, W), dtype=torch.uint8, device=dev)
        if V > 0:
            L.check(entry(L.load(), V, H, W, L.ptr(planes), L.ptr(out), L.raw_stream(dev)), "cgs_" + name)
    return out


def mask_orientation(masks, backend="gpu", device=None):
    """masks: uint8 or bool [V,H,W] (a tensor or an array), nonzero = set.  Returns uint8 [V,H,W], the orientation code of
    every pixel by the rule of the module docstring: 0 for an unset pixel, one bit for an oriented one, 0xFF otherwise.  H and
    W lie in [1, 16384].  ``backend="gpu"``: ``cgs_mask_orientation`` (masks not on a GPU are uploaded; ``device``: which
    GPU), the result stays on the device.  ``backend="host"``: numpy, a CPU tensor."""
    _check_backend(backend)
    masks = ES._as_masks(masks, "mask_orientation: masks")
    return _planes("mask_orientation", masks, backend, device, mask_orientation_host,
                   lambda lib, V, H, W, src, dst, s: lib.cgs_mask_orientation(V, H, W, src, dst, s))


def oriented_near(codes, tolerance_px, backend="gpu", device=None):
    """codes: uint8 [V,H,W], the result of ``mask_orientation``.  Returns uint8 [V,H,W]: the OR of the codes within
    ``tolerance_px`` pixels of every pixel (at most 4; squared and floored as ``edge_score.tolerances_squared`` does it).
    ``backend="gpu"``: ``cgs_oriented_near`` into a new tensor, the result stays on the device.  ``backend="host"``: numpy."""
    _check_backend(backend)
    tol2 = _tol2(tolerance_px)
    if (codes.dtype if torch.is_tensor(codes) else np.asarray(codes).dtype) not in (torch.uint8, np.uint8):
        raise ValueError("oriented_near: codes must be uint8 [V,H,W], the result of mask_orientation")
    codes = ES._as_masks(codes, "oriented_near: codes")
    return _planes("oriented_near", codes, backend, device, lambda c: oriented_near_host(c, tol2),
                   lambda lib, V, H, W, src, dst, s: lib.cgs_oriented_near(V, H, W, src, tol2, dst, s))


# ------------------------------------------------------------------------------------------------ the tally
def sample_partners(offsets):
    """int32 [P] (numpy): per sample of ``sample_edges``' layout (offsets int [E+1]) its partner -- the next sample of its edge,
    the previous one for an edge's last sample, itself on an edge of one sample."""
    off = ES._host(offsets)
    if off.ndim != 1 or off.size < 1:
        raise ValueError(f"offsets must be an integer [E+1] array (got {off.dtype} {off.shape})")
    off = SP._offsets(off, int(off[-1])).astype(np.int64)
    P = int(off[-1])
    partner = np.arange(P, dtype=np.int64) + 1
    n = np.diff(off)
    last = off[1:][n > 0] - 1
    partner[last] = last - 1
    partner[last[n[n > 0] == 1]] += 1   # an edge of one sample: itself
    return partner.astype(np.int32)


def _partner(partner, P):
    dtype = partner.dtype if torch.is_tensor(partner) else np.asarray(partner).dtype
    if dtype not in (torch.int32, np.int32):
        raise ValueError(f"partner must be int32, the result of sample_partners (got {dtype})")
    t = partner.detach() if torch.is_tensor(partner) else torch.from_numpy(np.ascontiguousarray(partner))
    if tuple(t.shape) != (P,):
        raise ValueError(f"partner must be [P] with P = {P} points (got {tuple(t.shape)})")
    return t.contiguous()


def _near(near, V):
    dtype = near.dtype if torch.is_tensor(near) else np.asarray(near).dtype
    if dtype not in (torch.uint8, np.uint8):
        raise ValueError(f"near must be uint8, the result of oriented_near (got {dtype})")
    t = near.detach() if torch.is_tensor(near) else torch.from_numpy(np.ascontiguousarray(near))
    if t.dim() != 3 or t.shape[0] != V:
        raise ValueError(f"near must be [V,H,W] with V = {V} cameras (got {tuple(t.shape)})")
    if V > 0:
        ES._check_size("oriented_tally: near", t.shape[1], t.shape[2])
    return t.contiguous()


def oriented_tally(points, partner, intrinsics, w2c, near, spread=SPREAD, backend="gpu", device=None, out=None, depth=None,
                   slack=EO.DEPTH_SLACK, hidden_out=None):
    """int32 [P,2].  points float32 [P,3]; partner int32 [P] (``sample_partners``; a value outside [0, P) or equal to its
    index means no partner); intrinsics [V,4] = (fx, fy, cx, cy) and w2c [V,3,4] float64 host arrays or tensors; near uint8
    [V,H,W], ``oriented_near`` of every view; ``spread`` in [0, 4].  tally[i,0] = the views in which ``cgs_project_points``
    keeps point i; tally[i,1] = those of them in which near at its pixel shares a bit with the orientations that the direction
    to its partner accepts (the module docstring).

    ``out``: a contiguous int32 [P,2] tensor that the counts are ADDED to and that is returned -- one call per chunk of views
    into the same tally; without it the counts of this call alone, in a new tensor.

    ``backend="gpu"``: ``cgs_sample_support_oriented``.  near must be on a GPU (CurveGSError otherwise), ``device``, when
    given, must be that GPU, and so must the device of ``out`` and of points and partner that are on a GPU; those on the host
    are uploaded.  The result stays on the device.  ``backend="host"``: numpy, CPU tensors.

    ``depth`` (None: no gate, the call above and nothing else), ``slack`` and ``hidden_out`` as ``edge_trim.sample_tally``
    takes them (``cgs_sample_support_oriented_depth``): a view that keeps sample i and whose depth plane hides it counts in
    neither column and is ADDED to hidden_out[i].  ONLY THE SAMPLE IS GATED: its partner is projected by the projection rule
    alone and gives its direction whether or not a surface lies in front of it."""
    _check_backend(backend)
    spread = _spread(spread)
    pts = SP._points(points)
    P = int(pts.shape[0])
    partner = _partner(partner, P)
    V, K, M = ES._cameras(intrinsics, w2c)
    near = _near(near, V)
    if out is not None:
        if not torch.is_tensor(out) or out.dtype != torch.int32 or tuple(out.shape) != (P, 2) or not out.is_contiguous():
            raise ValueError(f"oriented_tally: out must be a contiguous int32 [{P},2] tensor")
    EO.check_hidden_out("oriented_tally", hidden_out, depth, P)
    if backend == "host":
        SP._host_only("oriented_tally", near, pts, partner, out, hidden_out)
        if out is None:
            out = torch.zeros((P, 2), dtype=torch.int32)
        if depth is not None:
            depth, slack = EO.operator_depth("oriented_tally", depth, slack, V, int(near.shape[1]), int(near.shape[2]), "host")
        _tally_host(pts.numpy(), partner.numpy(), K, M, near.numpy(), spread, out.numpy(), depth, slack,
                    None if hidden_out is None else hidden_out.numpy())
        return out
    dev = SP._one_device("oriented_tally", "near", near, device, uploaded=[("points", pts), ("partner", partner)],
                         resident=[("out", [out]), ("hidden_out", [hidden_out])])
    with L.device_guard(dev):
        pts, partner = pts.to(dev).contiguous(), partner.to(dev).contiguous()
        if out is None:
            out = torch.zeros((P, 2), dtype=torch.int32, device=dev)
        if depth is not None:
            depth, slack = EO.operator_depth("oriented_tally", depth, slack, V, int(near.shape[1]), int(near.shape[2]), "gpu",
                                             dev)
        if P > 0 and V > 0:
            Kd, Md = ES.cameras_on(dev, K, M)
            args = [P, L.ptr(pts), L.ptr(partner), V, L.ptr(Kd), L.ptr(Md), int(near.shape[1]), int(near.shape[2]),
                    L.ptr(near), spread]
            if depth is None:
                L.check(L.load().cgs_sample_support_oriented(*args, L.ptr(out), L.raw_stream(dev)),
                        "cgs_sample_support_oriented")
            else:
                L.check(L.load().cgs_sample_support_oriented_depth(*args, L.ptr(depth), slack, L.ptr(out), L.ptr(hidden_out),
                                                                   L.raw_stream(dev)), "cgs_sample_support_oriented_depth")
    return out
