"""Edge maps from photographs: a classical (Canny) detector with a soft response (cgs_edge_gradients / cgs_edge_trace,
include/curvegs.h; csrc/edge_detect.hip).

The reference has no counterpart: its edge maps come from a learned detector (DexiNed, PidiNet) that runs outside it.  This
detector needs no weights and closes the path from photographs to edge maps inside the package; it is NOT a substitute
for a learned detector in quality.  The defaults (``sigma=1.4, low=0.05, high=0.15``) are untuned: nobody has tried them
on a real scan.

The rule, per view (uint8 ``[H,W]`` or ``[H,W,C]``, C in {1, 3, 4}, alpha ignored):
  luminance   Y = (0.299 R + 0.587 G + 0.114 B) / 255, or value / 255
  smoothing   separable Gaussian, radius ceil(3 sigma) (at most 12), taps computed in float64, normalised, rounded to
              float32; rows, then columns; replicate border; sigma == 0: none
  gradient    Sobel 3x3 on the smoothed image, replicate border, divided by 4: gx, gy; m = sqrt(gx^2 + gy^2)
  thinning    (``thin``) a pixel keeps m' = m iff m > m(first) and m >= m(second) of the neighbour pair along its gradient
              (``neighbour_offsets``), a neighbour outside the image counting 0; otherwise m' = 0
  hysteresis  candidates m' >= low, strong m' >= high; a candidate is kept iff its 8-connected component of candidates
              contains a strong pixel
  response    e = min(m' / high, 1) for kept pixels, 0 elsewhere

Two back ends: ``"gpu"``, HIP, ``_lib.EDGE_MAX_VIEWS`` views per call, and ``"host"``, numpy -- the back end for a machine
without a GPU and what the tests hold the kernels against.  The host gradients are a float64 restatement rounded to
float32 once; the host tracing evaluates the rule in float32 in the kernel's order, so on identical float32 inputs it is
bit-identical to the kernel."""
import ctypes as C
import math

import numpy as np
import torch

from .. import _lib as L

EDGE_BACKENDS = ("gpu", "host")
MAX_SIGMA = 4.0
THIN_T = np.float32(0.41421357)


def _check_backend(backend):
    if backend not in EDGE_BACKENDS:
        raise ValueError(f"unknown edge detection backend {backend!r}: expected one of {EDGE_BACKENDS}")


def _check_thresholds(low, high):
    low, high = float(low), float(high)
    if not (0.0 < low <= high) or not math.isfinite(high):
        raise ValueError(f"edge detection thresholds must satisfy 0 < low <= high (got low={low}, high={high})")
    return low, high


def gaussian_taps(sigma):
    """``(taps float32 [2 r + 1], r)``: r = ceil(3 sigma), the taps exp(-o^2 / (2 sigma^2)) in float64, normalised to sum 1,
    rounded to float32.  ``sigma == 0``: the single tap 1."""
    sigma = float(sigma)
    if not 0.0 <= sigma <= MAX_SIGMA:
        raise ValueError(f"edge detection sigma must lie in [0, {MAX_SIGMA:g}] (got {sigma})")
    radius = min(int(math.ceil(3.0 * sigma)), L.EDGE_MAX_RADIUS)
    if radius == 0:
        return np.ones(1, np.float32), 0
    o = np.arange(-radius, radius + 1, dtype=np.float64)
    w = np.exp(-(o * o) / (2.0 * sigma * sigma))
    return (w / w.sum()).astype(np.float32), radius


def _as_images(images, what):
    """uint8 tensors [H,W,C] (a [H,W] image becomes [H,W,1]), as given (no copy where none is needed)."""
    out = []
    for v, im in enumerate(images):
        if isinstance(im, np.ndarray):
            im = torch.from_numpy(np.ascontiguousarray(im))
        if not torch.is_tensor(im) or im.dtype != torch.uint8 or im.dim() not in (2, 3):
            raise ValueError(f"{what}: images[{v}] must be a uint8 [H,W] or [H,W,C] image")
        if im.dim() == 2:
            im = im.unsqueeze(-1)
        if im.shape[2] not in (1, 3, 4) or im.shape[0] == 0 or im.shape[1] == 0:
            raise ValueError(f"{what}: images[{v}] must have 1, 3 or 4 channels and a non-empty pixel grid (got shape "
                             f"{tuple(im.shape)})")
        out.append(im)
    return out


def _device_for(tensors, what):
    dev = next((t.device for t in tensors if t.is_cuda), None)
    if dev is None:
        if not torch.cuda.is_available():
            raise L.CurveGSError(f"{what}: backend='gpu' needs a GPU (backend='host' computes on the CPU)")
        dev = torch.device("cuda", torch.cuda.current_device())
    return dev


# ------------------------------------------------------------------------------------------------ gradients
def _blur_f64(a, taps, axis):
    r = (len(taps) - 1) // 2
    pad = [(0, 0), (0, 0)]
    pad[axis] = (r, r)
    p = np.pad(a, pad, mode="edge")
    n = a.shape[axis]
    out = np.zeros_like(a)
    for k, w in enumerate(taps):
        out += float(w) * (p[k:k + n, :] if axis == 0 else p[:, k:k + n])
    return out


def gradients_host_f64(image, sigma):
    """One view on the host: ``(gx, gy, m)``, float64 [H,W], before the cast to float32."""
    a = np.asarray(image, np.float64)
    a = a[:, :, None] if a.ndim == 2 else a
    lum = (a[:, :, 0] if a.shape[2] == 1 else 0.299 * a[:, :, 0] + 0.587 * a[:, :, 1] + 0.114 * a[:, :, 2]) / 255.0
    taps, _ = gaussian_taps(sigma)
    s = _blur_f64(_blur_f64(lum, taps, 1), taps, 0)
    H, W = s.shape
    p = np.pad(s, 1, mode="edge")
    sl = lambda dy, dx: p[1 + dy:1 + dy + H, 1 + dx:1 + dx + W]
    gx = ((sl(-1, 1) + 2.0 * sl(0, 1) + sl(1, 1)) - (sl(-1, -1) + 2.0 * sl(0, -1) + sl(1, -1))) / 4.0
    gy = ((sl(1, -1) + 2.0 * sl(1, 0) + sl(1, 1)) - (sl(-1, -1) + 2.0 * sl(-1, 0) + sl(-1, 1))) / 4.0
    return gx, gy, np.sqrt(gx * gx + gy * gy)


def edge_gradients(images, sigma=1.4, backend="gpu"):
    """images: uint8 ``[H,W]`` or ``[H,W,C]`` tensors or arrays (C 1, 3 or 4; sizes may differ).  Returns ``(gx, gy, m)``,
    three lists of float32 ``[H,W]`` tensors: the Sobel gradient of the smoothed luminance and its magnitude.

    ``backend="gpu"``: images not on a GPU are uploaded to the current one, the results stay on the device.
    ``backend="host"``: numpy, float64, rounded to float32 once; CPU tensors."""
    _check_backend(backend)
    taps, radius = gaussian_taps(sigma)
    images = _as_images(images, "edge_gradients")
    if backend == "host":
        res = [gradients_host_f64(im.detach().cpu().numpy(), sigma) for im in images]
        return tuple([torch.from_numpy(r[k].astype(np.float32)) for r in res] for k in range(3))
    if not images:
        return [], [], []
    lib = L.load()
    dev = _device_for(images, "edge_gradients")
    taps_c = (C.c_float * len(taps))(*[float(w) for w in taps])
    with L.device_guard(dev):
        srcs = [im.detach().to(dev).contiguous() for im in images]
        outs = [[torch.empty(s.shape[:2], dtype=torch.float32, device=dev) for s in srcs] for _ in range(3)]
        stream = L.raw_stream(dev)
        for first in range(0, len(srcs), L.EDGE_MAX_VIEWS):
            count = min(L.EDGE_MAX_VIEWS, len(srcs) - first)
            table = (L.EdgeGradientView * count)()
            for k in range(count):
                v = first + k
                table[k] = L.EdgeGradientView(srcs[v].data_ptr(), outs[0][v].data_ptr(), outs[1][v].data_ptr(),
                                              outs[2][v].data_ptr(), *(int(t) for t in srcs[v].shape), 0)
            rc = lib.cgs_edge_gradients(count, C.cast(table, C.c_void_p), C.cast(taps_c, C.c_void_p), radius, stream)
            L.check(rc, "cgs_edge_gradients")
    # (uploaded copies go back to the caching allocator on this stream: reuse is stream-ordered)
    return tuple(outs)


# ------------------------------------------------------------------------------------------------ tracing
def neighbour_offsets(gx, gy):
    """``(dx, dy)`` int arrays: the first neighbour of the thinning pair is (x + dx, y + dy), the second (x - dx, y - dy).
    float32, the kernel's tests in the kernel's order: |gy| <= T |gx| -> (-1, 0); |gx| <= T |gy| -> (0, -1);
    gx gy > 0 -> (-1, -1); otherwise (+1, -1)."""
    gx, gy = np.asarray(gx, np.float32), np.asarray(gy, np.float32)
    ax, ay = np.abs(gx), np.abs(gy)
    horizontal = ay <= THIN_T * ax
    vertical = ~horizontal & (ax <= THIN_T * ay)
    diagonal = ~horizontal & ~vertical & (gx * gy > np.float32(0))
    dx = np.where(horizontal, -1, np.where(vertical, 0, np.where(diagonal, -1, 1)))
    dy = np.where(horizontal, 0, -1)
    return dx, dy


def thin_host(gx, gy, m):
    """m' of the thinning rule, float32 [H,W]."""
    m = np.asarray(m, np.float32)
    H, W = m.shape
    dx, dy = neighbour_offsets(gx, gy)
    p = np.pad(m, 1, mode="constant")
    yy, xx = np.mgrid[0:H, 0:W]
    m1 = p[yy + 1 + dy, xx + 1 + dx]
    m2 = p[yy + 1 - dy, xx + 1 - dx]
    return np.where((m > m1) & (m >= m2), m, np.float32(0)).astype(np.float32)


_EIGHT = [(-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1)]


def hysteresis_host(mt, low, high):
    """bool [H,W]: the candidates (mt >= low) whose 8-connected component holds a strong pixel (mt >= high).  A breadth-first
    sweep from the strong pixels; each step costs what its frontier holds, not the image."""
    low, high = np.float32(low), np.float32(high)
    H, W = mt.shape
    open_ = np.zeros((H + 2, W + 2), bool)      # candidates not reached yet, with a closed border
    open_[1:-1, 1:-1] = mt >= low
    kept = np.zeros((H + 2, W + 2), bool)
    ys, xs = np.nonzero(mt >= high)
    ys, xs = ys + 1, xs + 1
    kept[ys, xs] = True
    open_[ys, xs] = False
    while ys.size:
        ny = np.concatenate([ys + dy for dy, _ in _EIGHT])
        nx = np.concatenate([xs + dx for _, dx in _EIGHT])
        hit = open_[ny, nx]
        flat = np.unique(ny[hit] * (W + 2) + nx[hit])
        ys, xs = flat // (W + 2), flat % (W + 2)
        open_[ys, xs] = False
        kept[ys, xs] = True
    return kept[1:-1, 1:-1]


def trace_host(gx, gy, m, low, high, thin):
    """One view on the host, float32 throughout: e [H,W]."""
    m = np.ascontiguousarray(m, np.float32)
    mt = thin_host(gx, gy, m) if thin else m
    kept = hysteresis_host(mt, low, high)
    e = np.minimum(mt / np.float32(high), np.float32(1))
    return np.where(kept, e, np.float32(0)).astype(np.float32)


def _as_fields(gx, gy, m):
    gx, gy, m = list(gx), list(gy), list(m)
    if not (len(gx) == len(gy) == len(m)):
        raise ValueError(f"trace_edges: {len(gx)} gx, {len(gy)} gy and {len(m)} m fields")
    for v, (a, b, c) in enumerate(zip(gx, gy, m)):
        for t in (a, b, c):
            if not torch.is_tensor(t) or t.dtype != torch.float32 or t.dim() != 2 or t.numel() == 0:
                raise ValueError(f"trace_edges: view {v}: gx, gy and m must be non-empty float32 [H,W] tensors")
        if not (a.shape == b.shape == c.shape):
            raise ValueError(f"trace_edges: view {v}: gx, gy and m differ in shape")
    return gx, gy, m


def trace_edges(gx, gy, m, low=0.05, high=0.15, thin=True, backend="gpu", stats=None):
    """gx, gy, m: lists of float32 ``[H,W]`` tensors (``edge_gradients``; finite values).  Returns a list of float32
    ``[1,H,W]`` tensors in [0,1]: the soft response of the pixels that survive thinning and hysteresis.

    ``backend="gpu"``: on the device; every ``_lib.EDGE_MAX_VIEWS`` views cost one classification launch, propagation
    rounds of one launch and one 4-byte readback each, until a round changes nothing, and one response launch.  A round
    settles every 64x16 tile against its neighbours' current state, so the count is about the number of tile borders the
    longest chain of weak pixels crosses on its way from a strong one, plus the final round that finds nothing to do.
    ``stats``: a dict; ``stats["rounds"]`` gets the rounds of every call appended.  ``backend="host"``: numpy, float32."""
    _check_backend(backend)
    low, high = _check_thresholds(low, high)
    gx, gy, m = _as_fields(gx, gy, m)
    if backend == "host":
        n = lambda t: t.detach().cpu().numpy()
        return [torch.from_numpy(trace_host(n(a), n(b), n(c), low, high, thin)).unsqueeze(0) for a, b, c in zip(gx, gy, m)]
    if not m:
        return []
    lib = L.load()
    dev = _device_for(gx + gy + m, "trace_edges")
    with L.device_guard(dev):
        up = lambda ts: [t.detach().to(dev).contiguous() for t in ts]
        gx, gy, m = up(gx), up(gy), up(m)
        outs = [torch.empty((1,) + tuple(t.shape), dtype=torch.float32, device=dev) for t in m]
        states = [torch.empty(t.shape, dtype=torch.uint8, device=dev) for t in m]
        flag = torch.zeros(1, dtype=torch.int32, device=dev)
        stream = L.raw_stream(dev)
        for first in range(0, len(m), L.EDGE_MAX_VIEWS):
            count = min(L.EDGE_MAX_VIEWS, len(m) - first)
            table = (L.EdgeTraceView * count)()
            for k in range(count):
                v = first + k
                table[k] = L.EdgeTraceView(gx[v].data_ptr(), gy[v].data_ptr(), m[v].data_ptr(), outs[v].data_ptr(),
                                           states[v].data_ptr(), int(m[v].shape[0]), int(m[v].shape[1]))
            rc = lib.cgs_edge_trace(count, C.cast(table, C.c_void_p), low, high, 1 if thin else 0,
                                    C.c_void_p(flag.data_ptr()), stream)
            L.check(rc, "cgs_edge_trace")
            if stats is not None:
                stats.setdefault("rounds", []).append(int(rc))
    return outs


def detect_edges(images, sigma=1.4, low=0.05, high=0.15, thin=True, backend="gpu", stats=None):
    """``trace_edges(*edge_gradients(images, sigma), low, high, thin)``: uint8 images -> float32 ``[1,H,W]`` edge maps in [0,1],
    bright = edge."""
    _check_backend(backend)
    _check_thresholds(low, high)
    gx, gy, m = edge_gradients(images, sigma, backend)
    return trace_edges(gx, gy, m, low, high, thin, backend, stats)
