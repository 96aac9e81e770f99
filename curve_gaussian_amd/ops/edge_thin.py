"""Parallel binary thinning of detected edge masks (cgs_thin_masks, include/curvegs.h; csrc/edge_thin.hip).  A learned
detector's response is several pixels wide; ``score_edges``, ``edge_support`` and ``seed_points`` were designed on drawn
maps one pixel thin and, with ``thin=True``, pass every chunk's detected masks through ``thin_masks`` first.  The reference
has no counterpart.

The rule, frozen: Guo-Hall two-subiteration thinning (Guo & Hall, CACM 1989).  The state is a binary image,
pixels outside it read as 0; the neighbours of (y, x) are P2 = (y-1, x), P3 = (y-1, x+1), P4 = (y, x+1), P5 = (y+1, x+1),
P6 = (y+1, x), P7 = (y+1, x-1), P8 = (y, x-1), P9 = (y-1, x-1).
  C  = (!P2 & (P3|P4)) + (!P4 & (P5|P6)) + (!P6 & (P7|P8)) + (!P8 & (P9|P2))
  N1 = (P9|P2) + (P3|P4) + (P5|P6) + (P7|P8),  N2 = (P2|P3) + (P4|P5) + (P6|P7) + (P8|P9),  N = min(N1, N2)
  m  = (P6 | P7 | !P9) & P8 in sub-iteration 0,  (P2 | P3 | !P5) & P4 in sub-iteration 1
  a set pixel is cleared iff C == 1 and 2 <= N <= 3 and m == 0
Every pixel of a sub-iteration decides from the state before it; an iteration is sub-iteration 0, then 1; the result is the
state after the first iteration that changes nothing.  The iteration COUNT includes that one (a settled input: 1) and is the
count of the view that settles last; ``max_iterations`` = n > 0 stops after n iterations or sooner when settled.

KNOWN LIMITS.  This thins a BINARY MASK: it is not non-maximum suppression on the response's strength, so the skeleton is
the medial axis of the thresholded blob, not the response's ridge.  Line ends retract by about half the response's width,
junction blobs leave short spurs.  THE OPTION IS UNTUNED: checked on dilated drawn maps only (tests/edge_thin_cases.py), no
real detector output.

Two back ends: ``"gpu"``, HIP, and ``"host"``, numpy -- booleans and integers only, so they agree bit for bit."""
import ctypes as C

import numpy as np
import torch

from .. import _lib as L
from . import edge_score as ES

THIN_BACKENDS = ES.SCORE_BACKENDS
PASS_ITERATIONS = L.THIN_PASS_ITERATIONS                  # iterations per launch
TILE_HEIGHT, TILE_WIDTH = L.THIN_TILE_HEIGHT, L.THIN_TILE_WIDTH   # the kernel's tile


def _check_backend(backend):
    if backend not in THIN_BACKENDS:
        raise ValueError(f"unknown thinning backend {backend!r}: expected one of {THIN_BACKENDS}")


def _sub_iteration_host(s, sub):
    """One sub-iteration of a bool [H,W] state: the state after it."""
    p = np.pad(s, 1)
    P2, P3, P4, P5 = p[:-2, 1:-1], p[:-2, 2:], p[1:-1, 2:], p[2:, 2:]
    P6, P7, P8, P9 = p[2:, 1:-1], p[2:, :-2], p[1:-1, :-2], p[:-2, :-2]
    n = lambda a, b, c, d: a.astype(np.uint8) + b + c + d
    c_count = n(~P2 & (P3 | P4), ~P4 & (P5 | P6), ~P6 & (P7 | P8), ~P8 & (P9 | P2))
    n_min = np.minimum(n(P9 | P2, P3 | P4, P5 | P6, P7 | P8), n(P2 | P3, P4 | P5, P6 | P7, P8 | P9))
    m = (P6 | P7 | ~P9) & P8 if sub == 0 else (P2 | P3 | ~P5) & P4
    return s & ~((c_count == 1) & (n_min >= 2) & (n_min <= 3) & ~m)


def thin_mask_host(mask, max_iterations=0):
    """One view, numpy: (uint8 [H,W] of 0 / 1, the iteration count)."""
    s = np.asarray(mask) != 0
    done = 0
    while True:
        after = _sub_iteration_host(_sub_iteration_host(s, 0), 1)
        done += 1
        changed = not np.array_equal(after, s)
        s = after
        if not changed or done == max_iterations:
            return s.astype(np.uint8), done


def thin_masks(masks, backend="gpu", device=None, max_iterations=0, return_iterations=False):
    """masks: uint8 or bool [V,H,W] (a tensor or an array), nonzero = set; it is not modified.  Returns uint8 [V,H,W] of
    0 / 1, thinned by the rule of the module docstring; with ``return_iterations`` also the number of iterations (an int; 0
    for an empty stack).  H and W lie in [1, 16384].  ``max_iterations``: 0 thins until nothing changes, n > 0 stops after n
    iterations.  ``backend="gpu"``: ``cgs_thin_masks`` on a copy (masks not on a GPU are uploaded; ``device``: which GPU),
    one more buffer of the same size as scratch; the result stays on the device.  ``backend="host"``: numpy, a CPU tensor."""
    _check_backend(backend)
    max_iterations = int(max_iterations)
    if max_iterations < 0:
        raise ValueError(f"thin_masks: max_iterations must be >= 0 (got {max_iterations})")
    masks = ES._as_masks(masks, "thin_masks: masks")
    V, H, W = (int(s) for s in masks.shape)
    if backend == "host":
        m = ES._host(masks)
        out = np.empty((V, H, W), np.uint8)
        iterations = 0
        for v in range(V):   # the views are independent: the stack's count is that of the view that settles last
            out[v], n = thin_mask_host(m[v], max_iterations)
            iterations = max(iterations, n)
        out = torch.from_numpy(out)
        return (out, iterations) if return_iterations else out
    dev = ES._device_for([masks], "thin_masks", device)
    lib = L.load()
    count = C.c_int(0)
    with L.device_guard(dev):
        out = masks.to(dev, copy=True)
        if V > 0:
            scratch = torch.empty_like(out)
            flag = torch.empty((1,), dtype=torch.int32, device=dev)
            rc = lib.cgs_thin_masks(V, H, W, L.ptr(out), L.ptr(scratch), L.ptr(flag), max_iterations, C.byref(count),
                                    L.raw_stream(dev))
            L.check(rc, "cgs_thin_masks")
    return (out, int(count.value)) if return_iterations else out
