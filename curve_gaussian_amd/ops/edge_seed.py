"""Seed points for the curves from a scan's own edge maps: a multi-view voxel vote (cgs_pack_near_bits / cgs_voxel_votes,
include/curvegs.h; csrc/edge_seed.hip), on request a ray-exclusive refinement of its selection (cgs_ray_claims /
cgs_ray_wins), and on request the seeds' directions from the kept voxels (cgs_voxel_moments).
The reference has no counterpart: it seeds a fixed 15^3 grid or the SfM cloud, every curve along +-Y.

Definitions (frozen), the same on both back ends bit for bit:
  grid       ``bounds`` = (lo, hi) float64 [3] each and ``dims`` = (nx, ny, nz) >= 1; step = (hi - lo) / dims in float64;
             voxel (i, j, k) has the linear index (k ny + j) nx + i and the centre lo + (i + 0.5) step per axis, computed in
             float64 and rounded to float32 -- the float32 point is what ``project_points`` (ops.edge_score) projects
  near mask  near[y][x] = (d2[y][x] <= tol2), d2 the ``edt_squared`` transform of the view's detected mask, tol2 =
             ``tolerances_squared``; one bit per pixel in uint32 words, word w of row y = pixels 32 w .. 32 w + 31, bit b =
             pixel 32 w + b, row stride ceil(W / 32) words, padding bits 0 (tensors hold the words as int32)
  votes      seen[g] = the views in which the projection keeps the centre of voxel g; hit[g] = those whose near bit at
             (floor(v), floor(u)) is set; uint16, at most 65535 views in total
  selection  kept iff seen >= min_views and hit >= need[seen], need[s] = ceil(min_ratio * s) built in float64
  thinning   cells of ``cell`` voxels per axis; a cell with kept voxels gives one seed, the mean of their integer
             coordinates (int64 sums over a count), at lo + (mean + 0.5) step in float64; seeds ordered by cell index;
             above ``max_seeds`` the cells with the largest summed hit are kept (ties: the lower cell index)

Directions (``directions=True``; frozen), the same on both back ends bit for bit:
  keep bits  the selection mask packed exactly like the near masks with x fastest: word w of row (j, k) = voxels
             i = 32 w .. 32 w + 31, bit b = voxel 32 w + b, row stride ceil(nx / 32) words, rows ordered (k ny + j), padding
             bits 0, the words held as int32 [nz, ny, ceil(nx / 32)]; made on the host by ``keep_bits`` for both back ends
  centre     the centre voxel of a seed, from the thinning's own integer sums: c_a = (2 sum_a + count) // (2 count) per
             axis, floor(mean + 0.5) in integers (``thin_to_seeds(return_centres=True)``)
  window     every voxel q of the grid with its keep bit set and |q - c|^2 <= r^2 -- an integer comparison over a ball
             clipped to the grid, not a cube; r = ``dir_radius``, 1 <= r <= 15 (SEED_MAX_RADIUS), so a row of the window
             spans at most 31 voxels and at most two words
  moments    with d = q - c over the window, int32 [N,10] = [m, sum dx, sum dy, sum dz, sum dx^2, sum dy^2, sum dz^2,
             sum dx dy, sum dx dz, sum dy dz]; every value is bounded by (2 r + 1)^3 r^2 <= 6.8e6: int32 is exact and the
             order of the summation cannot matter
  direction  host float64 code, the same for both back ends (``seed_directions``): the integer matrix
             m sum(d d^T) - (sum d)(sum d)^T in int64, converted to float64, ``np.linalg.eigh`` with eigenvalues
             l0 <= l1 <= l2; the direction is the eigenvector of l2 with its sign fixed so that its component of largest
             magnitude is positive (ties: the lowest axis); linearity = (l2 - l1) / l2, or 0 when l2 = 0; a seed is
             directed iff m >= dir_min_support and linearity >= dir_min_linearity; an undirected seed (a junction, a
             blob, a lone voxel) gets the zero vector and its curve is laid along +-Y

Ray-exclusive claims (``exclusive=True``; frozen), the same on both back ends bit for bit:
  list       ``index`` int32 [M]: the linear indices of the voxels that ``select_voxels`` kept, ascending (``np.nonzero`` on
             the host for both back ends); an index outside [0, n) is a ValueError (the kernels read nothing for it and
             give 0)
  support    support[m] = (hit * 65535) // seen of that voxel, in int64 on the host for both back ends
             (``voxel_support``): an integer in [1, 65535] for a voxel with a hit, uint16 [M]; 0 where seen = 0
  claim      listed voxel m HITS in view v when the rule of the votes keeps its centre and finds its near bit set: the same
             float32 centre, the same projection (c2 > 0, 0 <= u < W, 0 <= v < H), the bit at (floor(v), floor(u)).
             best[v][y][x] = the largest support over the listed voxels that hit at pixel (x, y) of view v, 0 where there
             is none; uint32 [V,H,W] (tensors hold the words as int32)
  wins       wins[m] = the number of views in which m hits and support[m] + margin >= max(best[v]) over the window
             |dx| <= w, |dy| <= w around m's pixel, clipped to the image; w = ``excl_window`` in [0, SEED_MAX_WINDOW],
             margin = ``excl_margin``, an integer in [0, 65535]; the sum is formed in 32 bits; uint16 [M]
  selection  voxel m stays iff wins[m] >= need_table(excl_win_ratio)[hit[m]]; the surviving mask is what the thinning,
             the keep bits and the moments then see

Depth gate (opt-in: ``depth=`` of ``voxel_votes`` / ``ray_claims`` / ``ray_wins``, ``occluder`` / ``depth_maps`` of
``seed_points``; frozen), the same on both back ends bit for bit:
  hidden     view v HIDES voxel g iff the projection keeps its centre and c2 > float64(depth[v][floor(v)][floor(u)]) + slack
             -- the one rule of ops/edge_occlusion.py (``nv_hidden``; ``gate_view_host`` on the host), c2 the centre's
             camera-space depth, depth float32 [V,H,W] camera z with +inf for no surface; a NaN depth hides nothing
  votes      a hiding view counts in neither seen nor hit but in hidden[g] (uint16): seen + hidden is the ungated seen
  claims     a listed voxel claims nothing and wins nothing in a view that hides it
  slack      the caller's; None is ``default_slack``, half the voxel diagonal (the centre of a voxel that holds an edge can lie
             that far behind the surface that carries the edge).  UNTUNED, drawn solids only (``seed_points``)

WITHOUT a depth source there is no occlusion reasoning in the vote: a voxel behind a surface is seen by the views that look
at it through the surface -- on a scan whose hidden lines are removed hit / seen then never reaches ``min_ratio`` on a rim
and nothing is kept --, and with few views the back-projections of unrelated edge pixels intersect in empty space ("ghosts");
min_views / min_ratio are its only defence.  ``exclusive=True`` adds a winner-take-all pass without depth: a voxel stays
only if, in enough of the views in which it hits, no listed voxel near the same ray is better supported.  That removes
most ghosts of a scan with few views (each of their pixels is explained better by a true voxel) and thins a true tube to
its best-supported ridge; it does NOT recover occlusion -- a voxel behind a surface still votes through it --, and a true
edge that is weakly supported everywhere and runs next to a strong one in the images loses.  The curve direction is not
seeded unless ``directions=True``.  The defaults of ``seed_points`` are untuned, those of the directions (DIR_RADIUS,
DIR_MIN_SUPPORT, DIR_MIN_LINEARITY) and of the claims (EXCL_WINDOW, EXCL_MARGIN, EXCL_WIN_RATIO) included.

Two back ends: ``"gpu"``, HIP, and ``"host"``, numpy -- the same rules, for a machine without a GPU and what the tests hold
the kernels against.  Selection, thinning, the list and its support, the keep bits and the eigen-decomposition are numpy
on both."""
import ctypes as C

import numpy as np
import torch

from .. import _lib as L
from ..edge_extraction.para_edge import EDGE_MAX_THRESHOLD
from . import edge_occlusion as EO
from . import edge_score as ES
from .edge_thin import thin_masks
from .view_chunks import check_budget, check_edge_maps, detected_lut, detected_masks, view_chunks

SEED_BACKENDS = ES.SCORE_BACKENDS
MAX_VIEWS = L.SEED_MAX_VIEWS
MAX_VOXELS = 2 ** 31 - 1
BYTE_BUDGET = 1 << 30     # bytes of masks, transforms, scratch and bits per chunk of views in seed_points
BYTES_PER_PIXEL = 8       # uint8 mask, uint16 column pass, int32 transform, one bit (rounded up)
EXCL_BYTES_PER_PIXEL = 4  # the second sweep of ``exclusive``: uint32 best (the near bits stay from the first sweep)
HOST_SLAB = 1 << 18       # voxels per numpy slab of the host back end
SEED_MAX_RADIUS = L.SEED_MAX_RADIUS
MOMENT_VALUES = 10        # m, sum d [3], sum d^2 [3], sum dx dy, sum dx dz, sum dy dz
# UNTUNED, like the other defaults of this module: no scan has been trained against them beyond the drawn test scan
DIR_RADIUS, DIR_MIN_SUPPORT, DIR_MIN_LINEARITY = 6, 6, 0.5
SEED_MAX_WINDOW = L.SEED_MAX_WINDOW
MAX_SUPPORT = 65535
# UNTUNED as well: one prototype run on the two drawn test scans, no real scan
EXCL_WINDOW, EXCL_MARGIN, EXCL_WIN_RATIO = 1, 0, 0.5


def _check_backend(backend):
    if backend not in SEED_BACKENDS:
        raise ValueError(f"unknown edge seed backend {backend!r}: expected one of {SEED_BACKENDS}")


def bits_stride(width):
    return (int(width) + 31) // 32


def _check_bits(name, bits, V, height, width):
    """The packed masks of V views as a tensor: int32 [V,height,ceil(width/32)]."""
    if not torch.is_tensor(bits):
        bits = torch.from_numpy(np.ascontiguousarray(bits))
    if bits.dtype != torch.int32 or tuple(bits.shape) != (V, height, bits_stride(width)):
        raise ValueError(f"{name}: bits must be int32 [{V},{height},{bits_stride(width)}] (got {bits.dtype} "
                         f"{tuple(bits.shape)})")
    return bits


def _check_window(name, window):
    if int(window) != window or not (0 <= int(window) <= SEED_MAX_WINDOW):
        raise ValueError(f"{name} must be an integer in [0, {SEED_MAX_WINDOW}] (got {window})")
    return int(window)


def _check_margin(name, margin):
    if int(margin) != margin or not (0 <= int(margin) <= MAX_SUPPORT):
        raise ValueError(f"{name} must be an integer in [0, {MAX_SUPPORT}] (got {margin})")
    return int(margin)


def _check_ratio(name, ratio):
    if not (0.0 <= float(ratio) <= 1.0):
        raise ValueError(f"{name} must lie in [0, 1] (got {ratio})")
    return float(ratio)


# ------------------------------------------------------------------------------------------------ near bits
def near_bits(dist2, tol_px, backend="gpu", device=None):
    """dist2: int32 [V,H,W] (tensor or array), the ``edt_squared`` transform of the detected masks.  Returns the packed
    near masks, int32 [V,H,ceil(W/32)] holding the uint32 words of the module docstring: bit = dist2 <= floor(tol_px^2).
    ``backend="gpu"``: ``cgs_pack_near_bits``, the result stays on the device; ``backend="host"``: numpy, a CPU tensor."""
    _check_backend(backend)
    tol2 = ES.tolerances_squared([tol_px])[0]
    if isinstance(dist2, np.ndarray):
        dist2 = torch.from_numpy(np.ascontiguousarray(dist2))
    if not torch.is_tensor(dist2) or dist2.dtype != torch.int32 or dist2.dim() != 3:
        raise ValueError("near_bits: dist2 must be an int32 [V,H,W] stack of squared distance transforms")
    V, H, W = (int(s) for s in dist2.shape)
    if V > 0:
        ES._check_size("near_bits", H, W)
    stride = bits_stride(W)
    if backend == "host":
        near = dist2.detach().cpu().numpy() <= tol2
        padded = np.zeros((V, H, stride * 32), bool)
        padded[:, :, :W] = near
        words = np.packbits(padded, axis=-1, bitorder="little").view("<u4")
        return torch.from_numpy(np.ascontiguousarray(words).view(np.int32).reshape(V, H, stride))
    dev = ES._device_for([dist2], "near_bits", device)
    with L.device_guard(dev):
        dist2 = dist2.to(dev).contiguous()
        bits = torch.empty((V, H, stride), dtype=torch.int32, device=dev)
        if V > 0:
            rc = L.load().cgs_pack_near_bits(V, H, W, L.ptr(dist2), tol2, L.ptr(bits), L.raw_stream(dev))
            L.check(rc, "cgs_pack_near_bits")
    return bits


def unpack_bits(bits, width):
    """The inverse of the packing: int32 [V,H,ceil(width/32)] words -> (near bool [V,H,width], padding bool
    [V,H,32 ceil(width/32) - width]) numpy arrays."""
    words = np.ascontiguousarray(ES._host(bits)).view(np.uint32).astype("<u4")
    flat = np.unpackbits(words.view(np.uint8), axis=-1, bitorder="little").astype(bool)
    return flat[..., :int(width)], flat[..., int(width):]


# ------------------------------------------------------------------------------------------------ grid and votes
def _grid(bounds, dims):
    lo, hi = (np.asarray(b, np.float64).reshape(-1) for b in bounds)
    if lo.shape != (3,) or hi.shape != (3,):
        raise ValueError("bounds must be (lo [3], hi [3])")
    dims = tuple(int(d) for d in dims)
    if len(dims) != 3 or min(dims) < 1:
        raise ValueError(f"dims must be three positive integers (got {dims})")
    if not (np.isfinite(lo).all() and np.isfinite(hi).all() and (hi > lo).all()):
        raise ValueError(f"bounds must be finite with hi > lo on every axis (got lo={lo.tolist()}, hi={hi.tolist()})")
    if dims[0] * dims[1] * dims[2] > MAX_VOXELS:
        raise ValueError(f"a grid holds at most 2^31 - 1 voxels (got {dims})")
    step = (hi - lo) / np.array(dims, np.float64)
    if not (np.isfinite(step).all() and (step > 0.0).all()):
        raise ValueError(f"the voxel size must be finite and positive (got {step.tolist()})")
    return lo, hi, dims, step


def _grid_c(lo, step):
    return (C.c_double * 3)(*lo), (C.c_double * 3)(*step)


def _centres(lo, dims, step, start, stop):
    return _centres_of(lo, dims, step, np.arange(start, stop, dtype=np.int64))


def _centres_of(lo, dims, step, g):
    ijk = np.stack([g % dims[0], (g // dims[0]) % dims[1], g // (dims[0] * dims[1])], 1).astype(np.float64)
    return (lo[None, :] + (ijk + 0.5) * step[None, :]).astype(np.float32)   # one rounded operation per ufunc: no FMA


def voxel_centres(bounds, dims, start=0, stop=None):
    """float32 [n,3]: the projected centres of the voxels with linear index in [start, stop), the rule of the docstring."""
    lo, _, dims, step = _grid(bounds, dims)
    return _centres(lo, dims, step, start, dims[0] * dims[1] * dims[2] if stop is None else stop)


def _pixels_host(pts, K, M, words, H, W, v, gate=None, hidden_at=None):
    """(at, px, py, bit): the positions among the centres ``pts`` that view v keeps, their pixels and the pixels' near bits
    in the packed uint32 ``words``.  ``gate``: None, or (depth float32 [V,H,W], slack) -- then ``at`` are the positions view v
    keeps and does not hide, by ``edge_occlusion.gate_view_host``, the host's one statement of the rule; ``hidden_at``: a
    list that receives the positions it keeps and hides."""
    if gate is None:
        pu, pv, keep = (x[0] for x in ES.project_points_host(pts, K[v:v + 1], M[v:v + 1], H, W))
    else:
        pu, pv, keep, hid = EO.gate_view_host(pts, K[v], M[v], gate[0][v], gate[1])
        if hidden_at is not None:
            hidden_at.append(np.nonzero(hid)[0])
    at = np.nonzero(keep)[0]
    px, py = np.floor(pu[at]).astype(np.int64), np.floor(pv[at]).astype(np.int64)
    return at, px, py, (words[v, py, px >> 5] >> (px & 31).astype(np.uint32)) & np.uint32(1)


def _votes_host(lo, dims, step, K, M, words, H, W, seen, hit, gate=None, hidden=None):
    n = dims[0] * dims[1] * dims[2]
    words = words.view(np.uint32)
    for s0 in range(0, n, HOST_SLAB):
        pts = _centres(lo, dims, step, s0, min(n, s0 + HOST_SLAB))
        for v in range(K.shape[0]):   # one view at a time: [slab] temporaries
            hidden_at = [] if hidden is not None else None
            at, _, _, bit = _pixels_host(pts, K, M, words, H, W, v, gate, hidden_at)
            seen[s0 + at] += np.uint16(1)
            hit[s0 + at] += bit.astype(np.uint16)
            if hidden_at:
                hidden[s0 + hidden_at[0]] += np.uint16(1)


def default_slack(bounds, dims):
    """Half the diagonal of a voxel of the grid, in world units: the default slack of the gated vote.  The point held against
    the depth plane is a voxel's centre, and the centre of a voxel that holds an edge can lie that far behind the surface
    that carries the edge.  UNTUNED (``seed_points``)."""
    _, _, _, step = _grid(bounds, dims)
    return 0.5 * float(np.sqrt((step * step).sum()))


def _gate_args(name, depth, slack, bounds, dims, V, height, width, backend, dev=None):
    """None without ``depth``; otherwise (depth, slack) checked by ``edge_occlusion.operator_depth`` -- a numpy array for
    ``backend="host"``, a tensor on ``dev`` otherwise; slack None is ``default_slack``."""
    if depth is None:
        return None
    return EO.operator_depth(name, depth, default_slack(bounds, dims) if slack is None else slack, V, height, width, backend, dev)


def voxel_votes(bounds, dims, intrinsics, w2c, bits, height, width, counts=None, backend="gpu", device=None, depth=None,
                slack=None, return_hidden=False):
    """(seen, hit): uint16 [nx ny nz] tensors, the votes of the module docstring over the views of this call.
    intrinsics [V,4] = (fx, fy, cx, cy) and w2c [V,3,4] float64 (arrays or tensors); ``bits``: ``near_bits`` of the same
    views, int32 [V,height,ceil(width/32)].  ``counts``: a (seen, hit) pair of an earlier call over the same grid -- the
    votes are added to it in place and it is returned; the views of all accumulating calls number at most 65535 (the
    caller's to keep: ``seed_points`` checks it).  ``backend="gpu"``: ``cgs_voxel_votes``, device tensors;
    ``backend="host"``: numpy, CPU tensors.

    ``depth`` (None: no gate, the call above and nothing else): float32 [V,height,width], camera z, +inf where there is no
    surface.  A view that keeps a centre HIDES it iff c2 > float64(depth[v][floor(v)][floor(u)]) + ``slack`` (finite, >= 0;
    None: ``default_slack``, half the voxel diagonal; ``cgs_voxel_votes_depth``): it counts in neither seen nor hit.
    ``return_hidden`` (needs ``depth``): (seen, hit, hidden), hidden uint16 [nx ny nz] the views that keep the centre and
    hide it -- seen + hidden is the ungated seen; ``counts`` is then a (seen, hit, hidden) triple.  depth on the host is
    uploaded for ``backend="gpu"``."""
    _check_backend(backend)
    if return_hidden and depth is None:
        raise ValueError("voxel_votes: return_hidden needs depth")
    lo, _, dims, step = _grid(bounds, dims)
    height, width = ES._check_size("voxel_votes", height, width)
    V, K, M = ES._cameras(intrinsics, w2c)
    if V > MAX_VIEWS:
        raise ValueError(f"voxel_votes: at most {MAX_VIEWS} views (got {V})")
    bits = _check_bits("voxel_votes", bits, V, height, width)
    n = dims[0] * dims[1] * dims[2]
    arity = 3 if return_hidden else 2
    if counts is not None:
        counts = tuple(counts)
        if len(counts) != arity:
            raise ValueError(f"voxel_votes: counts must hold {arity} tensors (got {len(counts)})")
        for c in counts:
            if not torch.is_tensor(c) or c.dtype != torch.uint16 or tuple(c.shape) != (n,) or not c.is_contiguous():
                raise ValueError(f"voxel_votes: counts must be a pair of contiguous uint16 [{n}] tensors")   # (or a triple)
    if backend == "host":
        gate = _gate_args("voxel_votes", depth, slack, bounds, dims, V, height, width, "host")
        out = counts if counts is not None else tuple(torch.zeros(n, dtype=torch.uint16) for _ in range(arity))
        if any(c.is_cuda for c in out):
            raise ValueError("voxel_votes: backend='host' accumulates into CPU tensors")
        _votes_host(lo, dims, step, K, M, bits.detach().cpu().numpy(), height, width, out[0].numpy(), out[1].numpy(), gate,
                    out[2].numpy() if return_hidden else None)
        return out
    dev = ES._device_for([bits] + list(counts or []), "voxel_votes", device)
    with L.device_guard(dev):
        if counts is not None:
            out = counts
            if any(c.device != dev for c in out):
                raise ValueError(f"voxel_votes: counts must be on {dev}")
        else:
            out = tuple(torch.empty(n, dtype=torch.uint16, device=dev) for _ in range(arity))
        gate = _gate_args("voxel_votes", depth, slack, bounds, dims, V, height, width, "gpu", dev)
        bits = bits.to(dev).contiguous()
        (Kd, Md), (lo_c, step_c) = ES.cameras_on(dev, K, M), _grid_c(lo, step)
        accumulate = 1 if counts is not None else 0
        if gate is None:
            rc = L.load().cgs_voxel_votes(*dims, lo_c, step_c, V, L.ptr(Kd), L.ptr(Md), height, width, L.ptr(bits),
                                          accumulate, L.ptr(out[0]), L.ptr(out[1]), L.raw_stream(dev))
            L.check(rc, "cgs_voxel_votes")
        else:
            rc = L.load().cgs_voxel_votes_depth(*dims, lo_c, step_c, V, L.ptr(Kd), L.ptr(Md), height, width, L.ptr(bits),
                                                L.ptr(gate[0]), gate[1], accumulate, L.ptr(out[0]), L.ptr(out[1]),
                                                L.ptr(out[2]) if return_hidden else None, L.raw_stream(dev))
            L.check(rc, "cgs_voxel_votes_depth")
    return out


# ------------------------------------------------------------------------------------------------ selection and thinning
def need_table(min_ratio, views):
    """int64 [views + 1]: need[s] = ceil(min_ratio * s), in float64."""
    return np.ceil(_check_ratio("min_ratio", min_ratio) * np.arange(int(views) + 1, dtype=np.float64)).astype(np.int64)


def _counts_host(x):
    return ES._host(x).astype(np.int64).reshape(-1)


def select_voxels(seen, hit, min_views, min_ratio):
    """bool [n] (numpy): seen >= min_views and hit >= need[seen] -- integer comparisons against the ``need_table``."""
    seen, hit = _counts_host(seen), _counts_host(hit)
    if seen.shape != hit.shape:
        raise ValueError("select_voxels: seen and hit differ in shape")
    need = need_table(min_ratio, int(seen.max()) if seen.size else 0)
    return (seen >= int(min_views)) & (hit >= need[seen])


def thin_to_seeds(keep, hit, bounds, dims, cell, max_seeds, return_centres=False):
    """One seed per cell of ``cell``^3 voxels that holds a kept voxel (module docstring).  Returns (seeds float64 [N,3],
    info): info = {"cells": the cells with a kept voxel, "capped": whether max_seeds cut them, "cell_index": int64 [N],
    "hit_sum": int64 [N]}, and with ``return_centres`` also "centre_voxel": int64 [N,3], the centre voxel of every seed
    (module docstring), cut by max_seeds along with the rest."""
    lo, _, (nx, ny, nz), step = _grid(bounds, dims)
    cell, max_seeds = int(cell), int(max_seeds)
    if cell < 1 or max_seeds < 1:
        raise ValueError(f"cell and max_seeds must be positive (got {cell}, {max_seeds})")
    keep = ES._host(keep).reshape(-1).astype(bool)
    hit = _counts_host(hit)
    if keep.size != nx * ny * nz or hit.size != keep.size:
        raise ValueError(f"thin_to_seeds: keep and hit must hold {nx * ny * nz} voxels")
    g = np.nonzero(keep)[0].astype(np.int64)
    ijk = np.stack([g % nx, (g // nx) % ny, g // (nx * ny)], 1)
    cx, cy = -(-nx // cell), -(-ny // cell)
    cidx = ((ijk[:, 2] // cell) * cy + ijk[:, 1] // cell) * cx + ijk[:, 0] // cell
    order = np.argsort(cidx, kind="stable")
    cells, first, count = np.unique(cidx[order], return_index=True, return_counts=True)
    if cells.size == 0:
        info = {"cells": 0, "capped": False, "cell_index": cells, "hit_sum": cells.copy()}
        if return_centres:
            info["centre_voxel"] = np.zeros((0, 3), np.int64)
        return np.zeros((0, 3), np.float64), info
    sums = np.add.reduceat(ijk[order], first, axis=0)          # int64
    hit_sum = np.add.reduceat(hit[g][order], first)
    capped = cells.size > max_seeds
    if capped:
        best = np.lexsort((cells, -hit_sum))[:max_seeds]       # the largest hit sums, ties to the lower cell index
        sel = np.sort(best)                                    # cells is ascending: back in cell order
        cells, sums, count, hit_sum = cells[sel], sums[sel], count[sel], hit_sum[sel]
    mean = sums.astype(np.float64) / count.astype(np.float64)[:, None]
    seeds = lo[None, :] + (mean + 0.5) * step[None, :]
    info = {"cells": int(first.size), "capped": bool(capped), "cell_index": cells, "hit_sum": hit_sum}
    if return_centres:
        info["centre_voxel"] = (2 * sums + count[:, None]) // (2 * count[:, None])   # int64: floor(mean + 0.5)
    return seeds, info


# ------------------------------------------------------------------------------------------------ ray-exclusive claims
def _list_index(name, index, n):
    idx = ES._host(index)
    if idx.size == 0:
        return np.zeros(0, np.int32)
    if idx.ndim != 1 or idx.dtype.kind not in "iu":
        raise ValueError(f"{name}: index must be an integer [M] list of linear voxel indices")
    idx = idx.astype(np.int64)
    if (idx < 0).any() or (idx >= n).any():
        raise ValueError(f"{name}: an index lies outside [0, {n})")
    return np.ascontiguousarray(idx.astype(np.int32))


def voxel_support(seen, hit, index):
    """uint16 [M] CPU tensor: support[m] = (hit * 65535) // seen of voxel index[m] in int64 (module docstring); 0 where
    seen = 0.  seen, hit: the votes (uint16 [n] tensors or integer arrays); index: integer [M] inside [0, n).  Host code on
    both back ends.  A hit above seen, counts of different shapes and an index outside the grid are ValueErrors."""
    seen, hit = _counts_host(seen), _counts_host(hit)
    if seen.shape != hit.shape:
        raise ValueError("voxel_support: seen and hit differ in shape")
    idx = _list_index("voxel_support", index, seen.size).astype(np.int64)
    s, h = seen[idx], hit[idx]
    if (h > s).any() or (h < 0).any():
        raise ValueError("voxel_support: hit must lie in [0, seen]")
    support = np.where(s > 0, (h * MAX_SUPPORT) // np.maximum(s, 1), 0)
    return torch.from_numpy(support.astype(np.uint16))


def _ray_args(name, bounds, dims, index, support, intrinsics, w2c, bits, height, width):
    lo, _, dims, step = _grid(bounds, dims)
    height, width = ES._check_size(name, height, width)
    V, K, M = ES._cameras(intrinsics, w2c)
    if V > MAX_VIEWS:
        raise ValueError(f"{name}: at most {MAX_VIEWS} views (got {V})")
    bits = _check_bits(name, bits, V, height, width)
    idx = _list_index(name, index, dims[0] * dims[1] * dims[2])
    sup = ES._host(support)
    if sup.size == 0:
        sup = np.zeros(0, np.uint16)
    if sup.ndim != 1 or sup.dtype.kind not in "iu" or sup.shape != idx.shape:
        raise ValueError(f"{name}: support must be an integer [{idx.size}] list, one value per listed voxel")
    sup = sup.astype(np.int64)
    if (sup < 0).any() or (sup > MAX_SUPPORT).any():
        raise ValueError(f"{name}: a support lies outside [0, {MAX_SUPPORT}]")
    return lo, dims, step, height, width, V, K, M, bits, idx, np.ascontiguousarray(sup.astype(np.uint16))


def _hits_host(pts, K, M, words, H, W, v, gate=None):
    """(the positions among the centres ``pts`` that hit in view v, their px, their py): the rule of ``_votes_host``, with
    its gate."""
    at, px, py, bit = _pixels_host(pts, K, M, words, H, W, v, gate)
    near = bit != 0
    return at[near], px[near], py[near]


def ray_claims(bounds, dims, index, support, intrinsics, w2c, bits, height, width, best=None, backend="gpu", device=None,
               depth=None, slack=None):
    """best: int32 [V,height,width] tensor holding the uint32 claims of the module docstring (values <= 65535) over the
    views of this call.  index: integer [M] linear indices inside the grid; support: integer [M] in [0, 65535]
    (``voxel_support``); cameras and ``bits`` as for ``voxel_votes``.  ``best``: the claims of an earlier call over the
    same views -- this list's claims are raised into it in place (a list claimed piece by piece) and it is returned;
    without it the claims start from 0.  ``backend="gpu"``: ``cgs_ray_claims``, a device tensor; ``backend="host"``:
    ``np.maximum.at``, a CPU tensor.  ``depth``, ``slack``: the gate of ``voxel_votes`` (``cgs_ray_claims_depth``) -- a listed
    voxel that a view hides claims nothing there."""
    _check_backend(backend)
    lo, dims, step, height, width, V, K, M, bits, idx, sup = _ray_args("ray_claims", bounds, dims, index, support,
                                                                       intrinsics, w2c, bits, height, width)
    if best is not None and (not torch.is_tensor(best) or best.dtype != torch.int32
                             or tuple(best.shape) != (V, height, width) or not best.is_contiguous()):
        raise ValueError(f"ray_claims: best must be a contiguous int32 [{V},{height},{width}] tensor")
    if backend == "host":
        if best is None:
            best = torch.zeros((V, height, width), dtype=torch.int32)
        if best.is_cuda:
            raise ValueError("ray_claims: backend='host' claims into a CPU tensor")
        gate = _gate_args("ray_claims", depth, slack, bounds, dims, V, height, width, "host")
        out, words = best.numpy(), bits.detach().cpu().numpy().view(np.uint32)
        for s0 in range(0, idx.size, HOST_SLAB):
            pts = _centres_of(lo, dims, step, idx[s0:s0 + HOST_SLAB].astype(np.int64))
            for v in range(V):   # one view at a time: [slab] temporaries
                at, px, py = _hits_host(pts, K, M, words, height, width, v, gate)
                np.maximum.at(out[v], (py, px), sup[s0 + at].astype(np.int32))
        return best
    dev = ES._device_for([bits] + ([best] if best is not None else []), "ray_claims", device)
    with L.device_guard(dev):
        clear = best is None
        if clear:
            best = torch.empty((V, height, width), dtype=torch.int32, device=dev)
        elif best.device != dev:
            raise ValueError(f"ray_claims: best must be on {dev}")
        bits = bits.to(dev).contiguous()
        (Kd, Md), (lo_c, step_c) = ES.cameras_on(dev, K, M), _grid_c(lo, step)
        idx_d, sup_d = torch.from_numpy(idx).to(dev), torch.from_numpy(sup).to(dev)
        gate = _gate_args("ray_claims", depth, slack, bounds, dims, V, height, width, "gpu", dev)
        if gate is None:
            rc = L.load().cgs_ray_claims(*dims, lo_c, step_c, idx.size, L.ptr(idx_d), L.ptr(sup_d), V, L.ptr(Kd), L.ptr(Md),
                                         height, width, L.ptr(bits), 1 if clear else 0, L.ptr(best), L.raw_stream(dev))
            L.check(rc, "cgs_ray_claims")
        else:
            rc = L.load().cgs_ray_claims_depth(*dims, lo_c, step_c, idx.size, L.ptr(idx_d), L.ptr(sup_d), V, L.ptr(Kd),
                                               L.ptr(Md), height, width, L.ptr(bits), L.ptr(gate[0]), gate[1],
                                               1 if clear else 0, L.ptr(best), L.raw_stream(dev))
            L.check(rc, "cgs_ray_claims_depth")
    return best


def ray_wins(bounds, dims, index, support, intrinsics, w2c, bits, best, height, width, window=EXCL_WINDOW,
             margin=EXCL_MARGIN, counts=None, backend="gpu", device=None, depth=None, slack=None):
    """wins: uint16 [M] tensor, the wins of the module docstring over the views of this call.  ``best``: ``ray_claims`` of
    ALL listed voxels over the same views, int32 [V,height,width]; ``window`` an integer in [0, SEED_MAX_WINDOW],
    ``margin`` an integer in [0, 65535].  ``counts``: the wins of an earlier call over the same list -- this call's are
    added to it in place and it is returned (the views of all accumulating calls number at most 65535).
    ``backend="gpu"``: ``cgs_ray_wins``, a device tensor; ``backend="host"``: numpy, a CPU tensor.  ``depth``, ``slack``: the
    gate of ``voxel_votes`` (``cgs_ray_wins_depth``) -- a listed voxel that a view hides wins nothing there; ``best`` must
    then be the claims under the same gate."""
    _check_backend(backend)
    lo, dims, step, height, width, V, K, M, bits, idx, sup = _ray_args("ray_wins", bounds, dims, index, support, intrinsics,
                                                                       w2c, bits, height, width)
    window, margin = _check_window("ray_wins: the window", window), _check_margin("ray_wins: the margin", margin)
    if not torch.is_tensor(best):
        best = torch.from_numpy(np.ascontiguousarray(best))
    if best.dtype != torch.int32 or tuple(best.shape) != (V, height, width):
        raise ValueError(f"ray_wins: best must be int32 [{V},{height},{width}] (got {best.dtype} {tuple(best.shape)})")
    if counts is not None and (not torch.is_tensor(counts) or counts.dtype != torch.uint16
                               or tuple(counts.shape) != (idx.size,) or not counts.is_contiguous()):
        raise ValueError(f"ray_wins: counts must be a contiguous uint16 [{idx.size}] tensor")
    if backend == "host":
        wins = counts if counts is not None else torch.zeros(idx.size, dtype=torch.uint16)
        if wins.is_cuda:
            raise ValueError("ray_wins: backend='host' accumulates into a CPU tensor")
        out, words = wins.numpy(), bits.detach().cpu().numpy().view(np.uint32)
        claims = best.detach().cpu().numpy().view(np.uint32)
        gate = _gate_args("ray_wins", depth, slack, bounds, dims, V, height, width, "host")
        for s0 in range(0, idx.size, HOST_SLAB):
            pts = _centres_of(lo, dims, step, idx[s0:s0 + HOST_SLAB].astype(np.int64))
            for v in range(V):   # one view at a time: [slab] temporaries
                at, px, py = _hits_host(pts, K, M, words, height, width, v, gate)
                x0, x1 = np.maximum(px - window, 0), np.minimum(px + window, width - 1)
                y0, y1 = np.maximum(py - window, 0), np.minimum(py + window, height - 1)
                top = np.zeros(at.size, np.int64)
                for dy in range(-window, window + 1):       # the shifted maximum of the clipped window
                    for dx in range(-window, window + 1):
                        top = np.maximum(top, claims[v, np.clip(py + dy, y0, y1), np.clip(px + dx, x0, x1)])
                out[s0 + at] += (sup[s0 + at].astype(np.int64) + margin >= top).astype(np.uint16)
        return wins
    dev = ES._device_for([bits, best] + ([counts] if counts is not None else []), "ray_wins", device)
    with L.device_guard(dev):
        if counts is not None:
            wins = counts
            if wins.device != dev:
                raise ValueError(f"ray_wins: counts must be on {dev}")
        elif V == 0:   # no view: the call is a no-op and nothing is won
            wins = torch.zeros(idx.size, dtype=torch.uint16, device=dev)
        else:
            wins = torch.empty(idx.size, dtype=torch.uint16, device=dev)
        bits, best = bits.to(dev).contiguous(), best.to(dev).contiguous()
        (Kd, Md), (lo_c, step_c) = ES.cameras_on(dev, K, M), _grid_c(lo, step)
        idx_d, sup_d = torch.from_numpy(idx).to(dev), torch.from_numpy(sup).to(dev)
        gate = _gate_args("ray_wins", depth, slack, bounds, dims, V, height, width, "gpu", dev)
        if gate is None:
            rc = L.load().cgs_ray_wins(*dims, lo_c, step_c, idx.size, L.ptr(idx_d), L.ptr(sup_d), V, L.ptr(Kd), L.ptr(Md),
                                       height, width, L.ptr(bits), L.ptr(best), window, margin,
                                       1 if counts is not None else 0, L.ptr(wins), L.raw_stream(dev))
            L.check(rc, "cgs_ray_wins")
        else:
            rc = L.load().cgs_ray_wins_depth(*dims, lo_c, step_c, idx.size, L.ptr(idx_d), L.ptr(sup_d), V, L.ptr(Kd), L.ptr(Md),
                                             height, width, L.ptr(bits), L.ptr(best), L.ptr(gate[0]), gate[1], window, margin,
                                             1 if counts is not None else 0, L.ptr(wins), L.raw_stream(dev))
            L.check(rc, "cgs_ray_wins_depth")
    return wins


def select_exclusive(wins, hit, win_ratio):
    """bool [M] (numpy): wins >= need[hit] -- an integer comparison against ``need_table(win_ratio)``.  wins, hit: one value
    per listed voxel (hit = the vote's hit of that voxel)."""
    wins, hit = _counts_host(wins), _counts_host(hit)
    if wins.shape != hit.shape:
        raise ValueError("select_exclusive: wins and hit differ in shape")
    if (wins < 0).any() or (hit < 0).any():
        raise ValueError("select_exclusive: wins and hit must not be negative")
    _check_ratio("select_exclusive: win_ratio", win_ratio)
    need = need_table(win_ratio, int(hit.max()) if hit.size else 0)
    return wins >= need[hit]


# ------------------------------------------------------------------------------------------------ directions
def keep_bits(keep, dims):
    """The selection mask ``keep`` (bool [nx ny nz], x fastest, as ``select_voxels`` returns it) packed into the keep bits
    of the module docstring: an int32 [nz, ny, ceil(nx / 32)] CPU tensor.  numpy on both back ends: n / 8 bytes."""
    nx, ny, nz = (int(d) for d in dims)
    if min(nx, ny, nz) < 1:
        raise ValueError(f"dims must be three positive integers (got {(nx, ny, nz)})")
    keep = ES._host(keep).reshape(-1).astype(bool)
    if keep.size != nx * ny * nz:
        raise ValueError(f"keep_bits: keep must hold {nx * ny * nz} voxels (got {keep.size})")
    stride = bits_stride(nx)
    padded = np.zeros((nz, ny, stride * 32), bool)
    padded[:, :, :nx] = keep.reshape(nz, ny, nx)
    words = np.packbits(padded, axis=-1, bitorder="little").view("<u4")
    return torch.from_numpy(np.ascontiguousarray(words).view(np.int32).reshape(nz, ny, stride))


def _ball_offsets(radius):
    """int64 [K,3]: the offsets (dx, dy, dz) with dx^2 + dy^2 + dz^2 <= radius^2."""
    a = np.arange(-radius, radius + 1, dtype=np.int64)
    dz, dy, dx = np.meshgrid(a, a, a, indexing="ij")
    d = np.stack([dx.ravel(), dy.ravel(), dz.ravel()], 1)
    return d[(d * d).sum(1) <= radius * radius]


def _moments_host(words, dims, centres, radius):
    nx, ny, nz = dims
    words = words.view(np.uint32)
    d = _ball_offsets(radius)
    feat = np.stack([np.ones(len(d), np.int64), d[:, 0], d[:, 1], d[:, 2], d[:, 0] ** 2, d[:, 1] ** 2, d[:, 2] ** 2,
                     d[:, 0] * d[:, 1], d[:, 0] * d[:, 2], d[:, 1] * d[:, 2]], 1)
    out = np.zeros((centres.shape[0], MOMENT_VALUES), np.int64)
    per = max(1, HOST_SLAB // len(d))   # seeds per slab: [slab, K] temporaries
    for s0 in range(0, centres.shape[0], per):
        q = centres[s0:s0 + per, None, :] + d[None, :, :]
        x, y, z = q[..., 0], q[..., 1], q[..., 2]
        inside = (x >= 0) & (x < nx) & (y >= 0) & (y < ny) & (z >= 0) & (z < nz)
        xi, yi, zi = np.where(inside, x, 0), np.where(inside, y, 0), np.where(inside, z, 0)
        bit = (words[zi, yi, xi >> 5] >> (xi & 31).astype(np.uint32)) & np.uint32(1)
        out[s0:s0 + per] = (inside & (bit != 0)).astype(np.int64) @ feat
    return out.astype(np.int32)


def voxel_moments(bits, dims, centres, radius, backend="gpu", device=None):
    """int32 [N,10] tensor: the moments of the module docstring of the kept voxels within ``radius`` voxels of every
    centre.  bits: ``keep_bits``, int32 [nz, ny, ceil(nx / 32)] (tensor or array); centres: integer [N,3] voxel
    coordinates inside the grid.  ``backend="gpu"``: ``cgs_voxel_moments``, a device tensor; ``backend="host"``: numpy, a
    CPU tensor.  A centre outside the grid, a radius outside [1, SEED_MAX_RADIUS] and bits of another shape or dtype are
    ValueErrors."""
    _check_backend(backend)
    dims = tuple(int(v) for v in dims)
    if len(dims) != 3 or min(dims) < 1:
        raise ValueError(f"dims must be three positive integers (got {dims})")
    if dims[0] * dims[1] * dims[2] > MAX_VOXELS:
        raise ValueError(f"a grid holds at most 2^31 - 1 voxels (got {dims})")
    if int(radius) != radius or not (1 <= int(radius) <= SEED_MAX_RADIUS):
        raise ValueError(f"voxel_moments: the radius must be an integer in [1, {SEED_MAX_RADIUS}] (got {radius})")
    radius = int(radius)
    if not torch.is_tensor(bits):
        bits = torch.from_numpy(np.ascontiguousarray(bits))
    want = (dims[2], dims[1], bits_stride(dims[0]))
    if bits.dtype != torch.int32 or tuple(bits.shape) != want:
        raise ValueError(f"voxel_moments: bits must be int32 {list(want)} (got {bits.dtype} {tuple(bits.shape)})")
    cen = ES._host(centres)
    if cen.size == 0:
        cen = cen.reshape(0, 3)
    if cen.ndim != 2 or cen.shape[1] != 3 or cen.dtype.kind not in "iu":
        raise ValueError("voxel_moments: centres must be integer [N,3] voxel coordinates")
    cen = np.ascontiguousarray(cen.astype(np.int64))
    if cen.shape[0] and ((cen < 0).any() or (cen >= np.array(dims, np.int64)[None, :]).any()):
        raise ValueError(f"voxel_moments: a centre lies outside the {dims} grid")
    N = cen.shape[0]
    if backend == "host":
        return torch.from_numpy(_moments_host(np.ascontiguousarray(bits.detach().cpu().numpy()), dims, cen, radius))
    dev = ES._device_for([bits], "voxel_moments", device)
    with L.device_guard(dev):
        bits = bits.to(dev).contiguous()
        cen_d = torch.from_numpy(cen.astype(np.int32)).to(dev)
        out = torch.empty((N, MOMENT_VALUES), dtype=torch.int32, device=dev)
        if N > 0:
            rc = L.load().cgs_voxel_moments(dims[0], dims[1], dims[2], L.ptr(bits), N, L.ptr(cen_d), radius, L.ptr(out),
                                            L.raw_stream(dev))
            L.check(rc, "cgs_voxel_moments")
    return out


def seed_directions(moments, min_support=DIR_MIN_SUPPORT, min_linearity=DIR_MIN_LINEARITY):
    """moments: int32 [N,10] (``voxel_moments``; tensor or array).  Returns (directions float64 [N,3] -- unit rows, zero
    rows for undirected seeds --, directed bool [N], linearity float64 [N]) by the direction rule of the module docstring.
    Host float64 code on both back ends."""
    mom = ES._host(moments).astype(np.int64)
    if mom.ndim != 2 or mom.shape[1] != MOMENT_VALUES:
        raise ValueError(f"seed_directions: moments must be [N,{MOMENT_VALUES}]")
    N = mom.shape[0]
    if N == 0:
        return np.zeros((0, 3), np.float64), np.zeros(0, bool), np.zeros(0, np.float64)
    m, s = mom[:, 0], mom[:, 1:4]
    second = np.empty((N, 3, 3), np.int64)
    for (a, b), col in (((0, 0), 4), ((1, 1), 5), ((2, 2), 6), ((0, 1), 7), ((0, 2), 8), ((1, 2), 9)):
        second[:, a, b] = second[:, b, a] = mom[:, col]
    scatter = m[:, None, None] * second - s[:, :, None] * s[:, None, :]   # int64: below 2^63 by the bound on the moments
    lam, vec = np.linalg.eigh(scatter.astype(np.float64))
    top = vec[:, :, 2]
    lead = np.argmax(np.abs(top), axis=1)                                  # the first of equal magnitudes: the lowest axis
    top = np.where(top[np.arange(N), lead][:, None] < 0.0, -top, top)
    positive = lam[:, 2] > 0.0
    linearity = np.where(positive, (lam[:, 2] - lam[:, 1]) / np.where(positive, lam[:, 2], 1.0), 0.0)
    directed = (m >= int(min_support)) & (linearity >= float(min_linearity))
    return np.where(directed[:, None], top, 0.0), directed, linearity


# ------------------------------------------------------------------------------------------------ a scan
def grid_dims(bounds, grid):
    """``grid`` voxels along the longest side of the box, the other axes rounded so that the voxels are near-cubic."""
    lo, hi = (np.asarray(b, np.float64).reshape(-1) for b in bounds)
    grid = int(grid)
    if grid < 1:
        raise ValueError(f"grid must be positive (got {grid})")
    if lo.shape != (3,) or hi.shape != (3,) or not (np.isfinite(lo).all() and np.isfinite(hi).all() and (hi > lo).all()):
        raise ValueError(f"bounds must be finite with hi > lo on every axis (got lo={lo.tolist()}, hi={hi.tolist()})")
    ext = hi - lo
    voxel = ext.max() / grid
    return tuple(int(max(1, min(grid, round(e / voxel)))) for e in ext)


def seed_points(cameras, edge_maps_u8, detector, bounds, grid=128, tol_px=2, min_views=3, min_ratio=0.8, cell=4,
                max_seeds=20000, edge_threshold=EDGE_MAX_THRESHOLD, backend="gpu", device=None, budget_bytes=None,
                directions=False, dir_radius=DIR_RADIUS, dir_min_support=DIR_MIN_SUPPORT,
                dir_min_linearity=DIR_MIN_LINEARITY, exclusive=False, excl_window=EXCL_WINDOW, excl_margin=EXCL_MARGIN,
                excl_win_ratio=EXCL_WIN_RATIO, thin=False, occluder=None, depth_maps=None, depth_slack=None,
                depth_window=EO.DEPTH_WINDOW, near_clip=None):
    """cameras: ``NovelViewCamera`` s; edge_maps_u8: one uint8 [H,W] map per camera (a list or an [V,H,W] array), the
    stored bytes of the detector's maps, as ``score_edges`` takes them.  bounds = (lo, hi) of the box to search.

    A pixel is detected when ``reprojection.detected_lut(detector, edge_threshold)`` says so; every view's detected mask
    goes through ``edt_squared`` and ``near_bits(tol_px)``; the views vote on a grid of ``grid`` voxels along the longest
    side (``grid_dims``); ``select_voxels(min_views, min_ratio)`` and ``thin_to_seeds(cell, max_seeds)`` give the seeds.
    Views are grouped by size and processed ``budget_bytes`` (default BYTE_BUDGET; 8 bytes per pixel, at least one view)
    at a time; the votes accumulate across the chunks, so the result does not depend on the chunking.

    Returns (seeds float64 [N,3], info) with info = {"dims", "voxels", "views", "kept_voxels", "cells", "seeds", "capped",
    "backend"}.  THE DEFAULTS ARE UNTUNED (no scan has been measured against them), the vote reasons about occlusion only
    when it is given a depth source (below; ``exclusive=True`` suppresses ghosts without depth), and the curve direction is
    not seeded unless ``directions=True``.  ``backend``: "gpu" (HIP; ``device``) or "host" (numpy).

    Depth (opt-in; at most one of the two, with the meaning and the checks of ``edge_support``): ``occluder`` -- float32
    [F,3,3] triangles or the path of an .obj / .ply mesh -- or ``depth_maps`` -- one float [H,W] array of camera z per
    camera -- give every chunk of views its depth planes (``edge_occlusion.ChunkDepth``: the window maximum of radius
    ``depth_window``, 8 bytes per pixel more, in both sweeps), and a view whose plane has a surface more than
    ``depth_slack`` in front of a voxel's centre does not see the voxel: it counts in neither seen nor hit, claims nothing
    and wins nothing (``voxel_votes``, ``ray_claims``, ``ray_wins`` with ``depth=``).  On a scan whose hidden lines are
    removed -- every real scan of a solid -- the ungated vote counts the views that look at a rim through the solid in seen,
    hit / seen stays below ``min_ratio`` and nothing is kept; the gate is the way out that lets no ghosts in.
    ``depth_slack=None`` is HALF THE VOXEL DIAGONAL (``default_slack``): the centre of a voxel that holds an edge can lie
    that far behind the surface that carries the edge, and ``edge_occlusion.DEPTH_SLACK``, made for samples, is far too
    tight for a voxel.  UNTUNED: one host prototype on the drawn solids of scene/solid_scan.py, no real scan -- unit-cube
    bounds, grid 64 (voxel diagonal 0.0271), 24 views of 240x320, tol_px 2, min_views 3, min_ratio 0.8, window 1, the scan's
    own z-buffer as depth maps, ground truth sampled at 0.005; "uncovered" = ground-truth samples with no kept centre
    within two diagonals, "far" = kept centres farther than 0.02 from the ground truth:

        solid      kept, ungated  uncovered, ungated  kept, gated  uncovered, gated  worst sample->kept, gated  far, gated
        box                   22         961 of 1192          903                 0                      0.012           0
        l_bracket             41         974 of 1430          960                 0                     0.0102           1
        cylinder               0          all of 752          541                 0                      0.017           0

    A slack of 1 or 2 diagonals still covers every sample and lets 15 far voxels through on l_bracket; ungated at
    min_ratio 0.5 every sample is covered too, with 38 far voxels on the box.  info then also holds the keys of
    ``ChunkDepth.settings()`` ("occluder" or "depth_maps", "depth_slack", "depth_window") and "hidden_pairs", the
    (voxel, view) pairs the gate hid, summed over the grid.  With neither source nothing changes: no key is added.  The
    gate's limits are those of ops/edge_occlusion.py: no near-plane clipping unless ``near_clip`` is given, concave edges can be hidden by their own faces.

    ``directions=True``: the kept voxels within ``dir_radius`` voxels of every seed's centre voxel give its direction
    (``keep_bits``, ``voxel_moments`` on ``backend``, ``seed_directions(dir_min_support, dir_min_linearity)``; module
    docstring); info additionally holds "directions" (float64 [N,3]: unit rows, zero rows for undirected seeds) and
    "directed" (their count).  These three defaults are untuned too.

    ``exclusive=True``: between the selection and the thinning the kept voxels claim the pixels they hit and only those
    that win their claims stay (``voxel_support``, ``ray_claims``, ``ray_wins(excl_window, excl_margin)``,
    ``select_exclusive(excl_win_ratio)``; module docstring).  A second sweep over the views does it chunk by chunk: the
    packed near bits of the first sweep are kept, view by view (one bit per pixel), ``best`` costs
    EXCL_BYTES_PER_PIXEL bytes per pixel of ``budget_bytes``, and the wins accumulate across the chunks, so the result
    does not depend on the chunking.  The thinning, the keep bits and the moments see the surviving mask; info
    additionally holds "exclusive_voxels", the voxels that remain ("kept_voxels" keeps its meaning).  These three
    defaults are untuned too; the pass itself uses no depth beyond the gate above, when that is given.

    ``thin=True``: every chunk's detected masks go through ``edge_thin.thin_masks`` on the same back end before the
    transform (a detector's response several pixels wide widens the near band by half its width; 2 bytes per pixel,
    released before the transform is allocated; untuned, limits in ops/edge_thin.py); info then holds "thin": True, and
    nothing otherwise."""
    _check_backend(backend)
    lut = detected_lut(detector, edge_threshold)
    cameras, maps = check_edge_maps("seed_points", cameras, edge_maps_u8)
    if len(cameras) > MAX_VIEWS:
        raise ValueError(f"seed_points: at most {MAX_VIEWS} views (got {len(cameras)})")
    ES.tolerances_squared([tol_px])
    if directions and (int(dir_radius) != dir_radius or not (1 <= int(dir_radius) <= SEED_MAX_RADIUS)):
        raise ValueError(f"seed_points: dir_radius must be an integer in [1, {SEED_MAX_RADIUS}] (got {dir_radius})")
    if exclusive:
        _check_window("seed_points: excl_window", excl_window)
        _check_margin("seed_points: excl_margin", excl_margin)
        _check_ratio("seed_points: excl_win_ratio", excl_win_ratio)
    dims = grid_dims(bounds, grid)
    _grid(bounds, dims)
    need_table(min_ratio, 0)
    budget = check_budget("seed_points", budget_bytes, BYTE_BUDGET)
    gate = EO.ChunkDepth("seed_points", cameras, occluder, depth_maps,
                         default_slack(bounds, dims) if depth_slack is None else depth_slack, depth_window, near_clip)
    if backend == "gpu":
        device = ES._device_for([], "seed_points", device)
    gate.to(backend, device)
    n = dims[0] * dims[1] * dims[2]
    on = {"backend": backend, "device": device}

    def gated(H, W, sel, intr, w2c):   # the gate's arguments of one chunk of views: its planes are built here, per chunk
        return {"depth": gate.planes(H, W, sel, intr, w2c), "slack": gate.slack} if gate.gated else {}

    counts, near = None, {}   # near: every view's near bits of the first sweep, for the second
    for H, W, sel, intr, w2c in view_chunks(cameras, BYTES_PER_PIXEL + gate.bytes_per_pixel, budget):
        det = detected_masks(lut, maps, sel)
        if thin:
            det = thin_masks(det, **on)
        d2 = ES.edt_squared(det, **on)
        del det
        bits = near_bits(d2, tol_px, **on)
        del d2
        counts = voxel_votes(bounds, dims, intr, w2c, bits, H, W, counts=counts, return_hidden=gate.gated,
                             **gated(H, W, sel, intr, w2c), **on)
        if exclusive:
            near.update(zip(sel, bits))
    if counts is None:   # no view: nothing is seen
        counts = tuple(torch.zeros(n, dtype=torch.uint16) for _ in range(3 if gate.gated else 2))
    seen, hit = (c.cpu().numpy() for c in counts[:2])
    keep = select_voxels(seen, hit, min_views, min_ratio)
    kept_voxels = int(np.count_nonzero(keep))
    if exclusive:   # the second sweep: the kept voxels claim their pixels, chunk of views by chunk of views
        index = np.nonzero(keep)[0].astype(np.int32)
        support = voxel_support(seen, hit, index)
        wins = None
        for H, W, sel, intr, w2c in view_chunks(cameras, EXCL_BYTES_PER_PIXEL + gate.bytes_per_pixel, budget):
            args = (bounds, dims, index, support, intr, w2c, torch.stack([near[v] for v in sel]))
            planes = gated(H, W, sel, intr, w2c)
            best = ray_claims(*args, H, W, **planes, **on)
            wins = ray_wins(*args, best, H, W, window=excl_window, margin=excl_margin, counts=wins, **planes, **on)
            del best, planes
        del near
        if wins is None:   # no view
            wins = torch.zeros(index.size, dtype=torch.uint16)
        keep = np.zeros(n, bool)
        keep[index[select_exclusive(wins, hit[index], excl_win_ratio)]] = True
    seeds, cells = thin_to_seeds(keep, hit, bounds, dims, cell, max_seeds, return_centres=bool(directions))
    info = {"dims": dims, "voxels": n, "views": len(cameras), "kept_voxels": kept_voxels,
            "cells": cells["cells"], "seeds": int(seeds.shape[0]), "capped": cells["capped"], "backend": backend}
    if thin:
        info["thin"] = True
    if gate.gated:
        info.update(gate.settings())
        info["hidden_pairs"] = int(counts[2].cpu().numpy().astype(np.int64).sum())
    if exclusive:
        info["exclusive_voxels"] = int(np.count_nonzero(keep))
    if directions:
        moments = voxel_moments(keep_bits(keep, dims), dims, cells["centre_voxel"], dir_radius, **on)
        vectors, directed, _ = seed_directions(moments, dir_min_support, dir_min_linearity)
        info["directions"], info["directed"] = vectors, int(np.count_nonzero(directed))
    return seeds, info
