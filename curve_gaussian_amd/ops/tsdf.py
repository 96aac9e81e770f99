"""A mesh occluder from per-view depth maps: a truncated signed distance field (TSDF) over the voxel centres of a grid, and
its zero surface as a triangle soup by marching tetrahedra (cgs_tsdf_integrate / cgs_tsdf_mesh_count / cgs_tsdf_mesh_emit,
include/curvegs.h; csrc/tsdf.hip).  The reference has no counterpart.  The maps are ``stereo_depth``'s (fused or not), a
z-buffer's planes or a sensor's; the soup is what ``read_triangle_mesh`` reads, so everything that takes ``--occluder`` takes
it, ``--ignore_contours`` and ``--near_clip`` included -- the two options that ``--depth_dir`` cannot serve.

  integrate     the maps of same-size views into the state (sum float64 [n], weight uint16 [n]) of a lattice
  extract       the state's surface: float32 [T,3,3], every triangle of the rule, ordered by cell
  drop_degenerate   the soup without the triangles that have two bitwise-equal vertices
  tsdf_mesh     depth maps and cameras in, the soup and an ``info`` record out

The field AVERAGES the signed distances the views report at a lattice point (it takes no minimum: noise on either side of
the surface cancels instead of pulling the surface toward the cameras), so all views share one surface.  The rule is frozen
in include/curvegs.h -- float64, one rounded operation at a time, running sums in view order -- and stated once for the
kernels in csrc/tsdf.h.  Two back ends: ``"gpu"``, HIP, and ``"host"``, numpy written operation for operation, so the two
agree BIT FOR BIT, and so does the brute force of tests/tsdf_cases.py.

WHAT THIS IS NOT.  A dense volume with weights of 1 and nearest-pixel depth reads: no sparse or hashed volume, no weights
by angle or distance, no bilinear reads, no colour, no carving from empty pixels (a pixel without a depth says nothing), no
removal of small floating components.  ``stereo_depth``, ``mesh_depth``, ``mesh_edges`` and the gate are untouched.  EVERY
DEFAULT BELOW IS UNTUNED: only the drawn solids of scene/solid_scan.py have been checked."""
import itertools

import numpy as np
import torch

from .. import _lib as L
from . import edge_occlusion as EO
from . import edge_score as ES
from . import edge_seed as SEED
from . import mesh_contours as MC
from .stereo_depth import BOUNDS
from .view_chunks import check_budget, view_chunks

GRID = 128                 # UNTUNED: lattice points along the longest side of the bounds
TRUNC_STEPS = 4.0          # UNTUNED: the truncation distance over the longest step of the lattice
MIN_WEIGHT = 2             # UNTUNED: a cell needs this many observing views at every corner
SLACK_DIAGONALS = 2.0      # UNTUNED: recommended_slack over the voxel diagonal
MAX_WEIGHT = L.TSDF_MAX_WEIGHT
CELL_MAX_TRIS = 12
BYTE_BUDGET = 1 << 30      # bytes of depth planes per chunk of views in tsdf_mesh
BYTES_PER_PIXEL = 4        # the float32 plane
HOST_SLAB = 1 << 18        # lattice points per numpy slab of the host back end


# ------------------------------------------------------------------------------------------------ the cases, derived
def _tets():
    """[(q0, q1, q2, q3), odd] of the 6 Kuhn tetrahedra: the orders of the axes in lexicographic order."""
    out = []
    for a, b, c in itertools.permutations(range(3)):
        odd = ((a > b) + (a > c) + (b > c)) % 2 == 1
        out.append(((0, 1 << a, (1 << a) | (1 << b), 7), odd))
    return out


def _case(m):
    """The triangles of an even tetrahedron with inside mask m: a list of ((lo, hi), (lo, hi), (lo, hi))."""
    ins = [x for x in range(4) if (m >> x) & 1]
    outs = [x for x in range(4) if not (m >> x) & 1]
    edge = lambda x, y: (min(x, y), max(x, y))
    turn = lambda t, turned: (t[0], t[2], t[1]) if turned else t
    if len(ins) in (0, 4):
        return []
    if len(ins) == 1:
        x = ins[0]
        return [turn(tuple(edge(x, o) for o in outs), x % 2 == 1)]
    if len(ins) == 3:
        x = outs[0]
        return [turn(tuple(edge(x, o) for o in ins), x % 2 == 0)]
    p = ins + outs
    turned = sum(p[x] > p[y] for x in range(4) for y in range(x + 1, 4)) % 2 == 1
    A, B, Cc, D = edge(p[0], p[2]), edge(p[0], p[3]), edge(p[1], p[3]), edge(p[1], p[2])
    return [turn((A, B, Cc), turned), turn((A, Cc, D), turned)]


TETS = _tets()
CASES = [_case(m) for m in range(16)]
_NTRI = np.array([len(c) for c in CASES], np.int64)


# ------------------------------------------------------------------------------------------------ checks
def _dims(bounds, grid):
    """``grid``: three lattice dimensions, or one number for ``edge_seed.grid_dims`` of the bounds."""
    if np.ndim(grid) == 0:
        return SEED.grid_dims(bounds, grid)
    return tuple(int(d) for d in grid)


def _check_trunc(what, trunc):
    trunc = float(trunc)
    if not (trunc > 0.0 and np.isfinite(trunc)):
        raise ValueError(f"{what}: trunc must be finite and > 0 (got {trunc})")
    return trunc


def _check_min_weight(what, min_weight):
    if int(min_weight) != min_weight or not 1 <= int(min_weight) <= MAX_WEIGHT:
        raise ValueError(f"{what}: min_weight must be an integer in [1, {MAX_WEIGHT}] (got {min_weight})")
    return int(min_weight)


def _check_state(what, state, n):
    s, w = state
    for t, dt in ((s, torch.float64), (w, torch.uint16)):
        if not torch.is_tensor(t) or t.dtype != dt or tuple(t.shape) != (n,) or not t.is_contiguous():
            raise ValueError(f"{what}: the state is (sum float64 [{n}], weight uint16 [{n}]), contiguous tensors")
    if s.device != w.device:
        raise ValueError(f"{what}: sum and weight must be on one device")
    return s, w


def default_trunc(bounds, grid):
    """``TRUNC_STEPS`` x the longest step of the lattice.  UNTUNED."""
    _, _, _, step = SEED._grid(bounds, _dims(bounds, grid))
    return TRUNC_STEPS * float(step.max())


def voxel_diagonal(bounds, grid):
    _, _, _, step = SEED._grid(bounds, _dims(bounds, grid))
    return float(np.sqrt((step * step).sum()))


# ------------------------------------------------------------------------------------------------ integration
def _integrate_host(lo, dims, step, K, M, planes, H, W, trunc, acc_all, wt_all):
    n = dims[0] * dims[1] * dims[2]
    for s0 in range(0, n, HOST_SLAB):
        s1 = min(n, s0 + HOST_SLAB)
        pts = SEED._centres(lo, dims, step, s0, s1).astype(np.float64)
        acc, wt = acc_all[s0:s1], wt_all[s0:s1].astype(np.int64)
        for v in range(K.shape[0]):   # in view order: the running sum of the rule
            c2, u, vv = EO._camera_points_host(pts, K[v], M[v])
            with np.errstate(all="ignore"):
                keep = ~(c2 <= 0.0) & (u >= 0.0) & (u < float(W)) & (vv >= 0.0) & (vv < float(H))
                idx = np.flatnonzero(keep)
                d = planes[v][np.floor(vv[idx]).astype(np.int64), np.floor(u[idx]).astype(np.int64)].astype(np.float64)
                sdf = d - c2[idx]
                ok = (d > 0.0) & (d < np.inf) & ~(sdf < -trunc) & (wt[idx] < MAX_WEIGHT)
                t = sdf / trunc
                t = np.where(t > 1.0, 1.0, t)
            sel = idx[ok]
            acc[sel] = acc[sel] + t[ok]
            wt[sel] += 1
        wt_all[s0:s1] = wt.astype(np.uint16)


def integrate(depth, intrinsics, w2c, grid, bounds, trunc, state=None, backend="gpu", device=None):
    """(sum float64 [n], weight uint16 [n]) tensors: cgs_tsdf_integrate of the views of this call into the lattice ``grid``
    (three dimensions, or one number for ``edge_seed.grid_dims``) of ``bounds``.  depth float32 [V,H,W], camera z; an entry
    that is not a positive finite number says nothing.  intrinsics [V,4], w2c [V,3,4] float64.  ``state``: the pair of an
    earlier call over the same lattice -- the views are added to it in place, in order, and it is returned; chunked calls
    give the bits of a single one.  ``backend="gpu"``: device tensors; ``"host"``: numpy, CPU tensors, the same bits."""
    ES._check_backend(backend)
    lo, _, dims, step = SEED._grid(bounds, _dims(bounds, grid))
    trunc = _check_trunc("tsdf integrate", trunc)
    V, K, M = ES._cameras(intrinsics, w2c)
    if V > SEED.MAX_VIEWS:
        raise ValueError(f"tsdf integrate: at most {SEED.MAX_VIEWS} views a call (got {V})")
    d = depth if torch.is_tensor(depth) else torch.from_numpy(np.array(depth, order="C"))
    if d.dim() != 3:
        raise ValueError(f"tsdf integrate: depth must be float32 [V,H,W] (got {tuple(d.shape)})")
    H, W = ES._check_size("tsdf integrate", d.shape[1], d.shape[2])
    d = EO._as_depth(d, V, H, W, "tsdf integrate")
    n = dims[0] * dims[1] * dims[2]
    if state is not None:
        state = _check_state("tsdf integrate", state, n)
    if backend == "host":
        if d.is_cuda or (state is not None and state[0].is_cuda):
            raise ValueError("tsdf integrate: backend='host' takes host arrays and CPU tensors")
        out = state if state is not None else (torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.uint16))
        _integrate_host(lo, dims, step, K, M, d.numpy(), H, W, trunc, out[0].numpy(), out[1].numpy())
        return out
    dev = ES._device_for([d] + list(state or []), "tsdf integrate", device)
    with L.device_guard(dev):
        if state is not None:
            if state[0].device != dev:
                raise ValueError(f"tsdf integrate: the state must be on {dev}")
            out = state
        else:
            out = (torch.empty(n, dtype=torch.float64, device=dev), torch.empty(n, dtype=torch.uint16, device=dev))
        d = d.to(dev)
        (Kd, Md), (lo_c, step_c) = ES.cameras_on(dev, K, M), SEED._grid_c(lo, step)
        rc = L.load().cgs_tsdf_integrate(*dims, lo_c, step_c, V, L.ptr(Kd), L.ptr(Md), H, W, L.ptr(d), trunc,
                                         1 if state is not None else 0, L.ptr(out[0]), L.ptr(out[1]), L.raw_stream(dev))
        L.check(rc, "cgs_tsdf_integrate")
    return out


# ------------------------------------------------------------------------------------------------ extraction
def _axis_coords(lo, step, n, axis):
    """float64 [n]: coordinate `axis` of the lattice points, the float32 rounding of seed_centre widened again."""
    return (lo[axis] + (np.arange(n, dtype=np.float64) + 0.5) * step[axis]).astype(np.float32).astype(np.float64)


def _count_host(dims, s, w, min_weight):
    """(counts uint8 [cells], f float64 [8,cells], live bool [cells]) of a lattice with cells."""
    nx, ny, nz = dims
    S, Wt = s.reshape(nz, ny, nx), w.reshape(nz, ny, nx)
    with np.errstate(all="ignore"):
        F = S / Wt.astype(np.float64)
    corner = lambda A, c: A[(c >> 2):nz - 1 + (c >> 2), ((c >> 1) & 1):ny - 1 + ((c >> 1) & 1), (c & 1):nx - 1 + (c & 1)]
    f = np.stack([corner(F, c).reshape(-1) for c in range(8)])
    live = np.ones(f.shape[1], bool)
    for c in range(8):
        live &= corner(Wt, c).reshape(-1) >= min_weight
    with np.errstate(invalid="ignore"):
        inside = f < 0.0
    counts = np.zeros(f.shape[1], np.int64)
    for q, _ in TETS:
        counts += _NTRI[sum(inside[q[x]].astype(np.int64) << x for x in range(4))]
    return np.where(live, counts, 0).astype(np.uint8), f, live


def _extract_host(lo, dims, step, s, w, min_weight):
    nx, ny, nz = dims
    if min(dims) < 2:
        return np.zeros((0,), np.uint8), np.zeros((0, 3, 3), np.float32)
    counts, f, _ = _count_host(dims, s, w, min_weight)
    offsets = np.cumsum(counts.astype(np.int64)) - counts
    tris = np.zeros((int(counts.sum(dtype=np.int64)), 3, 3), np.float32)
    act = np.flatnonzero(counts)
    f = f[:, act]
    ci, cj, ck = act % (nx - 1), (act // (nx - 1)) % (ny - 1), act // ((nx - 1) * (ny - 1))
    coords = [_axis_coords(lo, step, n, a) for a, n in enumerate(dims)]
    ends = [[coords[0][ci], coords[0][ci + 1]], [coords[1][cj], coords[1][cj + 1]], [coords[2][ck], coords[2][ck + 1]]]
    at = offsets[act]
    for q, odd in TETS:
        g = f[list(q)]
        with np.errstate(invalid="ignore"):
            m = sum((g[x] < 0.0).astype(np.int64) << x for x in range(4))
        for mm in range(1, 15):
            sel = np.flatnonzero(m == mm)
            if sel.size == 0:
                continue
            for r, tri in enumerate(CASES[mm]):
                if odd:
                    tri = (tri[0], tri[2], tri[1])
                for k, (a, b) in enumerate(tri):
                    fa, fb = g[a][sel], g[b][sel]
                    with np.errstate(all="ignore"):
                        wgt = fa / (fa - fb)
                        for axis in range(3):
                            pa, pb = ends[axis][(q[a] >> axis) & 1][sel], ends[axis][(q[b] >> axis) & 1][sel]
                            tris[at[sel] + r, k, axis] = (pa + wgt * (pb - pa)).astype(np.float32)
        at = at + _NTRI[m]
    return counts, tris


def extract(sum, weight, grid, bounds, min_weight=MIN_WEIGHT, backend="gpu", device=None, return_counts=False):
    """float32 [T,3,3] tensor: the surface of the state (``integrate``) by cgs_tsdf_mesh_count, an exclusive scan
    (``torch.cumsum``) and cgs_tsdf_mesh_emit -- EVERY triangle of the rule, those with equal vertices too
    (``drop_degenerate``), ordered by cell, tetrahedron, triangle; normals point from inside (f < 0) to outside.
    ``return_counts``: also the uint8 [cells] triangle counts."""
    ES._check_backend(backend)
    lo, _, dims, step = SEED._grid(bounds, _dims(bounds, grid))
    min_weight = _check_min_weight("tsdf extract", min_weight)
    n = dims[0] * dims[1] * dims[2]
    s, w = _check_state("tsdf extract", (sum, weight), n)
    cells = (dims[0] - 1) * (dims[1] - 1) * (dims[2] - 1)
    if backend == "host":
        if s.is_cuda:
            raise ValueError("tsdf extract: backend='host' takes CPU tensors")
        counts, tris = _extract_host(lo, dims, step, s.numpy(), w.numpy(), min_weight)
        counts, tris = torch.from_numpy(counts), torch.from_numpy(tris)
        return (tris, counts) if return_counts else tris
    dev = ES._device_for([s], "tsdf extract", device)
    with L.device_guard(dev):
        s, w = s.to(dev), w.to(dev)
        lib, stream = L.load(), L.raw_stream(dev)
        counts = torch.empty(cells, dtype=torch.uint8, device=dev)
        L.check(lib.cgs_tsdf_mesh_count(*dims, L.ptr(s), L.ptr(w), min_weight, L.ptr(counts), stream), "cgs_tsdf_mesh_count")
        ends = torch.cumsum(counts, 0, dtype=torch.int64)
        offsets = (ends - counts).contiguous()
        T = int(ends[-1]) if cells > 0 else 0
        tris = torch.empty((T, 3, 3), dtype=torch.float32, device=dev)
        lo_c, step_c = SEED._grid_c(lo, step)
        L.check(lib.cgs_tsdf_mesh_emit(*dims, lo_c, step_c, L.ptr(s), L.ptr(w), min_weight, L.ptr(offsets), T, L.ptr(tris),
                                       stream), "cgs_tsdf_mesh_emit")
    return (tris, counts) if return_counts else tris


def drop_degenerate(tris):
    """(float32 [F,3,3] numpy soup without the triangles that have two bitwise-equal vertices, the number dropped).  Such a
    triangle arises where an outside corner is exactly 0: its vertices on that corner's edges all sit on the corner."""
    t = np.ascontiguousarray(ES._host(tris), np.float32).reshape(-1, 3, 3)
    b = t.view(np.uint32)
    same = lambda x, y: (b[:, x] == b[:, y]).all(1)
    bad = same(0, 1) | same(1, 2) | same(0, 2)
    return np.ascontiguousarray(t[~bad]), int(bad.sum())


# ------------------------------------------------------------------------------------------------ maps in, mesh out
def tsdf_mesh(depth_maps, cameras, grid=GRID, bounds=BOUNDS, trunc=None, min_weight=MIN_WEIGHT, backend="gpu", device=None,
              budget_bytes=None):
    """(tris float32 [F,3,3] numpy, info): the TSDF mesh of one depth map per camera.  depth_maps: a float [H,W] array of
    camera z per ``NovelViewCamera``, of its camera's size; an entry that is not a positive finite number (``stereo_depth``'s
    0, a z-buffer's +inf, a NaN) says nothing.  The views are grouped by size and walked by ``ops.view_chunks`` in chunks
    whose planes fit ``budget_bytes`` (default ``BYTE_BUDGET``); the state accumulates across the chunks and the mesh does
    not depend on them when all views have one size (views of another size come after, in their own order).  Triangles
    with two bitwise-equal vertices are dropped.  OFF BY DEFAULT everywhere: nothing calls this but its tool.  UNTUNED:
    ``grid`` (128 points along the longest side), ``trunc`` (None: ``TRUNC_STEPS`` = 4 x the longest step), ``min_weight``
    (2).

    info: "dims", "lo", "step" (the lattice), "trunc", "min_weight", "views", "observed" (lattice points with weight > 0),
    "live_cells", "triangles" (kept), "degenerate" (dropped), "boundary" and "non_manifold" (``mesh_edges`` of the kept soup),
    "voxel_diagonal" and "recommended_slack" = ``SLACK_DIAGONALS`` x the voxel diagonal (UNTUNED; the edge vote's reasoning: a
    surface can sit that far from where the lattice resolves it)."""
    ES._check_backend(backend)
    cams, maps = list(cameras), [ES._host(m) for m in depth_maps]
    if len(cams) != len(maps):
        raise ValueError(f"tsdf_mesh: {len(cams)} cameras and {len(maps)} depth maps")
    for c, m in zip(cams, maps):
        if m.dtype.kind != "f" or m.shape != (c.height, c.width):
            raise ValueError(f"tsdf_mesh: the depth map of {c.name} must be a float [{c.height},{c.width}] array "
                             f"(got {m.dtype} {m.shape})")
    dims = _dims(bounds, grid)
    lo, _, dims, step = SEED._grid(bounds, dims)
    trunc = default_trunc(bounds, dims) if trunc is None else _check_trunc("tsdf_mesh", trunc)
    min_weight = _check_min_weight("tsdf_mesh", min_weight)
    budget = check_budget("tsdf_mesh", budget_bytes, BYTE_BUDGET)
    if len(cams) > MAX_WEIGHT:
        raise ValueError(f"tsdf_mesh: at most {MAX_WEIGHT} views (got {len(cams)})")
    n = dims[0] * dims[1] * dims[2]
    dev = ES._device_for([], "tsdf_mesh", device) if backend == "gpu" else torch.device("cpu")
    state = (torch.zeros(n, dtype=torch.float64, device=dev), torch.zeros(n, dtype=torch.uint16, device=dev))
    for H, W, sel, intr, w2c in view_chunks(cams, BYTES_PER_PIXEL, budget):
        planes = np.stack([maps[v].astype(np.float32) for v in sel])
        integrate(planes, intr, w2c, dims, bounds, trunc, state, backend, device)
    tris, dropped = drop_degenerate(extract(state[0], state[1], dims, bounds, min_weight, backend, device))
    edges = MC.mesh_edges(tris)
    diag = float(np.sqrt((step * step).sum()))
    info = {"dims": [int(d) for d in dims], "lo": lo.tolist(), "step": step.tolist(), "trunc": trunc, "min_weight": min_weight,
            "views": len(cams), "observed": int((state[1].cpu().numpy() > 0).sum()),
            "live_cells": _live_cells(dims, state[1].cpu().numpy(), min_weight), "triangles": int(tris.shape[0]),
            "degenerate": dropped, "boundary": int(edges.boundary), "non_manifold": int(edges.non_manifold),
            "voxel_diagonal": diag, "recommended_slack": SLACK_DIAGONALS * diag}
    return tris, info


def _live_cells(dims, w, min_weight):
    nx, ny, nz = dims
    if min(dims) < 2:
        return 0
    ok = w.reshape(nz, ny, nx) >= min_weight
    live = np.ones((nz - 1, ny - 1, nx - 1), bool)
    for c in range(8):
        live &= ok[(c >> 2):nz - 1 + (c >> 2), ((c >> 1) & 1):ny - 1 + ((c >> 1) & 1), (c & 1):nx - 1 + (c & 1)]
    return int(live.sum())
