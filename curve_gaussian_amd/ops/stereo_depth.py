"""Depth maps from a scan's own photographs: plane-sweep stereo (cgs_stereo_sweep / cgs_stereo_consistency,
include/curvegs.h; csrc/stereo_depth.hip).  The reference has no counterpart.  For a scan that has photographs and poses and
neither a mesh, a dense cloud nor depth maps: the maps are camera z, 0 where stereo gives nothing, which is what
``ops.edge_occlusion.check_depth_maps`` (``depth_maps=``, ``--depth_dir``) takes -- an entry <= 0 becomes +inf there and
hides nothing, so the gate fails open wherever stereo is unsure.

  luminance        a decoded photograph as the bytes the sweep matches: Y = (299 R + 587 G + 114 B + 500) // 1000
  plan_views       what the HOST decides for a group of same-size views: each view's inverse-depth hypotheses, its source
                   views, the relative poses and the consistency tolerance -- made once, so both back ends read the same bits
  sweep            the winner-take-all sweep of a planned group: float32 [V,H,W]
  consistency      the cross-view filter of a swept group
  stereo_depth     photographs and cameras in, one map per view out
  plan_fusion      the host's decisions for fusing a group's maps: each target's fusion sources, the poses that take a
                   source's camera coordinates INTO the target's, and plan_views' tolerance
  warp, fuse       cgs_stereo_warp / cgs_stereo_fuse on a range of targets of a planned group
  fuse_depth       maps and cameras in, one fused map per view out (``stereo_depth(..., fuse=True)`` chains the two)

The rule is frozen in include/curvegs.h -- float64, one rounded operation at a time, no square root, running sums -- and
stated once for the kernels in csrc/stereo_depth.h and csrc/stereo_fuse.h.  Two back ends: ``"gpu"``, HIP, and ``"host"``,
numpy written operation for operation (numpy evaluates one rounded operation per ufunc call), so the two agree BIT FOR BIT, and so does the brute
force of tests/stereo_cases.py.

WHAT THIS IS NOT.  Fronto-parallel patches on one scale of grey values: no patch-match propagation, no slanted planes, no
colour.  The fusion (OFF BY DEFAULT) works in map space: per pixel the largest cluster of agreeing inverse depths among the
own depth and the sources' warped ones, stored as its mean -- no fused point cloud, no second sweep.  EVERY DEFAULT BELOW
IS UNTUNED: only the drawn solids of scene/solid_scan.py with their value-noise photographs have been checked -- no real
photograph, no lighting change, no specular or textureless surface."""
import math
from typing import NamedTuple

import numpy as np
import torch

from .. import _lib as L
from . import edge_score as ES

MAX_RADIUS = L.STEREO_MAX_RADIUS
STEREO_Z_FLOOR = 0.05       # UNTUNED: the nearest hypothesis of a camera inside the bounds, world units
HYPOTHESES = 64             # UNTUNED
PATCH_RADIUS = 2            # UNTUNED: 5 x 5 taps
SOURCES = 3                 # UNTUNED
MAX_ANGLE_DEG = 60.0        # UNTUNED: a source's optical axis lies within this of the reference's
MIN_VAR = 4.0               # UNTUNED: a patch matches only with a grey-value variance above this (bytes squared)
MAX_COST = 0.5              # UNTUNED: 1 - the signed square of the normalised correlation, averaged over the sources
MIN_SOURCES = 1             # UNTUNED
CONSISTENCY_STEPS = 1.5     # UNTUNED: sources agree within this many hypothesis steps of inverse depth
MIN_CONSISTENT = 2          # UNTUNED
BOUNDS = ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
MAX_FUSE = L.STEREO_MAX_FUSE
FUSE_SOURCES = 7            # UNTUNED: what the numpy prototype of the fusion used
FUSE_SUPPORT = 3            # UNTUNED: likewise; the own depth counts
FUSE_CHUNK_BYTES = 1 << 30  # the warped planes of the targets fused at once stay under this (at least one target)


def luminance(image):
    """uint8 [H,W] of a decoded photograph: an [H,W] array as it is stored, [H,W,3] or [H,W,4] (alpha ignored) through
    Y = (299 R + 587 G + 114 B + 500) // 1000 on the bytes."""
    a = ES._host(image)
    if a.dtype != np.uint8 or a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] not in (3, 4)):
        raise ValueError(f"luminance: a photograph is uint8 [H,W], [H,W,3] or [H,W,4] (got {a.dtype} {a.shape})")
    if a.ndim == 2:
        return np.ascontiguousarray(a)
    c = a.astype(np.uint32)
    return ((299 * c[..., 0] + 587 * c[..., 1] + 114 * c[..., 2] + 500) // 1000).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ the host's decisions
def _check_params(what, hypotheses, patch_radius, sources, min_var, max_cost, min_sources, min_consistent):
    D, R, S = int(hypotheses), int(patch_radius), int(sources)
    if D < 1 or S < 1 or int(min_sources) < 1 or int(min_consistent) < 0:
        raise ValueError(f"{what}: hypotheses, sources and min_sources are at least 1 and min_consistent at least 0 (got {D}, {S}, "
                         f"{min_sources}, {min_consistent})")
    if not 0 <= R <= MAX_RADIUS:
        raise ValueError(f"{what}: the patch radius must lie in [0, {MAX_RADIUS}] (got {R})")
    if not float(min_var) >= 0.0 or math.isnan(float(max_cost)):
        raise ValueError(f"{what}: min_var must be >= 0 and max_cost a number (got {min_var}, {max_cost})")
    return D, R, S, float(min_var), float(max_cost), int(min_sources), int(min_consistent)


def relative_pose(R_ref, T_ref, R_src, T_src):
    """[R | T] (12 doubles, row-major) taking reference-camera coordinates to source-camera coordinates."""
    Rr, Rs = np.asarray(R_ref, np.float64), np.asarray(R_src, np.float64)
    Rel = Rs @ Rr.T
    t = np.asarray(T_src, np.float64) - Rel @ np.asarray(T_ref, np.float64)
    return np.concatenate([Rel, t[:, None]], 1).reshape(12)


def _nearest_views(v, centres, axes, cos_max, count):
    """The ``count`` nearest camera centres among the other views whose optical axes lie within the angle of view v's."""
    d2 = ((centres - centres[v]) ** 2).sum(1)
    cand = [w for w in range(len(centres)) if w != v and float(axes[w] @ axes[v]) >= cos_max]
    return sorted(cand, key=lambda w: d2[w])[:count]   # (sorted is stable: ties stay in index order)


class Plan(NamedTuple):
    """A group of same-size views as the entries take it, and per view the ends of its hypotheses and whether it is swept."""
    K: np.ndarray         # float64 [V,4]
    inv: np.ndarray       # float64 [V,D]
    src: np.ndarray       # int32 [V,S], -1: no source
    rel: np.ndarray       # float64 [V,S,12]
    tol: np.ndarray       # float64 [V]
    z_near: np.ndarray    # float64 [V]
    z_far: np.ndarray     # float64 [V]
    usable: np.ndarray    # bool [V]


def plan_views(cameras, bounds=BOUNDS, hypotheses=HYPOTHESES, sources=SOURCES, max_angle_deg=MAX_ANGLE_DEG,
               consistency_steps=CONSISTENCY_STEPS, min_sources=MIN_SOURCES, min_consistent=MIN_CONSISTENT):
    """The ``Plan`` of same-size ``NovelViewCamera`` s (R, T world -> camera).  SOURCES: the ``sources`` nearest camera centres
    among the other views whose optical axes lie within ``max_angle_deg`` of the view's, ties to the lower index; the rest
    of a row is -1.  A view with fewer than max(min_sources, min_consistent) sources has none: it is not swept.
    HYPOTHESES: ``hypotheses`` inverse depths, uniform from 1 / z_near to 1 / z_far, the least and greatest camera z of the 8
    corners of ``bounds``, z_near floored at ``STEREO_Z_FLOOR``; a view that has the bounds behind it (z_far <= z_near) is not
    swept either.  tol = consistency_steps * |inv[1] - inv[0]| (0 with one hypothesis)."""
    cams = list(cameras)
    V, D, S = len(cams), int(hypotheses), int(sources)
    K = np.array([[c.fx, c.fy, c.cx, c.cy] for c in cams], np.float64).reshape(V, 4)
    Rm = [np.asarray(c.R, np.float64).reshape(3, 3) for c in cams]
    Tm = [np.asarray(c.T, np.float64).reshape(3) for c in cams]
    centres = np.array([-(R.T @ T) for R, T in zip(Rm, Tm)], np.float64).reshape(V, 3)
    axes = np.array([R[2] / np.linalg.norm(R[2]) for R in Rm], np.float64).reshape(V, 3)
    lo, hi = np.asarray(bounds, np.float64).reshape(2, 3)
    corners = np.array([[(lo, hi)[a][0], (lo, hi)[b][1], (lo, hi)[c][2]] for a in (0, 1) for b in (0, 1) for c in (0, 1)])
    cos_max = math.cos(math.radians(float(max_angle_deg)))
    inv, src = np.ones((V, D), np.float64), np.full((V, S), -1, np.int32)
    rel, tol = np.zeros((V, S, 12), np.float64), np.zeros((V,), np.float64)
    z_near, z_far, usable = np.zeros(V), np.zeros(V), np.zeros(V, bool)
    for v in range(V):
        z = corners @ Rm[v][2] + Tm[v][2]
        z_near[v], z_far[v] = max(float(z.min()), STEREO_Z_FLOOR), float(z.max())
        if not z_far[v] > z_near[v]:
            inv[v] = 1.0 / z_near[v]
            continue
        inv[v] = np.linspace(1.0 / z_near[v], 1.0 / z_far[v], D) if D > 1 else 1.0 / z_near[v]
        tol[v] = float(consistency_steps) * abs(inv[v][1] - inv[v][0]) if D > 1 else 0.0
        cand = _nearest_views(v, centres, axes, cos_max, S)
        if len(cand) < max(int(min_sources), int(min_consistent), 1):
            continue
        usable[v] = True
        for s, w in enumerate(cand):
            src[v, s] = w
            rel[v, s] = relative_pose(Rm[v], Tm[v], Rm[w], Tm[w])
    return Plan(K, inv, src, rel, tol, z_near, z_far, usable)


def _check_fuse_params(what, fuse_sources, min_support):
    F, N = int(fuse_sources), int(min_support)
    if not 1 <= F <= MAX_FUSE or N < 1:
        raise ValueError(f"{what}: fuse_sources must lie in [1, {MAX_FUSE}] and min_support be at least 1 (got {F}, {N})")
    return F, N


def plan_fusion(cameras, bounds=BOUNDS, hypotheses=HYPOTHESES, fuse_sources=FUSE_SOURCES, max_angle_deg=MAX_ANGLE_DEG,
                consistency_steps=CONSISTENCY_STEPS):
    """(K [V,4], fsrc int32 [V,F], into [V,F,12], tol [V]) of same-size ``NovelViewCamera`` s, as cgs_stereo_warp and
    cgs_stereo_fuse take them.  fsrc: target v's ``fuse_sources`` nearest camera centres within ``max_angle_deg``, chosen as
    ``plan_views`` chooses (ties to the lower index, -1 pads) -- however few there are.  into[v][s] takes the SOURCE's camera
    coordinates to the TARGET's: ``relative_pose(R_w, T_w, R_v, T_v)``, the other direction than the sweep's ``rel``.  K and tol
    are those of ``plan_views`` for the same bounds, hypotheses and consistency_steps."""
    cams = list(cameras)
    F, _ = _check_fuse_params("plan_fusion", fuse_sources, 1)
    plan = plan_views(cams, bounds, hypotheses, 1, max_angle_deg, consistency_steps, 1, 0)
    V = len(cams)
    Rm = [np.asarray(c.R, np.float64).reshape(3, 3) for c in cams]
    Tm = [np.asarray(c.T, np.float64).reshape(3) for c in cams]
    centres = np.array([-(R.T @ T) for R, T in zip(Rm, Tm)], np.float64).reshape(V, 3)
    axes = np.array([R[2] / np.linalg.norm(R[2]) for R in Rm], np.float64).reshape(V, 3)
    cos_max = math.cos(math.radians(float(max_angle_deg)))
    fsrc, into = np.full((V, F), -1, np.int32), np.zeros((V, F, 12), np.float64)
    for v in range(V):
        for s, w in enumerate(_nearest_views(v, centres, axes, cos_max, F)):
            fsrc[v, s] = w
            into[v, s] = relative_pose(Rm[w], Tm[w], Rm[v], Tm[v])
    return plan.K, fsrc, into, plan.tol


# ------------------------------------------------------------------------------------------------ the host back end
def _sweep_view_host(gray64, K, inv, src, rel, v, R, thr, max_cost, min_sources):
    V, H, W = gray64.shape
    out = np.zeros((H, W), np.float32)
    if H < 2 * R + 1 or W < 2 * R + 1:
        return out
    D, S = inv.shape[1], src.shape[1]
    n = float((2 * R + 1) * (2 * R + 1))
    Hc, Wc = H - 2 * R, W - 2 * R                       # the pixels whose patch lies inside the image
    taps = [(di, dj) for di in range(-R, R + 1) for dj in range(-R, R + 1)]
    ref = gray64[v]
    fx, fy, cx, cy = K[v]
    with np.errstate(all="ignore"):
        r = np.stack([ref[R + di:R + di + Hc, R + dj:R + dj + Wc] for di, dj in taps])
        sr, srr = np.zeros((Hc, Wc)), np.zeros((Hc, Wc))
        for k in range(len(taps)):
            sr = sr + r[k]
            srr = srr + r[k] * r[k]
        var_r = n * srr - sr * sr
        dxs = ((np.arange(W, dtype=np.float64) + 0.5) - cx) / fx
        dys = ((np.arange(H, dtype=np.float64) + 0.5) - cy) / fy
        DX = np.stack([np.broadcast_to(dxs[None, R + dj:R + dj + Wc], (Hc, Wc)) for _, dj in taps])
        DY = np.stack([np.broadcast_to(dys[R + di:R + di + Hc, None], (Hc, Wc)) for di, _ in taps])
        costs = np.full((D, Hc, Wc), np.inf)
        for d in range(D):
            z = np.float64(1.0) / inv[v, d]
            X, Y = DX * z, DY * z
            total, count = np.zeros((Hc, Wc)), np.zeros((Hc, Wc), np.int64)
            for s in range(S):
                w = int(src[v, s])
                if not 0 <= w < V:
                    continue
                M, (fxs, fys, cxs, cys) = rel[v, s], K[w]
                c0 = ((M[0] * X + M[1] * Y) + M[2] * z) + M[3]
                c1 = ((M[4] * X + M[5] * Y) + M[6] * z) + M[7]
                c2 = ((M[8] * X + M[9] * Y) + M[10] * z) + M[11]
                valid = c2 > 0.0
                x = (fxs * (c0 / c2) + cxs) - 0.5
                y = (fys * (c1 / c2) + cys) - 0.5
                x0, y0 = np.floor(x), np.floor(y)
                valid &= (x0 >= 0.0) & (x0 + 1.0 <= float(W - 1)) & (y0 >= 0.0) & (y0 + 1.0 <= float(H - 1))
                a, b = x - x0, y - y0
                xi, yi = np.where(valid, x0, 0.0).astype(np.int64), np.where(valid, y0, 0.0).astype(np.int64)
                if W > 1 and H > 1:
                    img = gray64[w]
                    g00, g01, g10, g11 = img[yi, xi], img[yi, xi + 1], img[yi + 1, xi], img[yi + 1, xi + 1]
                else:                                       # (no footprint fits: every tap is invalid)
                    g00 = g01 = g10 = g11 = np.zeros_like(x)
                top = g00 * (1.0 - a) + g01 * a
                bot = g10 * (1.0 - a) + g11 * a
                val = top * (1.0 - b) + bot * b
                ss, sss, srs = np.zeros((Hc, Wc)), np.zeros((Hc, Wc)), np.zeros((Hc, Wc))
                for k in range(len(taps)):
                    ss = ss + val[k]
                    sss = sss + val[k] * val[k]
                    srs = srs + r[k] * val[k]
                var_s = n * sss - ss * ss
                counts = valid.all(0) & (var_s > thr)
                cov = n * srs - sr * ss
                cs = 1.0 - (cov * np.abs(cov)) / (var_r * var_s)
                total = np.where(counts, total + cs, total)
                count += counts
            costs[d] = np.where(count >= min_sources, total / count, np.inf)
        best = np.argmin(costs, 0)                           # the first of equal minima: the lowest d
        pick = lambda idx: np.take_along_axis(costs, idx[None], 0)[0]
        cb = pick(best)
        keep = (var_r > thr) & np.isfinite(cb) & (cb <= max_cost)
        lo_i, hi_i = np.maximum(best - 1, 0), np.minimum(best + 1, D - 1)
        cm, cp = pick(lo_i), pick(hi_i)
        den = (cm - 2.0 * cb) + cp
        refine = (best > 0) & (best < D - 1) & np.isfinite(cm) & np.isfinite(cp) & (den > 0.0)
        o = np.where(refine, np.minimum(np.maximum((0.5 * (cm - cp)) / den, -0.5), 0.5), 0.0)
        iv = inv[v]
        step = np.where(o >= 0.0, iv[hi_i] - iv[best], iv[best] - iv[lo_i])
        q = np.where(o != 0.0, iv[best] + o * step, iv[best])
        z_out = (1.0 / q).astype(np.float32)
    out[R:R + Hc, R:R + Wc] = np.where(keep, z_out, np.float32(0.0))
    return out


def _consistency_view_host(depth, K, src, rel, tol, v, min_consistent):
    V, H, W = depth.shape
    zf = depth[v]
    with np.errstate(all="ignore"):
        z = zf.astype(np.float64)
        has = z > 0.0
        fx, fy, cx, cy = K[v]
        X = (((np.arange(W, dtype=np.float64) + 0.5) - cx) / fx)[None, :] * z
        Y = (((np.arange(H, dtype=np.float64) + 0.5) - cy) / fy)[:, None] * z
        agree = np.zeros((H, W), np.int64)
        for s in range(src.shape[1]):
            w = int(src[v, s])
            if not 0 <= w < V:
                continue
            M, (fxs, fys, cxs, cys) = rel[v, s], K[w]
            c0 = ((M[0] * X + M[1] * Y) + M[2] * z) + M[3]
            c1 = ((M[4] * X + M[5] * Y) + M[6] * z) + M[7]
            c2 = ((M[8] * X + M[9] * Y) + M[10] * z) + M[11]
            u = fxs * (c0 / c2) + cxs
            vv = fys * (c1 / c2) + cys
            ok = has & ~(c2 <= 0.0) & (u >= 0.0) & (u < float(W)) & (vv >= 0.0) & (vv < float(H))
            ui, vi = np.where(ok, np.floor(u), 0.0).astype(np.int64), np.where(ok, np.floor(vv), 0.0).astype(np.int64)
            ds = depth[w][vi, ui].astype(np.float64)
            ok &= ds > 0.0
            ok &= np.abs(1.0 / ds - 1.0 / c2) <= tol[v]
            agree += ok
    return np.where(has & (agree >= min_consistent), zf, np.float32(0.0)).astype(np.float32)


# ------------------------------------------------------------------------------------------------ the two entries
def _as_group(what, gray, K, src, rel):
    g = gray if torch.is_tensor(gray) else torch.from_numpy(np.ascontiguousarray(gray))
    if g.dtype != torch.uint8 or g.dim() != 3:
        raise ValueError(f"{what}: gray must be uint8 [V,H,W] (got {g.dtype} {tuple(g.shape)})")
    V = int(g.shape[0])
    K = np.ascontiguousarray(np.asarray(K, np.float64).reshape(-1, 4))
    src = np.ascontiguousarray(np.asarray(src, np.int32))
    if K.shape != (V, 4) or src.ndim != 2 or src.shape[0] != V or src.shape[1] < 1:
        raise ValueError(f"{what}: intrinsics must be [{V},4] and src int32 [{V},S], S >= 1 (got {K.shape}, {src.shape})")
    rel = np.ascontiguousarray(np.asarray(rel, np.float64).reshape(V, src.shape[1], 12))
    return g.detach().contiguous(), V, K, src, rel


def sweep(gray, intrinsics, inv, src, rel, patch_radius=PATCH_RADIUS, min_var=MIN_VAR, max_cost=MAX_COST,
          min_sources=MIN_SOURCES, backend="gpu", device=None):
    """cgs_stereo_sweep on a group: gray uint8 [V,H,W], intrinsics [V,4], inv [V,D], src int32 [V,S], rel [V,S,12] -> float32
    [V,H,W], camera z, 0 where there is none.  ``"gpu"``: on the device, the result stays there; ``"host"``: numpy, a CPU
    tensor, the same bits."""
    ES._check_backend(backend)
    g, V, K, src, rel = _as_group("stereo sweep", gray, intrinsics, src, rel)
    inv = np.ascontiguousarray(np.asarray(inv, np.float64))
    if inv.ndim != 2 or inv.shape[0] != V:
        raise ValueError(f"stereo sweep: inv must be [{V},D] (got {inv.shape})")
    D, R, S, min_var, max_cost, min_sources, _ = _check_params("stereo sweep", inv.shape[1], patch_radius, src.shape[1],
                                                               min_var, max_cost, min_sources, 0)
    H, W = ES._check_size("stereo sweep", g.shape[1], g.shape[2])
    if backend == "host":
        n = float((2 * R + 1) * (2 * R + 1))
        g64 = g.cpu().numpy().astype(np.float64)
        out = np.zeros((V, H, W), np.float32)
        for v in range(V):
            out[v] = _sweep_view_host(g64, K, inv, src, rel, v, R, (min_var * n) * n, max_cost, min_sources)
        return torch.from_numpy(out)
    dev = ES._device_for([g], "stereo sweep", device)
    with L.device_guard(dev):
        g = g.to(dev)
        out = torch.empty((V, H, W), dtype=torch.float32, device=dev)
        if V > 0:
            Kd, invd, srcd, reld = (torch.from_numpy(a).to(dev) for a in (K, inv, src, rel))
            rc = L.load().cgs_stereo_sweep(V, H, W, L.ptr(g), L.ptr(Kd), D, L.ptr(invd), S, L.ptr(srcd), L.ptr(reld), R, min_var,
                                           max_cost, min_sources, L.ptr(out), L.raw_stream(dev))
            L.check(rc, "cgs_stereo_sweep")
    return out


def consistency(depth, intrinsics, src, rel, tol, min_consistent=MIN_CONSISTENT, backend="gpu", device=None):
    """cgs_stereo_consistency on a swept group: depth float32 [V,H,W] -> a new float32 [V,H,W] in which a pixel keeps its bits
    when at least ``min_consistent`` of its sources hold, where it lands in them, an inverse depth within tol[v] of its own,
    and is 0 otherwise."""
    ES._check_backend(backend)
    d = depth if torch.is_tensor(depth) else torch.from_numpy(np.ascontiguousarray(depth))
    if d.dtype != torch.float32 or d.dim() != 3:
        raise ValueError(f"stereo consistency: depth must be float32 [V,H,W] (got {d.dtype} {tuple(d.shape)})")
    d = d.detach().contiguous()
    V = int(d.shape[0])
    K = np.ascontiguousarray(np.asarray(intrinsics, np.float64).reshape(-1, 4))
    src = np.ascontiguousarray(np.asarray(src, np.int32))
    tol = np.ascontiguousarray(np.asarray(tol, np.float64).reshape(-1))
    if K.shape != (V, 4) or src.ndim != 2 or src.shape[0] != V or src.shape[1] < 1 or tol.shape != (V,):
        raise ValueError(f"stereo consistency: intrinsics [{V},4], src int32 [{V},S] with S >= 1 and tol [{V}] (got {K.shape}, "
                         f"{src.shape}, {tol.shape})")
    rel = np.ascontiguousarray(np.asarray(rel, np.float64).reshape(V, src.shape[1], 12))
    min_consistent = int(min_consistent)
    if min_consistent < 0:
        raise ValueError(f"stereo consistency: min_consistent must be >= 0 (got {min_consistent})")
    H, W = ES._check_size("stereo consistency", d.shape[1], d.shape[2])
    if backend == "host":
        a = d.cpu().numpy()
        out = np.zeros((V, H, W), np.float32)
        for v in range(V):
            out[v] = _consistency_view_host(a, K, src, rel, tol, v, min_consistent)
        return torch.from_numpy(out)
    dev = ES._device_for([d], "stereo consistency", device)
    with L.device_guard(dev):
        d = d.to(dev)
        out = torch.empty((V, H, W), dtype=torch.float32, device=dev)
        if V > 0:
            Kd, srcd, reld, told = (torch.from_numpy(a).to(dev) for a in (K, src, rel, tol))
            rc = L.load().cgs_stereo_consistency(V, H, W, L.ptr(d), L.ptr(Kd), int(src.shape[1]), L.ptr(srcd), L.ptr(reld),
                                                 L.ptr(told), min_consistent, L.ptr(out), L.raw_stream(dev))
            L.check(rc, "cgs_stereo_consistency")
    return out


# ------------------------------------------------------------------------------------------------ fusion: the host back end
def _is_depth(a):
    """A positive finite float32: what the fusion takes for a depth."""
    with np.errstate(invalid="ignore"):
        return (a > 0.0) & np.isfinite(a)


def _warp_slot_host(src_map, Kw, Kv, M, plane):
    """One source's map into one slot's plane (float32 [H,W], +inf where nothing has landed), in place."""
    H, W = src_map.shape
    with np.errstate(all="ignore"):
        ok = _is_depth(src_map)
        z = src_map.astype(np.float64)
        X = (((np.arange(W, dtype=np.float64) + 0.5) - Kw[2]) / Kw[0])[None, :] * z
        Y = (((np.arange(H, dtype=np.float64) + 0.5) - Kw[3]) / Kw[1])[:, None] * z
        c0 = ((M[0] * X + M[1] * Y) + M[2] * z) + M[3]
        c1 = ((M[4] * X + M[5] * Y) + M[6] * z) + M[7]
        c2 = ((M[8] * X + M[9] * Y) + M[10] * z) + M[11]
        u = Kv[0] * (c0 / c2) + Kv[2]
        vv = Kv[1] * (c1 / c2) + Kv[3]
        ok &= ~(c2 <= 0.0) & (u >= 0.0) & (u < float(W)) & (vv >= 0.0) & (vv < float(H))
        zf = c2.astype(np.float32)
        ok &= _is_depth(zf)
        at = np.floor(vv[ok]).astype(np.int64) * W + np.floor(u[ok]).astype(np.int64)
    np.minimum.at(plane.reshape(-1), at, zf[ok])   # (positive floats order as their bit patterns do)


def _fuse_view_host(own, warped, tol, min_support):
    """(out float32 [H,W], support uint8 [H,W]) of one target: own [H,W], warped [F,H,W]."""
    F = warped.shape[0]
    with np.errstate(all="ignore"):
        vals = np.concatenate([own[None], warped], 0)
        q = np.where(_is_depth(vals), 1.0 / vals.astype(np.float64), np.nan)    # an absent candidate fails every comparison
        sb, qb = np.full(own.shape, -1, np.int64), np.full(own.shape, np.nan)
        for k in range(F + 1):
            cnt = np.zeros(own.shape, np.int64)
            for m in range(F + 1):
                cnt += np.abs(q[m] - q[k]) <= tol
            better = ~np.isnan(q[k]) & ((cnt > sb) | ((cnt == sb) & (q[k] < qb)))
            sb, qb = np.where(better, cnt, sb), np.where(better, q[k], qb)
        total, count = np.zeros(own.shape), np.zeros(own.shape, np.int64)
        for m in range(F + 1):
            member = np.abs(q[m] - qb) <= tol
            total = np.where(member, total + q[m], total)
            count += member
        keep = sb >= min_support
        out = np.where(keep, (1.0 / (total / count)).astype(np.float32), np.float32(0.0)).astype(np.float32)
    return out, np.where(keep, count, 0).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ fusion: the two entries
def _as_maps(what, depth):
    d = depth if torch.is_tensor(depth) else torch.from_numpy(np.ascontiguousarray(depth))
    if d.dtype != torch.float32 or d.dim() != 3:
        raise ValueError(f"{what}: depth must be float32 [V,H,W] (got {d.dtype} {tuple(d.shape)})")
    return d.detach().contiguous()


def _check_range(what, V, v0, nv):
    v0, nv = int(v0), int(nv)
    if not (0 <= v0 <= V and 0 <= nv <= V - v0):
        raise ValueError(f"{what}: the targets v0 .. v0 + nv must lie in [0, {V}] (got v0={v0}, nv={nv})")
    return v0, nv


def warp(depth, intrinsics, fsrc, into, v0=0, nv=None, backend="gpu", device=None):
    """cgs_stereo_warp on the targets v0 .. v0 + nv - 1 (all from v0 on when ``nv`` is None) of a group: depth float32
    [V,H,W], intrinsics [V,4], fsrc int32 [V,F], into [V,F,12] (``plan_fusion``) -> float32 [nv,F,H,W]: per slot the source's
    depths where they land in the target, the nearest of those that share a pixel, +inf where none lands."""
    ES._check_backend(backend)
    d = _as_maps("stereo warp", depth)
    V = int(d.shape[0])
    K = np.ascontiguousarray(np.asarray(intrinsics, np.float64).reshape(-1, 4))
    fsrc = np.ascontiguousarray(np.asarray(fsrc, np.int32))
    if K.shape != (V, 4) or fsrc.ndim != 2 or fsrc.shape[0] != V or not 1 <= fsrc.shape[1] <= MAX_FUSE:
        raise ValueError(f"stereo warp: intrinsics must be [{V},4] and fsrc int32 [{V},F], 1 <= F <= {MAX_FUSE} (got {K.shape}, "
                         f"{fsrc.shape})")
    F = int(fsrc.shape[1])
    into = np.ascontiguousarray(np.asarray(into, np.float64).reshape(V, F, 12))
    v0, nv = _check_range("stereo warp", V, v0, V - int(v0) if nv is None else nv)
    H, W = ES._check_size("stereo warp", d.shape[1], d.shape[2])
    if backend == "host":
        a = d.cpu().numpy()
        out = np.full((nv, F, H, W), np.inf, np.float32)
        for t in range(nv):
            for s in range(F):
                w = int(fsrc[v0 + t, s])
                if 0 <= w < V:
                    _warp_slot_host(a[w], K[w], K[v0 + t], into[v0 + t, s], out[t, s])
        return torch.from_numpy(out)
    dev = ES._device_for([d], "stereo warp", device)
    with L.device_guard(dev):
        d = d.to(dev)
        out = torch.empty((nv, F, H, W), dtype=torch.float32, device=dev)
        if nv > 0:
            Kd, srcd, intod = (torch.from_numpy(a).to(dev) for a in (K, fsrc, into))
            rc = L.load().cgs_stereo_warp(V, H, W, L.ptr(d), L.ptr(Kd), F, L.ptr(srcd), L.ptr(intod), v0, nv, L.ptr(out),
                                          L.raw_stream(dev))
            L.check(rc, "cgs_stereo_warp")
    return out


def fuse(depth, warped, tol, min_support=FUSE_SUPPORT, v0=0, backend="gpu", device=None, return_support=False):
    """cgs_stereo_fuse on the targets v0 .. v0 + nv - 1 of a group: depth float32 [V,H,W], warped float32 [nv,F,H,W]
    (``warp`` of the same range), tol [V] -> float32 [nv,H,W]: per pixel the mean inverse depth of the largest cluster among
    the own depth and the warped ones, as a depth; 0 where the cluster has fewer than ``min_support`` members.
    ``return_support``: also uint8 [nv,H,W], the cluster's size (0 where the map is 0)."""
    ES._check_backend(backend)
    d = _as_maps("stereo fuse", depth)
    w = warped if torch.is_tensor(warped) else torch.from_numpy(np.ascontiguousarray(warped))
    V = int(d.shape[0])
    if w.dtype != torch.float32 or w.dim() != 4 or tuple(w.shape[2:]) != tuple(d.shape[1:]) or not 1 <= w.shape[1] <= MAX_FUSE:
        raise ValueError(f"stereo fuse: warped must be float32 [nv,F,{d.shape[1]},{d.shape[2]}], 1 <= F <= {MAX_FUSE} (got "
                         f"{w.dtype} {tuple(w.shape)})")
    w = w.detach().contiguous()
    F, min_support = _check_fuse_params("stereo fuse", w.shape[1], min_support)
    tol = np.ascontiguousarray(np.asarray(tol, np.float64).reshape(-1))
    if tol.shape != (V,):
        raise ValueError(f"stereo fuse: tol must be [{V}] (got {tol.shape})")
    v0, nv = _check_range("stereo fuse", V, v0, w.shape[0])
    H, W = ES._check_size("stereo fuse", d.shape[1], d.shape[2])
    if backend == "host":
        a, b = d.cpu().numpy(), w.cpu().numpy()
        out, sup = np.zeros((nv, H, W), np.float32), np.zeros((nv, H, W), np.uint8)
        for t in range(nv):
            out[t], sup[t] = _fuse_view_host(a[v0 + t], b[t], tol[v0 + t], min_support)
        return (torch.from_numpy(out), torch.from_numpy(sup)) if return_support else torch.from_numpy(out)
    dev = ES._device_for([d, w], "stereo fuse", device)
    with L.device_guard(dev):
        d, w = d.to(dev), w.to(dev)
        out = torch.empty((nv, H, W), dtype=torch.float32, device=dev)
        sup = torch.empty((nv, H, W), dtype=torch.uint8, device=dev) if return_support else None
        if nv > 0:
            told = torch.from_numpy(tol).to(dev)
            rc = L.load().cgs_stereo_fuse(V, H, W, L.ptr(d), F, L.ptr(w), L.ptr(told), min_support, v0, nv, L.ptr(out),
                                          L.ptr(sup) if return_support else None, L.raw_stream(dev))
            L.check(rc, "cgs_stereo_fuse")
    return (out, sup) if return_support else out


def fuse_depth(maps, cameras, bounds=BOUNDS, hypotheses=HYPOTHESES, max_angle_deg=MAX_ANGLE_DEG,
               consistency_steps=CONSISTENCY_STEPS, fuse_sources=FUSE_SOURCES, min_support=FUSE_SUPPORT, backend="gpu",
               device=None, return_info=False):
    """One fused float32 [H,W] numpy map of camera z per camera, 0 where there is none.  maps: one float [H,W] array per
    camera, of its camera's size, in which only a positive finite entry is a depth (``stereo_depth``'s maps, or the
    caller's own).  Views are grouped by size as ``stereo_depth`` groups them, a group is planned by ``plan_fusion`` and its
    targets are walked in chunks whose warped planes stay under ``FUSE_CHUNK_BYTES``; the result does not depend on the
    chunks.  A pixel's cluster counts its own depth, so a view without sources keeps nothing at ``min_support`` > 1.
    OFF BY DEFAULT in ``stereo_depth``; ``fuse_sources`` and ``min_support`` are UNTUNED.

    ``return_info``: also a dict with "coverage_before" and "coverage" (per view, the share of pixels that hold a depth
    before and after), "support_histogram" (entry n: the pixels whose cluster has n members, n = 0 .. fuse_sources + 1),
    "filled" (pixels without a depth that got one) and "dropped" (pixels that lost theirs)."""
    ES._check_backend(backend)
    cams, own = list(cameras), [ES._host(m) for m in maps]
    if len(cams) != len(own):
        raise ValueError(f"fuse_depth: {len(cams)} cameras and {len(own)} depth maps")
    F, min_support = _check_fuse_params("fuse_depth", fuse_sources, min_support)
    for c, m in zip(cams, own):
        if m.dtype.kind != "f" or m.shape != (c.height, c.width):
            raise ValueError(f"fuse_depth: the depth map of {c.name} must be a float [{c.height},{c.width}] array "
                             f"(got {m.dtype} {m.shape})")
    groups = {}
    for v, c in enumerate(cams):
        groups.setdefault((int(c.height), int(c.width)), []).append(v)
    fused, hist = [None] * len(cams), np.zeros(F + 2, np.int64)
    for (H, W), idx in groups.items():
        K, fsrc, into, tol = plan_fusion([cams[v] for v in idx], bounds, hypotheses, F, max_angle_deg, consistency_steps)
        depth = torch.from_numpy(np.stack([own[v].astype(np.float32) for v in idx]))
        if backend == "gpu":
            depth = depth.to(ES._device_for([depth], "fuse_depth", device))
        step = max(1, int(FUSE_CHUNK_BYTES) // (F * H * W * 4))
        for v0 in range(0, len(idx), step):
            nv = min(step, len(idx) - v0)
            warped = warp(depth, K, fsrc, into, v0, nv, backend, device)
            out, sup = fuse(depth, warped, tol, min_support, v0, backend, device, return_support=True)
            out, sup = out.cpu().numpy(), sup.cpu().numpy()
            hist += np.bincount(sup.reshape(-1), minlength=F + 2)[:F + 2]
            for k in range(nv):
                fused[idx[v0 + k]] = out[k]
    if not return_info:
        return fused
    had = [_is_depth(m.astype(np.float32)) for m in own]
    return fused, {"coverage_before": [float(h.mean()) for h in had], "coverage": [float((m > 0).mean()) for m in fused],
                   "support_histogram": [int(n) for n in hist],
                   "filled": int(sum((~h & (m > 0)).sum() for h, m in zip(had, fused))),
                   "dropped": int(sum((h & ~(m > 0)).sum() for h, m in zip(had, fused)))}


# ------------------------------------------------------------------------------------------------ photographs in, maps out
def stereo_depth(gray_u8, cameras, bounds=BOUNDS, hypotheses=HYPOTHESES, patch_radius=PATCH_RADIUS, sources=SOURCES,
                 max_angle_deg=MAX_ANGLE_DEG, min_var=MIN_VAR, max_cost=MAX_COST, min_sources=MIN_SOURCES,
                 consistency_steps=CONSISTENCY_STEPS, min_consistent=MIN_CONSISTENT, backend="gpu", device=None,
                 return_info=False, fuse=False, fuse_sources=FUSE_SOURCES, min_support=FUSE_SUPPORT):
    """One float32 [H,W] numpy map of camera z per camera, 0 where there is none.  gray_u8: one uint8 [H,W] luminance image
    per camera (``luminance``), each of its camera's size; cameras: ``NovelViewCamera`` s.  Views are grouped by size and a
    group is planned by ``plan_views`` (sources are views of the same size), swept and filtered; a view that is not swept
    gets an all-zero map.  ``min_consistent=0`` keeps every swept depth.  A group's photographs and maps are resident at
    once (5 bytes a pixel).  EVERY DEFAULT IS UNTUNED.

    ``return_info``: also a dict with "coverage" (per view, the share of pixels given a depth), "swept" (per view),
    "depth_step_max" -- the largest z^2 * |inv[1] - inv[0]| over the swept views at their far ends, what one hypothesis step
    is in depth -- and "recommended_slack" = 2 * depth_step_max: the gate's default slack (0.001) is far below what stereo
    resolves, so a gate fed these maps wants this slack instead.

    ``fuse`` (OFF BY DEFAULT): the filtered maps go through ``fuse_depth`` with ``fuse_sources`` and ``min_support`` (both
    UNTUNED) before they are returned; "coverage" is then the fused maps' and "fusion" holds ``fuse_depth``'s dict.
    "recommended_slack" is what it is without."""
    ES._check_backend(backend)
    cams, imgs = list(cameras), [ES._host(g) for g in gray_u8]
    if len(cams) != len(imgs):
        raise ValueError(f"stereo_depth: {len(cams)} cameras and {len(imgs)} photographs")
    D, R, S, min_var, max_cost, min_sources, min_consistent = _check_params(
        "stereo_depth", hypotheses, patch_radius, sources, min_var, max_cost, min_sources, min_consistent)
    if fuse:
        _check_fuse_params("stereo_depth", fuse_sources, min_support)
    for c, g in zip(cams, imgs):
        if g.dtype != np.uint8 or g.shape != (c.height, c.width):
            raise ValueError(f"stereo_depth: the photograph of {c.name} must be uint8 [{c.height},{c.width}] "
                             f"(got {g.dtype} {g.shape})")
    groups = {}
    for v, c in enumerate(cams):
        groups.setdefault((int(c.height), int(c.width)), []).append(v)
    maps, swept, step_max = [None] * len(cams), np.zeros(len(cams), bool), 0.0
    for (H, W), idx in groups.items():
        plan = plan_views([cams[v] for v in idx], bounds, D, S, max_angle_deg, consistency_steps, min_sources, min_consistent)
        gray = np.stack([imgs[v] for v in idx])
        if plan.usable.any():
            z = sweep(gray, plan.K, plan.inv, plan.src, plan.rel, R, min_var, max_cost, min_sources, backend, device)
            if min_consistent > 0:
                z = consistency(z, plan.K, plan.src, plan.rel, plan.tol, min_consistent, backend, device)
            z = z.cpu().numpy()
        else:
            z = np.zeros((len(idx), H, W), np.float32)
        for k, v in enumerate(idx):
            maps[v], swept[v] = z[k], bool(plan.usable[k])
            if plan.usable[k] and D > 1:
                step_max = max(step_max, float(plan.z_far[k] ** 2 * abs(plan.inv[k][1] - plan.inv[k][0])))
    fusion = None
    if fuse:
        maps, fusion = fuse_depth(maps, cams, bounds, D, max_angle_deg, consistency_steps, fuse_sources, min_support, backend,
                                  device, return_info=True)
    if not return_info:
        return maps
    info = {"coverage": [float((m > 0).mean()) for m in maps], "swept": [bool(s) for s in swept],
            "depth_step_max": step_max, "recommended_slack": 2.0 * step_max}
    if fuse:
        info["fusion"] = fusion
    return maps, info
