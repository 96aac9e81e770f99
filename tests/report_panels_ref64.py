"""numpy restatements of the training report's image panels (include/curvegs.h, cgs_report_panels; reference
train.py:346-364 followed by tensorboard's summary.image quantiser), the yardsticks of csrc/report.hip and
curve_gaussian_amd.evaluation.report_panels:

``panels32``  float32, the same operations in the same order as the kernel: the render, ground-truth and alpha panels (one
              clamp, one multiply) must be bit-equal to it.
``panels64``  float64, which also returns the values just before quantisation -- the colour-map coordinate ``t * 256`` of
              the depth panel and ``(n * 0.5 + 0.5) * 255`` of the direction panel.  ``compare`` holds a panel to it
              everywhere except at pixels whose float64 value lies within EXEMPT of a quantisation step without being on it,
              where the neighbouring level / table entry is accepted too.

EXEMPT = 1e-3 is derived, not measured: a divide, a square root and two multiplies in float32 on values <= 256 stay below
about 2e-4 absolute (each correctly rounded operation adds at most 2^-24 relative, 256 * 4 * 2^-24 = 6e-5, and the three
squares under the root as much again)."""
import os
import re

import numpy as np

PANELS = ("render", "ground_truth", "depth", "rend_dir", "rend_alpha")
EXEMPT = 1e-3
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "curve_gaussian_amd", "csrc",
                      "turbo_table.h")


def turbo_table():
    """The committed colour map, float64 [256,3], parsed from csrc/turbo_table.h."""
    src = re.sub(r"//[^\n]*", "", open(HEADER).read())
    body = src[src.index("cgs_turbo_table"):]
    rows = re.findall(r"\{\s*([0-9.eE+-]+)\s*,\s*([0-9.eE+-]+)\s*,\s*([0-9.eE+-]+)\s*\}", body)
    return np.array([[float(a) for a in r] for r in rows], np.float64)


def q(x):
    """uint8(clip(x * 255, 0, 255)), truncated, NaN -> 0, in the precision of x."""
    x = np.asarray(x)
    with np.errstate(invalid="ignore"):
        y = x * x.dtype.type(255)
        y = np.where(y > 0, y, x.dtype.type(0))        # NaN -> 0
        y = np.where(y < 255, y, x.dtype.type(255))
    return y.astype(np.uint8)


def turbo8():
    """The table as the kernel quantises it: float32 entries through q."""
    return q(turbo_table().astype(np.float32))


def _clamp01(x):
    with np.errstate(invalid="ignore"):
        return np.where(x < 0, x.dtype.type(0), np.where(x > 1, x.dtype.type(1), x))     # NaN stays NaN


def _grey(plane):
    return np.repeat(q(_clamp01(plane))[..., None], 3, -1)


def _depth_index(depth, ft):
    """-> (table index [H,W], black mask [H,W], s = depth / max * 256 in precision ft)."""
    d = depth[0].astype(ft)
    finite = d[~np.isnan(d)]
    m = ft(max(0.0, float(finite.max()))) if finite.size else ft(0)
    with np.errstate(invalid="ignore", divide="ignore"):
        s = d / m * ft(256)
        idx = np.where(s >= 255, 255, np.where(s > 0, np.trunc(np.where(np.isfinite(s), s, 0)), 0)).astype(np.int64)
    black = np.isnan(s) | ~(m > 0)
    return idx, black, s


def _dir_values(rend_dir, ft):
    """-> n * 0.5 + 0.5 [3,H,W] in precision ft (F.normalize(dim=0): v / max(|v|, 1e-12))."""
    v = rend_dir.astype(ft)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        length = np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
        den = np.where(length < ft(1e-12), ft(1e-12), length)                            # a NaN length stays NaN
        return v / den * ft(0.5) + ft(0.5)


def _panels(render, gt, depth, rend_dir, rend_alpha, ft):
    H, W = next(a for a in (render, gt, depth, rend_dir, rend_alpha) if a is not None).shape[1:]
    out = np.zeros((5, H, W, 3), np.uint8)
    pre = {}
    if render is not None:
        out[0] = _grey(render[0].astype(ft))
    if gt is not None:
        g = gt.astype(ft)
        out[1] = np.stack([q(_clamp01(g[c])) for c in range(3)], -1) if g.shape[0] == 3 else _grey(g[0])
    if depth is not None:
        idx, black, s = _depth_index(depth, ft)
        out[2] = np.where(black[..., None], np.uint8(0), turbo8()[idx])
        pre["depth"] = s
    if rend_dir is not None:
        n = _dir_values(rend_dir, ft)
        out[3] = np.moveaxis(q(n), 0, -1)
        with np.errstate(invalid="ignore"):
            pre["rend_dir"] = n * ft(255)
    if rend_alpha is not None:
        out[4] = _grey(rend_alpha[0].astype(ft))
    written = tuple(a is not None for a in (render, gt, depth, rend_dir, rend_alpha))
    return out, written, pre


def panels32(render=None, gt=None, depth=None, rend_dir=None, rend_alpha=None):
    """float32 numpy arrays (or None) -> (uint8 [5,H,W,3], written 5-tuple); unwritten panels are zero."""
    out, written, _ = _panels(render, gt, depth, rend_dir, rend_alpha, np.float32)
    return out, written


def panels64(render=None, gt=None, depth=None, rend_dir=None, rend_alpha=None):
    """-> (uint8 [5,H,W,3], written, {"depth": t * 256 [H,W], "rend_dir": (n * 0.5 + 0.5) * 255 [3,H,W]}) in float64."""
    return _panels(render, gt, depth, rend_dir, rend_alpha, np.float64)


def _exempt(x):
    with np.errstate(invalid="ignore"):
        r = np.abs(x - np.round(x))
        return (r > 0) & (r < EXEMPT)


def compare(kind, got, ref, pre):
    """Holds panel `kind` ("depth" or "rend_dir"), uint8 [H,W,3], to the float64 restatement `ref` with its
    pre-quantisation values `pre`.  -> (wrong, exempt share): the number of pixels that are neither equal to `ref` nor an
    exempt pixel on the neighbouring level, and the share of exempt pixels (of exempt channel values for rend_dir)."""
    got, ref = np.asarray(got), np.asarray(ref)
    ex = _exempt(pre)
    with np.errstate(invalid="ignore"):
        up = pre < np.round(pre)             # just below a step: the neighbour is the level above
    if kind == "depth":
        idx = np.where(pre >= 255, 255, np.where(pre > 0, np.trunc(np.where(np.isfinite(pre), pre, 0)), 0)).astype(np.int64)
        alt = turbo8()[np.clip(np.where(up, idx + 1, idx - 1), 0, 255)]
        ok = (got == ref).all(-1) | (ex & (got == alt).all(-1))
    elif kind == "rend_dir":
        ex, up = np.moveaxis(ex, 0, -1), np.moveaxis(up, 0, -1)
        alt = np.clip(ref.astype(np.int64) + np.where(up, 1, -1), 0, 255)
        ok = ((got == ref) | (ex & (got == alt))).all(-1)
    else:
        raise ValueError(kind)
    return int((~ok).sum()), float(ex.mean())


def synthetic_view(seed, H, W, gt_channels=3):
    """Random maps of one view, float32, 60 % of the pixels exactly zero in every map (a render of thin curves is mostly
    background): render / gt / alpha in [-0.3, 1.4), depth in [0, 6), directions of any length with a few exactly
    axis-aligned ones.  -> dict(render, gt, depth, rend_dir, rend_alpha)."""
    g = np.random.default_rng(seed)

    def sparse(shape, lo, hi):
        a = (lo + (hi - lo) * g.random(shape)).astype(np.float32)
        a[..., g.random(shape[-2:]) < 0.6] = 0
        return a

    v = {"render": sparse((1, H, W), -0.3, 1.4), "gt": sparse((gt_channels, H, W), -0.3, 1.4),
         "depth": sparse((1, H, W), 0.0, 6.0), "rend_alpha": sparse((1, H, W), -0.3, 1.4)}
    d = (g.standard_normal((3, H, W)) * np.exp(g.uniform(-3, 3, (1, H, W)))).astype(np.float32)
    d[:, g.random((H, W)) < 0.6] = 0
    flat = d.reshape(3, -1)
    for k in range(min(6, flat.shape[1])):           # +-x, +-y, +-z where the view has room for them
        flat[:, k] = 0
        flat[k % 3, k] = 2.5 if k < 3 else -0.75
    v["rend_dir"] = d
    return v
