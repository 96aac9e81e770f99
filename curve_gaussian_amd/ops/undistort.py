"""Undistortion of the edge maps of a COLMAP scan (cgs_undistort_images, include/curvegs.h; csrc/undistort.hip).

The reference reads undistorted scans only; a scan straight out of COLMAP has a lens model -- SIMPLE_RADIAL
by default -- and a principal point that is not the image centre, while the rasterizer projects with a centred pinhole
camera.  ``undistort_images`` resamples every edge map into that camera: each of its pixels is pushed forward through the
lens model (COLMAP's published camera models, restated) and the detected map is sampled there with bilinear weights.

Two back ends with one per-pixel rule: ``"gpu"``, one HIP launch per ``_lib.UNDISTORT_MAX_VIEWS`` views, and ``"host"``, a
float64 numpy restatement -- the back end for a machine without a GPU, and what the tests hold the kernel against.  The
oracle is that restatement of COLMAP's formulas, not COLMAP itself."""
import ctypes as C

import numpy as np
import torch

from .. import _lib as L

UNDISTORT_BACKENDS = ("gpu", "host")

# the camera models the kernel knows: name -> COLMAP model id; parameters: the focal length(s), cx, cy, then the coefficients
SUPPORTED_MODELS = {"SIMPLE_PINHOLE": 0, "PINHOLE": 1, "SIMPLE_RADIAL": 2, "RADIAL": 3, "OPENCV": 4, "FULL_OPENCV": 6}
_ONE_FOCAL = ("SIMPLE_PINHOLE", "SIMPLE_RADIAL", "RADIAL")


def _check_backend(backend):
    if backend not in UNDISTORT_BACKENDS:
        raise ValueError(f"unknown undistort backend {backend!r}: expected one of {UNDISTORT_BACKENDS}")


def distortion_of(intr, loaded_w, loaded_h):
    """What ``undistort_images`` needs to know of a ``ColmapCamera`` whose image was loaded at ``loaded_w x loaded_h``:
    ``(model id, (fx, fy, cx, cy), (out_fx, out_fy), coefficients)``.  The intrinsics are the file's, scaled by
    ``loaded_w / intr.width`` and ``loaded_h / intr.height``; the output focal lengths are the same scaled fx, fy (f for
    both axes of a one-focal model), which is the camera ``camera_from_colmap`` builds; the coefficients act on normalised
    coordinates and do not scale.  Fisheye, FOV and thin-prism models raise ``ValueError``."""
    if intr.model not in SUPPORTED_MODELS:
        raise ValueError(f"COLMAP camera model {intr.model} cannot be undistorted: supported are "
                         f"{', '.join(SUPPORTED_MODELS)}")
    p = [float(v) for v in intr.params]
    if intr.model in _ONE_FOCAL:
        fx = fy = p[0]
        cx, cy, coef = p[1], p[2], p[3:]
    else:
        fx, fy, cx, cy, coef = p[0], p[1], p[2], p[3], p[4:]
    sx, sy = loaded_w / intr.width, loaded_h / intr.height
    return SUPPORTED_MODELS[intr.model], (fx * sx, fy * sy, cx * sx, cy * sy), (fx * sx, fy * sy), tuple(coef)


def _distort(model, x, y, k):
    """(xd, yd) of the normalised ideal coordinates (x, y), float64, in the kernel's order of operations."""
    if model in (0, 1):
        return x, y
    r2 = x * x + y * y
    if model == 2:
        s = 1.0 + k[0] * r2
    elif model == 6:
        s = ((1.0 + k[0] * r2 + k[1] * r2 * r2 + k[4] * r2 * r2 * r2) /
             (1.0 + k[5] * r2 + k[6] * r2 * r2 + k[7] * r2 * r2 * r2))
    else:   # 3, 4
        s = 1.0 + k[0] * r2 + k[1] * r2 * r2
    xd, yd = x * s, y * s
    if model in (4, 6):
        p1, p2 = k[2], k[3]
        xd = xd + 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x)
        yd = yd + p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y
    return xd, yd


def source_positions(height, width, model, intrinsics, params, out_focals):
    """(u, v), float64 [height,width]: where each output pixel samples the source, in source pixel indices."""
    fx, fy, cx, cy = (float(t) for t in intrinsics)
    ofx, ofy = (float(t) for t in out_focals)
    k = np.zeros(8)
    k[:len(params)] = params
    i = np.arange(width, dtype=np.float64)[None, :]
    j = np.arange(height, dtype=np.float64)[:, None]
    x = np.broadcast_to((i + 0.5 - width / 2.0) / ofx, (height, width))
    y = np.broadcast_to((j + 0.5 - height / 2.0) / ofy, (height, width))
    with np.errstate(all="ignore"):
        xd, yd = _distort(int(model), x, y, k)
        return fx * xd + cx - 0.5, fy * yd + cy - 0.5


def undistort_host_f64(image, model, intrinsics, params, out_focals, fill=0.0):
    """One view on the host: ``(float64 [C,H,W], number of blank pixels)``, the blend before its cast to float32."""
    src = np.asarray(image, np.float64)
    _, H, W = src.shape
    u, v = source_positions(H, W, model, intrinsics, params, out_focals)
    valid = (u > -1.0) & (u < W) & (v > -1.0) & (v < H)          # a NaN compares false
    u, v = np.where(valid, u, 0.0), np.where(valid, v, 0.0)
    fu, fv = np.floor(u), np.floor(v)
    a, b = u - fu, v - fv
    x0, y0 = fu.astype(np.int64), fv.astype(np.int64)
    cx0, cx1, ry0, ry1 = x0 >= 0, x0 + 1 <= W - 1, y0 >= 0, y0 + 1 <= H - 1

    def tap(xs, ys, inside):
        t = src[:, np.clip(ys, 0, H - 1), np.clip(xs, 0, W - 1)]
        return np.where(inside[None], t, float(fill))

    out = (((1.0 - a) * (1.0 - b))[None] * tap(x0, y0, cx0 & ry0) + (a * (1.0 - b))[None] * tap(x0 + 1, y0, cx1 & ry0)
           + ((1.0 - a) * b)[None] * tap(x0, y0 + 1, cx0 & ry1)) + (a * b)[None] * tap(x0 + 1, y0 + 1, cx1 & ry1)
    blank = ~valid          # inside the range a tap of non-zero weight is in the source: x0 = -1 has a > 0, y0 = -1 has b > 0
    out = np.where(blank[None], float(fill), out)
    return out, int(blank.sum())


def _normalise(images, models, intrinsics, params, out_focals):
    images = list(images)
    n = len(images)
    models, intrinsics, params, out_focals = list(models), list(intrinsics), list(params), list(out_focals)
    if not (len(models) == len(intrinsics) == len(params) == len(out_focals) == n):
        raise ValueError(f"undistort_images: {n} images but {len(models)} models, {len(intrinsics)} intrinsics, "
                         f"{len(params)} coefficient lists and {len(out_focals)} output focal lengths")
    for v, im in enumerate(images):
        if not torch.is_tensor(im) or im.dim() != 3 or im.dtype != torch.float32:
            raise ValueError(f"undistort_images: images[{v}] must be a [C,H,W] float32 tensor")
        if not 1 <= im.shape[0] <= L.UNDISTORT_MAX_CHANNELS or im.shape[1] == 0 or im.shape[2] == 0:
            raise ValueError(f"undistort_images: images[{v}] must have 1..{L.UNDISTORT_MAX_CHANNELS} channels and a non-empty "
                             f"pixel grid (got shape {tuple(im.shape)})")
        if len(intrinsics[v]) != 4 or len(out_focals[v]) != 2 or len(params[v]) > 8:
            raise ValueError(f"undistort_images: view {v} needs (fx, fy, cx, cy), (out_fx, out_fy) and at most 8 coefficients")
    models = [int(m) for m in models]
    for v, m in enumerate(models):
        if m not in SUPPORTED_MODELS.values():
            raise ValueError(f"undistort_images: view {v}: camera model id {m} is not supported (supported: "
                             f"{', '.join(f'{name} {mid}' for name, mid in SUPPORTED_MODELS.items())})")
    return images, models, intrinsics, params, out_focals


def undistort_images(images, models, intrinsics, params, out_focals, fill=0.0, backend="gpu"):
    """images: [C,H,W] float32 tensors (C 1..4; sizes may differ), each detected in the camera ``models[v]`` (a COLMAP model
    id), ``intrinsics[v]`` = (fx, fy, cx, cy) in its own pixels, ``params[v]`` its distortion coefficients in COLMAP's
    order.  Returns ``(undistorted, blank_counts)``: the images as the pinhole camera with focal lengths ``out_focals[v]``
    and a centred principal point sees them, and an int32 tensor [V] of the pixels per view that no source pixel reaches
    (they hold ``fill``).  ``distortion_of`` derives the four per-view arguments from a ``ColmapCamera``.

    ``backend="gpu"``: images not on a GPU are uploaded to the current one; the results stay on the device, nothing is read
    back.  ``backend="host"``: numpy, float64, rounded to float32 once; CPU tensors."""
    _check_backend(backend)
    images, models, intrinsics, params, out_focals = _normalise(images, models, intrinsics, params, out_focals)
    if backend == "host":
        outs, counts = [], []
        for v, im in enumerate(images):
            out, cnt = undistort_host_f64(im.detach().cpu().numpy(), models[v], intrinsics[v], params[v], out_focals[v], fill)
            outs.append(torch.from_numpy(out.astype(np.float32)))
            counts.append(cnt)
        return outs, torch.tensor(counts, dtype=torch.int32)
    if not images:
        return [], torch.zeros(0, dtype=torch.int32)
    lib = L.load()
    dev = next((im.device for im in images if im.is_cuda), None)
    if dev is None:
        if not torch.cuda.is_available():
            raise L.CurveGSError("undistort_images: backend='gpu' needs a GPU (backend='host' computes on the CPU)")
        dev = torch.device("cuda", torch.cuda.current_device())
    with L.device_guard(dev):
        srcs = [im.detach().to(dev).contiguous() for im in images]
        dsts = [torch.empty_like(s) for s in srcs]
        blank = torch.zeros(len(srcs), dtype=torch.int32, device=dev)
        stream = L.raw_stream(dev)
        for first in range(0, len(srcs), L.UNDISTORT_MAX_VIEWS):
            count = min(L.UNDISTORT_MAX_VIEWS, len(srcs) - first)
            table = (L.UndistortView * count)()
            for k in range(count):
                v = first + k
                coef = (C.c_double * 8)(*[float(t) for t in params[v]])
                table[k] = L.UndistortView(srcs[v].data_ptr(), dsts[v].data_ptr(), *(int(t) for t in srcs[v].shape), models[v],
                                           *(float(t) for t in intrinsics[v]), *(float(t) for t in out_focals[v]), coef)
            rc = lib.cgs_undistort_images(count, C.cast(table, C.c_void_p), float(fill), C.c_void_p(blank[first:].data_ptr()),
                                          stream)
            L.check(rc, "cgs_undistort_images")
    # (uploaded copies go back to the caching allocator on this stream: reuse is stream-ordered)
    return dsts, blank
