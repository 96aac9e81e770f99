"""The truth of the per-view chain (curve tensors -> image -> curve-parameter gradients) at ANY sample count m, and the small
scenes the fused view kernels are held to it on (tests/test_view_ref64_cpu.py, tests/test_view_shapes_gpu.py).

view_ref64 is tests/golden/make_view_golden.py::chain -- the chain the frozen view_*.npz files hold -- with two arguments
changed: the float32 splat tensors of oracle/torch_ref.py (prepare_scaling_rot(..., m), normalize, sigmoid, the
straight-through mask, build_all_map) go through the C oracle's forward and backward (oracle/raster_ref.c), and its per-splat
gradients are pulled back through the same torch_ref functions in FLOAT64 autograd.

The scenes sit on no compositor decision edge (alpha < 1/255, T < 1e-4, the radius rounding, the mask threshold): that is
what lets the GPU tests compare element-wise with no outlier budget, and tests/test_view_ref64_cpu.py holds every scene
listed here to it.  A seed that fails there is replaced HERE; the GPU test is not loosened."""
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from make_view_golden import chain  # noqa: E402
from util import S  # noqa: E402

MASK_THR = 0.3
H, W = 64, 80           # ragged in both tile directions (16 x 16 tiles)
EYE, TARGET = (0.5, -1.7, 0.9), (0.5, 0.5, 0.5)
SECOND_EYE = (2.1, 1.2, 1.0)
# inside the cloud: the near plane (z <= 0.2) and the image border cut through curves
CULL_EYE, CULL_TARGET = (0.5, 0.2, 0.5), (0.5, 0.9, 0.5)

# (B, m) -> seed.  The seven slot shapes of test_sampling_gpu.py::SAMPLE_CASES and a full grid of several blocks plus a tail
# at MAX_M (25 x 32: eight curves per block, three full blocks and one curve)
SHAPE_SEEDS = {(1, 5): 11, (1, 32): 12, (22, 12): 33, (43, 12): 34, (9, 32): 25, (33, 8): 16, (65, 4): 87, (25, 32): 48}
# the two shapes that also run under the culling camera (curves three times as long, so that many are cut)
CULL_SEEDS = {(22, 12): 23, (9, 32): 45}
# the large instance of k_view_bwd is launched from 512 Ki splats: one curve below and one at the threshold
LARGE_B = (43690, 43691)
LARGE_M, LARGE_VISIBLE, LARGE_SEED = 12, 200, 41


def view_ref64(curves, mask_logit, mask_thr, cam, bg, dimg, m, **kw):
    """-> dict(color [1,H,W], radii [P], g_means2D [P,3], g_curve_points [B,4,3], g_width [B,1], g_opacity [B,1][, g_mask
    [B,m,1]], and the further outputs of `chain`)."""
    return chain(curves, mask_logit, cam, float(bg), np.asarray(dimg, np.float32).reshape(1, cam.image_height, cam.image_width),
                 m=m, mask_thr=mask_thr, pull=torch.float64, **kw)


def scene(B, m, seed, cull=False, second=False):
    """-> (curves, mask logits [B,m,1], camera, dL/dimage [1,H,W]): S.make_curves(B, seed) with fatter splats of varied width
    and opacity, mixed curve types and mask logits on both sides of MASK_THR.  second: the same curves from SECOND_EYE with
    another upstream gradient (the second view of a shared-sampling batch)."""
    c = S.make_curves(B, seed, m=m)
    g = torch.Generator().manual_seed(seed)
    c["width"] = c["width"] + 0.8 + 0.3 * torch.randn(B, 1, generator=g)
    # the m samples of a curve lie on top of each other on this image: an opacity of about min(0.5, 2 / m) per sample keeps
    # every pixel's transmittance far above the T < 1e-4 cut
    op = min(0.5, 2.0 / m)
    c["opacity"] = torch.full((B, 1), math.log(op / (1.0 - op))) + 0.7 * torch.randn(B, 1, generator=g)
    c["is_bezier"] = torch.rand(B, generator=g) > 0.25
    mask = torch.randn(B, m, 1, generator=g) * 3
    dimg = torch.randn(1, H, W, generator=g)
    if cull:
        p0 = c["curve_points"][:, :1]
        c["curve_points"] = (p0 + 3.0 * (c["curve_points"] - p0)).contiguous()
    cam = S.make_camera(CULL_EYE if cull else EYE, CULL_TARGET if cull else TARGET, (0, 0, 1), H, W)
    if second:
        cam = S.make_camera(SECOND_EYE, TARGET, (0, 0, 1), H, W)
        dimg = torch.randn(1, H, W, generator=g)
    return c, mask, cam, dimg


def large_scene(B):
    """LARGE_VISIBLE curves of scene(.., LARGE_M, LARGE_SEED) in front of the camera and B - LARGE_VISIBLE behind it: culled, so
    they cost the compositors nothing, and still reached by the two grid-wide norm sums of the sampling backward."""
    c, _mask, cam, dimg = scene(LARGE_VISIBLE, LARGE_M, LARGE_SEED)
    c["opacity"] = c["opacity"] - 1.5          # (several hundred curves on this image: fainter still, for the same reason)
    rest = S.make_curves(B - LARGE_VISIBLE, LARGE_SEED + 1)
    g = torch.Generator().manual_seed(LARGE_SEED + 1)
    rest["curve_points"] = rest["curve_points"] + torch.tensor([0.0, -4.0, 0.0])      # behind EYE, which looks along +y
    rest["is_bezier"] = torch.rand(B - LARGE_VISIBLE, generator=g) > 0.25
    out = {k: torch.cat([c[k], rest[k]]).contiguous() for k in ("curve_points", "width", "opacity", "is_bezier")}
    return out, None, cam, dimg


def partly_culled(radii, B, m):
    """[B] bool: curves with some but not all of their samples culled (radius 0)."""
    vis = (np.asarray(radii).reshape(B, m) > 0).sum(1)
    return (vis > 0) & (vis < m)
