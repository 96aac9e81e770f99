"""Shared cases of the training gate's tests (test_train_gate_cpu.py, test_train_gate_gpu.py): the smallest shapes at which
the gated per-splat kernel can still go wrong.

The scene: an image of 40 x 24 pixels (no multiple of the 16-pixel tile, six tiles), three views with three different planes,
and B curves of 12 splats with B = 20 (P = 240, one partial block) and B = 22 (P = 264, just above the 256-thread block).
View 0 looks at the cloud from outside; view 1 from close by, so that many centres fall off the image while their footprints
still overlap it; view 2 stands INSIDE the cloud, so that centres lie behind the camera.  The planes: view 0 a ramp through
the cloud with one NaN and one +inf entry under projected centres; view 1 a plane in front of everything (every in-image
centre is hidden); view 2 a constant plane through the middle of what it sees."""
import math

import numpy as np
import torch

from curve_gaussian_amd import synthetic as S

H, W = 24, 40
SLACK = 0.05
SIZES = (20, 22)      # curves: P = 240 (below one block of 256) and P = 264 (just above it)


def curves(B, seed=5):
    c = S.make_curves(B, seed)
    g = torch.Generator().manual_seed(seed)
    c["width"] = c["width"] + 0.8 + 0.3 * torch.randn(B, 1, generator=g)   # footprints of several pixels
    c["is_bezier"] = torch.rand(B, generator=g) > 0.25
    return c


def cameras():
    return [S.make_camera((0.5, -1.7, 0.9), (0.5, 0.5, 0.5), (0, 0, 1), H, W),
            S.make_camera((1.3, 0.5, 0.6), (0.5, 0.5, 0.5), (0, 0, 1), H, W),       # close: centres off the image
            # inside the cloud, a wider field of view: centres behind the camera
            S.make_camera((0.5, 0.3, 0.5), (0.5, 1.0, 0.5), (0, 0, 1), H, W, fovx=1.2, fovy=0.8)]


def planes():
    """float32 [3,H,W] (numpy), every entry finite and > 0 (what TrainGate's depth_maps accept); ``poke`` adds the NaN and
    the +inf afterwards."""
    jj, ii = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32))
    p0 = 2.0 + 0.02 * (jj - W / 2) + 0.01 * (ii - H / 2)       # a ramp through the cloud (the centre is 2.24 away)
    p1 = np.full((H, W), 0.05, np.float32)                      # in front of everything
    p2 = np.full((H, W), 0.66, np.float32)                      # through the middle of what view 2 keeps
    return np.stack([p0, p1, p2]).astype(np.float32)


def poke(stack, xyz, K, M):
    """Puts a NaN and a +inf into plane 0 (a tensor, in place) under two centres that view 0 keeps and the ramp HIDES, so
    that both entries change a verdict: -> ((row, col) of the NaN, (row, col) of the +inf)."""
    from curve_gaussian_amd.ops.edge_occlusion import gate_view_host
    u, v, _seen, hid = gate_view_host(xyz, K[0], M[0], stack[0].cpu().numpy(), SLACK)
    cells = []
    for p in np.flatnonzero(hid):
        cell = (int(math.floor(v[p])), int(math.floor(u[p])))
        if cell not in cells:
            cells.append(cell)
        if len(cells) == 2:
            break
    assert len(cells) == 2, "the ramp hides centres in fewer than two pixels: the NaN / +inf entries would change nothing"
    stack[0, cells[0][0], cells[0][1]] = float("nan")
    stack[0, cells[1][0], cells[1][1]] = float("inf")
    return cells[0], cells[1]


def manual_gate(cams, stack, slack=SLACK, device=None):
    """A TrainGate over ``cams`` whose planes are exactly ``stack`` (float32 [V,H,W] numpy, finite and > 0: no window)."""
    from curve_gaussian_amd.ops.train_gate import TrainGate
    return TrainGate(cams, depth_maps=[p for p in stack], depth_slack=slack, depth_window=0,
                     backend="host" if device is None else "gpu", device=device)


def box_scan(n_views=6, height=60, width=80, backend="host", device=None):
    from curve_gaussian_amd.scene.solid_scan import solid_scan
    return solid_scan("box", n_views, height, width, backend=backend, device=device)


def line_curves(edges, m=12):
    """The ground-truth lines of a solid as cubic Bezier curves (control points at the thirds): the model whose curves ARE
    the solid's edges.  -> the dict GaussianCurveModel.create_from_curves takes."""
    ends = torch.tensor(edges["lines_end_pts"], dtype=torch.float32).reshape(-1, 2, 3)
    a, b = ends[:, 0], ends[:, 1]
    cp = torch.stack([a, a + (b - a) / 3.0, a + (b - a) * (2.0 / 3.0), b], 1).contiguous()
    B = cp.shape[0]
    return {"curve_points": cp, "width": torch.full((B, 1), math.log(5e-3)), "opacity": torch.full((B, 1), math.log(0.9 / 0.1)),
            "is_bezier": torch.ones(B, dtype=torch.bool), "mask": torch.ones(B, m, 1)}
