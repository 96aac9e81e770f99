"""Float64 numpy restatement of the novel-view kernels (cgs_project_points / cgs_render_points), used by
tests/test_novel_view_cpu.py (pinned to the reference-generated fixture and to hand-computed pixels) and by
tests/test_novel_view_gpu.py (the kernels against it)."""
import numpy as np


def project(points, R, T, fx, fy, cx, cy, W, H):
    """(keep bool [P], u, v float64 [P]) with the reference's operation order: c = ((r0 X + r1 Y) + r2 Z) + t per row,
    dropped if c2 <= 0, u = fx (c0 / c2) + cx, v = fy (c1 / c2) + cy, kept if 0 <= u < W and 0 <= v < H."""
    X = np.asarray(points, np.float32).astype(np.float64)
    x, y, z = X[:, 0], X[:, 1], X[:, 2]
    R = np.asarray(R, np.float64)
    T = np.asarray(T, np.float64)
    c = [((R[k, 0] * x + R[k, 1] * y) + R[k, 2] * z) + T[k] for k in range(3)]
    with np.errstate(divide="ignore", invalid="ignore"):
        u = fx * (c[0] / c[2]) + cx
        v = fy * (c[1] / c[2]) + cy
    keep = (c[2] > 0) & (u >= 0) & (u < W) & (v >= 0) & (v < H)
    return keep, u, v


def composite(pix, colors, alpha, background, n_pix):
    """out [n_pix,3]: the points of `pix` (pixel index per point, in ascending point order) composited with constant
    alpha over the background, out = bg (1-a)^n + sum_j a c_j (1-a)^r_j, r_j = the number of later points in the pixel."""
    pix = np.asarray(pix, np.int64)
    colors = np.asarray(colors, np.float64).reshape(-1, 3)
    order = np.argsort(pix, kind="stable")
    sp = pix[order]
    n = np.bincount(pix, minlength=n_pix)
    start = np.concatenate([[0], np.cumsum(n)])[sp]
    r = n[sp] - 1 - (np.arange(len(sp)) - start)
    w = alpha * (1.0 - alpha) ** r.astype(np.float64)
    out = np.empty((n_pix, 3))
    bgw = (1.0 - alpha) ** n.astype(np.float64)
    for k in range(3):
        out[:, k] = np.bincount(sp, weights=w * colors[order, k], minlength=n_pix) + background[k] * bgw
    return out


def render(points, colors, R, T, fx, fy, cx, cy, W, H, alpha=0.5, background=(1.0, 1.0, 1.0)):
    """float64 [H,W,3] image of one view and the number of kept points."""
    keep, u, v = project(points, R, T, fx, fy, cx, cy, W, H)
    pix = np.floor(v[keep]).astype(np.int64) * W + np.floor(u[keep]).astype(np.int64)
    out = composite(pix, np.asarray(colors)[keep], alpha, np.asarray(background, np.float64), H * W)
    return out.reshape(H, W, 3), int(keep.sum())
