"""Float64 restatements of the training-loss and Adam components (test helper, not a conftest).

Each function restates the reference project's formula in float64 torch (any device), so a float32 HIP kernel can be
held to a high-precision value rather than to another float32 implementation:

  ssim64                 utils/loss_utils.py:56-86 / fused-ssim: 11-tap Gaussian (sigma 1.5, taps rounded to float32 as the
                         reference's ``.float()`` window is), zero padding, "same" or "valid"; map, mean, d mean / d img1,
                         and a per-pixel first-order bound on the error of a float32 evaluation (``ssim_error_bounds``)
  edge_aware_loss64      utils/loss_utils.py:94-115
  photometric64          a * edge_aware_loss + b * (1 - ssim), optionally on clamp(image, 0, 1) (inclusive gradient mask)
  regularizers64         train.py:113-131 (opacity, curve smoothness, width)
  connection64           train.py:133-146 from exact pairwise differences, with the pair count
  adam64_step            torch.optim.Adam (non-amsgrad, no weight decay) with per-element learning rates

Test tensors in, float64 out; nothing here calls a HIP kernel."""
import math

import numpy as np
import torch
import torch.nn.functional as F

EPS32 = 2.0 ** -24            # unit roundoff of float32 (round to nearest)
SSIM_C1, SSIM_C2 = 0.01 ** 2, 0.03 ** 2


def gaussian_taps32():
    """The reference's window: exp(-(x - 5)^2 / (2 * 1.5^2)) normalised, rounded to float32 (loss_utils.py:46-54)."""
    g = np.array([math.exp(-(x - 5) ** 2 / (2 * 1.5 ** 2)) for x in range(11)])
    return (g / g.sum()).astype(np.float32).astype(np.float64)


def _filt(x, taps):
    """Separable 11-tap filter of [..., H, W] with zero padding ("same" size), in the dtype of x."""
    H, W = x.shape[-2:]
    xp = F.pad(x, (5, 5, 5, 5))
    h = sum(taps[k] * xp[..., :, k:k + W] for k in range(11))
    return sum(taps[k] * h[..., k:k + H, :] for k in range(11))


def _crop(t, padding):
    return t if padding == "same" else t[..., 5:-5, 5:-5]


def ssim_parts64(img1, img2, C1=SSIM_C1, C2=SSIM_C2):
    """Float64 moments and SSIM map of two [..., H, W] images (no cropping)."""
    g = gaussian_taps32()
    x, y = img1.double(), img2.double()
    mu1, mu2 = _filt(x, g), _filt(y, g)
    e11, e22, e12 = _filt(x * x, g), _filt(y * y, g), _filt(x * y, g)
    A = mu1 * mu1 + mu2 * mu2 + C1
    B = (e11 - mu1 * mu1) + (e22 - mu2 * mu2) + C2
    Cn = 2 * mu1 * mu2 + C1
    D = 2 * (e12 - mu1 * mu2) + C2
    return dict(mu1=mu1, mu2=mu2, e11=e11, e22=e22, e12=e12, A=A, B=B, C=Cn, D=D, map=Cn * D / (A * B))


def ssim64(img1, img2, padding="same"):
    """(map, mean, d mean / d img1) in float64.  With "valid" on images of <= 10 px the crop is empty: the mean is NaN
    (mean of nothing) and the gradient is zero, as in the reference."""
    x = img1.detach().double().requires_grad_(True)
    m = _crop(ssim_parts64(x, img2)["map"], padding)
    mean = m.mean()
    if m.numel():
        (grad,) = torch.autograd.grad(mean, x)
    else:
        grad = torch.zeros_like(x)
    return m.detach(), mean.detach(), grad


def ssim_vjp64(img1, img2, dL_dmap):
    """d (sum dL_dmap * map) / d img1 in float64 (uncropped map)."""
    x = img1.detach().double().requires_grad_(True)
    m = ssim_parts64(x, img2)["map"]
    (grad,) = torch.autograd.grad(m, x, dL_dmap.double())
    return grad


def ssim_error_bounds(img1, img2, dL_dmap=None, K=64.0):
    """First-order bounds on |float32 evaluation - exact| for the SSIM map and for d L / d img1.

    Every filtered moment is 121 products summed in 2 x 11 steps with non-negative terms: relative error <= 22 eps of its
    magnitude (moments of |x| for signed images).  The variances and covariance subtract mu^2 terms: absolute error
    <= ~24 eps of the magnitudes SB = e11 + e22 + mu1^2 + mu2^2 + C2, SD = 2 (e12 + mu1 mu2) + C2, SC = 2 mu1 mu2 + C1;
    the ratio adds a few roundings more.  Dividing by B (>= C2) turns those into
    err(map) <= c eps (|map| + (|C| SD + |D| SC) / (A B) + |map| SB / B);  c = K = 64 covers 22 + 24 + ratio
    steps with room.  For the gradient the three derivative maps carry the same relative condition kappa = 1 + (SB + SD)/B
    and then go through two more 11-tap passes (22 eps of their magnitudes).  Returns (map_bound, grad_bound) [..., H, W]."""
    p = ssim_parts64(img1, img2)
    A, B, Cn, D, val = p["A"], p["B"], p["C"], p["D"], p["map"]
    g = gaussian_taps32()
    x, y = img1.double().abs(), img2.double().abs()
    mu1, mu2 = _filt(x, g), _filt(y, g)                  # magnitudes: equal to mu1, mu2 for images >= 0
    SB = p["e11"] + p["e22"] + mu1 * mu1 + mu2 * mu2 + SSIM_C2
    SD = 2 * (_filt(x * y, g) + mu1 * mu2) + SSIM_C2
    SC = 2 * mu1 * mu2 + SSIM_C1
    e = K * EPS32
    map_bound = e * (val.abs() + (Cn.abs() * SD + D.abs() * SC) / (A * B) + val.abs() * SB / B)
    if dL_dmap is None:
        return map_bound, None
    kappa = 1 + (SB + SD) / B
    m1 = 2 / (A * B) * (mu2.abs() * (D.abs() + Cn.abs()) + mu1.abs() * val.abs() * (B + A))
    m2 = val.abs() / B
    m3 = 2 * Cn.abs() / (A * B)
    dl = dL_dmap.double().abs()
    S = _filt(dl * m1 * (1 + kappa), g) + 2 * x * _filt(dl * m2 * (1 + kappa), g) + y * _filt(dl * m3 * (1 + kappa), g)
    grad_bound = e * S
    return map_bound, grad_bound


def edge_weights64(gt, threshold=0.1):
    """(edge mask [1,H,W], weights [1,H,W], n_pos) of loss_utils.py:100-108.  The edge map is the channel mean, compared
    with the threshold as float32 (torch compares a float32 tensor with the scalar in float32: a value equal to
    float32(threshold) is not an edge)."""
    edge_map = gt.double().mean(dim=0, keepdim=True)
    thr = float(np.float32(threshold))
    mask = edge_map > thr
    n_pos = float(mask.sum())
    n = float(mask.numel())
    n_neg = n - n_pos
    w = torch.where(mask, 5.0 * (n_neg + 1) / n, 1.0 * (n_pos + 1) / n).to(torch.float64)
    return mask, w, int(n_pos)


def edge_aware_loss64(image, gt, threshold=0.1):
    """(value, d value / d image) of loss_utils.py:94-115 in float64; image, gt [C,H,W]."""
    _, w, _ = edge_weights64(gt, threshold)
    d = image.double() - gt.double()
    val = (d * d * w).mean()
    return val, 2.0 * d * w / d.numel()


def photometric64(image, gt, a, b, threshold=0.1, clamp=False):
    """(value, d value / d image) of  a * edge_aware_loss(x, gt) + b * (1 - ssim(x, gt)),  x = clamp(image, 0, 1) if clamp
    (render()'s clamp: its gradient passes where 0 <= image <= 1, bounds included, as torch.clamp's does)."""
    img = image.detach().double().requires_grad_(True)
    x = img.clamp(0.0, 1.0) if clamp else img
    _, w, _ = edge_weights64(gt, threshold)
    d = x - gt.double()
    edge = (d * d * w).mean()
    ssim = ssim_parts64(x.unsqueeze(0), gt.double().unsqueeze(0))["map"].mean()
    val = a * edge + b * (1.0 - ssim)
    (grad,) = torch.autograd.grad(val, img)
    return val.detach(), grad


def quaternion_axis0_64(q):
    """Column 0 of pytorch3d.quaternion_to_matrix(F.normalize(q)) (the reference's get_rotation_matrix[..., 0])."""
    qn = q / q.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    r, i, j, k = qn.unbind(-1)
    two_s = 2.0 / (qn * qn).sum(-1)
    return torch.stack((1 - two_s * (j * j + k * k), two_s * (i * j + k * r), two_s * (i * k - j * r)), -1)


def regularizers64(rotation_raw, opacity_logit, width_log, radii, m, w_op=0.01, gate=1.0, w_smo=0.1, w_width=0.01,
                   width_thr=0.005):
    """train.py:113-131 written out literally (visibility_filter = radii > 0; the opacity of a splat is its curve's;
    get_curve_width = exp(_width)).  Returns (value, d/d rotation_raw, d/d opacity_logit, d/d width_log), float64."""
    rot = rotation_raw.detach().double().requires_grad_(True)
    op = opacity_logit.detach().double().requires_grad_(True)
    wl = width_log.detach().double().requires_grad_(True)
    vis = radii.reshape(-1) > 0
    loss = rot.sum() * 0.0 + op.sum() * 0.0 + wl.sum() * 0.0
    if bool(vis.sum() > 0):
        opacity = torch.sigmoid(op).reshape(-1, 1).repeat_interleave(m, 0)[vis]
        loss = loss + w_op * float(gate) * torch.log(1 + opacity ** 2 / 0.5).mean()
    if w_smo > 0 and bool(vis.sum() > 0):
        d = quaternion_axis0_64(rot).reshape(-1, m, 3)
        u, v = d[:, :-1, :], d[:, 1:, :]
        eps = 1e-8
        cos = (u * v).sum(-1) / (u.norm(dim=-1).clamp_min(eps) * v.norm(dim=-1).clamp_min(eps))
        loss = loss + w_smo * (1 - cos.abs()).mean()
    if w_width > 0:
        width = torch.exp(wl)
        mask = width >= width_thr
        if bool(mask.any()):
            loss = loss + w_width * (width[mask] - width_thr).mean()
    g = torch.autograd.grad(loss, (rot, op, wl))
    return (loss.detach(),) + tuple(g)


def connection64(curve_points, thr=0.05, weight=0.1, chunk=4096):
    """train.py:133-146: end points p (B starts, then B ends), every ordered pair (i, j) of different curves with
    |p_i - p_j| < thr (thr as float32), loss = weight * mean of those distances.  Brute force over all pairs, distances
    from exact coordinate differences (never the |a|^2 + |b|^2 - 2ab expansion) in float64, row chunk by row chunk:
    O(chunk * 2B) memory.
    Returns (value, d value / d curve_points [B, K, 3], pair count, ambiguous, max degree) where `ambiguous` counts the
    ordered pairs with |d - thr| <= 4 ulp(thr) (a float32 kernel may count those either way) and `max degree` is the
    largest number of partners of one end point."""
    cp = curve_points.detach().double()
    B = cp.shape[0]
    pts = torch.cat([cp[:, 0], cp[:, -1]], 0)
    N = 2 * B
    curve = torch.arange(N, device=cp.device) % B
    t = float(np.float32(thr))
    tol = 4 * float(np.spacing(np.float32(t)))
    g = torch.zeros_like(pts)
    deg = torch.zeros(N, dtype=torch.int64, device=cp.device)
    total, count, ambiguous = 0.0, 0, 0
    for a in range(0, N, chunk):
        rows = pts[a:a + chunk]
        d = sum((rows[:, k, None] - pts[None, :, k]) ** 2 for k in range(3)).sqrt()
        diff_curve = curve[a:a + chunk, None] != curve[None, :]
        ambiguous += int(((d - t).abs() <= tol)[diff_curve].sum())
        sel = (d < t) & diff_curve
        i, j = sel.nonzero(as_tuple=True)
        if i.numel() == 0:
            continue
        ii = i + a
        e = pts[ii] - pts[j]
        dist = e.norm(dim=-1)
        total += float(dist.sum())
        count += int(i.numel())
        nz = dist > 0
        g.index_add_(0, ii[nz], e[nz] / dist[nz, None])
        deg.index_add_(0, ii, torch.ones_like(ii))
    if count == 0:
        return 0.0, torch.zeros_like(cp), 0, ambiguous, 0
    grad = torch.zeros_like(cp)
    scale = 2.0 * weight / count           # each unordered pair appears twice in the mean
    grad[:, 0] = scale * g[:B]
    grad[:, -1] = scale * g[B:]
    return weight * total / count, grad, count, ambiguous, int(deg.max())


def adam64_step(p, g, m, v, step, lr, beta1=0.9, beta2=0.999, eps=1e-15):
    """One torch.optim.Adam step (non-amsgrad, no weight decay) in float64; lr scalar or per-element tensor.
    Returns (p, m, v)."""
    p, g, m, v = (t.double() for t in (p, g, m, v))
    m = beta1 * m + (1 - beta1) * g
    v = beta2 * v + (1 - beta2) * g * g
    bc1 = 1 - beta1 ** step
    bc2 = 1 - beta2 ** step
    denom = v.sqrt() / math.sqrt(bc2) + eps
    return p - (lr / bc1) * m / denom, m, v
