"""float64 numpy restatement of the held-out metrics (reference train.py:321-376 with utils/loss_utils.py l1_loss and
utils/image_utils.py psnr), the yardstick of csrc/metrics.hip and curve_gaussian_amd.evaluation: d is formed in float32
from the clamped render and edge map exactly as torch forms it, every reduction after that is float64."""
import math

import numpy as np


def view_sums(image, gt, half_width=False):
    """image [1,H,W], gt [Cg,H,W] -> (sum |d|, sum d^2, count) over the gt's channels (broadcast) and, with half_width,
    the columns W//2 .. W-1."""
    im = np.clip(np.asarray(image, np.float32), np.float32(0), np.float32(1))
    g = np.clip(np.asarray(gt, np.float32), np.float32(0), np.float32(1))
    if half_width:
        im, g = im[..., im.shape[-1] // 2:], g[..., g.shape[-1] // 2:]
    d = (np.broadcast_to(im, g.shape) - g).astype(np.float32).astype(np.float64)
    return float(np.abs(d).sum()), float((d * d).sum()), d.size


def view_metrics(images, gts, half_width=False):
    """-> (l1 [V], mse [V]) float64."""
    out = [view_sums(i, g, half_width) for i, g in zip(images, gts)]
    return np.array([a / n for a, _, n in out]), np.array([b / n for _, b, n in out])


def psnr(mse):
    return math.inf if mse == 0 else 20.0 * math.log10(1.0 / math.sqrt(mse))


def report(images, gts, half_width=False):
    """The printed values of one config: mean per-view L1 and mean per-view PSNR."""
    l1, mse = view_metrics(images, gts, half_width)
    return float(l1.mean()), float(np.mean([psnr(m) for m in mse]))
