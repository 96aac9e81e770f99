"""Held-out evaluation of the training loop (reference train.py:321-376, ``training_report``).

``view_metrics``     per-view L1 and MSE of clamped renders against their edge maps: ONE HIP launch for any number of
                     views (csrc/metrics.hip), float64 results that stay on the device.
``evaluate_views``   renders cameras forward-only through ``gaussian_renderer.render`` (the fused route for a
                     ``GaussianCurveModel`` under default flags) and reduces them with one ``view_metrics`` call and one
                     host readback.
``training_report``  drop-in for the reference's function of the same signature.

Arithmetic: the reference adds ``l1_loss(image, gt).mean().double()`` and ``psnr(image, gt).mean().double()`` over the
views (float32 means, PSNR = 20 log10(1 / sqrt(mse))) and divides by the number of views.  Here the per-view sums are
float64 (kernel), the PSNR of each view is taken in float64 from its MSE, and the report is the mean of the per-view
values -- not the PSNR of the mean MSE.  An exact match (mse = 0) gives inf, as in the reference."""
import ctypes as C
import math

import torch

from . import _lib as L


def _as_chw(t, what):
    if t.dim() == 2:
        t = t.unsqueeze(0)
    if t.dim() != 3:
        raise ValueError(f"view_metrics: {what} must be [C,H,W] or [H,W] (got shape {tuple(t.shape)})")
    return t.detach().float().contiguous()


def view_metrics(images, gts, half_width=False):
    """images: renders, each [1,H,W] (or [H,W]); gts: their edge maps, each [Cg,H,W] with the same H, W (broadcast over
    Cg as ``l1_loss(image, gt)`` / ``psnr(image, gt)`` broadcast).  Views may differ in size.  ``half_width``: only the
    columns W//2 .. W-1 (``train_test_exp``).  Returns device float64 ``(l1 [V], mse [V])`` of
    d = clamp(image, 0, 1) - clamp(gt, 0, 1); one kernel launch on the current stream, no synchronisation."""
    images, gts = list(images), list(gts)
    if len(images) != len(gts):
        raise ValueError(f"view_metrics: {len(images)} images but {len(gts)} ground truths")
    if not images:
        raise ValueError("view_metrics: no views")
    for i, (im, gt) in enumerate(zip(images, gts)):
        L.require_gpu_tensor(im, f"images[{i}]")
        L.require_gpu_tensor(gt, f"gts[{i}]")
    dev = images[0].device
    if any(t.device != dev for t in images + gts):
        raise ValueError("view_metrics: every image and ground truth must be on one device")
    lib = L.load()
    with L.device_guard(dev):
        ims = [_as_chw(t, "an image") for t in images]
        gs = [_as_chw(t, "a ground truth") for t in gts]
        V = len(ims)
        table = (L.MetricView * V)()
        for v, (im, gt) in enumerate(zip(ims, gs)):
            if im.shape[0] != 1:
                raise ValueError(f"view_metrics: images[{v}] must have one channel (got {im.shape[0]})")
            if im.shape[1:] != gt.shape[1:]:
                raise ValueError(f"view_metrics: view {v}: image {tuple(im.shape)} and ground truth {tuple(gt.shape)} "
                                 "differ in height or width")
            H, W = int(im.shape[1]), int(im.shape[2])
            table[v] = L.MetricView(im.data_ptr() if im.numel() else None, gt.data_ptr() if gt.numel() else None,
                                    int(gt.shape[0]), H, W, W // 2 if half_width else 0)
        ws = torch.empty(int(lib.cgs_view_metrics_workspace_bytes(V)), dtype=torch.uint8, device=dev)
        sums = torch.empty(V, 2, dtype=torch.float64, device=dev)
        means = torch.empty(V, 2, dtype=torch.float64, device=dev)
        rc = lib.cgs_view_metrics(V, C.cast(table, C.c_void_p), L.ptr(ws), L.ptr(sums), L.ptr(means), L.raw_stream(dev))
        L.check(rc, "cgs_view_metrics")
    # (converted copies and the workspace go back to the caching allocator on this stream: reuse is stream-ordered)
    return means[:, 0], means[:, 1]


def psnr_from_mse(mse):
    """20 log10(1 / sqrt(mse)) in float64 (utils/image_utils.py:17-19); mse = 0 -> inf."""
    mse = float(mse)
    if mse == 0.0:
        return math.inf
    return 20.0 * math.log10(1.0 / math.sqrt(mse))


def _summarise(images, gts, half_width):
    l1, mse = view_metrics(images, gts, half_width)
    host = torch.stack([l1, mse], 1).cpu().tolist()        # the one readback for all views
    n = len(host)
    return {"l1": sum(r[0] for r in host) / n, "psnr": sum(psnr_from_mse(r[1]) for r in host) / n, "views": n}


def evaluate_views(cameras, gaussians, pipe, bg, use_trained_exp=False, half_width=False):
    """Renders every camera under ``no_grad`` with the reference's report arguments (scaling_modifier = 1, no mask) and
    returns ``{"l1": mean per-view L1, "psnr": mean per-view PSNR, "views": V}`` against ``camera.original_image``.
    ``half_width``: compare the right halves only (``train_test_exp``).  The renders are reduced by one
    ``view_metrics`` launch; the host reads the results once.  Reads no random state and changes nothing a train step
    reads."""
    from .gaussian_renderer import render
    cameras = list(cameras)
    if not cameras:
        return {"l1": 0.0, "psnr": 0.0, "views": 0}
    images, gts = [], []
    with torch.no_grad():
        for cam in cameras:
            pkg = render(cam, gaussians, pipe, bg, scaling_modifier=1.0, use_trained_exp=use_trained_exp, use_mask=False,
                         compute_visibility=False, compute_rend_dir=False)
            images.append(pkg["render"])
            gts.append(cam.original_image.to(pkg["render"].device))
        return _summarise(images, gts, half_width)


def report_configs(scene):
    """The validation configs of training_report (train.py:332-333) without the empty ones: ("test", the test cameras),
    ("train", train cameras idx % n for idx in 5, 10, 15, 20, 25)."""
    train = scene.getTrainCameras()
    configs = (("test", list(scene.getTestCameras())),
               ("train", [train[idx % len(train)] for idx in range(5, 30, 5)] if len(train) else []))
    return [(name, cams) for name, cams in configs if cams]


def training_report(tb_writer, iteration, Ll1, loss, l1_loss, elapsed, testing_iterations, scene, renderFunc, renderArgs,
                    train_test_exp):
    """train.py:321-376 with the same signature.  At ``testing_iterations`` it evaluates the ``test`` config
    (``scene.getTestCameras()``) and the ``train`` config (train cameras ``idx % n`` for idx in 5, 10, .., 25), skips
    empty configs, prints the reference's line and returns ``{name: {"l1", "psnr"}}`` (``{}`` at other iterations).
    Each view is rendered with ``renderFunc(viewpoint, scene.gaussians, *renderArgs)`` under ``no_grad``; the metric
    arithmetic is view_metrics' kernel, so ``l1_loss`` is accepted for the signature and never called.  With a
    ``tb_writer`` the reference's scalar tags are written; its image summaries are not."""
    if tb_writer:
        tb_writer.add_scalar('train_loss_patches/l1_loss', Ll1.item(), iteration)
        tb_writer.add_scalar('train_loss_patches/total_loss', loss.item(), iteration)
        tb_writer.add_scalar('iter_time', elapsed, iteration)
        tb_writer.add_scalar('total_points', scene.gaussians.get_xyz.shape[0], iteration)
    out = {}
    if iteration not in testing_iterations:
        return out
    for name, cams in report_configs(scene):
        images, gts = [], []
        with torch.no_grad():
            for viewpoint in cams:
                img = renderFunc(viewpoint, scene.gaussians, *renderArgs)["render"]
                images.append(img)
                gts.append(viewpoint.original_image.to(img.device))
            res = _summarise(images, gts, train_test_exp)
        print("\n[ITER {}] Evaluating {}: L1 {} PSNR {}".format(iteration, name, res["l1"], res["psnr"]))
        if tb_writer:
            tb_writer.add_scalar(name + '/loss_viewpoint - l1_loss', res["l1"], iteration)
            tb_writer.add_scalar(name + '/loss_viewpoint - psnr', res["psnr"], iteration)
        out[name] = {"l1": res["l1"], "psnr": res["psnr"]}
    return out
