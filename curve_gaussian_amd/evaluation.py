"""Held-out evaluation of the training loop (reference train.py:321-376, ``training_report``).

``view_metrics``     per-view L1 and MSE of clamped renders against their edge maps: ONE HIP launch for any number of
                     views (csrc/metrics.hip), float64 results that stay on the device.
``evaluate_views``   renders cameras forward-only through ``gaussian_renderer.render`` (the fused route for a
                     ``GaussianCurveModel`` under default flags) and reduces them with one ``view_metrics`` call and one
                     host readback.
``report_panels``    the report's image summaries (train.py:346-364) as packed 8-bit panels: render, ground truth,
                     turbo-coloured depth, normalised direction map, alpha -- TWO HIP launches for any number of views
                     (csrc/report.hip), nothing read back.
``training_report``  drop-in for the reference's function of the same signature, image summaries included.
``ReportDirWriter``  a summary writer that needs no tensorboard: PNG files and a scalars.jsonl under one directory.

Arithmetic: the reference adds ``l1_loss(image, gt).mean().double()`` and ``psnr(image, gt).mean().double()`` over the
views (float32 means, PSNR = 20 log10(1 / sqrt(mse))) and divides by the number of views.  Here the per-view sums are
float64 (kernel), the PSNR of each view is taken in float64 from its MSE, and the report is the mean of the per-view
values -- not the PSNR of the mean MSE.  An exact match (mse = 0) gives inf, as in the reference."""
import ctypes as C
import json
import math
import os

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


PANELS = L.REPORT_PANELS   # ("render", "ground_truth", "depth", "rend_dir", "rend_alpha"): the panel order


def _panel_input(t, what, channels, dev):
    """A [C,H,W] (or [H,W]) floating-point GPU tensor on `dev` as contiguous float32, C among `channels`."""
    L.require_gpu_tensor(t, what)
    if t.device != dev:
        raise ValueError("report_panels: every map and ground truth must be on one device")
    if not t.is_floating_point():
        raise ValueError(f"report_panels: {what} must be a floating-point tensor (got {t.dtype})")
    if t.dim() == 2:
        t = t.unsqueeze(0)
    if t.dim() != 3 or t.shape[0] not in channels:
        raise ValueError(f"report_panels: {what} must be [C,H,W] with C in {tuple(channels)} (got shape {tuple(t.shape)})")
    return t.detach().float().contiguous()


def report_panels(pkgs, gts=None):
    """The image summaries of training_report (train.py:346-364) for any number of views, on the device.

    pkgs: ``render()`` result dicts; ``render``, ``depth`` and ``rend_alpha`` ([1,H,W]) are required, ``rend_dir``
    ([3,H,W]) may be None or absent (``render(compute_rend_dir=False)``).  gts: None, or one entry per view, each None or
    [Cg,H,W] with Cg 1 or 3.  Views may differ in size.  Returns ``(panels, written)``: per view a uint8 device tensor
    [5,H,W,3] in the order of ``PANELS`` and a 5-tuple of bools; a panel whose input is missing is not written (its bytes
    are whatever the allocator handed out) and its flag is False.

    Per pixel, float32 (include/curvegs.h has the exact order of operations), with q(x) = uint8(clip(x * 255, 0, 255)),
    which is what tensorboard's ``summary.image`` does to a float image:
      render / ground_truth / rend_alpha   q(clamp(x, 0, 1)), one channel replicated to RGB.  The reference hands
                   ``rend_alpha`` over unclamped; the summary writer's quantiser clips, so the bytes are the same.
      depth        turbo[min(int(depth / max(depth) * 256), 255)], the table matplotlib's "turbo" is; black where the
                   view's maximum is 0 and at NaN pixels (which the maximum skips).  The reference draws a 300-dpi
                   matplotlib figure with axes and a colour bar instead; the panel here is the camera's own pixel grid
                   (DESIGN section 6).
      rend_dir     q(F.normalize(rend_dir, dim=0) * 0.5 + 0.5).
    Two launches per ``_lib.REPORT_MAX_VIEWS`` views on the current stream, no synchronisation, no readback."""
    pkgs = list(pkgs)
    gts = [None] * len(pkgs) if gts is None else list(gts)
    if len(pkgs) != len(gts):
        raise ValueError(f"report_panels: {len(pkgs)} views but {len(gts)} ground truths")
    if not pkgs:
        raise ValueError("report_panels: no views")
    for v, pkg in enumerate(pkgs):
        for key in ("render", "depth", "rend_alpha"):
            if pkg.get(key) is None:
                raise ValueError(f"report_panels: pkgs[{v}] has no {key!r}")
    L.require_gpu_tensor(pkgs[0]["render"], "pkgs[0]['render']")
    dev = pkgs[0]["render"].device
    lib = L.load()
    with L.device_guard(dev):
        rows, offset = [], 0
        for v, (pkg, gt) in enumerate(zip(pkgs, gts)):
            maps = [_panel_input(pkg["render"], f"pkgs[{v}]['render']", (1,), dev),
                    None if gt is None else _panel_input(gt, f"gts[{v}]", (1, 3), dev),
                    _panel_input(pkg["depth"], f"pkgs[{v}]['depth']", (1,), dev),
                    None if pkg.get("rend_dir") is None else _panel_input(pkg["rend_dir"], f"pkgs[{v}]['rend_dir']", (3,), dev),
                    _panel_input(pkg["rend_alpha"], f"pkgs[{v}]['rend_alpha']", (1,), dev)]
            H, W = int(maps[0].shape[1]), int(maps[0].shape[2])
            if H == 0 or W == 0:
                raise ValueError(f"report_panels: view {v} is empty ({H} x {W})")
            for m, name in zip(maps, PANELS):
                if m is not None and tuple(m.shape[1:]) != (H, W):
                    raise ValueError(f"report_panels: view {v}: {name} {tuple(m.shape)} and render {tuple(maps[0].shape)} "
                                     "differ in height or width")
            rows.append((maps, H, W, offset))
            offset += (len(PANELS) * H * W * 3 + 15) & ~15      # every view's block starts 16-byte aligned
        out = torch.empty(offset, dtype=torch.uint8, device=dev)
        stream = L.raw_stream(dev)
        written = []
        for first in range(0, len(rows), L.REPORT_MAX_VIEWS):
            chunk = rows[first:first + L.REPORT_MAX_VIEWS]
            table = (L.ReportView * len(chunk))()
            for k, (maps, H, W, off) in enumerate(chunk):
                table[k] = L.ReportView(*[None if m is None else m.data_ptr() for m in maps],
                                        1 if maps[1] is None else int(maps[1].shape[0]), H, W, 0, off)
            ws = torch.empty(int(lib.cgs_report_panels_workspace_bytes(len(chunk))), dtype=torch.uint8, device=dev)
            rc = lib.cgs_report_panels(len(chunk), C.cast(table, C.c_void_p), L.ptr(ws), L.ptr(out), stream)
            L.check(rc, "cgs_report_panels")
            written += [tuple(bool(table[k].written >> p & 1) for p in range(len(PANELS))) for k in range(len(chunk))]
    # (converted copies and the workspace go back to the caching allocator on this stream: reuse is stream-ordered)
    panels = [out[off:off + len(PANELS) * H * W * 3].view(len(PANELS), H, W, 3) for _maps, H, W, off in rows]
    return panels, written


class ReportDirWriter:
    """The two methods of a tensorboard ``SummaryWriter`` that training_report uses, writing plain files under `path`:
    ``add_images`` saves ``images/iter_{step:06d}/{tag with '/' -> '__'}.png`` (image k > 0 of a batch gets ``_{k}`` before
    the suffix), ``add_scalar`` appends ``{"tag", "value", "step"}`` lines to ``scalars.jsonl``."""

    def __init__(self, path):
        self.path = str(path)
        os.makedirs(self.path, exist_ok=True)

    def add_scalar(self, tag, scalar_value, global_step=None):
        with open(os.path.join(self.path, "scalars.jsonl"), "a") as f:
            f.write(json.dumps({"tag": tag, "value": float(scalar_value), "step": global_step}) + "\n")

    def add_images(self, tag, img_tensor, global_step=None, dataformats="NCHW"):
        """img_tensor: uint8 [N,H,W,C] with ``dataformats="NHWC"``, C 1 or 3 -- what training_report passes."""
        import numpy as np
        from PIL import Image
        a = img_tensor.detach().cpu().numpy() if isinstance(img_tensor, torch.Tensor) else np.asarray(img_tensor)
        if dataformats != "NHWC" or a.dtype != np.uint8 or a.ndim != 4 or a.shape[3] not in (1, 3):
            raise ValueError(f"ReportDirWriter.add_images: expected uint8 [N,H,W,1 or 3] with dataformats='NHWC' (got "
                             f"{a.dtype} {a.shape}, dataformats={dataformats!r})")
        folder = os.path.join(self.path, "images", "iter_%06d" % int(global_step or 0))
        os.makedirs(folder, exist_ok=True)
        name = tag.replace("/", "__")
        for k, im in enumerate(a):
            im = np.ascontiguousarray(im[:, :, 0] if im.shape[2] == 1 else im)
            Image.fromarray(im).save(os.path.join(folder, name + ("" if k == 0 else f"_{k}") + ".png"))


REPORT_IMAGE_VIEWS = 5   # train.py:346: `idx < 5`


def _write_image_summaries(tb_writer, name, views, pkgs, gts, iteration, train_test_exp):
    """train.py:346-364 for the first views of one config: one report_panels call, then the reference's tags in the
    reference's order.  `gts` is None except at the first test iteration (:348)."""
    panels, written = report_panels(pkgs, gts)
    for viewpoint, panel, flags in zip(views, panels, written):
        half = panel.shape[2] // 2 if train_test_exp else 0    # (:343-345) render and ground truth: the right half
        for p, kind in enumerate(PANELS):
            if flags[p]:
                img = panel[p, :, half:] if p < 2 else panel[p]
                tb_writer.add_images(f"{name}_view_{viewpoint.image_name}/{kind}", img[None], global_step=iteration,
                                     dataformats="NHWC")


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
    arithmetic is view_metrics' kernel, so ``l1_loss`` is accepted for the signature and never called.

    With a ``tb_writer`` (a tensorboard ``SummaryWriter``, a ``ReportDirWriter``, anything with ``add_scalar``) the
    reference's scalar tags are written; ``Ll1``, ``loss`` and ``elapsed`` may be None, and their tags are then left out
    (the driver has no separate L1 term or iteration time to give).  A writer that also has ``add_images`` receives the
    reference's image summaries (:346-364) for the first five views of each config: ``{config}_view_{image_name}/render``,
    ``/ground_truth`` (at ``testing_iterations[0]`` only), ``/depth``, ``/rend_dir``, ``/rend_alpha``, each one
    ``add_images(tag, panel[None], global_step=iteration, dataformats="NHWC")`` with a uint8 [H,W,3] panel of
    ``report_panels`` -- one call of it per config; ``/rend_dir`` is left out when the render function returns none.  With
    ``train_test_exp`` the render and ground-truth panels are their right halves, as upstream.  The metrics, the printed
    line and the return value do not depend on the writer."""
    if tb_writer:
        if Ll1 is not None:
            tb_writer.add_scalar('train_loss_patches/l1_loss', Ll1.item(), iteration)
        if loss is not None:
            tb_writer.add_scalar('train_loss_patches/total_loss', loss.item(), iteration)
        if elapsed is not None:
            tb_writer.add_scalar('iter_time', elapsed, iteration)
        tb_writer.add_scalar('total_points', scene.gaussians.get_xyz.shape[0], iteration)
    out = {}
    if iteration not in testing_iterations:
        return out
    want_images = bool(tb_writer) and hasattr(tb_writer, "add_images")
    first_report = iteration == list(testing_iterations)[0]
    for name, cams in report_configs(scene):
        images, gts, shown = [], [], []
        with torch.no_grad():
            for idx, viewpoint in enumerate(cams):
                pkg = renderFunc(viewpoint, scene.gaussians, *renderArgs)
                img = pkg["render"]
                images.append(img)
                gts.append(viewpoint.original_image.to(img.device))
                if want_images and idx < REPORT_IMAGE_VIEWS:
                    shown.append(pkg)
            if shown:
                _write_image_summaries(tb_writer, name, cams[:len(shown)], shown, gts[:len(shown)] if first_report else None,
                                       iteration, train_test_exp)
            res = _summarise(images, gts, train_test_exp)
        print("\n[ITER {}] Evaluating {}: L1 {} PSNR {}".format(iteration, name, res["l1"], res["psnr"]))
        if tb_writer:
            tb_writer.add_scalar(name + '/loss_viewpoint - l1_loss', res["l1"], iteration)
            tb_writer.add_scalar(name + '/loss_viewpoint - psnr', res["psnr"], iteration)
        out[name] = {"l1": res["l1"], "psnr": res["psnr"]}
    return out
