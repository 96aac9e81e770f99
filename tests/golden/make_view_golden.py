#!/usr/bin/env python
"""Freezes the ORACLE CHAIN of the per-view path -- what bench.py's headline runs: curve tensors -> image -> curve-parameter
gradients -- on three small scenes -> tests/golden/view_{small,lines,masked}.npz.

    chain = oracle/torch_ref.py (prepare_scaling_rot, the straight-through mask and build_all_map of
            gaussian_renderer/__init__.py:72-76,98-104) around oracle/raster_ref.c (K1-K10), gradients pulled back through
            the torch graph in float32.

Like tests/golden/raster_*.npz these files freeze the oracle, they do NOT pin it to the reference (the rasterizer half is
parity-unpinned; the sampling half is pinned through rot_to_quat.npz).  A `-m "not gpu"` test holds
today's chain to the files, a `-m gpu` test holds cgs_view_forward / cgs_view_backward to them.

    python tests/golden/make_view_golden.py          # rewrites the three files (ONLY for a deliberate oracle change)

Scenes: `small` -- Bezier curves only, black background; `lines` -- a third of the curves are straight lines
(is_bezier = False: the line branch of prepare_scaling_rot), grey background; `masked` -- use_mask with mask logits on both
sides of the threshold (gaussian_renderer/__init__.py:72-76) and mixed curve types.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from curve_gaussian_amd import synthetic as S  # noqa: E402
from oracle import raster as ORA  # noqa: E402
from oracle import torch_ref as TR  # noqa: E402
from util import tanfov  # noqa: E402

M = 12
MASK_THR = 0.01


def scenes():
    """name -> (curves dict, mask logits or None, camera, background)."""
    out = {}
    c = S.make_curves(220, 401)
    c["width"] = c["width"] + 0.7
    out["small"] = (c, None, S.make_camera((0.5, -1.7, 0.8), (0.5, 0.5, 0.5), (0, 0, 1), 64, 80), 0.0)
    c = S.make_curves(260, 402)
    g = torch.Generator().manual_seed(402)
    c["width"] = c["width"] + 0.6 + 0.3 * torch.randn(260, 1, generator=g)
    c["is_bezier"] = torch.arange(260) % 3 != 0
    out["lines"] = (c, None, S.make_camera((2.1, 1.2, 1.0), (0.5, 0.5, 0.5), (0, 0, 1), 80, 96), 0.3)
    c = S.make_curves(240, 403)
    g = torch.Generator().manual_seed(403)
    c["width"] = c["width"] + 0.8
    c["is_bezier"] = torch.rand(240, generator=g) > 0.3
    mask = torch.randn(240, M, 1, generator=g) * 3.0 - 3.0   # sigmoid on both sides of 0.01
    out["masked"] = (c, mask, S.make_camera((0.5, -1.6, 1.1), (0.5, 0.5, 0.4), (0, 0, 1), 72, 72), 0.0)
    return out


def chain(curves, mask_logit, cam, bg, dimg, m=M, mask_thr=MASK_THR, pull=torch.float32, opac_scale=1.0, decisions=False):
    """The oracle chain -> dict(color, invdepth, all_map, radii, final_T, g_curve_points, g_width, g_opacity[, g_mask], g_means2D).

    The frozen files are this function under its defaults.  tests/view_ref64.py calls it at other sample counts `m` and with
    `pull=torch.float64`: the compositor still gets the float32 splat tensors, and its per-splat gradients are pulled back
    through a float64 copy of the same torch graph (the mask's on / off decisions are those of the float32 forward).
    `opac_scale` multiplies the splat opacities handed to the compositor and `decisions` adds its per-pixel decisions
    (n_contrib: the last contributor's list position; n_blended: how many list entries were blended) -- both for
    tests/test_view_ref64_cpu.py."""
    def graph(dt, on=None):
        leaves = [curves[k].clone().to(dt).requires_grad_(True) for k in ("curve_points", "width", "opacity")]
        ml = mask_logit.clone().to(dt).requires_grad_(True) if mask_logit is not None else None
        xyz, rot, scl = TR.prepare_scaling_rot(leaves[0], leaves[1], curves["is_bezier"], m)
        rotn = torch.nn.functional.normalize(rot)
        opac = torch.sigmoid(leaves[2]).unsqueeze(1).expand(-1, m, -1).reshape(-1, 1)
        scales = scl
        if ml is not None:   # gaussian_renderer/__init__.py:72-76 (straight-through estimator)
            sg = torch.sigmoid(ml)
            on = (sg > mask_thr) if on is None else on
            mk = (on.to(dt) - sg).detach() + sg
            scales = scl * mk.view(-1, 1)
            opac = opac * mk.view(-1, 1)
        return leaves, ml, xyz, rot, rotn, opac, scales, on
    leaves, ml, xyz, rot, rotn, opac, scales, on = graph(torch.float32)
    P = xyz.shape[0]
    amap = TR.build_all_map(rot.detach(), xyz.detach(), cam.camera_center, cam.world_view_transform).float().contiguous()
    tfx, tfy = tanfov(cam)
    H, W = cam.image_height, cam.image_width
    n = lambda t: np.ascontiguousarray(t.detach().numpy().astype(np.float32))
    opac_in = n(opac) if opac_scale == 1.0 else (n(opac).astype(np.float64) * opac_scale).astype(np.float32)
    fw = ORA.forward(np.full(3, bg, np.float32), n(xyz), np.ones((P, 1), np.float32), opac_in, n(scales), n(rotn), 1.0, None,
                     n(amap), n(cam.world_view_transform), n(cam.full_proj_transform), tfx, tfy, H, W, None, 0,
                     n(cam.camera_center))
    gr = ORA.backward(fw, np.ascontiguousarray(dimg, np.float32), None, None)
    if pull != torch.float32:
        leaves, ml, xyz, rot, rotn, opac, scales, on = graph(pull, on)
    t = lambda a: torch.from_numpy(np.asarray(a, np.float32)).to(pull)
    ((xyz * t(gr["dL_dmeans3D"])).sum() + (scales * t(gr["dL_dscales"])).sum() + (rotn * t(gr["dL_drotations"])).sum()
     + (opac * t(gr["dL_dopacity"])).sum()).backward()
    out = dict(color=fw.color.copy(), invdepth=fw.invdepth.copy(), out_all_map=fw.out_all_map.copy(),
               radii=fw.radii.astype(np.int32), final_T=fw.final_T.copy(), num_rendered=np.array([fw.num_rendered], np.int64),
               g_curve_points=leaves[0].grad.numpy(), g_width=leaves[1].grad.numpy(), g_opacity=leaves[2].grad.numpy(),
               g_means2D=np.asarray(gr["dL_dmeans2D"], np.float32))
    if ml is not None:
        out["g_mask"] = ml.grad.numpy()
    if decisions:
        from util import near_threshold_pairs, pixel_decisions, radius_margin
        out["n_contrib"] = fw.n_contrib.copy()
        out["n_blended"] = pixel_decisions(fw)
        out["near_pairs"] = near_threshold_pairs(fw)
        out["radius_margin"] = radius_margin(fw)
    fw.free()
    return out


def upstream(name, H, W):
    return torch.randn(1, H, W, generator=torch.Generator().manual_seed(2000 + len(name))).numpy().astype(np.float32)


def freeze(name, curves, mask_logit, cam, bg):
    H, W = cam.image_height, cam.image_width
    dimg = upstream(name, H, W)
    res = chain(curves, mask_logit, cam, bg, dimg)
    tfx, tfy = tanfov(cam)
    d = dict(curve_points=curves["curve_points"].numpy(), width=curves["width"].numpy(), opacity=curves["opacity"].numpy(),
             is_bezier=curves["is_bezier"].numpy(), bg=np.array([bg], np.float32), dL_dcolor=dimg,
             viewmatrix=cam.world_view_transform.numpy(), projmatrix=cam.full_proj_transform.numpy(),
             campos=cam.camera_center.numpy(), hw=np.array([H, W], np.int64), FoV=np.array([cam.FoVx, cam.FoVy], np.float64),
             tanfov=np.array([tfx, tfy], np.float64), mask_thr=np.array([MASK_THR], np.float32))
    if mask_logit is not None:
        d["mask"] = mask_logit.numpy()
    d.update(res)
    path = os.path.join(HERE, f"view_{name}.npz")
    np.savez_compressed(path, **d)
    print(f"{name}: B={curves['curve_points'].shape[0]} {W}x{H} R={int(res['num_rendered'][0])} visible={(res['radii'] > 0).sum()} "
          f"lines={int((~curves['is_bezier']).sum())} -> {os.path.getsize(path) / 1024:.0f} KiB")


def load_scene(name):
    """-> (curves dict, mask logits or None, camera, background value, npz)."""
    z = np.load(os.path.join(HERE, f"view_{name}.npz"))
    curves = {k: torch.from_numpy(z[k].copy()) for k in ("curve_points", "width", "opacity", "is_bezier")}
    mask = torch.from_numpy(z["mask"].copy()) if "mask" in z.files else None
    H, W = (int(v) for v in z["hw"])
    cam = S.SynthCamera(H, W, float(z["FoV"][0]), float(z["FoV"][1]), torch.from_numpy(z["viewmatrix"].copy()),
                        torch.from_numpy(z["projmatrix"].copy()), torch.from_numpy(z["campos"].copy()))
    return curves, mask, cam, float(z["bg"][0]), z


if __name__ == "__main__":
    ORA.set_num_threads(1)   # fixed accumulation order of the double-precision per-splat sums
    for name, (curves, mask, cam, bg) in scenes().items():
        freeze(name, curves, mask, cam, bg)
