"""GPU: the per-splat kernels' options (k_preprocess_fwd / k_preprocess_bwd: spherical-harmonic colours at degrees 0 .. 3,
antialiasing, cov3D_precomp, scale_modifier) against the float64 truth of tests/raster_ref64.py ("Options"), element by
element within its per-element bounds: every image element outside the scene's undecided pixels and every element of every
gradient, dL_dsh (in the operator's layout) and dL_dcov3D included; an element whose bound is 0 (a culled
splat's row, a clamped colour's coefficients, coefficients beyond the active degree, a splat antialiased below the 1/255 cut)
must be an exact zero.  No outlier fraction, no retry.  Every option set of raster_ref64.OPTION_SETS runs through the public
operator on the first call after cgs_reset_binning_hints() (exact layout) and on the second (buckets), each with a second
backward over the same forward state; sh3_aa_mod17 also through the `_C` binding; the reference binary, where it is built,
is held to the same bounds.

The constants are fixed on the CPU from the C oracle (test_splat_options_ref64_cpu.py), never from a run of this module.
Measured on an MI355X, worst ratio |got - truth| / bound over all tensors and both calls (HIP | the reference binary):
    sh0 0.311 | 0.257            sh1 0.243 | 0.253     sh2 0.284 | 0.132          sh3 0.493 | 0.278
    sh1_m16 0.126 | 0.132        aa 0.051 | 0.049      cov 0.228 | 0.190          mod05 0.626 | 0.555
    mod17 0.135 | 0.134          sh3_aa_mod17 0.144 | 0.142 (`_C` binding 0.144)  cov_aa_sh2 0.134 | 0.122
    nogeo_sh3 0.208 | 0.197
No kernel was found outside a bound: csrc/splat_math.h and csrc/preprocess.hip are unchanged.
"""
import functools
import os

import numpy as np
import pytest
import torch

import raster_ref64 as R64
from test_raster_ref64_gpu import _forward_stats, _print_report, ratio
from util import hip_settings

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ALL = (True, True, True)
IMAGES = ("color", "invdepth", "all_map")


@functools.lru_cache(maxsize=2)
def option_truth(name):
    """(scene, undecided pixels, upstream gradients, truth, image bounds, gradient bounds) of an option set, built once."""
    sc = R64.option_scene(name)
    mask = R64.undecided_pixels(sc, R64.Truth(sc, sc.sp, None, sc.render_geo, sc.opt))
    R64.check_mask(sc, mask)
    grads = R64.scene_grads(sc, ALL, mask)
    t = R64.Truth(sc, sc.sp, grads, sc.render_geo, sc.opt)
    R64.check_margins(R64.margins(sc, t, mask=mask))
    R64.option_edges(sc, t)
    img_b, g_b = R64.bounds(t)
    return sc, mask, grads, t, img_b, g_b


def compared(sc, t):
    return [k for k in t.g if not (k == "dL_dcolors" and sc.opt.sh is not None)]


def check(label, sc, mask, t, img_b, g_b, got, report):
    """Appends (label, tensor, ratio) for every image and gradient tensor of `got`."""
    keep = ~mask
    assert (got["radii"] == t.radii).all(), f"{label}: radii"
    for k in IMAGES:
        report.append((label, k, ratio(got[k][:, keep], t.out[k][:, keep], img_b[k][:, keep])))
    for k in compared(sc, t):
        report.append((label, k, ratio(np.asarray(got["g"][k]).reshape(t.g[k].shape), t.g[k], g_b[k])))


def _finish(name, report):
    print()
    _print_report(name, report)
    print(f"   {name}: worst ratio {max(r for _, _, r in report):.3f}")
    bad = [x for x in report if not x[2] <= 1.0]
    assert not bad, f"{name}: outside the float64 bounds (ratio > 1): " + "; ".join(f"[{l}] {k} {r:.2f}" for l, k, r in bad)


def run_operator(sc, grads):
    """GaussianRasterizer with the scene's options: the images, the layout of the forward and the gradients of two
    backwards over the one forward state."""
    from curve_gaussian_amd.diff_cur_rasterization import GaussianRasterizer
    o = sc.opt
    dev = torch.device(DEV)
    leaf = lambda v: v.to(dev).clone().requires_grad_(True)
    ins = {k: leaf(v) for k, v in sc.sp.items()}
    ins["means2D"] = torch.zeros(sc.P, 3, device=dev, requires_grad=True)
    rast = GaussianRasterizer(hip_settings(sc.cam, sc.bg, dev, sc.render_geo, o.antialiasing, o.scale_modifier, o.degree, False))
    kw = dict(means3D=ins["means3D"], means2D=ins["means2D"], opacities=ins["opacities"],
              all_map=ins["all_map"] if sc.render_geo else None)
    if o.cov3D is not None:
        ins["cov3D"] = leaf(o.cov3D)
        kw["cov3D_precomp"] = ins["cov3D"]
        del ins["scales"], ins["rotations"]
    else:
        kw["scales"], kw["rotations"] = ins["scales"], ins["rotations"]
    if o.sh is not None:
        ins["sh"] = leaf(o.sh.unsqueeze(2))          # get_features' layout [P, M, 1]
        kw["shs"] = ins["sh"]
        del ins["colors"]
    else:
        kw["colors_precomp"] = ins["colors"]
    if not sc.render_geo:
        del ins["all_map"]
    color, radii, invd, amap = rast(**kw)
    out = dict(color=color.detach().cpu().numpy(), radii=radii.cpu().numpy(), invdepth=invd.detach().cpu().numpy(),
               all_map=amap.detach().cpu().numpy(), layout=_forward_stats()[2])
    loss = sum((o_ * d.to(dev)).sum() for o_, d in zip((color, invd, amap), grads))
    names = list(ins)
    key = dict(means3D="dL_dmeans3D", means2D="dL_dmeans2D", opacities="dL_dopacity", colors="dL_dcolors", scales="dL_dscales",
               rotations="dL_drotations", all_map="dL_dall_map", sh="dL_dsh", cov3D="dL_dcov3D")
    out["backwards"] = []
    for again in (True, False):
        gs = torch.autograd.grad(loss, [ins[k] for k in names], retain_graph=again, allow_unused=True)
        g = {key[k]: (torch.zeros_like(ins[k]) if v is None else v).cpu().numpy() for k, v in zip(names, gs)}
        for k, shape in (("dL_dscales", (sc.P, 3)), ("dL_drotations", (sc.P, 4)), ("dL_dall_map", (sc.P, 4))):
            g.setdefault(k, np.zeros(shape, np.float32))     # an input the call does not have: no gradient
        out["backwards"].append(g)
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("name", list(R64.OPTION_SETS))
def test_hip_options_within_float64_bounds(name):
    """The public operator on every option set: first call after the reset (exact layout), second call (buckets), two
    backwards each; every element within its bound."""
    from curve_gaussian_amd import _lib
    sc, mask, grads, t, img_b, g_b = option_truth(name)
    report = []
    _lib.load().cgs_reset_binning_hints()
    try:
        for layout, lname in ((0, "exact"), (1, "second call")):
            got = run_operator(sc, grads)
            assert got["layout"] == layout, (lname, got["layout"])
            for i, g in enumerate(got["backwards"]):
                check(f"{lname}, backward {i + 1}", sc, mask, t, img_b, g_b, dict(got, g=g), report)
    finally:
        _lib.load().cgs_reset_binning_hints()
    _finish(sc.name, report)


def test_shim_binding_with_sh3_antialiasing_and_scale_modifier():
    """Degree 3 + antialiasing + scale_modifier 1.7 through the `_C` binding (rasterize_gaussians, then
    rasterize_gaussians_backward on its buffers), as test_raster_ref64_gpu.test_random_scenes_within_float64_bounds drives it."""
    from curve_gaussian_amd import _lib
    from curve_gaussian_amd.diff_cur_rasterization import _C
    sc, mask, grads, t, img_b, g_b = option_truth("sh3_aa_mod17")
    o = sc.opt
    dev = torch.device(DEV)
    rs = hip_settings(sc.cam, sc.bg, dev, True, True, o.scale_modifier, o.degree, False)
    d = {k: v.to(dev) for k, v in sc.sp.items()}
    sh = o.sh.unsqueeze(2).contiguous().to(dev)
    g = [x.to(dev).contiguous() for x in grads]
    e = torch.empty(0, device=dev)
    n = lambda x: x.detach().cpu().numpy()
    report = []
    _lib.load().cgs_reset_binning_hints()
    try:
        for label in ("1st forward", "2nd forward"):
            (R, color, radii, gB, bB, iB, invd, amap) = _C.rasterize_gaussians(
                rs.bg, d["means3D"], e, d["opacities"], d["scales"], d["rotations"], o.scale_modifier, e, d["all_map"], rs.viewmatrix,
                rs.projmatrix, rs.tanfovx, rs.tanfovy, sc.H, sc.W, sh, o.degree, rs.campos, False, True, True, False)
            (g_m2d, _, g_op, g_m3d, _, g_sh, g_sc, g_rot, g_amap) = _C.rasterize_gaussians_backward(
                rs.bg, e, d["means3D"], radii, e, d["all_map"], d["opacities"], d["scales"], d["rotations"], o.scale_modifier, e,
                rs.viewmatrix, rs.projmatrix, rs.tanfovx, rs.tanfovy, g[0], g[1], g[2], sh, o.degree, rs.campos, gB, R, bB, iB, True, True,
                False)
            torch.cuda.synchronize()
            assert tuple(g_sh.shape) == (sc.P, o.sh.shape[1], 3)
            got = dict(color=n(color), radii=n(radii), invdepth=n(invd), all_map=n(amap),
                       g=dict(dL_dmeans3D=n(g_m3d), dL_dmeans2D=n(g_m2d), dL_dopacity=n(g_op), dL_dscales=n(g_sc), dL_drotations=n(g_rot),
                              dL_dall_map=n(g_amap), dL_dsh=n(g_sh).sum(-1)))      # (autograd's sum onto the [P, M, 1] input)
            check(label, sc, mask, t, img_b, g_b, got, report)
    finally:
        _lib.load().cgs_reset_binning_hints()
    _finish(sc.name + " (_C binding)", report)


@pytest.mark.parametrize("name", list(R64.OPTION_SETS))
def test_reference_binary_options_within_the_same_bounds(name):
    """The reference's own kernels on the same option sets, held to the same bounds: they are not too tight for float32.
    Skips where oracle/_ref does not hold the reference binary."""
    from oracle import ref_raster as REF
    if not os.path.exists(os.environ.get("REF_RASTER_LIB", REF.REF_RASTER_SO)):
        pytest.skip("the reference binary is not built here")
    sc, mask, grads, t, img_b, g_b = option_truth(name)
    o = sc.opt
    d = lambda v: None if v is None else v.detach().to(DEV)
    sp = sc.sp
    has_cov = o.cov3D is not None
    fw = REF.forward(d(sc.bg), d(sp["means3D"]), None if o.sh is not None else d(sp["colors"]), d(sp["opacities"]),
                     None if has_cov else d(sp["scales"]), None if has_cov else d(sp["rotations"]), o.scale_modifier, d(o.cov3D),
                     d(sp["all_map"]), d(sc.cam.world_view_transform), d(sc.cam.full_proj_transform), sc.tfx, sc.tfy, sc.H, sc.W,
                     d(o.sh), o.degree, d(sc.cam.camera_center), antialiasing=o.antialiasing, render_geo=sc.render_geo)
    g = REF.backward(fw, *grads)
    torch.cuda.synchronize()
    n = lambda x: x.detach().cpu().numpy()
    got = dict(color=n(fw.color), radii=n(fw.radii), invdepth=n(fw.invdepth), all_map=n(fw.out_all_map),
               g={k: n(v) for k, v in g.items() if k in t.g})
    if o.sh is not None:
        got["g"]["dL_dsh"] = got["g"]["dL_dsh"].sum(-1)
    report = []
    check("reference binary", sc, mask, t, img_b, g_b, got, report)
    fw.free()
    _finish(sc.name + " (reference binary)", report)
