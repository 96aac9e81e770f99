"""GPU: the tile compositors (k_render_fwd3, k_render_bwd3, k_render_bwd_unit) against the float64 truth of
tests/raster_ref64.py, element by element within its per-element bounds -- no outlier fraction, no tile-cluster allowance --
on scenes constructed to sit on every list-length edge of the kernels, through the public operator in both binning layouts.

Prints the worst ratio |hip - truth| / bound per tensor and instance (pytest -s); a ratio of 1 is the bound (K = raster_ref64.K,
fixed on the CPU from the C oracle)."""
import functools
import os

import numpy as np
import pytest
import torch

import raster_ref64 as R64
import util
from util import carve_offsets, hip_settings

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

C, CD, CA, CDA = (True, False, False), (True, True, False), (True, False, True), (True, True, True)
# (label, scene variant, upstream gradients, render_geo, colour_grad, OPT_GENERAL_BACKWARD)
INSTANCES = [
    ("colour", "base", C, True, True, False),
    ("colour+invdepth", "base", CD, True, True, False),
    ("colour+all_map", "base", CA, True, True, False),
    ("all three", "base", CDA, True, True, False),
    ("no geo", "base", CD, False, True, False),
    ("reference call (unit)", "unit", C, True, False, False),
    ("reference call, general backward", "unit", C, True, False, True),
    ("one non-unit colour", "nonunit", C, True, False, False),
]


def _forward_stats():
    import ctypes
    from curve_gaussian_amd import _lib
    r, m, p = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int()
    _lib.load().cgs_last_forward_stats(ctypes.byref(r), ctypes.byref(m), ctypes.byref(p))
    return r.value, m.value, p.value


def run_operator(sp, cam, bg, grads, render_geo, colour_grad, options):
    """GaussianRasterizer as test_raster_gpu.run_hip drives it, plus the saved image state of the forward."""
    from curve_gaussian_amd.diff_cur_rasterization import GaussianRasterizer
    dev = torch.device(DEV)
    ins = {k: v.to(dev).clone().requires_grad_(colour_grad or k != "colors") for k, v in sp.items()}
    P = sp["means3D"].shape[0]
    H, W = cam.image_height, cam.image_width
    m2d = torch.zeros(P, 3, device=dev, requires_grad=True)
    prev, util.OPTIONS[0] = util.OPTIONS[0], util.OPTIONS[0] | options
    try:
        rast = GaussianRasterizer(hip_settings(cam, bg, dev, render_geo, False, 1.0, 0, False))
    finally:
        util.OPTIONS[0] = prev
    color, radii, invd, amap = rast(means3D=ins["means3D"], means2D=m2d, opacities=ins["opacities"],
                                    all_map=ins["all_map"] if render_geo else None, scales=ins["scales"],
                                    rotations=ins["rotations"], colors_precomp=ins["colors"])
    layout = _forward_stats()[2]
    img = color.grad_fn.saved_tensors[-1]      # imgBuffer: final_T [H W], n_contrib [H W], ... (csrc/common.h carve order)
    o = carve_offsets(img.data_ptr(), [(H * W, 4), (H * W, 4)])
    word = img[o[1]:o[1] + H * W * 4].cpu().numpy().view(np.uint32).reshape(H, W)
    out = dict(color=color.detach().cpu().numpy(), radii=radii.cpu().numpy(), invdepth=invd.detach().cpu().numpy(),
               all_map=amap.detach().cpu().numpy(), n_contrib=(word & 0x7fffffff).astype(np.int64), terminated=(word >> 31) == 1,
               layout=layout)
    loss = 0
    for o_, d in zip((color, invd, amap), grads):
        if d is not None:
            loss = loss + (o_ * d.to(dev)).sum()
    loss.backward()
    z = lambda t: (t.grad if t.grad is not None else torch.zeros_like(t)).cpu().numpy()
    out["g"] = dict(dL_dmeans3D=z(ins["means3D"]), dL_dmeans2D=z(m2d), dL_dopacity=z(ins["opacities"]),
                    dL_dcolors=z(ins["colors"]), dL_dscales=z(ins["scales"]), dL_drotations=z(ins["rotations"]),
                    dL_dall_map=z(ins["all_map"]))
    torch.cuda.synchronize()
    return out


def ratio(got, ref, bound):
    """worst |got - ref| / bound; an element whose bound is 0 (no pair reaches it) must be an exact zero."""
    got, ref, b = np.asarray(got, np.float64), np.asarray(ref, np.float64), np.asarray(bound, np.float64)
    assert got.shape == ref.shape == b.shape, (got.shape, ref.shape, b.shape)
    assert np.isfinite(got).all()
    err = np.abs(got - ref)
    zero = b == 0
    if (err[zero] != 0).any():
        return np.inf
    return float((err[~zero] / b[~zero]).max()) if (~zero).any() else 0.0


@functools.lru_cache(maxsize=2)
def scene_truth(name):
    return SceneTruth(name)


class SceneTruth:
    """Everything one scene's tests compare against, built once on the CPU."""

    def __init__(self, name):
        self.sc = sc = R64.Scene(name)
        base = R64.Truth(sc, sc.sp)
        R64.check_margins(R64.margins(sc, base))
        self.lists = R64.quadrant_lists(sc, base)
        self.J = base.jacobian()
        self.cache = {}

    def get(self, kind, which, render_geo):
        key = (kind, which, render_geo)
        if key not in self.cache:
            sc = self.sc
            t = R64.truth(sc, R64.scene_grads(sc, which), kind, render_geo)
            img_b, g_b = R64.bounds(t, J=self.J)
            self.cache[key] = (t, img_b, g_b, R64.expected_n_contrib(sc, t, self.lists))
        return self.cache[key]


def check_against_truth(label, got, t, img_b, g_b, want_pos, colour_grad, report):
    """Every element within its bound; decisions exact.  Appends (label, tensor, ratio) to report; returns the failures."""
    bad = []
    assert (got["radii"] == t.radii).all(), f"{label}: radii"
    term = t.terminated()
    assert (got["terminated"] == term).all(), f"{label}: terminated bit differs at {int((got['terminated'] != term).sum())} pixels"
    cmp = term & (want_pos >= 0)
    assert (got["n_contrib"][cmp] == want_pos[cmp]).all(), f"{label}: n_contrib of terminated pixels"
    for k in ("color", "invdepth", "all_map"):
        r = ratio(got[k], t.out[k], img_b[k])
        report.append((label, k, r))
        if not r <= 1.0:
            bad.append((label, k, r))
    for k, v in got["g"].items():
        if k == "dL_dcolors" and not colour_grad:
            continue
        r = ratio(v, t.g[k], g_b[k])
        report.append((label, k, r))
        if not r <= 1.0:
            bad.append((label, k, r))
    return bad


def _print_report(name, report):
    by = {}
    for label, k, r in report:
        by.setdefault(label, []).append(f"{k.replace('dL_d', 'd')} {r:.3f}")
    for label, items in by.items():
        print(f"   {name} [{label}]: " + " ".join(items))


@pytest.mark.parametrize("name", list(R64.SCENES))
def test_hip_compositors_within_float64_bounds(name):
    """HIP against truth within bounds: every scene, every instance, both binning layouts, every element."""
    from curve_gaussian_amd import _lib
    from curve_gaussian_amd.diff_cur_rasterization import OPT_GENERAL_BACKWARD
    st = scene_truth(name)
    sc = st.sc
    report, bad = [], []
    for label, kind, which, render_geo, colour_grad, general in INSTANCES:
        t, img_b, g_b, want_pos = st.get(kind, which, render_geo)
        sp = R64.variant(sc, kind)
        grads = R64.scene_grads(sc, which)
        _lib.load().cgs_reset_binning_hints()
        for layout, lname in ((0, "exact"), (1, "bucket")):      # first call after the reset: exact; the next: bucket
            got = run_operator(sp, sc.cam, sc.bg, grads, render_geo, colour_grad, OPT_GENERAL_BACKWARD if general else 0)
            assert got["layout"] == layout, (label, lname, got["layout"])
            bad += check_against_truth(f"{label}, {lname}", got, t, img_b, g_b, want_pos, colour_grad, report)
    print()
    _print_report(name, report)
    assert not bad, f"{name}: outside the float64 bounds (ratio > 1): " + "; ".join(f"[{l}] {k} {r:.2f}" for l, k, r in bad)


@pytest.mark.parametrize("name", list(R64.SCENES))
def test_reference_binary_within_the_same_bounds(name):
    """The reference's own kernels (float32 atomics) on the same scenes, held to the same bounds: K is not too tight for
    float32.  Skips where oracle/_ref does not hold the reference binary."""
    from oracle import ref_raster as REF
    if not os.path.exists(os.environ.get("REF_RASTER_LIB", REF.REF_RASTER_SO)):
        pytest.skip("the reference binary is not built here")
    st = scene_truth(name)
    sc = st.sc
    d = lambda v: v.detach().to(DEV)
    report, bad = [], []
    for label, kind, which in (("all three", "base", CDA), ("reference call (unit)", "unit", C)):
        t, img_b, g_b, _ = st.get(kind, which, True)
        sp = R64.variant(sc, kind)
        grads = R64.scene_grads(sc, which)
        fw = REF.forward(d(sc.bg), d(sp["means3D"]), d(sp["colors"]), d(sp["opacities"]), d(sp["scales"]), d(sp["rotations"]), 1.0,
                         None, d(sp["all_map"]), d(sc.cam.world_view_transform), d(sc.cam.full_proj_transform), sc.tfx, sc.tfy,
                         sc.H, sc.W, None, 0, d(sc.cam.camera_center), antialiasing=False, render_geo=True)
        g = REF.backward(fw, *grads)
        torch.cuda.synchronize()
        assert (fw.radii.cpu().numpy() == t.radii).all()
        for k, v in (("color", fw.color), ("invdepth", fw.invdepth), ("all_map", fw.out_all_map)):
            r = ratio(v.cpu().numpy(), t.out[k], img_b[k])
            report.append((label, k, r))
            bad += [(label, k, r)] if not r <= 1.0 else []
        for k in t.g:
            r = ratio(g[k].cpu().numpy().reshape(t.g[k].shape), t.g[k], g_b[k])
            report.append((label, k, r))
            bad += [(label, k, r)] if not r <= 1.0 else []
        fw.free()
    print()
    _print_report(name + " (reference binary)", report)
    assert not bad, f"{name}: the reference binary is outside the bounds: " + "; ".join(f"[{l}] {k} {r:.2f}" for l, k, r in bad)
