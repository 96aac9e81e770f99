"""GPU: the tile compositors (k_render_fwd3, k_render_bwd3, k_render_bwd_unit) against the float64 truth of
tests/raster_ref64.py, element by element within its per-element bounds -- no outlier fraction, no tile-cluster allowance --
on scenes constructed to sit on every list-length edge of the kernels, through the public operator in both binning layouts.

Prints the worst ratio |hip - truth| / bound per tensor and instance (pytest -s); a ratio of 1 is the bound (K = raster_ref64.K,
fixed on the CPU from the C oracle).

The long_* scenes (one tile of 1024 .. 9000 entries: the rank sort, the LDS network, the global-memory network, T and the
accumulators carried through up to 36 forward and 71 backward batches, termination in the fifth batch, depth ties), the
turned_* scenes (20 tiles under the turned cameras) and the random scenes of test_random_scenes_within_float64_bounds mask
their undecided pixels (raster_ref64: "Decisions"); every other element is compared, with no outlier fraction and no retry.
Measured on an MI355X at K = 64, worst ratio over all tensors, instances and both calls (HIP | the reference binary):
    long_1024 0.028 | 0.017   long_1025 0.023 | 0.013   long_2048 0.026 | 0.011   long_2049 0.023 | 0.006
    long_4096 0.058 | 0.016   long_4097 0.043 | 0.010   long_9000 0.187 | 0.041   long_term_1100 0.022 | 0.007
    long_ties 0.013 | 0.006   turned_0 0.103 | 0.102    turned_1 0.127 | 0.101    turned_2 0.168 | 0.168
    random seeds 2001 .. 2008 (HIP, worst of the four forward states): 0.075 0.593 0.233 0.063 0.591 0.012 0.024 0.027
(the long scenes' worst is a per-splat gradient of the "all three" instance, the turned and random scenes' an image channel or
dL_dall_map under sub-pixel or thin splats: the float32 per-splat state, see the K section of raster_ref64)."""
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
# the instances of the scenes whose float64 walk takes seconds (raster_ref64.SCENES, instances = "long"): three truths
LONG_INSTANCES = ("all three", "reference call (unit)", "reference call, general backward", "one non-unit colour")


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
    tiles = ((H + 15) // 16) * ((W + 15) // 16)
    o = carve_offsets(img.data_ptr(), [(H * W, 4), (H * W, 4), (tiles, 8)])
    word = img[o[1]:o[1] + H * W * 4].cpu().numpy().view(np.uint32).reshape(H, W)
    ranges = img[o[2]:o[2] + tiles * 8].cpu().numpy().view(np.uint32).reshape(tiles, 2).astype(np.int64)
    out = dict(color=color.detach().cpu().numpy(), radii=radii.cpu().numpy(), invdepth=invd.detach().cpu().numpy(),
               all_map=amap.detach().cpu().numpy(), n_contrib=(word & 0x7fffffff).astype(np.int64), terminated=(word >> 31) == 1,
               layout=layout, list_lens=ranges[:, 1] - ranges[:, 0])
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
        assert not R64.splat_failures(sc.sp, sc.cam, sc.H, sc.W).any()
        self.mask = R64.undecided_pixels(sc, base)      # (empty in the scenes whose table entry allows none: check_mask)
        R64.check_mask(sc, self.mask)
        R64.check_margins(R64.margins(sc, base, mask=self.mask))
        self.lists = R64.quadrant_lists(sc, base)
        self.J = base.jacobian()
        self.cache = {}

    def get(self, kind, which, render_geo):
        key = (kind, which, render_geo)
        if key not in self.cache:
            sc = self.sc
            t = R64.truth(sc, R64.scene_grads(sc, which, self.mask), kind, render_geo)
            img_b, g_b = R64.bounds(t, J=self.J)
            self.cache[key] = (t, img_b, g_b, R64.expected_n_contrib(sc, t, self.lists))
        return self.cache[key]


def check_against_truth(label, got, t, img_b, g_b, want_pos, colour_grad, report, mask=None):
    """Every element within its bound; decisions exact.  Appends (label, tensor, ratio) to report; returns the failures.
    `mask`: the scene's undecided pixels, left out of the image, `terminated` and n_contrib comparisons (their upstream
    gradients are zero: every gradient element is still compared, and one without other pairs must be an exact zero)."""
    bad = []
    keep = np.ones(t.terminated().shape, bool) if mask is None else ~mask
    assert (got["radii"] == t.radii).all(), f"{label}: radii"
    term = t.terminated()
    differs = (got["terminated"] != term) & keep
    assert not differs.any(), f"{label}: terminated bit differs at {int(differs.sum())} pixels"
    cmp = term & (want_pos >= 0) & keep
    assert (got["n_contrib"][cmp] == want_pos[cmp]).all(), f"{label}: n_contrib of terminated pixels"
    for k in ("color", "invdepth", "all_map"):
        r = ratio(got[k][:, keep], t.out[k][:, keep], img_b[k][:, keep])
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
        if sc.instances == "long" and label not in LONG_INSTANCES:
            continue
        t, img_b, g_b, want_pos = st.get(kind, which, render_geo)
        sp = R64.variant(sc, kind)
        grads = R64.scene_grads(sc, which, st.mask)
        _lib.load().cgs_reset_binning_hints()
        # first call after the reset: exact; the next: the layout the scene's table entry names (buckets, unless the list
        # is too long for a bucket)
        for layout, lname in ((0, "exact"), (sc.layout, "second call")):
            got = run_operator(sp, sc.cam, sc.bg, grads, render_geo, colour_grad, OPT_GENERAL_BACKWARD if general else 0)
            assert got["layout"] == layout, (label, lname, got["layout"])
            if sc.list_len is not None:
                assert got["list_lens"].tolist() == [sc.list_len], (label, lname, got["list_lens"])
            bad += check_against_truth(f"{label}, {lname}", got, t, img_b, g_b, want_pos, colour_grad, report, st.mask)
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
        grads = R64.scene_grads(sc, which, st.mask)
        fw = REF.forward(d(sc.bg), d(sp["means3D"]), d(sp["colors"]), d(sp["opacities"]), d(sp["scales"]), d(sp["rotations"]), 1.0,
                         None, d(sp["all_map"]), d(sc.cam.world_view_transform), d(sc.cam.full_proj_transform), sc.tfx, sc.tfy,
                         sc.H, sc.W, None, 0, d(sc.cam.camera_center), antialiasing=False, render_geo=True)
        g = REF.backward(fw, *grads)
        torch.cuda.synchronize()
        assert (fw.radii.cpu().numpy() == t.radii).all()
        for k, v in (("color", fw.color), ("invdepth", fw.invdepth), ("all_map", fw.out_all_map)):
            r = ratio(v.cpu().numpy()[:, ~st.mask], t.out[k][:, ~st.mask], img_b[k][:, ~st.mask])
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


@functools.lru_cache(maxsize=1)
def _random_truth(row):
    sc = R64.random_scene(row)
    base = R64.Truth(sc, sc.sp)
    mask = R64.undecided_pixels(sc, base)
    R64.check_mask(sc, mask)
    R64.check_margins(R64.margins(sc, base, mask=mask))
    grads = R64.scene_grads(sc, CDA, mask)
    t = R64.truth(sc, grads)
    img_b, g_b = R64.bounds(t)
    return sc, mask, grads, t, img_b, g_b


@pytest.mark.parametrize("row", R64.RANDOM_SCENES, ids=lambda r: f"seed{r[0]}")
def test_random_scenes_within_float64_bounds(row):
    """The sibling of test_raster_gpu.test_bucket_path_equals_exact_path_on_random_scenes, on scenes of the same generator:
    the debug forward's state (count -> scan -> scatter -> sort) and each of the three default-forward states (exact layout,
    buckets, buckets with the oversized splats deferred) go through the operator's backward ONCE, and every gradient element
    (and every image element outside the scene's undecided pixels) is held to the float64 truth's bound: no retry, no
    run-to-run noise allowance, no outlier fraction."""
    from curve_gaussian_amd import _lib
    from curve_gaussian_amd.diff_cur_rasterization import _C
    sc, mask, grads, t, img_b, g_b = _random_truth(row)
    dev = torch.device(DEV)
    H, W = sc.H, sc.W
    rs = hip_settings(sc.cam, sc.bg, dev)
    d = {k: v.to(dev) for k, v in sc.sp.items()}
    g = [x.to(dev).contiguous() for x in grads]
    e = torch.empty(0, device=dev)
    keep = ~mask
    report, bad = [], []
    _lib.load().cgs_reset_binning_hints()
    try:
        for label, debug in (("debug forward", True), ("1st default forward", False), ("2nd default forward", False),
                             ("3rd default forward", False)):
            (R, color, radii, gB, bB, iB, invd, amap) = _C.rasterize_gaussians(
                rs.bg, d["means3D"], d["colors"], d["opacities"], d["scales"], d["rotations"], 1.0, e, d["all_map"], rs.viewmatrix,
                rs.projmatrix, rs.tanfovx, rs.tanfovy, H, W, e, 0, rs.campos, False, False, True, debug)
            (g_m2d, g_col, g_op, g_m3d, _, _, g_sc, g_rot, g_amap) = _C.rasterize_gaussians_backward(
                rs.bg, e, d["means3D"], radii, d["colors"], d["all_map"], d["opacities"], d["scales"], d["rotations"], 1.0, e,
                rs.viewmatrix, rs.projmatrix, rs.tanfovx, rs.tanfovy, g[0], g[1], g[2], e, 0, rs.campos, gB, R, bB, iB, False, True,
                False)
            torch.cuda.synchronize()
            assert (radii.cpu().numpy() == t.radii).all(), f"{label}: radii"
            n = lambda x: x.detach().cpu().numpy()
            for k, v in (("color", color), ("invdepth", invd), ("all_map", amap)):
                report.append((label, k, ratio(n(v)[:, keep], t.out[k][:, keep], img_b[k][:, keep])))
            for k, v in (("dL_dmeans3D", g_m3d), ("dL_dmeans2D", g_m2d), ("dL_dopacity", g_op), ("dL_dcolors", g_col),
                         ("dL_dscales", g_sc), ("dL_drotations", g_rot), ("dL_dall_map", g_amap)):
                report.append((label, k, ratio(n(v).reshape(t.g[k].shape), t.g[k], g_b[k])))
    finally:
        _lib.load().cgs_reset_binning_hints()
    bad = [x for x in report if not x[2] <= 1.0]
    print(f"\n   {sc.name}: {sc.P} splats kept of {row[3]}, {W} x {H}, undecided pixels {int(mask.sum())}")
    _print_report(sc.name, report)
    assert not bad, f"{sc.name}: outside the float64 bounds (ratio > 1): " + "; ".join(f"[{l}] {k} {r:.2f}" for l, k, r in bad)
