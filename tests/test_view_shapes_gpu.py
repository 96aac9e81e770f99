"""GPU: the fused per-splat view kernels (k_view_fwd, k_view_bwd<WAVES>, k_sample_bwd_close; csrc/view.hip, csrc/sampling.hip)
held to the float64 truth of tests/view_ref64.py ELEMENT-WISE, with no outlier budget, at every block-slot shape.

Blocks of k_view_bwd hold 256 // m whole curves.  The shapes are those of test_sampling_gpu.py::SAMPLE_CASES -- one partial block
(1 x 5), MAX_M (1 x 32), 21 curves per block with four idle threads and a second block of one curve (22 x 12), three blocks
with a tail (43 x 12), no idle thread (9 x 32, 33 x 8), 64 curves per block (65 x 4) -- and 25 x 32 (three full blocks and a
tail at MAX_M), each with and without use_mask, mixed curve types, on a 64 x 80 image (ragged in both tile directions); two of
them again under a camera that culls part of the samples of some curves and all samples of others.  The scenes sit on no
alpha / T / radius / mask decision edge (tests/test_view_ref64_cpu.py), so every element has to agree.

Criterion per tensor: tests/util.py::assert_close with rel = 1e-4 of the tensor's maximum, abs_floor = 1e-6, outlier_frac = 0
(the small-shape settings of test_sampling_gpu.py) OR, where that is larger, four times the worst element error of the general
chain (sample_curves -> splat_attributes -> rasterizer op; not the code under test) against the same truth on the same scene
-- the project's allowance for the float-atomics order of two compositors (bucket-vs-exact fuzz of test_pipeline_gpu.py).

Measured worst element errors, as a fraction of the tensor's maximum, fused / general (MI355X; nothing came near 1e-4, so the
four-times-general clause never decided a case; the full per-tensor list is printed by the tests):

    scene            means2D          curve_points     width            opacity          mask
    1x5              1.9e-6 / 1.7e-6  8.6e-7 / 8.1e-7  1.6e-6 / 3.1e-6  3.3e-6 / 3.5e-6  4.6e-6 / 5.3e-6
    1x32             6.3e-6 / 6.3e-6  1.9e-6 / 2.0e-6  1.5e-6 / 6.0e-6  5.5e-6 / 5.2e-6  3.7e-6 / 3.7e-6
    22x12            4.6e-6 / 4.7e-6  3.6e-6 / 3.3e-6  4.3e-6 / 3.9e-6  2.5e-6 / 2.7e-6  9.4e-6 / 1.0e-5
    43x12            8.7e-6 / 8.0e-6  1.8e-6 / 1.8e-6  1.2e-6 / 1.6e-6  2.8e-6 / 2.5e-6  5.7e-6 / 5.3e-6
    9x32             3.9e-6 / 4.4e-6  1.8e-6 / 1.5e-6  3.6e-6 / 3.0e-6  1.6e-6 / 1.2e-6  5.7e-6 / 6.1e-6
    33x8             4.8e-6 / 6.6e-6  2.6e-6 / 3.5e-6  1.4e-6 / 1.3e-6  1.8e-6 / 2.2e-6  3.8e-6 / 4.6e-6
    65x4             5.3e-6 / 5.3e-6  5.0e-6 / 3.9e-6  1.3e-6 / 1.1e-6  1.8e-6 / 2.4e-6  1.9e-6 / 1.9e-6
    25x32            5.3e-6 / 5.3e-6  9.2e-7 / 1.5e-6  3.2e-6 / 2.0e-6  1.0e-6 / 1.1e-6  4.2e-6 / 4.1e-6
    22x12-cull       3.2e-6 / 3.7e-6  2.2e-6 / 2.2e-6  2.4e-7 / 3.4e-7  9.7e-7 / 1.0e-6  3.8e-6 / 3.2e-6
    9x32-cull        1.3e-5 / 1.3e-5  4.1e-6 / 3.9e-6  1.5e-6 / 2.1e-6  1.1e-6 / 9.9e-7  3.8e-6 / 6.0e-6
    shared 22x12     -                3.1e-6 / 2.7e-6  2.5e-6 / 3.0e-6  1.4e-6 / 1.2e-6  -
    shared 9x32      -                1.7e-6 / 1.7e-6  3.8e-6 / 3.8e-6  5.6e-7 / 8.2e-7  -
    large 43690x12   1.4e-5 / 1.4e-5  3.3e-6 / 3.4e-6  3.8e-6 / 2.0e-6  1.5e-6 / 1.9e-6  -
    large 43691x12   1.4e-5 / 1.4e-5  3.3e-6 / 3.4e-6  2.4e-6 / 2.4e-6  1.3e-6 / 1.2e-6  -

(rows of the slot shapes: the larger of the runs with and without use_mask.)  The culled curves of the large scenes on their own
scale: 3.0e-6 / 7.9e-6 (43 690) and 9.0e-6 / 7.1e-6 (43 691).  Two accumulate = 0 calls of cgs_view_backward differed by
exactly 0 at both shapes; accumulate = 1 landed within one float32 ulp of pre-fill + result."""
import functools

import numpy as np
import pytest
import torch

import view_ref64 as V
from util import assert_close, hip_settings, tanfov

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GRADS = ("g_means2D", "g_curve_points", "g_width", "g_opacity")


def _leaves(c, mask):
    leaves = [c[k].to(DEV).requires_grad_(True) for k in ("curve_points", "width", "opacity")]
    ml = mask.to(DEV).requires_grad_(True) if mask is not None else None
    return leaves, ml


def _collect(color, radii, dimg, leaves, ml, m2d):
    (color * dimg.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    out = dict(color=color.detach().cpu().numpy(), radii=radii.cpu().numpy(), g_means2D=m2d.grad.cpu().numpy(),
               g_curve_points=leaves[0].grad.cpu().numpy(), g_width=leaves[1].grad.cpu().numpy(),
               g_opacity=leaves[2].grad.cpu().numpy())
    if ml is not None:
        out["g_mask"] = ml.grad.cpu().numpy()
    return out


def _fused(c, mask, cam, dimg, m):
    """ops.view_render.view_render with a loss on the image alone: k_view_fwd, the unit-colour compositors, k_view_bwd and
    k_sample_bwd_close."""
    from curve_gaussian_amd.ops import view_render as VR
    camd, bg, isb = cam.to(DEV), torch.zeros(3, device=DEV), c["is_bezier"].to(DEV)
    for _ in range(4):   # (the first forward of a new shape may outgrow its buckets: the capacity is raised, render again)
        leaves, ml = _leaves(c, mask)
        m2d = torch.zeros(c["curve_points"].shape[0] * m, 3, device=DEV, requires_grad=True)
        pend = []
        color, _invd, _amap, radii, _dir = VR.view_render(leaves[0], leaves[1], leaves[2], ml, m2d, isb, m, V.MASK_THR, bg, camd,
                                                          *tanfov(cam), 0, None, False, False, pend)
        if VR.finish(pend.pop())[0]:
            return _collect(color, radii, dimg, leaves, ml, m2d)
    raise AssertionError("the fused forward kept outgrowing its buckets")


def _general(c, mask, cam, dimg, m):
    """What render(fused=False) does: sample_curves -> splat_attributes -> the rasterizer op."""
    from curve_gaussian_amd.diff_cur_rasterization import GaussianRasterizer
    from curve_gaussian_amd.ops.curve_sampling import sample_curves, splat_attributes
    camd = cam.to(DEV)
    leaves, ml = _leaves(c, mask)
    xyz, rot, scl = sample_curves(leaves[0], leaves[1], c["is_bezier"].to(DEV), m)
    rotn, opac, scales, amap_in = splat_attributes(rot, xyz, leaves[2], scl, camd.camera_center, camd.world_view_transform, m, ml,
                                                   V.MASK_THR)
    P = xyz.shape[0]
    m2d = torch.zeros(P, 3, device=DEV, requires_grad=True)
    color, radii, _invd, _amap = GaussianRasterizer(hip_settings(cam, torch.zeros(3), DEV))(
        means3D=xyz, means2D=m2d, shs=None, colors_precomp=torch.ones(P, 1, device=DEV), opacities=opac, scales=scales,
        rotations=rotn, all_map=amap_in, cov3D_precomp=None)
    return _collect(color, radii, dimg, leaves, ml, m2d)


def _worst(got, ref):
    ref = np.asarray(ref, np.float64)
    return float(np.abs(np.asarray(got, np.float64).reshape(ref.shape) - ref).max() / np.abs(ref).max())


def _hold(tag, name, fused, general, truth):
    """The criterion of the module docstring for one tensor; prints both worst element errors."""
    ref = np.asarray(truth, np.float64)
    assert np.abs(ref).max() > 0, f"{tag} {name}: the truth is all zero"
    fused, general = np.asarray(fused, np.float64).reshape(ref.shape), np.asarray(general, np.float64).reshape(ref.shape)
    e_f, e_g = _worst(fused, ref), _worst(general, ref)
    print(f"{tag}: {name} worst element error of max: fused {e_f:.2e}, general {e_g:.2e}")
    try:
        assert_close(f"{tag} {name}", fused, ref, rel=1e-4, abs_floor=1e-6, outlier_frac=0)
    except AssertionError:
        if not e_f <= 4.0 * e_g:
            raise


def _compare(tag, f, g, t, names):
    assert np.array_equal(f["radii"], g["radii"]), f"{tag}: radii of the fused route and of the general chain differ"
    assert np.array_equal(f["radii"], t["radii"]), f"{tag}: radii differ from the truth's"
    assert_close(f"{tag} image", f["color"], t["color"], outlier_frac=0)
    for name in names:
        _hold(tag, name, f[name], g[name], t[name])


SHAPE_CASES = [pytest.param(B, m, seed, False, id=f"{B}x{m}") for (B, m), seed in V.SHAPE_SEEDS.items()]
SHAPE_CASES += [pytest.param(B, m, seed, True, id=f"{B}x{m}-cull") for (B, m), seed in V.CULL_SEEDS.items()]


@pytest.mark.parametrize("use_mask", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("B,m,seed,cull", SHAPE_CASES)
def test_fused_view_route_matches_float64_at_every_slot_shape(B, m, seed, cull, use_mask):
    c, mask, cam, dimg = V.scene(B, m, seed, cull)
    mask = mask if use_mask else None
    t = V.view_ref64(c, mask, V.MASK_THR, cam, 0.0, dimg, m)
    if cull:
        vis = (t["radii"].reshape(B, m) > 0).sum(1)
        assert V.partly_culled(t["radii"], B, m).any() and (vis == 0).any(), "no curve is cut by this camera"
    f, g = _fused(c, mask, cam, dimg, m), _general(c, mask, cam, dimg, m)
    _compare(f"{B}x{m}{'-cull' if cull else ''} mask={use_mask}", f, g, t, GRADS + (("g_mask",) if use_mask else ()))


# ------------------------------------------------------------------------------------------------ accumulate bits (C ABI)
def _view_calls(c, cam, m, mask=None):
    from test_pipeline_gpu import _ViewCalls
    return _ViewCalls(c["curve_points"], c["width"], c["opacity"], c["is_bezier"], cam, 1024, mask=mask, m=m)


@pytest.mark.parametrize("B,m", list(V.CULL_SEEDS), ids=lambda v: str(v))
def test_view_backward_accumulate_bit_adds_element_wise(B, m):
    """cgs_view_backward(accumulate = 1) into buffers pre-filled with random values == pre-fill + the accumulate = 0 result,
    element by element; tolerance: the run-to-run difference of two accumulate = 0 calls (measured here) plus one float32 ulp
    of the sum."""
    c, mask, cam, dimg = V.scene(B, m, V.SHAPE_SEEDS[B, m])
    vc = _view_calls(c, cam, m, mask)
    d = dimg.to(DEV)
    shapes = [(B, 4, 3), (B, 1), (B, 1), (B, m, 1)]
    names = ("curve_points", "width", "opacity", "mask")

    def run(bufs, accumulate):
        vc.forward()
        vc.backward(d, bufs[0], bufs[1], bufs[2], accumulate, bufs[3])
        return [b.cpu().numpy().astype(np.float64) for b in bufs]
    one = run([vc.f32(*s) for s in shapes], 0)
    two = run([vc.f32(*s).fill_(1e6) for s in shapes], 0)            # (overwritten, not added to)
    gen = torch.Generator().manual_seed(B * m)
    pre = [torch.randn(*s, generator=gen) * max(float(np.abs(o).max()), 1e-3) for s, o in zip(shapes, one)]
    acc = run([p.to(DEV).contiguous() for p in pre], 1)
    for name, a, b, p, got in zip(names, one, two, pre, acc):
        assert np.abs(a).max() > 0, name
        want = p.numpy().astype(np.float64) + a
        noise = float(np.abs(a - b).max())
        ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
        err = np.abs(got - want)
        print(f"{B}x{m}: {name} run-to-run {noise:.2e}, accumulate worst {err.max():.2e} (max {np.abs(a).max():.2e})")
        assert (err <= noise + ulp).all(), f"{name}: accumulate = 1 is off by {err.max():.3e} (run-to-run {noise:.1e})"


@pytest.mark.parametrize("B,m", list(V.CULL_SEEDS), ids=lambda v: str(v))
def test_shared_sampling_over_two_views_matches_the_summed_truths(B, m):
    """cgs_view_shared_begin / cgs_view_forward_shared / cgs_view_backward(CGS_VIEW_ACCUMULATE | CGS_VIEW_SHARED) /
    cgs_view_shared_end over two views: the sum of the two single-view truths, under the criterion of the slot-shape test."""
    import ctypes as C
    from curve_gaussian_amd import _lib as L
    seed = V.SHAPE_SEEDS[B, m]
    views = [V.scene(B, m, seed), V.scene(B, m, seed, second=True)]
    c = views[0][0]
    truth = [V.view_ref64(c, None, V.MASK_THR, cam, 0.0, dimg, m) for _c, _mask, cam, dimg in views]
    general = [_general(c, None, cam, dimg, m) for _c, _mask, cam, dimg in views]
    vc = _view_calls(c, views[0][2], m)
    lib, pt, st = vc.lib, L.ptr, L.raw_stream(torch.device(DEV))
    g = [vc.f32(B, 4, 3), vc.f32(B, 1), vc.f32(B, 1)]
    L.check(lib.cgs_view_shared_begin(vc.B, vc.m, pt(vc.cp), pt(vc.isb), pt(vc.coef), pt(vc.norms), pt(vc.scratch), st),
            "cgs_view_shared_begin")
    for (_c, _mask, cam, dimg), t in zip(views, truth):
        vc.cam = cam.to(DEV)
        vc.forward(shared=True)
        assert np.array_equal(vc.radii.cpu().numpy(), t["radii"])
        vc.backward(dimg.to(DEV), *g, 3)
    L.check(lib.cgs_view_shared_end(vc.B, vc.m, pt(vc.cp), pt(vc.w), pt(vc.isb), pt(vc.coef), C.c_float(1e-8), pt(vc.norms),
                                    pt(vc.scratch), pt(g[0]), pt(g[1]), 0, st), "cgs_view_shared_end")
    torch.cuda.synchronize()
    for name, got in zip(("g_curve_points", "g_width", "g_opacity"), g):
        _hold(f"shared {B}x{m}", name, got.cpu().numpy(), general[0][name].astype(np.float64) + general[1][name],
              truth[0][name].astype(np.float64) + truth[1][name])


# ------------------------------------------------------------------------------------------------ the large instance
@functools.lru_cache(maxsize=None)
def _large_truth(B):
    c, mask, cam, dimg = V.large_scene(B)
    return c, cam, dimg, V.view_ref64(c, None, V.MASK_THR, cam, 0.0, dimg, V.LARGE_M)


@pytest.mark.parametrize("B", V.LARGE_B)
def test_view_backward_at_the_threshold_of_its_large_instance(B):
    """43 690 x 12 = 524 280 splats run k_view_bwd<CGS_VIEW_BWD_WAVES>, 43 691 x 12 = 524 292 run
    k_view_bwd<CGS_VIEW_BWD_WAVES_LARGE> (launched from 512 Ki splats).  The first view_ref64.LARGE_VISIBLE curves are a scene
    of the slot-shape test; every further curve lies behind the camera: culled, so it costs the compositors and the oracle
    nothing, and still reached by the two grid-wide norm sums -- every block of the launch writes gradients that are checked.
    Those are tiny next to the visible curves' (1e-5 against 1e2), so the culled curves' dL/dcurve_points is ALSO held on its
    own scale: 1e-4 of ITS maximum or four times the general chain's error there."""
    m, nv = V.LARGE_M, V.LARGE_VISIBLE
    assert (B * m >= 512 * 1024) == (B == V.LARGE_B[1])
    c, cam, dimg, t = _large_truth(B)
    f, g = _fused(c, None, cam, dimg, m), _general(c, None, cam, dimg, m)
    _compare(f"large {B}x{m}", f, g, t, GRADS)
    far_t = t["g_curve_points"][nv:].astype(np.float64)
    far_f, far_g = f["g_curve_points"][nv:].astype(np.float64), g["g_curve_points"][nv:].astype(np.float64)
    assert np.abs(far_f).max() > 0 and np.abs(far_t).max() > 0, "the culled curves' gradients are all zero"
    assert (np.abs(far_f).reshape(B - nv, -1).max(1) > 0).mean() > 0.99                # (every block wrote its curves)
    e_f, e_g = _worst(far_f, far_t), _worst(far_g, far_t)
    print(f"large {B}x{m}: culled curves' g_curve_points worst element error of THEIR max: fused {e_f:.2e}, general {e_g:.2e}")
    assert e_f <= max(1e-4, 4.0 * e_g)
