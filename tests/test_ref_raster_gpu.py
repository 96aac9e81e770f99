"""GPU: everything the rasterizer suite holds to the C restatement (oracle/raster_ref.c), held to the REFERENCE's own kernels.

oracle/_ref/libref_raster.so is the reference's cuda_rasterizer/{forward,backward,rasterizer_impl}.cu built for gfx950 by
oracle/ref_raster/Makefile (shim headers of ours, one textual edit: the launch chevrons), behind a C ABI of ours
(oracle/ref_raster.py).  Until it existed the restatement and the kernels were written by the same hands from the same reading
of forward.cu / backward.cu, and a shared misreading would have kept every test green.

Budgets are the ones the HIP-against-oracle tests use (tests/util.py::assert_close: 1e-4 of the maximum, 1e-4 outlier budget
for alpha >= 1/255 / T < 1e-4 decisions that flip under another rounding of the exponent).  The reference's forward has no
atomics: restatement against reference is held tighter (TIGHT_REL).  Its backward accumulates with order-dependent float
atomics: gradients keep the existing outlier budgets.  Known deviations of the HIP path, each handled where it
shows: tile culling changes num_rendered and the lists (binning compared with OPT_NO_TILE_CULLING); bit 31 of the saved
n_contrib word is the "terminated" flag (masked); the unit-colour forward saves the position in front of the terminating
entry (n_contrib compared on the general instance only, with the flip budget); the HIP backward recomputes cov3D (the values
agree, so the gradients are compared as they are)."""
import math
import time
import types

import numpy as np
import pytest
import torch

import quirk_cases as Q
import test_quirks_cpu as QC
import util
from oracle import ref_raster as REF
from util import S, assert_close, near_threshold_pairs, tanfov
from test_raster_gpu import (CAMS, GOLDEN, _binning_case, _curve_splats, _decode_state, _golden, _raster_raw, assert_radii,
                             rand_grads, run_hip)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# restatement (fixtures) against reference, forward outputs: same float32 arithmetic in the same order, contraction off on
# both sides; only the exponent's last bit differs (libm expf against the device's expf)
TIGHT_REL = 2e-6


@pytest.fixture
def no_tile_culling():
    from curve_gaussian_amd.diff_cur_rasterization import OPT_NO_TILE_CULLING
    prev, util.OPTIONS[0] = util.OPTIONS[0], util.OPTIONS[0] | OPT_NO_TILE_CULLING
    yield
    util.OPTIONS[0] = prev


def ref_forward(sp, cam, bg, render_geo=True, antialiasing=False, scale_modifier=1.0, cov3D=None, sh=None, degree=0):
    """The reference binary on the arguments util.oracle_forward gives the C restatement."""
    tfx, tfy = tanfov(cam)
    d = lambda t: None if t is None else t.detach().to(DEV)
    use_cov = cov3D is not None
    return REF.forward(d(bg), d(sp["means3D"]), None if sh is not None else d(sp["colors"]), d(sp["opacities"]),
                       None if use_cov else d(sp["scales"]), None if use_cov else d(sp["rotations"]), scale_modifier, d(cov3D),
                       d(sp["all_map"]), d(cam.world_view_transform), d(cam.full_proj_transform), tfx, tfy, cam.image_height,
                       cam.image_width, d(sh), degree, d(cam.camera_center), antialiasing=antialiasing, render_geo=render_geo)


def ref_backward(fw, grads):
    """-> numpy gradients under oracle.raster.backward's names; dL_dsh keeps the binding's [P,M,3] layout (quirk 16)."""
    g = REF.backward(fw, *grads)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in g.items()}


def _np(fw):
    return {"color": fw.color.cpu().numpy(), "invdepth": fw.invdepth.cpu().numpy(), "all_map": fw.out_all_map.cpu().numpy(),
            "radii": fw.radii.cpu().numpy()}


def compare_ref(sp, cam, bg, grads, grad_outlier_frac=None, grad_outlier_frac_big=None, colour_grad=True, debug=True,
                min_outlier_rows=0, **kw):
    """test_raster_gpu.compare with the reference binary in place of the C restatement: same criteria, same budgets."""
    fw = ref_forward(sp, cam, bg, **kw)
    ref = _np(fw)
    hip = run_hip(sp, cam, bg, grads, colour_grad=colour_grad, debug=debug, **kw)
    assert_radii(hip["radii"], ref["radii"])
    assert_close("color", hip["color"], ref["color"])
    assert_close("invdepth", hip["invdepth"], ref["invdepth"])
    assert_close("all_map", hip["all_map"], ref["all_map"])
    if grads is not None:
        gr = ref_backward(fw, grads)
        for k, v in hip["g"].items():
            if k == "dL_dcolors" and (kw.get("sh") is not None or not colour_grad):
                continue  # colours come from SH / no colour gradient requested
            r = gr[k]
            if k == "dL_dsh":
                # quirk 16: the reference writes P*M floats into the head of its [P,M,3] buffer; autograd sums that buffer
                # onto the [P,M,1] input.  The binary's own buffer, summed the same way, is what the HIP path must produce.
                r = r.sum(-1)
                v = v.reshape(r.shape)
            kw2 = {} if grad_outlier_frac is None else {"outlier_frac": grad_outlier_frac}
            row = int(np.prod(v.shape[1:])) if v.ndim > 1 else 1     # elements one splat owns in this tensor
            assert_close(k, v, r.reshape(v.shape), abs_floor=1e-6, outlier_frac_big=grad_outlier_frac_big,
                         min_outliers=min_outlier_rows * row, **kw2)
    fw.free()
    return hip, ref


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the reference binary against the frozen fixtures (= the C restatement, tests/golden/make_raster_golden.py)

def _near_pairs_of_fixture(z, cam):
    """near_threshold_pairs over the fixture's own saved state: how many (pixel, splat) decisions may legally flip."""
    fw = types.SimpleNamespace(H=cam.image_height, W=cam.image_width, means2D=z["means2D"], conic_opacity=z["conic_opacity"],
                               point_list=z["point_list"], ranges=z["ranges"])
    return near_threshold_pairs(fw, window=1e-5)


@pytest.mark.parametrize("name", GOLDEN)
def test_reference_binary_reproduces_the_frozen_fixtures(name):
    sp, cam, bg, z = _golden(name)
    H, W = cam.image_height, cam.image_width
    fw = ref_forward(sp, cam, bg)
    out = _np(fw)
    # integer work: bit-exact (both sorts are stable radix sorts: ties in list order by splat index)
    assert np.array_equal(out["radii"], z["radii"])
    assert fw.num_rendered == int(z["num_rendered"][0])
    assert np.array_equal(fw.ranges, z["ranges"])
    assert np.array_equal(fw.point_list, z["point_list"])
    # forward values: no atomics on either side -- tight, with room for the decisions that sit on a threshold only
    flips = _near_pairs_of_fixture(z, cam)
    nc_bad = int((fw.n_contrib != z["n_contrib"]).sum())
    assert nc_bad <= flips, f"n_contrib differs at {nc_bad} pixels, {flips} near-threshold decisions in the scene"
    for k, got, want in (("color", out["color"], z["color"]), ("invdepth", out["invdepth"], z["invdepth"]),
                         ("all_map", out["all_map"], z["out_all_map"]), ("final_T", fw.final_T[None], z["final_T"][None])):
        worst = assert_close(k, got, want, rel=TIGHT_REL, outlier_frac=0.0, min_outliers=4 * flips)
        print(f"reference vs fixture {name} {k}: worst {worst:.2e} of max")
    vis = out["radii"] > 0          # (the reference leaves the per-splat state of culled splats unwritten)
    for k in ("means2D", "conic_opacity", "depths"):
        assert_close(k, getattr(fw, k)[vis], z[k][vis], rel=TIGHT_REL, outlier_frac=0.0)
    t = lambda k: torch.from_numpy(z[k].copy())
    gr = ref_backward(fw, (t("dL_dcolor"), t("dL_dinvdepth"), t("dL_dout_all_map")))
    names = ["dL_dmeans2D", "dL_dcolors", "dL_dopacity", "dL_dmeans3D", "dL_dcov3D", "dL_dscales", "dL_drotations",
             "dL_dall_map", "dL_dconic", "dL_dinvdepths"]
    for k in names:
        want = z["g_" + k]
        assert_close(k, gr[k].reshape(want.shape), want, abs_floor=1e-6)
    assert gr["dL_dsh"].shape == (sp["means3D"].shape[0], 0, 3)
    gt = ref_backward(fw, (t("dL_dcolor"), None, None))     # the training configuration: only dL/dcolour flows in
    assert gt["dL_dinvdepths"].shape == (0, 1)
    for k in ("dL_dmeans3D", "dL_dmeans2D", "dL_dopacity", "dL_dscales", "dL_drotations", "dL_dconic"):
        want = z["gt_" + k]
        assert_close("training " + k, gt[k].reshape(want.shape), want, abs_floor=1e-6)
    fw.free()


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. the HIP path against the reference binary, directly

@pytest.mark.parametrize("cam_i", [0, 1, 2])
@pytest.mark.parametrize("P,H,W,seed", [(3000, 128, 160, 11), (800, 77, 130, 12), (20000, 208, 304, 13)])
def test_hip_matches_reference_on_random_clouds(P, H, W, seed, cam_i):
    sp = S.random_splats(P, seed, scale_range=(0.004, 0.05))
    cam = S.make_camera(*CAMS[cam_i], H, W)
    compare_ref(sp, cam, torch.tensor([0.3, 0.0, 0.0]), rand_grads(H, W, seed + 100))


@pytest.mark.parametrize("H,W", [(33, 47), (50, 70), (17, 209)])
def test_hip_matches_reference_on_ragged_images(H, W):
    sp = S.random_splats(900, 90 + H, scale_range=(0.004, 0.05))
    cam = S.make_camera(*CAMS[0], H, W)
    compare_ref(sp, cam, torch.tensor([0.2, 0.0, 0.0]), rand_grads(H, W, H + W))


def test_hip_matches_reference_on_ties_opaque_stacks_and_the_training_call():
    H, W = 64, 80
    cam = S.make_camera(*CAMS[1], H, W)
    sp = S.random_splats(600, 302, scale_range=(0.01, 0.05))
    sp["means3D"] = sp["means3D"][torch.arange(600) % 40].contiguous()          # coincident depths
    compare_ref(sp, cam, torch.zeros(3), rand_grads(H, W, 1))
    sp = S.random_splats(500, 303, scale_range=(0.02, 0.09))
    sp["opacities"][0::3] = 0.995                                                # the 0.99 clamp, T < 1e-4 everywhere
    sp["opacities"][1::6] = 0.9995
    compare_ref(sp, cam, torch.tensor([0.1, 0.0, 0.0]), rand_grads(H, W, 2))
    # train.py: unit colours without a gradient, only `render` in the loss (the gated unit-colour route)
    sp = S.random_splats(2500, 21)
    sp["colors"] = torch.ones_like(sp["colors"])
    compare_ref(sp, S.make_camera(*CAMS[0], 96, 144), torch.zeros(3), rand_grads(96, 144, 5, (True, False, False)),
                colour_grad=False, debug=False)


def test_hip_matches_reference_behind_the_camera_single_splat_and_empty():
    H, W = 50, 70
    cam = S.make_camera(*CAMS[0], H, W)
    bg = torch.tensor([0.4, 0.0, 0.0])
    sp = S.random_splats(500, 51)
    sp["means3D"] = sp["means3D"] + torch.tensor([0.0, -6.0, 0.0])              # every splat behind the camera
    hip, ref = compare_ref(sp, cam, bg, rand_grads(H, W, 1))
    assert (ref["radii"] == 0).all() and np.allclose(ref["color"], 0.4)
    sp = S.random_splats(500, 52)
    sp["means3D"][::2] += torch.tensor([0.0, -6.0, 0.0])                         # half of them behind
    compare_ref(sp, cam, bg, rand_grads(H, W, 2))
    ten = S.random_splats(10, 53, scale_range=(0.05, 0.1))
    i = int((ten["means3D"] - 0.5).norm(dim=1).argmin())                          # the one nearest the camera's target
    one = {k: v[i:i + 1].clone() for k, v in ten.items()}
    hip, ref = compare_ref(one, cam, bg, rand_grads(H, W, 3))
    assert ref["radii"][0] > 0
    # P == 0: the reference runs nothing (rasterize_points.cu:91): all-zero outputs, no background
    empty = {k: v[:0] for k, v in one.items()}
    fw = ref_forward(empty, cam, bg)
    assert fw.num_rendered == 0 and fw.radii.numel() == 0 and float(fw.color.abs().max()) == 0.0
    assert tuple(fw.invdepth.shape) == (1, H, W) and tuple(fw.out_all_map.shape) == (4, H, W)
    g = REF.backward(fw, *rand_grads(H, W, 4))
    assert all(v.numel() == 0 for v in g.values())
    fw.free()


def test_hip_matches_reference_without_geo_with_antialiasing_and_scale_modifier():
    H, W = 80, 112
    sp = S.random_splats(1500, 31)
    cam = S.make_camera(*CAMS[1], H, W)
    compare_ref(sp, cam, torch.tensor([0.1, 0, 0]), rand_grads(H, W, 7, (True, True, False)), render_geo=False)
    compare_ref(sp, cam, torch.tensor([0.1, 0, 0]), rand_grads(H, W, 8), antialiasing=True)
    compare_ref(sp, cam, torch.tensor([0.0, 0, 0]), rand_grads(H, W, 9), scale_modifier=1.7)


def test_hip_matches_reference_with_cov3d_precomp_and_single_channel_sh():
    H, W = 64, 96
    P = 1200
    sp = S.random_splats(P, 41)
    cam = S.make_camera(*CAMS[0], H, W)
    q = sp["rotations"]
    r, x, y, z = q[:, 0], q[:, 1], q[:, 2], q[:, 3]
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - r * z), 2 * (x * z + r * y), 2 * (x * y + r * z),
                     1 - 2 * (x * x + z * z), 2 * (y * z - r * x), 2 * (x * z - r * y), 2 * (y * z + r * x),
                     1 - 2 * (x * x + y * y)], 1).reshape(-1, 3, 3)
    Sg = R @ torch.diag_embed(sp["scales"] ** 2) @ R.transpose(1, 2)
    cov = torch.stack([Sg[:, 0, 0], Sg[:, 0, 1], Sg[:, 0, 2], Sg[:, 1, 1], Sg[:, 1, 2], Sg[:, 2, 2]], 1).contiguous()
    compare_ref(sp, cam, torch.zeros(3), rand_grads(H, W, 3), cov3D=cov)
    g = torch.Generator().manual_seed(77)
    for deg in (0, 1, 2, 3):
        sh = torch.randn(P, (deg + 1) ** 2, 1, generator=g) * 0.5               # get_features layout [P,M,1]
        compare_ref(sp, cam, torch.tensor([0.2, 0, 0]), rand_grads(H, W, 4 + deg), sh=sh, degree=deg)


def _compare_binning(sp, cam, P, H, W, check_n_contrib):
    """Tile culling off: num_rendered, tile ranges and every per-tile list equal the reference's, in both binning layouts."""
    fw = ref_forward(sp, cam, torch.zeros(3))
    ref_ranges, ref_list, ref_nc = fw.ranges, fw.point_list, fw.n_contrib
    nonempty = ref_ranges[:, 1] > ref_ranges[:, 0]
    for it in range(2):
        (R, color, radii, geomB, binB, imgB, invd, amap) = _raster_raw(sp, cam, H, W, torch.device(DEV), reset_hints=(it == 0))
        assert R == fw.num_rendered
        assert np.array_equal(radii.cpu().numpy(), fw.radii.cpu().numpy())
        ranges, point_list, n_contrib, _ = _decode_state(geomB, binB, imgB, P, H, W, R)   # (bit 31 masked there)
        lens = ranges[:, 1] - ranges[:, 0]
        assert np.array_equal(lens, ref_ranges[:, 1] - ref_ranges[:, 0])
        if it == 0:   # exact layout: the ranges themselves
            assert (ranges[nonempty] == ref_ranges[nonempty]).all()
        for t in np.nonzero(nonempty)[0]:
            assert (point_list[ranges[t, 0]:ranges[t, 1]] == ref_list[ref_ranges[t, 0]:ref_ranges[t, 1]]).all(), (it, t)
        if check_n_contrib:
            # same order, same arithmetic up to the exponent's rounding: n_contrib may differ at threshold flips only
            mism = (n_contrib.reshape(H, W) != ref_nc).mean()
            assert mism <= 2e-3, mism
        assert_close("color", color.cpu().numpy(), fw.color.cpu().numpy())
    fw.free()


@pytest.mark.parametrize("case", ["ties", "ties_mid", "oversized_bucket", "screen_filling", "elongated"])
def test_binning_matches_the_reference_bit_exact(case, no_tile_culling):
    H, W, P, sp = _binning_case(case)
    _compare_binning(sp, S.make_camera(*CAMS[0], H, W), P, H, W, case not in ("ties", "ties_mid"))


@pytest.mark.parametrize("name", GOLDEN)
def test_binning_of_the_fixture_scenes_matches_the_reference(name, no_tile_culling):
    sp, cam, bg, z = _golden(name)
    _compare_binning(sp, cam, sp["means3D"].shape[0], cam.image_height, cam.image_width, name != "ties")


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. the pencil-arithmetic quirk cases (tests/quirk_cases.py) hold for the reference binary too

def _ref_q(sp, antialiasing=False, cov3D=None):
    fw = ref_forward(sp, Q.camera(), torch.zeros(3), antialiasing=antialiasing, cov3D=cov3D)
    out = types.SimpleNamespace(color=fw.color.cpu().numpy(), radii=fw.radii.cpu().numpy(), num_rendered=fw.num_rendered,
                                n_contrib=fw.n_contrib, final_T=fw.final_T, fw=fw)
    return out


def _ref_q_grads(o, dimg):
    return ref_backward(o.fw, (torch.from_numpy(dimg), None, None))


def test_reference_quirk4_dilation_and_antialiasing_rescale():
    s = 2.0 * math.sqrt(0.3) / Q.focal()
    sp = Q.splats([(16, 16)], 2.0, s, 0.8)
    a, b = _ref_q(sp), _ref_q(sp, antialiasing=True)
    QC.check_quirk4(a, b, s)
    assert a.radii[0] == Q.radius_of(0.6) == 3


def test_reference_quirk5_eigenvalue_floor_and_det_zero_drop():
    o = _ref_q(Q.splats([(16, 16)], 2.0, 1e-7, 0.8))
    assert o.radii[0] == Q.radius_of(0.3) == 3
    sp = Q.splats([(15.5, 15.5)], Q.focal(), 0.0, 0.8)
    sp["means3D"][0, 2] = torch.tensor(np.float32(Q.focal()))
    cov = torch.tensor([[-0.3, 0.0, 0.0, 0.5, 0.0, 0.0]], dtype=torch.float32)
    o = _ref_q(sp, cov3D=cov)
    assert o.radii[0] == 0 and o.num_rendered == 0 and o.color.max() == 0
    cov[0, 0] = 0.25
    o = _ref_q(sp, cov3D=cov)
    assert o.radii[0] > 0 and o.color.max() > 0.5


def test_reference_quirk7_transmittance_stop_excludes_the_splat():
    o = _ref_q(QC.quirk7_scene())
    QC.check_quirk7_forward(o.color, o.final_T, o.n_contrib)
    d = np.zeros((1, Q.H, Q.W), np.float32)
    d[0, 16, 16] = 1.0
    QC.check_quirk7_backward(_ref_q_grads(o, d)["dL_dopacity"].reshape(-1))


def test_reference_quirk9_means2D_gradient_is_in_ndc_units():
    s = 2.0 * math.sqrt(0.7) / Q.focal()
    o = _ref_q(Q.splats([(16, 16)], 2.0, s, 0.8))
    d = np.zeros((1, Q.H, Q.W), np.float32)
    d[0, 16, 15] = 1.0
    QC.check_quirk9(_ref_q_grads(o, d)["dL_dmeans2D"], 1.0)


def test_reference_quirk12_masked_splat_stays_in_the_pipeline():
    o = _ref_q(Q.splats([(16, 16), (8, 8)], 2.0, [0.0, 0.1], [0.0, 0.8]))
    assert o.radii[0] == Q.radius_of(0.3) == 3 and o.radii[1] > 3
    assert o.num_rendered >= 2 and float(o.color[0, 16, 16]) == 0.0 and float(o.color[0, 8, 8]) > 0.7
    assert o.n_contrib[16, 16] == 0


# ---------------------------------------------------------------------------------------------------------------------------------
# 4. markVisible

@pytest.mark.parametrize("cam_i", [0, 2])
def test_mark_visible_matches_the_reference_bit_for_bit(cam_i):
    from curve_gaussian_amd.diff_cur_rasterization import GaussianRasterizer
    sp = S.random_splats(5000, 81, box=(-3.0, 3.0))
    m = sp["means3D"].clone()
    cam = S.make_camera(*CAMS[cam_i], 64, 64)
    # plus points on the near plane itself (view z within an ulp of 0.2, the `p_view.z <= 0.2f` test)
    vm = cam.world_view_transform
    R3, t3 = vm[:3, :3], vm[3, :3]
    zs = torch.tensor([0.2, np.nextafter(np.float32(0.2), np.float32(1)), np.nextafter(np.float32(0.2), np.float32(0))])
    view_pts = torch.stack([torch.zeros(3), torch.full((3,), 0.01), zs], 1)
    m = torch.cat([m, ((view_pts - t3) @ torch.linalg.inv(R3)).float()]).contiguous()
    rast = GaussianRasterizer(util.hip_settings(cam, torch.zeros(3), torch.device(DEV)))
    vis = rast.markVisible(m.to(DEV)).cpu().numpy()
    ref = REF.mark_visible(m.to(DEV), cam.world_view_transform.to(DEV), cam.full_proj_transform.to(DEV)).cpu().numpy()
    assert vis.dtype == np.bool_ and ref.dtype == np.bool_ and np.array_equal(vis, ref) and 0 < ref.sum() < len(ref)


# ---------------------------------------------------------------------------------------------------------------------------------
# 5. BASELINE configs at full size

@pytest.mark.parametrize("cfg,P", [("cfg1", 5004), ("cfg2", 50004), ("cfg3", 200004), ("cfg4", 300000), ("cfg5", 1000008)])
def test_baseline_config_matches_the_reference(cfg, P):
    """Forward and the TRAINING backward (unit colours without a gradient, only `render` in the loss) of every BASELINE
    config at full size, HIP against the reference binary; budgets of test_baseline_config_training_instance_matches_oracle
    (cfg5: 2e-4 / 6e-4 -- its every-pixel-terminates view flips ~1e-4 of the splats' threshold decisions)."""
    sp, cam = _curve_splats(cfg)
    assert sp["means3D"].shape[0] == P
    H, W = cam.image_height, cam.image_width
    g = rand_grads(H, W, 77, which=(True, False, False))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fw = ref_forward(sp, cam, torch.zeros(3))
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    ref_backward(fw, g)
    t2 = time.perf_counter()
    print(f"reference binary {cfg}: P={P} {W}x{H} num_rendered={fw.num_rendered}: forward {1e3 * (t1 - t0):.1f} ms, "
          f"backward {1e3 * (t2 - t1):.1f} ms (first call, incl. allocation and copies)")
    fw.free()
    big = cfg == "cfg5"
    # cfg1 (5 004 splats): the fractional budget is 1.5 elements per gradient tensor, less than one flipped decision.  Measured
    # on the MI355X: ONE pixel whose n_contrib differs between the reference and the C restatement (its T < 1e-4 test sits on
    # the rounding of the device's expf), which moves splats 440 - 442 of the pixel's list by up to 1.5e-3 of the maximum; the
    # HIP path agrees with the restatement there, and the reference repeats itself bit for bit.  Budget: one flipped decision
    # (four splats, as in test_raster_gpu.compare's campaign criterion).
    compare_ref(sp, cam, torch.zeros(3), g, colour_grad=False, debug=False, grad_outlier_frac=2e-4 if big else None,
                grad_outlier_frac_big=6e-4 if big else None, min_outlier_rows=4 if cfg == "cfg1" else 0)


# ---------------------------------------------------------------------------------------------------------------------------------
# 6. end to end: the product's render() under the defaults (fused view route) against the reference rasterizer

def test_render_under_the_defaults_matches_the_reference_rasterizer():
    """A GaussianCurveModel rendered by the product's render() (default flags: the fused view route) against the reference
    rasterizer, under the budgets of test_render_route_matches_the_oracle_at_cfg3_under_the_defaults.  The splats come from
    oracle/torch_ref.prepare_scaling_rot (pinned to the reference's own prepare_scaling_rot by
    tests/golden/prepare_scaling_rot.npz): they must agree with the model's derived tensors within test_sampling_gpu.py's budgets, and the curve-parameter
    gradients are the reference's per-splat gradients pulled back through that restatement.  The reference RASTERIZES the
    model's derived tensors, like the oracle in the cfg3 test: fed the restatement's, whose last bits differ, it decides one
    alpha >= 1/255 test the other way (measured on the MI355X: rend_dir off by 5.5e-3 of the maximum at one pixel)."""
    from oracle import torch_ref as TR
    from curve_gaussian_amd.gaussian_renderer import PipelineParams, render
    from test_render_route_gpu import _model
    curves, cams = S.make_config("cfg2", n_views=1)
    cam = cams[0]
    H, W = cam.image_height, cam.image_width
    gm = _model(curves)
    pkg = render(cam.to(DEV), gm, PipelineParams(), torch.zeros(3, device=DEV))
    dimg = torch.randn(1, H, W, generator=torch.Generator().manual_seed(17))
    (pkg["render"] * dimg.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    leaves = [curves[k].clone().requires_grad_(True) for k in ("curve_points", "width", "opacity")]
    xyz, rot, scl = TR.prepare_scaling_rot(leaves[0], leaves[1], curves["is_bezier"])
    P = xyz.shape[0]
    rotn = torch.nn.functional.normalize(rot)
    opac = torch.sigmoid(leaves[2]).repeat_interleave(12, 0)
    xyz_h, rot_h, scl_h = (t.detach().cpu() for t in (gm._xyz, gm._rotation, gm._scaling))
    assert xyz_h.shape[0] == P
    assert_close("xyz: model vs restatement", xyz_h.numpy(), xyz.detach().numpy(), rel=1e-6, outlier_frac=0.0)
    # (the budgets of test_sampling_gpu.py: |B(t) - B(t-h)| cancels about three digits in float32)
    assert_close("scaling: model vs restatement", scl_h.numpy(), scl.detach().numpy(), rel=1e-4, outlier_frac=0.0)
    assert_close("rotation: model vs restatement", rot_h.numpy(), rot.detach().numpy(), rel=1e-4, outlier_frac=2e-3)
    rotn_h = torch.nn.functional.normalize(rot_h)
    amap = TR.build_all_map(rot_h, xyz_h, cam.camera_center, cam.world_view_transform).float().contiguous()
    sp = dict(means3D=xyz_h, scales=scl_h, rotations=rotn_h, opacities=opac.detach(), all_map=amap, colors=torch.ones(P, 1))
    fw = ref_forward(sp, cam, torch.zeros(3))
    ref = _np(fw)
    radii = pkg["radii"].cpu().numpy()
    off = radii != ref["radii"]
    assert off.mean() <= 1e-5 and (np.abs(radii[off] - ref["radii"][off]) <= 1).all()
    assert_close("render", pkg["render"].detach().cpu().numpy(), np.clip(ref["color"], 0, 1))
    assert_close("rend_alpha", pkg["rend_alpha"].detach().cpu().numpy(), ref["all_map"][3:4])
    assert_close("depth", pkg["depth"].detach().cpu().numpy(), ref["invdepth"])
    rd = torch.tensor(ref["all_map"][0:3]).permute(1, 2, 0) @ cam.world_view_transform[:3, :3].T
    assert_close("rend_dir", pkg["rend_dir"].detach().cpu().numpy(), rd.permute(2, 0, 1).numpy())
    # render() clamps the image to [0, 1]: the upstream gradient only flows where the clamp is inactive
    dref = torch.from_numpy(np.where((ref["color"] > 0) & (ref["color"] < 1), dimg.numpy(), 0).astype(np.float32))
    gr = ref_backward(fw, (dref, None, None))
    fw.free()
    assert_close("means2D grad", pkg["viewspace_points"].grad.cpu().numpy(), gr["dL_dmeans2D"], abs_floor=1e-6)
    t = lambda a: torch.from_numpy(np.asarray(a, np.float32))
    ((xyz * t(gr["dL_dmeans3D"])).sum() + (scl * t(gr["dL_dscales"])).sum() + (rotn * t(gr["dL_drotations"])).sum()
     + (opac * t(gr["dL_dopacity"]).reshape(-1, 1)).sum()).backward()
    for name, leaf in zip(("_curve_points", "_width", "_opacity"), leaves):
        got = getattr(gm, name).grad.cpu()
        rel = float((got - leaf.grad).norm() / leaf.grad.norm())
        print(f"render() vs reference rasterizer, cfg2: dL/d{name} relative L2 {rel:.2e}")
        assert rel < 1e-4, f"dL/d{name}: relative L2 error {rel:.2e}"
        assert_close(f"dL/d{name} (element-wise)", got.numpy(), leaf.grad.numpy(), outlier_frac=1e-3, max_outlier=1e-3)
