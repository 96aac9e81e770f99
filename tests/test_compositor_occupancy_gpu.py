"""GPU: what the seven-wave compositors' shared storage can break (render.hip: s_si inside s_list, s_fmask inside s_ord, the
pixel operands in LDS; render_unit_bwd.hip: s_pix), on 48 x 32 images (6 tiles) and one 41 x 27 image.

Operator API (the sorting forward with tagged lists, the gated unit backward), per scene:
  * the bucket layout (the forward sorts each tile's bucket itself: fused rank + stage up to 256 entries, tile_rank_sort up
    to 1024) against the exact layout of the same build: images, saved image state and per-tile lists bit for bit;
  * both calls against the float64 truth of raster_ref64 within its per-element bounds (test_raster_ref64_gpu's own check).
Scenes: tile 0's list has exactly 1, 255, 256, 257, 1023, 1024 entries; 256 entries two of which share a depth (the fused
path claims its mask array, loses, and tile_rank_sort redoes the tile); every pixel terminates inside the first batch of a
three-batch list; every quadrant list empty but one; a ragged 41 x 27 image.

View entry points (cgs_view_forward / cgs_view_backward: the unit-colour forward and k_render_bwd_unit<8, false>): curve scenes
whose longest tile list lies on either side of the fused path's 256, on 48 x 32 and 41 x 27, against the chain of oracles with
smoke()'s bounds.  (Curves give no handle on exact list lengths: those are pinned through the operator above.)"""
import functools
import math

import numpy as np
import pytest
import torch

import raster_ref64 as R64
import util
from test_pipeline_gpu import _ViewCalls
from test_raster_gpu import _decode_state
from test_raster_ref64_gpu import check_against_truth, run_operator
from util import ORA, S, assert_close, hip_settings, tanfov

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, W = 32, 48
C_ONLY = (True, False, False)


def _b_len(n, seed):
    b = R64.Builder(H, W, seed)
    R64._faint(b, n, 2.0, 0.0005)
    return b


def _b_tie(seed):
    b = R64.Builder(H, W, seed)
    R64._faint(b, 256, 2.0, 0.0005, tie_groups=255)     # rows 0 and 255 share one centre: equal depth keys
    return b


def _b_term(seed):
    """Five opaque, all but uniform splats in front (the fifth terminates every pixel: T >= 0.12^4 > 1e-4 > 0.14^5, as in
    raster_ref64._scene_term_group), then 600 faint ones in tile 0: a list of 605 = three batches, left after the first."""
    b = R64.Builder(H, W, seed)
    for i in range(5):
        b.add(23.5, 15.5, 2.0 + 0.01 * i, 200.3, 200.3, b.rng.uniform(0.86, 0.88), 0.0)
    R64._faint(b, 600, 3.0, 0.0005)
    return b


def _b_one_quadrant(seed):
    b = R64.Builder(H, W, seed)
    r = b.rng
    for k in range(33):     # (raster_ref64._scene_uneven's splats, quadrant 3 of tile 0)
        b.add(11.5 + r.uniform(-0.4, 0.4), 11.5 + r.uniform(-0.4, 0.4), 2.0 + 0.01 * k, r.uniform(0.85, 1.0), r.uniform(0.85, 1.0),
              (4.0 / 33) * r.uniform(0.9, 1.0), r.uniform(0, math.pi))
    return b


def _b_ragged(seed):
    return R64._stack(27, 41, 40, seed, (30.4, 20.6), 12.0)


# name -> (builder, args, seed, exact length of tile 0's list or None)
CASES = {
    "len_1": (_b_len, (1,), 9101, 1), "len_255": (_b_len, (255,), 9102, 255), "len_256": (_b_len, (256,), 9103, 256),
    "len_257": (_b_len, (257,), 9104, 257), "len_1023": (_b_len, (1023,), 9105, 1023), "len_1024": (_b_len, (1024,), 9106, 1024),
    "tie_256": (_b_tie, (), 9107, 256), "term_first_batch": (_b_term, (), 9108, 605),
    "one_quadrant": (_b_one_quadrant, (), 9109, 33), "ragged_41x27": (_b_ragged, (), 9110, None),
}


@functools.lru_cache(maxsize=1)
def _truth(name):
    fn, args, seed, _ = CASES[name]
    b = fn(*args, seed)
    b.clear()
    sc = R64.Scene(name, built=(b.splats(), b.cam, b.H, b.W, seed))
    base = R64.Truth(sc, sc.sp)
    assert not R64.splat_failures(sc.sp, sc.cam, sc.H, sc.W).any()
    mask = R64.undecided_pixels(sc, base)
    R64.check_mask(sc, mask)
    R64.check_margins(R64.margins(sc, base, mask=mask))
    lists = R64.quadrant_lists(sc, base)
    grads = R64.scene_grads(sc, C_ONLY, mask)
    t = R64.truth(sc, grads, "unit", True)
    img_b, g_b = R64.bounds(t, J=base.jacobian())
    return sc, mask, lists, grads, t, img_b, g_b, R64.expected_n_contrib(sc, t, lists)


@pytest.mark.parametrize("name", list(CASES))
def test_bucket_layout_equals_exact_layout_and_both_sit_within_float64_bounds(name):
    from curve_gaussian_amd import _lib
    from curve_gaussian_amd.diff_cur_rasterization import _C
    sc, mask, lists, grads, t, img_b, g_b, want_pos = _truth(name)
    want_len = CASES[name][3]
    if name == "one_quadrant":
        assert [len(q) for q in lists[0]["quadrants"]] == [0, 0, 0, 33]
    if name == "term_first_batch":
        assert t.terminated()[~mask].all() and (want_pos[:16, :16][~mask[:16, :16]] <= 256).all()
    sp = R64.variant(sc, "unit")
    dev = torch.device(DEV)
    lib = _lib.load()
    # ---- forward alone, exact layout then buckets: bit for bit
    rs = hip_settings(sc.cam, sc.bg, dev)
    d = {k: v.to(dev) for k, v in sp.items()}
    e = torch.empty(0, device=dev)
    lib.cgs_reset_binning_hints()
    try:
        states = []
        for call in range(2):
            (R, color, radii, gB, bB, iB, invd, amap) = _C.rasterize_gaussians(
                rs.bg, d["means3D"], d["colors"], d["opacities"], d["scales"], d["rotations"], 1.0, e, d["all_map"], rs.viewmatrix,
                rs.projmatrix, rs.tanfovx, rs.tanfovy, sc.H, sc.W, e, 0, rs.campos, False, False, True, False)
            torch.cuda.synchronize()
            layout = _forward_layout(lib)
            ranges, plist, n_contrib, final_T = _decode_state(gB, bB, iB, sc.P, sc.H, sc.W, R)
            states.append((layout, ranges.astype(np.int64), plist, n_contrib, final_T.view(np.uint32), color.cpu().numpy().view(np.uint32),
                           invd.cpu().numpy().view(np.uint32), amap.cpu().numpy().view(np.uint32)))
        (l0, r0, p0, *img0), (l1, r1, p1, *img1) = states
        assert (l0, l1) == (0, 1), (l0, l1)
        lens = r0[:, 1] - r0[:, 0]
        assert (r1[:, 1] - r1[:, 0] == lens).all()
        if want_len is not None:
            assert lens[0] == want_len, lens.tolist()
        for tile in range(len(lens)):
            assert (p0[r0[tile, 0]:r0[tile, 1]] == p1[r1[tile, 0]:r1[tile, 1]]).all(), f"list order of tile {tile}"
        for what, a, b in zip(("n_contrib", "final_T", "color", "invdepth", "all_map"), img0, img1):
            assert np.array_equal(a, b), f"{what}: buckets differ from the exact layout"
        # ---- forward and backward through the operator, both layouts, against the float64 truth
        lib.cgs_reset_binning_hints()
        report, bad = [], []
        for layout, lname in ((0, "exact"), (1, "buckets")):
            got = run_operator(sp, sc.cam, sc.bg, grads, True, False, 0)
            assert got["layout"] == layout, (lname, got["layout"])
            bad += check_against_truth(f"{name}, {lname}", got, t, img_b, g_b, want_pos, False, report, mask)
    finally:
        lib.cgs_reset_binning_hints()
    print("\n   " + name + ": " + " ".join(f"{k.replace('dL_d', 'd')} {r:.3f}" for _, k, r in report))
    assert not bad, f"{name}: outside the float64 bounds (ratio > 1): " + "; ".join(f"[{l}] {k} {r:.2f}" for l, k, r in bad)


def _forward_layout(lib):
    import ctypes
    r, m, p = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int()
    lib.cgs_last_forward_stats(ctypes.byref(r), ctypes.byref(m), ctypes.byref(p))
    return p.value


# (curves, H, W, bucket capacity, longest list: low, high)
VIEW_CASES = {"short_48x32": (12, 32, 48, 1024, 1, 256), "long_48x32": (120, 32, 48, 1024, 257, 1024),
              "long_41x27": (120, 27, 41, 1024, 257, 1024)}


@pytest.mark.parametrize("name", list(VIEW_CASES))
def test_view_entry_points_match_the_oracle_chain(name):
    """smoke()'s view-path check (the same calls, the same bounds) on small images whose longest list is held to one side of
    the fused path's limit."""
    from oracle import torch_ref as TR
    Bc, Hv, Wv, cap, lo, hi = VIEW_CASES[name]
    cam = S.make_camera((0.5, -1.6, 0.7), (0.5, 0.5, 0.5), (0, 0, 1), Hv, Wv)
    curves = S.make_curves(Bc, 5)
    curves["width"] = curves["width"] + 0.8
    dcol = torch.randn(1, Hv, Wv, generator=torch.Generator().manual_seed(0))
    leaves = [curves[k].clone().requires_grad_(True) for k in ("curve_points", "width", "opacity")]
    xyz, rot, scl = TR.prepare_scaling_rot(leaves[0], leaves[1], curves["is_bezier"])
    Pc = xyz.shape[0]
    rotn = torch.nn.functional.normalize(rot)
    opac = torch.sigmoid(leaves[2]).repeat_interleave(12, 0)
    amap = TR.build_all_map(rot.detach(), xyz.detach(), cam.camera_center, cam.world_view_transform).float().contiguous()
    tfx, tfy = tanfov(cam)
    n = lambda t: np.ascontiguousarray(t.detach().numpy())
    fw = ORA.forward(np.zeros(3, np.float32), n(xyz), np.ones((Pc, 1), np.float32), n(opac), n(scl), n(rotn), 1.0, None,
                     n(amap), n(cam.world_view_transform), n(cam.full_proj_transform), tfx, tfy, Hv, Wv, None, 0,
                     n(cam.camera_center))
    try:
        gr = ORA.backward(fw, dcol.numpy(), None, None)
        t = lambda a: torch.from_numpy(np.asarray(a, np.float32))
        ((xyz * t(gr["dL_dmeans3D"])).sum() + (scl * t(gr["dL_dscales"])).sum() + (rotn * t(gr["dL_drotations"])).sum()
         + (opac * t(gr["dL_dopacity"])).sum()).backward()
        vc = _ViewCalls(curves["curve_points"], curves["width"], curves["opacity"], curves["is_bezier"], cam, cap)
        vc.forward()
        tiles = ((Wv + 15) // 16) * ((Hv + 15) // 16)
        o = util.carve_offsets(vc.img.data_ptr(), [(Hv * Wv, 4), (Hv * Wv, 4), (tiles, 8)])
        ranges = vc.img[o[2]:o[2] + tiles * 8].cpu().numpy().view(np.uint32).reshape(tiles, 2).astype(np.int64)
        longest = int((ranges[:, 1] - ranges[:, 0]).max())
        print(f"\n   {name}: list lengths {(ranges[:, 1] - ranges[:, 0]).tolist()}")
        assert lo <= longest <= hi, (name, longest)
        assert_close("view color", vc.color.cpu().numpy(), fw.color, outlier_frac=2e-3)
        gbuf = [vc.f32(Bc, 4, 3), vc.f32(Bc, 1), vc.f32(Bc, 1)]
        vc.backward(dcol.to(DEV), *gbuf, 0)
        for gname, got, leaf in zip(("curve_points", "width", "opacity"), gbuf, leaves):
            rel = float((got.cpu() - leaf.grad).norm() / leaf.grad.norm())
            print(f"   {name}: dL/d{gname} relative L2 error {rel:.2e}")
            assert rel < 2e-3, f"view path dL/d{gname}: relative L2 error {rel:.2e}"
    finally:
        fw.free()
