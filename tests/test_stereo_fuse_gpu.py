"""GPU: the fusion kernels (cgs_stereo_warp / cgs_stereo_fuse, csrc/stereo_fuse.hip) against the host back end of
ops.stereo_depth bit for bit -- every case of the CPU tests, a spread of shapes with all ranges, crowded target pixels,
mixed sizes and chunks through the Python layer -- the raw entries' argument checks, and the box arc end to end."""
import ctypes

import numpy as np
import pytest
import torch

import stereo_fuse_cases as FC
from curve_gaussian_amd import _lib
from curve_gaussian_amd.ops import stereo_depth as SD
from curve_gaussian_amd.scene import solid_scan as SS

pytestmark = pytest.mark.gpu


def both_warps(c, v0, nv):
    args = (c["depth"], c["K"], c["fsrc"], c["into"], v0, nv)
    return SD.warp(*args, backend="gpu").cpu().numpy(), SD.warp(*args, backend="host").numpy()


def check_case(c, supports, ranges=None):
    """warp and fuse on both back ends over the ranges; returns the fused maps of the last one."""
    V, F = c["fsrc"].shape
    out = None
    for v0, nv in ranges or FC.ranges(V):
        warped, want = both_warps(c, v0, nv)
        assert warped.shape == (nv, F) + c["depth"].shape[1:] and FC.same_bits(warped, want), (v0, nv)
        for n in supports:
            out, sup = SD.fuse(c["depth"], warped, c["tol"], n, v0, backend="gpu", return_support=True)
            out_h, sup_h = SD.fuse(c["depth"], want, c["tol"], n, v0, backend="host", return_support=True)
            out, sup = out.cpu().numpy(), sup.cpu().numpy()
            assert FC.same_bits(out, out_h.numpy()) and (sup == sup_h.numpy()).all(), (v0, nv, n)
            plain = SD.fuse(c["depth"], warped, c["tol"], n, v0, backend="gpu")          # support = NULL
            assert FC.same_bits(plain.cpu().numpy(), out), (v0, nv, n)
    return out


@pytest.mark.parametrize("F", [1, 3, 16])
@pytest.mark.parametrize("H,W", [(1, 1), (5, 7), (9, 11)])
@pytest.mark.parametrize("V", [1, 2, 5])
def test_equals_host_on_the_cpu_matrix(V, H, W, F):
    check_case(FC.random_case(V, H, W, F, 10 * V + H + F), (1, 2, 3, F + 1, F + 2))


# sizes 1x1, 5x7, 24x32, 33x65 (no multiple of the 16 x 16 tile or of the 256-pixel block); V: 1 and 5; F: 1, 3, 16
SHAPES = [(5, 33, 65, 16), (5, 24, 32, 3), (1, 33, 65, 1), (5, 5, 7, 16), (1, 24, 32, 16), (5, 33, 65, 3), (5, 1, 1, 3),
          (1, 1, 1, 1), (5, 24, 32, 1), (1, 5, 7, 3), (5, 17, 16, 3)]


@pytest.mark.parametrize("V,H,W,F", SHAPES)
def test_equals_host_across_shapes(V, H, W, F):
    out = check_case(FC.random_case(V, H, W, F, 3 * H + F + V), (1, 3, F + 2))
    assert not out.any()                                                # the last range, min_support = F + 2


def test_exact_and_named_cases():
    c = FC.exact_case()
    hole, odd, alone = (dict(c, depth=c["depth"].copy()) for _ in range(3))
    hole["depth"][1, 3, 4], odd["depth"][1, 3, 4] = 0.0, 1.0
    alone["depth"][[0, 2]] = 0.0
    for case in (c, hole, odd, alone):
        check_case(case, (1, 2, 3))
    out = SD.fuse(hole["depth"], both_warps(hole, 0, 3)[0], hole["tol"], 2, backend="gpu").cpu().numpy()
    assert out[1, 3, 4] == np.float32(2.0)
    for row, T in (([2.0, 1.0, 0.0, 0.0], (0.0, 0.0, 2.0)), ([1.0, 2.0, 0.0, 0.0], (0.0, 0.0, 2.0)), ([2.0] * 5, (1.0, 0.0, 0.0)),
                   ([2.0] * 5, (0.0, 0.0, -5.0)), ([2.0] * 5, (0.0, 0.0, -2.0))):
        check_case(FC.two_views(row, T), (1,), [(0, 1), (0, 2)])
    assert both_warps(FC.two_views([2.0, 1.0, 0.0, 0.0], (0.0, 0.0, 2.0)), 0, 1)[0][0, 0, 0, 0] == np.float32(3.0)
    assert np.isinf(both_warps(FC.two_views([2.0] * 5, (1.0, 0.0, 0.0)), 0, 1)[0][0, 0, 0, 0])


@pytest.mark.parametrize("own,others,tol", [(2.0, [2.0, 4.0, 4.0], 0.01), (4.0, [2.0, 4.0, 2.0], 0.01), (0.0, [2.0, 4.0], 0.01),
                                            (2.0, [2.0, 2.0000002, 4.0], 0.0), (2.0, [2.0] * 16, 0.0),
                                            (2.0, [4.0, 0.0, 4.0, float("inf"), float("nan"), -3.0], float("inf")),
                                            (2.0, [2.0, 2.0], float("nan")), (2.0, [2.0, 2.0], -1.0), (3.0, [float("inf")], 0.01)])
def test_pixels_by_hand(own, others, tol):
    depth, warped, tol = FC.pixel_case(own, others, tol)
    for n in (1, 2, len(others) + 1, len(others) + 2):
        out, sup = SD.fuse(depth, warped, tol, n, backend="gpu", return_support=True)
        want, want_sup = SD.fuse(depth, warped, tol, n, backend="host", return_support=True)
        assert FC.same_bits(out.cpu().numpy(), want.numpy()) and (sup.cpu().numpy() == want_sup.numpy()).all()


def test_crowded_target_pixels():
    """Sources much farther away: a whole map lands on a few target pixels, so the atomic minimum decides most of them."""
    c = FC.crowded_case()
    warped, want = both_warps(c, 0, 3)
    assert FC.same_bits(warped, want)
    landed = int(np.isfinite(warped).sum())
    assert 0 < landed < 0.1 * int((c["fsrc"] >= 0).sum()) * 24 * 32
    check_case(c, (1, 2), [(0, 3)])


def test_mixed_sizes_and_chunks_through_the_python_layer(monkeypatch):
    small = SS.solid_scan("box", 3, 24, 32, synth_cameras=SS.arc_cameras(3, 24, 32))
    large = SS.solid_scan("box", 2, 33, 65, synth_cameras=SS.arc_cameras(2, 33, 65))
    cams = [small.cameras[0], large.cameras[0], small.cameras[1], large.cameras[1], small.cameras[2]]
    mesh = lambda d: np.where(np.isfinite(d), d, 0.0).astype(np.float32)
    maps = [mesh(small.depth[0]), mesh(large.depth[0]), mesh(small.depth[1]), mesh(large.depth[1]), mesh(small.depth[2])]
    kw = dict(hypotheses=12, fuse_sources=2, min_support=2, return_info=True)
    (gpu, info), (host, info_h) = SD.fuse_depth(maps, cams, backend="gpu", **kw), SD.fuse_depth(maps, cams, backend="host", **kw)
    assert all(FC.same_bits(a, b) for a, b in zip(gpu, host)) and info == info_h and all((m > 0).any() for m in gpu)
    for targets in (1, 2):
        monkeypatch.setattr(SD, "FUSE_CHUNK_BYTES", targets * 2 * 24 * 32 * 4)      # (one target of the larger size at least)
        parts, info_p = SD.fuse_depth(maps, cams, backend="gpu", **kw)
        assert all(FC.same_bits(a, b) for a, b in zip(parts, host)) and info_p == info_h


# ------------------------------------------------------------------------------------------------ the raw entries
def test_raw_entries():
    lib = _lib.load()
    c = FC.random_case(3, 9, 11, 3, 60)
    dev = torch.device("cuda", torch.cuda.current_device())
    t = {k: torch.from_numpy(np.ascontiguousarray(c[k])).to(dev) for k in ("depth", "K", "fsrc", "into", "tol")}
    before = t["depth"].clone()
    warped = torch.full((2, 3, 9, 11), -7.0, dtype=torch.float32, device=dev)
    out = torch.full((2, 9, 11), -7.0, dtype=torch.float32, device=dev)
    sup = torch.full((2, 9, 11), 99, dtype=torch.uint8, device=dev)
    p, s = _lib.ptr, _lib.raw_stream(dev)
    at = lambda x, n: ctypes.c_void_p(x.data_ptr() + n)

    def untouched(*tensors):
        torch.cuda.synchronize()
        return torch.equal(t["depth"].view(torch.int32), before.view(torch.int32)) and all(
            bool((x == (99 if x.dtype == torch.uint8 else -7.0)).all()) for x in tensors)

    good = [3, 9, 11, p(t["depth"]), p(t["K"]), 3, p(t["fsrc"]), p(t["into"]), 1, 2, p(warped), s]
    for pos, bad in ((0, -1), (1, 0), (2, _lib.EDT_MAX_SIZE + 1), (3, None), (4, None), (5, 0), (5, 17), (6, None), (7, None),
                     (8, -1), (8, 2), (9, -1), (9, 3), (10, None), (10, p(t["depth"])), (10, at(t["depth"], 4 * 50)),
                     (3, at(warped, 4 * 100))):
        args = list(good)
        args[pos] = bad
        assert lib.cgs_stereo_warp(*args) == -1, (pos, bad)
        assert _lib.last_error().startswith("cgs_stereo_warp: invalid argument") and untouched(warped), (pos, bad)
    args = list(good)
    args[9] = 0
    assert lib.cgs_stereo_warp(*args) == 0 and untouched(warped)       # nv = 0 is a no-op
    assert lib.cgs_stereo_warp(*good) == 0
    torch.cuda.synchronize()
    want = SD.warp(c["depth"], c["K"], c["fsrc"], c["into"], 1, 2, backend="host").numpy()
    assert FC.same_bits(warped.cpu().numpy(), want)
    kept = warped.clone()

    good = [3, 9, 11, p(t["depth"]), 3, p(warped), p(t["tol"]), 2, 1, 2, p(out), p(sup), s]
    for pos, bad in ((0, -1), (1, 0), (2, 0), (3, None), (4, 0), (4, 17), (5, None), (6, None), (7, 0), (8, -1), (8, 2), (9, -1),
                     (9, 3), (10, None), (10, p(t["depth"])), (10, at(warped, 4 * 10)), (11, at(t["depth"], 7)), (11, at(warped, 0)),
                     (11, at(out, 4 * 2 * 99 - 1))):
        args = list(good)
        args[pos] = bad
        assert lib.cgs_stereo_fuse(*args) == -1, (pos, bad)
        assert _lib.last_error().startswith("cgs_stereo_fuse: invalid argument") and untouched(out, sup), (pos, bad)
        assert torch.equal(warped.view(torch.int32), kept.view(torch.int32)), (pos, bad)
    args = list(good)
    args[9] = 0
    assert lib.cgs_stereo_fuse(*args) == 0 and untouched(out, sup)
    assert lib.cgs_stereo_fuse(*good) == 0
    torch.cuda.synchronize()
    want_out, want_sup = SD.fuse(c["depth"], want, c["tol"], 2, 1, backend="host", return_support=True)
    assert FC.same_bits(out.cpu().numpy(), want_out.numpy()) and (sup.cpu().numpy() == want_sup.numpy()).all()
    assert untouched() and torch.equal(warped.view(torch.int32), kept.view(torch.int32))
    out.fill_(-7.0)
    args = list(good)
    args[11] = None                                                     # support = NULL
    assert lib.cgs_stereo_fuse(*args) == 0
    torch.cuda.synchronize()
    assert FC.same_bits(out.cpu().numpy(), want_out.numpy())


# ------------------------------------------------------------------------------------------------ end to end
def test_box_arc_end_to_end():
    from curve_gaussian_amd.edge_extraction.reprojection import score_edges
    scan = SS.solid_scan("box", 8, 48, 64, backend="host", synth_cameras=SS.arc_cameras(8, 48, 64))
    photos = list(SS.photographs(scan))
    kw = dict(hypotheses=32, patch_radius=2, sources=2, return_info=True, fuse=True)
    (gpu, info), (host, info_h) = SD.stereo_depth(photos, scan.cameras, backend="gpu", **kw), \
        SD.stereo_depth(photos, scan.cameras, backend="host", **kw)
    assert all(FC.same_bits(a, b) for a, b in zip(gpu, host)) and info == info_h and min(info["coverage"]) > 0
    assert info["fusion"]["filled"] > 0
    rows = []
    for backend, maps in (("gpu", gpu), ("host", host)):
        res = score_edges(scan.edges, scan.cameras, scan.maps, "PidiNet", backend=backend, depth_maps=maps,
                          depth_slack=info["recommended_slack"])
        rows.append([(r["kept_points"], r["hidden_points"], r["n_pred"], r["n_det"], r["pred_hits"], r["det_hits"])
                     for r in res["views"]])
        assert res["settings"]["depth_maps"] is True
    assert rows[0] == rows[1] and sum(r[1] for r in rows[0]) > 0
