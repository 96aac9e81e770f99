"""GPU: cgs_thin_masks (csrc/edge_thin.hip) against the host back end of ops.edge_thin, bit for bit -- at the tile's borders,
over more iterations than one pass holds, under every iteration cap around a pass, with views that settle at different
times, with garbage in its scratch -- and the ``thin`` option of the three operators on both back ends."""
import ctypes
import functools
import itertools

import numpy as np
import pytest
import torch

import edge_dir_cases as DC
import edge_score_cases as EC
import edge_support_cases as SPC
import edge_thin_cases as C
from curve_gaussian_amd import _lib as L
from curve_gaussian_amd.edge_extraction import reprojection as RP
from curve_gaussian_amd.ops import edge_seed as SD
from curve_gaussian_amd.ops import edge_support as SP
from curve_gaussian_amd.ops import edge_thin as ET

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TH, TW, K = L.THIN_TILE_HEIGHT, L.THIN_TILE_WIDTH, L.THIN_PASS_ITERATIONS   # the tile is TH rows by TW columns
HEIGHTS = [1, 2, 3, TH - 1, TH, TH + 1, 2 * TH + 3]
WIDTHS = [1, 33, TW + 1, 3 * TW - 1]
BIG = (2 * TH + 3, 3 * TW - 1)


def _gpu(masks, max_iterations=0):
    """cgs_thin_masks itself on a copy of ``masks`` (uint8 [V,H,W] array), scratch and flag filled with 0xFF:
    (uint8 [V,H,W] CPU tensor, iterations, passes)."""
    work = torch.from_numpy(np.ascontiguousarray(masks)).to(DEV)
    V, H, W = work.shape
    scratch = torch.full_like(work, 0xFF)
    flag = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    n = ctypes.c_int(-1)
    passes = L.load().cgs_thin_masks(V, H, W, L.ptr(work), L.ptr(scratch), L.ptr(flag), max_iterations, ctypes.byref(n),
                                     L.raw_stream(DEV))
    L.check(passes, "cgs_thin_masks")
    return work.cpu(), n.value, passes


def _host(masks, max_iterations=0):
    return ET.thin_masks(masks, backend="host", max_iterations=max_iterations, return_iterations=True)


def _assert_equals_host(masks, max_iterations=0, what=""):
    want, want_n = _host(masks, max_iterations)
    got, got_n, passes = _gpu(masks, max_iterations)
    assert torch.equal(got, want), what
    assert got_n == want_n, what
    return want, want_n, passes


@functools.lru_cache(maxsize=None)
def _disc():
    """A filled disc wider than 4 K + 2 pixels, across a tile corner: more iterations than one pass holds."""
    d = C.disc((TH + 40, TW + 40), (TH + 3, TW - 2), 2 * K + 9)
    assert d.sum(1).max() > 4 * K + 2
    return d


@functools.lru_cache(maxsize=None)
def _noise():
    return C.random_mask((TH + 17, 2 * TW + 5), 0.6)


# ------------------------------------------------------------------------------------------------ tile borders
@pytest.mark.parametrize("density", C.DENSITIES)
def test_random_masks_of_every_size_around_the_tile(density):
    views = itertools.cycle([1, 3, 5])
    changed = 0
    for H in HEIGHTS:
        for W in WIDTHS:
            V = next(views)
            masks = np.stack([C.random_mask((H, W), density, seed=v) for v in range(V)])
            want, _, _ = _assert_equals_host(masks, what=f"{V} x {H} x {W}")
            changed += int(masks.sum() - want.sum())
    assert changed > 0


def test_strokes_across_tile_corners_along_tile_edges_and_along_the_border():
    H, W = BIG
    views = []
    for width in range(1, 10):
        m = np.zeros(BIG, np.uint8)
        C.draw_stroke(m, (TH - 30, TW - 30), (TH + 30, TW + 30), width)            # across a tile corner
        C.draw_stroke(m, (2 * TH + 2, 2 * TW - 20), (2 * TH - 25, 2 * TW + 9), width)   # across another, the other way
        C.draw_stroke(m, (TH, 3), (TH, W - 4), width)                               # along a tile's first row
        C.draw_stroke(m, (TH + 60, TW - 1), (2 * TH - 40, TW - 1), width)           # along a tile's last column
        C.draw_stroke(m, (0, 0), (0, W - 1), width)                                 # along the image border
        C.draw_stroke(m, (H - 1, 5), (H - 1, W - 1), width)
        C.draw_stroke(m, (20, 0), (TH - 50, 0), width)
        C.draw_stroke(m, (TH + 50, W - 1), (H - 20, W - 1), width)
        views.append(m)
    want, n, _ = _assert_equals_host(np.stack(views))
    assert n > 2 and 0 < want.sum() < np.stack(views).sum()


# ------------------------------------------------------------------------------------------------ passes
def test_more_iterations_than_one_pass_holds():
    ones = np.ones((1, 2 * TH + 3, TW + 1), np.uint8)
    _, n, passes = _assert_equals_host(ones)
    assert n > 2 * K and passes >= 3, (n, passes)
    _, n, passes = _assert_equals_host(_disc()[None])
    assert n > K and passes >= 2, (n, passes)


@pytest.mark.parametrize("max_iterations", sorted({1, 2, K - 1, K, K + 1, 2 * K + 1}))
def test_every_iteration_cap_around_a_pass(max_iterations):
    for name, mask in (("disc", _disc()), ("noise", _noise())):
        _, n, passes = _assert_equals_host(mask[None], max_iterations, name)
        assert n <= max_iterations and passes == -(-n // K), (name, n, passes)   # a pass holds K iterations
    assert _host(_disc()[None], max_iterations)[1] == max_iterations, "the disc needs more iterations than any of these caps"


def test_views_that_settle_at_different_times():
    shape = _disc().shape
    pixel = np.zeros(shape, np.uint8)
    pixel[TH, TW] = 1
    views = [np.zeros(shape, np.uint8), pixel, _disc()]
    alone = [_host(v[None])[0][0] for v in views]
    for order in itertools.permutations(range(3)):
        want, _, _ = _assert_equals_host(np.stack([views[i] for i in order]), what=str(order))
        for k, i in enumerate(order):
            assert torch.equal(want[k], alone[i])
    assert torch.equal(alone[1], torch.from_numpy(pixel)) and not alone[0].any()


# ------------------------------------------------------------------------------------------------ determinism and reuse
def test_the_same_call_twice_and_bytes_that_are_not_0_or_1():
    masks = np.stack([_noise(), C.stroke_field(_noise().shape, 30, seed=1)])
    first, second = _gpu(masks), _gpu(masks)
    assert torch.equal(first[0], second[0]) and first[1:] == second[1:]
    loud = masks * np.random.default_rng(0).integers(1, 256, masks.shape).astype(np.uint8)
    assert loud.max() > 1
    got = _gpu(loud)
    assert torch.equal(got[0], first[0]) and got[1:] == first[1:]
    # a settled input of bytes 255: one pass, one iteration, nothing changes -- and the result is still 0 / 1
    line = np.zeros((1, TH + 5, TW + 5), np.uint8)
    line[0, TH - 1, :] = 255
    out, n, passes = _gpu(line)
    assert (n, passes) == (1, 1) and torch.equal(out, torch.from_numpy(line // 255))


def test_the_operator_leaves_its_input_and_stays_on_the_device():
    masks = torch.from_numpy(np.stack([_disc(), _disc() * np.uint8(7)]))
    want, want_n = _host(masks)
    on_dev = masks.to(DEV)
    out, n = ET.thin_masks(on_dev, return_iterations=True)
    assert out.device == on_dev.device and out.dtype == torch.uint8 and torch.equal(on_dev.cpu(), masks)
    assert torch.equal(out.cpu(), want) and n == want_n
    assert torch.equal(ET.thin_masks(masks.numpy().astype(bool), device=DEV).cpu(), want)
    empty, n0 = ET.thin_masks(torch.zeros((0, 3, 4), dtype=torch.uint8), device=DEV, return_iterations=True)
    assert tuple(empty.shape) == (0, 3, 4) and n0 == 0


def test_one_larger_case():
    masks = np.stack([C.stroke_field((600, 800), 300, seed=s) for s in (2, 3)])
    want, n, passes = _assert_equals_host(masks)
    assert 0 < want.sum() < masks.sum() and n >= 4


# ------------------------------------------------------------------------------------------------ the operators
def test_edge_support_thinned_on_both_back_ends():
    cams, maps = C.thick_scan(2)
    kw = dict(resolution=EC.SCAN_RESOLUTION, keep_tolerance_px=2, min_visible=0.5, min_near=0.8,
              frames_ratio=SPC.SCAN_FRAMES_RATIO, thin=True)
    host = SP.edge_support(SPC.scan_edges()[0], cams, maps, "PidiNet", backend="host", **kw)
    per_view = SP.BYTES_PER_PIXEL * DC.DIR_H * DC.DIR_W
    for budget in (None, 1, 5 * per_view):
        gpu = SP.edge_support(SPC.scan_edges()[0], cams, maps, "PidiNet", backend="gpu", budget_bytes=budget, **kw)
        assert torch.equal(gpu["counts"], host["counts"]) and np.array_equal(gpu["kept"], host["kept"]), budget
        assert gpu["settings"]["thin"] is True
    assert np.array_equal(host["kept"], SPC.scan_edges()[1])


def test_score_edges_thinned_on_both_back_ends():
    cams, maps = C.thick_scan(2)
    kw = dict(sample_resolution=EC.SCAN_RESOLUTION, thin=True)
    host = RP.score_edges(EC.SCAN_EDGES, cams, maps, "PidiNet", backend="host", **kw)
    gpu = RP.score_edges(EC.SCAN_EDGES, cams, maps, "PidiNet", backend="gpu", **kw)
    for key in ("precision", "recall", "fscore", "chamfer_views", "views", "n_pred", "n_det"):
        assert gpu["aggregate"][key] == host["aggregate"][key], key
    for key in ("accuracy_px", "completeness_px", "chamfer_px"):
        assert gpu["aggregate"][key] == pytest.approx(host["aggregate"][key], rel=1e-11, abs=0.0), key
    for a, b in zip(gpu["views"], host["views"]):
        for key in ("name", "kept_points", "n_pred", "n_det", "pred_hits", "det_hits", "both_nonempty"):
            assert a[key] == b[key], key
    assert gpu["settings"]["thin"] is True


def test_seed_points_thinned_on_both_back_ends():
    cams, maps = C.thick_scan(2)
    kw = dict(thin=True, **DC.DIR_OPTIONS)
    host, host_info = SD.seed_points(cams, maps, "PidiNet", DC.DIR_BOUNDS, backend="host", **kw)
    gpu, gpu_info = SD.seed_points(cams, maps, "PidiNet", DC.DIR_BOUNDS, backend="gpu", **kw)
    assert len(host) > 0 and np.array_equal(gpu, host)
    assert {k: v for k, v in gpu_info.items() if k != "backend"} == {k: v for k, v in host_info.items() if k != "backend"}
