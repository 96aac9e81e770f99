"""Host: ops.view_chunks, the driver that score_edges, edge_support, seed_points and render_views share -- the chunks
against the loop that every one of them used to write out, the two argument checks, the detected masks, and the drivers'
independence of the chunking on the host back end.  (edge_support at one view per chunk: test_edge_support_cpu
test_chunking_the_views_changes_nothing; seed_points with the claims and the directions: test_edge_excl_cpu
test_chunking_the_second_sweep_changes_nothing.)"""
import numpy as np
import pytest

import edge_score_cases as EC
import edge_seed_cases as SC
from curve_gaussian_amd.edge_extraction.novel_view import NovelViewCamera
from curve_gaussian_amd.ops import view_chunks as VC

SIZES = {"A": (6, 8), "B": (5, 7), "C": (3, 4)}   # (H, W)
ORDER = "ABACBAA"


def _cameras(order=ORDER):
    rng = np.random.default_rng(4)
    return [NovelViewCamera(f"{k}{s}", rng.normal(size=(3, 3)), rng.normal(size=3), *rng.uniform(1, 9, 4), SIZES[s][1], SIZES[s][0])
            for k, s in enumerate(order)]


def _old_loop(cameras, bytes_per_pixel, budget):
    """The loop as score_edges, edge_support, seed_points and render_views each wrote it before view_chunks."""
    out = []
    by_size = {}
    for v, c in enumerate(cameras):
        by_size.setdefault((c.height, c.width), []).append(v)
    for (H, W), idx in by_size.items():
        per = max(1, budget // (bytes_per_pixel * H * W))
        for b in range(0, len(idx), per):
            sel = idx[b:b + per]
            intr = np.array([[cameras[v].fx, cameras[v].fy, cameras[v].cx, cameras[v].cy] for v in sel], np.float64).reshape(-1, 4)
            w2c = np.array([np.concatenate([cameras[v].R, cameras[v].T[:, None]], 1) for v in sel], np.float64).reshape(-1, 3, 4)
            out.append((H, W, sel, intr, w2c))
    return out


@pytest.mark.parametrize("per", [1, 2, "all"])
def test_chunks_are_those_of_the_old_loop(per):
    cams, bpp = _cameras(), 7
    budget = 1 << 30 if per == "all" else per * bpp * 6 * 8   # `per` views of the largest size, A, and as many of B
    got, want = list(VC.view_chunks(cams, bpp, budget)), _old_loop(cams, bpp, budget)
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g[:3] == w[:3] and isinstance(g[2], list)
        for a, b in zip(g[3:], w[3:]):
            assert a.dtype == b.dtype == np.float64 and a.shape == b.shape and a.tobytes() == b.tobytes()
    sels = [g[2] for g in got]
    assert [(g[0], g[1]) for g in got if g[2][0] in (0, 1, 3)] == [SIZES["A"], SIZES["B"], SIZES["C"]], "first-seen order"
    if per == 1:
        assert sels == [[0], [2], [5], [6], [1], [4], [3]]
    elif per == 2:
        assert sels == [[0, 2], [5, 6], [1, 4], [3]]
    else:
        assert sels == [[0, 2, 5, 6], [1, 4], [3]]


def test_a_small_budget_and_no_camera():
    cams = _cameras()
    assert [g[2] for g in VC.view_chunks(cams, 12, 1)] == [[0], [2], [5], [6], [1], [4], [3]], "at least one view"
    assert list(VC.view_chunks([], 12, 1 << 30)) == []
    assert VC.check_budget("f", None, 5) == 5 and VC.check_budget("f", 7.9, 5) == 7
    for bad in (0, -3):
        with pytest.raises(ValueError, match="f: budget_bytes must be positive"):
            VC.check_budget("f", bad, 5)


def test_check_edge_maps():
    cams = _cameras("AB")
    maps = [np.zeros(SIZES["A"], np.uint8), np.zeros(SIZES["B"], np.uint8)]
    got_cams, got_maps = VC.check_edge_maps("f", iter(cams), maps)
    assert got_cams == cams and all(a is b for a, b in zip(got_maps, maps))
    with pytest.raises(ValueError, match="my_op: 2 cameras and 1 edge maps"):
        VC.check_edge_maps("my_op", cams, maps[:1])
    with pytest.raises(ValueError, match=r"my_op: the edge map of 1B must be uint8 \[5,7\] \(got float32"):
        VC.check_edge_maps("my_op", cams, [maps[0], maps[1].astype(np.float32)])
    with pytest.raises(ValueError, match=r"my_op: the edge map of 0A must be uint8 \[6,8\] \(got uint8 \(5, 7\)\)"):
        VC.check_edge_maps("my_op", cams, [maps[1], maps[1]])


@pytest.mark.parametrize("detector", ["DexiNed", "PidiNet"])
def test_detected_masks(detector):
    rng = np.random.default_rng(8)
    maps = [rng.integers(0, 256, (5, 7), dtype=np.uint8) for _ in range(4)]
    lut = VC.detected_lut(detector, 0.5)
    got = VC.detected_masks(lut, maps, [3, 1])
    want = lut[np.stack([maps[3], maps[1]])].astype(np.uint8)
    assert got.numpy().dtype == np.uint8 and tuple(got.shape) == (2, 5, 7)
    assert np.array_equal(got.numpy(), want) and 0 < want.sum() < want.size


def test_score_edges_does_not_depend_on_the_chunks():
    """The six-view drawn scan, one view per chunk against all six in one.  Every integer is equal; the two distance sums
    (a view's accuracy_px and completeness_px, and the aggregate built from them) are compared as test_edge_score_gpu
    compares them across chunkings, by their repr."""
    from curve_gaussian_amd.edge_extraction import reprojection as RP
    cams, maps = SC.seed_novel_cameras()
    kw = dict(sample_resolution=EC.SCAN_RESOLUTION, backend="host")
    whole = RP.score_edges(EC.SCAN_EDGES, cams, maps, "PidiNet", **kw)
    single = RP.score_edges(EC.SCAN_EDGES, cams, maps, "PidiNet", budget_bytes=1, **kw)
    assert len(whole["views"]) == len(single["views"]) == 6 and whole["settings"] == single["settings"]
    floats = ("accuracy_px", "completeness_px")
    for a, b in zip(whole["views"], single["views"]):
        assert {k: v for k, v in a.items() if k not in floats} == {k: v for k, v in b.items() if k not in floats}
        assert all(repr(a[k]) == repr(b[k]) for k in floats)
        assert a["n_pred"] > 0 and a["n_det"] > 0
    assert repr(whole["aggregate"]) == repr(single["aggregate"]) and whole["aggregate"]["chamfer_views"] == 6
