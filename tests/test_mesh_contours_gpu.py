"""GPU: cgs_mesh_contours (csrc/mesh_contours.hip) against the host back end of ops.mesh_contours, bit for bit -- the
hand-made tents, the solids with and without the plane for both kinds, row counts around a wave and a workgroup, waves
whose rows are all contours or none, segments longer than a wave and shorter than a step, different cameras in one launch,
two chunkings of the views, and the score with the don't-care zone."""
import numpy as np
import pytest
import torch

import mesh_contours_cases as C
from curve_gaussian_amd import synthetic
from curve_gaussian_amd.edge_extraction import reprojection as R
from curve_gaussian_amd.ops import edge_occlusion as EO
from curve_gaussian_amd.ops import mesh_contours as MC
from curve_gaussian_amd.ops.view_chunks import camera_arrays
from curve_gaussian_amd.scene import solid_scan as SS
from test_mesh_contours_cpu import SCAN_H, SCAN_VIEWS, SCAN_W, check_contour_scores

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _np(t):
    return t.cpu().numpy()


def _both(rows, K, M, H, W, depth=None, slack=0.001):
    """The GPU masks, checked against the host's bit for bit."""
    host = MC.row_masks(rows, K, M, H, W, depth=depth, slack=slack, backend="host").numpy()
    got = MC.row_masks(rows, K, M, H, W, depth=depth, slack=slack)
    assert got.is_cuda and got.dtype == torch.uint8 and C.same_bits(_np(got), host)
    return host


@pytest.mark.parametrize("name", sorted(C.HAND_CASES))
def test_hand_made_cases(name):
    row, eye, want = C.HAND_CASES[name]
    K, M = C.camera(eye)
    assert C.same_bits(_np(MC.row_masks(row, K, M, C.H, C.W))[0], want), name


def test_a_ridge_behind_a_nearer_quad_and_the_winding():
    K, M = C.camera(C.EYE_SIDE)
    plane = EO.mesh_depth(C.QUAD, K, M, C.H, C.W, window=0)
    assert C.same_bits(_np(MC.row_masks(C.tent_row(), K, M, C.H, C.W, depth=plane, slack=0.001))[0], C.BEHIND_QUAD_WITH_PLANE)
    assert C.same_bits(_np(MC.row_masks(C.tent_row(), K, M, C.H, C.W))[0], C.BEHIND_QUAD_WITHOUT)
    K3, M3 = C.cameras([C.EYE_SIDE, C.EYE_FRONT, C.EYE_EDGE_ON])
    want = MC.contour_masks(C.tent_tris(), K3, M3, C.H, C.W, kind="all", backend="host").numpy()
    for flip_c in (False, True):
        for flip_d in (False, True):
            got = MC.contour_masks(C.tent_tris(flip_c, flip_d), K3, M3, C.H, C.W, kind="all")
            assert C.same_bits(_np(got), want), (flip_c, flip_d)


@pytest.mark.parametrize("shape", SS.SHAPES)
def test_the_solids_with_and_without_the_plane(shape):
    tris, _ = SS.solid_geometry(shape)
    intr, w2c = camera_arrays(SS.emap_cameras_of(synthetic.fibonacci_cameras(SCAN_VIEWS, SCAN_H, SCAN_W)))
    plane = EO.mesh_depth(tris, intr, w2c, SCAN_H, SCAN_W, backend="host")
    for kind in MC.KINDS:
        for depth in (None, plane):
            host = MC.contour_masks(tris, intr, w2c, SCAN_H, SCAN_W, depth=depth, kind=kind, backend="host").numpy()
            got = MC.contour_masks(tris, intr, w2c, SCAN_H, SCAN_W, depth=depth, kind=kind)
            assert C.same_bits(_np(got), host), (kind, depth is None)
            assert bool(host.any()) == (kind == "all" or shape == "cylinder")


@pytest.mark.parametrize("E", [0, 1, 63, 64, 65, 340])   # 340 = 256 + 64 + 20: a partial wave in the middle of a workgroup
def test_row_counts_around_a_wave_and_a_workgroup(E):
    H, W, V = 24, 32, 3
    K, M = C.cube_cameras(V, H, W)
    plane = EO.mesh_depth(SS.solid_geometry("box")[0], K, M, H, W, backend="host")
    free = _both(C.random_rows(E), K, M, H, W)
    gated = _both(C.random_rows(E), K, M, H, W, depth=plane)
    assert (E < 63) or 0 < gated.sum() < free.sum()
    rows_dev = torch.from_numpy(C.random_rows(E)).to(DEV)   # rows already on the device
    assert C.same_bits(_np(MC.row_masks(rows_dev, K, M, H, W)), free)
    assert MC.row_masks(C.random_rows(E), K[:0], M[:0], H, W).shape == (0, H, W)   # V = 0


def test_waves_of_all_contours_and_of_none():
    K, M = C.camera(C.EYE_SIDE)
    every = _both(C.fan(64, lambda i: True), K, M, C.H, C.W)
    assert every.any() and not _both(C.fan(64, lambda i: False), K, M, C.H, C.W).any()
    # 192 rows: a wave of contours, a wave of none, a mixed one
    mixed = C.fan(192, lambda i: i < 64 or (i >= 128 and i % 3 == 0))
    assert MC.contour_flags(mixed, K, M)[0].sum() == 64 + 21
    _both(mixed, K, M, C.H, C.W)


def test_segments_longer_than_a_wave_and_shorter_than_a_step():
    H, W = 120, 160
    K = np.array([[40.0, 40.0, 80.0, 60.0]], np.float64)   # the tent 10 x larger in the image: 60 pixels, 121 steps
    M = C.camera(C.EYE_SIDE)[1]
    long_ = _both(C.tent_row(), K, M, H, W)
    assert long_[0, :, 140].sum() == 61 and long_.sum() == 61, "u = 40 * 1.5 + 80 = 140, v = 30 .. 90"
    clipped = _both(C.tent_row(a=(0.0, -60.0, 2.0)), K, M, H, W)   # enters far above the image
    assert clipped[0, :, 140].sum() == 91 and clipped.sum() == 91
    short = _both(C.tent_row(a=(0.0, 0.0101, 2.0), b=(0.0, 0.0201, 2.0)), K, M, H, W)   # 0.2 pixels long
    assert short.sum() == 1 and short[0, 60, 140] == 1


def test_different_cameras_in_one_launch_and_two_chunkings():
    tris, _ = SS.solid_geometry("cylinder")
    rows = MC.edge_rows(tris, "smooth")
    intr, w2c = camera_arrays(SS.emap_cameras_of(synthetic.fibonacci_cameras(SCAN_VIEWS, SCAN_H, SCAN_W)))
    plane = EO.mesh_depth(tris, intr, w2c, SCAN_H, SCAN_W)
    whole = _np(MC.row_masks(rows, intr, w2c, SCAN_H, SCAN_W, depth=plane))
    assert all(whole[v].any() for v in range(SCAN_VIEWS)) and not C.same_bits(whole[0], whole[1])
    for step in (1, 5):
        parts = [_np(MC.row_masks(rows, intr[v:v + step], w2c[v:v + step], SCAN_H, SCAN_W, depth=plane[v:v + step]))
                 for v in range(0, SCAN_VIEWS, step)]
        assert C.same_bits(np.concatenate(parts), whole), step
    rev = _np(MC.row_masks(rows[::-1].copy(), intr, w2c, SCAN_H, SCAN_W, depth=plane))
    assert C.same_bits(rev, whole), "the order of the rows does not matter"


def test_score_with_the_zone_equals_the_host():
    scans = {(shape, contours): SS.solid_scan(shape, SCAN_VIEWS, SCAN_H, SCAN_W, contours=contours)
             for shape, contours in (("cylinder", False), ("cylinder", True), ("box", True))}
    host = SS.solid_scan("cylinder", SCAN_VIEWS, SCAN_H, SCAN_W, backend="host", contours=True)
    assert C.same_bits(scans["cylinder", True].maps, host.maps) and C.same_bits(scans["cylinder", True].contours, host.contours)
    gpu = check_contour_scores(scans, "gpu")
    want = R.score_edges(host.edges, host.cameras, host.maps, "PidiNet", backend="host", occluder=host.tris,
                         ignore_contours=True)
    assert gpu["views"] == want["views"] and gpu["aggregate"] == want["aggregate"]
    chunked = R.score_edges(host.edges, host.cameras, host.maps, "PidiNet", occluder=host.tris, ignore_contours=True,
                            budget_bytes=1)
    assert chunked["views"] == want["views"]
