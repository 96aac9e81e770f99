"""GPU: cgs_mesh_depth / cgs_depth_window_max / cgs_point_mask_depth (csrc/edge_occlusion.hip) against the host back end of
ops.edge_occlusion and the brute force of edge_occlusion_cases.py, bit for bit -- triangle counts around a wave and a
workgroup, images narrower than a tile and of more than one, every window, sample counts around a wave and a workgroup, two
chunkings of the views in the score, the solids' scores, and the two shapes of 1600 x 1200 that the profile times."""
import itertools

import numpy as np
import pytest
import torch

import edge_occlusion_cases as C
from curve_gaussian_amd import _lib as L
from curve_gaussian_amd import synthetic
from curve_gaussian_amd.edge_extraction import reprojection as R
from curve_gaussian_amd.ops import edge_occlusion as EO
from curve_gaussian_amd.ops import edge_score as ES
from curve_gaussian_amd.ops.view_chunks import camera_arrays
from curve_gaussian_amd.scene import solid_scan as SS
from test_edge_occlusion_cpu import check_solid_score

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)   # a copy: the shared cases are read-only


def _np(t):
    return t.cpu().numpy()


@pytest.mark.parametrize("F", C.FACES)
def test_zbuffer_and_window_equal_the_brute_force_and_the_host(F):
    for W, V in itertools.product(C.WIDTHS, C.VIEWS):
        K, M = C.cameras(V, C.HEIGHT, W)
        want = C.reference_zbuffer(F, W, V)
        raw = EO.mesh_depth(C.triangles(F), K, M, C.HEIGHT, W, window=0)
        assert raw.is_cuda and C.same_bits(_np(raw), want), (W, V)
        for r in C.WINDOWS:
            host = EO.mesh_depth(C.triangles(F), K, M, C.HEIGHT, W, window=r, backend="host").numpy()
            assert C.same_bits(_np(EO.mesh_depth(_dev(C.triangles(F)), K, M, C.HEIGHT, W, window=r)), host), (W, V, r)
            assert C.same_bits(_np(EO.depth_window_max(raw, r)), host), (W, V, r)


def test_window_maximum_over_many_tiles():
    rng = np.random.default_rng(2)
    for H, W in ((1, 1), (17, 65), (40, 130), (33, 64)):
        d = rng.uniform(0.5, 9.0, (3, H, W)).astype(np.float32)
        d[rng.random(d.shape) < 0.05] = np.inf
        for r in range(EO.MAX_WINDOW + 1):
            want = EO.depth_window_max(d, r, backend="host").numpy()
            assert C.same_bits(_np(EO.depth_window_max(d, r)), want), (H, W, r)
            if H * W < 2000:
                assert C.same_bits(want, C.window_max_brute(d, r)), (H, W, r)


@pytest.mark.parametrize("P", C.POINT_COUNTS)
def test_gated_mask_equals_the_host(P):
    pts = C.samples(P)
    for W, V in itertools.product(C.WIDTHS, C.VIEWS):
        K, M = C.cameras(V, C.HEIGHT, W)
        depth = EO.depth_window_max(C.reference_zbuffer(257, W, V), 1, backend="host").numpy()
        for slack in (0.0, 0.01):
            want = EO.point_masks_depth(pts, K, M, depth, slack, backend="host", return_counts=True)
            got = EO.point_masks_depth(_dev(pts), K, M, _dev(depth), slack, return_counts=True)
            assert all(g.is_cuda for g in got)
            for g, w in zip(got, want):
                assert C.same_bits(_np(g), w.numpy()), (W, V, slack)
    # the raw entry without the optional counters
    K, M = C.cameras(2, C.HEIGHT, 33)
    depth = _dev(C.reference_zbuffer(65, 33, 2))
    want = EO.point_masks_depth(pts, K, M, _np(depth), 0.0, backend="host")
    mask = torch.full((2, C.HEIGHT, 33), 7, dtype=torch.uint8, device=DEV)
    p, Kd, Md = _dev(pts), _dev(K), _dev(M.reshape(2, 12))
    rc = L.load().cgs_point_mask_depth(P, L.ptr(p), 2, L.ptr(Kd), L.ptr(Md), C.HEIGHT, 33, L.ptr(depth), 0.0, L.ptr(mask), None,
                                       None, L.raw_stream(DEV))
    assert rc == 0 and C.same_bits(_np(mask), want.numpy())


@pytest.mark.parametrize("shape", ["box", "l_bracket"])
def test_a_solids_ground_truth_scores_one_with_the_occluder_and_less_without(shape):
    s = check_solid_score(shape, "gpu")
    host = SS.solid_scan(shape, len(s.cameras), s.maps.shape[1], s.maps.shape[2], backend="host")
    assert C.same_bits(s.maps, host.maps) and C.same_bits(s.depth, host.depth) and C.same_bits(s.hidden, host.hidden)


def test_score_edges_does_not_depend_on_the_chunking_or_the_back_end():
    s = SS.solid_scan("l_bracket", 5, 48, 64, backend="host")
    want = R.score_edges(s.edges, s.cameras, s.maps, "PidiNet", backend="host", occluder=s.tris)
    per_view = (ES.BYTES_PER_PIXEL + ES.DEPTH_BYTES_PER_PIXEL) * 48 * 64
    for budget in (None, 2 * per_view, 1):   # one chunk, chunks of two views, one view at a time
        for gate in (dict(occluder=s.tris), dict(depth_maps=list(s.depth))):
            got = R.score_edges(s.edges, s.cameras, s.maps, "PidiNet", budget_bytes=budget, **gate)
            assert got["views"] == want["views"] and got["aggregate"] == want["aggregate"], (budget, list(gate))


def test_the_timing_shapes_equal_the_host():
    H, W, V = 1200, 1600, 3
    K, M = camera_arrays(SS.emap_cameras_of(synthetic.fibonacci_cameras(V, H, W)))
    rng = np.random.default_rng(9)
    tris = (rng.uniform(0.1, 0.9, (100, 1, 3)) + rng.uniform(-0.06, 0.06, (100, 3, 3))).astype(np.float32)
    for window in (0, 1):
        want = EO.mesh_depth(tris, K, M, H, W, window=window, backend="host").numpy()
        assert np.isfinite(want).mean() > 0.05
        assert C.same_bits(_np(EO.mesh_depth(tris, K, M, H, W, window=window)), want), window
    # two triangles covering the image of camera 0: the longest loops a wave runs
    K0 = np.array([[1.0, 1.0, 0.0, 0.0]] * V)
    M0 = np.stack([np.eye(4)[:3, :4]] * V)
    M0[1, 0, 3], M0[2, 1, 3] = 3.0, -2.0
    cover = np.array([[[-8, -8, 1], [3 * W, -8, 2], [-8, 3 * H, 3]], [[2 * W, 2 * H, 2], [-2 * W, 2 * H, 2], [2 * W, -2 * H, 4]]],
                     np.float32)
    cover[..., :2] *= cover[..., 2:]
    want = EO.mesh_depth(cover, K0, M0, H, W, window=0, backend="host").numpy()
    assert np.isfinite(want).all()
    assert C.same_bits(_np(EO.mesh_depth(cover, K0, M0, H, W, window=0)), want)
