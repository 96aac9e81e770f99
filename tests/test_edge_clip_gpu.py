"""GPU: cgs_mesh_depth_clipped (csrc/edge_occlusion.hip, k_mesh_depth<true>) and cgs_mesh_contours_clipped
(csrc/mesh_contours.hip) against the host back end and the brute force of edge_clip_cases.py, bit for bit -- 0, 1, 2 and 3
vertices IN in images of 1 x 1, 5 x 33 and 5 x 67, a vertex at and one ulp below the plane, NaN, the floor that covers every pixel, the shared straddling edge,
triangle and row counts around a wave and a workgroup with the camera inside the cloud --, under a permutation of the
triangles, against the unclipped entries where every vertex is IN, against the ray cast, and on the indoor fixture."""
import itertools

import numpy as np
import pytest
import torch

import edge_clip_cases as C
import mesh_contours_cases as MCC
from curve_gaussian_amd import _lib as L
from curve_gaussian_amd.ops import edge_occlusion as EO
from curve_gaussian_amd.ops import mesh_contours as MC
from curve_gaussian_amd.ops.view_chunks import camera_arrays
from curve_gaussian_amd.scene import solid_scan as SS
from test_edge_clip_cpu import ROOM, check_ray_cast, check_room

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)   # a copy: the shared cases are read-only


def _np(t):
    return t.cpu().numpy()


def _gpu(tris, K, M, W, near=C.NEAR):
    out = EO.mesh_depth(tris, K, M, C.height(W), W, window=0, near_clip=near)
    assert out.is_cuda
    return _np(out)


def _host(tris, K, M, W, near=C.NEAR):
    return EO.mesh_depth(tris, K, M, C.height(W), W, window=0, backend="host", near_clip=near).numpy()


def test_single_triangles_and_pairs_equal_the_brute_force_and_the_host():
    for W, V in itertools.product(C.WIDTHS, C.VIEWS):
        K, M = C.cameras(V, C.height(W), W)
        for name in list(C.SINGLES) + list(C.PAIRS):
            tris = C.single(name) if name in C.SINGLES else C.pair(name)
            got = _gpu(tris, K, M, W)
            assert C.same_bits(got, C.zbuffer_clipped_brute(tris, K, M, C.height(W), W)), (name, W, V)
            assert C.same_bits(got, _host(tris, K, M, W)), (name, W, V)
            if name in C.PAIRS or name == "floor":
                assert np.isfinite(got[0]).all(), (name, W, "no pixel of camera 0 is +inf: no crack, the whole image")
            if name in C.EXPECT_EMPTY:
                assert np.isinf(got[0]).all(), name


@pytest.mark.parametrize("F", C.FACES)
def test_a_cloud_around_the_camera_equals_the_brute_force_in_any_order(F):
    rng = np.random.default_rng(F)
    for W, V in ((33, 2), (1, 1), (67, 5)):
        K, M = C.cameras(V, C.height(W), W)
        tris = C.cloud(F)
        got = _gpu(_dev(tris), K, M, W)
        if (W, V) == (33, 2) or F == 65:   # (the brute force is Python: every F at one size, one F at every size)
            assert C.same_bits(got, C.reference_cloud(F, W, V)), (F, W, V)
        assert C.same_bits(got, _host(tris, K, M, W)), (F, W, V)
        assert C.same_bits(got, _gpu(tris[rng.permutation(F)], K, M, W)), (F, W, V, "a permutation of the triangles")
        for r in (1, EO.MAX_WINDOW):   # through the window maximum, as the operators use it
            a = EO.mesh_depth(tris, K, M, C.height(W), W, window=r, near_clip=C.NEAR)
            b = EO.mesh_depth(tris, K, M, C.height(W), W, window=r, backend="host", near_clip=C.NEAR)
            assert C.same_bits(_np(a), b.numpy()), (F, W, V, r)


def test_with_every_vertex_in_front_the_entries_give_their_siblings_bits():
    for shape in SS.SHAPES:
        tris, _ = SS.solid_geometry(shape)
        K, M = MCC.cube_cameras(5, 37, 70)
        a = EO.mesh_depth(tris, K, M, 37, 70, window=0)
        b = EO.mesh_depth(tris, K, M, 37, 70, window=0, near_clip=EO.NEAR_CLIP)
        assert C.same_bits(_np(a), _np(b)) and np.isfinite(_np(a)).any(), shape
        planes = EO.depth_window_max(a, 1)
        for kind in MC.KINDS:
            rows = MC.edge_rows(tris, kind)
            for d in (None, planes):
                m0 = MC.row_masks(rows, K, M, 37, 70, d)
                m1 = MC.row_masks(rows, K, M, 37, 70, d, near_clip=EO.NEAR_CLIP)
                assert C.same_bits(_np(m0), _np(m1)), (shape, kind, d is None)
                assert _np(m0).any() or (kind == "smooth" and shape != "cylinder"), (shape, kind, "only the cylinder is curved")


def test_contours_equal_the_brute_force_and_the_host():
    K, M = MCC.camera(MCC.EYE_SIDE)
    for name, (row, _) in C.TENT_ROWS.items():
        got = _np(MC.row_masks(row, K, M, MCC.H, MCC.W, near_clip=C.NEAR))
        assert C.same_bits(got, C.contours_clipped_brute(row, K, M, MCC.H, MCC.W)), name
        assert C.same_bits(got, MC.row_masks(row, K, M, MCC.H, MCC.W, backend="host", near_clip=C.NEAR).numpy()), name
    for E, (W, V) in zip(C.ROWS, itertools.cycle([(33, 2), (67, 5), (1, 1)])):
        K, M = C.cameras(V, C.height(W), W)
        rows = C.cloud_rows(E)
        depth = EO.depth_window_max(C.reference_cloud(65, W, V), 1, backend="host").numpy()
        for d, slack in ((None, 0.0), (depth, 0.01)):
            got = MC.row_masks(_dev(rows), K, M, C.height(W), W, None if d is None else _dev(d), slack, near_clip=C.NEAR)
            assert got.is_cuda
            want = MC.row_masks(rows, K, M, C.height(W), W, d, slack, backend="host", near_clip=C.NEAR).numpy()
            assert C.same_bits(_np(got), want), (E, W, V, d is None)
            if E <= 65:
                assert C.same_bits(want, C.contours_clipped_brute(rows, K, M, C.height(W), W, d, slack)), (E, W, V)


def test_planes_agree_with_a_ray_cast_of_the_unclipped_triangles():
    worst = check_ray_cast(_gpu)
    print(f"ray cast: small cases, largest relative error {worst:.3g}")


def test_the_room_on_the_gpu_is_the_hosts_and_agrees_with_the_ray_cast():
    room = check_room("gpu")
    V, H, W = ROOM
    host = SS.solid_scan("room", V, H, W, backend="host")
    assert C.same_bits(room.depth, host.depth) and C.same_bits(room.maps, host.maps) and C.same_bits(room.hidden, host.hidden)
    K, M = camera_arrays(room.cameras)
    border, rel = C.against_ray_cast(room.depth, C.ray_cast(room.tris, K, M.reshape(V, 3, 4), H, W, EO.NEAR_CLIP))
    print(f"ray cast: room border pixels {border} of {V * H * W}, largest relative error {rel:.3g}")
    assert border == 0 and rel <= C.ULP2, (border, rel)   # (the host's bytes, so the host's count: none left out)
    # the contours of the room's and the pillar's edges ("all": the outline with the hidden lines removed), clipped
    planes = EO.mesh_depth(room.tris, K, M, H, W, near_clip=EO.NEAR_CLIP)
    got = MC.contour_masks(room.tris, K, M, H, W, planes, kind="all", near_clip=EO.NEAR_CLIP)
    want = MC.contour_masks(room.tris, K, M, H, W, _np(planes), kind="all", backend="host", near_clip=EO.NEAR_CLIP)
    assert C.same_bits(_np(got), want.numpy()) and _np(got).any()


def test_the_raw_entries_reject_a_bad_plane_before_any_launch():
    K, M = C.cameras(2, C.height(33), 33)
    Kd, Md, t = _dev(K), _dev(M.reshape(2, 12)), _dev(C.cloud(65))
    depth = torch.full((2, C.height(33), 33), 7.0, dtype=torch.float32, device=DEV)
    mask = torch.full((2, C.height(33), 33), 7, dtype=torch.uint8, device=DEV)
    rows = _dev(C.cloud_rows(65))
    lib = L.load()
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert lib.cgs_mesh_depth_clipped(65, L.ptr(t), 2, L.ptr(Kd), L.ptr(Md), C.height(33), 33, bad, L.ptr(depth),
                                          L.raw_stream(DEV)) == -1
        assert lib.cgs_mesh_contours_clipped(65, L.ptr(rows), 2, L.ptr(Kd), L.ptr(Md), C.height(33), 33, None, 0.0, bad,
                                             L.ptr(mask), L.raw_stream(DEV)) == -1
    torch.cuda.synchronize()
    assert (_np(depth) == 7.0).all() and (_np(mask) == 7).all(), "rejected before anything is written"
    assert lib.cgs_mesh_depth_clipped(65, L.ptr(t), 0, L.ptr(Kd), L.ptr(Md), C.height(33), 33, 0.25, L.ptr(depth),
                                      L.raw_stream(DEV)) == 0
    torch.cuda.synchronize()
    assert (_np(depth) == 7.0).all(), "V = 0 is a no-op"
    assert lib.cgs_mesh_depth_clipped(65, L.ptr(t), 2, L.ptr(Kd), L.ptr(Md), C.height(33), 33, C.NEAR, L.ptr(depth),
                                      L.raw_stream(DEV)) == 0
    assert C.same_bits(_np(depth), C.reference_cloud(65, 33, 2))
