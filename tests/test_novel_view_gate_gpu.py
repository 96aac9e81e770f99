"""GPU: the depth gate on the drawn views (cgs_project_points_depth / cgs_render_points_depth) -- the projection against the
numpy back end bit for bit, the render against the ungated render of each view's visible subset (the same compositor on the
same points in the same order: an exact oracle), the counters, the chunking, the all-+inf identity and the box scan's own
hidden counts."""
import numpy as np
import pytest
import torch

import edge_visgate_cases as C
from curve_gaussian_amd import _lib
from curve_gaussian_amd.edge_extraction import novel_view as NV
from curve_gaussian_amd.edge_extraction.abc import pred_points_and_directions
from curve_gaussian_amd.ops import edge_occlusion as EO
from curve_gaussian_amd.ops.view_chunks import camera_arrays
from curve_gaussian_amd.scene import solid_scan as SS

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
SLACK = 0.001


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("V", [1, 3])
@pytest.mark.parametrize("P", [1, 255, 257, 1000])
def test_projection_equals_the_host_bit_for_bit(P, V):
    pts, _ = C.view_points(P, seed=P)
    intr, w2c = C.view_cameras(V, seed=V)
    planes = C.view_planes(V, seed=P + V)
    want_uv, want_hid = NV.project_points_depth(pts, intr, w2c, planes, SLACK, return_hidden=True, backend="host")
    uv, hid = NV.project_points_depth(torch.from_numpy(pts).to(DEV), intr, w2c, planes, SLACK, return_hidden=True)
    assert uv.is_cuda and uv.dtype == torch.float64 and hid.dtype == torch.uint8
    assert _same_bits(uv.cpu().numpy(), want_uv.numpy())   # NaN payloads included
    assert _same_bits(hid.cpu().numpy(), want_hid.numpy())
    only = NV.project_points_depth(torch.from_numpy(pts).to(DEV), intr, w2c, planes, SLACK)   # hidden_out == NULL
    assert _same_bits(only.cpu().numpy(), want_uv.numpy())
    if P >= 255:
        assert want_hid.any() and (~torch.isnan(want_uv[..., 0])).any()
    # seen | hidden is what the ungated entry keeps, with its coordinates
    plain = NV.project_points(torch.from_numpy(pts).to(DEV), intr, w2c, C.H, C.W).cpu().numpy()
    np.testing.assert_array_equal(~np.isnan(plain[..., 0]), ~np.isnan(want_uv.numpy()[..., 0]) | want_hid.numpy().astype(bool))
    seen = ~np.isnan(want_uv.numpy()[..., 0])
    assert _same_bits(plain[seen], want_uv.numpy()[seen])


@pytest.fixture(scope="module")
def crowd():
    pts, col = C.crowded_points(1000)
    intr, w2c = C.view_cameras(3)
    planes = C.view_planes(3)
    dp, dc = torch.from_numpy(pts).to(DEV), torch.from_numpy(col).to(DEV)
    img, kept, hidden = NV.render_points_depth(dp, dc, intr, w2c, planes, SLACK, alpha=0.5, return_counts=True)
    torch.cuda.synchronize()
    return dict(pts=dp, col=dc, intr=intr, w2c=w2c, planes=planes, img=img.cpu().numpy(), kept=kept.cpu().numpy(),
                hidden=hidden.cpu().numpy())


def test_render_equals_the_ungated_render_of_the_visible_subset(crowd):
    c = crowd
    uv, hid = NV.project_points_depth(c["pts"], c["intr"], c["w2c"], c["planes"], SLACK, return_hidden=True)
    plain = NV.project_points(c["pts"], c["intr"], c["w2c"], C.H, C.W).cpu().numpy()
    uv, hid = uv.cpu().numpy(), hid.cpu().numpy().astype(bool)
    crowded = 0
    for v in range(3):
        vis = ~np.isnan(uv[v, :, 0])
        sel = torch.from_numpy(np.flatnonzero(vis)).to(DEV)   # ascending: the subset keeps the order
        want, k = NV.render_points(c["pts"][sel], c["col"][sel], c["intr"][v:v + 1], c["w2c"][v:v + 1], C.H, C.W, 0.5,
                                   return_kept=True)
        assert _same_bits(c["img"][v], want[0].cpu().numpy()), v
        assert c["kept"][v] == int(k[0]) == int(vis.sum()) and c["hidden"][v] == int(hid[v].sum())
        # a pixel with more than K = 25 visible points and a hidden one among its 25 newest
        pix = (np.floor(plain[v, :, 1]) * C.W + np.floor(plain[v, :, 0]))
        for p in np.unique(pix[vis]):
            idx_vis = np.flatnonzero(vis & (pix == p))
            if len(idx_vis) > 25 and (hid[v] & (pix == p) & (np.arange(len(vis)) > idx_vis[-25])).any():
                crowded += 1
    assert crowded > 0, "no pixel holds more than 25 visible points with hidden ones interleaved"
    assert c["hidden"].sum() > 0 and c["kept"].sum() > 0


def test_counters_chunking_and_identities(crowd):
    c = crowd
    lib = _lib.load()
    _, plain_kept = NV.render_points(c["pts"], c["col"], c["intr"], c["w2c"], C.H, C.W, 0.5, return_kept=True)
    np.testing.assert_array_equal(c["kept"] + c["hidden"], plain_kept.cpu().numpy())
    # one view per chunk and all three in one: depth and hidden are indexed by the absolute view
    one = lib.cgs_render_points_workspace_bytes(1000, 1, C.H, C.W)
    assert lib.cgs_render_points_workspace_bytes(1000, 3, C.H, C.W) > one
    img1, kept1, hid1 = NV.render_points_depth(c["pts"], c["col"], c["intr"], c["w2c"], c["planes"], SLACK, alpha=0.5,
                                               workspace_bytes=one, return_counts=True)
    assert _same_bits(img1.cpu().numpy(), c["img"])
    np.testing.assert_array_equal(kept1.cpu().numpy(), c["kept"])
    np.testing.assert_array_equal(hid1.cpu().numpy(), c["hidden"])
    assert len({int(h) for h in c["hidden"]}) > 1, "the views hide different numbers: a wrong view's plane would show"
    # an all-+inf depth is the ungated image to the bit
    inf = np.full_like(c["planes"], np.inf)
    img, kept, hid = NV.render_points_depth(c["pts"], c["col"], c["intr"], c["w2c"], inf, SLACK, alpha=0.5, return_counts=True)
    want = NV.render_points(c["pts"], c["col"], c["intr"], c["w2c"], C.H, C.W, 0.5)
    assert _same_bits(img.cpu().numpy(), want.cpu().numpy())
    assert not hid.any() and torch.equal(kept, plain_kept)
    # everything hidden: the background, nothing kept
    bg = (0.25, 0.5, 0.75)
    img, kept, hid = NV.render_points_depth(c["pts"], c["col"], c["intr"], c["w2c"], np.zeros_like(c["planes"]), SLACK,
                                            alpha=0.5, background=bg, return_counts=True)
    assert not kept.any() and torch.equal(hid, plain_kept)
    assert _same_bits(img.cpu().numpy(), np.broadcast_to(np.asarray(bg, np.float32), (3, C.H, C.W, 3)))
    # no points at all
    img, kept, hid = NV.render_points_depth(c["pts"][:0], c["col"][:0], c["intr"], c["w2c"], c["planes"], SLACK, background=bg,
                                            return_counts=True)
    assert not kept.any() and not hid.any()
    assert _same_bits(img.cpu().numpy(), np.broadcast_to(np.asarray(bg, np.float32), (3, C.H, C.W, 3)))


def test_hidden_counts_of_the_box_scan_are_the_scans_own():
    scan = SS.solid_scan("box", 6, 60, 80, backend="gpu", device=DEV)
    pts = np.ascontiguousarray(pred_points_and_directions(scan.edges, SS.SAMPLE_RESOLUTION).points, np.float32).reshape(-1, 3)
    intr, w2c = camera_arrays(scan.cameras)
    planes = EO.depth_window_max(scan.depth, EO.DEPTH_WINDOW, backend="gpu", device=DEV)
    dp = torch.from_numpy(pts).to(DEV)
    _, kept, hidden = NV.render_points_depth(dp, torch.ones_like(dp), intr, w2c, planes, EO.DEPTH_SLACK, return_counts=True)
    np.testing.assert_array_equal(hidden.cpu().numpy(), scan.hidden)
    assert scan.hidden.sum() > 0 and kept.sum() > 0
