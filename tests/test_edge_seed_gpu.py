"""GPU: cgs_pack_near_bits / cgs_voxel_votes against the host back end, bit for bit; accumulation, chunking, the drawn scan end
to end, and a Scene seeded from the edge votes."""
import numpy as np
import pytest
import torch

import edge_seed_cases as SC
from curve_gaussian_amd.ops import edge_score as ES
from curve_gaussian_amd.ops import edge_seed as SD

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
_HOST = {}


def _host_bits(V, tol_px):
    key = ("bits", V, tol_px)
    if key not in _HOST:
        _HOST[key] = SD.near_bits(ES.edt_squared(SC.vote_masks(V), "host"), tol_px, backend="host")
    return _HOST[key]


def _host_seeds():
    if "seeds" not in _HOST:
        cams, maps = SC.seed_novel_cameras()
        _HOST["seeds"] = SD.seed_points(cams, maps, "PidiNet", SC.SEED_BOUNDS, backend="host", **SC.SEED_OPTIONS)
    return _HOST["seeds"]


@pytest.mark.parametrize("width", SC.BITS_WIDTHS)
@pytest.mark.parametrize("tol_px", [0, 2])   # tol2 0 and 4
def test_bits_are_bit_identical_to_the_host(width, tol_px):
    from curve_gaussian_amd import _lib as L
    d2 = SC.bits_dist2(width)
    want = SD.near_bits(d2, tol_px, backend="host")
    d2_dev = torch.from_numpy(d2).to(DEV)
    assert torch.equal(SD.near_bits(d2_dev, tol_px, backend="gpu").cpu(), want)
    got = torch.full(want.shape, -1, dtype=torch.int32, device=DEV)   # every word is written, padding included
    L.check(L.load().cgs_pack_near_bits(3, SC.BITS_HEIGHT, width, L.ptr(d2_dev), tol_px * tol_px, L.ptr(got), L.raw_stream(DEV)),
            "cgs_pack_near_bits")
    assert torch.equal(got.cpu(), want)


@pytest.mark.parametrize("dims", SC.VOTE_GRIDS, ids=lambda d: "x".join(map(str, d)))
@pytest.mark.parametrize("V", SC.VOTE_VIEWS)
def test_votes_are_bit_identical_to_the_host(dims, V):
    K, M = SC.vote_cameras(V)
    bits = _host_bits(V, 2)
    want_seen, want_hit = SD.voxel_votes(SC.VOTE_BOUNDS, dims, K, M, bits, SC.MASK_H, SC.MASK_W, backend="host")
    seen, hit = SD.voxel_votes(SC.VOTE_BOUNDS, dims, K, M, bits.to(DEV), SC.MASK_H, SC.MASK_W, backend="gpu")
    assert seen.dtype == torch.uint16 and seen.is_cuda
    assert torch.equal(seen.cpu(), want_seen) and torch.equal(hit.cpu(), want_hit)
    if dims[0] >= 63:
        assert want_seen.numpy().max() >= 1 and want_seen.numpy().min() < V, "the case must hold kept and dropped projections"


def test_votes_on_the_image_bounds():
    K, M = SC.vote_cameras(1)
    ones = torch.ones((1, SC.MASK_H, SC.MASK_W), dtype=torch.uint8, device=DEV)
    bits = SD.near_bits(ES.edt_squared(ones, "gpu"), 0, backend="gpu")
    seen, hit = SD.voxel_votes(SC.BOUNDARY_BOUNDS, SC.BOUNDARY_DIMS, K, M, bits, SC.MASK_H, SC.MASK_W, backend="gpu")
    want = SC.boundary_expected_seen()
    assert np.array_equal(seen.cpu().numpy(), want) and np.array_equal(hit.cpu().numpy(), want)


def test_accumulation_and_repeat_runs():
    K, M = SC.vote_cameras(40)
    bits = _host_bits(40, 2).to(DEV)
    dims = (65, 3, 2)
    run = lambda: SD.voxel_votes(SC.VOTE_BOUNDS, dims, K, M, bits, SC.MASK_H, SC.MASK_W, backend="gpu")
    one, again = run(), run()
    assert torch.equal(one[0], again[0]) and torch.equal(one[1], again[1])
    part = SD.voxel_votes(SC.VOTE_BOUNDS, dims, K[:13], M[:13], bits[:13], SC.MASK_H, SC.MASK_W, backend="gpu")
    both = SD.voxel_votes(SC.VOTE_BOUNDS, dims, K[13:], M[13:], bits[13:], SC.MASK_H, SC.MASK_W, counts=part, backend="gpu")
    assert both[0] is part[0] and torch.equal(both[0], one[0]) and torch.equal(both[1], one[1])
    none = SD.voxel_votes(SC.VOTE_BOUNDS, dims, K[:0], M[:0], bits[:0], SC.MASK_H, SC.MASK_W, backend="gpu")
    assert not none[0].cpu().numpy().any() and not none[1].cpu().numpy().any(), "no view zeroes the counts"


def test_chunking_changes_nothing():
    cams, maps = SC.seed_novel_cameras()
    whole, info = SD.seed_points(cams, maps, "PidiNet", SC.SEED_BOUNDS, backend="gpu", device=DEV, **SC.SEED_OPTIONS)
    budget = 2 * SD.BYTES_PER_PIXEL * SC.SEED_H * SC.SEED_W   # two views at a time
    parts, info_p = SD.seed_points(cams, maps, "PidiNet", SC.SEED_BOUNDS, backend="gpu", device=DEV, budget_bytes=budget,
                                   **SC.SEED_OPTIONS)
    assert len(whole) > 0 and np.array_equal(whole, parts) and info == info_p


def test_one_view_per_chunk_with_claims_and_directions_equals_host():
    """budget_bytes=1: both sweeps of seed_points go one view at a time -- six uploads of one camera, six SeedViews of one
    view, the votes and the wins accumulated across them.  Seeds, directions and every integer of info equal the host's."""
    cams, maps = SC.seed_novel_cameras()
    kw = dict(exclusive=True, directions=True, **SC.SEED_OPTIONS)
    want, want_info = SD.seed_points(cams, maps, "PidiNet", SC.SEED_BOUNDS, backend="host", **kw)
    got, info = SD.seed_points(cams, maps, "PidiNet", SC.SEED_BOUNDS, backend="gpu", device=DEV, budget_bytes=1, **kw)
    assert len(got) > 0 and got.dtype == np.float64 and np.array_equal(got, want)
    assert np.array_equal(info["directions"], want_info["directions"]) and info["backend"] == "gpu"
    keys = set(want_info) - {"backend", "directions"}
    assert keys == set(info) - {"backend", "directions"} and all(info[k] == want_info[k] for k in keys)
    assert 0 < info["exclusive_voxels"] < info["kept_voxels"] and info["directed"] > 0 and info["views"] == 6


def test_seed_points_gpu_equals_host():
    cams, maps = SC.seed_novel_cameras()
    want, want_info = _host_seeds()
    got, info = SD.seed_points(cams, maps, "PidiNet", SC.SEED_BOUNDS, backend="gpu", device=DEV, **SC.SEED_OPTIONS)
    assert got.dtype == np.float64 and np.array_equal(got, want), "the float64 positions included"
    assert {**info, "backend": "host"} == want_info and len(got) > 100


@pytest.mark.parametrize("layout", ["emap", "colmap"])
def test_scene_seeded_from_the_edge_votes(layout, tmp_path):
    """One curve per seed, laid symmetrically around it (P0 + P3 = P1 + P2 = 2 p): the mean of the four float32 control
    points is the float32 seed up to the rounding of p and of the four sums, at most 2^-23 of the largest coordinate
    each -- bounded by 2^-21 of it."""
    from curve_gaussian_amd.edge_extraction.reprojection import scene_cameras
    from curve_gaussian_amd.gaussian_renderer import PipelineParams, render
    from curve_gaussian_amd.scene import GaussianCurveModel, Scene, default_seed_bounds
    scan = SC.write_seed_scan(tmp_path, layout)
    gm = GaussianCurveModel(0, 12, device=DEV)
    scene = Scene(scan, gm, device=DEV, init="edge_votes", init_options=dict(SC.SEED_OPTIONS))
    from curve_gaussian_amd.scene.colmap_io import read_colmap
    bounds = default_seed_bounds(layout, read_colmap(scan)[2].points if layout == "colmap" else None)
    cams, maps = scene_cameras(scene.getTrainCameras())
    want, info = SD.seed_points(cams, maps, "DexiNed", bounds, backend="host", **SC.SEED_OPTIONS)
    cp = gm.get_curve_points.detach().double().cpu().numpy()
    assert info["seeds"] > 100 and cp.shape == (info["seeds"], 4, 3), "one curve per seed"
    assert np.array_equal(np.asarray(scene.point_cloud.points), want)
    assert np.abs(cp.mean(1) - want).max() <= 2.0 ** -21 * np.abs(cp).max()
    gm.training_setup()
    with torch.no_grad():
        out = render(scene.getTrainCameras()[0], gm, PipelineParams(), torch.zeros(3, device=DEV))["render"]
    assert torch.isfinite(out).all() and out.abs().sum() > 0
