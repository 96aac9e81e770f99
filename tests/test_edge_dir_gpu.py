"""GPU: cgs_voxel_moments against the host back end, bit for bit; the launch geometry, seed_points with directions on the
drawn scan, a Scene whose curves lie along the seeded directions, and the raw call's argument errors."""
import numpy as np
import pytest
import torch

import edge_dir_cases as DC
import edge_seed_cases as SC
from curve_gaussian_amd.ops import edge_seed as SD

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
_HOST = {}


def _raw(dims, bits, centres, radius):
    """The raw call into an output prefilled with -1: every word is written."""
    from curve_gaussian_amd import _lib as L
    cen = torch.from_numpy(np.ascontiguousarray(centres, np.int32)).to(DEV)
    out = torch.full((len(centres), SD.MOMENT_VALUES), -1, dtype=torch.int32, device=DEV)
    rc = L.load().cgs_voxel_moments(dims[0], dims[1], dims[2], L.ptr(bits), len(centres), L.ptr(cen), radius, L.ptr(out),
                                    L.raw_stream(DEV))
    L.check(rc, "cgs_voxel_moments")
    return out.cpu()


@pytest.mark.parametrize("dims", DC.MOMENT_GRIDS, ids=lambda d: "x".join(map(str, d)))
@pytest.mark.parametrize("radius", DC.MOMENT_RADII)
def test_moments_are_bit_identical_to_the_host(dims, radius):
    """Centres: every corner, the x around the word boundaries, random ones; (5, 4, 3) is narrower than the window."""
    centres = DC.moment_centres(dims)
    for kind in DC.MOMENT_MASKS:
        bits = SD.keep_bits(DC.moment_mask(dims, kind), dims)
        want = SD.voxel_moments(bits, dims, centres, radius, backend="host")
        bits_dev = bits.to(DEV)
        got = SD.voxel_moments(bits_dev, dims, centres, radius, backend="gpu")
        assert got.is_cuda and got.dtype == torch.int32 and torch.equal(got.cpu(), want), kind
        assert torch.equal(_raw(dims, bits_dev, centres, radius), want), kind
        if kind == "zeros":
            assert not want.numpy().any()
        if kind == "ones" and dims == (70, 9, 7) and radius == 1:
            assert want.numpy()[:, 0].max() == 7 and want.numpy()[:, 0].min() == 4


@pytest.mark.parametrize("count", DC.MOMENT_COUNTS)
def test_seed_counts_and_partial_blocks(count):
    dims = (70, 9, 7)
    bits = SD.keep_bits(DC.moment_mask(dims, "d0.5"), dims)
    centres = DC.moment_centres(dims, count)
    assert centres.shape == (count, 3)
    want = SD.voxel_moments(bits, dims, centres, 6, backend="host")
    assert torch.equal(SD.voxel_moments(bits.to(DEV), dims, centres, 6, backend="gpu").cpu(), want)
    if count:
        assert torch.equal(_raw(dims, bits.to(DEV), centres, 6), want)


def test_the_largest_sums():
    """All-one, r = 15 in a 33^3 grid: the centre's window is the whole ball, 14147 voxels."""
    dims = DC.BIG_DIMS
    bits = SD.keep_bits(DC.moment_mask(dims, "ones"), dims)
    centres = np.array([[16, 16, 16], [0, 0, 0], [32, 32, 32], [16, 0, 32], [31, 16, 16]], np.int64)
    want = SD.voxel_moments(bits, dims, centres, 15, backend="host")
    assert want[0].tolist()[:4] == [14147, 0, 0, 0] and want[0, 4] == want[0, 5] == want[0, 6] and want[0, 4] > 6 * 10 ** 5
    assert torch.equal(_raw(dims, bits.to(DEV), centres, 15), want)


def test_launch_geometry_does_not_matter():
    dims = (70, 9, 7)
    bits = SD.keep_bits(DC.moment_mask(dims, "d0.5"), dims).to(DEV)
    centres = DC.moment_centres(dims, 257)
    one = SD.voxel_moments(bits, dims, centres, 6, backend="gpu")
    again = SD.voxel_moments(bits, dims, centres, 6, backend="gpu")
    assert torch.equal(one, again)
    back = SD.voxel_moments(bits, dims, centres[::-1].copy(), 6, backend="gpu")
    assert torch.equal(back.flip(0), one), "a seed's row does not depend on its wave or block"


def _host_directed():
    if "seeds" not in _HOST:
        cams, maps = DC.dir_novel_cameras()
        _HOST["seeds"] = SD.seed_points(cams, maps, "PidiNet", DC.DIR_BOUNDS, backend="host", directions=True, **DC.DIR_OPTIONS)
    return _HOST["seeds"]


def test_seed_points_with_directions_gpu_equals_host():
    cams, maps = DC.dir_novel_cameras()
    want, want_info = _host_directed()
    got, info = SD.seed_points(cams, maps, "PidiNet", DC.DIR_BOUNDS, backend="gpu", device=DEV, directions=True, **DC.DIR_OPTIONS)
    assert len(got) > 100 and np.array_equal(got, want)
    assert info["directions"].dtype == np.float64 and np.array_equal(info["directions"], want_info["directions"])
    assert info["directed"] == want_info["directed"] > 0
    budget = 2 * SD.BYTES_PER_PIXEL * DC.DIR_H * DC.DIR_W   # two views at a time
    parts, info_p = SD.seed_points(cams, maps, "PidiNet", DC.DIR_BOUNDS, backend="gpu", device=DEV, directions=True,
                                   budget_bytes=budget, **DC.DIR_OPTIONS)
    assert np.array_equal(parts, got) and np.array_equal(info_p["directions"], info["directions"])
    assert {k: v for k, v in info_p.items() if k != "directions"} == {k: v for k, v in info.items() if k != "directions"}
    # the drawn scan of edge_seed_cases, whose fat tubes leave junction-like seeds undirected
    cams, maps = SC.seed_novel_cameras()
    want, want_info = SD.seed_points(cams, maps, "PidiNet", SC.SEED_BOUNDS, backend="host", directions=True, **SC.SEED_OPTIONS)
    got, info = SD.seed_points(cams, maps, "PidiNet", SC.SEED_BOUNDS, backend="gpu", device=DEV, directions=True, **SC.SEED_OPTIONS)
    assert np.array_equal(got, want) and np.array_equal(info["directions"], want_info["directions"])
    assert 0 < info["directed"] == want_info["directed"] < len(got)


@pytest.mark.parametrize("layout", ["emap", "colmap"])
def test_scene_seeded_with_directions(layout, tmp_path):
    """One curve per seed, laid symmetrically around it along the seeded direction.  The mean of the control points is the
    seed within 2^-21 of the largest coordinate (the bound of test_scene_seeded_from_the_edge_votes); the normalised chord
    P3 - P0 of float32 control points is within 1e-5 of the direction."""
    from curve_gaussian_amd.edge_extraction.reprojection import scene_cameras
    from curve_gaussian_amd.gaussian_renderer import PipelineParams, render
    from curve_gaussian_amd.scene import GaussianCurveModel, Scene, default_seed_bounds
    from curve_gaussian_amd.scene.colmap_io import read_colmap
    scan = SC.write_seed_scan(tmp_path, layout)
    gm = GaussianCurveModel(0, 12, device=DEV)
    scene = Scene(scan, gm, device=DEV, init="edge_votes", init_options=dict(SC.SEED_OPTIONS, directions=True))
    bounds = default_seed_bounds(layout, read_colmap(scan)[2].points if layout == "colmap" else None)
    cams, maps = scene_cameras(scene.getTrainCameras())
    want, info = SD.seed_points(cams, maps, "DexiNed", bounds, backend="host", directions=True, **SC.SEED_OPTIONS)
    cp = gm.get_curve_points.detach().double().cpu().numpy()
    assert info["seeds"] > 100 and cp.shape == (info["seeds"], 4, 3), "one curve per seed"
    assert np.array_equal(np.asarray(scene.point_cloud.points), want)
    assert np.array_equal(np.asarray(scene.point_cloud.normals), info["directions"])
    assert np.abs(cp.mean(1) - want).max() <= 2.0 ** -21 * np.abs(cp).max()
    chord = cp[:, 3] - cp[:, 0]
    chord /= np.linalg.norm(chord, axis=1, keepdims=True)
    directed = np.linalg.norm(info["directions"], axis=1) > 0
    assert 0 < directed.sum() == info["directed"] < len(want), "the scan holds directed and undirected seeds"
    assert np.abs(chord[directed] - info["directions"][directed]).max() <= 1e-5
    assert np.abs(chord[~directed] - np.array([0.0, 1.0, 0.0])).max() <= 1e-5, "undirected seeds lie along Y"
    gm.training_setup()
    with torch.no_grad():
        out = render(scene.getTrainCameras()[0], gm, PipelineParams(), torch.zeros(3, device=DEV))["render"]
    assert torch.isfinite(out).all() and out.abs().sum() > 0


def test_raw_argument_errors():
    from curve_gaussian_amd import _lib as L
    lib = L.load()
    dims = (5, 4, 3)
    bits = SD.keep_bits(np.ones(60, bool), dims).to(DEV)
    cen = torch.zeros((1, 3), dtype=torch.int32, device=DEV)
    out = torch.full((1, SD.MOMENT_VALUES), -1, dtype=torch.int32, device=DEV)

    def call(nx=5, N=1, radius=1, keep=L.ptr(bits), centres=L.ptr(cen), moments=L.ptr(out)):
        return lib.cgs_voxel_moments(nx, 4, 3, keep, N, centres, radius, moments, L.raw_stream(DEV))

    for kw in [dict(radius=0), dict(radius=16), dict(keep=None), dict(centres=None), dict(moments=None), dict(N=-1), dict(nx=0)]:
        assert call(**kw) == -1 and b"cgs_voxel_moments: invalid argument" in lib.cgs_last_error(), kw
    torch.cuda.synchronize(DEV)
    assert (out.cpu() == -1).all(), "nothing was launched"
    assert call(N=0) == 0 and (out.cpu() == -1).all(), "no seed is a no-op"
    assert call() == 0 and out.cpu().tolist() == [[4, 1, 1, 1, 1, 1, 1, 0, 0, 0]]
