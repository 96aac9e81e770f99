"""CPU: the edge-vote seed (ops/edge_seed.py, host back end) against a brute-force loop, its packing, boundaries, selection,
thinning and accumulation rules, the drawn scan, the argument checks of the op and of the C ABI, and the tool."""
import ctypes
import math

import numpy as np
import pytest
import torch

import edge_score_cases as EC
import edge_seed_cases as SC
from curve_gaussian_amd.ops import edge_score as ES
from curve_gaussian_amd.ops import edge_seed as SD


# ------------------------------------------------------------------------------------------------ 1. brute force
def _brute_votes(bounds, dims, K, M, masks, tol_px):
    """A plain loop with no code of the op: float64 projection written out, edt_brute."""
    lo, hi = bounds
    nx, ny, nz = dims
    step = [(hi[a] - lo[a]) / dims[a] for a in range(3)]
    V, H, W = masks.shape
    d2 = [EC.edt_brute(masks[v]) for v in range(V)]
    tol2 = math.floor(tol_px * tol_px)
    seen, hit = np.zeros(nx * ny * nz, np.uint16), np.zeros(nx * ny * nz, np.uint16)
    for k in range(nz):
        for j in range(ny):
            for i in range(nx):
                X, Y, Z = (float(np.float32(lo[a] + (t + 0.5) * step[a])) for a, t in enumerate((i, j, k)))
                for v in range(V):
                    m = [float(x) for x in np.asarray(M[v]).reshape(12)]
                    c0 = ((m[0] * X + m[1] * Y) + m[2] * Z) + m[3]
                    c1 = ((m[4] * X + m[5] * Y) + m[6] * Z) + m[7]
                    c2 = ((m[8] * X + m[9] * Y) + m[10] * Z) + m[11]
                    if c2 <= 0.0:
                        continue
                    pu = float(K[v][0]) * (c0 / c2) + float(K[v][2])
                    pv = float(K[v][1]) * (c1 / c2) + float(K[v][3])
                    if not (0.0 <= pu < W and 0.0 <= pv < H):
                        continue
                    g = (k * ny + j) * nx + i
                    seen[g] += 1
                    hit[g] += int(d2[v][math.floor(pv), math.floor(pu)] <= tol2)
    return seen, hit


@pytest.mark.parametrize("tol_px", [0, 2])
def test_host_votes_equal_a_brute_force_loop(tol_px):
    K, M = EC.mask_cameras()
    masks = SC.vote_masks(3, density=0.1)
    bounds, dims = ((-0.4, -0.3, -0.2), (1.4, 1.3, 1.2)), (5, 4, 3)
    bits = SD.near_bits(ES.edt_squared(masks, "host"), tol_px, backend="host")
    seen, hit = SD.voxel_votes(bounds, dims, K, M, bits, SC.MASK_H, SC.MASK_W, backend="host")
    want_seen, want_hit = _brute_votes(bounds, dims, K, M, masks, tol_px)
    assert want_seen.max() >= 2 and 0 < want_hit.sum() < want_seen.sum(), "the case must exercise both counts"
    assert np.array_equal(seen.numpy(), want_seen) and np.array_equal(hit.numpy(), want_hit)


# ------------------------------------------------------------------------------------------------ 2. bit packing
@pytest.mark.parametrize("width", SC.BITS_WIDTHS)
@pytest.mark.parametrize("tol_px", [0, 2])
def test_bit_packing(width, tol_px):
    d2 = SC.bits_dist2(width)
    bits = SD.near_bits(d2, tol_px, backend="host")
    assert bits.dtype == torch.int32 and tuple(bits.shape) == (3, SC.BITS_HEIGHT, (width + 31) // 32)
    near, padding = SD.unpack_bits(bits, width)
    assert np.array_equal(near, d2 <= tol_px * tol_px)
    assert not padding.any(), "padding bits are zero"
    assert not bits[2].any(), "a view without features packs to zero"
    # the layout, spelled out: bit b of word w of row y is pixel 32 w + b
    words = bits.numpy().view(np.uint32)
    for x in range(width):
        assert np.array_equal((words[:, :, x // 32] >> np.uint32(x % 32)) & np.uint32(1), (d2[:, :, x] <= tol_px * tol_px))


# ------------------------------------------------------------------------------------------------ 3. boundaries
def test_centres_on_the_image_bounds_of_the_identity_camera():
    K, M = SC.vote_cameras(1)
    centres = SD.voxel_centres(SC.BOUNDARY_BOUNDS, SC.BOUNDARY_DIMS).astype(np.float64)
    assert set(centres[:, 0]) == {0.0, 33.5, 67.0, 100.5} and set(centres[:, 1]) == {0.0, 22.5, 45.0, 67.5}
    assert set(centres[:, 2]) == {-1.0, 0.0, 1.0}, "the centres are exact in float32"
    ones = np.full((1, SC.MASK_H, SC.MASK_W), 1, np.uint8)
    bits = SD.near_bits(ES.edt_squared(ones, "host"), 0, backend="host")
    seen, hit = SD.voxel_votes(SC.BOUNDARY_BOUNDS, SC.BOUNDARY_DIMS, K, M, bits, SC.MASK_H, SC.MASK_W, backend="host")
    want = SC.boundary_expected_seen()
    assert want.sum() == 4
    assert np.array_equal(seen.numpy(), want), "u = 0, v = 0 kept; u = W, v = H, c2 = 0 and c2 < 0 dropped"
    assert np.array_equal(hit.numpy(), want)


# ------------------------------------------------------------------------------------------------ 4. selection, thinning, accumulation
def test_selection_on_hand_written_counts():
    assert SD.need_table(0.8, 10).tolist() == [0, 1, 2, 3, 4, 4, 5, 6, 7, 8, 8]
    seen = np.array([0, 2, 3, 3, 5, 5, 10, 10, 6], np.uint16)
    hit = np.array([0, 2, 3, 2, 4, 3, 8, 7, 5], np.uint16)
    #               s<3 s<3 ok  3>2 ok  4>3 ok  8>7 ok
    assert SD.select_voxels(seen, hit, 3, 0.8).tolist() == [False, False, True, False, True, False, True, False, True]
    assert SD.select_voxels(seen, hit, 0, 0.8).tolist() == [True, True, True, False, True, False, True, False, True]
    assert SD.select_voxels(seen, hit, 6, 0.0).tolist() == [False] * 6 + [True] * 3


def test_thinning_on_a_hand_written_mask():
    dims, bounds, cell = (5, 4, 2), ((0.0, 10.0, -1.0), (5.0, 12.0, 1.0)), 2   # step (1, 0.5, 1); cells 3 x 2 x 1
    keep = np.zeros(dims[::-1], bool)   # [k][j][i]
    hit = np.zeros(dims[::-1], np.uint16)
    for (i, j, k), h in {(0, 0, 0): 3, (1, 1, 1): 4, (1, 0, 0): 1,     # cell 0: mean (2/3, 1/3, 1/3), hit sum 8
                         (4, 0, 1): 5,                                 # cell 2 (the odd last column): hit sum 5
                         (2, 3, 0): 2, (3, 2, 1): 3,                   # cell 4: mean (2.5, 2.5, 0.5), hit sum 5
                         (4, 3, 0): 9}.items():                        # cell 5: hit sum 9
        keep[k, j, i], hit[k, j, i] = True, h
    hit[1, 3, 0] = 7                                                   # not kept: counts nowhere
    seeds, info = SD.thin_to_seeds(keep.reshape(-1), hit.reshape(-1), bounds, dims, cell, 100)
    assert info["cells"] == 4 and not info["capped"] and info["cell_index"].tolist() == [0, 2, 4, 5]
    assert info["hit_sum"].tolist() == [8, 5, 5, 9]
    lo, step = np.array(bounds[0]), np.array([1.0, 0.5, 1.0])
    means = np.array([[2 / 3, 1 / 3, 1 / 3], [4, 0, 1], [2.5, 2.5, 0.5], [4, 3, 0]])
    assert seeds.dtype == np.float64 and np.array_equal(seeds, lo + (means + 0.5) * step)
    # the cap: the largest hit sums win (cells 5 and 0), the tie between cells 2 and 4 goes to the lower index
    capped, info3 = SD.thin_to_seeds(keep.reshape(-1), hit.reshape(-1), bounds, dims, cell, 3)
    assert info3["capped"] and info3["cells"] == 4 and info3["cell_index"].tolist() == [0, 2, 5]
    assert np.array_equal(capped, seeds[[0, 1, 3]])
    two, info2 = SD.thin_to_seeds(keep.reshape(-1), hit.reshape(-1), bounds, dims, cell, 2)
    assert info2["cell_index"].tolist() == [0, 5] and np.array_equal(two, seeds[[0, 3]])
    none, info0 = SD.thin_to_seeds(np.zeros(40, bool), hit.reshape(-1), bounds, dims, cell, 2)
    assert none.shape == (0, 3) and info0["cells"] == 0


def test_accumulating_over_two_chunks_equals_one_call():
    K, M = SC.vote_cameras(3)
    bits = SD.near_bits(ES.edt_squared(SC.vote_masks(3, density=0.1), "host"), 2, backend="host")
    dims = (9, 5, 4)
    one = SD.voxel_votes(SC.VOTE_BOUNDS, dims, K, M, bits, SC.MASK_H, SC.MASK_W, backend="host")
    part = SD.voxel_votes(SC.VOTE_BOUNDS, dims, K[:1], M[:1], bits[:1], SC.MASK_H, SC.MASK_W, backend="host")
    both = SD.voxel_votes(SC.VOTE_BOUNDS, dims, K[1:], M[1:], bits[1:], SC.MASK_H, SC.MASK_W, counts=part, backend="host")
    assert both[0] is part[0] and one[0].numpy().max() == 3
    assert torch.equal(both[0], one[0]) and torch.equal(both[1], one[1])


# ------------------------------------------------------------------------------------------------ 5. the drawn scan
def test_drawn_scan_recall_and_selectivity():
    """Six fibonacci_cameras views of 48x64, bounds [0,1]^3, grid 32, cell 2, tol_px 3 (the largest pixel distance between a
    point's pixel and its voxel centre's pixel is 2.0).  Measured on the host back end: no sampled point is excluded
    (0 of 701), every one has a seed within cell * |step| = 0.108, and 3177 of 32768 voxels (9.7 %) are kept."""
    worst, excluded = SC.seed_pixel_distance()
    assert SC.SEED_TOL_PX == math.ceil(worst) + 1, worst
    cams, maps = SC.seed_novel_cameras()
    seeds, info = SD.seed_points(cams, maps, "PidiNet", SC.SEED_BOUNDS, backend="host", **SC.SEED_OPTIONS)
    pts = SC.seed_points_sampled()
    share = info["kept_voxels"] / info["voxels"]
    print(f"points {len(pts)}, excluded {int(excluded.sum())}, pixel distance {worst}, kept share {share:.4f}, {info}")
    assert info["dims"] == (32, 32, 32) and info["views"] == 6 and not info["capped"] and info["seeds"] == len(seeds) > 0
    assert excluded.mean() <= 0.10
    # A point that is not excluded has, in every view, its centre's pixel inside the image and SEED_TOL_PX from the border,
    # its own pixel within SEED_TOL_PX - 1 of that -- so drawn --, hence the centre is seen and hit in all six views and
    # kept.  The seed of its cell lies in the hull of the cell's voxel centres, the point in the cell's box: they are at
    # most the box's diagonal apart.
    step = (np.array(SC.SEED_BOUNDS[1]) - np.array(SC.SEED_BOUNDS[0])) / SC.SEED_GRID
    bound = SC.SEED_CELL * float(np.linalg.norm(step))
    nearest = np.sqrt(((pts[~excluded, None, :] - seeds[None, :, :]) ** 2).sum(-1)).min(1)
    assert nearest.max() <= bound, (nearest.max(), bound)
    assert share < 0.25


# ------------------------------------------------------------------------------------------------ 6. arguments and the ABI
def test_argument_errors():
    from curve_gaussian_amd.scene import GaussianCurveModel, Scene
    K, M = SC.vote_cameras(3)
    bits = torch.zeros((3, SC.MASK_H, 3), dtype=torch.int32)
    ok = dict(bounds=SC.VOTE_BOUNDS, dims=(2, 2, 2), intrinsics=K, w2c=M, bits=bits, height=SC.MASK_H, width=SC.MASK_W)
    with pytest.raises(ValueError, match="unknown edge seed backend"):
        SD.voxel_votes(**ok, backend="cuda")
    with pytest.raises(ValueError, match="unknown edge seed backend"):
        SD.near_bits(np.zeros((1, 2, 2), np.int32), 1, backend="numpy")
    with pytest.raises(ValueError, match="hi > lo"):
        SD.voxel_votes(**{**ok, "bounds": ((0, 0, 0), (1, 0, 1))}, backend="host")
    with pytest.raises(ValueError, match="positive integers"):
        SD.voxel_votes(**{**ok, "dims": (2, 0, 2)}, backend="host")
    with pytest.raises(ValueError, match="bits must be int32"):
        SD.voxel_votes(**{**ok, "bits": bits[:, :-1]}, backend="host")
    with pytest.raises(ValueError, match="bits must be int32"):
        SD.voxel_votes(**{**ok, "bits": bits.to(torch.int64)}, backend="host")
    with pytest.raises(ValueError, match="at most 65535 views"):
        SD.voxel_votes(**{**ok, "intrinsics": np.ones((65536, 4)), "w2c": np.ones((65536, 3, 4))}, backend="host")
    cams, maps = SC.seed_novel_cameras()
    with pytest.raises(ValueError, match="must be uint8"):
        SD.seed_points(cams, [m[:-1] for m in maps], "PidiNet", SC.SEED_BOUNDS, backend="host")
    with pytest.raises(ValueError, match="must be uint8"):
        SD.seed_points(cams, [m.astype(np.float32) for m in maps], "PidiNet", SC.SEED_BOUNDS, backend="host")
    with pytest.raises(ValueError, match="at most 65535 views"):
        SD.seed_points(cams[:1] * 65536, maps[:1] * 65536, "PidiNet", SC.SEED_BOUNDS, backend="host")
    with pytest.raises(ValueError, match="hi > lo"):
        SD.seed_points(cams, maps, "PidiNet", ((0, 0, 0), (1, 1, 0)), backend="host")
    with pytest.raises(ValueError, match="unknown edge seed backend"):
        SD.seed_points(cams, maps, "PidiNet", SC.SEED_BOUNDS, backend="tpu")
    with pytest.raises(ValueError, match="unknown init"):
        Scene("/nonexistent", GaussianCurveModel(0, 12, device="cpu"), init="sfm")


def test_scene_without_a_seed_raises(tmp_path):
    """No silent fallback: a box that no view looks into names the bounds and the counts."""
    from curve_gaussian_amd.scene import dataset_io as IO
    scan = SC.write_seed_scan(tmp_path, "emap")
    cams = IO.read_emap(scan)
    with pytest.raises(ValueError, match=r"no seed in the box lo=\[50.0, 50.0, 50.0\].*6 views.*0 passed"):
        IO.edge_vote_point_cloud(cams, "DexiNed", ((50, 50, 50), (51, 51, 51)), backend="host", grid=8)


def test_abi_rejections_without_a_gpu():
    from curve_gaussian_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(64)   # never dereferenced: every call below is rejected before anything is launched
    lo, step = (ctypes.c_double * 3)(0, 0, 0), (ctypes.c_double * 3)(1, 1, 1)
    lo_p, step_p = ctypes.cast(lo, ctypes.c_void_p), ctypes.cast(step, ctypes.c_void_p)

    def votes(nx=2, ny=2, nz=2, lo=lo_p, step=step_p, V=1, intr=p, w2c=p, height=4, width=4, bits=p, acc=0, seen=p, hit=p):
        return lib.cgs_voxel_votes(nx, ny, nz, lo, step, V, intr, w2c, height, width, bits, acc, seen, hit, None)

    bad = [dict(V=-1), dict(V=65536), dict(nx=0), dict(ny=-1), dict(nz=0), dict(height=0), dict(width=0), dict(width=16385),
           dict(nx=2048, ny=2048, nz=512), dict(nx=65536, ny=65536, nz=1), dict(lo=None), dict(step=None), dict(intr=None),
           dict(w2c=None), dict(bits=None), dict(seen=None), dict(hit=None)]
    for kw in bad:
        assert votes(**kw) == -1 and b"cgs_voxel_votes: invalid argument" in lib.cgs_last_error(), kw
    for k, value in ((0, 0.0), (1, -1.0), (2, float("nan")), (0, float("inf"))):
        s = (ctypes.c_double * 3)(1, 1, 1)
        s[k] = value
        assert votes(step=ctypes.cast(s, ctypes.c_void_p)) == -1, (k, value)
    nan_lo = (ctypes.c_double * 3)(0, float("nan"), 0)
    assert votes(lo=ctypes.cast(nan_lo, ctypes.c_void_p)) == -1
    assert votes(V=0, acc=1, intr=None, w2c=None, bits=None) == 0, "nothing to add is a no-op"

    def pack(V=1, height=4, width=4, dist2=p, tol2=0, bits=p):
        return lib.cgs_pack_near_bits(V, height, width, dist2, tol2, bits, None)

    for kw in [dict(V=-1), dict(height=0), dict(width=0), dict(height=16385), dict(tol2=-1), dict(dist2=None), dict(bits=None)]:
        assert pack(**kw) == -1 and b"cgs_pack_near_bits: invalid argument" in lib.cgs_last_error(), kw
    assert pack(V=0, dist2=None, bits=None) == 0


def test_default_seed_bounds():
    from curve_gaussian_amd.scene import default_seed_bounds
    lo, hi = default_seed_bounds("emap")
    assert lo.tolist() == [-0.05] * 3 and hi.tolist() == [1.05] * 3 and lo.dtype == np.float64
    pts = np.stack([np.linspace(0.0, 100.0, 101), np.linspace(-50.0, 0.0, 101), np.linspace(2.0, 4.0, 101)], 1)
    pts[0] = [-1e6, 1e6, 1e6]   # an outlier the percentiles trim
    lo, hi = default_seed_bounds("colmap", pts)
    p2, p98 = np.percentile(pts, 2, axis=0), np.percentile(pts, 98, axis=0)
    assert np.allclose(lo, p2 - 0.1 * (p98 - p2), rtol=0, atol=1e-12) and np.allclose(hi, p98 + 0.1 * (p98 - p2), rtol=0, atol=1e-12)
    assert hi[0] < 120 and lo[1] > -60 and hi[2] < 5
    with pytest.raises(ValueError, match="SfM points"):
        default_seed_bounds("colmap")
    with pytest.raises(ValueError, match="unknown layout"):
        default_seed_bounds("replica")


def test_train_options_default_to_the_reference():
    from curve_gaussian_amd import train
    dataset, _, _ = train.parse_args(["-s", "scan", "-m", "out"])
    assert dataset.init == "reference" and dataset.init_options == {} and train.ModelParams().init == "reference"
    dataset, _, _ = train.parse_args(["-s", "scan", "-m", "out", "--init", "edge_votes", "--init_grid", "64", "--init_tol_px", "1.5",
                                      "--init_min_views", "4", "--init_min_ratio", "0.9", "--init_cell", "3", "--init_bounds",
                                      "0", "0", "0", "1", "2", "3"])
    assert dataset.init == "edge_votes"
    assert dataset.init_options == {"grid": 64, "tol_px": 1.5, "min_views": 4, "min_ratio": 0.9, "cell": 3,
                                    "bounds": ([0.0, 0.0, 0.0], [1.0, 2.0, 3.0])}


# ------------------------------------------------------------------------------------------------ 7. the tool
@pytest.mark.parametrize("layout", ["emap", "colmap"])
def test_tool_on_a_tiny_scan(layout, tmp_path, capsys):
    from curve_gaussian_amd import edge_seed_cli as CLI
    from curve_gaussian_amd.scene.dataset_io import read_ply_table
    scan = SC.write_seed_scan(tmp_path, layout)
    out = str(tmp_path / "seeds.ply")
    assert CLI.main(["--scan", scan, "--layout", layout, "--backend", "host", "--out", out, "--grid", "16", "--tol_px", "3",
                     "--cell", "2"]) == 0
    printed = capsys.readouterr().out
    seeds, info = CLI.seed_scan(scan, layout, backend="host", grid=16, tol_px=3, cell=2)
    assert f"views 6, grid 16x16x16, kept voxels {info['kept_voxels']}, cells {info['cells']}, seeds {len(seeds)}" in printed
    table = read_ply_table(out)
    assert len(seeds) > 0 and np.allclose(np.stack([table["x"], table["y"], table["z"]], 1), seeds, rtol=1e-9, atol=0)
    lo, hi = info["bounds"]
    assert (seeds >= np.array(lo)).all() and (seeds <= np.array(hi)).all()
    if layout == "emap":
        assert lo == [-0.05] * 3 and hi == [1.05] * 3
