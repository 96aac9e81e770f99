"""CPU: the direction of a seed from the kept voxels around it (ops/edge_seed.py) on the host back end -- keep
bits, centre voxels, moments, the eigen-direction on tubes whose axis is known, the model layer and the drawn scan."""
import ctypes
import fractions

import numpy as np
import pytest
import torch

import edge_dir_cases as DC
import edge_seed_cases as SC
from curve_gaussian_amd.ops import edge_seed as SD

CENTRE = np.array([DC.TUBE_CENTRE], np.int64)


def _direction(keep, radius=DC.BALL_RADIUS, min_support=SD.DIR_MIN_SUPPORT, min_linearity=SD.DIR_MIN_LINEARITY):
    mom = SD.voxel_moments(SD.keep_bits(keep, DC.TUBE_DIMS), DC.TUBE_DIMS, CENTRE, radius, backend="host")
    vec, directed, lin = SD.seed_directions(mom, min_support, min_linearity)
    return vec[0], bool(directed[0]), float(lin[0]), mom[0].numpy()


# ------------------------------------------------------------------------------------------------ keep bits and centres
@pytest.mark.parametrize("nx", SC.BITS_WIDTHS)
def test_keep_bits_round_trip(nx):
    dims = (nx, 3, 2)
    keep = np.random.default_rng(nx).random(nx * 6) < 0.5
    bits = SD.keep_bits(keep, dims)
    assert bits.dtype == torch.int32 and tuple(bits.shape) == (2, 3, SD.bits_stride(nx))
    got, padding = SD.unpack_bits(bits, nx)
    assert np.array_equal(got.reshape(-1), keep) and not padding.any()
    ones = SD.keep_bits(np.ones(nx * 6, bool), dims)
    got, padding = SD.unpack_bits(ones, nx)
    assert got.all() and not padding.any(), "padding bits are 0"
    with pytest.raises(ValueError):
        SD.keep_bits(keep[:-1], dims)


def test_centre_voxel_is_the_rounded_mean():
    dims, cell = (13, 9, 7), 4
    rng = np.random.default_rng(4)
    keep = rng.random(13 * 9 * 7) < 0.3
    hit = rng.integers(0, 9, keep.size).astype(np.uint16)
    bounds = ((0.0, 0.0, 0.0), (1.3, 0.9, 0.7))
    plain_seeds, plain = SD.thin_to_seeds(keep, hit, bounds, dims, cell, 1000)
    assert sorted(plain) == ["capped", "cell_index", "cells", "hit_sum"], "without the keyword: today's keys"
    seeds, info = SD.thin_to_seeds(keep, hit, bounds, dims, cell, 1000, return_centres=True)
    assert np.array_equal(seeds, plain_seeds) and sorted(info) == sorted(list(plain) + ["centre_voxel"])
    centres = info["centre_voxel"]
    assert centres.dtype == np.int64 and centres.shape == (len(seeds), 3) and len(seeds) > 10
    g = np.nonzero(keep)[0]
    ijk = np.stack([g % 13, (g // 13) % 9, g // (13 * 9)], 1)
    cidx = ((ijk[:, 2] // cell) * 3 + ijk[:, 1] // cell) * 4 + ijk[:, 0] // cell
    half = fractions.Fraction(1, 2)
    for row, c in enumerate(info["cell_index"]):
        members = ijk[cidx == c]
        for a in range(3):
            mean = fractions.Fraction(int(members[:, a].sum()), len(members))
            assert int(centres[row, a]) == (mean + half).numerator // (mean + half).denominator
    # max_seeds cuts the centres along with the rest
    cut_seeds, cut = SD.thin_to_seeds(keep, hit, bounds, dims, cell, 5, return_centres=True)
    keep_rows = np.isin(info["cell_index"], cut["cell_index"])
    assert cut["capped"] and np.array_equal(cut["centre_voxel"], centres[keep_rows]) and len(cut_seeds) == 5
    empty_seeds, empty = SD.thin_to_seeds(np.zeros_like(keep), hit, bounds, dims, cell, 5, return_centres=True)
    assert empty["centre_voxel"].shape == (0, 3) and len(empty_seeds) == 0


# ------------------------------------------------------------------------------------------------ moments and directions
def test_moments_of_a_hand_made_window():
    """A 5 x 4 x 3 grid, r = 1, centre (2, 1, 1): the window is the centre and its six neighbours."""
    dims = (5, 4, 3)
    keep = np.zeros((3, 4, 5), bool)   # [z][y][x]
    keep[1, 1, 2] = keep[1, 1, 3] = keep[1, 2, 2] = keep[0, 1, 2] = True   # the centre, +x, +y, -z
    keep[1, 2, 3] = keep[2, 2, 2] = True                                  # at distance sqrt(2): outside the ball
    mom = SD.voxel_moments(SD.keep_bits(keep.reshape(-1), dims), dims, np.array([[2, 1, 1]]), 1, backend="host")
    assert mom.dtype == torch.int32 and mom.tolist() == [[4, 1, 1, -1, 1, 1, 1, 0, 0, 0]]
    corner = SD.voxel_moments(SD.keep_bits(np.ones(60, bool), dims), dims, np.array([[0, 0, 0], [4, 3, 2]]), 1, backend="host")
    assert corner.tolist() == [[4, 1, 1, 1, 1, 1, 1, 0, 0, 0], [4, -1, -1, -1, 1, 1, 1, 0, 0, 0]], "clipped to the grid"


def test_moments_argument_errors():
    dims = (5, 4, 3)
    bits = SD.keep_bits(np.ones(60, bool), dims)
    ok = np.array([[0, 0, 0]])
    for bad in ([[5, 0, 0]], [[0, -1, 0]], [[0, 0, 3]]):
        with pytest.raises(ValueError, match="outside"):
            SD.voxel_moments(bits, dims, np.array(bad), 1, backend="host")
    for radius in (0, 16, 2.5):
        with pytest.raises(ValueError, match="radius"):
            SD.voxel_moments(bits, dims, ok, radius, backend="host")
    with pytest.raises(ValueError, match="bits"):
        SD.voxel_moments(bits.to(torch.int64), dims, ok, 1, backend="host")
    with pytest.raises(ValueError, match="bits"):
        SD.voxel_moments(bits[:, :3], dims, ok, 1, backend="host")
    with pytest.raises(ValueError, match="backend"):
        SD.voxel_moments(bits, dims, ok, 1, backend="cuda")
    with pytest.raises(ValueError, match="centres"):
        SD.voxel_moments(bits, dims, np.array([[0.0, 0.0, 0.0]]), 1, backend="host")
    assert tuple(SD.voxel_moments(bits, dims, np.zeros((0, 3), np.int64), 1, backend="host").shape) == (0, 10)


def test_abi_rejections_without_a_gpu():
    from curve_gaussian_amd import _lib
    lib = _lib.load()
    p = ctypes.c_void_p(64)   # never dereferenced: every call below is rejected before anything is launched

    def moments(nx=2, ny=2, nz=2, keep=p, N=1, centres=p, radius=1, out=p):
        return lib.cgs_voxel_moments(nx, ny, nz, keep, N, centres, radius, out, None)

    bad = [dict(radius=0), dict(radius=16), dict(radius=-3), dict(N=-1), dict(nx=0), dict(ny=-1), dict(nz=0), dict(keep=None),
           dict(centres=None), dict(out=None), dict(nx=2048, ny=2048, nz=512), dict(nx=65536, ny=65536, nz=1)]
    for kw in bad:
        assert moments(**kw) == -1 and b"cgs_voxel_moments: invalid argument" in lib.cgs_last_error(), kw
    assert moments(N=0) == 0, "no seed is a no-op"


@pytest.mark.parametrize("lattice", DC.lattice_directions(), ids=lambda v: "".join("-0+"[c + 1] for c in v))
def test_lattice_directions_are_exact(lattice):
    """The kept set is invariant under the lattice symmetries that fix the line, so the principal axis IS the line.  The
    sign rule cannot be told apart from its mirror where two components tie in magnitude up to an ulp, so the vector is
    compared up to sign and the rule is checked on the returned vector."""
    vec, directed, lin, mom = _direction(DC.tube_mask(lattice))
    want = np.array(lattice, np.float64) / np.linalg.norm(lattice)
    assert directed and lin >= 0.5 and mom[0] >= SD.DIR_MIN_SUPPORT
    assert min(np.abs(vec - want).max(), np.abs(vec + want).max()) <= 1e-9
    assert vec[np.argmax(np.abs(vec))] > 0 and abs(np.linalg.norm(vec) - 1.0) <= 1e-12
    assert not mom[1:4].any(), "the tube is symmetric about the centre"


def test_sign_rule():
    """Moments of voxels along (1, -2, 0) and along (-1, -1, -3): the largest component comes out positive."""
    for pts in ([(1, -2, 0), (-1, 2, 0), (2, -4, 0), (-2, 4, 0)], [(-1, -1, -3), (1, 1, 3)]):
        p = np.array([(0, 0, 0)] + pts, np.int64)
        mom = np.array([[len(p), *p.sum(0), *(p * p).sum(0), (p[:, 0] * p[:, 1]).sum(), (p[:, 0] * p[:, 2]).sum(),
                         (p[:, 1] * p[:, 2]).sum()]], np.int32)
        vec, directed, lin = SD.seed_directions(mom, 2, 0.5)
        want = np.array(pts[0], np.float64) / np.linalg.norm(pts[0])
        want = want if want[np.argmax(np.abs(want))] > 0 else -want
        assert directed[0] and abs(lin[0] - 1.0) <= 1e-12 and np.abs(vec[0] - want).max() <= 1e-12


def test_crossing_lines_have_no_direction():
    keep = DC.tube_mask((1, 0, 0)) | DC.tube_mask((0, 1, 0))
    vec, directed, lin, mom = _direction(keep)
    assert mom[0] > 50 and abs(lin) <= 1e-12 and not directed and not vec.any()


def test_weak_support_has_no_direction():
    lone = np.zeros(17 ** 3, bool)
    lone[(8 * 17 + 8) * 17 + 8] = True
    vec, directed, lin, mom = _direction(lone)
    assert mom.tolist() == [1] + [0] * 9 and lin == 0.0 and not directed and not vec.any()
    few = lone.copy()
    for x in (6, 7, 9, 10):                       # five voxels in a row: perfectly linear, below min_support = 6
        few[(8 * 17 + 8) * 17 + x] = True
    vec, directed, lin, mom = _direction(few)
    assert mom[0] == 5 and abs(lin - 1.0) <= 1e-12 and not directed and not vec.any()
    vec, directed, _, _ = _direction(few, min_support=5)
    assert directed and np.abs(vec - [1.0, 0.0, 0.0]).max() <= 1e-12
    empty = SD.seed_directions(np.zeros((0, 10), np.int32))
    assert empty[0].shape == (0, 3) and empty[1].shape == (0,) and empty[2].shape == (0,)


def test_generic_directions_are_close():
    """A coarse quality guard: 100 random directions and sub-voxel offsets, tube radius 1.5, r = 6.  The bound of 8 degrees
    is twice the worst value (3.8) of an independent numpy experiment over tube radii 1, 1.5 and 2.5 at r = 6; this test
    measures 2.34 degrees."""
    directions, offsets = DC.generic_tubes(100, 0)
    worst = 0.0
    for d, off in zip(directions, offsets):
        vec, directed, _, _ = _direction(DC.tube_mask(d, off))
        assert directed
        worst = max(worst, float(DC.angle_deg(vec, d)[0]))
    print(f"worst angle over 100 generic tubes: {worst:.3f} degrees")
    assert worst <= 8.0


# ------------------------------------------------------------------------------------------------ the model layer
def test_initialize_bezier_curves_with_directions():
    from curve_gaussian_amd.scene import initialize_bezier_curves
    g = torch.Generator().manual_seed(0)
    p, b = torch.rand(7, 3, generator=g), 0.01 + torch.rand(7, 1, generator=g)
    plain = initialize_bezier_curves(p, b)
    assert torch.equal(plain, initialize_bezier_curves(p, b, directions=None))
    d = torch.nn.functional.normalize(torch.randn(7, 3, generator=g, dtype=torch.float64), dim=1)
    d[2] = 0.0
    d[5] = 0.0
    cp = initialize_bezier_curves(p, b, directions=d)
    assert cp.shape == (7, 4, 3) and cp.dtype == p.dtype
    zero = torch.tensor([2, 5])
    assert torch.equal(cp[zero], plain[zero]), "zero rows are laid along +-Y"
    rows = torch.tensor([0, 1, 3, 4, 6])
    chord = (cp[rows, 3] - cp[rows, 0]).double()
    want = 2.0 * b[rows].double() * d[rows]
    assert (chord - want).abs().max() <= 4 * 2.0 ** -24 * (p.abs().max() + b.max()), "P3 - P0 = 2 bound d in float32"
    assert torch.allclose(cp[:, 0] + cp[:, 3], 2 * p, atol=1e-6) and torch.allclose(cp[:, 1] + cp[:, 2], 2 * p, atol=1e-6)
    assert torch.allclose(cp[rows, 2] - cp[rows, 1], (b[rows].double() * d[rows]).float(), atol=1e-6)
    with pytest.raises(ValueError):
        initialize_bezier_curves(p, b, directions=d[:3])


# ------------------------------------------------------------------------------------------------ the drawn scan
def test_seed_points_without_directions_is_unchanged():
    cams, maps = SC.seed_novel_cameras()
    seeds, info = SD.seed_points(cams, maps, "PidiNet", SC.SEED_BOUNDS, backend="host", **SC.SEED_OPTIONS)
    off_seeds, off = SD.seed_points(cams, maps, "PidiNet", SC.SEED_BOUNDS, backend="host", directions=False, **SC.SEED_OPTIONS)
    assert sorted(info) == ["backend", "capped", "cells", "dims", "kept_voxels", "seeds", "views", "voxels"]
    assert info == off and np.array_equal(seeds, off_seeds)
    on_seeds, on = SD.seed_points(cams, maps, "PidiNet", SC.SEED_BOUNDS, backend="host", directions=True, **SC.SEED_OPTIONS)
    assert np.array_equal(on_seeds, seeds) and sorted(set(on) - set(info)) == ["directed", "directions"]
    assert on["directions"].shape == seeds.shape and on["directions"].dtype == np.float64
    norms = np.linalg.norm(on["directions"], axis=1)
    assert on["directed"] == int((norms > 0).sum()) and np.abs(norms[norms > 0] - 1.0).max() <= 1e-12
    with pytest.raises(ValueError, match="dir_radius"):
        SD.seed_points(cams, maps, "PidiNet", SC.SEED_BOUNDS, backend="host", directions=True, dir_radius=16, **SC.SEED_OPTIONS)


def test_drawn_scan_directions_follow_the_edges():
    """The six-view 48 x 64 scan of edge_seed_cases keeps tubes about 2.4 voxels in radius with ghosts between them (about
    half of its seeds are directed at r = 6), so this runs the twelve-view 96 x 128 scan of edge_dir_cases, at the default
    r = 6.  Measured: 267 of 271 seeds directed, median angle to the nearest drawn tangent 2.21 degrees, against 56.4
    degrees for +Y."""
    cams, maps = DC.dir_novel_cameras()
    seeds, info = SD.seed_points(cams, maps, "PidiNet", DC.DIR_BOUNDS, backend="host", directions=True, **DC.DIR_OPTIONS)
    vec = info["directions"]
    directed = np.linalg.norm(vec, axis=1) > 0
    tangents = DC.nearest_tangents(seeds)[directed]
    seeded = np.median(DC.angle_deg(vec[directed], tangents))
    along_y = np.median(DC.angle_deg(np.tile([0.0, 1.0, 0.0], (len(tangents), 1)), tangents))
    print(f"seeds {len(seeds)}, directed {info['directed']}, median angle {seeded:.3f} degrees, +Y {along_y:.3f} degrees")
    assert len(seeds) > 100 and info["directed"] == int(directed.sum())
    assert 2 * info["directed"] >= len(seeds), "at least half of the seeds are directed"
    assert seeded <= along_y / 3.0


def test_edge_vote_point_cloud_and_cli_carry_the_directions(tmp_path, capsys):
    from curve_gaussian_amd import edge_seed_cli as CLI
    from curve_gaussian_amd.scene import dataset_io as IO
    scan = SC.write_seed_scan(tmp_path, "emap", detector="PidiNet")
    options = dict(SC.SEED_OPTIONS, backend="host")
    cams = IO.read_emap(scan, detector="PidiNet")
    bounds = IO.default_seed_bounds("emap")
    plain = IO.edge_vote_point_cloud(cams, "PidiNet", bounds, **options)
    assert not np.asarray(plain.normals).any()
    cloud = IO.edge_vote_point_cloud(cams, "PidiNet", bounds, directions=True, **options)
    assert np.array_equal(cloud.points, plain.points)
    seeds, info = CLI.seed_scan(scan, "emap", "PidiNet", backend="host", directions=True, **SC.SEED_OPTIONS)
    assert np.array_equal(cloud.normals, info["directions"]) and 0 < info["directed"] <= len(seeds)
    out = tmp_path / "seeds.ply"
    argv = ["--scan", scan, "--detector", "PidiNet", "--backend", "host", "--out", str(out), "--grid", str(SC.SEED_GRID),
            "--tol_px", str(SC.SEED_TOL_PX), "--cell", str(SC.SEED_CELL)]
    assert CLI.main(argv + ["--directions"]) == 0
    assert f"directed {info['directed']}" in capsys.readouterr().out
    lines = out.read_text().splitlines()
    head = lines.index("end_header")
    assert lines[head - 3:head] == ["property double nx", "property double ny", "property double nz"]
    rows = np.array([[float(v) for v in ln.split()] for ln in lines[head + 1:]])
    assert rows.shape == (len(seeds), 6) and np.allclose(rows[:, :3], seeds, rtol=1e-9) and np.allclose(rows[:, 3:], info["directions"], atol=1e-9)
    assert CLI.main(argv) == 0
    assert "directed" not in capsys.readouterr().out and "property double nx" not in out.read_text()


def test_train_forwards_the_direction_options():
    from curve_gaussian_amd import train as T
    dataset, _, _ = T.parse_args(["-s", "scan", "-m", "out", "--init", "edge_votes", "--init_directions", "--init_dir_radius", "8",
                                  "--init_dir_min_support", "4", "--init_dir_min_linearity", "0.25"])
    assert dataset.init_options == {"directions": True, "dir_radius": 8, "dir_min_support": 4, "dir_min_linearity": 0.25}
    dataset, _, _ = T.parse_args(["-s", "scan", "-m", "out", "--init", "edge_votes"])
    assert dataset.init_options == {}
