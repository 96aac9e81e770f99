"""GPU: cgs_sample_cover (csrc/edge_dedupe.hip) against the host back end of ops.edge_dedupe, bit for bit -- sample counts
around a wave and a tile, edge counts with empty and one-sample edges and rank ties, pairs exactly on the bound of the
distance and of the direction test, coincident points, clusters that straddle the tiles, whole tiles exactly a tolerance
apart (the box cull on its bound), a dirty workspace, the constructed scan end to end, and the argument errors."""
import numpy as np
import pytest
import torch

import edge_dedupe_cases as C
import edge_score_cases as EC
from curve_gaussian_amd import _lib as L
from curve_gaussian_amd.ops import edge_dedupe as ED

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _compare(pts, off, ranks, tolerance, cos_min):
    want = ED.sample_cover(pts, off, ranks, tolerance, cos_min, backend="host")
    got = ED.sample_cover(pts, off, ranks, tolerance, cos_min, backend="gpu")
    assert got.is_cuda and got.dtype == torch.int32 and got.shape == want.shape
    assert torch.equal(got.cpu(), want)
    return want.numpy()


@pytest.mark.parametrize("P,E", C.SHAPES)
def test_sample_and_edge_counts(P, E):
    pts, off, ranks = C.grid_case(P, E)
    want = _compare(pts, off, ranks, C.GRID_TOL, 0.9)
    assert want.shape == (P,)
    if P >= 256 and E >= 2:
        assert 0 < (want != C.NO_COVER).sum() < P, "covered and free samples"
    again = ED.sample_cover(torch.from_numpy(pts).to(DEV), torch.from_numpy(off).to(DEV), torch.from_numpy(ranks).to(DEV),
                            C.GRID_TOL, 0.9, device=DEV)
    assert torch.equal(again.cpu(), torch.from_numpy(want)), "device tensors give the same cover"


@pytest.mark.parametrize("cos_min", [0.0, 1.0])
def test_the_direction_test_at_its_ends(cos_min):
    """cos_min = 0: the direction test always passes; cos_min = 1: only parallel tangents pass, by equality."""
    pts, off, ranks = C.grid_case(4161, 65)
    want = _compare(pts, off, ranks, C.GRID_TOL, cos_min)
    assert 0 < (want != C.NO_COVER).sum() < len(want)


@pytest.mark.parametrize("cos_min", [0.0, 0.9, 1.0])
def test_equality_in_both_tests_covers(cos_min):
    pts, off, ranks, want = C.equality_case()
    assert np.array_equal(_compare(pts, off, ranks, C.GRID_TOL, cos_min), want)
    less = np.nextafter(np.float32(C.GRID_TOL), np.float32(0))
    assert (_compare(pts, off, ranks, less, cos_min)[40:70] == C.NO_COVER).all()


def test_coincident_points():
    pts, off, ranks, want = C.coincident_case()
    for cos_min in (0.0, 1.0):
        assert np.array_equal(_compare(pts, off, ranks, C.GRID_TOL, cos_min), want)


@pytest.mark.parametrize("cos_min", [0.0, 0.9])
def test_clusters_that_straddle_the_tiles(cos_min):
    pts, off, ranks = C.cluster_case()
    want = _compare(pts, off, ranks, C.GRID_TOL, cos_min)
    if cos_min == 0.0:
        for c in range(1, C.CLUSTERS):   # covered from the neighbouring cluster, at exactly the tolerance
            assert want[off[2 + 2 * c]] == ranks[1 + 2 * (c - 1)], c
    # a tolerance that reaches across many clusters, and one that reaches nothing
    _compare(pts, off, ranks, 8 * C.GRID_TOL, cos_min)
    assert (_compare(pts, off, ranks, float(C.GRID) / 2, cos_min) != C.NO_COVER).sum() < len(want)


@pytest.mark.parametrize("cos_min", [0.0, 0.9])
def test_whole_tiles_exactly_a_tolerance_apart(cos_min):
    """Tile-aligned clusters whose boxes are 5 cells apart: fl(g*g) == tol2 in the cull, in both directions, and a tile on
    that bound must not be skipped -- a pair at d2 == tol2 across it decides the cover.  At 6 cells the tile may be."""
    pts, off, ranks, queries = C.tile_gap_case(5)
    assert C.tile_box_gaps(pts, C.GRID_TOL)[0] == 2 * (C.GAP_CLUSTERS - 1)
    want = _compare(pts, off, ranks, C.GRID_TOL, cos_min)
    if cos_min == 0.0:
        assert [int(want[i]) for i, _ in queries] == [r for _, r in queries]
    wide, off6, ranks6, queries6 = C.tile_gap_case(6)
    assert C.tile_box_gaps(wide, C.GRID_TOL) == (0, C.GAP_CLUSTERS * (C.GAP_CLUSTERS - 1))
    want = _compare(wide, off6, ranks6, C.GRID_TOL, cos_min)
    assert all(int(want[i]) > r for i, r in queries6)
    # the same two inputs at a tolerance of 6 cells: now the wider gap is the one on the bound (36 * 2^-12 is exact too)
    six = 6.0 * float(C.GRID)
    assert C.tile_box_gaps(wide, six)[0] == 2 * (C.GAP_CLUSTERS - 1) and C.tile_box_gaps(pts, six) == (0, 20)
    want = _compare(wide, off6, ranks6, six, cos_min)
    if cos_min == 0.0:
        assert [int(want[i]) for i, _ in queries6] == [r for _, r in queries6]
    _compare(pts, off, ranks, six, cos_min)


def test_the_raw_call_twice_on_a_dirty_workspace():
    pts, off, ranks = C.grid_case(4161, 65)
    want = ED.sample_cover(pts, off, ranks, C.GRID_TOL, 0.9, backend="host")
    lib = L.load()
    P, E = len(pts), len(ranks)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    p, o, r = dev(pts), dev(off), dev(ranks)
    nbytes = int(lib.cgs_sample_cover_workspace_bytes(P))
    work = torch.full((nbytes + 64,), 0xFF, dtype=torch.uint8, device=DEV)
    cover = torch.full((P + 8,), -1, dtype=torch.int32, device=DEV)   # 0xFF bytes
    tol2 = float(np.float32(C.GRID_TOL) * np.float32(C.GRID_TOL))
    cos2 = float(np.float32(0.9) * np.float32(0.9))
    for _ in range(2):
        rc = lib.cgs_sample_cover(P, L.ptr(p), E, L.ptr(o), L.ptr(r), tol2, cos2, L.ptr(cover), L.ptr(work), L.raw_stream(DEV))
        assert rc == 0
        assert torch.equal(cover[:P].cpu(), want) and (cover[P:] == -1).all()
        assert (work[nbytes:] == 0xFF).all(), "nothing is written past the workspace"


def test_the_constructed_scan_agrees_with_the_host():
    for delta in (0.5, 1.0):
        host = C.constructed_dedupe(delta, "host")
        got = C.constructed_dedupe(delta, "gpu")
        assert sorted(got) == sorted(host)
        assert torch.equal(got["cover"], host["cover"]) and not got["cover"].is_cuda
        assert got["spans"] == host["spans"] and got["edge_dict"] == host["edge_dict"]
        assert got["covered_by"] == host["covered_by"] and np.array_equal(got["redundant"], host["redundant"])
        for key in ("source", "offsets", "ranks"):
            assert np.array_equal(got[key], host[key]), key
        assert {**got["settings"], "backend": "host"} == host["settings"]
    edges = C.trimmed_scan_edges()
    for k in (2, 8):
        both = [ED.dedupe_edges(edges, resolution=EC.SCAN_RESOLUTION, tolerance=k * EC.SCAN_RESOLUTION, backend=b)
                for b in ("host", "gpu")]
        assert torch.equal(both[0]["cover"], both[1]["cover"]) and both[0]["edge_dict"] == both[1]["edge_dict"]


def test_argument_errors():
    pts, off, ranks = C.grid_case(65, 2)
    on_gpu = torch.from_numpy(pts).to(DEV)
    with pytest.raises(L.CurveGSError, match="GPU tensor"):
        ED.sample_cover(torch.from_numpy(pts), off, ranks, C.GRID_TOL, 0.9)
    with pytest.raises(L.CurveGSError, match="contiguous"):
        ED.sample_cover(torch.zeros((65, 6), device=DEV)[:, ::2], off, ranks, C.GRID_TOL, 0.9)
    with pytest.raises(L.CurveGSError, match="one device"):
        ED.sample_cover(on_gpu, off, ranks, C.GRID_TOL, 0.9, device="cpu")
    with pytest.raises(ValueError, match="float32"):
        ED.sample_cover(on_gpu.double(), off, ranks, C.GRID_TOL, 0.9)
    with pytest.raises(ValueError, match="finite"):
        ED.sample_cover(torch.full((65, 3), float("nan"), device=DEV), off, ranks, C.GRID_TOL, 0.9)
    with pytest.raises(ValueError, match="host"):
        ED.sample_cover(on_gpu, off, ranks, C.GRID_TOL, 0.9, backend="host")
    with pytest.raises(ValueError, match="ranks"):
        ED.sample_cover(on_gpu, off, [0, 0], C.GRID_TOL, 0.9)
    lib = L.load()
    p = L.ptr(on_gpu)
    assert lib.cgs_sample_cover(1, p, 1, p, p, -1.0, 0.5, p, p, L.raw_stream(DEV)) == -1
    assert lib.cgs_last_error() == b"cgs_sample_cover: invalid argument (tol2=-1, cos2=0.5; tol2 >= 0 and cos2 lies in [0, 1])"
