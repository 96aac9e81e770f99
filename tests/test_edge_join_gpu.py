"""GPU: cgs_end_attach (csrc/edge_join.hip) against the host back end of ops.edge_join, bit for bit -- sample counts around a
wave and a tile, edge counts up to a second tile of ends, edges without samples and of one and two samples, every
comparison of the rule exactly on its bound next to the input that fails it, ties, coincident points, the end's own edge,
the answer in the last partial tile and in another split than the runner-up, reach below the tolerance and none, dirty
buffers, the drawn fixtures end to end, and the argument errors."""
import numpy as np
import pytest
import torch

import edge_dedupe_cases as C
import edge_join_cases as J
import edge_score_cases as EC
from curve_gaussian_amd import _lib as L
from curve_gaussian_amd.ops import edge_join as EJ

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _compare(pts, off, tolerance, reach):
    want = EJ.end_attach(pts, off, tolerance, reach, backend="host")
    got = EJ.end_attach(pts, off, tolerance, reach, backend="gpu")
    assert got.is_cuda and got.dtype == torch.int64 and got.shape == want.shape
    assert torch.equal(got.cpu(), want)
    return want.numpy()


@pytest.mark.parametrize("P,E", J.SHAPES)
def test_sample_and_edge_counts(P, E):
    pts, off = J.grid_case(P, E)
    want = _compare(pts, off, J.GRID_TOL, J.GRID_REACH)
    assert want.shape == (2 * E,)
    if P >= 255 and E >= 2:
        assert (want != J.NO_ATTACH).any()
    _compare(pts, off, J.GRID_TOL, 2 * float(J.GRID))    # reach < tolerance
    _compare(pts, off, J.GRID_TOL, 0.0)                  # reach == 0
    again = EJ.end_attach(torch.from_numpy(pts).to(DEV), torch.from_numpy(off).to(DEV), J.GRID_TOL, J.GRID_REACH, device=DEV)
    assert torch.equal(again.cpu(), torch.from_numpy(want)), "device tensors give the same keys"


@pytest.mark.parametrize("name", [row[0] for row in J.PLACED])
def test_every_comparison_on_its_bound(name):
    pts, off, tol, reach, key = J.placed_case(name)
    assert _compare(pts, off, tol, reach)[1] == key


def test_coincident_points():
    pts, off, want = J.coincident_case()
    assert np.array_equal(_compare(pts, off, J.GRID_TOL, J.GRID_REACH), want)
    assert np.array_equal(_compare(pts, off, J.GRID_TOL, 0.0), want)


@pytest.mark.parametrize("swap", [False, True])
def test_the_answer_in_the_last_partial_tile_and_in_another_split(swap):
    pts, off, key = J.split_case(swap)
    assert _compare(pts, off, J.GRID_TOL, J.GRID_REACH)[1] == key


@pytest.mark.parametrize("fill", [0x00, 0xFF])
def test_the_raw_call_twice_on_dirty_buffers(fill):
    pts, off = J.grid_case(4161, 129)
    want = EJ.end_attach(pts, off, J.GRID_TOL, J.GRID_REACH, backend="host")
    lib = L.load()
    P, E = len(pts), len(off) - 1
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    p, o = dev(pts), dev(off)
    nbytes = int(lib.cgs_end_attach_workspace_bytes(P, E))
    work = torch.full((nbytes + 64,), fill, dtype=torch.uint8, device=DEV)
    keys = torch.full((2 * E + 8,), -1 if fill else 0, dtype=torch.int64, device=DEV)
    tol2 = float(np.float32(J.GRID_TOL) * np.float32(J.GRID_TOL))
    reach2 = float(np.float32(J.GRID_REACH) * np.float32(J.GRID_REACH))
    for _ in range(2):
        rc = lib.cgs_end_attach(P, L.ptr(p), E, L.ptr(o), tol2, reach2, L.ptr(keys), L.ptr(work), L.raw_stream(DEV))
        assert rc == 0
        assert torch.equal(keys[:2 * E].cpu(), want) and (keys[2 * E:] == (-1 if fill else 0)).all()
        assert (work[nbytes:] == fill).all(), "nothing is written past the workspace"


def test_the_drawn_fixtures_agree_with_the_host():
    """(a) the shortened scan: the corner vertex within 1e-5 (test_edge_join_cpu.py derives the bound) for g = 1, 3, 5,
    nothing at 7, the shared point at 0; (b) the constructed scan after deduping: one end-to-end vertex, three T-junctions
    on their own drawn lines; (c) the trimmed scan: the invariants -- each the same through the kernel."""
    for g in (0, 1, 3, 5, 7):
        host, got = J.join_scan(J.shortened_scan(g), "host"), J.join_scan(J.shortened_scan(g), "gpu")
        J.same_result(got, host)
        assert not got["keys"].is_cuda
        a, b = J.CORNER_ENDS
        ends = got["edge_vertices"].reshape(-1)
        if g == 7:
            assert (got["attach"]["kind"] == 0).all()
        else:
            assert ends[a] == ends[b] and np.linalg.norm(got["vertices"][ends[a]] - J.CORNER) < 1e-5
            assert g > 0 or got["vertices"][ends[a]].tobytes() == J.CORNER.tobytes()
    host, got = J.join_scan(J.constructed_pieces(), "host"), J.join_scan(J.constructed_pieces(), "gpu")
    J.same_result(got, host)
    assert got["attach"]["kind"].tolist() == [0, 0, 0, 1, 1, 0, 0, 0, 2, 0, 2, 0, 2, 0]
    assert [(t["end"], t["host"], t["sample"]) for t in got["t_junctions"]] == [(8, 1, 86), (10, 2, 95), (12, 3, 100)]
    edges = C.trimmed_scan_edges()
    host, got = (EJ.join_edges(edges, resolution=EC.SCAN_RESOLUTION, backend=b) for b in ("host", "gpu"))
    J.same_result(got, host)
    assert (got["moved"] <= J.SCAN_REACH).all() and 0 <= got["edge_vertices"].min()
    assert got["edge_vertices"].max() < len(got["vertices"])


def test_argument_errors():
    pts, off = J.grid_case(65, 2)
    on_gpu = torch.from_numpy(pts).to(DEV)
    with pytest.raises(L.CurveGSError, match="GPU tensor"):
        EJ.end_attach(torch.from_numpy(pts), off, J.GRID_TOL, J.GRID_REACH)
    with pytest.raises(L.CurveGSError, match="contiguous"):
        EJ.end_attach(torch.zeros((65, 6), device=DEV)[:, ::2], off, J.GRID_TOL, J.GRID_REACH)
    with pytest.raises(L.CurveGSError, match="one device"):
        EJ.end_attach(on_gpu, off, J.GRID_TOL, J.GRID_REACH, device="cpu")
    with pytest.raises(ValueError, match="float32"):
        EJ.end_attach(on_gpu.double(), off, J.GRID_TOL, J.GRID_REACH)
    with pytest.raises(ValueError, match="finite"):
        EJ.end_attach(torch.full((65, 3), float("nan"), device=DEV), off, J.GRID_TOL, J.GRID_REACH)
    with pytest.raises(ValueError, match="host"):
        EJ.end_attach(on_gpu, off, J.GRID_TOL, J.GRID_REACH, backend="host")
    lib = L.load()
    p = L.ptr(on_gpu)
    stream = L.raw_stream(DEV)
    fn = "cgs_end_attach: invalid argument "
    rows = [((-1, p, 1, p, 0.5, 0.5, p, p), "(P=-1, E=1)"), ((1, p, -1, p, 0.5, 0.5, p, p), "(P=1, E=-1)"),
            ((1, p, 1, p, -1.0, 0.5, p, p), "(tol2=-1, reach2=0.5; neither may be negative or NaN)"),
            ((1, p, 1, p, 0.5, float("nan"), p, p), "(tol2=0.5, reach2=nan; neither may be negative or NaN)"),
            ((1, None, 1, p, 0.5, 0.5, p, p), "(NULL pointer; P=1, E=1)"), ((1, p, 1, None, 0.5, 0.5, p, p), "(NULL pointer; P=1, E=1)"),
            ((1, p, 1, p, 0.5, 0.5, None, p), "(NULL pointer; P=1, E=1)"), ((1, p, 1, p, 0.5, 0.5, p, None), "(NULL pointer; P=1, E=1)")]
    for args, text in rows:
        assert lib.cgs_end_attach(*args, stream) == -1 and lib.cgs_last_error().decode() == fn + text, args
    assert lib.cgs_end_attach(1, p, 0, p, 0.5, 0.5, None, p, stream) == 0, "no edge: nothing is launched"
