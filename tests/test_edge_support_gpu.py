"""GPU: cgs_edge_support against the host back end, bit for bit -- edge counts, points per edge, widths, views and
tolerances, empty offsets, points on the frame's bounds, more views than one launch takes, the chunking of edge_support,
the drawn scan end to end, and the argument errors."""
import numpy as np
import pytest
import torch

import edge_dir_cases as DC
import edge_score_cases as EC
import edge_support_cases as C
from curve_gaussian_amd import _lib as L
from curve_gaussian_amd.ops import edge_score as ES
from curve_gaussian_amd.ops import edge_support as SP

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SENTINEL = -12345


def _case(E, width, V, tol, seed=0):
    K, M = C.support_cameras(V, width)
    d2 = C.support_d2(V, width, seed)
    pts, off = C.support_points(C.edge_sizes(E, seed), width, seed)
    return pts, off, K, M, d2, tol


def _compare(pts, off, K, M, d2, tol):
    want = SP.support_counts(pts, off, K, M, d2, tol, backend="host")
    d2_dev = torch.from_numpy(d2).to(DEV)
    got = SP.support_counts(pts, off, K, M, d2_dev, tol, backend="gpu")
    assert got.is_cuda and got.dtype == torch.int32 and got.shape == want.shape
    assert torch.equal(got.cpu(), want)
    again = SP.support_counts(torch.from_numpy(pts).to(DEV), torch.from_numpy(off).to(DEV), torch.from_numpy(K),
                              torch.from_numpy(M), d2_dev, tol, backend="gpu", device=DEV)
    assert torch.equal(again, got), "device tensors give the same counts"
    return want


@pytest.mark.parametrize("E", C.EDGE_COUNTS)
def test_edge_counts(E):
    k = C.EDGE_COUNTS.index(E)
    case = _case(E, C.WIDTHS[k % 3], C.VIEW_COUNTS[(k + 1) % 3], C.TOLERANCES[k % 2], seed=k)
    want = _compare(*case)
    assert tuple(want.shape)[0] == E
    if E >= 63:
        assert 0 < int(want[:, :, 0].sum()) < want.shape[1] * len(case[0]), "points inside and outside the views"


@pytest.mark.parametrize("tol", C.TOLERANCES, ids=["T1", "T4"])
@pytest.mark.parametrize("V", C.VIEW_COUNTS)
@pytest.mark.parametrize("width", C.WIDTHS)
def test_widths_views_and_tolerances(width, V, tol):
    pts, off, K, M, d2, tol = _case(65, width, V, tol)
    sizes = np.diff(off)
    assert set(C.POINT_COUNTS) <= set(sizes.tolist()), "every point count in one call"
    want = _compare(pts, off, K, M, d2, tol).numpy()
    # the identity camera (view 0) keeps the special points on u = 0 and v = 0 and in the last row and column, and drops
    # those on u = width and v = height, behind it and at its eye: 4 of the 8
    e = int(np.argmax(sizes == 4096))
    first = SP.support_counts(pts[off[e]:off[e] + 8], [0, 8], K[:1], M[:1], torch.from_numpy(d2[:1]).to(DEV), (1,))
    assert int(first[0, 0, 0]) == 4
    assert not want[sizes == 0].any() and want[:, :, 0].max() > 64, "a lane sees more than one point of an edge"


def test_the_raw_call_writes_every_word_and_nothing_else():
    pts, off, K, M, d2, _ = _case(65, 33, 2, None)
    lib = L.load()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    p, o, Kd, Md, dd = dev(pts), dev(off), dev(K), dev(M.reshape(-1, 12)), dev(d2)
    E, V = len(off) - 1, 2
    for tol in C.TOLERANCES:
        T = len(tol)
        tol2 = ES.tolerances_squared(tol)
        out = torch.full((E * V * (1 + T) + 8,), SENTINEL, dtype=torch.int32, device=DEV)
        rc = lib.cgs_edge_support(E, len(pts), L.ptr(p), L.ptr(o), V, L.ptr(Kd), L.ptr(Md), C.SUPPORT_H, 33, L.ptr(dd), T,
                                  L.ptr(dev(np.array(tol2, np.int32))), L.ptr(out), L.raw_stream(DEV))
        assert rc == 0
        want = SP.support_counts(pts, off, K, M, d2, tol, backend="host")
        assert torch.equal(out[:-8].cpu().reshape(E, V, 1 + T), want) and (out[-8:] == SENTINEL).all()


def test_all_empty_offsets_and_no_views():
    K, M = C.support_cameras(2, 33)
    d2 = torch.from_numpy(C.support_d2(2, 33)).to(DEV)
    none = np.zeros((0, 3), np.float32)
    got = SP.support_counts(none, np.zeros(66, np.int32), K, M, d2, (1, 2))
    assert got.is_cuda and tuple(got.shape) == (65, 2, 3) and not got.any()
    got = SP.support_counts(none, [0], K, M, d2, (1,))
    assert tuple(got.shape) == (0, 2, 2)
    pts, off = C.support_points(np.array([3, 0, 9]), 33)
    got = SP.support_counts(pts, off, K[:0], M[:0], d2[:0], (1,))
    assert got.is_cuda and tuple(got.shape) == (3, 0, 2)


def test_more_views_than_one_launch_takes():
    """65537 views of one pixel: the second launch starts at view 65535."""
    V = 65537
    rng = np.random.default_rng(4)
    K = np.tile(np.array([[1.0, 1.0, 0.0, 0.0]]), (V, 1))
    K[:, 2] = rng.uniform(-1.0, 1.0, V)   # u = X / Z + cx: in [0, 1) for about half of the views
    K[65535:, 2] = [0.25, -0.3]           # the two views of the second launch see two points and one point of edge 0
    M = np.tile(np.eye(4)[None, :3, :4], (V, 1, 1))
    d2 = rng.integers(0, 3, (V, 1, 1)).astype(np.int32)
    d2[65535:, 0, 0] = [0, 2]
    pts = np.array([[0.25, 0.5, 1.0], [1.0, 1.0, 2.0], [0.5, 0.25, -1.0], [0.0, 0.0, 4.0]], np.float32)
    off = np.array([0, 3, 3, 4], np.int32)
    _, _, keep = ES.project_points_host(pts, K, M.reshape(V, 12), 1, 1)           # [V,P]
    near = keep & (d2.reshape(V, 1) <= 1)
    want = np.zeros((3, V, 2), np.int32)
    for e in range(3):
        want[e, :, 0] = keep[:, off[e]:off[e + 1]].sum(1)
        want[e, :, 1] = near[:, off[e]:off[e + 1]].sum(1)
    assert want[0, 65535:].tolist() == [[2, 2], [1, 0]] and 0 < want[:, :, 1].sum() < want[:, :, 0].sum()
    got = SP.support_counts(pts, off, K, M, torch.from_numpy(d2).to(DEV), (1,))
    assert torch.equal(got.cpu(), torch.from_numpy(want))


def test_the_drawn_scan_agrees_key_for_key_at_two_chunkings():
    host = C.scan_support("host", 2)
    whole = C.scan_support("gpu", 2)
    parts = C.scan_support("gpu", 2, budget_bytes=5 * SP.BYTES_PER_PIXEL * DC.DIR_H * DC.DIR_W)   # 5 + 5 + 2 views
    single = C.scan_support("gpu", 2, budget_bytes=1)                                            # one view at a time
    drawn = C.scan_edges()[1]
    for got in (whole, parts, single):
        assert sorted(got) == sorted(host)
        for key in host:
            if key == "settings":
                assert {**got[key], "backend": "host"} == host[key]
            elif key == "counts":
                assert torch.equal(got[key], host[key])
            else:
                assert np.array_equal(got[key], host[key], equal_nan=key == "share"), key
        assert np.array_equal(got["kept"], drawn)


def test_argument_errors():
    pts, off, K, M, d2, tol = _case(3, 33, 2, (1,))
    d2_dev = torch.from_numpy(d2).to(DEV)
    with pytest.raises(L.CurveGSError, match="GPU tensor"):
        SP.support_counts(pts, off, K, M, torch.from_numpy(d2), tol)
    with pytest.raises(L.CurveGSError, match="GPU tensor"):
        SP.support_counts(pts, off, K, M, d2, tol, backend="gpu")
    with pytest.raises(L.CurveGSError, match="one device"):
        SP.support_counts(pts, off, K, M, d2_dev, tol, device="cpu")
    with pytest.raises(ValueError, match="int32"):
        SP.support_counts(pts, off, K, M, d2_dev.to(torch.int64), tol)
    with pytest.raises(ValueError, match="float32"):
        SP.support_counts(torch.from_numpy(pts).to(DEV).double(), off, K, M, d2_dev, tol)
    with pytest.raises(ValueError, match="offsets"):
        SP.support_counts(pts, torch.from_numpy(off).to(DEV).float(), K, M, d2_dev, tol)
    with pytest.raises(ValueError, match="offsets"):
        SP.support_counts(pts, off[:-1], K, M, d2_dev, tol)
    with pytest.raises(ValueError, match="host"):
        SP.support_counts(pts, off, K, M, d2_dev, tol, backend="host")
    lib = L.load()
    p = L.ptr(d2_dev)
    assert lib.cgs_edge_support(1, 1, p, p, 1, p, p, 5, 33, p, 5, p, p, L.raw_stream(DEV)) == -1
    assert b"cgs_edge_support: invalid argument" in lib.cgs_last_error()
