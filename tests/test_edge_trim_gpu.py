"""GPU: cgs_sample_support (csrc/edge_trim.hip) against the host back end of ops.edge_trim, bit for bit -- sample counts around
a wave and a workgroup, widths, views and tolerances, points on the frame's bounds, accumulation over chunks of views, many
views, the per-edge sums against cgs_edge_support, the drawn scan end to end, and the argument errors."""
import numpy as np
import pytest
import torch

import edge_dir_cases as DC
import edge_support_cases as SC
import edge_trim_cases as C
from curve_gaussian_amd import _lib as L
from curve_gaussian_amd.ops import edge_score as ES
from curve_gaussian_amd.ops import edge_support as SP
from curve_gaussian_amd.ops import edge_trim as ET

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SENTINEL = -12345


def _case(P, width, V, tol, seed=0):
    K, M = SC.support_cameras(V, width)
    return C.tally_points(P, width, seed), K, M, SC.support_d2(V, width, seed), tol


def _compare(pts, K, M, d2, tol):
    want = ET.sample_tally(pts, K, M, d2, tol, backend="host")
    d2_dev = torch.from_numpy(d2).to(DEV)
    got = ET.sample_tally(pts, K, M, d2_dev, tol, backend="gpu")
    assert got.is_cuda and got.dtype == torch.int32 and got.shape == want.shape
    assert torch.equal(got.cpu(), want)
    again = ET.sample_tally(torch.from_numpy(pts).to(DEV), torch.from_numpy(K), torch.from_numpy(M), d2_dev, tol, device=DEV)
    assert torch.equal(again, got), "device tensors give the same tally"
    return want.numpy()


@pytest.mark.parametrize("P", C.POINT_COUNTS)
def test_sample_counts(P):
    k = C.POINT_COUNTS.index(P)
    want = _compare(*_case(P, SC.WIDTHS[k % 3], SC.VIEW_COUNTS[(k + 1) % 3], SC.TOLERANCES[k % 2], seed=k))
    assert want.shape[0] == P
    if P >= 63:
        assert 0 < int(want[:, 0].sum()) < SC.VIEW_COUNTS[(k + 1) % 3] * P, "points inside and outside the views"


@pytest.mark.parametrize("tol", SC.TOLERANCES, ids=["T1", "T4"])
@pytest.mark.parametrize("V", SC.VIEW_COUNTS)
@pytest.mark.parametrize("width", SC.WIDTHS)
def test_widths_views_and_tolerances(width, V, tol):
    pts, K, M, d2, tol = _case(4096 + 65, width, V, tol)
    want = _compare(pts, K, M, d2, tol)
    # the identity camera (view 0) keeps the special points on u = 0 and v = 0 and in the last row and column, and drops
    # those on u = width and v = height, behind it and at its eye: 4 of the first 8
    first = ET.sample_tally(pts[:8], K[:1], M[:1], torch.from_numpy(d2[:1]).to(DEV), (1,))
    assert first[:, 0].tolist() == [0, 0, 1, 1, 0, 0, 1, 1]
    assert (want[:, 1:] <= want[:, :1]).all() and 0 < want[:, 0].sum() < V * len(pts)
    if width > 1:   # (a plane of one column: few points fall into it)
        assert want[:, 0].max() == V and 0 < want[:, -1].sum() < want[:, 0].sum()


def test_calls_add_up_and_a_tally_handed_in_is_added_to():
    pts, K, M, d2, tol = _case(4096 + 65, 33, 5, (0, 1, 2.5, 5))
    d2_dev = torch.from_numpy(d2).to(DEV)
    whole = ET.sample_tally(pts, K, M, d2_dev, tol)
    out = torch.zeros_like(whole)
    assert ET.sample_tally(pts, K[:2], M[:2], d2_dev[:2], tol, out=out) is out
    ET.sample_tally(pts, K[2:], M[2:], d2_dev[2:], tol, out=out)
    assert torch.equal(out, whole) and torch.equal(whole.cpu(), ET.sample_tally(pts, K, M, d2, tol, backend="host"))
    seven = torch.full_like(whole, 7)
    ET.sample_tally(pts, K, M, d2_dev, tol, out=seven)
    assert torch.equal(seven, whole + 7)
    none = ET.sample_tally(pts, K[:0], M[:0], d2_dev[:0], (1,))
    assert none.is_cuda and tuple(none.shape) == (len(pts), 2) and not none.any()
    none = ET.sample_tally(pts[:0], K, M, d2_dev, (1,))
    assert none.is_cuda and tuple(none.shape) == (0, 2)


def test_the_raw_call_touches_its_rows_and_nothing_else():
    pts, K, M, d2, _ = _case(257, 33, 2, None)
    lib = L.load()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    p, Kd, Md, dd = dev(pts), dev(K), dev(M.reshape(-1, 12)), dev(d2)
    for tol in SC.TOLERANCES:
        T = len(tol)
        out = torch.full((257 * (1 + T) + 8,), SENTINEL, dtype=torch.int32, device=DEV)
        rc = lib.cgs_sample_support(257, L.ptr(p), 2, L.ptr(Kd), L.ptr(Md), SC.SUPPORT_H, 33, L.ptr(dd), T,
                                    L.ptr(dev(np.array(ES.tolerances_squared(tol), np.int32))), L.ptr(out), L.raw_stream(DEV))
        assert rc == 0
        want = ET.sample_tally(pts, K, M, d2, tol, backend="host") + SENTINEL
        assert torch.equal(out[:-8].cpu().reshape(257, 1 + T), want) and (out[-8:] == SENTINEL).all()


def test_many_views():
    """65537 views of one pixel and three points: more views than a grid dimension holds."""
    V = 65537
    rng = np.random.default_rng(4)
    K = np.tile(np.array([[1.0, 1.0, 0.0, 0.0]]), (V, 1))
    K[:, 2] = rng.uniform(-1.0, 1.0, V)   # u = X / Z + cx: in [0, 1) for about half of the views
    K[65535:, 2] = [0.25, -0.3]           # the last two views see points 0 and 1, and point 1 alone
    M = np.tile(np.eye(4)[None, :3, :4], (V, 1, 1))
    d2 = rng.integers(0, 3, (V, 1, 1)).astype(np.int32)
    d2[65535:, 0, 0] = [0, 2]
    pts = np.array([[0.25, 0.5, 1.0], [1.0, 1.0, 2.0], [0.5, 0.25, -1.0]], np.float32)
    _, _, keep = ES.project_points_host(pts, K, M.reshape(V, 12), 1, 1)           # [V,P], all views at once
    near = keep & (d2.reshape(V, 1) <= 1)
    want = np.stack([keep.sum(0), near.sum(0)], 1).astype(np.int32)
    assert np.stack([keep[65535:].sum(0), near[65535:].sum(0)], 1).tolist() == [[1, 1], [2, 1], [0, 0]]
    assert 0 < want[:, 1].sum() < want[:, 0].sum() and want[0, 0] > 20000
    got = ET.sample_tally(pts, K, M, torch.from_numpy(d2).to(DEV), (1,))
    assert torch.equal(got.cpu(), torch.from_numpy(want))


def test_the_edge_sums_equal_those_of_cgs_edge_support():
    K, M = SC.support_cameras(5, 67)
    d2 = torch.from_numpy(SC.support_d2(5, 67)).to(DEV)
    pts, off = SC.support_points(SC.edge_sizes(65), 67)
    tol = (0, 1, 2.5, 5)
    tally = ET.sample_tally(pts, K, M, d2, tol).cpu().numpy().astype(np.int64)
    counts = SP.support_counts(pts, off, K, M, d2, tol).cpu().numpy().astype(np.int64)
    run = np.concatenate([np.zeros((1, 5), np.int64), np.cumsum(tally, 0)])
    assert np.array_equal(run[off[1:]] - run[off[:-1]], counts.sum(1)) and counts.sum() > 0


def test_the_drawn_scan_agrees_with_the_host():
    host = C.scan_trim("extended", "host", 1)
    whole = C.scan_trim("extended", "gpu", 1)
    parts = C.scan_trim("extended", "gpu", 1, 5 * ET.BYTES_PER_PIXEL * DC.DIR_H * DC.DIR_W)   # 5 + 5 + 2 views
    for got in (whole, parts):
        assert sorted(got) == sorted(host)
        assert torch.equal(got["tally"], host["tally"]) and not got["tally"].is_cuda
        assert got["spans"] == host["spans"] and got["edge_dict"] == host["edge_dict"]
        assert np.array_equal(got["source"], host["source"]) and np.array_equal(got["offsets"], host["offsets"])
        assert {**got["settings"], "backend": "host"} == host["settings"]
    assert [len(s) for s in whole["spans"]] == [1, 1, 1, 1]
    for which in ("drawn", "bogus"):
        assert torch.equal(C.scan_trim(which, "gpu", 2)["tally"], C.scan_trim(which, "host", 2)["tally"]), which


def test_argument_errors():
    pts, K, M, d2, tol = _case(65, 33, 2, (1,))
    d2_dev = torch.from_numpy(d2).to(DEV)
    with pytest.raises(L.CurveGSError, match="GPU tensor"):
        ET.sample_tally(pts, K, M, torch.from_numpy(d2), tol)
    with pytest.raises(L.CurveGSError, match="one device"):
        ET.sample_tally(pts, K, M, d2_dev, tol, device="cpu")
    with pytest.raises(L.CurveGSError, match="one device"):
        ET.sample_tally(pts, K, M, d2_dev, tol, out=torch.zeros((65, 2), dtype=torch.int32))
    with pytest.raises(ValueError, match="int32"):
        ET.sample_tally(pts, K, M, d2_dev.to(torch.int64), tol)
    with pytest.raises(ValueError, match="float32"):
        ET.sample_tally(torch.from_numpy(pts).to(DEV).double(), K, M, d2_dev, tol)
    with pytest.raises(ValueError, match="out must be"):
        ET.sample_tally(pts, K, M, d2_dev, tol, out=torch.zeros((65, 3), dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError, match="host"):
        ET.sample_tally(pts, K, M, d2_dev, tol, backend="host")
    lib = L.load()
    p = L.ptr(d2_dev)
    assert lib.cgs_sample_support(1, p, 1, p, p, 5, 33, p, 5, p, p, L.raw_stream(DEV)) == -1
    assert lib.cgs_last_error() == b"cgs_sample_support: invalid argument (P=1, V=1, T=5; T lies in [1, 4])"
