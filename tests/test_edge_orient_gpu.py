"""GPU: cgs_mask_orientation, cgs_oriented_near and cgs_sample_support_oriented (csrc/edge_orient.hip) against the host back end
of ops.edge_orient, bit for bit -- plane sizes around the tile, densities, every disk, pre-filled outputs, hand-placed masks,
sample counts around a wave and a workgroup, random near bytes and partners, directions on the octant boundaries, chunks of
views, the distance transform and cgs_sample_support as cross-checks, the drawn scans end to end, and the argument errors."""
import numpy as np
import pytest
import torch

import edge_dir_cases as DC
import edge_orient_cases as C
import edge_support_cases as SC
import edge_trim_cases as TC
import test_edge_orient_cpu as CPU
from curve_gaussian_amd import _lib as L
from curve_gaussian_amd.ops import edge_orient as OR
from curve_gaussian_amd.ops import edge_score as ES
from curve_gaussian_amd.ops import edge_trim as ET

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ------------------------------------------------------------------------------------------------ the planes
@pytest.mark.parametrize("size", C.PLANE_SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_planes_against_the_host(size):
    H, W = size
    for density in C.DENSITIES:
        masks = C.random_masks(3, H, W, density)
        want = OR.mask_orientation(masks, backend="host")
        codes = OR.mask_orientation(masks, backend="gpu")
        assert codes.is_cuda and codes.dtype == torch.uint8 and torch.equal(codes.cpu(), want), density
        assert torch.equal(OR.mask_orientation(_dev(masks), device=DEV), codes), "a device tensor gives the same codes"
        for v in range(3):   # V = 1: a view's result does not depend on its neighbours
            assert torch.equal(OR.mask_orientation(masks[v:v + 1])[0], codes[v]), (density, v)
        for tol2 in C.TOL2S:
            near = OR.oriented_near(codes, C.TOL_PX[tol2])
            assert near.is_cuda and torch.equal(near.cpu(), OR.oriented_near(want, C.TOL_PX[tol2], backend="host")), (density, tol2)
        assert torch.equal(OR.oriented_near(codes[1:2], 2)[0], OR.oriented_near(codes, 2)[1])


@pytest.mark.parametrize("fill", [0x00, 0xFF])
def test_two_raw_calls_in_a_row_write_every_byte_and_nothing_else(fill):
    lib, s = L.load(), L.raw_stream(DEV)
    V, H, W = 3, C.TH + 1, C.TW + 1
    masks = C.random_masks(V, H, W, 0.3)
    want = OR.mask_orientation(masks, backend="host")
    m, n = _dev(masks), V * H * W
    guard = 64
    for tol2 in (0, 5, 16):
        code = torch.full((n + guard,), fill, dtype=torch.uint8, device=DEV)
        near = torch.full((n + guard,), fill, dtype=torch.uint8, device=DEV)
        for _ in range(2):
            assert lib.cgs_mask_orientation(V, H, W, L.ptr(m), L.ptr(code), s) == 0
            assert lib.cgs_oriented_near(V, H, W, L.ptr(code), tol2, L.ptr(near), s) == 0
        assert torch.equal(code[:n].cpu().reshape(V, H, W), want) and (code[n:] == fill).all()
        assert torch.equal(near[:n].cpu().reshape(V, H, W), OR.oriented_near(want, C.TOL_PX[tol2], backend="host"))
        assert (near[n:] == fill).all()


@pytest.mark.parametrize("offset", [0, 1, 2, 3])
def test_near_into_a_plane_that_starts_at_any_byte(offset):
    """Rows of a multiple of four pixels are stored a word at a time only where the output is word-aligned."""
    lib, s = L.load(), L.raw_stream(DEV)
    V, H, W = 2, C.TH + 3, C.TW + 4
    codes = OR.mask_orientation(C.random_masks(V, H, W, 0.3, seed=offset), backend="host")
    c, n = _dev(codes.numpy()), V * H * W
    near = torch.full((n + 8,), 0xAA, dtype=torch.uint8, device=DEV)
    assert lib.cgs_oriented_near(V, H, W, L.ptr(c), 5, L.ptr(near[offset:]), s) == 0
    assert torch.equal(near[offset:offset + n].cpu().reshape(V, H, W), OR.oriented_near(codes, C.TOL_PX[5], backend="host"))
    assert (near[:offset] == 0xAA).all() and (near[offset + n:] == 0xAA).all()


def test_hand_placed_masks():
    code = lambda m: OR.mask_orientation(m[None])[0].cpu().numpy()
    n = 15
    for kind, at, bit in (("h", 7, 0), ("v", 7, 4), ("d", 0, 2), ("a", n - 1, 6), ("h", 0, 0), ("h", n - 1, 0), ("v", 0, 4),
                          ("v", n - 1, 4)):
        m = C.line_mask(n, n, kind, at)
        got = code(m)
        assert (got[m != 0] == 1 << bit).all() and not got[m == 0].any(), (kind, at)
    m = np.zeros((9, 9), np.uint8)
    m[4, 4] = 1
    assert code(m)[4, 4] == 0xFF
    m[4, 5] = 1
    assert code(m)[4, 4:6].tolist() == [0xFF, 0xFF]
    plus = np.zeros((n, n), np.uint8)
    plus[7, :] = plus[:, 7] = 1
    assert code(plus)[7, 7] == 0xFF and code(plus)[7, 0] == 0x01 and code(plus)[0, 7] == 0x10
    block = np.ones((n, n), np.uint8)
    assert torch.equal(OR.mask_orientation(block[None]).cpu(), OR.mask_orientation(block[None], backend="host"))
    assert code(block)[7, 7] == 0xFF
    for offsets, _, _, o in CPU.TIES:
        assert code(CPU._window_mask(offsets))[3, 3] == 1 << o
    assert code(CPU._window_mask(CPU.COHERENT))[3, 3] == 1 << 2 and code(CPU._window_mask(CPU.INCOHERENT))[3, 3] == 0xFF


@pytest.mark.parametrize("tol2", C.TOL2S)
def test_near_is_nonzero_exactly_where_the_distance_transform_is_within_the_tolerance(tol2):
    for density in (0.0, 0.02, 0.3, 1.0):
        masks = _dev(C.random_masks(2, C.TH + 1, C.TW + 5, density, seed=tol2))
        near = OR.oriented_near(OR.mask_orientation(masks), C.TOL_PX[tol2])
        assert torch.equal(near != 0, ES.edt_squared(masks) <= tol2), density


# ------------------------------------------------------------------------------------------------ the tally
def _compare(pts, partner, K, M, near, spread):
    want = OR.oriented_tally(pts, partner, K, M, near, spread, backend="host")
    near_dev = _dev(near)
    got = OR.oriented_tally(pts, partner, K, M, near_dev, spread)
    assert got.is_cuda and got.dtype == torch.int32 and got.shape == want.shape
    assert torch.equal(got.cpu(), want), spread
    again = OR.oriented_tally(_dev(pts), _dev(partner), torch.from_numpy(K), torch.from_numpy(M), near_dev, spread, device=DEV)
    assert torch.equal(again, got), "device tensors give the same tally"
    return want.numpy()


@pytest.mark.parametrize("V", [1, 3, 12])
@pytest.mark.parametrize("P", TC.POINT_COUNTS)
def test_sample_counts_views_and_spreads(P, V):
    k = TC.POINT_COUNTS.index(P)
    pts, partner, K, M, near = CPU._tally_case(P, SC.WIDTHS[1 + (k + V) % 2], V, seed=k)
    for spread in range(5):
        want = _compare(pts, partner, K, M, near, spread)
    assert want.shape[0] == P
    if P >= 63:
        assert 0 < int(want[:, 0].sum()) < V * P, "points inside and outside the views"


def test_calls_add_up_and_a_tally_handed_in_is_added_to():
    pts, partner, K, M, near = CPU._tally_case(4096 + 65, 33, 12)
    near_dev = _dev(near)
    whole = OR.oriented_tally(pts, partner, K, M, near_dev)
    assert torch.equal(whole.cpu(), OR.oriented_tally(pts, partner, K, M, near, backend="host"))
    for cuts in ([0, 5, 12], [0, 1, 2, 9, 12]):
        out = torch.zeros_like(whole)
        for a, b in zip(cuts[:-1], cuts[1:]):
            assert OR.oriented_tally(pts, partner, K[a:b], M[a:b], near_dev[a:b], out=out) is out
        assert torch.equal(out, whole), cuts
    seven = torch.full_like(whole, 7)
    OR.oriented_tally(pts, partner, K, M, near_dev, out=seven)
    assert torch.equal(seven, whole + 7)
    none = OR.oriented_tally(pts, partner, K[:0], M[:0], near_dev[:0])
    assert none.is_cuda and tuple(none.shape) == (len(pts), 2) and not none.any()
    none = OR.oriented_tally(pts[:0], partner[:0], K, M, near_dev)
    assert none.is_cuda and tuple(none.shape) == (0, 2)


def test_the_raw_call_touches_its_rows_and_nothing_else():
    pts, partner, K, M, near = CPU._tally_case(257, 33, 2)
    sentinel = -12345
    out = torch.full((257 * 2 + 8,), sentinel, dtype=torch.int32, device=DEV)
    p, q, Kd, Md, nd = _dev(pts), _dev(partner), _dev(K), _dev(M.reshape(-1, 12)), _dev(near)
    rc = L.load().cgs_sample_support_oriented(257, L.ptr(p), L.ptr(q), 2, L.ptr(Kd), L.ptr(Md), SC.SUPPORT_H, 33, L.ptr(nd), 1,
                                              L.ptr(out), L.raw_stream(DEV))
    assert rc == 0
    want = OR.oriented_tally(pts, partner, K, M, near, backend="host") + sentinel
    assert torch.equal(out[:-8].cpu().reshape(257, 2), want) and (out[-8:] == sentinel).all()


def test_directions_on_the_octant_boundaries_and_one_step_beside_them():
    pts, partner, K, M, _ = C.hand_tally_case()
    for spread in range(5):
        _compare(pts, partner, K, M, C.random_near(len(K), C.HAND_SIZE, C.HAND_SIZE, seed=spread), spread)
    CPU.hand_tally_checks("gpu", _dev)


def test_all_ones_within_the_tolerance_give_the_tally_of_cgs_sample_support():
    V, W = 5, 67
    K, M = SC.support_cameras(V, W)
    d2 = _dev(SC.support_d2(V, W))
    pts = TC.tally_points(4096 + 65, W)
    partner = C.random_partners(len(pts))[0]
    for tol2 in (0, 4, 16):
        plain = ET.sample_tally(pts, K, M, d2, [C.TOL_PX[tol2]])
        near = (d2 <= tol2).to(torch.uint8) * 0xFF
        for spread in (0, 1, 4):
            assert torch.equal(OR.oriented_tally(pts, partner, K, M, near, spread), plain), (tol2, spread)
        assert plain[:, 1].sum() > 0


# ------------------------------------------------------------------------------------------------ the drawn scans
def _same(got, host):
    assert sorted(got) == sorted(host)
    assert torch.equal(got["tally"], host["tally"]) and not got["tally"].is_cuda
    assert got["spans"] == host["spans"] and got["edge_dict"] == host["edge_dict"]
    assert np.array_equal(got["source"], host["source"]) and np.array_equal(got["offsets"], host["offsets"])
    assert {**got["settings"], "backend": host["settings"]["backend"]} == host["settings"]


@pytest.mark.parametrize("setting", sorted(CPU.BOGUS), ids=lambda s: "tol%d-gap%d-span%d" % s)
def test_the_bogus_scan_agrees_with_the_host(setting):
    tol, gap, span = setting
    got = C.scan_trim("bogus", "gpu", tol, gap, span)
    _same(got, C.scan_trim("bogus", "host", tol, gap, span))
    plain = TC.scan_trim("bogus", "gpu", tol, None, gap, span)
    _same(C.scan_trim("bogus", "gpu", tol, gap, span, oriented=False), plain)
    p0, k0, whole0 = C.bogus_counts(plain)
    p1, k1, whole1 = C.bogus_counts(got)
    assert whole0 and whole1 and p1 < p0 and k1 < k0 and ((p0, k0), (p1, k1)) == CPU.BOGUS[setting]


def test_the_other_scans_and_the_chunks_agree_with_the_host():
    for tol in (1, 2):
        for gap, span in ((3, 10), (0, 2)):
            got = C.scan_trim("drawn", "gpu", tol, gap, span)
            _same(got, C.scan_trim("drawn", "host", tol, gap, span))
            assert all(len(s) == 1 for s in got["spans"])
        got = C.scan_trim("extended", "gpu", tol, 0, 2)
        _same(got, C.scan_trim("extended", "host", tol, 0, 2))
        assert (TC.cut_errors(got) <= TC.CUT_CAP[tol]).all()
        assert (TC.cut_errors(got) <= TC.cut_errors(TC.scan_trim("extended", "gpu", tol))).all()
    parts = C.scan_trim("bogus", "gpu", 1, budget_bytes=5 * OR.BYTES_PER_PIXEL * DC.DIR_H * DC.DIR_W)   # 5 + 5 + 2 views
    _same(parts, C.scan_trim("bogus", "host", 1))
    _same(C.scan_trim("bogus", "gpu", 1, dilate=5, thin=True), C.scan_trim("bogus", "host", 1, dilate=5, thin=True))


# ------------------------------------------------------------------------------------------------ errors
def test_argument_errors():
    pts, partner, K, M, near = CPU._tally_case(65, 33, 2)
    near_dev = _dev(near)
    with pytest.raises(L.CurveGSError, match="GPU tensor"):
        OR.oriented_tally(pts, partner, K, M, torch.from_numpy(near))
    with pytest.raises(L.CurveGSError, match="one device"):
        OR.oriented_tally(pts, partner, K, M, near_dev, device="cpu")
    with pytest.raises(L.CurveGSError, match="one device"):
        OR.oriented_tally(pts, partner, K, M, near_dev, out=torch.zeros((65, 2), dtype=torch.int32))
    with pytest.raises(ValueError, match="uint8"):
        OR.oriented_tally(pts, partner, K, M, near_dev.to(torch.int32))
    with pytest.raises(ValueError, match="int32"):
        OR.oriented_tally(pts, _dev(partner).long(), K, M, near_dev)
    with pytest.raises(ValueError, match="out must be"):
        OR.oriented_tally(pts, partner, K, M, near_dev, out=torch.zeros((65, 3), dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError, match="host"):
        OR.oriented_tally(pts, partner, K, M, near_dev, backend="host")
    with pytest.raises(ValueError, match="at most 4 pixels"):
        OR.oriented_near(near_dev, 5)
    lib, s = L.load(), L.raw_stream(DEV)
    p = L.ptr(near_dev)
    assert lib.cgs_oriented_near(2, SC.SUPPORT_H, 33, p, 1, p, s) == -1
    assert lib.cgs_last_error() == b"cgs_oriented_near: invalid argument (code and near overlap)"
    assert lib.cgs_sample_support_oriented(1, p, p, 1, p, p, 5, 33, p, 5, p, s) == -1
    assert lib.cgs_last_error() == b"cgs_sample_support_oriented: invalid argument (P=1, V=1, spread=5; the spread lies in [0, 4])"
    assert torch.equal(near_dev.cpu(), torch.from_numpy(near)), "a rejected call writes nothing"
