"""Host: orientation-aware 2D support (ops.edge_orient: mask_orientation, oriented_near, sample_partners, oriented_tally) on
the numpy back end -- the three planes and the tally against brute-force definitions, hand-placed masks with their moments
written out, directions on every octant boundary, the drawn scans trimmed with and without orientation, the command line, the
driver's options and the C ABI's argument checks."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import edge_dir_cases as DC
import edge_orient_cases as C
import edge_support_cases as SC
import edge_trim_cases as TC
from curve_gaussian_amd.ops import edge_orient as OR
from curve_gaussian_amd.ops import edge_score as ES
from curve_gaussian_amd.ops import edge_trim as ET


# ------------------------------------------------------------------------------------------------ the planes
@pytest.mark.parametrize("size", [s for s in C.PLANE_SIZES if s[0] * s[1] <= 64 * 65], ids=lambda s: f"{s[0]}x{s[1]}")
def test_codes_and_near_against_the_brute_force(size):
    H, W = size
    densities = C.DENSITIES if H * W <= 64 else [0.02, 0.3]   # the brute force is a Python loop
    for density in densities:
        masks = C.random_masks(3, H, W, density)
        codes = OR.mask_orientation(masks, backend="host")
        assert codes.dtype == torch.uint8 and tuple(codes.shape) == (3, H, W)
        want = C.codes_brute(masks)
        assert np.array_equal(codes.numpy(), want), density
        assert np.array_equal(codes.numpy() != 0, masks != 0)
        for v in range(3):   # a view's result does not depend on its neighbours
            assert np.array_equal(OR.mask_orientation(masks[v:v + 1], backend="host")[0].numpy(), want[v])
        for tol2 in (C.TOL2S if H * W <= 64 else [1, 5, 16]):
            near = OR.oriented_near(codes, C.TOL_PX[tol2], backend="host")
            assert np.array_equal(near.numpy(), C.near_brute(want, tol2)), (density, tol2)


def test_the_tolerances_give_the_squares_of_the_issue():
    assert [ES.tolerances_squared([C.TOL_PX[t]])[0] for t in C.TOL2S] == C.TOL2S
    assert OR._tol2(4) == 16 and OR._tol2(1) == 1 and OR._tol2(2.5) == 6


@pytest.mark.parametrize("tol2", C.TOL2S)
def test_near_is_nonzero_exactly_where_the_distance_transform_is_within_the_tolerance(tol2):
    for density in (0.0, 0.02, 0.3, 1.0):
        masks = C.random_masks(2, 33, 37, density, seed=tol2)
        near = OR.oriented_near(OR.mask_orientation(masks, backend="host"), C.TOL_PX[tol2], backend="host").numpy()
        d2 = ES.edt_squared(masks, backend="host").numpy()
        assert np.array_equal(near != 0, d2 <= tol2), density


def test_octants_of_the_table():
    """Every sign pattern and the ties of the table, for the integer and the float reading."""
    rows = [((1, 0), 0), ((2, 1), 0), ((1, 1), 1), ((1, 2), 1), ((0, 1), 2), ((-1, 2), 2), ((-1, 1), 3), ((-2, 1), 3),
            ((-1, 0), 4), ((-2, -1), 4), ((-1, -1), 5), ((-1, -2), 5), ((0, -1), 6), ((1, -2), 6), ((1, -1), 7), ((2, -1), 7)]
    for (a, b), o in rows:
        assert C.octant(a, b) == o and C.octant(float(a), float(b)) == o
    a, b = np.array([r[0][0] for r in rows]), np.array([r[0][1] for r in rows])
    want = [r[1] for r in rows]
    assert OR.octant_host(a, b).tolist() == want and OR.octant_host(a.astype(np.float64), b * 0.5 * 2).tolist() == want
    assert [int(OR.accept_bits_host(np.array([o]), s)[0]) for o, s in ((0, 0), (0, 1), (7, 1), (3, 2), (5, 3), (2, 4))] == \
        [0x01, 0x83, 0xC1, 0x3E, 0xFD, 0xFF]
    for o in range(8):
        for s in range(5):
            a, b = [(2, 1), (1, 2), (-1, 2), (-2, 1), (-2, -1), (-1, -2), (1, -2), (2, -1)][o]
            assert int(OR.accept_bits_host(np.array([o]), s)[0]) == C.accept_bits(a, b, s)


def _code_at(mask, y, x, backend="host"):
    return int(OR.mask_orientation(mask[None], backend=backend)[0, y, x])


def test_lines_give_their_bits_in_the_open_and_along_the_border():
    """One-pixel lines through a 15 x 15 image.  A pixel in the middle of a horizontal line sees N = 7, Sx = Sy = 0,
    Sxx = 28, Syy = Sxy = 0: A = 196, B = C = 0, (a, b) = (196, 0), coherence 4 * 196^2 >= 196^2, octant 0.  Vertical: A and
    C swap, (a, b) = (-196, 0), octant 4.  y = x: Sxx = Syy = Sxy = 28, A = B = C = 196, (a, b) = (0, 392), octant 2;
    y = -x: Sxy = -28, (a, b) = (0, -392), octant 6.  On the border the window is clipped: the corner pixel of a line along
    the border sees N = 4, Sx = 6, Sxx = 14, A = 56 - 36 = 20, (a, b) = (20, 0): octant 0 still."""
    n = 15
    for kind, at, bit, pixel in (("h", 7, 0, (7, 7)), ("v", 7, 4, (7, 7)), ("d", 0, 2, (7, 7)), ("a", n - 1, 6, (7, 7))):
        m = C.line_mask(n, n, kind, at)
        assert C.derived(C.moments(m, *pixel))[3:] == {0: (196, 0), 4: (-196, 0), 2: (0, 392), 6: (0, -392)}[bit]
        codes = OR.mask_orientation(m[None], backend="host")[0].numpy()
        assert (codes[m != 0] == 1 << bit).all() and not codes[m == 0].any(), kind
    for kind, at, bit in (("h", 0, 0), ("h", n - 1, 0), ("v", 0, 4), ("v", n - 1, 4)):
        m = C.line_mask(n, n, kind, at)
        codes = OR.mask_orientation(m[None], backend="host")[0].numpy()
        assert (codes[m != 0] == 1 << bit).all(), (kind, at)
    corner = C.moments(C.line_mask(n, n, "h", 0), 0, 0)
    assert corner == (4, 6, 0, 14, 0, 0) and C.derived(corner) == (20, 0, 0, 20, 0)


def test_pixels_without_an_orientation_accept_everything():
    """A lone pixel (N = 1) and a pair (N = 2) are below N >= 3.  A plus junction of two 7-pixel lines has N = 13,
    Sxx = Syy = 28, Sx = Sy = Sxy = 0: A = C = 364, B = 0, (a, b) = (0, 0).  A full block has N = 49, Sxx = Syy = 196:
    A = C = 9604, (a, b) = (0, 0) again."""
    m = np.zeros((9, 9), np.uint8)
    m[4, 4] = 1
    assert _code_at(m, 4, 4) == 0xFF and C.moments(m, 4, 4)[0] == 1
    m[4, 5] = 1
    assert _code_at(m, 4, 4) == 0xFF and _code_at(m, 4, 5) == 0xFF and C.moments(m, 4, 4)[0] == 2
    m[4, 6] = 1
    assert _code_at(m, 4, 5) == 0x01, "three in a row are a line"
    plus = np.zeros((15, 15), np.uint8)
    plus[7, :] = plus[:, 7] = 1
    assert C.moments(plus, 7, 7) == (13, 0, 0, 28, 28, 0) and C.derived(C.moments(plus, 7, 7)) == (364, 0, 364, 0, 0)
    assert _code_at(plus, 7, 7) == 0xFF and _code_at(plus, 7, 0) == 0x01 and _code_at(plus, 0, 7) == 0x10
    block = np.ones((15, 15), np.uint8)
    assert C.moments(block, 7, 7) == (49, 0, 0, 196, 196, 0) and C.derived(C.moments(block, 7, 7))[:3] == (9604, 0, 9604)
    assert _code_at(block, 7, 7) == 0xFF
    assert 4 * (19208 ** 2) < 2 ** 31, "the largest (A + C)^2 times four fits 32 bits"


# (dy, dx) of the set pixels around a centre; their moments; (A, B, C, a, b); the octant the table gives the tie.  Found by a
# search over the four-pixel patterns of a window; no three-pixel pattern has |a| == |b|.
TIES = [(((-3, -3), (-3, 2), (0, 3)), (4, 2, -6, 22, 18, 3), (84, 24, 36, 48, 48), 1),
        (((-3, -3), (-2, 1), (3, 0)), (4, -2, -2, 10, 22, 7), (36, 24, 84, -48, 48), 3),
        (((-3, -1), (-1, -2), (2, -3)), (4, -6, -2, 14, 14, -1), (20, -16, 52, -32, -32), 5),
        (((-3, -2), (-3, 3), (0, -3)), (4, -2, -6, 22, 18, -3), (84, -24, 36, 48, -48), 7)]


def _window_mask(offsets):
    m = np.zeros((7, 7), np.uint8)
    m[3, 3] = 1
    for dy, dx in offsets:
        m[3 + dy, 3 + dx] = 1
    return m


def test_ties_of_the_magnitudes_go_where_the_table_sends_them():
    for offsets, mom, der, o in TIES:
        m = _window_mask(offsets)
        assert C.moments(m, 3, 3) == mom and C.derived(mom) == der and abs(der[3]) == abs(der[4])
        assert 4 * (der[3] ** 2 + der[4] ** 2) >= (der[0] + der[2]) ** 2, "oriented"
        assert C.octant(der[3], der[4]) == o and _code_at(m, 3, 3) == 1 << o


# A pattern whose coherence is 0.5 exactly: N = 4, (Sx, Sy) = (-4, -8), (Sxx, Syy, Sxy) = (10, 22, 11), A = C = 24, B = 12,
# (a, b) = (0, 24), 4 (0 + 576) = 2304 = 48^2 -- oriented, octant 2.  One more pixel at (-3, -1): N = 5, (-5, -11),
# (11, 31, 14), A = 30, B = 15, C = 34, (a, b) = (-4, 30), 4 (16 + 900) = 3664 < 64^2 = 4096 -- not oriented.
COHERENT = ((-3, -3), (-3, 0), (-2, -1))
INCOHERENT = COHERENT + ((-3, -1),)


def test_the_coherence_bound_is_met_with_equality_and_missed_by_one_pixel():
    m = _window_mask(COHERENT)
    assert C.moments(m, 3, 3) == (4, -4, -8, 10, 22, 11) and C.derived(C.moments(m, 3, 3)) == (24, 12, 24, 0, 24)
    assert _code_at(m, 3, 3) == 1 << 2
    m = _window_mask(INCOHERENT)
    assert C.moments(m, 3, 3) == (5, -5, -11, 11, 31, 14) and C.derived(C.moments(m, 3, 3)) == (30, 15, 34, -4, 30)
    assert _code_at(m, 3, 3) == 0xFF


# ------------------------------------------------------------------------------------------------ partners and the tally
def test_partners():
    off = np.array([0, 0, 1, 3, 3, 7, 8], np.int32)   # sizes 0, 1, 2, 0, 4, 1
    assert OR.sample_partners(off).tolist() == [0, 2, 1, 4, 5, 6, 5, 7]
    assert OR.sample_partners(off).dtype == np.int32
    assert OR.sample_partners(np.array([0], np.int32)).tolist() == [] and OR.sample_partners([0, 0]).tolist() == []
    assert OR.sample_partners(torch.tensor([0, 3])).tolist() == [1, 2, 1]
    with pytest.raises(ValueError, match="non-decreasing"):
        OR.sample_partners(np.array([0, 3, 2]))
    with pytest.raises(ValueError, match="non-decreasing"):
        OR.sample_partners(np.array([1, 3]))
    for P in TC.POINT_COUNTS:
        partner, off = C.random_partners(P)
        assert len(partner) == P == off[-1]
        i = np.arange(P)
        edge = np.repeat(np.arange(len(off) - 1), np.diff(off))
        assert (edge[partner] == edge).all() and (np.abs(partner - i) <= 1).all()
        assert ((partner == i) == (np.diff(off)[edge] == 1)).all()


def _tally_case(P, width, V, seed=0):
    K, M = SC.support_cameras(V, width)
    partner = C.random_partners(P, seed)[0]
    if P >= 8:   # partners outside [0, P) mean "none" and are never read
        partner[3], partner[5] = -1, P
    return TC.tally_points(P, width, seed), partner, K, M, C.random_near(V, SC.SUPPORT_H, width, seed)


@pytest.mark.parametrize("P", TC.POINT_COUNTS)
def test_the_tally_against_the_brute_force(P):
    k = TC.POINT_COUNTS.index(P)
    V = [1, 3, 12][k % 3] if P < 4096 else 3
    pts, partner, K, M, near = _tally_case(P, SC.WIDTHS[1 + k % 2], V, seed=k)
    for spread in ([k % 5] if P > 65 else range(5)):
        got = OR.oriented_tally(pts, partner, K, M, near, spread, backend="host")
        assert got.dtype == torch.int32 and tuple(got.shape) == (P, 2)
        want = C.oriented_tally_brute(pts, partner, K, M, near, spread)
        assert np.array_equal(got.numpy(), want), spread
        if P >= 63 and spread <= 1:   # (a random byte misses seven accepted bits once in 128)
            assert 0 < want[:, 1].sum() < want[:, 0].sum() < V * P, "seen and unseen, agreeing and not"


def test_the_tally_adds_and_does_not_depend_on_the_chunks():
    pts, partner, K, M, near = _tally_case(257, 33, 12)
    whole = OR.oriented_tally(pts, partner, K, M, near, backend="host")
    for cuts in ([0, 5, 12], [0, 1, 2, 9, 12]):
        out = torch.zeros((257, 2), dtype=torch.int32)
        for a, b in zip(cuts[:-1], cuts[1:]):
            assert OR.oriented_tally(pts, partner, K[a:b], M[a:b], near[a:b], backend="host", out=out) is out
        assert torch.equal(out, whole) and whole.any()
    seven = torch.full((257, 2), 7, dtype=torch.int32)
    OR.oriented_tally(pts, partner, K, M, near, backend="host", out=seven)
    assert torch.equal(seven, whole + 7)
    assert not OR.oriented_tally(pts, partner, K[:0], M[:0], near[:0], backend="host").any()
    assert tuple(OR.oriented_tally(pts[:0], partner[:0], K, M, near, backend="host").shape) == (0, 2)


def test_spread_four_and_all_ones_are_the_plain_tally():
    """With every bit accepted, or every bit offered wherever the distance is within the tolerance, the oriented tally is
    cgs_sample_support's."""
    V, W = 5, 33
    K, M = SC.support_cameras(V, W)
    d2 = SC.support_d2(V, W)
    pts = TC.tally_points(257, W)
    partner = C.random_partners(257)[0]
    for tol2 in (0, 4, 16):
        plain = ET.sample_tally(pts, K, M, d2, [C.TOL_PX[tol2]], backend="host")
        near = (0xFF * (d2 <= tol2)).astype(np.uint8)
        for spread in (0, 1, 4):
            assert torch.equal(OR.oriented_tally(pts, partner, K, M, near, spread, backend="host"), plain)
        bits = (C.random_near(V, SC.SUPPORT_H, W) | 1) * (d2 <= tol2).astype(np.uint8)
        assert torch.equal(OR.oriented_tally(pts, partner, K, M, bits, 4, backend="host"), plain)


def hand_tally_checks(backend, to):
    """The hand cases of the tally on one back end; ``to`` moves a near plane to where the back end wants it."""
    pts, partner, K, M, octants = C.hand_tally_case()
    V, n = len(K), C.HAND_SIZE
    dirs = C.hand_directions()
    for (dx, dy, o) in dirs:   # the expected octants are the definition's, and the step is what the camera was built for
        assert C.octant(dx * dx - dy * dy, 2.0 * (dx * dy)) == o, (dx, dy)
    tx, ty = C.TIE
    assert tx * tx - ty * ty == 2.0 * (tx * ty), "the tie is exact"
    assert sorted(set(octants.tolist())) == list(range(8))
    plane = lambda byte: np.broadcast_to(np.asarray(byte, np.uint8).reshape(-1, 1, 1), (V, n, n)).copy()
    own = plane(1 << octants)
    tally = lambda near, spread, p=partner: OR.oriented_tally(pts, p, K, M, to(near), spread, backend=backend).cpu().tolist()
    assert tally(own, 0) == [[V, V], [V, V]], "both points see the other in the octant of the step between them"
    assert tally(~own, 0) == [[V, 0], [V, 0]], "and in no other"
    for spread in range(1, 5):
        for shift in range(8):
            hit = V if min(shift, 8 - shift) <= spread else 0
            assert tally(plane(1 << ((octants + shift) % 8)), spread) == [[V, hit], [V, hit]], (spread, shift)
    # no partner, a partner out of range, a partner at the same pixel position and one that is not seen accept everything
    for p in ([0, 1], [-1, 2], [2, -5]):
        assert tally(~own, 0, np.array(p, np.int32)) == [[V, V], [V, V]], p
    three = np.concatenate([pts, pts[:1], [[0, 0, -1]], [[9, 9, 1]]]).astype(np.float32)   # a twin, one behind, one outside
    for j in (2, 3, 4):
        got = OR.oriented_tally(three, np.array([j, 0, 2, 3, 4], np.int32), K, M, to(~own), 0, backend=backend).cpu().numpy()
        assert got[0].tolist() == [V, V] and got[1].tolist() == [V, 0], j
    # the camera of the issue: u = X and v = Y exactly; steps along the axes and the diagonals
    K1, M1 = np.array([[1.0, 1.0, 0.0, 0.0]]), np.eye(4)[None, :3, :4]
    for (dx, dy), o in (((1, 0), 0), ((1, 1), 2), ((0, 1), 4), ((-1, 1), 6), ((-2, 0), 0), ((3, -3), 6)):
        two = np.array([[4, 4, 1], [4 + dx, 4 + dy, 1]], np.float32)
        for byte, hit in ((1 << o, 1), (0xFF ^ (1 << o), 0)):
            near = np.full((1, n, n), byte, np.uint8)
            got = OR.oriented_tally(two, np.array([1, 0], np.int32), K1, M1, to(near), 0, backend=backend).cpu().tolist()
            assert got == [[1, hit], [1, hit]], (dx, dy, byte)


def test_directions_on_the_octant_boundaries_and_one_step_beside_them():
    pts, partner, K, M, octants = C.hand_tally_case()
    for spread in (0, 1):
        near = C.random_near(len(K), C.HAND_SIZE, C.HAND_SIZE)
        assert np.array_equal(OR.oriented_tally(pts, partner, K, M, near, spread, backend="host").numpy(),
                              C.oriented_tally_brute(pts, partner, K, M, near, spread))
    hand_tally_checks("host", lambda near: near)


def test_argument_errors():
    pts, partner, K, M, near = _tally_case(65, 33, 2)
    tally = lambda **kw: OR.oriented_tally(**{**dict(points=pts, partner=partner, intrinsics=K, w2c=M, near=near,
                                                     backend="host"), **kw})
    with pytest.raises(ValueError, match="unknown edge orientation backend"):
        tally(backend="cuda")
    with pytest.raises(ValueError, match="spread"):
        tally(spread=5)
    with pytest.raises(ValueError, match="spread"):
        tally(spread=-1)
    with pytest.raises(ValueError, match="spread"):
        tally(spread=1.5)
    with pytest.raises(ValueError, match="float32"):
        tally(points=pts.astype(np.float64))
    with pytest.raises(ValueError, match="partner must be int32"):
        tally(partner=partner.astype(np.int64))
    with pytest.raises(ValueError, match=r"partner must be \[P\]"):
        tally(partner=partner[:-1])
    with pytest.raises(ValueError, match="near must be uint8"):
        tally(near=near.astype(np.int32))
    with pytest.raises(ValueError, match=r"near must be \[V,H,W\]"):
        tally(near=near[:1])
    with pytest.raises(ValueError, match="out must be"):
        tally(out=torch.zeros((65, 3), dtype=torch.int32))
    with pytest.raises(ValueError, match="at most 4 pixels"):
        OR.oriented_near(near, 4.2, backend="host")
    with pytest.raises(ValueError, match="uint8"):
        OR.oriented_near(near.astype(bool), 1, backend="host")
    with pytest.raises(ValueError, match="stack of masks"):
        OR.mask_orientation(near[0], backend="host")
    with pytest.raises(ValueError, match="unknown edge orientation backend"):
        OR.mask_orientation(near, backend="cpu")
    assert tuple(OR.mask_orientation(near[:0], backend="host").shape) == (0, SC.SUPPORT_H, 33)


# ------------------------------------------------------------------------------------------------ the drawn scans
# (pieces, kept samples) on the 72 bogus chords at (tolerance, max_gap, min_span): un-oriented, oriented.  Measured on the
# host back end; the prototype's figures of the issue are the same.
BOGUS = {(1, 3, 10): ((40, 954), (28, 679)), (2, 3, 10): ((99, 2043), (39, 961)), (1, 0, 2): ((149, 1555), (57, 773))}


@pytest.mark.parametrize("setting", sorted(BOGUS), ids=lambda s: "tol%d-gap%d-span%d" % s)
def test_the_bogus_chords_lose_pieces_and_samples_and_the_drawn_edges_stay_whole(setting):
    tol, gap, span = setting
    plain = TC.scan_trim("bogus", "host", tol, None, gap, span)
    same = C.scan_trim("bogus", "host", tol, gap, span, oriented=False)
    assert torch.equal(same["tally"], plain["tally"]) and same["spans"] == plain["spans"]
    assert same["edge_dict"] == plain["edge_dict"] and same["settings"] == plain["settings"], "oriented=False changes nothing"
    got = C.scan_trim("bogus", "host", tol, gap, span)
    p0, k0, whole0 = C.bogus_counts(plain)
    p1, k1, whole1 = C.bogus_counts(got)
    print(f"tolerance {tol} px, max_gap {gap}, min_span {span}: {p0} pieces / {k0} samples on the bogus chords without "
          f"orientation, {p1} / {k1} with")
    assert whole0 and whole1, "the four drawn edges come back whole"
    assert p1 < p0 and k1 < k0
    assert ((p0, k0), (p1, k1)) == BOGUS[setting]
    assert torch.equal(got["tally"][:, 0], plain["tally"][:, 0]) and (got["tally"][:, 1] <= plain["tally"][:, 1]).all()
    assert got["settings"] == {**plain["settings"], "oriented": True, "spread": 1}
    assert sum(len(s) for s in got["spans"]) == p1 + 4 == {(1, 3, 10): 32, (2, 3, 10): 43, (1, 0, 2): 61}[setting]


def test_the_drawn_edges_are_kept_whole_and_the_extended_ones_are_cut_no_later():
    for tol in (1, 2):
        for gap, span in ((3, 10), (0, 2)):
            r = C.scan_trim("drawn", "host", tol, gap, span)
            n = np.diff(r["offsets"].astype(np.int64))
            assert r["spans"] == [[(0, int(k) - 1)] for k in n], (tol, gap, span)
        plain, got = TC.scan_trim("extended", "host", tol), C.scan_trim("extended", "host", tol, 0, 2)
        assert [len(s) for s in got["spans"]] == [1, 1, 1, 1]
        e0, e1 = TC.cut_errors(plain), TC.cut_errors(got)
        print(f"tolerance {tol} px: cut errors {e0} without orientation, {e1} with")
        assert (e1 <= TC.CUT_CAP[tol]).all() and (e1 <= e0).all() and (e1 > 0).all()
        want = {1: [(72, 323), (0, 156), (63, 237), (0, 183)], 2: [(69, 323), (0, 159), (60, 237), (0, 185)]}[tol]
        assert [s[0] for s in got["spans"]] == want


def test_chunking_the_views_changes_nothing_and_the_walk_has_no_distance_transform(monkeypatch):
    whole = C.scan_trim("bogus", "host", 1)
    five = C.scan_trim("bogus", "host", 1, budget_bytes=5 * OR.BYTES_PER_PIXEL * DC.DIR_H * DC.DIR_W)   # 5 + 5 + 2 views
    one = C.scan_trim("bogus", "host", 1, budget_bytes=1)
    for part in (five, one):
        assert torch.equal(part["tally"], whole["tally"]) and part["spans"] == whole["spans"]
    assert OR.BYTES_PER_PIXEL == 3
    chunks = []
    real = ET.view_chunks
    monkeypatch.setattr(ET, "view_chunks", lambda cams, bpp, budget: chunks.append(bpp) or real(cams, bpp, budget))
    monkeypatch.setattr(ES, "edt_squared", lambda *a, **k: pytest.fail("the oriented walk needs no distance transform"))
    cams, maps = DC.dir_novel_cameras()
    args = (TC.extended_edges()[0], cams, maps, "PidiNet")
    ET.trim_edges(*args, resolution=C.EC.SCAN_RESOLUTION, backend="host", oriented=True)
    assert chunks == [3]
    with pytest.raises(ValueError, match="spread"):
        ET.trim_edges(*args, backend="host", oriented=True, spread=5)
    with pytest.raises(ValueError, match="at most 4 pixels"):
        ET.trim_edges(*args, backend="host", oriented=True, tolerance_px=5)


def stub_angles(result):
    """Degrees, one per piece on a bogus chord: the angle at which it leaves the nearest drawn edge, from its middle sample."""
    from curve_gaussian_amd.ops import edge_support as SP
    import edge_score_cases as EC
    edge_dict = SC.scan_edges()[0]
    pts, off = SP.sample_edges(edge_dict["curves_ctl_pts"], edge_dict["lines_end_pts"], EC.SCAN_RESOLUTION)
    s, t = DC.dir_samples()
    out = []
    for e, spans in enumerate(result["spans"]):
        if e in C.DRAWN_EDGES:
            continue
        for a, b in spans:
            p = pts[off[e] + a:off[e] + b + 1].astype(np.float64)
            mid = p[len(p) // 2]
            k = int(np.argmin(((s - mid) ** 2).sum(1)))
            out.append(float(DC.angle_deg(p[-1] - p[0], t[k])[0]))
    return np.array(out)


def test_recorded_the_fallback_on_thick_strokes_and_the_angles_of_the_stubs():
    """Recorded, not asserted beyond what the rule guarantees: on strokes dilated to 5 px every pixel is isotropic in its
    window, so orientation can only refuse less than on the thin strokes; thinning brings the test back."""
    for tol in (1,):
        plain = C.scan_trim("bogus", "host", tol, oriented=False, dilate=5)
        thick = C.scan_trim("bogus", "host", tol, dilate=5)
        thinned = C.scan_trim("bogus", "host", tol, dilate=5, thin=True)
        thinned_plain = C.scan_trim("bogus", "host", tol, oriented=False, dilate=5, thin=True)
        for name, r in (("5 px, plain", plain), ("5 px, oriented", thick), ("5 px thinned, plain", thinned_plain),
                        ("5 px thinned, oriented", thinned)):
            print(f"{name}: pieces, samples, drawn edges whole = {C.bogus_counts(r)}")
        assert (thick["tally"][:, 1] <= plain["tally"][:, 1]).all() and (thinned["tally"][:, 1] <= thinned_plain["tally"][:, 1]).all()
        assert thinned["settings"]["thin"] is True and thinned["settings"]["oriented"] is True
    for name, r in (("plain", TC.scan_trim("bogus", "host", 1, None, 3, 10)), ("oriented", C.scan_trim("bogus", "host", 1))):
        ang = stub_angles(r)
        print(f"{name}: {len(ang)} stubs leave the drawn edges at {ang.min():.1f} to {ang.max():.1f} degrees, median "
              f"{np.median(ang):.1f}; {(ang > 45).sum()} beyond 45")


# ------------------------------------------------------------------------------------------------ files and options
def test_the_command_line_with_and_without_the_flag(tmp_path, capsys):
    from curve_gaussian_amd.edge_extraction import support as S
    base, data = SC.write_support_scan(tmp_path)
    room = os.path.join(base, "room")
    argv = ["--base_dir", base, "--dataset_dir", data, "--detector", "PidiNet", "--backend", "host", "--frames_ratio", "0.5",
            "--sample_resolution", str(C.EC.SCAN_RESOLUTION), "--trim", "--trim_tolerance", "1"]
    read = lambda: {name: open(os.path.join(room, name), "rb").read() for name in sorted(os.listdir(room))}
    assert S.main(argv) == 0
    first = read()
    assert S.main(argv) == 0
    assert read() == first, "two runs without the flag write the same bytes"
    assert "oriented" not in json.loads(first[S.TRIM_FILE])["settings"]
    assert S.main(argv + ["--oriented"]) == 0
    flagged = read()
    assert sorted(flagged) == sorted(first) == sorted([S.SUPPORT_FILE, S.TRIM_FILE, "parametric_edges.json", S.TRIMMED_FILE])
    for name in first:
        assert (flagged[name] != first[name]) == (name in (S.TRIM_FILE, S.TRIMMED_FILE)), name
    out = json.loads(flagged[S.TRIM_FILE])
    want = C.scan_trim("bogus", "host", 1)
    assert out["settings"] == {**want["settings"], "layout": "emap", "undistort": False}
    assert out["settings"]["oriented"] is True and out["settings"]["spread"] == 1
    assert out["pieces"] == 32 and json.loads(flagged[S.TRIMMED_FILE]) == want["edge_dict"]
    assert "trimmed to 32 pieces" in capsys.readouterr().out
    assert S.main(argv + ["--oriented", "--orient_spread", "0"]) == 0
    assert json.loads(read()[S.TRIM_FILE])["settings"]["spread"] == 0
    with pytest.raises(SystemExit):
        S.main([a for a in argv if a != "--trim"] + ["--oriented"])
    assert "--oriented needs --trim" in capsys.readouterr().err


def test_dedupe_and_join_take_the_oriented_pieces(tmp_path):
    from curve_gaussian_amd.edge_extraction import support as S
    base, data = SC.write_support_scan(tmp_path)
    room = os.path.join(base, "room")
    argv = ["--base_dir", base, "--dataset_dir", data, "--detector", "PidiNet", "--backend", "host", "--frames_ratio", "0.5",
            "--sample_resolution", str(C.EC.SCAN_RESOLUTION), "--trim", "--oriented", "--dedupe", "--join"]
    assert S.main(argv) == 0
    dedupe = json.load(open(os.path.join(room, S.DEDUPE_FILE)))
    assert dedupe["input"] == S.TRIMMED_FILE and dedupe["total"] == 32
    assert json.load(open(os.path.join(room, S.GRAPH_FILE)))["input"] == S.DEDUPED_FILE


def test_the_driver_parses_the_options():
    import inspect

    from curve_gaussian_amd import train as T
    _, _, args = T.parse_args(["-s", "scan", "-m", "out", "--trim_edges", "--trim_oriented", "--trim_orient_spread", "2"])
    assert T.trim_options(args) == {"oriented": True, "spread": 2}
    assert set(T.trim_options(args)) <= set(inspect.signature(ET.trim_edges).parameters)
    _, _, args = T.parse_args(["-s", "scan", "-m", "out", "--trim_edges", "--trim_oriented", "--thin_edge_maps"])
    assert T.trim_options(args) == {"thin": True, "oriented": True}
    _, _, args = T.parse_args(["-s", "scan", "-m", "out", "--trim_edges", "--trim_orient_spread", "2"])
    assert T.trim_options(args) == {}, "the spread alone switches nothing on"


def test_the_export_passes_the_option_through(tmp_path, capsys):
    from curve_gaussian_amd.edge_extraction import support as S
    cams, maps = DC.dir_novel_cameras()
    options = dict(resolution=C.EC.SCAN_RESOLUTION, frames_ratio=0.5, backend="host", oriented=True)
    trimmed, res = S.trim_scene(str(tmp_path), SC.scan_edges()[0], cams, maps, "PidiNet", **options)
    assert "after trimming:  32 pieces" in capsys.readouterr().out
    assert res["settings"]["oriented"] is True and trimmed == C.scan_trim("bogus", "host", 1)["edge_dict"]


# ------------------------------------------------------------------------------------------------ the C ABI
def test_abi_argument_checks_are_pinned():
    """Status and the exact text of cgs_last_error() for every rejection of the three entries; the pointers are dummies that
    are never dereferenced, and no row passes validation with work to do."""
    from curve_gaussian_amd import _lib
    lib = _lib.load()
    p, q = ctypes.c_void_p(1 << 20), ctypes.c_void_p(1 << 30)

    def planes(fn, with_tol):
        def call(V=2, H=4, W=6, src=p, dst=q, tol2=1):
            args = (V, H, W, src) + ((tol2,) if with_tol else ()) + (dst, None)
            return getattr(lib, fn)(*args)
        return call

    for fn, with_tol in (("cgs_mask_orientation", False), ("cgs_oriented_near", True)):
        call, head = planes(fn, with_tol), fn + ": invalid argument "
        rows = [(dict(V=-1), "(V=-1, height=4, width=6; sizes lie in [1, 16384])"),
                (dict(H=0), "(V=2, height=0, width=6; sizes lie in [1, 16384])"),
                (dict(H=16385), "(V=2, height=16385, width=6; sizes lie in [1, 16384])"),
                (dict(W=0), "(V=2, height=4, width=0; sizes lie in [1, 16384])"),
                (dict(V=0, W=-3), "(V=0, height=4, width=-3; sizes lie in [1, 16384])"),
                (dict(W=16385, src=None), "(V=2, height=4, width=16385; sizes lie in [1, 16384])"),
                (dict(src=None), "(NULL pointer)"), (dict(dst=None), "(NULL pointer)"), (dict(V=0, dst=None), "(NULL pointer)")]
        if with_tol:
            rows += [(dict(tol2=-1), "(tol2=-1; tol2 lies in [0, 16])"), (dict(tol2=17), "(tol2=17; tol2 lies in [0, 16])"),
                     (dict(V=0, tol2=17, src=None), "(tol2=17; tol2 lies in [0, 16])"),
                     (dict(dst=p), "(code and near overlap)"),
                     (dict(dst=ctypes.c_void_p((1 << 20) + 47)), "(code and near overlap)"),
                     (dict(dst=ctypes.c_void_p((1 << 20) - 47)), "(code and near overlap)")]
        for kw, text in rows:
            assert call(**kw) == -1 and lib.cgs_last_error().decode() == head + text, (fn, kw)
        assert call(V=0) == 0, "no view leaves nothing to write"
        if with_tol:
            assert call(V=0, dst=p) == 0, "nothing of nothing overlaps"

    head = "cgs_sample_support_oriented: invalid argument "

    def call(P=5, points=p, partner=p, V=2, intr=p, w2c=p, H=4, W=6, near=p, spread=1, tally=p):
        return lib.cgs_sample_support_oriented(P, points, partner, V, intr, w2c, H, W, near, spread, tally, None)

    rows = [(dict(P=-1), "(P=-1, V=2, spread=1; the spread lies in [0, 4])"),
            (dict(V=-1), "(P=5, V=-1, spread=1; the spread lies in [0, 4])"),
            (dict(spread=-1), "(P=5, V=2, spread=-1; the spread lies in [0, 4])"),
            (dict(spread=5, H=0), "(P=5, V=2, spread=5; the spread lies in [0, 4])"),
            (dict(P=0, spread=5), "(P=0, V=2, spread=5; the spread lies in [0, 4])"),
            (dict(H=0), "(height=0, width=6; sizes lie in [1, 16384])"),
            (dict(H=16385), "(height=16385, width=6; sizes lie in [1, 16384])"),
            (dict(W=0, points=None), "(height=4, width=0; sizes lie in [1, 16384])"),
            (dict(V=0, W=16385), "(height=4, width=16385; sizes lie in [1, 16384])")]
    rows += [({name: None}, "(NULL pointer; P=5, V=2)") for name in ("points", "partner", "intr", "w2c", "near", "tally")]
    rows += [(dict(P=0, intr=None), "(NULL pointer; P=0, V=2)"), (dict(V=0, near=None), "(NULL pointer; P=5, V=0)"),
             (dict(V=0, partner=None), "(NULL pointer; P=5, V=0)")]
    for kw, text in rows:
        assert call(**kw) == -1 and lib.cgs_last_error().decode() == head + text, kw
    for kw in (dict(P=0), dict(V=0), dict(P=0, points=None, partner=None, tally=None),
               dict(P=0, V=0, points=None, partner=None, tally=None)):
        assert call(**kw) == 0, "no sample or no view leaves nothing to add"
    i, vp = ctypes.c_int, ctypes.c_void_p
    assert _lib.SIGNATURES["cgs_mask_orientation"] == (i, [i, i, i, vp, vp, vp])
    assert _lib.SIGNATURES["cgs_oriented_near"] == (i, [i, i, i, vp, i, vp, vp])
    assert _lib.SIGNATURES["cgs_sample_support_oriented"] == (i, [i, vp, vp, i, vp, vp, i, i, vp, i, vp, vp])


def test_the_constants_mirror_the_header():
    from curve_gaussian_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "curvegs.h")).read()
    for name, value in (("CGS_ORIENT_RADIUS", OR.RADIUS), ("CGS_ORIENT_MAX_TOL2", OR.MAX_TOL2),
                        ("CGS_ORIENT_MAX_SPREAD", OR.MAX_SPREAD), ("CGS_ORIENT_TILE_WIDTH", OR.TILE_WIDTH),
                        ("CGS_ORIENT_TILE_HEIGHT", OR.TILE_HEIGHT)):
        assert f"#define {name} {value}\n" in header, name
    assert (OR.RADIUS, OR.MAX_TOL2, OR.MAX_SPREAD) == (3, 16, 4) == (C.R, max(C.TOL2S), 4)
    assert OR.MAX_TOL2 == _lib.EDGE_SUPPORT_MAX_TOL ** 2
    assert (OR.TILE_HEIGHT, OR.TILE_WIDTH) == (_lib.ORIENT_TILE_HEIGHT, _lib.ORIENT_TILE_WIDTH) == (32, 64)
