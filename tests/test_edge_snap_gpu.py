"""GPU: cgs_sample_snap_terms (csrc/edge_snap.hip) against the brute-force definition and the host back end of ops.edge_snap,
bit for bit -- sample counts around a wave and a workgroup, view counts, planes without a footprint and with one, every
capture, the all-infinite plane, chunks of views, a pair handed in, guard elements around the raw call's rows, and the
drawn scan snapped end to end on both back ends."""
import numpy as np
import pytest
import torch

import edge_dir_cases as DC
import edge_score_cases as EC
import edge_snap_cases as C
from curve_gaussian_amd import _lib as L
from curve_gaussian_amd.ops import edge_snap as SN

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)   # a copy: the shared cases are read-only


@pytest.mark.parametrize("P", C.POINT_COUNTS)
def test_terms_equal_the_brute_force_bit_for_bit(P):
    for V in C.VIEW_COUNTS:
        for H, W in C.PLANES:
            for capture_px in C.CAPTURES:
                pts, K, M, d2, cap2, want = C.kernel_case(P, V, H, W, capture_px)
                terms, views = SN.snap_terms(pts.copy(), K, M, _dev(d2), capture_px)
                assert terms.is_cuda and views.is_cuda and tuple(terms.shape) == (P, 10) and tuple(views.shape) == (P,)
                assert C.same_bits((terms, views), want), (V, H, W, capture_px)
    pts, K, M, d2, cap2, want = C.kernel_case(P, 2, 37, 70, 8, "inf")   # past the table if the lookup came before the comparison
    got = SN.snap_terms(_dev(pts), K, M, _dev(d2), 8, device=DEV)
    assert C.same_bits(got, want) and not got[1].any() and not got[0].any()


@pytest.mark.parametrize("capture_px", C.CAPTURES)
def test_many_workgroups_equal_the_host(capture_px):
    for H, W in C.PLANES:
        for kind in ("random", "inf"):
            pts, K, M = C.snap_points(C.BIG_P, H, W), *C.snap_cameras(5, H, W)
            d2 = C.snap_d2(5, H, W, SN.capture_squared(capture_px), kind=kind)
            want = SN.snap_terms(pts, K, M, d2, capture_px, backend="host")
            assert C.same_bits(SN.snap_terms(pts, K, M, _dev(d2), capture_px), want), (H, W, kind)
            assert want[1].any() == (kind == "random" and H >= 2 and W >= 2)


def test_chunks_of_views_add_up_to_the_bits_of_one_call():
    pts, K, M, d2, cap2, want = C.kernel_case(257, 13, 37, 70, 3)
    d2_dev, P = _dev(d2), 257
    for cuts in ([0, 2, 5, 13], list(range(14))):   # the issue's [0:2], [2:5] and the rest; then one view per call
        out = (torch.zeros((P, 10), dtype=torch.float64, device=DEV), torch.zeros((P,), dtype=torch.int32, device=DEV))
        for a, b in zip(cuts[:-1], cuts[1:]):
            got = SN.snap_terms(pts.copy(), K[a:b], M[a:b], d2_dev[a:b], 3, out=out)
            assert got[0] is out[0] and got[1] is out[1]
        assert C.same_bits(out, want), cuts
    # a non-zero pair handed in is added to, exactly as the host back end adds to it
    rng = np.random.default_rng(5)
    start = (rng.normal(size=(P, 10)), rng.integers(0, 9, P).astype(np.int32))
    host = (torch.from_numpy(start[0].copy()), torch.from_numpy(start[1].copy()))
    SN.snap_terms(pts.copy(), K, M, d2.copy(), 3, backend="host", out=host)
    out = (_dev(start[0]), _dev(start[1]))
    SN.snap_terms(pts.copy(), K, M, d2_dev, 3, out=out)
    assert C.same_bits(out, host) and not C.same_bits(out, want)
    none = SN.snap_terms(pts.copy(), K[:0], M[:0], d2_dev[:0], 3)
    assert none[0].is_cuda and tuple(none[0].shape) == (P, 10) and not none[0].any() and not none[1].any()


def test_the_raw_call_touches_its_rows_and_nothing_else():
    P, V, H, W = 257, 5, 37, 70
    pts, K, M, d2, cap2, want = C.kernel_case(P, V, H, W, 3)
    guard, sentinel = 16, -12345
    terms = torch.full((guard + P * 10 + guard,), float(sentinel), dtype=torch.float64, device=DEV)
    views = torch.full((guard + P + guard,), sentinel, dtype=torch.int32, device=DEV)
    terms[guard:guard + P * 10] = 0.0
    views[guard:guard + P] = 0
    p, Kd, Md, dd, lut = _dev(pts), _dev(K), _dev(M.reshape(-1, 12)), _dev(d2), _dev(SN.distance_table(cap2))
    rc = L.load().cgs_sample_snap_terms(P, L.ptr(p), V, L.ptr(Kd), L.ptr(Md), H, W, L.ptr(dd), cap2, L.ptr(lut),
                                        terms.data_ptr() + 8 * guard, views.data_ptr() + 4 * guard, L.raw_stream(DEV))
    assert rc == 0
    torch.cuda.synchronize()
    assert C.same_bits((terms[guard:guard + P * 10].reshape(P, 10), views[guard:guard + P]), want)
    for t in (terms, views):
        assert (t[:guard] == sentinel).all() and (t[-guard:] == sentinel).all()


def test_the_drawn_scan_snaps_to_the_same_bits_on_both_back_ends():
    host = C.scan_snap("perturbed")
    gpu = C.scan_snap("perturbed", backend="gpu")
    assert gpu["edge_dict"] == host["edge_dict"] and gpu["edges"] == host["edges"] and host["moved"].all()
    assert {**gpu["settings"], "backend": "host"} == host["settings"]
    many = C.scan_snap("perturbed", backend="gpu", budget_bytes=1)   # one view per chunk, the transform recomputed per pass
    assert many["settings"]["chunks"] == 12 and many["edge_dict"] == host["edge_dict"] and many["edges"] == host["edges"]
    cams, maps = DC.dir_novel_cameras()
    shifted = SN.snap_edges(C.shifted_edge(), cams, maps, "PidiNet", resolution=EC.SCAN_RESOLUTION,
                            frames_ratio=C.SCAN_FRAMES_RATIO, backend="gpu")
    assert shifted["edge_dict"] == C.shifted_edge() and shifted["edges"] == C.scan_snap("shifted")["edges"]


def test_argument_errors():
    pts, K, M, d2, cap2, _ = C.kernel_case(65, 2, 37, 70, 3)
    with pytest.raises(L.CurveGSError, match="d2"):
        SN.snap_terms(pts.copy(), K, M, d2.copy(), 3)   # a host transform
    out = (torch.zeros((65, 10), dtype=torch.float64), torch.zeros((65,), dtype=torch.int32))
    with pytest.raises(L.CurveGSError, match="out is on"):
        SN.snap_terms(pts.copy(), K, M, _dev(d2), 3, out=out)
    with pytest.raises(ValueError, match="backend='host' takes host arrays"):
        SN.snap_terms(pts.copy(), K, M, _dev(d2), 3, backend="host")
    lib, p, s = L.load(), _dev(d2), L.raw_stream(DEV)
    assert lib.cgs_sample_snap_terms(1, L.ptr(p), 1, L.ptr(p), L.ptr(p), 37, 70, L.ptr(p), 65, L.ptr(p), L.ptr(p), L.ptr(p), s) == -1
    assert lib.cgs_last_error() == b"cgs_sample_snap_terms: invalid argument (P=1, V=1, cap2=65; cap2 lies in [1, 64])"
