"""GPU: the plane-sweep kernels (cgs_stereo_sweep / cgs_stereo_consistency, csrc/stereo_depth.hip) against the host back end
of ops.stereo_depth bit for bit -- every case of the CPU tests, a spread of shapes, mixed sizes through the Python layer --
the raw entries' argument checks, and the box arc end to end."""
import ctypes

import numpy as np
import pytest
import torch

import stereo_cases as SC
from curve_gaussian_amd import _lib
from curve_gaussian_amd.ops import edge_occlusion as EO
from curve_gaussian_amd.ops import stereo_depth as SD
from curve_gaussian_amd.scene import solid_scan as SS

pytestmark = pytest.mark.gpu


def both_sweeps(case):
    return (SD.sweep(*SC.sweep_args(case), backend="gpu").cpu().numpy(), SD.sweep(*SC.sweep_args(case), backend="host").numpy())


def both_consistencies(c, mc):
    args = (c["depth"], c["K"], c["src"], c["rel"], c["tol"], mc)
    return SD.consistency(*args, backend="gpu").cpu().numpy(), SD.consistency(*args, backend="host").numpy()


@pytest.mark.parametrize("H,W,R", [(1, 1, 0), (1, 1, 1), (5, 7, 0), (5, 7, 1), (9, 11, 0), (9, 11, 1)])
def test_sweep_equals_host_on_the_cpu_matrix(H, W, R):
    got, want = both_sweeps(SC.random_case(3, H, W, 4, 3, R, 7 * H + R))
    assert SC.same_bits(got, want)


NAMED = SC.named_cases()


@pytest.mark.parametrize("name", sorted(NAMED))
def test_sweep_equals_host_on_the_named_cases(name):
    case, check = NAMED[name]
    got, want = both_sweeps(case)
    assert SC.same_bits(got, want)
    check(got)


# D: 1, 2, 3, 33; R: 0, 1, 3; S: 1, 3 (with -1 pads when S = 3); sizes 1x1, 5x7, 24x32, 33x65 (no multiple of the 16 x 16
# tile); V: 1 and 5.  Every value appears, the largest of each together once.
SHAPES = [(5, 33, 65, 33, 3, 3), (5, 24, 32, 3, 3, 1), (5, 33, 65, 2, 1, 1), (5, 24, 32, 1, 3, 3), (1, 24, 32, 33, 1, 1),
          (1, 33, 65, 3, 3, 0), (5, 5, 7, 33, 3, 1), (5, 5, 7, 2, 1, 0), (5, 1, 1, 3, 3, 0), (1, 1, 1, 1, 1, 1),
          (5, 33, 65, 1, 1, 3), (1, 5, 7, 2, 3, 3), (5, 24, 32, 33, 1, 0), (5, 17, 16, 3, 1, 1)]


@pytest.mark.parametrize("V,H,W,D,S,R", SHAPES)
def test_sweep_equals_host_across_shapes(V, H, W, D, S, R):
    case = SC.random_case(V, H, W, D, S, R, 3 * H + D + S)
    got, want = both_sweeps(case)
    assert SC.same_bits(got, want)
    if V > 1 and R > 0 and H > 2 * R + 2 and D > 1:
        assert (got > 0).any()


@pytest.mark.parametrize("V,H,W,S,mc", [(3, 5, 7, 3, 1), (3, 9, 11, 3, 2), (1, 1, 1, 1, 1), (4, 6, 5, 2, 0), (5, 33, 65, 3, 2),
                                        (5, 24, 32, 1, 1)])
def test_consistency_equals_host(V, H, W, S, mc):
    got, want = both_consistencies(SC.random_consistency_case(V, H, W, S, 40 + V + H), mc)
    assert SC.same_bits(got, want)


def test_consistency_named_cases():
    c = SC.consistency_case()
    odd = dict(c, depth=c["depth"].copy())
    odd["depth"][1, 3, 4] = np.float32(2.0000002)
    zero = dict(c, depth=c["depth"].copy(), tol=np.full((3,), np.inf))
    zero["depth"][2] = 0.0
    for case, mc in ((c, 2), (odd, 2), (zero, 2), (zero, 1), (SC.consistency_case(zs=(2.0, 3.0, 4.0)), 1)):
        got, want = both_consistencies(case, mc)
        assert SC.same_bits(got, want)


def test_a_source_index_beyond_the_views_is_no_source():
    case = SC.random_case(3, 9, 11, 4, 3, 1, 50)
    wild = dict(case, src=np.where(case["src"] < 0, 7, case["src"]).astype(np.int32))
    assert SC.same_bits(both_sweeps(wild)[0], both_sweeps(case)[0])


def test_mixed_sizes_through_the_python_layer():
    small = SS.solid_scan("box", 3, 24, 32, synth_cameras=SS.arc_cameras(3, 24, 32))
    large = SS.solid_scan("box", 2, 33, 65, synth_cameras=SS.arc_cameras(2, 33, 65))
    cams = [small.cameras[0], large.cameras[0], small.cameras[1], large.cameras[1], small.cameras[2]]
    ps, pl = SS.photographs(small), SS.photographs(large)
    photos = [ps[0], pl[0], ps[1], pl[1], ps[2]]
    kw = dict(hypotheses=12, patch_radius=1, sources=2, min_consistent=1)
    gpu, host = SD.stereo_depth(photos, cams, backend="gpu", **kw), SD.stereo_depth(photos, cams, backend="host", **kw)
    assert all(SC.same_bits(a, b) for a, b in zip(gpu, host)) and any((m > 0).any() for m in gpu)


# ------------------------------------------------------------------------------------------------ the raw entries
def _device_case():
    case = SC.random_case(3, 9, 11, 4, 3, 1, 60)
    dev = torch.device("cuda", torch.cuda.current_device())
    t = {k: torch.from_numpy(np.ascontiguousarray(case[k])).to(dev) for k in ("gray", "K", "inv", "src", "rel")}
    return case, dev, t


def test_raw_sweep_entry():
    lib = _lib.load()
    case, dev, t = _device_case()
    out = torch.full((3, 9, 11), -7.0, dtype=torch.float32, device=dev)
    p, s = _lib.ptr, _lib.raw_stream(dev)
    good = [3, 9, 11, p(t["gray"]), p(t["K"]), 4, p(t["inv"]), 3, p(t["src"]), p(t["rel"]), 1, 1.0, 1.5, 1, p(out), s]
    for pos, bad in ((0, -1), (1, 0), (2, _lib.EDT_MAX_SIZE + 1), (3, None), (4, None), (5, 0), (6, None), (7, 0), (8, None),
                     (9, None), (10, -1), (10, _lib.STEREO_MAX_RADIUS + 1), (11, -1.0), (12, float("nan")), (13, 0), (14, None)):
        args = list(good)
        args[pos] = bad
        assert lib.cgs_stereo_sweep(*args) == -1, (pos, bad)
        torch.cuda.synchronize()
        assert bool((out == -7.0).all()), (pos, bad)           # a rejected call leaves the output untouched
    args = list(good)
    args[0] = 0
    assert lib.cgs_stereo_sweep(*args) == 0                     # V = 0 is allowed: nothing is written
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())
    assert lib.cgs_stereo_sweep(*good) == 0
    torch.cuda.synchronize()
    assert SC.same_bits(out.cpu().numpy(), SD.sweep(*SC.sweep_args(case), backend="host").numpy())


def test_raw_consistency_entry():
    lib = _lib.load()
    c = SC.random_consistency_case(3, 9, 11, 3, 61)
    dev = torch.device("cuda", torch.cuda.current_device())
    t = {k: torch.from_numpy(np.ascontiguousarray(c[k])).to(dev) for k in ("depth", "K", "src", "rel", "tol")}
    out = torch.full((3, 9, 11), -7.0, dtype=torch.float32, device=dev)
    p, s = _lib.ptr, _lib.raw_stream(dev)
    good = [3, 9, 11, p(t["depth"]), p(t["K"]), 3, p(t["src"]), p(t["rel"]), p(t["tol"]), 2, p(out), s]
    before = t["depth"].clone()
    inside = ctypes.c_void_p(t["depth"].data_ptr() + 4 * 50)    # out overlapping depth
    for pos, bad in ((0, -1), (1, 0), (2, 0), (3, None), (4, None), (5, 0), (6, None), (7, None), (8, None), (9, -1),
                     (10, None), (10, inside), (10, p(t["depth"]))):
        args = list(good)
        args[pos] = bad
        assert lib.cgs_stereo_consistency(*args) == -1, (pos, bad)
        torch.cuda.synchronize()
        assert bool((out == -7.0).all()) and torch.equal(t["depth"].view(torch.int32), before.view(torch.int32)), (pos, bad)
    args = list(good)
    args[0] = 0
    assert lib.cgs_stereo_consistency(*args) == 0
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())
    assert lib.cgs_stereo_consistency(*good) == 0
    torch.cuda.synchronize()
    want = SD.consistency(c["depth"], c["K"], c["src"], c["rel"], c["tol"], 2, backend="host").numpy()
    assert SC.same_bits(out.cpu().numpy(), want)


# ------------------------------------------------------------------------------------------------ end to end
def test_box_arc_end_to_end():
    from curve_gaussian_amd.edge_extraction.reprojection import score_edges
    scan = SS.solid_scan("box", 8, 48, 64, backend="host", synth_cameras=SS.arc_cameras(8, 48, 64))
    photos = list(SS.photographs(scan))
    kw = dict(hypotheses=32, patch_radius=2, sources=2, return_info=True)
    (gpu, info), (host, info_h) = SD.stereo_depth(photos, scan.cameras, backend="gpu", **kw), \
        SD.stereo_depth(photos, scan.cameras, backend="host", **kw)
    assert all(SC.same_bits(a, b) for a, b in zip(gpu, host)) and info == info_h and min(info["coverage"]) > 0
    rows = []
    for backend, maps in (("gpu", gpu), ("host", host)):
        res = score_edges(scan.edges, scan.cameras, scan.maps, "PidiNet", backend=backend, depth_maps=maps,
                          depth_slack=info["recommended_slack"])
        rows.append([(r["kept_points"], r["hidden_points"], r["n_pred"], r["n_det"], r["pred_hits"], r["det_hits"])
                     for r in res["views"]])
        assert res["settings"]["depth_maps"] is True
    assert rows[0] == rows[1] and sum(r[1] for r in rows[0]) > 0
