"""GPU: the distance-field kernels (cgs_tsdf_integrate / cgs_tsdf_mesh_count / cgs_tsdf_mesh_emit, csrc/tsdf.hip) against
the host back end of ops.tsdf bit for bit -- every case of the CPU tests, larger lattices and images, mixed sizes and
chunks through the Python layer --, the raw entries' argument checks, and the box end to end."""
import ctypes

import numpy as np
import pytest
import torch

import tsdf_cases as TC
from curve_gaussian_amd import _lib
from curve_gaussian_amd.ops import mesh_contours as MC
from curve_gaussian_amd.ops import tsdf as TS
from curve_gaussian_amd.scene import solid_scan as SS

pytestmark = pytest.mark.gpu


def integrate(c, backend, state=None):
    s, w = TS.integrate(c["depth"], c["K"], c["M"], c["dims"], c["bounds"], c["trunc"], state=state, backend=backend)
    return s.cpu().numpy(), w.cpu().numpy()


def same_state(a, b):
    return bool((a[0].view(np.uint64) == b[0].view(np.uint64)).all() and (a[1] == b[1]).all())


def check_integrate(c):
    got, want = integrate(c, "gpu"), integrate(c, "host")
    assert got[0].shape == want[0].shape and same_state(got, want)
    return got


def extract(total, weight, dims, bounds, min_weight, backend):
    s, w = torch.from_numpy(np.ascontiguousarray(total, np.float64)), torch.from_numpy(np.ascontiguousarray(weight, np.uint16))
    tris, counts = TS.extract(s, w, dims, bounds, min_weight, backend=backend, return_counts=True)
    return counts.cpu().numpy(), tris.cpu().numpy()


def check_extract(total, weight, dims, bounds, min_weight):
    (counts, tris), (want_counts, want) = (extract(total, weight, dims, bounds, min_weight, b) for b in ("gpu", "host"))
    assert counts.shape == want_counts.shape and (counts == want_counts).all() and TC.same_bits(tris, want)
    return counts, tris


# ------------------------------------------------------------------------------------------------ integration
@pytest.mark.parametrize("H,W", [(1, 1), (5, 7), (9, 11)])
@pytest.mark.parametrize("V", [1, 3])
@pytest.mark.parametrize("dims", [(1, 1, 1), (2, 2, 2), (3, 4, 5), (5, 13, 5)])
def test_integration_equals_host_on_the_cpu_matrix(dims, V, H, W):
    check_integrate(TC.random_case(dims, V, H, W, 7 * V + H + dims[1]))


# lattices up to 33 x 17 x 9 (4641 points: 19 blocks, the last one partial), images up to 33 x 65, 1 and 5 views
@pytest.mark.parametrize("dims,V,H,W", [((33, 17, 9), 5, 33, 65), ((33, 17, 9), 1, 24, 32), ((16, 16, 1), 5, 5, 7),
                                        ((7, 5, 4), 5, 33, 65), ((1, 1, 300), 1, 9, 11), ((64, 4, 1), 5, 24, 32)])
def test_integration_equals_host_across_shapes(dims, V, H, W):
    got = check_integrate(TC.random_case(dims, V, H, W, H + V + dims[0]))
    assert int((got[1] > 0).sum()) > 0


def test_named_integration_cases():
    for d, kw, total, weight in ((2.0, dict(tz=-5.0), 0.0, 0), (2.0, dict(cx=0.5), 0.0, 0), (2.0, {}, 0.0, 1), (1.75, {}, -1.0, 1),
                                 (float(np.nextafter(np.float32(1.75), np.float32(0.0))), {}, 0.0, 0), (2.25, {}, 1.0, 1),
                                 (5.0, {}, 1.0, 1), (2.125, {}, 0.5, 1), (0.0, {}, 0.0, 0), (-2.0, {}, 0.0, 0), (TC.NAN, {}, 0.0, 0),
                                 (TC.INF, {}, 0.0, 0)):
        got = check_integrate(TC.one_point(d, **kw))
        assert got[0][0] == total and got[1][0] == weight, (d, kw)


def test_chunked_views_and_saturation():
    c = TC.random_case((5, 13, 5), 3, 9, 11, 5)
    whole = check_integrate(c)
    state = TS.integrate(c["depth"][:1], c["K"][:1], c["M"][:1], c["dims"], c["bounds"], c["trunc"], backend="gpu")
    back = TS.integrate(c["depth"][1:], c["K"][1:], c["M"][1:], c["dims"], c["bounds"], c["trunc"], state=state, backend="gpu")
    assert back[0] is state[0] and same_state((state[0].cpu().numpy(), state[1].cpu().numpy()), whole)
    one = TC.one_point(2.125)
    c = dict(one, depth=np.repeat(one["depth"], 3, 0), K=np.repeat(one["K"], 3, 0), M=np.repeat(one["M"], 3, 0))
    raw = lambda dev: (torch.tensor([7.25], dtype=torch.float64, device=dev),
                       torch.tensor([TC.MAX_WEIGHT - 1], dtype=torch.int32).to(torch.uint16).to(dev))
    got, want = integrate(c, "gpu", raw("cuda")), integrate(c, "host", raw("cpu"))
    assert same_state(got, want) and got[0][0] == 7.75 and got[1][0] == TC.MAX_WEIGHT


# ------------------------------------------------------------------------------------------------ extraction
def test_every_corner_pattern_of_a_cell():
    rng = np.random.default_rng(11)
    for pattern in range(256):
        for mags in (None, rng.uniform(0.25, 4.0, 8)):
            check_extract(*TC.pattern_state(pattern, mags), (2, 2, 2), TC.CELL_BOUNDS, 2)


def test_zero_corner_min_weight_and_flat_grids():
    total, weight = TC.pattern_state(0b00001010)
    total[0] = 0.0
    counts, tris = check_extract(total, weight, (2, 2, 2), TC.CELL_BOUNDS, 2)
    assert counts[0] > 0 and TS.drop_degenerate(tris)[1] > 0
    total[0] = -0.0
    check_extract(total, weight, (2, 2, 2), TC.CELL_BOUNDS, 2)
    total[0] = TC.NAN
    check_extract(total, weight, (2, 2, 2), TC.CELL_BOUNDS, 2)
    total, weight = TC.pattern_state(0b00010110)
    weight[5] = 1
    assert check_extract(total, weight, (2, 2, 2), TC.CELL_BOUNDS, 2)[0].tolist() == [0]
    assert check_extract(total, weight, (2, 2, 2), TC.CELL_BOUNDS, 1)[0][0] > 0
    for dims in ((1, 3, 3), (3, 1, 3), (3, 3, 1), (1, 1, 1)):
        total, weight = TC.shell_field(dims, 1, True)
        counts, tris = check_extract(-total, weight, dims, TC.UNIT, 1)
        assert counts.shape == (0,) and tris.shape == (0, 3, 3)


# 33 x 17 x 9: 4096 cells, 16 full blocks; 18 x 17 x 9: 2176 cells, the last block partial
@pytest.mark.parametrize("dims,unit", [((6, 6, 6), True), ((6, 6, 6), False), ((7, 5, 4), True), ((7, 5, 4), False),
                                       ((33, 17, 9), False), ((18, 17, 9), True)])
def test_random_closed_fields(dims, unit):
    total, weight = TC.shell_field(dims, dims[0], unit)
    first, raw = check_extract(total, weight, dims, TC.BOUNDS, 2)
    tris, dropped = TS.drop_degenerate(raw)
    edges = MC.mesh_edges(tris)
    assert len(tris) > 0 and dropped == 0 and edges.boundary == 0 and edges.non_manifold == 0 and TC.closed_and_oriented(tris)
    for e in np.flatnonzero(first)[::5]:                          # holes: cells that are not live, offsets that skip them
        i, j, k = e % (dims[0] - 1), (e // (dims[0] - 1)) % (dims[1] - 1), e // ((dims[0] - 1) * (dims[1] - 1))
        weight[i + dims[0] * (j + dims[1] * k)] = 1
    counts, holed = check_extract(total, weight, dims, TC.BOUNDS, 2)
    assert 0 < len(holed) < len(raw) and int(counts.astype(np.int64).sum()) == len(holed)


def test_sphere():
    total, weight = TC.sphere_field(17)
    _, raw = check_extract(total, weight, (17, 17, 17), TC.UNIT, 1)
    tris, dropped = TS.drop_degenerate(raw)
    assert dropped == 0 and TC.closed_and_oriented(tris) and TC.euler_characteristic(tris) == 2 and TC.signed_volume(tris) > 0.0


# ------------------------------------------------------------------------------------------------ the Python layer
def test_mixed_sizes_and_chunks_through_the_python_layer():
    small, large = SS.solid_scan("box", 3, 24, 32, backend="host"), SS.solid_scan("box", 2, 33, 65, backend="host")
    cams = [small.cameras[0], large.cameras[0], small.cameras[1], large.cameras[1], small.cameras[2]]
    maps = [small.depth[0], large.depth[0], small.depth[1], large.depth[1], small.depth[2]]
    kw = dict(grid=12, min_weight=1)
    (gpu, info), (host, info_h) = TS.tsdf_mesh(maps, cams, backend="gpu", **kw), TS.tsdf_mesh(maps, cams, backend="host", **kw)
    assert len(gpu) > 0 and TC.same_bits(gpu, host) and info == info_h
    for views in (1, 2):
        parts, info_p = TS.tsdf_mesh(maps, cams, backend="gpu", budget_bytes=views * 33 * 65 * 4, **kw)
        assert TC.same_bits(parts, host) and info_p == info_h


# ------------------------------------------------------------------------------------------------ the raw entries
def test_raw_entries():
    lib = _lib.load()
    dev = torch.device("cuda", torch.cuda.current_device())
    c = TC.random_case((5, 4, 3), 2, 9, 11, 9)
    lo, step = TC.lattice(c["bounds"], c["dims"])
    lo_c, step_c = (ctypes.c_double * 3)(*lo), (ctypes.c_double * 3)(*step)
    nan_c = (ctypes.c_double * 3)(lo[0], TC.NAN, lo[2])
    depth, K, M = (torch.from_numpy(np.ascontiguousarray(c[k])).to(dev) for k in ("depth", "K", "M"))
    total = torch.full((60,), -7.0, dtype=torch.float64, device=dev)
    weight = torch.full((60,), 99, dtype=torch.int32).to(torch.uint16).to(dev)
    p, s = _lib.ptr, _lib.raw_stream(dev)

    def untouched(*tensors):
        torch.cuda.synchronize()
        return all(bool((x.to(torch.float64) == (99 if x.dtype in (torch.uint8, torch.uint16) else -7.0)).all()) for x in tensors)

    good = [5, 4, 3, lo_c, step_c, 2, p(K), p(M), 9, 11, p(depth), c["trunc"], 0, p(total), p(weight), s]
    for pos, bad in ((0, 0), (1, -1), (2, 0), (0, 1 << 30), (3, None), (4, None), (3, nan_c), (4, (ctypes.c_double * 3)(0.1, 0.0, 0.1)),
                     (5, -1), (5, _lib.SEED_MAX_VIEWS + 1), (6, None), (7, None), (8, 0), (9, _lib.EDT_MAX_SIZE + 1), (10, None),
                     (11, 0.0), (11, -1.0), (11, TC.INF), (11, TC.NAN), (13, None), (14, None)):
        args = list(good)
        args[pos] = bad
        assert lib.cgs_tsdf_integrate(*args) == -1, (pos, bad)
        assert _lib.last_error().startswith("cgs_tsdf_integrate: invalid argument") and untouched(total, weight), (pos, bad)
    empty = list(good)
    empty[5], empty[6], empty[7], empty[10], empty[12] = 0, None, None, None, 1
    assert lib.cgs_tsdf_integrate(*empty) == 0 and untouched(total, weight)      # V = 0 with accumulate: nothing
    empty[12] = 0
    assert lib.cgs_tsdf_integrate(*empty) == 0                                   # V = 0 without: the empty state
    torch.cuda.synchronize()
    assert not total.any() and not weight.to(torch.int32).any()
    assert lib.cgs_tsdf_integrate(*good) == 0
    torch.cuda.synchronize()
    want = TS.integrate(c["depth"], c["K"], c["M"], c["dims"], c["bounds"], c["trunc"], backend="host")
    assert same_state((total.cpu().numpy(), weight.cpu().numpy()), (want[0].numpy(), want[1].numpy()))

    field, w2 = (torch.from_numpy(x).to(dev) for x in TC.shell_field((5, 4, 3), 2, False))
    kept = field.clone()
    counts = torch.full((24,), 99, dtype=torch.uint8, device=dev)
    good = [5, 4, 3, p(field), p(w2), 2, p(counts), s]
    for pos, bad in ((0, 0), (1, -1), (2, 1 << 30), (3, None), (4, None), (5, 0), (5, 65536), (6, None)):
        args = list(good)
        args[pos] = bad
        assert lib.cgs_tsdf_mesh_count(*args) == -1, (pos, bad)
        assert _lib.last_error().startswith("cgs_tsdf_mesh_count: invalid argument") and untouched(counts), (pos, bad)
    flat = list(good)
    flat[1] = 1
    assert lib.cgs_tsdf_mesh_count(*flat) == 0 and untouched(counts)             # a dimension of 1: no cells, nothing written
    assert lib.cgs_tsdf_mesh_count(*good) == 0
    torch.cuda.synchronize()
    want_counts, want_tris = extract(kept.cpu().numpy(), w2.cpu().numpy(), (5, 4, 3), TC.BOUNDS, 2, "host")
    assert (counts.cpu().numpy() == want_counts).all() and want_tris.shape[0] > 0

    offsets = (torch.cumsum(counts, 0, dtype=torch.int64) - counts).contiguous()   # what the count pass produced
    T = int(want_tris.shape[0])
    tris = torch.full((T + 2, 3, 3), -7.0, dtype=torch.float32, device=dev)
    good = [5, 4, 3, lo_c, step_c, p(field), p(w2), 2, p(offsets), T, p(tris), s]
    for pos, bad in ((0, 0), (1, -1), (2, 1 << 30), (3, None), (4, None), (3, nan_c), (5, None), (6, None), (7, 0), (7, 65536),
                     (8, None), (9, -1), (10, None)):
        args = list(good)
        args[pos] = bad
        assert lib.cgs_tsdf_mesh_emit(*args) == -1, (pos, bad)
        assert _lib.last_error().startswith("cgs_tsdf_mesh_emit: invalid argument") and untouched(tris), (pos, bad)
    for pos, value in ((1, 1), (9, 0)):                                          # no cells; T = 0: nothing to write
        args = list(good)
        args[pos] = value
        assert lib.cgs_tsdf_mesh_emit(*args) == 0 and untouched(tris), (pos, value)
    short = list(good)
    short[9] = T - 1                                                             # the last cell's range does not fit: it writes nothing
    assert lib.cgs_tsdf_mesh_emit(*short) == 0
    torch.cuda.synchronize()
    last = int(offsets[counts > 0][-1])
    assert TC.same_bits(tris[:last].cpu().numpy(), want_tris[:last]) and untouched(tris[last:])
    assert lib.cgs_tsdf_mesh_emit(*good) == 0
    torch.cuda.synchronize()
    assert TC.same_bits(tris[:T].cpu().numpy(), want_tris) and untouched(tris[T:])
    assert torch.equal(field, kept)


# ------------------------------------------------------------------------------------------------ end to end
def test_box_end_to_end(tmp_path):
    tris, info, _, scan = TC.box_end_to_end("gpu", tmp_path)
    host, info_h = TS.tsdf_mesh(list(scan.depth), scan.cameras, grid=48, backend="host")
    assert TC.same_bits(tris, host) and info == info_h
