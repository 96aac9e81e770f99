"""GPU: the five 3-NN initialisation kernels of csrc/knn.hip (bbox, Morton keys, single-workgroup bitonic sort, per-1024
boxes, pruned exact search) behind simple_knn.distCUDA2, against the float64 reference of tests/knn_ref64.py on the clouds
built there: every size next to a box (1024) or a power of two, P = 4 .. 7 where the +-3 seed window is clipped at both
ends, planar / collinear / all-negative clouds (0/0 or a seeded maximum in the Morton quotient), clusters far from the origin
whose codes collapse, points that hug the top octant split, exact lattices, duplicates and identical points.

Criterion (derived, not tuned): a float32 d^2 carries at most about 6 roundings (the difference, three squares or FMAs, two
adds), the three-term sum and the division 3 more, every term is non-negative so nothing cancels: below 10 * 2^-24 ~ 6e-7
relative.  Where float32 picks another third neighbour than float64 the two candidates tie within the same bound.  So
|out - ref| <= 1e-6 * ref for EVERY element, no outlier allowance, no absolute floor; where ref is exactly 0 (three or more
copies of the point) out must be exactly 0.  The clouds keep every non-zero d^2 above 1e-20 (knn_ref64._finish).

Order independence is bit-exact: the three smallest float32 d^2 of a point are one multiset and the insertion leaves them
sorted, so ``distCUDA2(x[perm]) == distCUDA2(x)[perm]``; a difference means a lost or repeated key or a box skipped in error.

Measured on an MI355X, worst |out - ref| / ref per case (pytest -s prints them):
    cube P = 4 1.03e-7, 5 0.93e-7, 7 1.13e-7, 8 0.70e-7, 1023 1.37e-7, 1024 1.42e-7, 1025 1.56e-7, 2047 1.43e-7,
         2048 1.54e-7, 2049 1.47e-7, 3073 1.58e-7
    at P = 1025 | 2049:  cube 1.49e-7 | 1.43e-7   dupes 1.62e-7 | 1.51e-7 (90 | 180 exact zeros)   far_pair 3.8e-8 | 3.7e-8
         far_tight 4.0e-8 | 4.0e-8   far_tight_neg 4.0e-8 | 4.0e-8   lattice 3.4e-8 | 3.4e-8   line_x 1.15e-7 | 1.28e-7
         negative 1.27e-7 | 1.66e-7   plane_off 1.47e-7 | 1.39e-7   plane_z0 1.29e-7 | 1.39e-7   seam 1.53e-7 | 2.27e-7
    at P = 4097:  seam 1.53e-7   far_tight 4.0e-8   far_tight_neg 4.0e-8
    colmap_like P = 70 001: 1.90e-7 (distCUDA2 wall time 5.9 ms, the single-workgroup sort included)
All under 1e-6; the far clouds and the lattice have exact float32 differences and squares, what is left is the sum and the
division.  far_tight cannot give ALL points one code at the centre (1000, -1000, 1000): the points on the bbox's maximum
in x or z fall into cell 1023, the rest into 1022 (knn_ref64.far_tight); far_tight_neg is the fully collapsed cloud.

create_from_pcd on the duplicate groups: the span read back as the difference of two stored float32 end points is within
1.1e-4 of 2 * 0.5 * sqrt(1e-7) -- that is the half ulp of each end point (coordinates up to 1 against a span of 3.2e-4), not
the kernel or the clamp, so the comparison carries that storage term on top of 1e-6 and the end points are ALSO held bit
for bit to y -+ 0.5f * sqrtf(1e-7f).
"""
import functools
import time
import types

import numpy as np
import pytest
import torch

import knn_ref64 as K
from oracle import torch_ref as TR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RTOL = 1e-6


def _dist(pts):
    from curve_gaussian_amd.simple_knn import distCUDA2
    return distCUDA2(pts.to(DEV)).cpu()


@functools.lru_cache(maxsize=None)
def _case(name, P, seed=0):
    """(points, float64 reference): built once, shared by the tests, never written to."""
    pts = K.BUILDERS[name](P, seed)
    return pts, K.mean_dist2_ref64(pts)


def _hold(out, ref, label):
    assert out.dtype == torch.float32 and out.shape == ref.shape and bool(torch.isfinite(out).all()), label
    err = (out.double() - ref).abs()
    nz = ref > 0
    worst = float((err[nz] / ref[nz]).max()) if bool(nz.any()) else 0.0
    print(f"knn_ref64 {label}: worst relative error {worst:.3e}, exact zeros {int((~nz).sum())}")
    assert bool((out[~nz] == 0).all()), label
    assert bool((err <= RTOL * ref).all()), (label, worst)
    return worst


@pytest.mark.parametrize("P", [4, 5, 7, 8, 1023, 1024, 1025, 2047, 2048, 2049, 3073])
def test_size_edges_on_the_cube(P):
    pts, ref = _case("cube", P, P)
    _hold(_dist(pts), ref, f"cube P={P}")


@pytest.mark.parametrize("P", [1, 2, 3])
def test_fewer_than_four_points_give_the_float32_tail_bit_for_bit(P):
    pts = K.cube(P, P)
    want = K.mean_dist2_fp32_small_p(pts.numpy())
    got = _dist(pts).numpy()
    assert got.dtype == np.float32 and got.view(np.uint32).tolist() == want.view(np.uint32).tolist()


CLOUDS = [(name, P) for name in sorted(K.BUILDERS) if not name.startswith("same") for P in (1025, 2049)]
CLOUDS += [(name, 4097) for name in ("seam", "far_tight", "far_tight_neg")]


@pytest.mark.parametrize("name,P", CLOUDS)
def test_every_cloud_within_the_float32_bound(name, P):
    pts, ref = _case(name, P)
    _hold(_dist(pts), ref, f"{name} P={P}")


@pytest.mark.parametrize("name", ["same_origin", "same_offset"])
@pytest.mark.parametrize("P", [4, 1025, 2049])
def test_identical_points_give_exact_zeros(name, P):
    out = _dist(K.BUILDERS[name](P, 0))          # at the origin: 0/0 on all three axes of the Morton quotient
    assert out.shape == (P,) and bool((out == 0).all())


@pytest.mark.parametrize("P", [1025, 2049])
def test_duplicate_groups(P):
    pts, ref = _case("dupes", P)
    out = _dist(pts)
    groups = K.dupes_groups(P, 0)
    a = pts.double()
    for size, members in groups.items():
        for m in members:
            m = torch.as_tensor(m)
            d2 = ((a[m[0]][None] - a) ** 2).sum(-1)
            d2[m] = float("inf")
            nearest = torch.sort(d2).values          # the other, distinct points, ascending
            if size >= 4:
                assert bool((out[m] == 0).all()) and bool((ref[m] == 0).all())
                continue
            want = float(nearest[0]) / 3 if size == 3 else float(nearest[0] + nearest[1]) / 3
            assert want > 0 and bool(((ref[m] - want).abs() <= 1e-15 * want).all())
            assert bool(((out[m].double() - want).abs() <= RTOL * want).all()), (size, want, out[m])


@pytest.mark.parametrize("name", ["cube", "lattice", "seam", "far_tight"])
def test_order_independence_is_bit_exact(name):
    pts, ref = _case(name, 2049)
    out = _dist(pts)
    assert torch.equal(out, _dist(pts))                                  # two runs on the same input
    for seed in (1, 2, 3):
        perm = torch.randperm(2049, generator=torch.Generator().manual_seed(seed))
        assert torch.equal(_dist(pts[perm]), out[perm]), (name, seed)
    _hold(out, ref, f"{name} P=2049 (order)")


def test_colmap_like_cloud_at_scale():
    P = 70001
    pts = K.colmap_like(P, 0)
    ref = K.mean_dist2_ref64(pts, device=DEV, chunk=256)                 # plain torch float64 ops, none of the library's
    x = pts.to(DEV)
    from curve_gaussian_amd.simple_knn import distCUDA2
    distCUDA2(x)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = distCUDA2(x)
    torch.cuda.synchronize()
    print(f"knn_ref64 colmap_like P={P}: distCUDA2 wall time {1e3 * (time.perf_counter() - t0):.2f} ms")
    _hold(out.cpu(), ref, f"colmap_like P={P}")


def test_wrapper_dtypes_strides_empty_and_cpu_input():
    from curve_gaussian_amd import _lib as L
    from curve_gaussian_amd.simple_knn import distCUDA2
    pts, ref = _case("cube", 1025, 1025)
    out = _dist(pts)
    assert torch.equal(distCUDA2(pts.double().to(DEV)).cpu(), out)
    buf = torch.full((1025, 6), 7.0)
    buf[:, :3] = pts
    view = buf.to(DEV)[:, :3]
    assert not view.is_contiguous() and torch.equal(distCUDA2(view).cpu(), out)
    empty = distCUDA2(torch.zeros(0, 3, device=DEV))
    assert tuple(empty.shape) == (0,) and empty.dtype == torch.float32 and empty.is_cuda
    with pytest.raises(L.CurveGSError, match="points must be a GPU tensor"):
        distCUDA2(pts)


@pytest.mark.parametrize("P", [1, 1025, 2049])
def test_workspace_carving_stays_inside_the_reported_size(P):
    """The guard is the tail of the SAME allocation, so an overrun would show as a changed byte and nothing else."""
    from curve_gaussian_amd import _lib as L
    lib = L.load()
    pts = K.cube(P, P)
    want = _dist(pts)
    dev = torch.device(DEV)
    x = pts.to(dev).contiguous()
    nbytes = int(lib.cgs_knn_workspace_bytes(P))
    n, nb = max(P, 1), (max(P, 1) + K.KNN_BOX - 1) // K.KNN_BOX
    assert nbytes >= 32 + 8 * n + 4 * n + 24 * nb + 3 * 127          # bbox, keys, indices, boxes, 128-byte alignment
    ws = torch.full((nbytes + 4096,), 0xA5, dtype=torch.uint8, device=dev)
    out = torch.zeros(P, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        L.check(lib.cgs_knn_mean_dist2(P, L.ptr(x), L.ptr(out), L.ptr(ws), L.raw_stream(dev)), "cgs_knn_mean_dist2")
    torch.cuda.synchronize()
    assert bool((ws[nbytes:] == 0xA5).all())
    assert torch.equal(out.cpu(), want)


class _Cam:
    def __init__(self, n):
        self.image_name = n


def test_create_from_pcd_on_the_seam_cloud():
    from curve_gaussian_amd.scene import GaussianCurveModel
    pts, ref = _case("seam", 1025)
    tr = TR.knn_mean_dist2_f64(pts)                      # the restatement's distances: accurate on this cloud?
    assert bool(((tr - ref).abs() <= 1e-9 * ref).all())
    colors = np.random.default_rng(0).random((1025, 3)).astype(np.float32)
    pcd = types.SimpleNamespace(points=pts.numpy(), colors=colors)
    gm = GaussianCurveModel(0, 12, device=DEV).create_from_pcd(pcd, [_Cam("a")], 1.0)
    want = TR.create_from_pcd(pcd.points, pcd.colors, 12, 0)
    for name, got in (("curve_points", gm._curve_points), ("opacity", gm._opacity), ("width", gm._width),
                      ("features_dc", gm._features_dc), ("mask", gm._mask), ("xyz", gm._xyz), ("scaling", gm._scaling),
                      ("rotation", gm._rotation)):
        r = want[name]
        assert tuple(got.shape) == tuple(r.shape), name
        assert torch.allclose(got.detach().cpu(), r, rtol=2e-5, atol=2e-6), name
    assert abs(float(gm.dist) - float(want["dist"])) < 1e-6
    cp = gm._curve_points.detach().cpu()
    span = (cp[:, 3, 1] - cp[:, 0, 1]).double()
    # the two float32 end points are stored rounded: half an ulp of a coordinate below 2 each, on top of the 1e-5 of the
    # existing grid test for the square root's argument
    assert bool(((span - torch.sqrt(ref)).abs() <= 1e-5 * torch.sqrt(ref) + 2.0 ** -23).all())


def test_create_from_pcd_clamps_duplicate_groups():
    """Groups of four or more copies have distCUDA2 == 0 and take the clamp_min(1e-7) branch: the curve spans
    2 * 0.5 * sqrt(1e-7) along Y."""
    from curve_gaussian_amd.scene import GaussianCurveModel
    P = 1025
    pts, _ = _case("dupes", P)
    pcd = types.SimpleNamespace(points=pts.numpy(), colors=np.full((P, 3), 0.5, np.float32))
    gm = GaussianCurveModel(0, 12, device=DEV).create_from_pcd(pcd, [_Cam("a")], 1.0)
    cp = gm._curve_points.detach().cpu().double()
    assert bool(torch.isfinite(cp).all())
    groups = K.dupes_groups(P, 0)
    m = torch.as_tensor(np.concatenate(groups[4] + groups[5]))
    want = 2 * 0.5 * float(np.sqrt(np.float64(np.float32(1e-7))))
    span = cp[m, 3, 1] - cp[m, 0, 1]
    # 1e-6 relative on the span itself; the test reads it as the difference of two STORED float32 end points y -+ bound,
    # each rounded by at most half an ulp of its own magnitude, ulp(v) <= |v| * 2^-23 and |v| <= |y| + bound: the two
    # halves together are at most (|y| + bound) * 2^-23, which the comparison has to carry on top
    store = (pts[m, 1].double().abs() + want) * 2.0 ** -23
    print(f"knn_ref64 dupes create_from_pcd: worst |span - want| / want {float(((span - want).abs() / want).max()):.3e}")
    assert bool(((span - want).abs() <= 1e-6 * want + store).all())
    # and what that rounding hides, bit for bit: the stored end points are y -+ bound in float32 with
    # bound = 0.5f * sqrtf(1e-7f), square root and sums correctly rounded
    b32 = np.float32(0.5) * np.sqrt(np.float32(1e-7))
    y32 = pts[m, 1].numpy()
    got = gm._curve_points.detach().cpu().numpy()[m.numpy()]
    for k, off in enumerate((-b32, np.float32(-0.5) * b32, np.float32(0.5) * b32, b32)):
        assert np.array_equal(got[:, k, 1], y32 + off), k
    assert torch.equal(cp[m, :, 0], pts[m, 0].double()[:, None].expand(-1, 4))
    assert torch.equal(cp[m, :, 2], pts[m, 2].double()[:, None].expand(-1, 4))
