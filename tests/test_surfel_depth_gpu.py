"""GPU: cgs_surfel_depth (csrc/surfel_depth.hip, k_surfel_depth) against the host back end of ops.edge_occlusion, bit for bit
-- every case of test_surfel_depth_cpu.py (where the host back end is held to the brute force), the raw C entry with its
empty inputs and rejected arguments, 1, 63, 64, 65 and 257 surfels with small and large disks side by side, the order of
the points --, a point-cloud occluder through ChunkDepth and its consumers, and surfel_radii on both back ends.

surfel_radii: the GPU back end takes mean_dist2 from cgs_knn_mean_dist2 in float32, the host back end from an exact float64
3-NN rounded to float32 once.  Against the float64 value the kernel is granted 1e-6 relative (tests/test_knn_ref64_gpu.py,
RTOL, which states why: 2.4e-7 from the arithmetic, the rest for a third neighbour that ties within it) and the host's one
rounding is 2^-24 = 6e-8; the radius is the square root, which halves a relative error, so two radii that both come from
the uncapped branch differ by at most (1e-6 + 6e-8) / 2 relative, and a capped one by the same through the median; each
radius is then stored as float32, one more rounding of 2^-24 on either side.  The largest differences on this input are
printed before they are asserted."""
import ctypes

import numpy as np
import pytest
import torch

import edge_gate_cases as GC
import edge_vote_gate_cases as VG
import surfel_cases as C
from curve_gaussian_amd import _lib as L
from curve_gaussian_amd.edge_extraction import reprojection as R
from curve_gaussian_amd.ops import edge_occlusion as EO
from curve_gaussian_amd.ops import edge_score as ES
from curve_gaussian_amd.scene import solid_scan as SS
from knn_ref64 import mean_dist2_ref64
from test_knn_ref64_gpu import RTOL as KNN_RTOL

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
INVALID = -1   # CGS_ERR_INVALID_ARGUMENT


def both(pts, nrm, rad, K, M, H, W, window=0):
    """(the kernel's planes, the host's)."""
    cloud = EO.Surfels(pts, nrm, rad)
    got = EO.surfel_depth(cloud, K, M, H, W, window=window, device=DEV)
    assert got.is_cuda and got.dtype == torch.float32
    return got.cpu().numpy(), EO.surfel_depth(cloud, K, M, H, W, window=window, backend="host").numpy()


# ------------------------------------------------------------------------------------------------ the rule
@pytest.mark.parametrize("normals", [True, False], ids=["normals", "normals_none"])
@pytest.mark.parametrize("H, W", C.SIZES)
def test_the_kernel_equals_the_host_on_every_branch(H, W, normals):
    pts, nrm, rad = C.special(normals=normals)
    K, M = C.cameras(C.VIEWS, H, W)
    got, want = both(pts, nrm, rad, K, M, H, W)
    assert C.same_bits(got, want)
    assert np.isfinite(got[0]).all()
    for window in (1, 4):
        assert C.same_bits(*both(pts, nrm, rad, K, M, H, W, window))


def test_every_branch_on_its_own():
    H, W = C.SIZES[-1]
    K, M = C.cameras(C.VIEWS, H, W)
    for name in C.SPECIAL:
        got, want = both(*C.special([name]), K, M, H, W)
        assert C.same_bits(got, want), name
        if name in C.STORES_NOTHING:
            assert not np.isfinite(got[0]).any(), name
    pts, nrm, rad = C.special()
    base, _ = both(pts, nrm, rad, K, M, H, W)
    assert C.same_bits(base, both(pts, -nrm, rad, K, M, H, W)[0]), "two-sided"
    assert C.same_bits(both(*C.special(["coincident_a"]), K, M, H, W)[0],
                       both(*C.special(["coincident_a", "coincident_b"]), K, M, H, W)[0])


@pytest.mark.parametrize("P", C.WAVE_COUNTS)
def test_wave_shape_edges_with_small_and_large_disks_mixed(P):
    """One surfel, a workgroup of four short by one, full, one into the next, and 257 (a last workgroup of one wave); boxes of
    a fraction of a pixel up to 60 pixels across side by side, so that waves with one step and with dozens run in one
    launch, a stretch of 64 surfels with small disks only, and a large disk last."""
    H, W = C.WAVE_SIZE
    K, M = C.cameras(C.VIEWS, H, W)
    pts, nrm, rad = C.wave_cloud(P)
    got, want = both(pts, nrm, rad, K, M, H, W)
    assert C.same_bits(got, want)
    assert np.isfinite(got).any() and not np.isfinite(got).all()
    assert C.same_bits(*both(pts, None, rad, K, M, H, W))


def test_the_order_of_the_points_does_not_show():
    H, W = C.WAVE_SIZE
    K, M = C.cameras(C.VIEWS, H, W)
    pts, nrm, rad = C.wave_cloud(257)
    base, want = both(pts, nrm, rad, K, M, H, W)
    for seed in (3, 4):
        perm = np.random.default_rng(seed).permutation(len(pts))
        assert C.same_bits(base, both(pts[perm], nrm[perm], rad[perm], K, M, H, W)[0])
    assert C.same_bits(base, want)


# ------------------------------------------------------------------------------------------------ the raw C entry
def test_the_raw_entry_with_empty_inputs_and_rejected_arguments():
    lib = L.load()
    H, W = C.WAVE_SIZE
    K, M = C.cameras(C.VIEWS, H, W)
    pts, nrm, rad = (torch.from_numpy(a).to(DEV) for a in C.wave_cloud(65))
    Kd, Md = ES.cameras_on(DEV, K, M.reshape(len(K), 12))
    stream = L.raw_stream(DEV)
    want = EO.surfel_depth(EO.Surfels(*C.wave_cloud(65)), K, M, H, W, window=0, backend="host").numpy()
    want_flat = EO.surfel_depth(EO.Surfels(C.wave_cloud(65)[0], None, C.wave_cloud(65)[2]), K, M, H, W, window=0,
                                backend="host").numpy()

    def call(P=65, points=pts, normals=nrm, radii=rad, V=C.VIEWS, intr=Kd, w2c=Md, height=H, width=W, depth="fresh"):
        out = torch.full((C.VIEWS, H, W), 7.0, dtype=torch.float32, device=DEV) if isinstance(depth, str) else depth
        rc = lib.cgs_surfel_depth(P, L.ptr(points), L.ptr(normals), L.ptr(radii), V, L.ptr(intr), L.ptr(w2c), height, width,
                                  L.ptr(out), stream)
        torch.cuda.synchronize(DEV)
        return rc, None if out is None else out.cpu().numpy()

    rc, out = call()
    assert rc == 0 and C.same_bits(out, want)
    rc, out = call(normals=None)
    assert rc == 0 and C.same_bits(out, want_flat), "normals = NULL: every disk faces the camera plane"
    rc, out = call(P=0)
    assert rc == 0 and np.isposinf(out).all(), "P = 0 still clears the planes"
    rc, out = call(P=0, points=None, normals=None, radii=None)
    assert rc == 0 and np.isposinf(out).all()
    rc, out = call(V=0)
    assert rc == 0 and (out == 7.0).all(), "V = 0 is a no-op"
    for bad in (dict(P=-1), dict(V=-1), dict(height=0), dict(width=L.EDT_MAX_SIZE + 1), dict(points=None), dict(radii=None),
                dict(intr=None), dict(w2c=None), dict(height=0, V=0), dict(points=None, V=0)):
        rc, out = call(**bad)
        assert rc == INVALID and (out == 7.0).all(), bad
        assert lib.cgs_last_error().decode().startswith("cgs_surfel_depth: invalid argument ("), bad
    rc, _ = call(depth=None)
    assert rc == INVALID


# ------------------------------------------------------------------------------------------------ through ChunkDepth
@pytest.fixture(scope="module")
def box():
    scan = GC.solid("box", 5, 48, 64)
    pts, nrm = SS.surfel_cloud(scan.tris, 0.02)
    return scan, EO.Surfels(pts, nrm, EO.surfel_radii(pts, backend="host"))


def test_chunk_depth_planes_of_a_cloud_equal_the_hosts(box):
    from curve_gaussian_amd.ops.view_chunks import camera_arrays
    scan, cloud = box
    K, M = camera_arrays(scan.cameras)
    sel = list(range(len(scan.cameras)))
    host = EO.ChunkDepth("t", scan.cameras, occluder=cloud).to("host").planes(48, 64, sel, K, M)
    gate = EO.ChunkDepth("t", scan.cameras, occluder=cloud).to("gpu", DEV)
    assert all(t is None or t.is_cuda for t in gate.surfels), "uploaded once"
    got = gate.planes(48, 64, sel, K, M)
    assert got.is_cuda and C.same_bits(got.cpu().numpy(), host.numpy())
    assert np.isfinite(host.numpy()).any()
    assert gate.settings()["occluder_kind"] == "surfels" and gate.settings()["surfels"] == len(cloud.points)


def test_the_score_the_checks_and_the_vote_take_a_cloud_on_the_gpu(box):
    scan, cloud = box
    want = R.score_edges(scan.edges, scan.cameras, scan.maps, "PidiNet", backend="host", occluder=cloud)
    got = R.score_edges(scan.edges, scan.cameras, scan.maps, "PidiNet", occluder=cloud, device=DEV)
    assert got["views"] == want["views"] and got["aggregate"] == want["aggregate"]
    assert got["settings"]["occluder_kind"] == "surfels" and sum(row["hidden_points"] for row in got["views"]) > 0
    want = GC.comparable(GC.scan_level(scan, "host", None, occluder=cloud))
    assert GC.comparable(GC.scan_level(scan, "gpu", None, device=DEV, occluder=cloud)) == want   # edge_support, trim, snap
    vote_scan = VG.solid("box")
    pts, nrm = SS.surfel_cloud(vote_scan.tris, 0.02)
    vote_cloud = EO.Surfels(pts, nrm, EO.surfel_radii(pts, backend="host"))
    seeds, info, keep, _, counts = VG.solid_votes("box", "gpu", DEV, occluder=vote_cloud)
    want_seeds, want_info, want_keep, _, want_counts = VG.solid_votes("box", "host", occluder=vote_cloud)
    assert np.array_equal(seeds, want_seeds) and np.array_equal(keep, want_keep) and info["hidden_pairs"] == want_info["hidden_pairs"] > 0
    assert all(np.array_equal(a, b) for a, b in zip(counts, want_counts))
    assert info["occluder_kind"] == "surfels"


# ------------------------------------------------------------------------------------------------ surfel_radii
def test_surfel_radii_on_both_back_ends():
    rng = np.random.default_rng(17)
    pts = rng.uniform(0, 1, (500, 3)).astype(np.float32)
    pts = np.concatenate([pts, pts[:1]])                                   # an exact duplicate pair
    gpu = EO.surfel_radii(pts, device=DEV)
    host = EO.surfel_radii(pts, backend="host")
    ref = mean_dist2_ref64(torch.from_numpy(pts)).numpy()
    exact = np.sqrt(ref)
    exact = np.minimum(exact, EO.SURFEL_RADIUS_CAP * np.median(exact))
    worst = {name: float((np.abs(r.astype(np.float64) - exact) / exact).max()) for name, r in (("gpu", gpu), ("host", host))}
    between = float((np.abs(gpu.astype(np.float64) - host.astype(np.float64)) / exact).max())
    print(f"\n   surfel_radii, 501 points: worst relative error against float64, gpu {worst['gpu']:.3e}, host {worst['host']:.3e}; "
          f"between the back ends {between:.3e}")
    assert gpu.dtype == host.dtype == np.float32 and gpu.shape == host.shape == (501,)
    assert gpu[0] == gpu[500] and host[0] == host[500] and (exact > 0).all()
    store = 2.0 ** -24                                                     # the radius itself is stored as float32
    assert worst["host"] <= 2.0 ** -24 / 2 + store
    assert worst["gpu"] <= KNN_RTOL / 2 + store
    assert between <= (KNN_RTOL + 2.0 ** -24) / 2 + 2 * store
    with pytest.raises(ValueError, match="factor"):
        EO.surfel_radii(pts, -1.0, device=DEV)
