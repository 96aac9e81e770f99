"""Float64 reference and hard point clouds for the 3-NN initialisation kernels (csrc/knn.hip, simple_knn.distCUDA2).

Reference.  ``mean_dist2_ref64`` widens the float32 points to float64 and forms every squared distance from explicit
differences, ``((a[:, None, :] - b[None]) ** 2).sum(-1)``: the differences of two float32 numbers are exact in float64
(their exponents are at most 2^11 apart in every cloud below), so each d^2 carries three squarings and two adds, about
5 * 2^-53 relative, wherever the cloud sits.  ``oracle/torch_ref.py::knn_mean_dist2`` goes through ``torch.cdist``, which for
more than about 25 points may expand |a|^2 + |b|^2 - 2 a.b and takes a square root: on a cluster at 1000 with spacing 1e-3
the expansion would lose |x|^2 * 2^-53 ~ 7e-10 absolute against d^2 ~ 1e-6 and below.  tests/test_knn_ref64_cpu.py prints
what that oracle actually loses there (4e-16 relative with torch 2.10, whose float64 cdist stays on the direct path); the
reference here does not depend on which path a torch version picks.

Clouds.  Every builder is ``(P, seed) -> float32 [P, 3]``, deterministic, and asserts the property it exists for, so that an
edit cannot quietly turn a hard case into an easy one.  Every builder also asserts that the smallest non-zero gap between
two coordinates of an axis is above 1e-10, so every non-zero d^2 is above 1e-20 and no float32 subnormal is involved.

``morton_codes`` restates k_knn_bbox / k_knn_morton (the reference's simple_knn.cu:55-62 and :192-200) in float32 numpy:
the bounding box seeded with the origin, ``uint32(((c - min) / (max - min)) * 1023)`` per axis, bits interleaved x, y, z
from the bottom.  On an axis of zero extent the quotient is 0/0 and the cast's result is arbitrary on the device; the
restatement puts 0 there (the same for every point, as on the device, so the order among the points is unaffected)."""
import numpy as np
import torch

FLT_MAX = np.float32(3.4028234663852886e38)
KNN_BOX = 1024          # csrc/knn.hip


# ----------------------------------------------------------------------------- references
def mean_dist2_ref64(points_f32, device="cpu", chunk=None):
    """Mean of the three smallest squared distances to the OTHER points (self excluded by index, so duplicates count at
    distance 0), float64 [P] on the CPU.  Plain torch float64 ops on `device`, in row chunks; no cdist, no GEMM expansion,
    no square root.  Needs P >= 4 (below that the kernel's answer is the float32 tail of mean_dist2_fp32_small_p)."""
    pts = torch.as_tensor(points_f32)
    assert pts.dtype == torch.float32 and pts.dim() == 2 and pts.shape[1] == 3
    P = pts.shape[0]
    if P < 4:
        raise ValueError("fewer than four points: see mean_dist2_fp32_small_p")
    a = pts.to(device).double()
    if chunk is None:
        chunk = max(1, min(P, (1 << 22) // P))          # [chunk, P, 3] float64: at most 96 MiB
    out = torch.empty(P, dtype=torch.float64, device=a.device)
    for r0 in range(0, P, chunk):
        r1 = min(P, r0 + chunk)
        d2 = ((a[r0:r1, None, :] - a[None]) ** 2).sum(-1)
        rows = torch.arange(r1 - r0, device=a.device)
        d2[rows, rows + r0] = float("inf")
        best = torch.topk(d2, 3, dim=1, largest=False, sorted=True).values
        out[r0:r1] = ((best[:, 0] + best[:, 1]) + best[:, 2]) / 3.0
    return out.cpu()


def mean_dist2_fp32_small_p(points):
    """The reference's float32 tail for P < 4 (simple_knn.cu:132-184): best[] starts at FLT_MAX, every other point goes
    through the three-slot insertion, and the result is ``((best0 + best1) + best2) / 3.0f`` in float32.  Float32 [P]."""
    p = np.asarray(points, dtype=np.float32)
    P = p.shape[0]
    assert P < 4
    out = np.empty(P, np.float32)
    with np.errstate(over="ignore"):
        for i in range(P):
            best = [FLT_MAX, FLT_MAX, FLT_MAX]
            for j in range(P):
                if j == i:
                    continue
                d = p[j] - p[i]
                dist = np.float32(np.float32(d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
                for k in range(3):
                    if best[k] > dist:
                        best[k], dist = dist, best[k]
            out[i] = np.float32(np.float32(best[0] + best[1]) + best[2]) / np.float32(3.0)
    return out


def _spread(v):
    v = v.astype(np.uint32)
    v = (v | (v << 16)) & 0x030000FF
    v = (v | (v << 8)) & 0x0300F00F
    v = (v | (v << 4)) & 0x030C30C3
    v = (v | (v << 2)) & 0x09249249
    return v


def morton_cells(points):
    """The kernel's per-axis 10-bit cells, uint32 [P, 3] (see the module docstring for the 0/0 axis)."""
    p = np.asarray(points, dtype=np.float32)
    mn = np.minimum(p.min(0), np.float32(0))
    mx = np.maximum(p.max(0), np.float32(0))
    with np.errstate(invalid="ignore", divide="ignore"):
        r = ((p - mn) / (mx - mn)) * np.float32(1023)
    return np.where(np.isfinite(r), r, 0).astype(np.uint32)


def morton_codes(points):
    c = morton_cells(points)
    return _spread(c[:, 0]) | (_spread(c[:, 1]) << 1) | (_spread(c[:, 2]) << 2)


def morton_order(points):
    """The sorted order of k_knn_sort: ascending (code << 32 | index)."""
    code = morton_codes(points).astype(np.uint64)
    return np.argsort((code << np.uint64(32)) | np.arange(len(code), dtype=np.uint64), kind="stable")


# ----------------------------------------------------------------------------- clouds
def _rng(seed, salt):
    return np.random.default_rng([int(seed), salt])


def _uniform(rng, *shape):
    """Uniform multiples of 2^-24 in [0, 1), as float32 (exact)."""
    return rng.random(shape, dtype=np.float32)


def _finish(pts, P):
    pts = np.ascontiguousarray(pts, dtype=np.float32)
    assert pts.shape == (P, 3) and np.isfinite(pts).all()
    for c in range(3):
        gaps = np.diff(np.unique(pts[:, c]).astype(np.float64))
        assert gaps.size == 0 or gaps.min() > 1e-10          # every non-zero d^2 is above 1e-20
    return torch.from_numpy(pts)


def cube(P, seed):
    pts = _uniform(_rng(seed, 1), P, 3)
    assert pts.min() >= 0 and pts.max() < 1
    return _finish(pts, P)


def plane_z0(P, seed):
    pts = _uniform(_rng(seed, 2), P, 3)
    pts[:, 2] = 0
    assert (pts[:, 2] == 0).all() and (P < 2 or np.ptp(pts[:, 0]) > 0)
    return _finish(pts, P)


def plane_off(P, seed):
    pts = _uniform(_rng(seed, 3), P, 3)
    pts[:, 2] = np.float32(0.37)
    assert (pts[:, 2] == np.float32(0.37)).all()
    return _finish(pts, P)


def line_x(P, seed):
    pts = _uniform(_rng(seed, 4), P, 3)
    pts[:, 1:] = 0
    assert (pts[:, 1:] == 0).all()
    return _finish(pts, P)


def negative(P, seed):
    pts = -(np.float32(1) - _uniform(_rng(seed, 5), P, 3))           # [-1, 0): multiples of 2^-24, exact
    assert pts.max() < 0 and pts.min() >= -1                         # the bbox maximum stays at the seeded origin
    return _finish(pts, P)


def _far_cluster(P, seed, salt, centre, extent):
    u = _rng(seed, salt).random((P, 3))
    return (np.asarray(centre, np.float64) + (u - 0.5) * extent).astype(np.float32)


def far_tight(P, seed):
    """Centre (1000, -1000, 1000), extent 0.01.  The bbox runs from the seeded origin to the cluster, so y falls into cell
    0 and x, z into cell 1022 -- except for the points ON the bbox's maximum in x or z, whose quotient is exactly 1 and whose
    cell is 1023 (no cluster on the positive side can avoid that: some point is the maximum).  Asserted: every point off
    those two faces has one and the same 30-bit code, at least 95 % of the cloud, and the others differ from it in the lowest
    Morton level only.  far_tight_neg is the cloud where all P codes are equal."""
    pts = _far_cluster(P, seed, 6, (1000.0, -1000.0, 1000.0), 0.01)
    code = morton_codes(pts)
    on_max = (pts[:, 0] == pts[:, 0].max()) | (pts[:, 2] == pts[:, 2].max())
    assert len(np.unique(code[~on_max])) <= 1 and len(np.unique(code >> 3)) == 1
    assert P < 100 or on_max.sum() <= 0.05 * P
    return _finish(pts, P)


def far_tight_neg(P, seed):
    """far_tight mirrored to (-1000, -1000, -1000): every quotient is below 1e-5, every cell 0, all P codes equal."""
    pts = _far_cluster(P, seed, 7, (-1000.0, -1000.0, -1000.0), 0.01)
    assert len(np.unique(morton_codes(pts))) == 1
    return _finish(pts, P)


def far_pair(P, seed):
    """Two 1e-3-wide clusters at +-(1000, 1000, 1000): 17 float32 values per axis and cluster, so many exact duplicates."""
    n = P // 2
    pts = np.concatenate([_far_cluster(n, seed, 8, (1000.0,) * 3, 1e-3), _far_cluster(P - n, seed, 9, (-1000.0,) * 3, 1e-3)])
    pts = pts[_rng(seed, 10).permutation(P)]
    hi = (pts > 0).all(1)
    assert ((pts < 0).all(1) | hi).all() and (P < 2 or (hi.any() and (~hi).any()))
    assert np.abs(np.abs(pts) - 1000).max() <= 0.5e-3 + 2 ** -14
    return _finish(pts, P)


def seam(P, seed):
    """The eight cube corners pin the bbox to [0, 1]^3; the other points come in pairs that face each other across one of the
    planes x, y, z = 0.5 (six pairs in ten across z, the top bit of the code), each 1e-4 .. 1e-3 from the plane and within
    2e-4 of each other along it, so a point's nearest neighbour is its partner on the other side of the octant split.  The
    x and y pairs lie below z = 0.49: they fill the lower half of the sorted array, which pushes the z partners of the
    first quadrant more than a box apart (tests/test_knn_ref64_cpu.py holds the cloud to that)."""
    assert P >= 8
    rng = _rng(seed, 11)
    n = P - 8
    corners = np.array([[i, j, k] for i in (0, 1) for j in (0, 1) for k in (0, 1)], np.float64)
    npair = (n + 1) // 2
    axis = rng.choice(3, size=npair, p=[0.2, 0.2, 0.6])
    base = 0.02 + 0.96 * rng.random((npair, 3))
    base[:, 2] *= 0.49                                   # the x and y pairs fill the lower half of the sorted array
    lo, hi = base.copy(), base + (rng.random((npair, 3)) - 0.5) * 4e-4
    rows = np.arange(npair)
    lo[rows, axis] = 0.5 - (1e-4 + 8e-4 * rng.random(npair))
    hi[rows, axis] = 0.5 + (1e-4 + 8e-4 * rng.random(npair))
    rest = np.stack([lo, hi], 1).reshape(-1, 3)[:n]
    pts = np.concatenate([corners, rest]).astype(np.float32)
    pts = pts[rng.permutation(P)]
    assert (pts.min(0) == 0).all() and (pts.max(0) == 1).all()
    off = pts.astype(np.float64) - 0.5
    inner = (np.abs(off) < 0.5).all(1)
    assert inner.sum() == n and (np.abs(off[inner]).min(1) <= 1e-3).all()
    for c in range(3 if n >= 64 else 0):
        near = inner & (np.abs(off[:, c]) <= 1e-3)
        assert (off[near, c] < 0).any() and (off[near, c] > 0).any()
    return _finish(pts, P)


def lattice(P, seed):
    """P distinct sites of an integer lattice, scaled by 2^-4: every d^2 is a multiple of 2^-8 below 2^24 * 2^-8, exact in
    float32, and most points have many neighbours at the same distance."""
    side = 2
    while side ** 3 < 2 * P:
        side += 1
    sites = _rng(seed, 12).permutation(side ** 3)[:P]
    ijk = np.stack([sites // (side * side), (sites // side) % side, sites % side], 1)
    pts = (ijk / 16.0).astype(np.float32)
    assert len(np.unique(sites)) == P and (pts * 16 == ijk).all() and 3 * side * side < 2 ** 24
    return _finish(pts, P)


def dupes_groups(P, seed):
    """{group size: [index arrays]} of dupes(P, seed): P // 100 (at least one) groups of each size 2, 3, 4, 5."""
    assert P >= 14
    g = max(1, P // 100)
    idx = _rng(seed, 13).permutation(P)[:14 * g]
    out, at = {}, 0
    for size in (2, 3, 4, 5):
        out[size] = [idx[at + k * size: at + (k + 1) * size] for k in range(g)]
        at += g * size
    return out


def dupes(P, seed):
    pts = cube(P, seed).numpy().copy()
    groups = dupes_groups(P, seed)
    merged = 0
    for size, members in groups.items():
        for m in members:
            pts[m] = pts[m[0]]
            assert len(m) == size and (pts[m] == pts[m[0]]).all()
            merged += size - 1
    assert len(np.unique(pts, axis=0)) == P - merged          # exact copies inside the groups and nowhere else
    return _finish(pts, P)


def same_origin(P, seed):
    pts = np.zeros((P, 3), np.float32)
    assert (pts == 0).all()
    return _finish(pts, P)


def same_offset(P, seed):
    pts = np.full((P, 3), 0.3, np.float32)
    assert (pts == np.float32(0.3)).all()
    return _finish(pts, P)


def colmap_like(P, seed):
    """Points along about 300 random 3D segments with 1e-3 noise, shifted by (20, -5, 8): a sparse reconstruction's shape."""
    rng = _rng(seed, 14)
    a = rng.uniform(-2, 2, (300, 3))
    b = a + rng.uniform(-1, 1, (300, 3))
    s = rng.integers(0, 300, P)
    t = rng.random((P, 1))
    pts = a[s] * (1 - t) + b[s] * t + rng.normal(0, 1e-3, (P, 3)) + np.array([20.0, -5.0, 8.0])
    pts = pts.astype(np.float32)
    assert pts[:, 0].min() > 16 and pts[:, 1].max() < 0 and pts[:, 2].min() > 4
    return _finish(pts, P)


BUILDERS = dict(cube=cube, plane_z0=plane_z0, plane_off=plane_off, line_x=line_x, negative=negative, far_tight=far_tight,
                far_tight_neg=far_tight_neg, far_pair=far_pair, seam=seam, lattice=lattice, dupes=dupes,
                same_origin=same_origin, same_offset=same_offset)
