"""The float64 3-NN reference and the hard clouds of tests/knn_ref64.py, checked on the CPU: the reference against exact
rational arithmetic and against the brute-force oracle where that oracle is accurate, the float32 tail for P < 4, the
kernel's Morton key restated in numpy, and the claim the seam cloud exists for.  Without these the GPU module
(tests/test_knn_ref64_gpu.py) would compare the kernels with one more restatement that nothing vouches for."""
from fractions import Fraction

import numpy as np
import pytest
import torch

import knn_ref64 as K
from oracle import torch_ref as TR


def _exact_mean_dist2(pts):
    """Triple loop in exact rational arithmetic: points, the other points, the three coordinates."""
    rows = [[Fraction(float(v)) for v in p] for p in pts.tolist()]
    out = []
    for i, a in enumerate(rows):
        d2 = []
        for j, b in enumerate(rows):
            if j == i:
                continue
            s = Fraction(0)
            for c in range(3):
                s += (a[c] - b[c]) ** 2
            d2.append(s)
        d2.sort()
        out.append((d2[0] + d2[1] + d2[2]) / 3)
    return out


@pytest.mark.parametrize("name", sorted(K.BUILDERS))
@pytest.mark.parametrize("P", [14, 27, 40])
def test_ref64_matches_exact_arithmetic(name, P):
    pts = K.BUILDERS[name](P, 7)
    assert pts.dtype == torch.float32 and tuple(pts.shape) == (P, 3)
    assert torch.equal(pts, K.BUILDERS[name](P, 7))                       # deterministic
    ref = K.mean_dist2_ref64(pts)
    assert ref.dtype == torch.float64 and ref.device.type == "cpu"
    assert torch.equal(ref, K.mean_dist2_ref64(pts, chunk=5))             # the row chunks do not show
    for got, want in zip(ref.tolist(), _exact_mean_dist2(pts)):
        # exact differences, then 3 squarings, 2 + 2 adds and a division: below 8 * 2^-53 relative, nothing cancels
        assert abs(Fraction(got) - want) <= want * Fraction(1, 10 ** 15)


def test_builders_hold_at_the_gpu_sizes():
    """Every builder's own assertions at the sizes the GPU module uses, and duplicate groups where they are meant to be."""
    for name, build in K.BUILDERS.items():
        for P in (1025, 2049):
            assert tuple(build(P, 0).shape) == (P, 3), name
    for P in (4097,):
        for name in ("seam", "far_tight", "far_tight_neg"):
            K.BUILDERS[name](P, 0)
    assert len(np.unique(K.morton_codes(K.far_tight_neg(2049, 0)))) == 1
    assert len(np.unique(K.morton_codes(K.far_tight(2049, 0)))) <= 4      # cells (1022|1023, 0, 1022|1023)
    assert len(np.unique(K.morton_codes(K.same_origin(1025, 0)))) == 1
    assert len(np.unique(K.morton_cells(K.plane_z0(1025, 0))[:, 2])) == 1
    assert K.morton_cells(K.negative(1025, 0)).max() < 1023               # maxx = 0 is no point of the cloud
    g = K.dupes_groups(2049, 0)
    assert [len(g[s]) for s in (2, 3, 4, 5)] == [20] * 4
    K.colmap_like(70001, 0)


def test_morton_restatement_on_known_cells():
    pts = np.array([[0, 0, 0], [1, 1, 1], [1, 0, 0], [0, 1, 0], [0, 0, 1], [0.5, 0.25, 0.75]], np.float32)
    cells = K.morton_cells(pts)
    assert cells.tolist() == [[0, 0, 0], [1023, 1023, 1023], [1023, 0, 0], [0, 1023, 0], [0, 0, 1023], [511, 255, 767]]
    code = K.morton_codes(pts)
    assert code[1] == (1 << 30) - 1 and code[2] == 0x09249249 and code[3] == 0x09249249 << 1 and code[4] == 0x09249249 << 2
    assert K.morton_order(pts).tolist() == [0, 2, 3, 5, 4, 1]           # z is the top bit of every level, then y, then x
    assert K.morton_order(np.zeros((5, 3), np.float32)).tolist() == [0, 1, 2, 3, 4]     # equal codes: by index


def _grid15():
    lin = torch.linspace(-0.05, 1.05, 15)
    return torch.stack(torch.meshgrid(lin, lin, lin, indexing="ij"), -1).reshape(-1, 3)


@pytest.mark.parametrize("cloud", ["cube", "grid15"])
def test_ref64_agrees_with_the_brute_force_oracle_on_easy_clouds(cloud):
    pts = K.cube(1500, 3) if cloud == "cube" else _grid15()
    ref = K.mean_dist2_ref64(pts)
    tr = TR.knn_mean_dist2_f64(pts)
    assert float(((tr - ref).abs() / ref).max()) <= 1e-9
    assert torch.equal(TR.knn_mean_dist2(pts), tr.float())


def test_cdist_oracle_error_on_far_tight_is_recorded(capsys):
    """Why the new reference exists: the figure is printed, not asserted (it is the OTHER oracle's error)."""
    for name in ("far_tight", "far_pair"):
        pts = K.BUILDERS[name](1025, 0)
        ref = K.mean_dist2_ref64(pts)
        tr = TR.knn_mean_dist2_f64(pts)
        nz = ref > 0
        rel = float(((tr - ref).abs()[nz] / ref[nz]).max())
        with capsys.disabled():
            print(f"\n{name} P=1025: cdist oracle vs explicit differences, worst relative error {rel:.3e}; "
                  f"worst absolute where the truth is 0: {float(tr[~nz].abs().max()) if (~nz).any() else 0.0:.3e}")


def test_seam_true_neighbours_are_far_in_morton_order():
    P = 2049
    pts = K.seam(P, 0)
    order = K.morton_order(pts.numpy())
    pos = np.empty(P, np.int64)
    pos[order] = np.arange(P)
    a = pts.double()
    d2 = ((a[:, None, :] - a[None]) ** 2).sum(-1)
    d2.fill_diagonal_(float("inf"))
    nn = d2.argmin(1).numpy()
    gap = np.abs(pos - pos[nn])
    far = float((gap > K.KNN_BOX).mean())
    other_box = float((pos // K.KNN_BOX != pos[nn] // K.KNN_BOX).mean())
    print(f"seam P={P}: nearest neighbour more than {K.KNN_BOX} sorted positions away for {far:.3f} of the points, "
          f"in another box for {other_box:.3f}")
    assert far >= 0.1


def test_small_p_float32_tail():
    third = np.float32(K.FLT_MAX) / np.float32(3.0)
    for P in (1, 2):
        out = K.mean_dist2_fp32_small_p(K.cube(P, 1).numpy())
        assert out.dtype == np.float32 and out.shape == (P,) and np.isposinf(out).all()
    out = K.mean_dist2_fp32_small_p(K.cube(3, 2).numpy())
    assert out.view(np.uint32).tolist() == [third.view(np.uint32)] * 3
    assert third.view(np.uint32) == 0x7EAAAAAA                              # FLT_MAX / 3, rounded to nearest
    with pytest.raises(ValueError):
        K.mean_dist2_ref64(K.cube(3, 2))
