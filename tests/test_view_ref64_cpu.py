"""CPU: the truth the fused view kernels are compared with element-wise (tests/view_ref64.py) and the scenes they are compared
on (tests/test_view_shapes_gpu.py).

A comparison with NO outlier budget is only honest where the truth itself has no decision that a last-bit difference can take
the other way.  Every scene of the GPU test is held to that here, on the oracle alone:

* the oracle run as is, with every splat opacity scaled by 1 + 4e-6 and by 1 - 4e-6 (twice the 2e-6 by which the HIP
  compositor's exponent differs from the oracle's, tests/util.py::near_threshold_pairs) gives identical radii, identical
  per-pixel contributor counts and identical last-contributor positions: no alpha >= 1/255 and no T < 1e-4 decision flips;
* no pixel comes near termination at all: final T > 1e-2 everywhere, and with alpha <= 0.99 a T (1 - alpha) < 1e-4 test then
  cannot fire;
* no visible splat's 3 sigma extent lies within 2e-4 (relative) of the integer its radius is rounded up to -- twice the 1e-4
  to which test_sampling_gpu.py holds the HIP sampling kernels' `scaling` to torch's;
* no mask logit's sigmoid lies within 1e-4 of the threshold.

The seeds are those of view_ref64.SHAPE_SEEDS / CULL_SEEDS / LARGE_SEED (chosen by running this test: a seed that fails is
replaced there, nothing is loosened here or on the GPU):

    1 x 5: 11    1 x 32: 12    22 x 12: 33    43 x 12: 34    9 x 32: 25    33 x 8: 16    65 x 4: 87    25 x 32: 48
    culling camera  22 x 12: 23    9 x 32: 45        large scenes (43 690 / 43 691 x 12): 41

And view_ref64 at m = 12 is pinned to the frozen chain: it reproduces tests/golden/view_{small,lines,masked}.npz under the
bounds of tests/test_view_golden_cpu.py."""
import numpy as np
import pytest
import torch

import view_ref64 as V
from make_view_golden import load_scene

SEEDS_STATED = {(1, 5): 11, (1, 32): 12, (22, 12): 33, (43, 12): 34, (9, 32): 25, (33, 8): 16, (65, 4): 87, (25, 32): 48}
CULL_SEEDS_STATED = {(22, 12): 23, (9, 32): 45}

CASES = [pytest.param(B, m, seed, "", id=f"{B}x{m}") for (B, m), seed in V.SHAPE_SEEDS.items()]
CASES += [pytest.param(B, m, seed, "cull", id=f"{B}x{m}-cull") for (B, m), seed in V.CULL_SEEDS.items()]
# the second view of the shared-sampling batches (same curves as the first, from view_ref64.SECOND_EYE)
CASES += [pytest.param(B, m, V.SHAPE_SEEDS[B, m], "second", id=f"{B}x{m}-second") for B, m in V.CULL_SEEDS]


def test_the_seeds_are_the_stated_ones():
    assert V.SHAPE_SEEDS == SEEDS_STATED and V.CULL_SEEDS == CULL_SEEDS_STATED and V.LARGE_SEED == 41
    assert V.LARGE_B[0] * V.LARGE_M < 512 * 1024 <= V.LARGE_B[1] * V.LARGE_M      # on either side of the launcher's threshold


def _no_decision_edge(curves, mask, cam, dimg, m):
    base = V.view_ref64(curves, mask, V.MASK_THR, cam, 0.0, dimg, m, decisions=True)
    for scale in (1.0 + 4e-6, 1.0 - 4e-6):
        other = V.view_ref64(curves, mask, V.MASK_THR, cam, 0.0, dimg, m, decisions=True, opac_scale=scale)
        for k in ("radii", "n_blended", "n_contrib"):
            assert np.array_equal(base[k], other[k]), f"{k} changes when every opacity is scaled by {scale!r}"
    assert base["near_pairs"] == 0
    assert base["final_T"].min() > 1e-2, f"a pixel's transmittance falls to {base['final_T'].min():.2e}"
    assert base["radius_margin"] > 2e-4, f"a radius is rounded from within {base['radius_margin']:.1e} of an integer"
    assert (base["radii"] > 0).any() and base["n_blended"].max() >= 2
    if mask is not None:
        assert float((torch.sigmoid(mask.double()) - V.MASK_THR).abs().min()) > 1e-4
    return base


@pytest.mark.parametrize("use_mask", [False, True])
@pytest.mark.parametrize("B,m,seed,view", CASES)
def test_scene_sits_on_no_decision_edge(B, m, seed, view, use_mask):
    curves, mask, cam, dimg = V.scene(B, m, seed, cull=view == "cull", second=view == "second")
    assert B == 1 or 0 < int(curves["is_bezier"].sum()) < B                       # mixed curve types
    base = _no_decision_edge(curves, mask if use_mask else None, cam, dimg, m)
    if use_mask:
        on = torch.sigmoid(mask) > V.MASK_THR
        assert 0 < int(on.sum()) < on.numel() and np.abs(base["g_mask"]).max() > 0
    if view == "cull":
        # some curves keep only part of their samples (radii == 0 inside a reduced curve), some none at all (they get their
        # gradient through the two grid-wide norm sums alone)
        vis = (base["radii"].reshape(B, m) > 0).sum(1)
        assert V.partly_culled(base["radii"], B, m).sum() >= 2 and (vis == 0).any() and (vis == m).any()
        gone = vis == 0
        assert np.abs(base["g_curve_points"][gone]).max() > 0
    elif view == "":
        assert (base["radii"] > 0).all()


@pytest.mark.parametrize("B", V.LARGE_B)
def test_large_scene_sits_on_no_decision_edge(B):
    curves, mask, cam, dimg = V.large_scene(B)
    base = _no_decision_edge(curves, mask, cam, dimg, V.LARGE_M)
    nv = V.LARGE_VISIBLE * V.LARGE_M
    assert (base["radii"][:nv] > 0).all() and (base["radii"][nv:] == 0).all()
    assert np.abs(base["g_curve_points"][V.LARGE_VISIBLE:]).max() > 0               # reached through the norm sums


def _tight(name, got, ref, rel=1e-6):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, name
    tol = rel * max(np.abs(ref).max(), 1e-30)
    assert np.abs(got - ref).max() <= tol, f"{name}: {np.abs(got - ref).max():.3e} from the frozen output (tol {tol:.1e})"


@pytest.mark.parametrize("name", ["small", "lines", "masked"])
def test_view_ref64_reproduces_the_frozen_chain_at_m_12(name):
    """Bounds of tests/test_view_golden_cpu.py: 1e-6 of the maximum on the compositor's outputs, 1e-5 on the pulled-back
    gradients (there: another summation order; here: the pull-back in float64 instead of float32)."""
    curves, mask, cam, bg, z = load_scene(name)
    res = V.view_ref64(curves, mask, float(z["mask_thr"][0]), cam, bg, z["dL_dcolor"], 12)
    assert np.array_equal(res["radii"], z["radii"]) and int(res["num_rendered"][0]) == int(z["num_rendered"][0])
    for k in ("color", "invdepth", "out_all_map", "final_T", "g_means2D"):
        _tight(k, res[k], z[k])
    for k in ("g_curve_points", "g_width", "g_opacity") + (("g_mask",) if mask is not None else ()):
        _tight(k, res[k], z[k], rel=1e-5)
