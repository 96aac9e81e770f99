"""GPU: the three curve-fit kernels (csrc/curve_fit.hip) against their float64 restatement (curve_fit_ref64.py) on identical
float32 inputs, fit_curve_to_line / merge_curves with backend="gpu" against backend="host" on whole models, and the driver
with --topology_backend gpu.

Integer and boolean outputs must match exactly.  Real outputs must agree within 1e-8 absolute on unit-cube data: float64 eps
is 2.2e-16, the worst amplifier is the principal direction's 1 / (relative eigengap), bounded at 1e6 by the inputs (asserted),
which gives ~2e-10; 200-term sums and the Bernstein normal equations (condition ~1e3) give ~5e-11; 1e-8 leaves a factor ~50.
Control points are stored as float32 and compared with the float32 rounding of the restatement's value (1 ulp), up to the
reversal of the curve (the sign of a principal direction is free).  Every input keeps its thresholded quantities away from
the thresholds (asserted, never skipped): a threshold test cannot be compared across arithmetics on an input that sits on it."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import curve_fit_ref64 as R
from test_curve_fit_cpu import CHAIN_SEEDS, MARGIN
from test_train_driver_gpu import scan      # noqa: F401 -- the synthetic scan fixture of the driver tests
from util import S

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ATOL = 1e-8
EIGENGAP = 1e-6


def _dev(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV) if dtype is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


# ------------------------------------------------------------------------------------------------ cgs_curve_straightness
@pytest.mark.parametrize("sample_num", [100, 2, 37, 256])
def test_straightness_matches_ref64(sample_num):
    from curve_gaussian_amd.ops.curve_fit import curve_straightness
    planted = R.straightness_curves()
    rnd = S.make_curves(300, 24)["curve_points"].numpy()     # (seeds 21 and 22 put one curve within 1e-6 of a threshold)
    cp = np.concatenate([planted, rnd]).astype(np.float32)
    isb = np.ones(len(cp), bool)
    isb[3] = False
    isb[len(planted) + 5::7] = False                     # (the planted threshold rows stay Bezier curves)
    thr, thr_max = 0.002, 0.004
    ref_mean, ref_max, ref_straight, gap = R.curve_straightness(cp, isb, thr, thr_max, sample_num)
    coincident = len(planted) - 5                        # the row of coincident control points: no direction, distances 0
    assert ref_mean[coincident] < 1e-15 and ref_straight[coincident]
    rows = np.arange(len(cp)) != coincident
    assert gap[rows].min() >= EIGENGAP
    assert np.abs(ref_mean - thr).min() >= MARGIN and np.abs(ref_max - thr_max).min() >= MARGIN
    mean, mx, straight = curve_straightness(_dev(cp), _dev(isb), thr, thr_max, sample_num)
    mean, mx, straight = mean.cpu().numpy(), mx.cpu().numpy(), straight.cpu().numpy()
    print(f"sample_num {sample_num}: max |mean - ref| {np.abs(mean - ref_mean).max():.2e}, max |max - ref| "
          f"{np.abs(mx - ref_max).max():.2e}, smallest eigengap {gap[rows].min():.2e}, {int(straight.sum())} straight")
    assert np.isfinite(mean).all() and np.isfinite(mx).all()
    assert np.array_equal(straight, ref_straight)
    assert not straight[~isb].any()
    assert np.abs(mean - ref_mean).max() <= ATOL and np.abs(mx - ref_max).max() <= ATOL
    if sample_num == 100:                                # the planted curves: one just on each side of each threshold
        assert list(straight[len(planted) - 4:len(planted)]) == [True, False, False, False]
        assert ref_max[len(planted) - 4] < thr_max < ref_max[len(planted) - 3]
        # ... and of the mean threshold, with the maximum threshold out of the way
        m2, x2, s2 = (t.cpu().numpy() for t in curve_straightness(_dev(cp), _dev(isb), thr, 0.01, sample_num))
        assert list(s2[len(planted) - 4:len(planted)]) == [True, True, True, False]
        assert m2[len(planted) - 2] < thr < m2[len(planted) - 1] and x2[len(planted) - 1] < 0.01
        assert np.array_equal(s2, R.curve_straightness(cp, isb, thr, 0.01, sample_num)[2])
        assert straight[len(planted) - 6]                # exactly straight
    again = curve_straightness(_dev(cp), _dev(isb), thr, thr_max, sample_num)
    assert torch.equal(again[0].cpu(), torch.from_numpy(mean)) and torch.equal(again[1].cpu(), torch.from_numpy(mx))


def test_straightness_empty_and_argument_errors():
    from curve_gaussian_amd import _lib
    from curve_gaussian_amd.ops.curve_fit import curve_straightness
    out = curve_straightness(torch.zeros(0, 4, 3, device=DEV), torch.zeros(0, dtype=torch.bool, device=DEV), 0.002, 0.004)
    assert [tuple(o.shape) for o in out] == [(0,), (0,), (0,)]
    for n in (1, 257):
        with pytest.raises(_lib.CurveGSError, match="sample_num"):
            curve_straightness(torch.zeros(3, 4, 3, device=DEV), torch.ones(3, dtype=torch.bool, device=DEV), 0.002, 0.004, n)


# ------------------------------------------------------------------------------------------------ cgs_segment_merge_labels
def _labels(seg, dthr=0.02, sthr=0.97):
    from curve_gaussian_amd.ops.curve_fit import segment_merge_labels
    labels, ncomp = segment_merge_labels(_dev(seg), dthr, sthr)
    return labels.cpu().numpy(), ncomp


@pytest.mark.parametrize("seed", CHAIN_SEEDS)
def test_segment_labels_match_ref64(seed):
    seg = R.chain_segments(seed)
    seg = np.concatenate([seg, R.chain_segments(seed + 100, n_lines=3, pieces=4)]).astype(np.float32)   # n = 212: not a multiple of 64
    assert len(seg) % 64 != 0
    assert min(R.segment_margins(seg, 0.02, 0.97)) >= MARGIN
    ref, ref_n = R.segment_merge_labels(seg, 0.02, 0.97)
    got, got_n = _labels(seg)
    print(f"seed {seed}: n {len(seg)}, {ref_n} components, largest {np.bincount(ref).max()}")
    assert np.array_equal(got, ref) and got_n == ref_n
    assert 1 < ref_n < len(seg)
    assert np.array_equal(_labels(seg)[0], got)


def test_segment_labels_planted_cases():
    # n = 0 and n = 1
    assert _labels(np.zeros((0, 6), np.float32))[1] == 0
    lab, n = _labels(np.array([[0.1, 0.1, 0.1, 0.2, 0.1, 0.1]], np.float32))
    assert list(lab) == [0] and n == 1
    # a zero-length segment between two touching parallel ones joins nothing (on the host its similarity is 0)
    seg = np.array([[0.1, 0.5, 0.5, 0.3, 0.5, 0.5], [0.3, 0.5, 0.5, 0.3, 0.5, 0.5], [0.305, 0.5, 0.5, 0.5, 0.502, 0.5],
                    [0.8, 0.1, 0.2, 0.8, 0.3, 0.2]], np.float32)
    assert min(R.segment_margins(seg, 0.02, 0.97)) >= MARGIN
    ref, ref_n = R.segment_merge_labels(seg, 0.02, 0.97)
    assert list(ref) == [0, 1, 0, 3] and ref_n == 3
    lab, n = _labels(seg)
    assert list(lab) == [0, 1, 0, 3] and n == 3
    # all zero-length
    lab, n = _labels(np.tile(np.array([[0.2, 0.2, 0.2, 0.2, 0.2, 0.2]], np.float32), (70, 1)))
    assert np.array_equal(lab, np.arange(70)) and n == 70


@pytest.mark.parametrize("order", ["along", "shuffled"])
def test_segment_labels_chain_of_8192_is_one_component(order):
    """8192 segments end to end on one line, joined only to their neighbours (distance threshold far below a segment's
    length): one component whatever the numbering.  The restatement is compared on the first 512 of them (its dense n x n
    form does not fit at 8192); the full answer is known by construction."""
    n = 8192
    x = np.arange(n + 1, dtype=np.float64) / n * 0.8 + 0.1
    seg = np.stack([x[:-1], np.full(n, 0.5), np.full(n, 0.5), x[1:], np.full(n, 0.5), np.full(n, 0.5)], 1).astype(np.float32)
    if order == "shuffled":
        seg = seg[np.random.default_rng(5).permutation(n)]
    dthr = 1e-5                                           # neighbours touch (distance 0); the next one is 9.8e-5 away
    sub = seg[:512]
    assert min(R.segment_margins(sub, dthr, 0.97)) >= MARGIN
    ref, ref_n = R.segment_merge_labels(sub, dthr, 0.97)
    got, got_n = _labels(sub, dthr)
    assert np.array_equal(got, ref) and got_n == ref_n
    lab, ncomp = _labels(seg, dthr)
    assert ncomp == 1 and not lab.any()
    # one link cut: two components, the second labelled by its smallest member
    cut = seg.copy()
    k = 5000 if order == "along" else int(np.argmax(seg[:, 0] > 0.6))
    cut[k, 3:] = cut[k, :3]                               # segment k collapses to a point: it joins nothing
    lab, ncomp = _labels(cut, dthr)
    assert ncomp == 3 and lab[k] == k
    left = cut[:, 0] < cut[k, 0]
    left[k] = False
    right = ~left
    right[k] = False
    assert (lab[left] == np.nonzero(left)[0].min()).all() and (lab[right] == np.nonzero(right)[0].min()).all()


def test_segment_labels_above_the_limit_is_an_error():
    from curve_gaussian_amd import _lib
    from curve_gaussian_amd.ops.curve_fit import MAX_SEGMENTS, segment_merge_labels
    assert MAX_SEGMENTS >= 8192
    with pytest.raises(_lib.CurveGSError, match="invalid argument"):
        segment_merge_labels(torch.zeros(MAX_SEGMENTS + 1, 6, device=DEV), 0.02, 0.97)


# ------------------------------------------------------------------------------------------------ cgs_pair_consensus_fit
def _fit_inputs():
    """float32 [B,4,3] and pairs: the noisy bent pair, a cut cubic, two curves that are one point (no line), random pairs."""
    whole, halves = R.cut_cubic()
    rnd = S.make_curves(12, 31)["curve_points"].numpy()
    point = np.zeros((2, 4, 3), np.float32)     # every sample is exactly the origin: no two points at a non-zero distance
    cp = np.concatenate([R.noisy_bent_pair(), halves, point, rnd]).astype(np.float32)
    pairs = np.array([[0, 1], [2, 3], [4, 5], [3, 2], [6, 7], [8, 9], [10, 6], [1, 2]], np.int32)
    return cp, pairs


def _same_ctrl(got, ref64):
    """float32 control points against the float32 rounding of the reference's, within 1 ulp, in either direction."""
    def close(r):
        r32 = r.astype(np.float32)
        return bool((np.abs(got.astype(np.float64) - r32.astype(np.float64)) <= np.spacing(np.abs(r32)).astype(np.float64)).all())
    return close(ref64) or close(ref64[::-1])


def test_pair_consensus_fit_matches_ref64():
    from curve_gaussian_amd.ops.curve_fit import pair_consensus_fit
    cp, pairs = _fit_inputs()
    thr, err = 0.005, 0.02
    ref = R.pair_consensus_fit(cp, pairs, 100, thr, err)
    ctrl, rmse, inl, ok = (t.cpu().numpy() for t in pair_consensus_fit(_dev(cp), _dev(pairs), 100, thr, err))
    for k, r in enumerate(ref):
        print(f"pair {k} {tuple(pairs[k])}: inliers {inl[k]} (ref {r['inliers']}), rmse {rmse[k]:.3e} (ref {r['rmse']:.3e}), ok {ok[k]}, "
              f"count gap {r['count_gap']}, sum gap {r['sum_gap']}, eigengap {r['eigengap']}")
        assert R.winner_is_unique(r)
        assert inl[k] == r["inliers"] and bool(ok[k]) == r["ok"]
        if r["winner"] is None:
            assert not ok[k] and rmse[k] == 0 and not ctrl[k].any()
            continue
        assert r["eigengap"] >= EIGENGAP and r["residual_margin"] >= 1e-12 and abs(r["rmse"] - err) >= MARGIN
        assert abs(rmse[k] - r["rmse"]) <= ATOL
        assert _same_ctrl(ctrl[k], r["ctrl"]), (ctrl[k], r["ctrl"])
        if ok[k]:
            assert rmse[k] <= err
    assert not ok[2] and inl[2] < 2                       # coincident points: no two-point line at all
    assert ok[1] and ok[3] and rmse[1] < 2e-3             # the cut cubic comes back as one curve, in either order
    assert inl[0] < 200                                   # the noisy pair is not all inliers: the consensus had to choose
    again = pair_consensus_fit(_dev(cp), _dev(pairs), 100, thr, err)
    assert torch.equal(again[0].cpu(), torch.from_numpy(ctrl)) and torch.equal(again[1].cpu(), torch.from_numpy(rmse))


def test_pair_consensus_fit_other_sizes():
    from curve_gaussian_amd import _lib
    from curve_gaussian_amd.ops.curve_fit import pair_consensus_fit
    cp, pairs = _fit_inputs()
    out = pair_consensus_fit(_dev(cp), torch.zeros(0, 2, dtype=torch.int32, device=DEV))            # K = 0
    assert [tuple(o.shape) for o in out] == [(0, 4, 3), (0,), (0,), (0,)]
    for n in (7, 256):
        ref = R.pair_consensus_fit(cp, pairs[:2], n, 0.005, 0.02)
        ctrl, rmse, inl, ok = (t.cpu().numpy() for t in pair_consensus_fit(_dev(cp), _dev(pairs[:2]), n, 0.005, 0.02))
        for k, r in enumerate(ref):
            assert R.winner_is_unique(r) and r["eigengap"] >= EIGENGAP
            assert inl[k] == r["inliers"] and bool(ok[k]) == r["ok"] and abs(rmse[k] - r["rmse"]) <= ATOL
            assert _same_ctrl(ctrl[k], r["ctrl"])
    with pytest.raises(_lib.CurveGSError, match="index curves"):
        pair_consensus_fit(_dev(cp), torch.tensor([[0, len(cp)]], dtype=torch.int32, device=DEV))
    with pytest.raises(_lib.CurveGSError, match="sample_num"):
        pair_consensus_fit(_dev(cp), _dev(pairs), 257)


# ------------------------------------------------------------------------------------------------ whole models
def _clone_model(cp, width, opac, isb):
    from curve_gaussian_amd.scene import GaussianCurveModel
    B = cp.shape[0]
    return GaussianCurveModel(0, 12, device=DEV).create_from_curves(cp.clone(), width.clone(), opac.clone(), torch.ones(B, 12, 1),
                                                                  isb.clone())


def _same_curves(a, b, atol=1e-4, fit_tol=0.02):
    """Two models hold the same curves in the same order: equal flags; segments: their two end points within atol, in either
    order; Bezier curves: control points within atol, or -- a pair refitted along two different consensus lines (random
    trials on the host, exhaustive search on the GPU) -- the same curve within the fit's own error bound, in either direction."""
    assert torch.equal(a.is_bezier, b.is_bezier)
    pa, pb = a._curve_points.detach().cpu().numpy(), b._curve_points.detach().cpu().numpy()
    assert pa.shape == pb.shape
    isb = a.is_bezier.cpu().numpy()
    A = R.bernstein(np.linspace(0, 1, 50))
    for k in range(len(pa)):
        if not isb[k]:
            x, y = pa[k][[0, 3]], pb[k][[0, 3]]
            d = min(np.abs(x - y).max(), np.abs(x - y[::-1]).max())
            assert d <= atol, (k, d)
        elif np.abs(pa[k] - pb[k]).max() > atol:
            x, y = A @ pa[k].astype(np.float64), A @ pb[k].astype(np.float64)
            far = lambda p, q: np.linalg.norm(p[:, None] - q[None], axis=2).min(axis=1).max()
            assert max(far(x, y), far(y, x)) <= fit_tol, k
    for name in ("_opacity", "_width"):
        torch.testing.assert_close(getattr(a, name).detach(), getattr(b, name).detach(), rtol=0, atol=1e-6)


def _run_both(build, steps=0):
    """fit_curve_to_line + merge_curves on two copies of a model, one per back end -> {backend: (model, n_fitted, removed)}."""
    out = {}
    for backend in ("host", "gpu"):
        gm = build()
        if steps:
            from curve_gaussian_amd.gaussian_renderer import PipelineParams, render
            from curve_gaussian_amd.train_step import TrainStep
            cam = S.make_camera((0.5, -1.7, 0.9), (0.5, 0.5, 0.5), (0, 0, 1), 64, 96).to(DEV)
            gt = render(cam, gm, PipelineParams(), torch.zeros(3, device=DEV))["render"].detach()
            ts = TrainStep(gm, [cam], [gt], seed=1)
            for _ in range(steps):
                ts.step()
            assert float(gm.optimizer.state_of("curve_points")[0].abs().max()) > 0
        B0 = gm._curve_points.shape[0]
        n = gm.fit_curve_to_line(0.002, 0.004, backend=backend)
        if steps:
            assert float(gm.optimizer.state_of("curve_points")[0].abs().max()) == 0.0      # replace_tensor_to_optimizer
        removed = gm.merge_curves(0.02, 0.97, backend=backend)
        B1 = gm._curve_points.shape[0]
        assert gm.is_bezier.shape[0] == B1 == gm._opacity.shape[0] == gm._mask.shape[0] == gm._width.shape[0]
        if steps:
            k = B1 - (B0 - removed)                       # the appended curves: their Adam moments start at zero
            assert k > 0
            for grp in ("curve_points", "opacity", "width"):
                m, v = gm.optimizer.state_of(grp)
                assert m.shape[0] == B1 and float(m[-k:].abs().max()) == 0.0 and float(v[-k:].abs().max()) == 0.0
            assert np.isfinite(float(ts.step()[0]))       # still trains
        out[backend] = (gm, n, removed)
    return out


def test_line_merge_scenario_gives_the_same_model_on_both_back_ends():
    """tests/test_topology_gpu.py's model of 30 bent curves, 6 straight ones and a cubic cut in two, after three training steps."""
    from test_topology_gpu import _line_merge_model
    out = _run_both(lambda: _line_merge_model()[0], steps=3)
    (gh, nh, rh), (gg, ng, rg) = out["host"], out["gpu"]
    cp = _line_merge_model()[0]._curve_points.detach().cpu().numpy()
    mean_d, max_d, _s, _g = R.curve_straightness(cp, np.ones(len(cp), bool), 0.002, 0.004)
    assert np.abs(mean_d - 0.002).min() >= MARGIN and np.abs(max_d - 0.004).min() >= MARGIN
    print(f"fitted {nh} / {ng}, removed {rh} / {rg}, curves left {gh._curve_points.shape[0]}")
    assert nh == ng and 6 <= ng <= 8 and rh == rg and rg >= 2
    _same_curves(gh, gg)
    assert int(gg.is_bezier.sum()) == int(gh.is_bezier.sum())


def test_touching_segments_scenario_gives_the_same_model_on_both_back_ends():
    """tests/test_topology_gpu.py::test_merge_curves_fuses_touching_parallel_segments, on both back ends."""
    c = S.make_curves(12, 13)
    seg = torch.zeros(3, 4, 3)
    seg[0, 0], seg[0, 3] = torch.tensor([0.1, 0.5, 0.5]), torch.tensor([0.3, 0.5, 0.5])
    seg[1, 0], seg[1, 3] = torch.tensor([0.305, 0.5, 0.5]), torch.tensor([0.5, 0.502, 0.5])
    seg[2, 0], seg[2, 3] = torch.tensor([0.8, 0.1, 0.2]), torch.tensor([0.8, 0.3, 0.2])       # far away: stays
    for k in range(3):
        seg[k, 1] = seg[k, 0] + (seg[k, 3] - seg[k, 0]) / 3
        seg[k, 2] = seg[k, 0] + (seg[k, 3] - seg[k, 0]) * 2 / 3
    cp = torch.cat([c["curve_points"], seg])
    isb = torch.cat([torch.ones(12, dtype=torch.bool), torch.zeros(3, dtype=torch.bool)])
    assert min(R.segment_margins(seg[:, [0, 3]].reshape(3, 6).numpy(), 0.02, 0.97)) >= MARGIN
    res = {}
    for backend in ("host", "gpu"):
        gm = _clone_model(cp, torch.cat([c["width"], c["width"][:3]]), torch.cat([c["opacity"], c["opacity"][:3]]), isb)
        res[backend] = (gm, gm.merge_curves(0.02, 0.97, backend=backend))
    assert res["host"][1] == res["gpu"][1] >= 2
    _same_curves(res["host"][0], res["gpu"][0])
    lines = res["gpu"][0]._curve_points.detach()[~res["gpu"][0].is_bezier]
    assert lines.shape[0] == 2 and float((lines[:, 0] - lines[:, 3]).norm(dim=-1).max()) > 0.39


def test_large_model_gives_the_same_model_on_both_back_ends():
    """1000 straight segments (200 lines in 5 pieces) and 100 cubics cut in two: the same `removed`, the same flags, the same
    partition (the merged segments and curves agree one by one within 1e-4), and the fit of every pair equals the restatement's."""
    from curve_gaussian_amd.ops.curve_fit import pair_consensus_fit
    from curve_gaussian_amd.scene import topology as T
    cp, isb = R.large_model()
    n_lines, n_bez = int((~isb).sum()), int(isb.sum())
    assert n_lines >= 1000 and n_bez >= 200
    # the margins of this input, under the restatement's arithmetic and the host's
    seg = cp[~isb][:, [0, 3]].reshape(-1, 6)
    md, ms = R.segment_margins(seg, 0.02, 0.97)
    sim = np.abs(T._pairwise_cosine_similarity(seg)).astype(np.float64)
    off = ~np.eye(len(seg), dtype=bool)
    mean_d, max_d, straight, gap = R.curve_straightness(cp, isb, 0.002, 0.004)
    print(f"large model: segment margins dist {md:.2e} cos {ms:.2e} (host cos {np.abs(sim[off] - 0.97).min():.2e}); straightness "
          f"margins {np.abs(mean_d - 0.002).min():.2e} {np.abs(max_d - 0.004).min():.2e}")
    assert min(md, ms, np.abs(sim[off] - 0.97).min()) >= MARGIN
    assert np.abs(mean_d - 0.002).min() >= MARGIN and np.abs(max_d - 0.004).min() >= MARGIN and not straight.any()
    g = torch.Generator().manual_seed(3)
    width, opac = torch.rand(len(cp), 1, generator=g) + 0.5, torch.randn(len(cp), 1, generator=g)
    out = _run_both(lambda: _clone_model(torch.from_numpy(cp), width, opac, torch.from_numpy(isb)))
    (gh, nh, rh), (gg, ng, rg) = out["host"], out["gpu"]
    ref_labels, ref_ncomp = R.segment_merge_labels(seg, 0.02, 0.97)
    merged_lines = int((np.bincount(ref_labels)[ref_labels] > 1).sum())
    print(f"large model: fitted {nh} / {ng}, removed {rh} / {rg}, {ref_ncomp} line components, {merged_lines} lines merged")
    assert nh == ng == 0 and rh == rg == merged_lines + n_bez
    _same_curves(gh, gg)
    assert int(gg.is_bezier.sum()) == n_bez // 2 and int((~gg.is_bezier).sum()) == ref_ncomp
    # the pairs themselves: halves 2k, 2k + 1 of the Bezier rows
    bez = np.nonzero(isb)[0]
    pairs = bez.reshape(-1, 2).astype(np.int32)
    ctrl, rmse, inl, ok = (t.cpu().numpy() for t in pair_consensus_fit(_dev(cp), _dev(pairs), 100, 0.005, 0.02))
    assert ok.all() and (rmse <= 0.02).all()
    for k in range(0, len(pairs), 10):                    # every tenth against the restatement (0.5 s each on the host)
        r = R.pair_consensus_fit(cp, pairs[k:k + 1], 100, 0.005, 0.02)[0]
        assert R.winner_is_unique(r) and r["eigengap"] >= EIGENGAP
        assert inl[k] == r["inliers"] and r["ok"] and abs(rmse[k] - r["rmse"]) <= ATOL and _same_ctrl(ctrl[k], r["ctrl"])


# ------------------------------------------------------------------------------------------------ driver
def test_driver_runs_with_the_gpu_topology_backend(scan, tmp_path):
    from curve_gaussian_amd import train as T
    out = tmp_path / "cli"
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-m", "curve_gaussian_amd.train", "-s", scan[0], "-m", str(out), "--iterations", "600",
                        "--test_iterations", "600", "--checkpoint_iterations", "600", "--quiet", "--topology_backend", "gpu"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    edges = json.load(open(out / "parametric_edges.json"))
    assert set(edges) == {"lines_end_pts", "curves_ctl_pts"}
    # the same sequence of events as the host back end, on a schedule short enough to reach the merge iterations
    opt = dict(iterations=2000, densify_from_iter=100, densification_interval=200, densify_until_iter=600, opacity_reset_interval=500)
    events = {}
    for backend in ("host", "gpu"):
        d = T.ModelParams(source_path=scan[0], model_path=str(tmp_path / backend))
        res = T.training(d, T.OptimizationParams(**opt), [2000], [2000], [], None, backend="direct", quiet=True, device=DEV,
                         topology_backend=backend)
        events[backend] = [(it, ev) for it, ev, _n in res["events"]]
        assert os.path.exists(os.path.join(d.model_path, "parametric_edges.json"))
    assert events["gpu"] == events["host"]
    assert [e for _it, e in events["gpu"]].count("merge_curves") == 2 and (1000, "fit_curve_to_line") in events["gpu"]
