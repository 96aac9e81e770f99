"""CPU: the float64 restatement of the curve-fit kernels (curve_fit_ref64.py) against the host code of scene/topology.py that
the kernels stand in for, on inputs that keep every thresholded quantity at least 1e-6 away from its threshold under the
host's float32 arithmetic (asserted, never skipped); the argument checks of the three C entry points without a GPU; the
driver's --topology_backend flag; the backend keyword."""
import ctypes

import numpy as np
import pytest
import torch

import curve_fit_ref64 as R
CS = R          # the seeded inputs live next to the restatement

MARGIN = 1e-6
# chain_segments seeds whose 19 900 pairs all keep the margin (of seeds 0 .. 7, seeds 0 and 2 put one pair within 1e-6 of a
# threshold: those are not inputs a threshold test can be compared on; the tests assert the margin of the seeds they use)
CHAIN_SEEDS = [1, 3, 4, 6]


# ------------------------------------------------------------------------------------------------ ref64 vs host helpers
@pytest.mark.parametrize("seed", CHAIN_SEEDS)
def test_ref64_labels_equal_scipy_components_of_the_host_predicate(seed):
    from scipy.sparse.csgraph import connected_components
    from curve_gaussian_amd.scene import topology as T
    seg = CS.chain_segments(seed)
    dthr, sthr = 0.02, 0.97
    dmat = T._pairwise_segment_distances(seg)
    sim = np.abs(T._pairwise_cosine_similarity(seg))
    off = ~np.eye(len(seg), dtype=bool)
    gap_d, gap_s = np.abs(dmat[off] - dthr).min(), np.abs(sim[off] - sthr).min()
    ref_d, ref_s = R.segment_margins(seg, dthr, sthr)
    print(f"seed {seed}: host margins dist {gap_d:.2e} cos {gap_s:.2e}; ref64 margins dist {ref_d:.2e} cos {ref_s:.2e}")
    assert min(gap_d, gap_s, ref_d, ref_s) >= MARGIN
    adj = (dmat <= dthr) & (sim >= sthr)
    _n, lab = connected_components(adj)
    canon = np.array([np.nonzero(lab == l)[0].min() for l in lab])
    labels, ncomp = R.segment_merge_labels(seg, dthr, sthr)
    assert np.array_equal(labels, canon) and ncomp == _n
    assert 50 <= int(np.triu(adj, 1).sum()) <= 200       # a real graph: neither empty nor complete


def _host_straightness(samples32, thr, thr_max):
    """is_curve_straight's mean and maximum distance, with its own float32 arithmetic."""
    from curve_gaussian_amd.scene import topology as T
    _s, _e, direction, mean_point, t_min, t_max = T.fit_straight_line(samples32)
    t = np.dot(samples32 - mean_point, direction)
    d = np.linalg.norm(samples32 - (mean_point + np.clip(t, t_min, t_max).reshape(-1, 1) * direction), axis=1)
    return float(np.mean(d)), float(d.max())


def test_ref64_straight_flags_equal_is_curve_straight():
    from curve_gaussian_amd.scene import topology as T
    cp = CS.straightness_curves()
    thr, thr_max = 0.002, 0.004
    t = torch.linspace(0, 1, 100)[:, None, None]
    c = torch.from_numpy(cp)
    samples = ((1 - t) ** 3 * c[:, 0] + 3 * (1 - t) ** 2 * t * c[:, 1] + 3 * (1 - t) * t ** 2 * c[:, 2]
               + t ** 3 * c[:, 3]).permute(1, 0, 2).contiguous()
    mean_d, max_d, straight, _gap = R.curve_straightness(cp, np.ones(len(cp), bool), thr, thr_max)
    host = np.zeros(len(cp), bool)
    for b in range(len(cp)):
        hm, hx = _host_straightness(samples[b].numpy(), thr, thr_max)
        assert min(abs(hm - thr), abs(hx - thr_max), abs(mean_d[b] - thr), abs(max_d[b] - thr_max)) >= MARGIN, b
        host[b] = T.is_curve_straight(None, samples[b], thr, thr_max)[0]
    assert np.array_equal(straight, host)
    assert 0 < int(host.sum()) < len(cp)                  # both outcomes occur
    # rows that are not Bezier curves are never selected (the host loop skips them)
    assert not R.curve_straightness(cp, np.zeros(len(cp), bool), thr, thr_max)[2].any()


class _RecordingRng:
    def __init__(self, seed):
        self.rng, self.drawn = np.random.default_rng(seed), []

    def choice(self, *a, **k):
        out = self.rng.choice(*a, **k)
        self.drawn.append(tuple(int(v) for v in out))
        return out


@pytest.mark.parametrize("seed", [0, 1, 2, 3, 4])
def test_ref64_consensus_is_at_least_the_sampled_line(seed):
    """The exhaustive winner has at least as many inliers as the line _ransac_line's random trials settle on."""
    from curve_gaussian_amd.scene import topology as T
    pts64 = R.sample_curves(CS.noisy_bent_pair(), 100).reshape(-1, 3)
    pts32 = pts64.astype(np.float32)
    thr = 0.005
    rng = _RecordingRng(seed)
    mask = T._ransac_line(pts32, thr, 1000, rng)
    # which trial won, by the host's own rule and arithmetic
    best, best_count, best_res, best_mask = None, 0, np.inf, None
    for i, j in rng.drawn:
        d = pts32[j] - pts32[i]
        d = d / np.linalg.norm(d)
        r = pts32 - pts32[i]
        res = np.linalg.norm(r - np.outer(r @ d, d), axis=1)
        cnt, rs = int((res < thr).sum()), float((res ** 2).sum())
        if cnt > best_count or (cnt == best_count and rs < best_res):
            best, best_count, best_res, best_mask = (i, j), cnt, rs, res < thr
    assert np.array_equal(best_mask, mask)               # the replay found the line the mask belongs to
    res64 = R.line_residuals(pts64, *best)               # that line, re-evaluated in float64
    out = R.pair_consensus_fit_one(pts64, thr, 0.02)
    print(f"seed {seed}: sampled line {best} has {int(mask.sum())} inliers, exhaustive winner {out['winner']} has {out['inliers']}")
    assert R.winner_is_unique(out) and out["residual_margin"] >= MARGIN
    assert out["inliers"] >= int((res64 < thr).sum())


def test_ref64_fit_reproduces_a_cut_cubic():
    """The two halves of one cubic are exact pieces of it: the fit returns the whole curve (up to its direction)."""
    whole, halves = CS.cut_cubic()
    out = R.pair_consensus_fit(halves, [[0, 1]])[0]
    assert out["ok"] and out["rmse"] < 2e-3
    err = min(np.abs(out["ctrl"] - whole).max(), np.abs(out["ctrl"][::-1] - whole).max())
    assert err < 2e-2          # (the samples are uniform in each half's parameter, not in the whole curve's: not exact)


# ------------------------------------------------------------------------------------------------ C ABI without a GPU
def test_invalid_arguments_are_rejected_without_a_gpu():
    from curve_gaussian_amd import _lib
    lib = _lib.load()
    d = ctypes.c_double
    one = ctypes.c_void_p(16)        # never dereferenced: every call below is rejected (or a no-op) before any GPU work

    def bad(rc):
        return rc == -1 and b"invalid argument" in lib.cgs_last_error()
    # cgs_curve_straightness
    assert bad(lib.cgs_curve_straightness(-1, one, one, 100, d(0.002), d(0.004), one, one, one, None))
    assert bad(lib.cgs_curve_straightness(4, one, one, 1, d(0.002), d(0.004), one, one, one, None))
    assert bad(lib.cgs_curve_straightness(4, one, one, 257, d(0.002), d(0.004), one, one, one, None))
    assert bad(lib.cgs_curve_straightness(4, one, one, 100, d(float("nan")), d(0.004), one, one, one, None))
    assert bad(lib.cgs_curve_straightness(4, None, one, 100, d(0.002), d(0.004), one, one, one, None))
    assert lib.cgs_curve_straightness(0, None, None, 100, d(0.002), d(0.004), None, None, None, None) == 0
    # cgs_segment_merge_labels
    assert lib.cgs_segment_merge_workspace_bytes(8192) >= 8192 * 128 * 8
    assert lib.cgs_segment_merge_workspace_bytes(8192) < 8192 * 8192 * 4 // 16      # far from n^2 floats
    assert lib.cgs_segment_merge_workspace_bytes(65) >= 65 * 2 * 8
    assert bad(lib.cgs_segment_merge_labels(-1, one, d(0.02), d(0.97), one, one, one, None))
    assert bad(lib.cgs_segment_merge_labels(12289, one, d(0.02), d(0.97), one, one, one, None))
    assert bad(lib.cgs_segment_merge_labels(10, None, d(0.02), d(0.97), one, one, one, None))
    assert bad(lib.cgs_segment_merge_labels(10, one, d(0.02), d(0.97), one, one, None, None))
    assert bad(lib.cgs_segment_merge_labels(10, one, d(0.02), d(float("nan")), one, one, one, None))
    # cgs_pair_consensus_fit
    assert bad(lib.cgs_pair_consensus_fit(10, one, -1, one, 100, d(0.005), d(0.02), one, one, one, one, None))
    assert bad(lib.cgs_pair_consensus_fit(10, one, 3, one, 1, d(0.005), d(0.02), one, one, one, one, None))
    assert bad(lib.cgs_pair_consensus_fit(10, one, 3, one, 257, d(0.005), d(0.02), one, one, one, one, None))
    assert bad(lib.cgs_pair_consensus_fit(10, one, 3, None, 100, d(0.005), d(0.02), one, one, one, one, None))
    assert bad(lib.cgs_pair_consensus_fit(0, None, 3, one, 100, d(0.005), d(0.02), one, one, one, one, None))
    assert bad(lib.cgs_pair_consensus_fit(10, one, 3, one, 100, d(float("nan")), d(0.02), one, one, one, one, None))
    assert lib.cgs_pair_consensus_fit(10, one, 0, None, 100, d(0.005), d(0.02), None, None, None, None, None) == 0


def test_ops_have_no_cpu_fallback():
    from curve_gaussian_amd import _lib
    from curve_gaussian_amd.ops import curve_fit as CF
    with pytest.raises(_lib.CurveGSError, match="GPU tensor"):
        CF.curve_straightness(torch.zeros(2, 4, 3), torch.ones(2, dtype=torch.bool), 0.002, 0.004)
    with pytest.raises(_lib.CurveGSError, match="GPU tensor"):
        CF.segment_merge_labels(torch.zeros(3, 6), 0.02, 0.97)
    with pytest.raises(_lib.CurveGSError, match="GPU tensor"):
        CF.pair_consensus_fit(torch.zeros(2, 4, 3), torch.zeros(1, 2, dtype=torch.int32))
    assert CF.MAX_SAMPLES >= 256 and CF.MAX_SEGMENTS >= 8192


# ------------------------------------------------------------------------------------------------ driver and keyword
def test_parser_accepts_the_topology_backend_and_defaults_to_host():
    from curve_gaussian_amd import train as T
    assert T.build_parser().parse_args(["-s", "scan", "-m", "out"]).topology_backend == "host"
    assert T.build_parser().parse_args(["-s", "scan", "-m", "out", "--topology_backend", "gpu"]).topology_backend == "gpu"
    with pytest.raises(SystemExit):
        T.build_parser().parse_args(["-s", "scan", "-m", "out", "--topology_backend", "bogus"])
    import inspect
    assert inspect.signature(T.training).parameters["topology_backend"].default == "host"


def test_unknown_backend_raises(tmp_path):
    import inspect
    from curve_gaussian_amd import train as T
    from curve_gaussian_amd.scene import GaussianCurveModel, topology
    for fn in (topology.fit_curve_to_line, topology.merge_curves, GaussianCurveModel.fit_curve_to_line,
               GaussianCurveModel.merge_curves):
        assert inspect.signature(fn).parameters["backend"].default == "host"
        with pytest.raises(ValueError, match="bogus"):
            fn(None, backend="bogus")
    with pytest.raises(ValueError, match="bogus"):
        T.training(T.ModelParams(source_path="scan", model_path=str(tmp_path / "o")), T.OptimizationParams(), [], [], [],
                   topology_backend="bogus")
