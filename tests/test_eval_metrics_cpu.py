"""CPU: the float64 restatement of the held-out metrics (tests/metrics_ref64.py) against the reference's own
training_report (tests/golden/eval_metrics.npz, tests/golden/make_eval_golden.py), and training_report's camera selection
(curve_gaussian_amd.evaluation.report_configs) against the order in which the reference rendered the cameras."""
import os

import numpy as np
import pytest

import metrics_ref64 as M

GOLDEN = np.load(os.path.join(os.path.dirname(__file__), "golden", "eval_metrics.npz"))
CASES = [str(c) for c in GOLDEN["cases"]]


def case_views(case):
    n = int(GOLDEN[f"{case}_n_test"]) + int(GOLDEN[f"{case}_n_train"])
    return [GOLDEN[f"{case}_render_{i}"] for i in range(n)], [GOLDEN[f"{case}_gt_{i}"] for i in range(n)]


class _Scene:
    def __init__(self, train, test):
        self.train, self.test = train, test

    def getTrainCameras(self):
        return self.train

    def getTestCameras(self):
        return self.test


def selection(case):
    """report_configs on a scene whose cameras are their fixture indices -> {config: [indices]}."""
    from curve_gaussian_amd.evaluation import report_configs
    nt = int(GOLDEN[f"{case}_n_test"])
    n = nt + int(GOLDEN[f"{case}_n_train"])
    return {name: cams for name, cams in report_configs(_Scene(list(range(nt, n)), list(range(nt))))}


@pytest.mark.parametrize("case", CASES)
def test_camera_selection_matches_the_reference(case):
    sel = selection(case)
    assert list(sel) == [str(c) for c in GOLDEN[f"{case}_configs"]]       # empty configs skipped, test before train
    assert [i for cams in sel.values() for i in cams] == GOLDEN[f"{case}_order"].tolist()


@pytest.mark.parametrize("case", CASES)
def test_float64_restatement_matches_the_reference_report(case):
    images, gts = case_views(case)
    half = bool(GOLDEN[f"{case}_train_test_exp"])
    for k, (name, idx) in enumerate(selection(case).items()):
        l1, ps = M.report([images[i] for i in idx], [gts[i] for i in idx], half)
        np.testing.assert_allclose(l1, GOLDEN[f"{case}_l1"][k], rtol=1e-5, atol=1e-7)
        np.testing.assert_allclose(ps, GOLDEN[f"{case}_psnr"][k], rtol=1e-5)


def test_cases_cover_the_issue():
    assert any(np.isinf(GOLDEN[f"{c}_psnr"]).any() for c in CASES)                       # exact match
    assert any(bool(GOLDEN[f"{c}_train_test_exp"]) for c in CASES)
    assert any(int(GOLDEN[f"{c}_n_test"]) == 0 for c in CASES)                           # empty test config
    chans = {GOLDEN[f"{c}_gt_{i}"].shape[0] for c in CASES for i in range(len(case_views(c)[0]))}
    assert chans == {1, 3}
    vals = np.concatenate([GOLDEN[f"{c}_render_0"].ravel() for c in CASES])
    assert vals.min() < 0 and vals.max() > 1


def test_psnr_of_an_exact_match_is_inf_and_the_mean_is_per_view():
    assert M.psnr(0.0) == float("inf")
    a = np.full((1, 2, 2), 0.5, np.float32)
    l1, ps = M.report([a, a], [a + 0.1, a + 0.3])
    assert ps == pytest.approx((M.psnr(0.01) + M.psnr(0.09)) / 2, rel=1e-6)
    assert ps != pytest.approx(M.psnr(0.05), rel=1e-3)                                    # not the PSNR of the mean MSE


def test_view_metrics_has_no_cpu_fallback():
    import torch
    from curve_gaussian_amd import _lib as L
    from curve_gaussian_amd.evaluation import view_metrics
    with pytest.raises(L.CurveGSError, match="GPU tensor"):
        view_metrics([torch.zeros(1, 4, 4)], [torch.zeros(3, 4, 4)])
