"""CPU: curve_gaussian_amd.train runs the reference's schedule.  Its real loop runs on the recording fakes of
tests/train_fakes.py and must write the call log the reference's own training() wrote on the same fakes
(tests/golden/train_schedule.json, make_train_schedule_golden.py): every edit, snapshot, report, checkpoint, use_mask switch
and optimizer step at the same iteration and in the same order, and on an edit iteration the optimizer step comes after
the edits, so the replaced groups get no update.  The command line derives its options as train.py:378-404 does."""
import json
import os

import pytest
import torch

import train_fakes as TF

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = json.load(open(os.path.join(HERE, "golden", "train_schedule.json")))
GPU_OVERRIDES = dict(iterations=5000, densify_from_iter=100, densification_interval=200, densify_until_iter=1000,
                     opacity_reset_interval=500)


def run_product(opt, lists, tmp_path, checkpoint=None):
    from curve_gaussian_amd import train as T
    rec = TF.Recorder()
    model = TF.FakeModel(rec)
    scene = TF.FakeScene(rec, model)
    step = TF.FakeStep(rec, model, opt.densify_until_iter)
    dataset = T.ModelParams(source_path="scan", model_path=str(tmp_path / "out"))
    saves = list(lists["save"]) + [opt.iterations]          # train.py:404
    out = T.training(dataset, opt, lists["test"], saves, lists["checkpoint"], checkpoint, quiet=True, scene=(scene, model),
                     step=step, report=lambda it, tests, sc, bg: rec.add("report"),
                     save_ply=lambda g, path, it: rec.add("save"), save_checkpoint=lambda obj, path: rec.add("checkpoint"),
                     export=lambda g, d, o: rec.add("export"))
    return TF.compress(TF.normalise(rec.log)), out


@pytest.mark.parametrize("run", ["defaults", "replica", "resumed3000", "gpu_options"])
def test_driver_writes_the_reference_call_log(run, tmp_path):
    from curve_gaussian_amd import train as T
    g = GOLDEN["runs"][run]
    opt = (T.OptimizationParamsReplica() if run == "replica" else
           T.OptimizationParams(**(GPU_OVERRIDES if run == "gpu_options" else {})))
    ck = None
    if "checkpoint" in g:
        ck = str(tmp_path / f"chkpnt{g['checkpoint']}.pth")
        torch.save(({"fake": True}, g["checkpoint"]), ck)
    log, out = run_product(opt, g["lists"], tmp_path, ck)
    assert log["events"] == g["log"]["events"]
    assert log["plain_steps"] == g["log"]["plain_steps"]
    assert out["first_iter"] == g.get("checkpoint", 0)
    # the driver's own event log: the same edits, saves, reports and checkpoints in the same order
    mine = [(it, name) for it, name, _n in out["events"]]
    ref = [tuple(e[:2]) for e in g["log"]["events"] if e[1] not in ("optimizer.step",) and not e[1].startswith("use_mask")]
    assert mine == ref


def test_edit_iterations_take_their_optimizer_step_after_the_edits(tmp_path):
    """train.py:183-236: the edits run between backward and optimizer step, so every group an edit replaced is skipped by
    that step; the last iteration takes no step at all (:227)."""
    from curve_gaussian_amd import train as T
    opt = T.OptimizationParams(**GPU_OVERRIDES)
    log, _ = run_product(opt, GOLDEN["runs"]["gpu_options"]["lists"], tmp_path)
    steps = {e[0]: e[2] for e in log["events"] if e[1] == "optimizer.step"}
    edits = {}
    for e in log["events"]:
        if e[1] in TF.REPLACES:
            edits.setdefault(e[0], set()).update(TF.REPLACES[e[1]])
    assert edits and opt.iterations in edits
    for it, groups in edits.items():
        if it == opt.iterations:
            assert it not in steps
            assert all(not (a <= it <= b) for a, b in log["plain_steps"])
        else:
            assert set(steps[it]) == groups, it
    assert set(steps) == set(edits) - {opt.iterations}
    for it in range(1, opt.iterations):
        assert it in steps or any(a <= it <= b for a, b in log["plain_steps"]), it


def test_edit_iteration_rule_matches_the_logged_edits():
    from curve_gaussian_amd import train as T
    opt = T.OptimizationParams()
    logged = {e[0] for e in GOLDEN["runs"]["defaults"]["log"]["events"] if e[1] in TF.REPLACES}
    assert {it for it in range(1, opt.iterations + 1) if T.edit_iteration(it, opt)} == logged


def test_command_line_matches_the_reference_main():
    """train.py:378-404: the reference's flags and defaults, `iterations` appended to the save list, the variant by scan."""
    from curve_gaussian_amd import train as T
    d, opt, args = T.parse_args(["-s", "/data/scan1", "-m", "/out/x"])
    assert (d.source_path, d.model_path, d.detector, d.resolution, d.eval, d.sh_degree, d.n_gaussians) == \
        ("/data/scan1", "/out/x", "DexiNed", -1, False, 0, 12)
    assert opt.iterations == 10000 and type(opt) is T.OptimizationParams
    assert args.test_iterations == [3000, 10000] and args.save_iterations == [3000, 10000, 10000]
    assert args.checkpoint_iterations == [10000] and args.start_checkpoint is None and args.backend == "graphed"
    d, opt, args = T.parse_args(["-s", "rel/Replica/room0", "-m", "o", "--iterations", "600", "--test_iterations", "300",
                                 "--save_iterations", "200", "--checkpoint_iterations", "100", "400", "--start_checkpoint",
                                 "c.pth", "--eval", "-r", "2", "--detector", "PidiNet", "--quiet", "--backend", "direct"])
    assert type(opt) is T.OptimizationParamsReplica and opt.iterations == 600 and opt.lambda_mse == 1.0
    assert d.source_path == os.path.abspath("rel/Replica/room0") and d.eval and d.resolution == 2 and d.detector == "PidiNet"
    assert args.test_iterations == [300] and args.save_iterations == [200, 600] and args.checkpoint_iterations == [100, 400]
    assert args.start_checkpoint == "c.pth" and args.quiet and args.backend == "direct"
    assert type(T.parse_args(["-s", "/d/ABC/0001", "--detector", "Pidinet"])[1]) is T.OptimizationParamsPidinet
    assert type(T.parse_args(["-s", "/d/ABC/0001"])[1]) is T.OptimizationParams
    with pytest.raises(SystemExit):
        T.parse_args(["-s", "x", "--backend", "triton"])


def test_options_carry_the_reference_defaults():
    from curve_gaussian_amd import train as T
    o = T.OptimizationParams()
    assert (o.densify_from_iter, o.densify_until_iter, o.densification_interval, o.opacity_reset_interval) == (500, 7000, 2000, 3000)
    assert (o.opacity_cull, o.opacity_cull_second, o.densify_grad_threshold, o.merge_endpoints_flag) == (0.01, 0.05, 2000, True)
    p = T.OptimizationParamsPidinet()
    assert (p.lambda_mse, p.lambda_width, p.distance_threshold, p.similarity_threshold) == (2.0, 0.0, 0.03, 0.95)
    with pytest.raises(TypeError):
        T.OptimizationParams(no_such_option=1)
