"""The reference's training driver (train.py:38-248, ``__main__`` :378-416) on this package's parts: scan -> trained curves ->
``parametric_edges.json``.

    python -m curve_gaussian_amd.train -s SCAN -m OUT [--iterations N] [--backend graphed|direct|autograd|torch]
                                       [--draw_snapshots] [--topology_backend host|gpu] [--report_dir DIR] [--undistort]
                                       [--init reference|edge_votes] [--init_directions] [--init_exclusive]
                                       [--init_occluder FILE | --init_depth_dir DIR] [--init_near_clip [VALUE]]
                                       [--thin_edge_maps]

The loop keeps the reference's order.  Per iteration: learning rate, SH degree every 1000 iterations, a random view without
replacement, render + losses + every regulariser + backward (one ``TrainStep`` call), densification statistics before
``densify_until_iter``, the held-out report, the topology edits, the snapshot, the optimizer step, the checkpoint.

The topology edits run between the backward and the optimizer step (:183-236), so those iterations are run with
``step(update=False)`` and finished with ``apply_update()``; they are known in advance from the iteration number.  So are
the report and snapshot iterations, which read the model before its update (:176-229).  With ``draw`` (``--draw_snapshots``)
every snapshot is followed by the reference's two inspection files, ``curve_step{N}.ply`` and ``ellipsoids_step{N}.ply``
(``draw_curve`` / ``draw_ellipsoids``, :215-220; scene/snapshot_viz.py); it is off by default.  Every other iteration runs
straight through, and with ``backend="graphed"`` it is one graph replay.  An edit that replaced a curve parameter leaves
that group without gradient, and torch.optim.Adam then skips it; the flat one-launch Adam skips the whole step then
(``TrainStep.apply_update``).

With ``report_writer`` (``--report_dir DIR``: an ``evaluation.ReportDirWriter``) the held-out report also writes the
reference's tensorboard summaries (:323-373) -- the report's scalars and, for the first five views of each config, the
render, ground truth, depth, direction and alpha panels -- as ``DIR/scalars.jsonl`` and
``DIR/images/iter_{N:06d}/{config}_view_{name}__{panel}.png``.  Without it nothing is written and the run is what it was.

Out of scope: the network GUI, view-parallel runs, sparse_adam."""
import argparse
import os
import sys

import torch


class ModelParams:
    """The fields of the reference's ModelParams (arguments/__init__.py:47-66) this driver reads."""

    def __init__(self, source_path="", model_path="", sh_degree=0, n_gaussians=12, detector="DexiNed", resolution=-1,
                 white_background=False, eval=False, undistort=False, init="reference", init_options=None):
        self.source_path, self.model_path = source_path, model_path
        self.sh_degree, self.n_gaussians, self.detector = sh_degree, n_gaussians, detector
        self.resolution, self.white_background, self.eval = resolution, white_background, eval
        self.undistort = undistort   # not in the reference: COLMAP scans with lens distortion (scene/colmap_io.py)
        # not in the reference: "edge_votes" seeds the curves from the edge maps (Scene; ops/edge_seed.py)
        self.init, self.init_options = init, dict(init_options or {})


class OptimizationParams:
    """arguments/__init__.py:77-124, the reference's defaults."""

    def __init__(self, **overrides):
        self.iterations = 10_000
        self.position_lr_delay_mult = 0.01
        self.position_lr_max_steps = 30_000
        self.lr_curve_points_init = 0.0005
        self.lr_curve_points_final = 0.000005
        self.feature_lr = 0.0025
        self.opacity_lr = 0.025
        self.scaling_lr = 0.005
        self.rotation_lr = 0.001
        self.mask_lr = 0.01
        self.exposure_lr_init = 0.01
        self.exposure_lr_final = 0.001
        self.exposure_lr_delay_steps = 0
        self.exposure_lr_delay_mult = 0.0
        self.percent_dense = 0.01
        self.lambda_dssim = 0.1
        self.opacity_cull = 0.01
        self.opacity_cull_second = 0.05
        self.opacity_loss_weight = 0.01
        self.lambda_mse = 10.
        self.lambda_curve_smo = 0.1
        self.lambda_points_conn = 0.1
        self.lambda_width = 0.01
        self.lambda_mask = 0.0005
        self.mask_threshold = 0.01
        self.merge_endpoints_flag = True
        self.visible_checking = False
        self.densification_interval = 2000
        self.opacity_reset_interval = 3000
        self.prune_interval = 1500
        self.densify_from_iter = 500
        self.densify_until_iter = 7000
        self.conn_from_iter = 7000
        self.densify_grad_threshold = 2000
        self.random_background = False
        self.optimizer_type = "default"
        self.threshold_line = 0.0015
        self.threshold_max_line = 0.005
        self.threshold_angle = 20
        self.threshold_angle_skip = 30
        self.distance_threshold = 0.02
        self.similarity_threshold = 0.97
        self._variant()
        for k, v in overrides.items():
            if not hasattr(self, k):
                raise TypeError(f"OptimizationParams: unknown option {k!r}")
            setattr(self, k, v)

    def _variant(self):
        pass


class OptimizationParamsPidinet(OptimizationParams):
    """arguments/__init__.py:127-135"""

    def _variant(self):
        self.lambda_mse = 2.0
        self.lambda_width = 0.0
        self.threshold_line = 0.002
        self.threshold_max_line = 0.006
        self.distance_threshold = 0.03
        self.similarity_threshold = 0.95


class OptimizationParamsReplica(OptimizationParams):
    """arguments/__init__.py:138-147"""

    def _variant(self):
        self.opacity_cull = 0.05
        self.lambda_mse = 1.0
        self.lambda_width = 0.0
        self.threshold_line = 0.0002
        self.threshold_max_line = 0.001
        self.similarity_threshold = 0.95


BACKENDS = ("graphed", "direct", "autograd", "torch")


def edit_iteration(it, opt):
    """True on the iterations where train.py:189-211 edits the topology (after the backward, before the optimizer step)."""
    return ((it < opt.densify_until_iter and it > opt.densify_from_iter and it % opt.densification_interval == 0)
            or it == opt.densify_until_iter
            or (it % 1000 == 500 and it > opt.densify_until_iter)                      # :202
            or (it % 1000 == 0 and it > 3000 and it != opt.iterations)                 # :206
            or (it % 1000 == 0 and it > opt.densify_until_iter) or it == opt.iterations)   # :209


def make_scene(dataset, opt, device):
    """train.py:45-48: the model, the scan, the optimizer groups."""
    from .scene import GaussianCurveModel, Scene
    gaussians = GaussianCurveModel(dataset.sh_degree, dataset.n_gaussians, opt.optimizer_type, device=device)
    scene = Scene(dataset.source_path, gaussians, detector=dataset.detector, eval=dataset.eval,
                  resolution=dataset.resolution, device=device, undistort=dataset.undistort, init=dataset.init,
                  init_options=dataset.init_options)
    scene.model_path = dataset.model_path
    gaussians.training_setup(opt)
    return scene, gaussians


def make_step(backend, gaussians, cameras, opt, seed=0, depth_gate=None, gate_from_iter=0):
    """The per-iteration object of `backend` with train.py's loss weights, every regulariser and the statistics on;
    ``depth_gate`` (an ``ops.train_gate.TrainGate`` over ``cameras``) gates the training render from ``gate_from_iter`` on."""
    from .train_step import GraphedTrainStep, TrainStep
    if backend not in BACKENDS:
        raise ValueError(f"training: unknown backend {backend!r} (one of {BACKENDS})")
    gts = [c.original_image[:1].contiguous() for c in cameras]
    kw = dict(lambda_mse=opt.lambda_mse, lambda_dssim=opt.lambda_dssim, lambda_mask=opt.lambda_mask,
              densify_until_iter=opt.densify_until_iter, mask_threshold=opt.mask_threshold, seed=seed, regularisers=True,
              opacity_loss_weight=opt.opacity_loss_weight, lambda_curve_smo=opt.lambda_curve_smo,
              lambda_width=opt.lambda_width, lambda_points_conn=opt.lambda_points_conn, conn_from_iter=opt.conn_from_iter,
              densification_stats=True)
    if depth_gate is not None:
        kw.update(depth_gate=depth_gate, gate_from_iter=gate_from_iter)
    if backend == "graphed":
        return GraphedTrainStep(gaussians, cameras, gts, **kw)
    return TrainStep(gaussians, cameras, gts, fused=backend != "torch", direct=backend == "direct", **kw)


def _report(iteration, testing_iterations, scene, bg, writer=None):
    from . import evaluation as E
    from .gaussian_renderer import PipelineParams, render
    return E.training_report(writer, iteration, None, None, None, None, testing_iterations, scene, render,
                             (PipelineParams(), bg), False)


def _save_ply(gaussians, model_path, iteration):
    """scene/__init__.py:94-96 (Scene.save)."""
    from .scene.dataset_io import save_ply
    save_ply(gaussians, os.path.join(model_path, "point_cloud", f"iteration_{iteration}", "point_cloud.ply"))


def _export(gaussians, dataset, opt, visibility_options=None):
    """train.py:250-293 (extract_curves).  ``visibility_options``: the depth gate of the visibility check (--gate_visibility)."""
    from .scene.dataset_io import write_parametric_edges
    return write_parametric_edges(gaussians, dataset.model_path, merge_endpoints=opt.merge_endpoints_flag,
                                  distance_threshold=0.015, visible_checking=opt.visible_checking,   # :264
                                  scan_dir=dataset.source_path, detector=dataset.detector,
                                  **({"visibility_options": visibility_options} if visibility_options else {}))


def training(dataset, opt, testing_iterations, saving_iterations, checkpoint_iterations, checkpoint=None, backend="graphed",
             seed=0, device="cuda", quiet=False, scene=None, step=None, report=None, save_ply=None, save_checkpoint=None,
             export=None, draw=False, topology_backend="host", report_writer=None, train_gate=None, gate_from_iter=0):
    """train.py:38-248.  Returns {"events": [(iteration, event, n_curves_after)] for every edit, report, save, checkpoint and
    the export, "losses": {iteration: loss} (the first iteration and every iteration run with a deferred update),
    "first_iter", "scene", "gaussians"}.

    Collaborators (defaults in brackets), injectable so that the loop itself can be run by a CPU test: ``scene`` = (scene,
    gaussians) [make_scene], ``step`` = the per-iteration object [make_step(backend, ...)], ``report(iteration,
    testing_iterations, scene, bg)`` [evaluation.training_report], ``save_ply(gaussians, model_path, iteration)``,
    ``save_checkpoint(obj, path)`` [torch.save], ``export(gaussians, dataset, opt)`` [write_parametric_edges].  ``draw``: after
    every snapshot, ``gaussians.draw_curve(dir, iteration)`` and ``gaussians.draw_ellipsoids(dir, iteration)`` into the
    snapshot's directory (train.py:215-220); no event is logged for them.  ``topology_backend``: "host" runs fit_curve_to_line
    and merge_curves in numpy like the reference, "gpu" in the kernels of ops/curve_fit.py (scene/topology.py); the schedule and
    the event log are the same.  ``report_writer``: a summary writer (``evaluation.ReportDirWriter``, a tensorboard
    ``SummaryWriter``) handed to the default ``report``, which then writes the reference's scalar and image summaries at the
    test iterations; None writes nothing.  An injected ``report`` is called as before and never sees it.
    ``train_gate`` (--gate_training; OFF BY DEFAULT, UNTUNED): ``cameras -> keywords of ops.train_gate.TrainGate``, called with
    the train cameras; the gate built from them culls, from iteration ``gate_from_iter`` on, every splat of the training render
    whose centre its view's depth plane hides, and ``<model_path>/train_gate.json`` is written after the export
    (``write_train_gate_report``).  Not with an injected ``step`` or ``backend="torch"``."""
    from .scene.topology import _check_backend
    _check_backend(topology_backend)
    topo = {} if topology_backend == "host" else {"backend": topology_backend}
    say = (lambda *a: None) if quiet else print
    os.makedirs(dataset.model_path, exist_ok=True)
    scene, gaussians = scene if scene is not None else make_scene(dataset, opt, device)
    first_iter = 0
    if checkpoint:                                                                  # :49-51
        model_params, first_iter = torch.load(checkpoint, weights_only=False)
        gaussians.restore(model_params, opt)
    gate = None
    if train_gate is not None:
        if step is not None or backend == "torch":
            raise ValueError("training(train_gate=...): the depth gate lives in the fused view forward of this package's own "
                             "steps (not backend='torch', not an injected step)")
        from .ops.train_gate import TrainGate
        cams = scene.getTrainCameras()
        gate = TrainGate(cams, device=gaussians._curve_points.device, **train_gate(cams))
        say(f"Training gate: {gate.V} planes of {gate.width}x{gate.height}, {gate.planes_bytes} bytes, slack {gate.slack:g}, "
            f"from iteration {int(gate_from_iter)}")
    step = step if step is not None else make_step(backend, gaussians, scene.getTrainCameras(), opt, seed, gate, gate_from_iter)
    step.start_at(first_iter)
    bg = torch.tensor([1, 1, 1] if dataset.white_background else [0, 0, 0], dtype=torch.float32,
                      device=gaussians._curve_points.device)                        # :53-54
    step.bg = bg
    if report is None:
        report = _report if report_writer is None else (lambda *a: _report(*a, writer=report_writer))
    save_ply = save_ply or _save_ply
    save_checkpoint = save_checkpoint or torch.save
    export = export or _export
    events, losses = [], {}
    finish = getattr(step, "finish", lambda: None)
    n_curves = lambda: int(gaussians._curve_points.shape[0])

    def log(it, name):
        events.append((it, name, n_curves()))

    for iteration in range(first_iter + 1, opt.iterations + 1):
        if iteration % 1000 == 0:                                                   # :81-82
            gaussians.oneupSHdegree()
        deferred = (edit_iteration(iteration, opt) or iteration in testing_iterations or iteration in saving_iterations
                    or iteration == opt.iterations)
        loss, pkg = step.step(update=not deferred)
        if iteration == first_iter + 1 or deferred:
            losses[iteration] = float(loss)
        if not deferred:
            if iteration in checkpoint_iterations:
                finish()
                save_checkpoint((gaussians.capture(), iteration), os.path.join(dataset.model_path, f"chkpnt{iteration}.pth"))
                log(iteration, "checkpoint")
            continue
        if iteration in testing_iterations:                                         # :176-179
            report(iteration, testing_iterations, scene, bg)
            log(iteration, "report")
        if iteration < opt.densify_until_iter:                                      # :182-191 (statistics: in the step)
            if iteration > opt.densify_from_iter and iteration % opt.densification_interval == 0:
                size_threshold = 20 if iteration > opt.opacity_reset_interval else None   # :190
                gaussians.densify_and_prune(opt.densify_grad_threshold, opt.opacity_cull, scene.cameras_extent,
                                            size_threshold, pkg["radii"])
                log(iteration, "densify_and_prune")
        if iteration == opt.densify_until_iter:                                     # :195-199
            gaussians.prune_curves((gaussians.get_curve_opacity <= opt.opacity_cull_second).squeeze())
            log(iteration, "prune_curves")
            gaussians.fix_opacity()
            log(iteration, "fix_opacity")
        if iteration % 1000 == 500 and iteration > opt.densify_until_iter:          # :202-204
            gaussians.only_prune(opt.opacity_cull, opt.mask_threshold)
            log(iteration, "only_prune")
            gaussians.mask_trim_split(opt.mask_threshold)
            log(iteration, "mask_trim_split")
        if iteration % 1000 == 0 and iteration > 3000 and iteration != opt.iterations:   # :206-207
            gaussians.curve_split_curvature(opt.threshold_angle, opt.threshold_angle_skip)
            log(iteration, "curve_split_curvature")
        if (iteration % 1000 == 0 and iteration > opt.densify_until_iter) or iteration == opt.iterations:   # :209-211
            gaussians.fit_curve_to_line(opt.threshold_line, opt.threshold_max_line, **topo)
            log(iteration, "fit_curve_to_line")
            gaussians.merge_curves(opt.distance_threshold, opt.similarity_threshold, **topo)
            log(iteration, "merge_curves")
        if iteration in saving_iterations:                                          # :213-229
            say(f"\n[ITER {iteration}] Saving Gaussians")
            save_ply(gaussians, dataset.model_path, iteration)
            log(iteration, "save")
            if draw:                                                                # :215-220
                snap = os.path.join(dataset.model_path, "point_cloud", f"iteration_{iteration}")
                gaussians.draw_curve(snap, iteration)
                gaussians.draw_ellipsoids(snap, iteration)
        if iteration < opt.iterations:                                              # :227-236
            step.apply_update()
        else:
            step.drop_update()
        if iteration in checkpoint_iterations:                                      # :238-240
            say(f"\n[ITER {iteration}] Saving Checkpoint")
            finish()
            save_checkpoint((gaussians.capture(), iteration), os.path.join(dataset.model_path, f"chkpnt{iteration}.pth"))
            log(iteration, "checkpoint")
    finish()
    export(gaussians, dataset, opt)                                                 # :248
    log(opt.iterations, "export")
    if gate is not None:
        write_train_gate_report(os.path.join(dataset.model_path, "train_gate.json"), gaussians, gate, gate_from_iter)
    return {"events": events, "losses": losses, "first_iter": first_iter, "scene": scene, "gaussians": gaussians}


def write_train_gate_report(path, gaussians, gate, gate_from_iter=0, backend="gpu"):
    """``train_gate.json`` of a gated run, from the FINAL splat centres and existing operators only: per view what
    ``point_masks_depth`` counts (the centres the view keeps and does not hide, and those it hides), and per splat, from the
    same rule on the host (``ops.train_gate.splat_visibility``), how many views see it, how many of those hide it, and whether
    it is "dead": hidden in EVERY view that sees it, so that no gradient of a gated run can reach it.  ``backend``: where
    ``point_masks_depth`` runs ("host" for a gate built on the host).  Returns the dict."""
    import json
    from .ops.edge_occlusion import point_masks_depth
    from .ops.train_gate import splat_visibility
    xyz = gaussians.get_xyz.detach().float().contiguous()
    _mask, kept, hidden_v = point_masks_depth(xyz, gate.intr, gate.w2c, gate.planes, gate.slack, backend=backend,
                                              return_counts=True)
    seen, hidden, dead = splat_visibility(xyz, gate)
    out = {"settings": dict(gate.settings(), gate_from_iter=int(gate_from_iter)), "splats": int(xyz.shape[0]),
           "views": [{"kept": int(k), "hidden": int(h)} for k, h in zip(kept.cpu().tolist(), hidden_v.cpu().tolist())],
           "never_seen": int((seen == 0).sum()), "hidden_somewhere": int((hidden > 0).sum()), "dead": int(dead.sum()),
           "seen_views": [int(x) for x in seen], "hidden_views": [int(x) for x in hidden],
           "dead_splats": [int(i) for i in dead.nonzero()[0]]}
    with open(path, "w") as f:
        json.dump(out, f)
    return out


def select_options(source_path, detector):
    """train.py:396-402: 'ABC' scans with the Pidinet detector and 'Replica' scans take their option variants.  (The
    reference tests the ModelParams object's class default, never 'Pidinet', and builds the variant after parsing, so its
    own run keeps the base values; here the variant's values are the defaults of the parsed options -- DESIGN section 6.)"""
    cls = OptimizationParams
    if "ABC" in source_path and detector == "Pidinet":
        cls = OptimizationParamsPidinet
    if "Replica" in source_path:
        cls = OptimizationParamsReplica
    return cls


def build_parser():
    p = argparse.ArgumentParser(description="Training script parameters")
    p.add_argument("--source_path", "-s", default="")
    p.add_argument("--model_path", "-m", default="")
    p.add_argument("--sh_degree", type=int, default=0)
    p.add_argument("--n_gaussians", type=int, default=12)
    p.add_argument("--detector", default="DexiNed")
    p.add_argument("--resolution", "-r", type=int, default=-1)
    p.add_argument("--white_background", "-w", action="store_true")
    p.add_argument("--eval", action="store_true")
    p.add_argument("--undistort", action="store_true",
                   help="COLMAP scans: resample the edge maps through each camera's lens model and principal point (accepts "
                        "SIMPLE_RADIAL, RADIAL and FULL_OPENCV cameras too); without it distortion is ignored, as in the reference")
    p.add_argument("--init", choices=("reference", "edge_votes"), default="reference",
                   help="the seed of the curves: the reference's (the 15^3 grid, or the SfM cloud of a COLMAP scan) or a "
                        "multi-view voxel vote of the training views' edge maps (untuned defaults; occlusion reasoning only "
                        "with --init_occluder / --init_depth_dir; see also --init_exclusive)")
    p.add_argument("--init_grid", type=int, default=None, help="edge_votes: voxels along the longest side of the box")
    p.add_argument("--init_tol_px", type=float, default=None, help="edge_votes: pixel distance to a detected edge that votes")
    p.add_argument("--init_min_views", type=int, default=None, help="edge_votes: views that must see a voxel")
    p.add_argument("--init_min_ratio", type=float, default=None, help="edge_votes: share of the seeing views that must vote")
    p.add_argument("--init_cell", type=int, default=None, help="edge_votes: voxels per axis thinned to one seed")
    p.add_argument("--init_directions", action="store_true",
                   help="edge_votes: lay every curve along the principal axis of the kept voxels around its seed instead of "
                        "+-Y (untuned defaults)")
    p.add_argument("--init_dir_radius", type=int, default=None, help="edge_votes: voxels around a seed that give its direction")
    p.add_argument("--init_dir_min_support", type=int, default=None,
                   help="edge_votes: kept voxels a seed needs around it to be given a direction")
    p.add_argument("--init_dir_min_linearity", type=float, default=None,
                   help="edge_votes: (l2 - l1) / l2 of the voxels' scatter a seed needs to be given a direction")
    p.add_argument("--init_exclusive", action="store_true",
                   help="edge_votes: keep only the voted voxels that win the pixels they claim -- suppresses the ghosts of a "
                        "scan with few views (untuned defaults; no depth of its own: see --init_occluder)")
    p.add_argument("--init_excl_window", type=int, default=None,
                   help="edge_votes: pixels around a voxel's pixel in which a better supported voxel beats it")
    p.add_argument("--init_excl_margin", type=int, default=None,
                   help="edge_votes: support (of 65535) by which a voxel may fall short of the best claim and still win")
    p.add_argument("--init_excl_win_ratio", type=float, default=None,
                   help="edge_votes: share of the views a voxel hits in that it must win")
    p.add_argument("--init_occluder", default=None, metavar="FILE",
                   help="edge_votes: a mesh file inside the scan directory (mesh.ply, .obj); a view that sees a voxel's centre "
                        "behind it does not count the voxel as seen -- without a depth source the vote keeps next to nothing "
                        "on a scan of a solid (untuned; no near-plane clipping unless --init_near_clip)")
    from .ops.edge_occlusion import NEAR_CLIP
    p.add_argument("--init_near_clip", nargs="?", type=float, const=NEAR_CLIP, default=None, metavar="VALUE",
                   help="edge_votes, with --init_occluder: clip the mesh at this camera depth instead of dropping a triangle "
                        f"that reaches behind the camera, for cameras INSIDE the mesh (bare flag: {NEAR_CLIP}; untuned)")
    p.add_argument("--init_depth_dir", default=None, metavar="DIR",
                   help="edge_votes: a directory inside the scan holding <image stem>.npy depth maps (camera z) instead of a mesh")
    p.add_argument("--init_depth_slack", type=float, default=None,
                   help="edge_votes: world units a voxel's centre may lie behind the surface (default: half the voxel diagonal; "
                        "untuned)")
    p.add_argument("--init_depth_window", type=int, default=None,
                   help="edge_votes: radius of the window maximum over the depth planes (untuned)")
    p.add_argument("--init_bounds", nargs=6, type=float, default=None, metavar=("X0", "Y0", "Z0", "X1", "Y1", "Z1"),
                   help="edge_votes: the box to search (default: the reference's box, or the trimmed extent of the SfM cloud)")
    p.add_argument("--iterations", type=int, default=None)
    p.add_argument("--test_iterations", nargs="+", type=int, default=[3_000, 10_000])        # :386-391
    p.add_argument("--save_iterations", nargs="+", type=int, default=[3_000, 10_000])
    p.add_argument("--quiet", action="store_true")
    p.add_argument("--checkpoint_iterations", nargs="+", type=int, default=[10000])
    p.add_argument("--start_checkpoint", type=str, default=None)
    p.add_argument("--backend", choices=BACKENDS, default="graphed")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--topology_backend", choices=("host", "gpu"), default="host",
                   help="where fit_curve_to_line / merge_curves compute: numpy on the host like the reference, or HIP kernels")
    p.add_argument("--draw_snapshots", action="store_true",
                   help="write curve_step{N}.ply and ellipsoids_step{N}.ply next to every snapshot")
    p.add_argument("--report_dir", default=None,
                   help="write the report's summaries here at every test iteration: scalars.jsonl and, per view, the render, "
                        "ground-truth, depth, direction and alpha panels as images/iter_{N}/*.png")
    p.add_argument("--reprojection_score", action="store_true",
                   help="after the export, score parametric_edges.json in 2D against the edge maps of the train cameras and, "
                        "separately, of the test cameras (the held-out ones under --eval): reprojection_score.json in the "
                        "model directory")
    from .edge_extraction.reprojection import add_depth_arguments
    add_depth_arguments(p)   # --occluder / --depth_dir (inside --source_path), --depth_slack, --depth_window: for the score
    p.add_argument("--gate_edge_checks", action="store_true",
                   help="--snap_edges, --support_check and --trim_edges also take the depth source that --occluder or "
                        "--depth_dir names: a (sample, view) pair the depth hides counts as not seen (needs one of the two; "
                        "untuned, checked on drawn solids only)")
    p.add_argument("--visible_checking", action="store_true",
                   help="the export keeps only the edges that the scan's edge maps show (the reference's OptimizationParams "
                        "field of the same name, off in every option set; the check of get_parametric_edge, on the GPU)")
    p.add_argument("--gate_visibility", action="store_true",
                   help="the export's edge-map visibility check, which decides what goes into parametric_edges.json, also takes "
                        "the depth source that --occluder or --depth_dir names (with --near_clip): a control or end point the "
                        "depth hides is dropped before its frame is judged (needs one of the two, and the check itself: "
                        "--visible_checking; untuned, checked on drawn solids only)")
    p.add_argument("--gate_training", action="store_true",
                   help="the TRAINING render also takes the depth source that --occluder or --depth_dir names (with "
                        "--depth_window and --near_clip): in every view, a splat whose centre the view's depth plane hides is "
                        "culled like a frustum-culled one -- not drawn, no gradient; train_gate.json in the model directory "
                        "tallies the final splats (needs exactly one of the two sources; not with --backend torch; OFF BY "
                        "DEFAULT, untuned, checked on drawn solids only)")
    p.add_argument("--train_gate_slack", type=float, default=None, metavar="S",
                   help="--gate_training: how far behind the plane a centre may lie, in world units (default: the chain's "
                        "depth slack, untuned)")
    p.add_argument("--gate_from_iter", type=int, default=0, metavar="N",
                   help="--gate_training: the gate applies from iteration N on (default 0: from the start)")
    p.add_argument("--snap_edges", action="store_true",
                   help="after the export, FIRST move every edge of parametric_edges.json onto the detected edges of the "
                        "train cameras' edge maps: edge_snap.json and parametric_edges_snapped.json in the model directory; "
                        "--support_check, --trim_edges, --dedupe_edges and --join_edges then start from the snapped edges; "
                        "parametric_edges.json stays as it is (untuned defaults; no depth; not a filter)")
    p.add_argument("--snap_capture", type=float, default=None,
                   help="snapping: pixel distance to a detected edge within which a view pulls a sample, 1 to 8")
    p.add_argument("--snap_iterations", type=int, default=None, help="snapping: steps and refits")
    p.add_argument("--snap_min_constrained", type=float, default=None,
                   help="snapping: share of an edge's samples that must be constrained for it to take part")
    p.add_argument("--support_check", action="store_true",
                   help="after the export, check every edge of parametric_edges.json along its length against the edge "
                        "maps of the train cameras: edge_support.json and parametric_edges_supported.json in the model "
                        "directory; parametric_edges.json stays as it is (untuned defaults; no depth)")
    p.add_argument("--support_tol_px", type=float, default=None,
                   help="support check: pixel distance to a detected edge within which a sample counts as near")
    p.add_argument("--support_min_near", type=float, default=None,
                   help="support check: share of the samples a view sees that must be near")
    p.add_argument("--support_min_visible", type=float, default=None,
                   help="support check: share of an edge's samples that a view must see")
    p.add_argument("--support_frames_ratio", type=float, default=None,
                   help="support check: an edge is kept when more than ceil(ratio * views) views support it")
    p.add_argument("--trim_edges", action="store_true",
                   help="after the export, cut every edge of parametric_edges.json down to the spans of its length that the "
                        "edge maps of the train cameras show: edge_trim.json and parametric_edges_trimmed.json in the model "
                        "directory; parametric_edges.json stays as it is (untuned defaults; no depth)")
    p.add_argument("--trim_tol_px", type=float, default=None,
                   help="trimming: pixel distance to a detected edge within which a sample counts as near")
    p.add_argument("--trim_max_gap", type=int, default=None,
                   help="trimming: two supported runs at most this many samples apart are merged")
    p.add_argument("--trim_min_span", type=int, default=None, help="trimming: a supported run of fewer samples is dropped")
    p.add_argument("--trim_oriented", action="store_true",
                   help="trimming: a sample counts as near only where a detected pixel within the tolerance runs the way its "
                        "edge does (ops.edge_orient; untuned; thick strokes fall back to the distance test)")
    p.add_argument("--trim_orient_spread", type=int, default=None,
                   help="oriented trimming: the octants of 22.5 degrees to either side that still agree, 0 to 4")
    p.add_argument("--dedupe_edges", action="store_true",
                   help="after the export, drop the parts of the edges that a longer edge already covers in 3D -- of the "
                        "trimmed pieces with --trim_edges, of parametric_edges.json otherwise: edge_dedupe.json and "
                        "parametric_edges_deduped.json in the model directory; the other files stay as they are (untuned "
                        "defaults; the longer edge always wins)")
    p.add_argument("--dedupe_tolerance", type=float, default=None,
                   help="deduping: 3D distance within which a sample of a longer edge covers one (default: 2 x the sampling "
                        "resolution)")
    p.add_argument("--dedupe_cos_min", type=float, default=None,
                   help="deduping: least |cosine| between the two edges' directions for a cover")
    p.add_argument("--dedupe_min_run", type=int, default=None, help="deduping: a run of fewer covered samples is not redundant")
    p.add_argument("--dedupe_min_span", type=int, default=None, help="deduping: a free run of fewer samples is dropped")
    p.add_argument("--join_edges", action="store_true",
                   help="after the export, rejoin the ends of the edges at their junctions in 3D -- of the deduped edges with "
                        "--dedupe_edges, else of the trimmed pieces with --trim_edges, else of parametric_edges.json: "
                        "edge_graph.json and parametric_edges_joined.json in the model directory; the other files stay as "
                        "they are (untuned defaults; hosts of T-junctions are not split, an end joins at most one thing)")
    p.add_argument("--join_tolerance", type=float, default=None,
                   help="joining: 3D distance within which an end attaches in any direction, and the half width of the tube "
                        "ahead of it (default: 2 x the sampling resolution; untuned)")
    p.add_argument("--join_reach", type=float, default=None,
                   help="joining: how far ahead along its tangent an end looks (default: 8 x the sampling resolution; untuned)")
    p.add_argument("--thin_edge_maps", action="store_true",
                   help="thin every view's detected mask (Guo-Hall) before --support_check, --trim_edges, "
                        "--reprojection_score and --init edge_votes compare it with projected geometry: for a detector whose response is several pixels wide "
                        "(untuned; a binary thinning, not non-maximum suppression)")
    return p


def support_options(args):
    """The options of ops.edge_support.edge_support that the command line sets; the rest keep their defaults."""
    opts = {k: v for k, v in (("min_near", args.support_min_near), ("min_visible", args.support_min_visible),
                              ("frames_ratio", args.support_frames_ratio)) if v is not None}
    if args.support_tol_px is not None:
        opts["tolerances_px"] = (args.support_tol_px,)
        opts["keep_tolerance_px"] = args.support_tol_px
    if args.thin_edge_maps:
        opts["thin"] = True
    return opts


def snap_options(args):
    """The options of ops.edge_snap.snap_edges that the command line sets; the rest keep their defaults."""
    opts = {k: v for k, v in (("capture_px", args.snap_capture), ("iterations", args.snap_iterations),
                              ("min_constrained", args.snap_min_constrained)) if v is not None}
    if args.thin_edge_maps:
        opts["thin"] = True
    return opts


def trim_options(args):
    """The options of ops.edge_trim.trim_edges that the command line sets; the rest keep their defaults."""
    opts = {k: v for k, v in (("tolerance_px", args.trim_tol_px), ("max_gap", args.trim_max_gap),
                              ("min_span", args.trim_min_span)) if v is not None}
    if args.thin_edge_maps:
        opts["thin"] = True
    if args.trim_oriented:
        opts["oriented"] = True
        if args.trim_orient_spread is not None:
            opts["spread"] = args.trim_orient_spread
    return opts


def dedupe_options(args):
    """The options of ops.edge_dedupe.dedupe_edges that the command line sets; the rest keep their defaults."""
    return {k: v for k, v in (("tolerance", args.dedupe_tolerance), ("cos_min", args.dedupe_cos_min),
                              ("min_run", args.dedupe_min_run), ("min_span", args.dedupe_min_span)) if v is not None}


def join_options(args):
    """The options of ops.edge_join.join_edges that the command line sets; the rest keep their defaults."""
    return {k: v for k, v in (("tolerance", args.join_tolerance), ("reach", args.join_reach)) if v is not None}


def parse_args(argv):
    """(ModelParams, OptimizationParams, args) of a command line, as :378-404 derives them."""
    parser = build_parser()
    args = parser.parse_args(argv)
    if args.gate_edge_checks and args.occluder is None and args.depth_dir is None:
        parser.error("--gate_edge_checks needs a depth source: --occluder or --depth_dir")
    if args.gate_edge_checks and args.occluder is not None and args.depth_dir is not None:
        parser.error("--gate_edge_checks takes one depth source: --occluder or --depth_dir, not both")
    if args.gate_visibility and args.occluder is None and args.depth_dir is None:
        parser.error("--gate_visibility needs a depth source: --occluder or --depth_dir")
    if args.gate_visibility and args.occluder is not None and args.depth_dir is not None:
        parser.error("--gate_visibility takes one depth source: --occluder or --depth_dir, not both")
    if args.gate_training and (args.occluder is None) == (args.depth_dir is None):
        parser.error("--gate_training needs exactly one depth source: --occluder or --depth_dir")
    if args.gate_training and args.backend == "torch":
        parser.error("--gate_training gates the fused view forward: not with --backend torch")
    if not args.gate_training and (args.train_gate_slack is not None or args.gate_from_iter != 0):
        parser.error("--train_gate_slack and --gate_from_iter belong to --gate_training")
    if args.gate_training and ((args.train_gate_slack is not None and not args.train_gate_slack >= 0) or args.gate_from_iter < 0):
        parser.error("--train_gate_slack and --gate_from_iter are >= 0")
    if args.near_clip is not None and args.occluder is None:
        parser.error("--near_clip needs --occluder: the mesh that is clipped")
    if args.init_near_clip is not None and args.init_occluder is None:
        parser.error("--init_near_clip needs --init_occluder: the mesh that is clipped")
    if args.init_occluder is not None and args.init_depth_dir is not None:
        parser.error("--init edge_votes takes one depth source: --init_occluder or --init_depth_dir, not both")
    if args.ignore_contours and args.occluder is None:
        parser.error("--ignore_contours needs --occluder: the mesh whose contours are predicted")
    source_path = os.path.abspath(args.source_path)                                 # ModelParams.extract (:63-66)
    opt = select_options(source_path, args.detector)()
    if args.visible_checking:
        opt.visible_checking = True
    if args.gate_visibility and not opt.visible_checking:
        parser.error("--gate_visibility gates the export's visibility check, which this run leaves off: give "
                     "--visible_checking too")
    if args.iterations is not None:
        opt.iterations = args.iterations
    args.save_iterations.append(opt.iterations)                                     # :404
    init_options = {k: v for k, v in (("grid", args.init_grid), ("tol_px", args.init_tol_px), ("min_views", args.init_min_views),
                                      ("min_ratio", args.init_min_ratio), ("cell", args.init_cell),
                                      ("dir_radius", args.init_dir_radius), ("dir_min_support", args.init_dir_min_support),
                                      ("dir_min_linearity", args.init_dir_min_linearity),
                                      ("excl_window", args.init_excl_window), ("excl_margin", args.init_excl_margin),
                                      ("excl_win_ratio", args.init_excl_win_ratio), ("occluder", args.init_occluder),
                                      ("depth_dir", args.init_depth_dir), ("depth_slack", args.init_depth_slack),
                                      ("depth_window", args.init_depth_window),
                                      ("near_clip", args.init_near_clip)) if v is not None}
    if args.init_directions:
        init_options["directions"] = True
    if args.init_exclusive:
        init_options["exclusive"] = True
    if args.thin_edge_maps:
        init_options["thin"] = True
    if args.init_bounds is not None:
        init_options["bounds"] = (args.init_bounds[:3], args.init_bounds[3:])
    dataset = ModelParams(source_path, args.model_path, args.sh_degree, args.n_gaussians, args.detector, args.resolution,
                          args.white_background, args.eval, args.undistort, args.init, init_options)
    return dataset, opt, args


def main(argv=None):
    dataset, opt, args = parse_args(sys.argv[1:] if argv is None else argv)
    if not dataset.model_path:
        raise SystemExit("train: -m / --model_path is required")
    print("Optimizing " + dataset.model_path)
    writer = None
    if args.report_dir:
        from .evaluation import ReportDirWriter
        writer = ReportDirWriter(args.report_dir)
    export = None
    if args.gate_visibility:   # the depth maps are one per frame of the scan, found by the frames' names
        cams = None
        if args.depth_dir is not None:
            from .edge_extraction.reprojection import emap_cameras
            cams = emap_cameras(dataset.source_path, dataset.detector)[0]
        vis = gate_options(args, dataset.source_path, cams, flag="gate_visibility")
        export = lambda g, d, o: _export(g, d, o, vis)
    train_gate = {}
    if args.gate_training:
        train_gate = dict(train_gate=lambda cams: train_gate_options(args, dataset.source_path, cams),
                          gate_from_iter=args.gate_from_iter)
    out = training(dataset, opt, args.test_iterations, args.save_iterations, args.checkpoint_iterations, args.start_checkpoint,
                   backend=args.backend, seed=args.seed, quiet=args.quiet, draw=args.draw_snapshots,
                   topology_backend=args.topology_backend, report_writer=writer, export=export, **train_gate)
    if args.reprojection_score:
        from .edge_extraction.reprojection import scan_line, score_scene
        gate = {}
        if args.occluder is not None or args.depth_dir is not None:
            gate = dict(depth_slack=args.depth_slack, depth_window=args.depth_window)
            if args.occluder is not None:
                gate["occluder"] = os.path.join(dataset.source_path, args.occluder)
            if args.depth_dir is not None:
                gate["depth_dir"] = os.path.join(dataset.source_path, args.depth_dir)
        if args.near_clip is not None:   # (score_edges rejects it without an occluder)
            gate["near_clip"] = args.near_clip
        from .edge_extraction.reprojection import contour_options
        scores = score_scene(dataset.model_path, out["scene"], dataset.detector,
                             **({"thin": True} if args.thin_edge_maps else {}), **gate,
                             **contour_options(args.ignore_contours, args.contour_radius_px, args.crease_deg))
        for split, res in scores.items():
            if res is not None:
                print(scan_line(split, res["aggregate"]))
    if args.snap_edges or args.support_check or args.trim_edges or args.dedupe_edges or args.join_edges:
        export_checks(args, dataset.model_path, out["scene"].getTrainCameras(), dataset.detector,
                      source_path=dataset.source_path)
    print("\nTraining complete.")


def gate_options(args, source_path, cameras, flag="gate_edge_checks"):
    """The depth keywords of the chain's 2D steps under --gate_edge_checks: ``occluder`` (the mesh inside ``source_path``) or
    ``depth_maps`` (``<source_path>/<depth_dir>/<image stem>.npy`` of ``cameras``, NovelViewCamera s), and the slack and the
    window; {} without the flag.  ``flag="gate_visibility"``: the same keywords for the export's visibility check
    (``write_parametric_edges(visibility_options=)``; ``cameras`` are then the scan's frames)."""
    if not getattr(args, flag, False):
        return {}
    if args.occluder is not None and args.depth_dir is not None:
        raise ValueError("--gate_edge_checks: give --occluder or --depth_dir, not both")
    gate = dict(depth_slack=args.depth_slack, depth_window=args.depth_window)
    if args.occluder is not None:
        gate["occluder"] = os.path.join(source_path, args.occluder)
    else:
        from .edge_extraction.reprojection import scan_depth_maps
        gate["depth_maps"] = scan_depth_maps(os.path.join(source_path, args.depth_dir), cameras)
    if getattr(args, "near_clip", None) is not None:   # (the operators reject it without an occluder)
        gate["near_clip"] = args.near_clip
    return gate


def train_gate_options(args, source_path, cameras):
    """The keywords of ``ops.train_gate.TrainGate`` under --gate_training: ``gate_options`` of the train cameras (a Scene's;
    the depth maps of --depth_dir are found by their names), with --train_gate_slack in place of the slack when it is given."""
    from .edge_extraction.reprojection import scene_cameras
    gate = gate_options(args, source_path, scene_cameras(cameras)[0], flag="gate_training")
    if args.train_gate_slack is not None:
        gate["depth_slack"] = args.train_gate_slack
    return gate


def export_checks(args, model_path, cameras, detector, edge_maps=None, source_path=None):
    """The opt-in steps after the export, on ``<model_path>/parametric_edges.json`` and the train cameras (``edge_maps``
    None: a Scene's cameras carry their maps): --snap_edges first, then --support_check, --trim_edges, --dedupe_edges and
    --join_edges, each from the last product of the chain.  With --gate_edge_checks the first three take the depth source
    of --occluder / --depth_dir inside ``source_path`` (``gate_options``)."""
    import json
    from .edge_extraction.support import (DEDUPED_FILE, SNAPPED_FILE, TRIMMED_FILE, dedupe_scene, join_scene, snap_scene,
                                          support_scene, trim_scene)
    with open(os.path.join(model_path, "parametric_edges.json")) as f:
        edge_dict = json.load(f)
    source, named = "parametric_edges.json", {}
    gate = {}
    if getattr(args, "gate_edge_checks", False):
        if edge_maps is None:   # the depth maps are found by the cameras' names
            from .edge_extraction.reprojection import scene_cameras
            cameras, edge_maps = scene_cameras(cameras)
        gate = gate_options(args, source_path, cameras)
    if args.snap_edges:
        edge_dict, _ = snap_scene(model_path, edge_dict, cameras, edge_maps, detector, **snap_options(args), **gate)
        source, named = SNAPPED_FILE, {"input_file": SNAPPED_FILE}
    if args.support_check:
        support_scene(model_path, edge_dict, cameras, edge_maps, detector, **named, **support_options(args), **gate)
    if args.trim_edges:
        trimmed, _ = trim_scene(model_path, edge_dict, cameras, edge_maps, detector, **named, **trim_options(args), **gate)
    if args.dedupe_edges:
        deduped, _ = dedupe_scene(model_path, trimmed if args.trim_edges else edge_dict,
                                  input_file=TRIMMED_FILE if args.trim_edges else source, **dedupe_options(args))
    if args.join_edges:
        given, name = ((deduped, DEDUPED_FILE) if args.dedupe_edges else (trimmed, TRIMMED_FILE) if args.trim_edges else
                       (edge_dict, source))
        join_scene(model_path, given, input_file=name, **join_options(args))


if __name__ == "__main__":
    main()
