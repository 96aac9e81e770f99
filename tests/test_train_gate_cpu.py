"""CPU: the depth gate of the training render -- the two gated entries are declared, bound and exported; every rejection of
the gate's arguments returns its status and a message before anything could be launched; the driver's parser errors fire;
``TrainGate`` draws, on the host, the planes ``mesh_depth`` draws for the same cameras; the shared cases hold what they claim."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import train_gate_cases as TG

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A = ctypes.c_void_p(64)          # a dummy pointer, 16-byte aligned, never dereferenced
NAN, INF = float("nan"), float("inf")
ENTRIES = ("cgs_view_forward_depth", "cgs_view_forward_render_depth")

_FWD = ("B m curve_points width is_bezier coef eps norms opacity_logit mask_logit mask_thr colors_precomp geometry_buffer "
        "binning_buffer binning_bytes image_buffer bucket_capacity background width_px height_px viewmatrix projmatrix cam_pos "
        "tan_fovx tan_fovy out_color out_invdepth out_all_map radii xyz rotation scaling gate stream")
_RENDER = ("checked B m curve_points width is_bezier coef eps norms opacity_logit mask_logit mask_thr geometry_buffer "
           "binning_buffer binning_bytes image_buffer bucket_capacity background width_px height_px viewmatrix projmatrix "
           "cam_pos tan_fovx tan_fovy out_color out_invdepth out_all_map radii out_color_clamped out_rend_dir gate stream")
_BASE = dict(B=5, m=12, eps=1e-8, mask_logit=None, mask_thr=0.5, binning_bytes=1 << 30, bucket_capacity=64, width_px=64,
             height_px=48, tan_fovx=0.3, tan_fovy=0.3, stream=None)
_ARGS = {"cgs_view_forward_depth": (_FWD, dict(_BASE, colors_precomp=None)),
         "cgs_view_forward_render_depth": (_RENDER, dict(_BASE, checked=0))}
_GATE = dict(planes=64, intr=64, w2c=64, view_index=None, slack=0.5, V=3, view=1, height=48, width=64)


def _call(lib, fn, changes=None, gate=None, no_gate=False):
    from curve_gaussian_amd import _lib
    names, base = _ARGS[fn]
    names = names.split()
    assert len(names) == len(_lib.SIGNATURES[fn][1])
    vg = _lib.ViewGate(**dict(_GATE, **(gate or {})))
    values = dict({n: A for n in names}, **base)
    values["gate"] = None if no_gate else ctypes.byref(vg)
    values.update(changes or {})
    rc = getattr(lib, fn)(*[values[n] for n in names])
    return rc, lib.cgs_last_error().decode()


def test_the_two_gated_entries_are_declared_bound_and_exported():
    from curve_gaussian_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "curvegs.h")).read(), flags=re.S)
    lib = _lib.load()
    for fn, sibling in zip(ENTRIES, ("cgs_view_forward", "cgs_view_forward_render")):
        assert re.search(r"\bint\s+%s\s*\(" % fn, src), fn
        assert hasattr(lib, fn) and fn in _lib.SIGNATURES
        res, args = _lib.SIGNATURES[fn]
        s_res, s_args = _lib.SIGNATURES[sibling]
        assert res is s_res and args == s_args[:-1] + [ctypes.c_void_p, s_args[-1]]   # the sibling's, the gate before the stream
    assert "typedef struct cgs_view_gate" in src
    # the struct's layout is the header's: four pointers, a double, four int32
    assert ctypes.sizeof(_lib.ViewGate) == 4 * 8 + 8 + 4 * 4
    assert [f[0] for f in _lib.ViewGate._fields_] == ["planes", "intr", "w2c", "view_index", "slack", "V", "view", "height",
                                                      "width"]
    # no gated sibling for the shared, checked and two-halves forwards, and the header says so
    for fn in ("cgs_view_forward_shared_depth", "cgs_view_forward_checked_depth", "cgs_view_forward_begin_depth"):
        assert fn not in src and fn not in _lib.SIGNATURES and not hasattr(lib, fn)
    doc = open(os.path.join(ROOT, "include", "curvegs.h")).read()
    assert "cgs_view_forward_shared, cgs_view_forward_checked and cgs_view_forward_begin get NO gated sibling" in doc


@pytest.mark.parametrize("fn", ENTRIES)
def test_every_rejection_of_the_gate_returns_its_status_and_a_message(fn):
    """No GPU is touched: every row is rejected by the checks in front of the first launch (this file runs on GPU machines
    too, where a row that slipped through would launch on address 64)."""
    from curve_gaussian_amd import _lib
    lib = _lib.load()
    inv = f"{fn}: invalid argument "
    rows = [
        (dict(no_gate=True), inv + "(NULL gate)"),
        (dict(gate=dict(planes=None)), inv + "(NULL plane or camera pointer)"),
        (dict(gate=dict(intr=None)), inv + "(NULL plane or camera pointer)"),
        (dict(gate=dict(w2c=None)), inv + "(NULL plane or camera pointer)"),
        (dict(gate=dict(V=0)), inv + "(V=0; the stack holds at least one view)"),
        (dict(gate=dict(V=-2)), inv + "(V=-2; the stack holds at least one view)"),
        (dict(gate=dict(view=-1)), inv + "(view=-1 outside [0, 3))"),
        (dict(gate=dict(view=3)), inv + "(view=3 outside [0, 3))"),
        (dict(gate=dict(slack=-0.5)), inv + "(slack=-0.5; the slack is >= 0)"),
        (dict(gate=dict(slack=NAN)), inv + "(slack=nan; the slack is >= 0)"),
        (dict(gate=dict(height=47)), inv + "(planes 64x47, image 64x48; the planes have the image's size)"),
        (dict(gate=dict(width=48, height=64)), inv + "(planes 48x64, image 64x48; the planes have the image's size)"),
        # +inf is a slack (it hides nothing): the row is rejected by the NEXT check, the size
        (dict(gate=dict(slack=INF, width=63)), inv + "(planes 63x48, image 64x48; the planes have the image's size)"),
        # a device view index takes the place of the host view: an out-of-range `view` is then not looked at
        (dict(gate=dict(view_index=64, view=99, width=63)), inv + "(planes 63x48, image 64x48; the planes have the image's size)"),
        # the order: the pointers before V, V before the view, the view before the slack, the slack before the size
        (dict(gate=dict(planes=None, V=0)), inv + "(NULL plane or camera pointer)"),
        (dict(gate=dict(V=0, view=7)), inv + "(V=0; the stack holds at least one view)"),
        (dict(gate=dict(view=7, slack=-1.0)), inv + "(view=7 outside [0, 3))"),
        (dict(gate=dict(slack=-1.0, height=1)), inv + "(slack=-1; the slack is >= 0)"),
        # the sibling's own checks come first, under the sibling's name; the bucket capacity comes after the gate
        (dict(changes=dict(B=0), gate=dict(V=0)),
         "cgs_view_forward: invalid argument (B=0 m=12 W=64 H=48, NULL / misaligned pointer or zero capacity)"),
        (dict(changes=dict(radii=None), no_gate=True),
         "cgs_view_forward: invalid argument (B=5 m=12 W=64 H=48, NULL / misaligned pointer or zero capacity)"),
        (dict(changes=dict(binning_bytes=4096), gate=dict(slack=-0.5)), inv + "(slack=-0.5; the slack is >= 0)"),
    ]
    for kw, message in rows:
        rc, text = _call(lib, fn, **kw)
        assert rc == -1 and text == message, (fn, kw, rc, text)
    # a valid gate leaves the sibling's remaining check, the capacity, in place (and still nothing is launched)
    rc, text = _call(lib, fn, changes=dict(binning_bytes=4096))
    assert rc == -1 and text.startswith("cgs_view_forward: bucket capacity 64 needs "), text


def test_the_driver_rejects_bad_gate_flags(capsys):
    from curve_gaussian_amd import train as T
    base = ["-s", "scan", "-m", "out"]
    for extra, text in ((["--gate_training"], "--gate_training needs exactly one depth source"),
                        (["--gate_training", "--occluder", "mesh.ply", "--depth_dir", "depth"],
                         "--gate_training needs exactly one depth source"),
                        (["--gate_training", "--occluder", "mesh.ply", "--backend", "torch"], "not with --backend torch"),
                        (["--train_gate_slack", "0.01"], "belong to --gate_training"),
                        (["--gate_from_iter", "5"], "belong to --gate_training"),
                        (["--gate_training", "--occluder", "mesh.ply", "--train_gate_slack", "-1"], "are >= 0"),
                        (["--gate_training", "--occluder", "mesh.ply", "--gate_from_iter", "-3"], "are >= 0")):
        with pytest.raises(SystemExit) as e:
            T.parse_args(base + extra)
        assert e.value.code == 2 and text in capsys.readouterr().err, extra
    _, _, args = T.parse_args(base)
    assert not args.gate_training and args.train_gate_slack is None and args.gate_from_iter == 0      # OFF BY DEFAULT
    _, _, args = T.parse_args(base + ["--gate_training", "--occluder", "mesh.ply", "--train_gate_slack", "0.004",
                                      "--gate_from_iter", "40", "--near_clip"])
    assert args.gate_training and args.train_gate_slack == 0.004 and args.gate_from_iter == 40
    # the options the gate is built from: gate_options' keywords, the slack replaced
    gate = T.train_gate_options(args, "/scan", [])
    from curve_gaussian_amd.ops.edge_occlusion import NEAR_CLIP
    assert gate == dict(depth_slack=0.004, depth_window=args.depth_window, occluder="/scan/mesh.ply", near_clip=NEAR_CLIP)
    _, _, args = T.parse_args(base + ["--gate_training", "--occluder", "mesh.ply"])
    from curve_gaussian_amd.ops.edge_occlusion import DEPTH_SLACK
    assert T.train_gate_options(args, "/scan", [])["depth_slack"] in (None, DEPTH_SLACK)   # the chain's default, untuned


@pytest.fixture(scope="module")
def box():
    return TG.box_scan()


def test_train_gate_on_the_host_draws_the_planes_of_mesh_depth(box):
    from curve_gaussian_amd.ops import edge_occlusion as EO
    from curve_gaussian_amd.ops.train_gate import TrainGate
    from curve_gaussian_amd.ops.view_chunks import camera_arrays
    gate = TrainGate(box.cameras, occluder=box.tris, backend="host")
    intr, w2c = camera_arrays(box.cameras)
    want = EO.mesh_depth(box.tris, intr, w2c, 60, 80, window=EO.DEPTH_WINDOW, backend="host")
    want = want if torch.is_tensor(want) else torch.from_numpy(np.asarray(want))
    assert gate.planes.dtype == torch.float32 and tuple(gate.planes.shape) == (6, 60, 80) == (gate.V, gate.height, gate.width)
    assert torch.equal(gate.planes, want.cpu())
    assert bool(torch.isfinite(gate.planes).any()) and bool(torch.isinf(gate.planes).any())       # the solid and the sky
    assert gate.planes_bytes == 6 * 60 * 80 * 4 == gate.planes.numel() * 4
    assert gate.slack == EO.DEPTH_SLACK and gate.window == EO.DEPTH_WINDOW and gate.near is None   # the chain's defaults
    assert np.array_equal(gate.intr.numpy(), intr) and np.array_equal(gate.w2c.numpy(), w2c.reshape(6, 12))
    assert gate.settings() == {"occluder": True, "depth_slack": EO.DEPTH_SLACK, "depth_window": EO.DEPTH_WINDOW,
                               "planes_bytes": 115200}
    # the caller's maps instead: the same stack after the window maximum
    raw = EO.mesh_depth(box.tris, intr, w2c, 60, 80, window=0, backend="host")
    raw = raw.numpy() if torch.is_tensor(raw) else np.asarray(raw)
    from_maps = TrainGate(box.cameras, depth_maps=[p for p in raw], backend="host")
    assert torch.equal(from_maps.planes, gate.planes)
    # the renderer's own cameras give the same intrinsics (the field of view at the image's size, the centre)
    synth = TrainGate(box.synth_cameras, occluder=box.tris, backend="host")
    assert np.array_equal(synth.intr.numpy(), intr) and np.allclose(synth.w2c.numpy(), w2c.reshape(6, 12), atol=1e-6)


def test_train_gate_refuses_what_it_cannot_hold(box):
    from curve_gaussian_amd.ops.train_gate import TrainGate
    with pytest.raises(ValueError, match="exactly one depth source"):
        TrainGate(box.cameras, backend="host")
    with pytest.raises(ValueError, match="exactly one depth source"):
        TrainGate(box.cameras, occluder=box.tris, depth_maps=[box.depth[v] for v in range(6)], backend="host")
    mixed = list(box.cameras[:5]) + [box.cameras[5]._replace(width=64)]
    with pytest.raises(ValueError, match="mixed image sizes"):
        TrainGate(mixed, occluder=box.tris, backend="host")
    with pytest.raises(ValueError, match=r"need 115200 bytes, over the budget of 100000"):
        TrainGate(box.cameras, occluder=box.tris, backend="host", max_bytes=100000)
    with pytest.raises(ValueError, match="slack"):
        TrainGate(box.cameras, occluder=box.tris, backend="host", depth_slack=-1.0)
    with pytest.raises(ValueError, match="near_clip needs an occluder"):
        TrainGate(box.cameras, depth_maps=[box.depth[v] for v in range(6)], backend="host", near_clip=0.01)
    gate = TrainGate(box.cameras, occluder=box.tris, backend="host")
    for bad in (-1, 6):
        with pytest.raises(ValueError, match=r"outside \[0, 6\)"):
            gate.view_args(bad)
    with pytest.raises(ValueError, match="one-element int32 tensor"):
        gate.view_args(torch.zeros(1, dtype=torch.int64))
    with pytest.raises(ValueError, match="the planes are 80x60, the view is 64x60"):
        gate.check(60, 64, torch.device("cpu"))
    with pytest.raises(ValueError, match="the planes are on cpu"):     # a host gate must be uploaded before it gates a render
        gate.check(60, 80, torch.device("cuda:0"))


def test_the_steps_reject_the_gate_where_it_cannot_apply(box):
    from curve_gaussian_amd.ops.train_gate import TrainGate
    from curve_gaussian_amd.train_step import TrainStep
    gate = TrainGate(box.cameras, occluder=box.tris, backend="host")
    cams = list(box.synth_cameras)
    with pytest.raises(ValueError, match="world > 1"):       # (raised before the model is looked at)
        TrainStep(None, cams, [], world=2, depth_gate=gate)
    with pytest.raises(ValueError, match="fused=True"):
        TrainStep(None, cams, [], fused=False, depth_gate=gate)
    with pytest.raises(ValueError, match="6 planes, the loop 5 cameras"):
        TrainStep(None, cams[:5], [], depth_gate=gate)


def test_the_tally_of_dead_splats(box):
    """splat_visibility on the box: a point inside the solid is hidden by every view that sees it (dead), a point on a corner
    is seen and hidden by some, a point far outside every frustum is seen by none and is not dead."""
    from curve_gaussian_amd.ops.train_gate import TrainGate, splat_visibility
    gate = TrainGate(box.cameras, occluder=box.tris, backend="host")
    pts = np.array([[0.5, 0.5, 0.5], [0.2, 0.25, 0.3], [50.0, 50.0, 50.0]], np.float32)
    seen, hidden, dead = splat_visibility(pts, gate)
    assert seen[0] == 6 and hidden[0] == 6 and dead[0]
    assert seen[1] == 6 and 0 < hidden[1] < 6 and not dead[1]
    assert seen[2] == 0 and hidden[2] == 0 and not dead[2]


def test_the_report_of_a_gated_run(box, tmp_path):
    """train_gate.json from the final centres: per view what point_masks_depth counts, per splat the tally, the dead ones."""
    import json
    from types import SimpleNamespace
    from curve_gaussian_amd import train as T
    from curve_gaussian_amd.ops.train_gate import TrainGate, splat_visibility
    gate = TrainGate(box.cameras, occluder=box.tris, backend="host")
    pts = torch.tensor([[0.5, 0.5, 0.5], [0.2, 0.25, 0.3], [50.0, 50.0, 50.0], [0.8, 0.75, 0.7]])
    path = str(tmp_path / "train_gate.json")
    out = T.write_train_gate_report(path, SimpleNamespace(get_xyz=pts), gate, gate_from_iter=7, backend="host")
    assert json.load(open(path)) == out
    seen, hidden, dead = splat_visibility(pts, gate)
    assert out["splats"] == 4 and out["seen_views"] == seen.tolist() and out["hidden_views"] == hidden.tolist()
    assert out["dead"] == 1 and out["dead_splats"] == [0] and out["never_seen"] == 1
    assert out["hidden_somewhere"] == int((hidden > 0).sum()) >= 2
    assert [v["kept"] + v["hidden"] for v in out["views"]] == [3] * 6           # three of the four centres are in every image
    assert sum(v["hidden"] for v in out["views"]) == int(hidden.sum())          # the operator and the host tally agree
    assert out["settings"]["gate_from_iter"] == 7 and out["settings"]["planes_bytes"] == 115200


def test_the_shared_cases_hold_what_they_claim():
    """The GPU tests' scene on the CPU (the torch restatement of the curve sampling): off-image centres, centres behind the
    camera, a view that hides every in-image centre, and hidden centres for the NaN and the +inf to sit under."""
    from curve_gaussian_amd.ops.edge_occlusion import gate_view_host
    from curve_gaussian_amd.ops.train_gate import gate_cameras
    from curve_gaussian_amd.ops.view_chunks import camera_arrays
    from oracle import torch_ref as TR
    assert (TG.H % 16, TG.W % 16) != (0, 0) and [12 * b for b in TG.SIZES] == [240, 264]
    K, M = camera_arrays(gate_cameras(TG.cameras()))
    M = M.reshape(3, 12)
    for B in TG.SIZES:
        c = TG.curves(B)
        xyz = TR.prepare_scaling_rot(c["curve_points"], c["width"], c["is_bezier"])[0].numpy()
        stack = torch.from_numpy(TG.planes())
        TG.poke(stack, xyz, K, M)
        assert int(torch.isnan(stack[0]).sum()) == 1 and int(torch.isinf(stack[0]).sum()) == 1
        X = xyz.astype(np.float64)
        per_view = []
        for v in range(3):
            _u, _v, seen, hid = gate_view_host(xyz, K[v], M[v], stack[v].numpy(), TG.SLACK)
            c2 = X @ M[v][8:11] + M[v][11]
            per_view.append((seen, hid, c2))
        seen0, hid0, _ = per_view[0]
        assert 0 < hid0.sum() < (seen0 | hid0).sum()                       # the ramp hides some of what view 0 keeps
        seen1, hid1, c21 = per_view[1]
        assert hid1.sum() > 0 and seen1.sum() == 0                         # in front of everything: all kept centres hidden
        assert ((c21 > 0) & ~(seen1 | hid1)).sum() >= 12                   # centres in front of the camera but off the image
        seen2, hid2, c22 = per_view[2]
        assert (c22 <= 0).sum() >= 12 and 0 < hid2.sum() and seen2.sum() > 0   # centres behind the camera
