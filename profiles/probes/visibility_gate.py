"""python profiles/probes/visibility_gate.py [--views 100] [--width 1600] [--height 1200] [--curves 12000] [--lines 8000]
                                              [--edges 4000] [--samples 100] [--grid 224] [--reps 20] [--host_views 2]
                                              [--check_edges 2000] [--parent_lib FILE] [--out FILE]

Times the depth-gated control-point visibility check and the depth-gated drawn views beside their ungated siblings
(profiles/visibility_gate.md): ``cgs_edge_visibility_depth`` beside ``cgs_edge_visibility`` on ``--curves`` + ``--lines``
random edges of the unit cube in ``--views`` cameras on a sphere around it, and ``cgs_render_points_depth`` beside
``cgs_render_points`` on the samples of profiles/probes/edge_dedupe.py (400 708 at the defaults) in the same cameras.  The
depth is the z-buffer of the fine sphere of profiles/probes/edge_occlusion.py (2 x grid x grid triangles) with the default
window, so part of the points is hidden.  Everything resident, raw calls between device events after a warm-up, the variants
alternating within each of three rounds.

``--parent_lib``: a ``libcurvegs.so`` built from the commit before the gate.  Its two ungated entries are loaded beside this
build's, asserted to write the same bits, and timed in the same rounds: "the existing kernels did not get slower" is judged
against them.  Without it that comparison is NOT MEASURED and the output says so.

Before anything is timed the gated counts of the first ``--check_edges`` curves and lines in the first ``--host_views`` views
are compared with the host back end bit for bit, and kept + hidden of the gated render with the ungated render's kept."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from edge_dedupe import straight_edges  # noqa: E402  (the sibling probes: the same inputs)
from edge_occlusion import sphere_mesh  # noqa: E402
from edge_orient import sphere_cameras  # noqa: E402
from edge_support import events_ms  # noqa: E402
from edge_thin import dilate, segment_views  # noqa: E402

UNGATED = ("cgs_edge_visibility", "cgs_render_points")


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--views", type=int, default=100)
    p.add_argument("--width", type=int, default=1600)
    p.add_argument("--height", type=int, default=1200)
    p.add_argument("--curves", type=int, default=12000)
    p.add_argument("--lines", type=int, default=8000)
    p.add_argument("--edges", type=int, default=4000)
    p.add_argument("--samples", type=int, default=100)
    p.add_argument("--grid", type=int, default=224)
    p.add_argument("--distinct", type=int, default=10)
    p.add_argument("--segments", type=int, default=150)
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--host_views", type=int, default=2)
    p.add_argument("--check_edges", type=int, default=2000)
    p.add_argument("--parent_lib", default=None)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    import torch
    from curve_gaussian_amd import _lib as L
    from curve_gaussian_amd.edge_extraction import para_edge as PE
    from curve_gaussian_amd.ops import edge_occlusion as EO
    from curve_gaussian_amd.ops import edge_score as ES
    if not torch.cuda.is_available():
        raise SystemExit("visibility_gate: needs a GPU; nothing is measured without one")
    dev = torch.device("cuda", 0)
    H, W, V = a.height, a.width, a.views
    lib, stream, ptr = L.load(), L.raw_stream(dev), L.ptr
    K4, M = sphere_cameras(V, H, W)
    depth = EO.mesh_depth(sphere_mesh(a.grid), K4, M, H, W, EO.DEPTH_WINDOW, backend="gpu", device=dev)
    slack = EO.DEPTH_SLACK
    strokes = dilate(segment_views(min(a.distinct, V), H, W, a.segments), 1)   # three-pixel strokes
    maps = (np.tile(strokes, (-(-V // strokes.shape[0]), 1, 1))[:V] * np.uint8(255)).astype(np.uint8)   # PidiNet bytes
    g = np.random.default_rng(0)
    curves, lines = g.uniform(0.0, 1.0, (a.curves, 4, 3)), g.uniform(0.0, 1.0, (a.lines, 2, 3))
    K3 = np.zeros((V, 3, 3))
    K3[:, 0, 0], K3[:, 1, 1], K3[:, 0, 2], K3[:, 1, 2], K3[:, 2, 2] = K4[:, 0], K4[:, 1], K4[:, 2], K4[:, 3], 1.0
    c2w = np.tile(np.eye(4), (V, 1, 1))
    c2w[:, :3] = M
    c2w = np.linalg.inv(c2w)   # (the operators invert it again; the raw calls below take M itself)

    # equality with the host back end first
    hv, ce = max(1, min(a.host_views, V)), a.check_edges
    args = (curves[:ce], lines[:ce], maps[:hv], K3[:hv], c2w[:hv], "PidiNet")
    host = PE.edge_visibility_counts_depth(*args, depth[:hv].cpu(), slack, backend="host").numpy()
    got = PE.edge_visibility_counts_depth(*args, depth[:hv], slack, backend="gpu", device=dev).cpu().numpy()
    assert got.tobytes() == host.tobytes(), "cgs_edge_visibility_depth disagrees with its host back end"

    E = a.curves + a.lines
    pts, _ = straight_edges(a.edges, a.samples, 0.001)
    P = len(pts)
    col = g.uniform(0.0, 1.0, (P, 3)).astype(np.float32)
    Kd, Md = ES.cameras_on(dev, K4, np.ascontiguousarray(M.reshape(V, 12)))
    K3d = torch.from_numpy(K3).to(dev)
    maps_d, curves_d, lines_d = torch.from_numpy(maps).to(dev), torch.from_numpy(curves).to(dev), torch.from_numpy(lines).to(dev)
    pts_d, col_d = torch.from_numpy(pts).to(dev), torch.from_numpy(col).to(dev)
    bg = np.ones(3, np.float64)
    bgp = bg.ctypes.data_as(ctypes.c_void_p)
    ws_bytes = lib.cgs_render_points_workspace_bytes(P, V, H, W)
    ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=dev)   # one workspace: the calls run one after the other
    image = torch.empty((V, H, W, 3), dtype=torch.float32, device=dev)   # one image buffer, likewise
    z = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=dev)

    def entries(lib, gated, tag):
        """name -> (call, outputs): the two entries of ``lib`` on counters of their own."""
        sfx = "_depth" if gated else ""
        counts, kept, hidden = z(E, 2) if gated else z(E), z(V), z(V)
        gate = (ptr(depth), slack) if gated else ()
        out = {
            "edge_visibility": (lambda: getattr(lib, "cgs_edge_visibility" + sfx)(
                a.curves, ptr(curves_d), a.lines, ptr(lines_d), V, ptr(K3d), ptr(Md), H, W, ptr(maps_d), 0, *gate, ptr(counts),
                stream), (counts,)),
            "render_points": (lambda: getattr(lib, "cgs_render_points" + sfx)(
                P, ptr(pts_d), ptr(col_d), V, ptr(Kd), ptr(Md), H, W, *gate, 0.5, bgp, ptr(image), ptr(kept),
                *((ptr(hidden),) if gated else ()), ptr(ws), ws_bytes, stream), (kept, hidden))}
        return {f"{name}{sfx} [{tag}]": v for name, v in out.items()}

    table = {**entries(lib, False, "this build"), **entries(lib, True, "this build")}
    if a.parent_lib:
        parent = ctypes.CDLL(os.path.abspath(a.parent_lib))
        for name in UNGATED:
            getattr(parent, name).restype, getattr(parent, name).argtypes = L.SIGNATURES[name]
        table.update(entries(parent, False, "parent"))
    sums = {}
    for name, (call, _) in table.items():   # the warm-up; the one image buffer is summed after each render
        assert call() == 0, name
        torch.cuda.synchronize()
        if name.startswith("render_points"):
            sums[name] = image.view(torch.int32).to(torch.int64).sum().item()   # the bits, summed as integers
    bits = {name: [t.cpu().numpy().tobytes() for t in outs] for name, (_, outs) in table.items()}
    if a.parent_lib:
        for k in ("edge_visibility", "render_points"):
            assert bits[f"{k} [parent]"] == bits[f"{k} [this build]"], f"cgs_{k}: this build and the parent write different bits"
        assert sums["render_points [parent]"] == sums["render_points [this build]"], "cgs_render_points: the images differ"
    plain = table["edge_visibility [this build]"][1][0].cpu().numpy()
    gated = table["edge_visibility_depth [this build]"][1][0].cpu().numpy()
    kept0 = table["render_points [this build]"][1][0].cpu().numpy().astype(np.int64)
    kept1, hid1 = (t.cpu().numpy().astype(np.int64) for t in table["render_points_depth [this build]"][1])
    assert (kept1 + hid1 == kept0).all(), "kept + hidden of the gated render is not the ungated kept"
    print(f"{E} edges x {V} views {W}x{H}: gated check equal to the host back end on 2 x {ce} edges x {hv} views; visible cells "
          f"{int(plain.sum())} ungated, {int(gated[:, 0].sum())} gated; the gate dropped a point in {int(gated[:, 1].sum())} of "
          f"{E * V} cells ({gated[:, 1].sum() / (E * V):.1%}).  {P} samples: {int(kept0.sum())} kept sample-views, "
          f"{int(hid1.sum())} of them hidden ({hid1.sum() / max(kept0.sum(), 1):.1%}); ungated entries "
          + ("bit-equal to the parent build's" if a.parent_lib else "NOT compared with a parent build (no --parent_lib)"), flush=True)
    ms = {name: [] for name in table}
    for _ in range(3):
        for name, (call, _) in table.items():
            ms[name].append(events_ms(torch, call, a.reps))
    for name, t in ms.items():
        print(f"  {name}: {[round(x, 4) for x in t]} ms per call over {a.reps} calls each", flush=True)
    result = {"views": V, "width": W, "height": H, "edges": E, "points": P, "reps": a.reps, "rounds": 3,
              "visible_cells": int(plain.sum()), "visible_cells_gated": int(gated[:, 0].sum()), "touched_cells": int(gated[:, 1].sum()),
              "kept": int(kept0.sum()), "hidden": int(hid1.sum()), "parent": bool(a.parent_lib), "ms": ms,
              "device": torch.cuda.get_device_name(dev)}
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
