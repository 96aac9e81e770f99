"""python profiles/probes/tsdf_mesh.py [--timing] [--views 100] [--width 1600] [--height 1200] [--grid 256] [--reps 10]
                                      [--geometry_lib FILE] [--box] [--stereo box cylinder ...] [--out FILE]

The measurements of profiles/tsdf_mesh.md, on one GPU.

TIMING (``--timing``).  Integration: the box seen by ``--views`` cameras of ``--width`` x ``--height`` on a sphere, the planes
``cgs_mesh_depth`` with the default window -- the workload of profiles/edge_seed_gate.md --, a lattice of ``--grid`` points a
side over the unit cube, trunc 4 steps.  ``cgs_voxel_votes_depth`` runs in the same rounds as the yardstick (the same walk
and the same gather).  Everything resident, raw calls between device events after a warm-up, three rounds of ``--reps``
calls, the entries alternating within a round.  With ``--geometry_lib`` (built from profiles/probes/tsdf_geometries.hip) the
linear (baseline) geometry runs beside the library's kernel after its state is compared with the library's bit for bit.  Then the same
on SPARSE maps: the planes with a depth kept at 6 % of the pixels (0 elsewhere).  Extraction: cgs_tsdf_mesh_count, the scan
and cgs_tsdf_mesh_emit on the analytic field of a sphere of radius 0.3 on the same lattice.

QUALITY.  ``--box``: the end-to-end fixture of tests/tsdf_cases.py (12 views of 80 x 60, exact maps, lattice 48^3) -- the
depth error of the TSDF mesh, the (sample, view) pairs the two gates hide, the ground truth scored at 1 px.
``--stereo SHAPE ...``: the stereo chain at 24 views of 320 x 240 with the defaults (the scan of profiles/stereo_fuse.md),
the fused maps into ``tsdf_mesh`` at the defaults, the fused maps' own gate beside the TSDF mesh's; on the cylinder also with
``ignore_contours`` and the number of edges ``smooth()`` takes for contours at 30 degrees."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from edge_seed_exclusive import events_ms  # noqa: E402  (the sibling probe's timer)

BOUNDS = ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))


def timing(a):
    import torch
    from curve_gaussian_amd import _lib as L
    from curve_gaussian_amd.ops import edge_occlusion as EO
    from curve_gaussian_amd.ops import edge_score as ES
    from curve_gaussian_amd.ops import edge_seed as SEED
    from curve_gaussian_amd.ops import tsdf as TS
    from curve_gaussian_amd.ops.view_chunks import camera_arrays
    from curve_gaussian_amd.scene.solid_scan import solid_scan
    dev = torch.device("cuda", 0)
    on = dict(backend="gpu", device=dev)
    H, W, V = a.height, a.width, a.views
    scan = solid_scan("box", V, H, W, **on)
    intr, w2c = camera_arrays(scan.cameras)
    dense = EO.mesh_depth(scan.tris, intr, w2c, H, W, EO.DEPTH_WINDOW, **on)
    g = torch.Generator(device=dev).manual_seed(0)
    sparse = torch.where(torch.rand(dense.shape, device=dev, generator=g) < 0.06,
                         torch.where(torch.isfinite(dense), dense, torch.full_like(dense, 2.0)), torch.zeros_like(dense))
    per = max(1, SEED.BYTE_BUDGET // (SEED.BYTES_PER_PIXEL * H * W))
    bits = torch.cat([SEED.near_bits(ES.edt_squared(torch.from_numpy((scan.maps[b:b + per] > 127).astype(np.uint8)), **on), 2, **on)
                      for b in range(0, V, per)])
    dims = SEED.grid_dims(BOUNDS, a.grid)
    n = dims[0] * dims[1] * dims[2]
    trunc, slack = TS.default_trunc(BOUNDS, dims), SEED.default_slack(BOUNDS, dims)
    lib, stream, ptr = L.load(), L.raw_stream(dev), L.ptr
    lo, hi = (np.asarray(x, np.float64) for x in BOUNDS)
    lo_c, step_c = (C.c_double * 3)(*lo), (C.c_double * 3)(*((hi - lo) / np.array(dims, np.float64)))
    grid = (dims[0], dims[1], dims[2], C.cast(lo_c, C.c_void_p), C.cast(step_c, C.c_void_p))
    Kd, Md = torch.from_numpy(intr).to(dev), torch.from_numpy(np.ascontiguousarray(w2c.reshape(V, 12))).to(dev)
    z16 = lambda: torch.zeros(n, dtype=torch.uint16, device=dev)
    seen, hit, hid = z16(), z16(), z16()
    state = {k: (torch.zeros(n, dtype=torch.float64, device=dev), z16()) for k in ("lib", "linear")}
    probe = None
    if a.geometry_lib:
        probe = C.CDLL(os.path.abspath(a.geometry_lib))
        probe.probe_tsdf_integrate_linear.restype = C.c_int
        probe.probe_tsdf_integrate_linear.argtypes = L.SIGNATURES["cgs_tsdf_integrate"][1]

    def integrate(fn, planes, key):
        s, w = state[key]
        return lambda: fn(*grid, V, ptr(Kd), ptr(Md), H, W, ptr(planes), trunc, 0, ptr(s), ptr(w), stream)

    votes = lambda planes: (lambda: lib.cgs_voxel_votes_depth(*grid, V, ptr(Kd), ptr(Md), H, W, ptr(bits), ptr(planes), slack, 0,
                                                              ptr(seen), ptr(hit), ptr(hid), stream))
    result = {"views": V, "width": W, "height": H, "dims": list(dims), "trunc": trunc, "reps": a.reps, "linear_probe": bool(probe),
              "device": torch.cuda.get_device_name(dev)}
    for label, planes in (("dense", dense), ("sparse", sparse)):
        calls = {"voxel_votes_depth": votes(planes), "tsdf_integrate": integrate(lib.cgs_tsdf_integrate, planes, "lib")}
        if probe:
            calls["tsdf_integrate_linear"] = integrate(probe.probe_tsdf_integrate_linear, planes, "linear")
        for name, call in calls.items():   # the warm-up
            assert call() == 0, name
        torch.cuda.synchronize()
        if probe:                          # the states are compared before anything is timed
            assert all(torch.equal(x.view(torch.int16 if x.dtype == torch.uint16 else torch.int64),
                                   y.view(torch.int16 if y.dtype == torch.uint16 else torch.int64))
                       for x, y in zip(state["lib"], state["linear"])), "the geometries disagree"
        w = state["lib"][1].to(torch.int32)
        result[label] = {"pixels_with_depth": float(((planes > 0) & torch.isfinite(planes)).float().mean()),
                         "observed_points": int((w > 0).sum()), "observations": int(w.sum()), "ms": {k: [] for k in calls}}
        for _ in range(3):
            for name, call in calls.items():
                result[label]["ms"][name].append(events_ms(torch, call, a.reps))
        print(label, json.dumps(result[label]), flush=True)

    # extraction on the sphere's analytic field
    ax = [torch.from_numpy((lo[k] + (np.arange(dims[k], dtype=np.float64) + 0.5) * ((hi - lo) / np.array(dims))[k])
                           .astype(np.float32).astype(np.float64)).to(dev) for k in range(3)]
    Z, Y, X = torch.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    field = (torch.sqrt((X - 0.4873) ** 2 + (Y - 0.5219) ** 2 + (Z - 0.5102) ** 2) - 0.3).reshape(-1).contiguous()
    ones = torch.ones(n, dtype=torch.int32, device=dev).to(torch.uint16)
    cells = (dims[0] - 1) * (dims[1] - 1) * (dims[2] - 1)
    counts = torch.zeros(cells, dtype=torch.uint8, device=dev)
    count = lambda: lib.cgs_tsdf_mesh_count(*dims, ptr(field), ptr(ones), 1, ptr(counts), stream)
    assert count() == 0
    ends = torch.cumsum(counts, 0, dtype=torch.int64)
    offsets, T = (ends - counts).contiguous(), int(ends[-1])
    tris = torch.zeros((T, 3, 3), dtype=torch.float32, device=dev)
    emit = lambda: lib.cgs_tsdf_mesh_emit(*grid, ptr(field), ptr(ones), 1, ptr(offsets), T, ptr(tris), stream)
    scan_ = lambda: torch.cumsum(counts, 0, dtype=torch.int64) - counts
    assert emit() == 0
    torch.cuda.synchronize()
    ms = {"count": [], "scan": [], "emit": []}
    for _ in range(3):
        for name, call in (("count", count), ("scan", scan_), ("emit", emit)):
            ms[name].append(events_ms(torch, call, a.reps))
    result["extraction"] = {"triangles": T, "cells": cells, "ms": ms}
    print("extraction", json.dumps(result["extraction"]), flush=True)
    return result


def gate_figures(scan, tris, slack, backend="gpu", **score_kw):
    """The pairs the TSDF mesh's gate hides beside the solid's own gate, and the ground truth scored at 1 px."""
    import test_stereo_depth_cpu as T
    from curve_gaussian_amd.edge_extraction.reprojection import score_edges
    from curve_gaussian_amd.ops import edge_occlusion as EO
    from curve_gaussian_amd.ops.view_chunks import camera_arrays
    intr, w2c = camera_arrays(scan.cameras)
    H, W = scan.depth.shape[1:]
    widen = lambda d: EO.depth_window_max(d, EO.DEPTH_WINDOW, backend=backend).cpu().numpy()
    seen, hid_m = T.gate_pairs(scan, widen(scan.depth), EO.DEPTH_SLACK)
    planes = EO.mesh_depth(tris, intr, w2c, H, W, EO.DEPTH_WINDOW, backend=backend).cpu().numpy()
    _, hid = T.gate_pairs(scan, planes, slack)
    agg = score_edges(scan.edges, scan.cameras, scan.maps, "PidiNet", backend=backend, occluder=tris, depth_slack=slack,
                      **score_kw)["aggregate"]
    return {"pairs_seen": int(seen.sum()), "hidden_by_mesh": int(hid_m.sum()), "hidden_by_both": int((hid & hid_m).sum()),
            "hidden_by_tsdf_only": int((hid & ~hid_m).sum()), "hidden_by_mesh_only": int((hid_m & ~hid).sum()),
            "precision_1px": agg["precision"][0], "recall_1px": agg["recall"][0]}


def box_fixture():
    import tsdf_cases as TC

    import pathlib
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        tris, info, figures, scan = TC.box_end_to_end("gpu", pathlib.Path(tmp))
    out = {"info": info, "depth_error": figures}
    out.update(gate_figures(scan, tris, info["recommended_slack"]))
    print("box fixture", json.dumps(out), flush=True)
    return out


def stereo_chain(shape):
    import test_stereo_depth_cpu as T
    from curve_gaussian_amd.edge_extraction.reprojection import score_edges
    from curve_gaussian_amd.ops import edge_occlusion as EO
    from curve_gaussian_amd.ops import mesh_contours as MC
    from curve_gaussian_amd.ops import stereo_depth as SD
    from curve_gaussian_amd.ops import tsdf as TS
    from curve_gaussian_amd.scene import solid_scan as SS
    H, W, views = 240, 320, 24
    contours = shape == "cylinder"
    scan = SS.solid_scan(shape, views, H, W, synth_cameras=SS.arc_cameras(views, H, W), contours=contours)
    fused, sinfo = SD.stereo_depth(list(SS.photographs(scan)), scan.cameras, backend="gpu", return_info=True, fuse=True)
    widen = lambda d: EO.depth_window_max(d, EO.DEPTH_WINDOW, backend="gpu").cpu().numpy()
    seen, hid_m = T.gate_pairs(scan, widen(scan.depth), EO.DEPTH_SLACK)
    _, hid_f = T.gate_pairs(scan, widen(np.stack(EO.check_depth_maps(scan.cameras, fused))), sinfo["recommended_slack"])
    agg = score_edges(scan.edges, scan.cameras, scan.maps, "PidiNet", depth_maps=fused,
                      depth_slack=sinfo["recommended_slack"])["aggregate"]
    out = {"shape": shape, "views": views, "height": H, "width": W, "pairs_seen": int(seen.sum()), "hidden_by_mesh": int(hid_m.sum()),
           "fused_maps": {"recommended_slack": sinfo["recommended_slack"], "hidden_by_both": int((hid_f & hid_m).sum()),
                          "hidden_by_maps_only": int((hid_f & ~hid_m).sum()), "precision_1px": agg["precision"][0],
                          "recall_1px": agg["recall"][0]}}
    tris, info = TS.tsdf_mesh(fused, scan.cameras, backend="gpu")
    out["tsdf_mesh"] = dict(gate_figures(scan, tris, info["recommended_slack"]), info=info)
    out["tsdf_mesh_half_slack"] = gate_figures(scan, tris, 0.5 * info["recommended_slack"])
    if contours:
        out["tsdf_mesh_ignore_contours"] = gate_figures(scan, tris, info["recommended_slack"], ignore_contours=True)
        edges = MC.mesh_edges(tris)
        out["contour_edges"] = {"edges": int(len(edges.cos)), "smooth_at_30_deg": int(MC.smooth(edges.cos, 30.0).sum())}
        solid = MC.mesh_edges(scan.tris)
        out["contour_edges_of_the_solid"] = {"edges": int(len(solid.cos)), "smooth_at_30_deg": int(MC.smooth(solid.cos, 30.0).sum())}
    print("stereo chain", json.dumps(out), flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--timing", action="store_true")
    ap.add_argument("--views", type=int, default=100)
    ap.add_argument("--width", type=int, default=1600)
    ap.add_argument("--height", type=int, default=1200)
    ap.add_argument("--grid", type=int, default=256)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--geometry_lib", default=None)
    ap.add_argument("--box", action="store_true")
    ap.add_argument("--stereo", nargs="*", default=[])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    result = {}
    if a.timing:
        result["timing"] = timing(a)
    if a.box:
        result["box"] = box_fixture()
    if a.stereo:
        result["stereo"] = [stereo_chain(s) for s in a.stereo]
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
