"""python profiles/probes/stereo_depth.py [--shape box] [--views 8] [--width 1600] [--height 1200] [--hypotheses 64]
                                          [--patch_radius 2] [--sources 3] [--reps 3] [--geometry_lib FILE]
                                          [--quality VIEWS ...] [--out FILE]

The measurements of profiles/stereo_depth.md, on one GPU.

TIMING.  ``--views`` reference views of the drawn ``--shape`` on an arc 8 degrees apart, photographed with the value-noise
texture of scene/solid_scan.py, planned by ``ops.stereo_depth.plan_views``; everything resident, raw calls of
cgs_stereo_sweep between device events after a warm-up, three rounds of ``--reps`` calls.  With ``--geometry_lib`` (built from
profiles/probes/stereo_depth_geometries.hip) the plain geometry runs beside the library's kernel, alternating within a
round, after its maps are compared with the library's bit for bit.  cgs_stereo_consistency is timed the same way.  The
share of pixels that reach the sweep (a patch inside the image with enough variance: the background has none) is reported,
because the time is theirs.

QUALITY (``--quality 24 48``).  The figures tests/test_stereo_depth_cpu.py prints, at that many views of 320 x 240 with the
defaults of ``stereo_depth`` on the GPU back end (the host back end is too slow there): coverage and depth error against
``mesh_depth`` of the same solid, the pairs each gate hides, the ground truth scored without a gate and with the stereo
maps at the recommended slack."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timing(a):
    import torch
    from curve_gaussian_amd import _lib as L
    from curve_gaussian_amd.ops import stereo_depth as SD
    from curve_gaussian_amd.scene import solid_scan as SS
    dev = torch.device("cuda:0")
    scan = SS.solid_scan(a.shape, a.views, a.height, a.width, synth_cameras=SS.arc_cameras(a.views, a.height, a.width))
    photos = SS.photographs(scan)
    plan = SD.plan_views(scan.cameras, hypotheses=a.hypotheses, sources=a.sources)
    V, H, W, D, S, R = a.views, a.height, a.width, a.hypotheses, a.sources, a.patch_radius
    t = {k: torch.from_numpy(np.ascontiguousarray(x)).to(dev) for k, x in
         (("gray", photos), ("K", plan.K), ("inv", plan.inv), ("src", plan.src), ("rel", plan.rel), ("tol", plan.tol))}
    lib, p, s = L.load(), L.ptr, L.raw_stream(dev)
    out = {name: torch.zeros((V, H, W), dtype=torch.float32, device=dev) for name in ("library", "plain", "filtered")}
    args = lambda o: [V, H, W, p(t["gray"]), p(t["K"]), D, p(t["inv"]), S, p(t["src"]), p(t["rel"]), R, SD.MIN_VAR, SD.MAX_COST,
                      SD.MIN_SOURCES, p(o), s]
    calls = {"library": lambda: L.check(lib.cgs_stereo_sweep(*args(out["library"])), "cgs_stereo_sweep")}
    if a.geometry_lib:
        probe = ctypes.CDLL(os.path.abspath(a.geometry_lib))
        probe.probe_stereo_sweep_plain.restype = ctypes.c_int
        probe.probe_stereo_sweep_plain.argtypes = L.SIGNATURES["cgs_stereo_sweep"][1]
        calls["plain"] = lambda: L.check(probe.probe_stereo_sweep_plain(*args(out["plain"])), "probe_stereo_sweep_plain")
    calls["consistency"] = lambda: L.check(lib.cgs_stereo_consistency(
        V, H, W, p(out["library"]), p(t["K"]), S, p(t["src"]), p(t["rel"]), p(t["tol"]), SD.MIN_CONSISTENT, p(out["filtered"]), s),
        "cgs_stereo_consistency")
    for f in calls.values():   # warm-up; the maps are compared before anything is timed
        f()
    torch.cuda.synchronize()
    if a.geometry_lib:
        assert torch.equal(out["library"].view(torch.int32), out["plain"].view(torch.int32)), "the geometries disagree"
    g = photos.astype(np.float64)
    result = {"shape": a.shape, "views": V, "height": H, "width": W, "hypotheses": D, "patch_radius": R, "sources": S,
              "reps": a.reps, "swept_coverage": float((out["library"] > 0).float().mean()),
              "filtered_coverage": float((out["filtered"] > 0).float().mean()),
              "textured_share": float((np.abs(g[:, 1:-1, 1:-1] - g[:, :-2, 1:-1]) > 0).mean()), "rounds": []}
    for _ in range(3):
        row = {}
        for name, f in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.reps):
                f()
            e1.record()
            torch.cuda.synchronize()
            row[name] = e0.elapsed_time(e1) / a.reps / V
        result["rounds"].append(row)
        print("ms per view:", row, flush=True)
    for name in calls:
        vals = [r[name] for r in result["rounds"]]
        result[name + "_ms_per_view"] = {"median": float(np.median(vals)), "spread": float(max(vals) - min(vals))}
    return result


def quality(a, views):
    import test_stereo_depth_cpu as T
    from curve_gaussian_amd.edge_extraction.reprojection import score_edges
    from curve_gaussian_amd.ops import edge_occlusion as EO
    from curve_gaussian_amd.ops import stereo_depth as SD
    from curve_gaussian_amd.scene import solid_scan as SS
    H, W = 240, 320
    scan = SS.solid_scan(a.shape, views, H, W, synth_cameras=SS.arc_cameras(views, H, W))
    maps, info = SD.stereo_depth(list(SS.photographs(scan)), scan.cameras, backend="gpu", return_info=True)
    slack = info["recommended_slack"]
    row = {"shape": a.shape, "views": views, "height": H, "width": W, "recommended_slack": slack}
    row.update(T.stereo_quality(scan, maps, SD.HYPOTHESES, SD.SOURCES))
    widen = lambda d: EO.depth_window_max(d, EO.DEPTH_WINDOW, backend="gpu").cpu().numpy()
    seen, hid_s = T.gate_pairs(scan, widen(np.stack(EO.check_depth_maps(scan.cameras, maps))), slack)
    _, hid_m = T.gate_pairs(scan, widen(scan.depth), EO.DEPTH_SLACK)
    row.update({"pairs_seen": int(seen.sum()), "hidden_by_both": int((hid_s & hid_m).sum()),
                "hidden_by_stereo_only": int((hid_s & ~hid_m).sum()), "hidden_by_mesh_only": int((hid_m & ~hid_s).sum())})
    plain = score_edges(scan.edges, scan.cameras, scan.maps, "PidiNet")["aggregate"]
    gated = score_edges(scan.edges, scan.cameras, scan.maps, "PidiNet", depth_maps=maps, depth_slack=slack)["aggregate"]
    row.update({"precision_1px": [plain["precision"][0], gated["precision"][0]],
                "recall_1px": [plain["recall"][0], gated["recall"][0]]})
    print(row, flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="box")
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--width", type=int, default=1600)
    ap.add_argument("--height", type=int, default=1200)
    ap.add_argument("--hypotheses", type=int, default=64)
    ap.add_argument("--patch_radius", type=int, default=2)
    ap.add_argument("--sources", type=int, default=3)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--geometry_lib", default=None)
    ap.add_argument("--quality", type=int, nargs="*", default=[])
    ap.add_argument("--no_timing", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    result = {}
    if not a.no_timing:
        result["timing"] = timing(a)
    if a.quality:
        result["quality"] = [quality(a, v) for v in a.quality]
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
