"""python profiles/probes/stereo_fuse.py [--shape box] [--views 8] [--width 1600] [--height 1200] [--hypotheses 64]
                                         [--patch_radius 2] [--sources 3] [--fuse_sources 7] [--reps 3] [--fuse_reps 500]
                                         [--geometry_lib FILE] [--quality VIEWS ...] [--out FILE]

The measurements of profiles/stereo_fuse.md, on one GPU.

TIMING.  ``--views`` views of the drawn ``--shape`` on an arc 8 degrees apart, photographed, planned, swept and filtered as
profiles/probes/stereo_depth.py does; the filtered maps are what the fusion gets.  Everything resident, raw calls of
cgs_stereo_sweep, cgs_stereo_warp and cgs_stereo_fuse between device events after a warm-up, three rounds of ``--reps``
calls of the sweep and ``--fuse_reps`` calls of the others (they are a hundred times shorter, and a window of a millisecond
measures the clock), all targets in one call.  With ``--geometry_lib`` (built from
profiles/probes/stereo_fuse_geometries.hip) the other warp geometry runs beside the library's kernel within a round, after
its planes are compared with the library's bit for bit.  Then warp and fuse again on maps that hold a depth at EVERY pixel (a fronto-parallel plane through the middle
of the bounds per view), because the drawn shape fills a sixth of the image and the warp's time is its depths'.

QUALITY (``--quality 24``).  At that many views of 320 x 240 with the defaults on the GPU back end, unfused beside fused:
the figures of tests/test_stereo_depth_cpu.py's ``stereo_quality``, the pairs each gate hides at the recommended slack and
at half of it, and the ground truth scored at 1 px."""
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
    K, fsrc, into, tol = SD.plan_fusion(scan.cameras, hypotheses=a.hypotheses, fuse_sources=a.fuse_sources)
    V, H, W, D, S, R, F = a.views, a.height, a.width, a.hypotheses, a.sources, a.patch_radius, a.fuse_sources
    t = {k: torch.from_numpy(np.ascontiguousarray(x)).to(dev) for k, x in
         (("gray", photos), ("K", plan.K), ("inv", plan.inv), ("src", plan.src), ("rel", plan.rel), ("tol", plan.tol),
          ("fsrc", fsrc), ("into", into))}
    lib, p, s = L.load(), L.ptr, L.raw_stream(dev)
    swept, filtered, fused = (torch.zeros((V, H, W), dtype=torch.float32, device=dev) for _ in range(3))
    support = torch.zeros((V, H, W), dtype=torch.uint8, device=dev)
    warped, other = (torch.zeros((V, F, H, W), dtype=torch.float32, device=dev) for _ in range(2))
    centre = np.array([0.5, 0.5, 0.5])
    full = torch.from_numpy(np.stack([np.full((H, W), float(np.asarray(c.R)[2] @ centre + np.asarray(c.T)[2]), np.float32)
                                      for c in scan.cameras])).to(dev)
    sweep = lambda: L.check(lib.cgs_stereo_sweep(V, H, W, p(t["gray"]), p(t["K"]), D, p(t["inv"]), S, p(t["src"]), p(t["rel"]), R,
                                                 SD.MIN_VAR, SD.MAX_COST, SD.MIN_SOURCES, p(swept), s), "cgs_stereo_sweep")
    warp_args = lambda d, o: [V, H, W, p(d), p(t["K"]), F, p(t["fsrc"]), p(t["into"]), 0, V, p(o), s]
    warp = lambda d: (lambda: L.check(lib.cgs_stereo_warp(*warp_args(d, warped)), "cgs_stereo_warp"))
    fuse = lambda d: (lambda: L.check(lib.cgs_stereo_fuse(V, H, W, p(d), F, p(warped), p(t["tol"]), SD.FUSE_SUPPORT, 0, V, p(fused),
                                                          p(support), s), "cgs_stereo_fuse"))
    sweep()
    L.check(lib.cgs_stereo_consistency(V, H, W, p(swept), p(t["K"]), S, p(t["src"]), p(t["rel"]), p(t["tol"]), SD.MIN_CONSISTENT,
                                       p(filtered), s), "cgs_stereo_consistency")
    calls = {"sweep": sweep, "warp": warp(filtered), "fuse": fuse(filtered), "warp_full": warp(full), "fuse_full": fuse(full)}
    if a.geometry_lib:
        probe = ctypes.CDLL(os.path.abspath(a.geometry_lib))
        probe.probe_stereo_warp_rows.restype = ctypes.c_int
        probe.probe_stereo_warp_rows.argtypes = L.SIGNATURES["cgs_stereo_warp"][1]
        rows = lambda d: (lambda: L.check(probe.probe_stereo_warp_rows(*warp_args(d, other)), "probe_stereo_warp_rows"))
        for d in (filtered, full):   # the planes are compared before anything is timed
            warp(d)()
            rows(d)()
            torch.cuda.synchronize()
            assert torch.equal(warped.view(torch.int32), other.view(torch.int32)), "the geometries disagree"
        calls = {"sweep": sweep, "warp": warp(filtered), "warp_rows": rows(filtered), "fuse": fuse(filtered),
                 "warp_full": warp(full), "warp_rows_full": rows(full), "fuse_full": fuse(full)}
    result = {"shape": a.shape, "views": V, "height": H, "width": W, "hypotheses": D, "patch_radius": R, "sources": S,
              "fuse_sources": F, "min_support": SD.FUSE_SUPPORT, "reps": a.reps, "fuse_reps": a.fuse_reps, "rounds": []}
    for name, f in calls.items():   # warm-up, and what the drawn shape's calls see and give
        f()
        torch.cuda.synchronize()
        if name == "fuse":
            result.update({"filtered_coverage": float((filtered > 0).float().mean()),
                           "fused_coverage": float((fused > 0).float().mean()),
                           "warped_share": float(torch.isfinite(warped).float().mean())})
        if name == "fuse_full":
            result.update({"full_fused_coverage": float((fused > 0).float().mean()),
                           "full_warped_share": float(torch.isfinite(warped).float().mean())})
    for _ in range(3):
        row = {}
        for name, f in calls.items():
            if name.startswith("fuse"):   # (the planes the fusion reads: its own maps')
                (warp(full) if name == "fuse_full" else warp(filtered))()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            reps = a.reps if name == "sweep" else a.fuse_reps
            e0.record()
            for _ in range(reps):
                f()
            e1.record()
            torch.cuda.synchronize()
            row[name] = e0.elapsed_time(e1) / reps / V
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
    photos = list(SS.photographs(scan))
    unfused, info = SD.stereo_depth(photos, scan.cameras, backend="gpu", return_info=True)
    fused, finfo = SD.fuse_depth(unfused, scan.cameras, backend="gpu", return_info=True)
    slack = info["recommended_slack"]
    widen = lambda d: EO.depth_window_max(d, EO.DEPTH_WINDOW, backend="gpu").cpu().numpy()
    seen, hid_m = T.gate_pairs(scan, widen(scan.depth), EO.DEPTH_SLACK)
    plain = score_edges(scan.edges, scan.cameras, scan.maps, "PidiNet")["aggregate"]
    out = {"shape": a.shape, "views": views, "height": H, "width": W, "recommended_slack": slack, "fuse_sources": SD.FUSE_SOURCES,
           "min_support": SD.FUSE_SUPPORT, "pairs_seen": int(seen.sum()), "hidden_by_mesh": int(hid_m.sum()),
           "precision_1px_ungated": plain["precision"][0], "recall_1px_ungated": plain["recall"][0],
           "fusion": {k: finfo[k] for k in ("support_histogram", "filled", "dropped")}}
    for name, maps in (("unfused", unfused), ("fused", fused)):
        row = T.stereo_quality(scan, maps, SD.HYPOTHESES, SD.SOURCES)
        planes = widen(np.stack(EO.check_depth_maps(scan.cameras, maps)))
        for label, sl in (("", slack), ("_half_slack", 0.5 * slack)):
            _, hid = T.gate_pairs(scan, planes, sl)
            row.update({"hidden_by_both" + label: int((hid & hid_m).sum()), "hidden_by_stereo_only" + label: int((hid & ~hid_m).sum()),
                        "hidden_by_mesh_only" + label: int((hid_m & ~hid).sum())})
        gated = score_edges(scan.edges, scan.cameras, scan.maps, "PidiNet", depth_maps=maps, depth_slack=slack)["aggregate"]
        row.update({"precision_1px": gated["precision"][0], "recall_1px": gated["recall"][0]})
        out[name] = row
        print(name, row, flush=True)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="box")
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--width", type=int, default=1600)
    ap.add_argument("--height", type=int, default=1200)
    ap.add_argument("--hypotheses", type=int, default=64)
    ap.add_argument("--patch_radius", type=int, default=2)
    ap.add_argument("--sources", type=int, default=3)
    ap.add_argument("--fuse_sources", type=int, default=7)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--fuse_reps", type=int, default=500)
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
