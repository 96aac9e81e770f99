"""python profiles/probes/mesh_contours.py [--views 100] [--width 1600] [--height 1200] [--grid 224] [--reps 20] [--out FILE]

Times cgs_mesh_contours (profiles/mesh_contours.md) beside cgs_mesh_depth on the same mesh in the same run, everything
resident, raw calls between device events after a warm-up, three rounds, the variants alternating within a round:

  the FINE mesh of profiles/probes/edge_occlusion.py (a sphere of 2 x grid x grid small triangles) and its COARSE one (the
  12 triangles of a box that fills every image); for each the rows of ``kind="smooth"`` and of ``kind="all"``, without a
  plane and with the mesh's own planes (window 1, the default slack).

Before anything is timed the masks of the first two views are compared with the host back end bit for bit, for every
variant.  Then, as plain numbers, what the existing chain does on the cylinder scan of scene/solid_scan.py with and without
contours in its maps: the seeds of ``seed_points`` with and without ``exclusive`` and how many lie away from every
ground-truth edge, and the support check of the ground truth plus one bogus line laid along a side of the cylinder."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from edge_occlusion import box_mesh, sphere_mesh  # noqa: E402  (the sibling probes: the same inputs)
from edge_orient import sphere_cameras  # noqa: E402
from edge_support import events_ms  # noqa: E402

MIN_RATIOS = (0.8, 0.5)  # seed_points' default, and one at which a hidden-line-removed scan keeps voxels at all
GHOST_DISTANCE = 0.02   # a seed farther than this from every ground-truth sample explains no 3D edge (2.5 voxels of 1/128)


def chain_on_the_cylinder(torch, views, height, width, backend="gpu"):
    from curve_gaussian_amd.edge_extraction.abc import pred_points_and_directions
    from curve_gaussian_amd.ops import edge_seed as SD
    from curve_gaussian_amd.ops import edge_support as SP
    from curve_gaussian_amd.scene import solid_scan as SS
    out = {}
    for contours in (False, True):
        scan = SS.solid_scan("cylinder", views, height, width, backend=backend, contours=contours)
        gt = np.asarray(pred_points_and_directions(scan.edges, 0.002).points, np.float64).reshape(-1, 3)
        row = {"detected_pixels": int((scan.maps != 0).sum()),
               "contour_pixels": int(scan.contours.sum()) if contours else 0}
        for min_ratio in MIN_RATIOS:
            for exclusive in (False, True):
                seeds, info = SD.seed_points(scan.cameras, scan.maps, "PidiNet", ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0)),
                                             min_ratio=min_ratio, exclusive=exclusive, backend=backend)
                far = 0
                if len(seeds):
                    d = torch.cdist(torch.from_numpy(np.asarray(seeds, np.float64)), torch.from_numpy(gt)).min(1).values
                    far = int((d > GHOST_DISTANCE).sum())
                row[f"seeds_ratio{min_ratio:g}" + ("_exclusive" if exclusive else "")] = {
                    "seeds": int(len(seeds)), "ghosts": far, "kept_voxels": int(info["kept_voxels"])}
        bogus = [0.8, 0.5, 0.25, 0.8, 0.5, 0.75]   # a generator of the cylinder's side: on the surface, no edge
        edges = {"curves_ctl_pts": scan.edges["curves_ctl_pts"], "lines_end_pts": scan.edges["lines_end_pts"] + [bogus]}
        res = SP.edge_support(edges, scan.cameras, scan.maps, "PidiNet", occluder=scan.tris, backend=backend)
        pick = lambda k, e: np.asarray(res[k])[e].tolist()
        row["support_ground_truth"] = {k: pick(k, slice(0, -1)) for k in ("seeing_views", "supporting_views", "kept")}
        row["support_bogus_line"] = {k: pick(k, -1) for k in ("seeing_views", "supporting_views", "share", "kept")}
        out["with_contours" if contours else "without_contours"] = row
        print(("with" if contours else "without") + " contours: " + json.dumps(row), flush=True)
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--views", type=int, default=100)
    p.add_argument("--width", type=int, default=1600)
    p.add_argument("--height", type=int, default=1200)
    p.add_argument("--grid", type=int, default=224)
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--chain_views", type=int, default=24)
    p.add_argument("--chain_backend", default=None, choices=("gpu", "host"),
                   help="run the cylinder chain alone, on this back end (both give the same numbers), and stop")
    p.add_argument("--out", default=None)
    a = p.parse_args()
    import torch
    if a.chain_backend:
        print(json.dumps(chain_on_the_cylinder(torch, a.chain_views, 240, 320, a.chain_backend)))
        return
    from curve_gaussian_amd import _lib as L
    from curve_gaussian_amd.ops import edge_occlusion as EO
    from curve_gaussian_amd.ops import edge_score as ES
    from curve_gaussian_amd.ops import mesh_contours as MC
    if not torch.cuda.is_available():
        raise SystemExit("mesh_contours: needs a GPU; nothing is measured without one")
    dev = torch.device("cuda", 0)
    H, W, V = a.height, a.width, a.views
    lib, stream = L.load(), L.raw_stream(dev)
    K, M = sphere_cameras(V, H, W)
    Kd, Md = ES.cameras_on(dev, K, np.ascontiguousarray(M.reshape(V, 12)))
    result = {"views": V, "width": W, "height": H, "rounds": 3, "reps": a.reps, "device": torch.cuda.get_device_name(dev),
              "ms": {}, "meshes": {}}
    depth = torch.empty((V, H, W), dtype=torch.float32, device=dev)
    mask = torch.empty((V, H, W), dtype=torch.uint8, device=dev)
    for name, tris in (("fine", sphere_mesh(a.grid)), ("coarse", box_mesh())):
        table = MC.mesh_edges(tris)
        rows = {"smooth": np.ascontiguousarray(table.rows[MC.smooth(table.cos)]), "all": table.rows}
        flags = MC.contour_flags(rows["all"], K[:2], M[:2])
        info = {"triangles": len(tris), "rows_all": len(rows["all"]), "rows_smooth": len(rows["smooth"]),
                "boundary": table.boundary, "non_manifold": table.non_manifold,
                "contours_all_first_two_views": flags.sum(1).tolist()}
        planes = EO.mesh_depth(tris, K, M, H, W, window=EO.DEPTH_WINDOW)
        for kind, r in rows.items():   # equality first
            for d in (None, planes[:2]):
                want = MC.row_masks(r, K[:2], M[:2], H, W, depth=None if d is None else d.cpu(), backend="host")
                got = MC.row_masks(r, K[:2], M[:2], H, W, depth=d)
                assert torch.equal(got.cpu(), want), f"{name} {kind}: cgs_mesh_contours disagrees with the host"
        t_d = torch.from_numpy(tris).to(dev)
        calls = {f"mesh_depth_{name}": lambda: L.check(lib.cgs_mesh_depth(
            len(tris), L.ptr(t_d), V, L.ptr(Kd), L.ptr(Md), H, W, L.ptr(depth), stream), "cgs_mesh_depth")}
        keep = []
        for kind, r in rows.items():
            r_d = torch.from_numpy(r).to(dev)
            keep.append(r_d)
            for gated in (False, True):
                calls[f"mesh_contours_{name}_{kind}" + ("_plane" if gated else "")] = (
                    lambda r_d=r_d, gated=gated: L.check(lib.cgs_mesh_contours(
                        int(r_d.shape[0]), L.ptr(r_d), V, L.ptr(Kd), L.ptr(Md), H, W, L.ptr(planes) if gated else None,
                        EO.DEPTH_SLACK, L.ptr(mask), stream), "cgs_mesh_contours"))
        print(f"{name}: {json.dumps(info)}; equal to the host back end in 2 views for both kinds, with and without the plane",
              flush=True)
        for call in calls.values():   # the warm-up
            call()
        torch.cuda.synchronize()
        ms = {k: [] for k in calls}
        for _ in range(3):
            for k, call in calls.items():
                ms[k].append(events_ms(torch, call, a.reps))
        for k, call in calls.items():
            if k.startswith("mesh_contours"):
                call()
                info["pixels_" + k[len("mesh_contours_") + len(name) + 1:]] = int(mask.sum(dtype=torch.int64))
        for k, t in ms.items():
            print(f"  {k}: {[round(x, 4) for x in t]} ms per call", flush=True)
        result["ms"].update(ms)
        result["meshes"][name] = info
        del planes, keep
    print("a clear of the masks alone (torch's fill kernel):", flush=True)
    mask.zero_()
    torch.cuda.synchronize()
    result["ms"]["clear"] = [events_ms(torch, lambda: mask.zero_(), a.reps) for _ in range(3)]
    print(f"  clear: {[round(x, 4) for x in result['ms']['clear']]} ms per call", flush=True)
    del depth, mask
    result["cylinder_chain"] = chain_on_the_cylinder(torch, a.chain_views, 240, 320)
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
