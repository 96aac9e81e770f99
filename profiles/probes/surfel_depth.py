"""python profiles/probes/surfel_depth.py [--views 100] [--width 1600] [--height 1200] [--points 2000000] [--big 1000]
                                           [--reps 20] [--heavy_reps 2] [--thresholds 16 64 256] [--geometry_lib FILE]
                                           [--gate] [--out FILE]

The measurements of profiles/surfel_depth.md.

``--gate`` (host back end, no GPU): the surfel gate against the mesh gate on the drawn solids -- 6 views of 60 x 80,
``surfel_cloud`` at spacing 0.01, radii from ``surfel_radii`` at every factor of (0.6, 0.8, 1.0, 1.2) -- holes, seen pairs,
pairs each gate hides, mesh-only and surplus; then the ground truth of the box scored from a written scan with ``mesh.ply``
and with ``cloud.ply`` as the occluder.

Otherwise (one GPU): cgs_surfel_depth, everything resident, raw calls between device events after a warm-up, three rounds,
the variants alternating within a round, on three clouds seen by ``--views`` cameras around the unit cube:

  A  ``--points`` surfels on the sphere of profiles/probes/edge_occlusion.py (radius 0.45: a Fibonacci lattice on it, the
     normals radial), radii from ``surfel_radii`` on the GPU: disks of a few pixels
  B  ``--big`` surfels within 0.1 of the cube's centre with radius 0.5 and random normals: each fills a large part of every image
  C  A with the first 100 of B mixed in at random positions

With ``--geometry_lib`` (built from profiles/probes/surfel_depth_geometries.hip) the pure geometries -- one thread, one wave
per (surfel, view) -- and the hybrid at every threshold of ``--thresholds`` run beside the library's kernel, after their
planes are compared with the library's bit for bit.  Those calls do not fill the planes, so a fill of the same planes goes in
front of each, as inside the library's call; the fill alone is timed too.  Variants that take a second or more a call (the
wave geometry on A and C, everything on B, the thread geometry on C) run ``--heavy_reps`` calls a round.  cgs_mesh_depth on
the 100 352-triangle mesh of the same sphere is timed beside A.  Before anything is timed the library's planes of the first
4000 surfels of A and the first 2 of B in the first view are compared with the host back end bit for bit."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

FACTORS = (0.6, 0.8, 1.0, 1.2)


def gate_counts(shape, factor, views=6, H=60, W=80, spacing=0.01):
    from curve_gaussian_amd import synthetic
    from curve_gaussian_amd.edge_extraction.abc import pred_points_and_directions
    from curve_gaussian_amd.ops import edge_occlusion as EO
    from curve_gaussian_amd.ops.view_chunks import camera_arrays
    from curve_gaussian_amd.scene import solid_scan as SS
    tris, edges = SS.solid_geometry(shape)
    K, M = camera_arrays(SS.emap_cameras_of(synthetic.fibonacci_cameras(views, H, W)))
    pts, nrm = SS.surfel_cloud(tris, spacing)
    rad = EO.surfel_radii(pts, factor, backend="host")
    samples = np.ascontiguousarray(pred_points_and_directions(edges, SS.SAMPLE_RESOLUTION).points, np.float32).reshape(-1, 3)
    raw = {"mesh": EO.mesh_depth(tris, K, M, H, W, window=0, backend="host").numpy(),
           "cloud": EO.surfel_depth(EO.Surfels(pts, nrm, rad), K, M, H, W, window=0, backend="host").numpy()}
    Md = np.asarray(M, np.float64).reshape(len(K), 12)
    hid, seen = {}, None
    for name, planes in raw.items():
        planes = EO.depth_window_max(planes, EO.DEPTH_WINDOW, backend="host").numpy()
        rows = [EO.gate_view_host(samples, K[v], Md[v], planes[v], EO.DEPTH_SLACK) for v in range(len(K))]
        seen = np.stack([r[2] | r[3] for r in rows])
        hid[name] = np.stack([r[3] for r in rows])
    return {"shape": shape, "factor": factor, "surfels": len(pts), "median_radius": float(np.median(rad)),
            "holes": int((np.isfinite(raw["mesh"]) & ~np.isfinite(raw["cloud"])).sum()), "seen": int(seen.sum()),
            "mesh_hides": int(hid["mesh"].sum()), "surfels_hide": int(hid["cloud"].sum()),
            "mesh_only": int((hid["mesh"] & ~hid["cloud"]).sum()), "surplus": int((hid["cloud"] & ~hid["mesh"]).sum())}


def gate(out):
    import tempfile
    from curve_gaussian_amd.edge_extraction import reprojection as R
    from curve_gaussian_amd.scene import solid_scan as SS
    result = {"gate": [], "score": {}}
    for shape in ("box", "cylinder", "l_bracket"):
        for factor in FACTORS:
            row = gate_counts(shape, factor)
            result["gate"].append(row)
            print(row, flush=True)
    with tempfile.TemporaryDirectory() as tmp:
        scan = SS.solid_scan("box", 6, 60, 80, backend="host")
        SS.write_solid_scan(os.path.join(tmp, "data", "box"), scan, cloud=0.01)
        os.makedirs(os.path.join(tmp, "out", "box"))
        with open(os.path.join(tmp, "out", "box", "parametric_edges.json"), "w") as f:
            json.dump(scan.edges, f)
        for occluder in ("mesh.ply", "cloud.ply"):
            res = R.score_scan(os.path.join(tmp, "out"), os.path.join(tmp, "data"), "box", detector="PidiNet", backend="host",
                               occluder=occluder)
            a = res["aggregate"]
            result["score"][occluder] = {"precision": a["precision"], "recall": a["recall"],
                                         "hidden_points": sum(r["hidden_points"] for r in res["views"])}
            print(occluder, result["score"][occluder], flush=True)
    finish(result, out)


def finish(result, out):
    line = json.dumps(result)
    print(line)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(line + "\n")


def fibonacci_sphere(n, radius=0.45, centre=0.5):
    k = np.arange(n, dtype=np.float64)
    z = 1.0 - 2.0 * (k + 0.5) / n
    r = np.sqrt(np.maximum(0.0, 1.0 - z * z))
    th = np.pi * (3.0 - np.sqrt(5.0)) * k
    nrm = np.stack([r * np.cos(th), r * np.sin(th), z], 1)
    return (centre + radius * nrm).astype(np.float32), nrm.astype(np.float32)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--views", type=int, default=100)
    p.add_argument("--width", type=int, default=1600)
    p.add_argument("--height", type=int, default=1200)
    p.add_argument("--points", type=int, default=2000000)
    p.add_argument("--big", type=int, default=1000)
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--heavy_reps", type=int, default=2)
    p.add_argument("--thresholds", type=int, nargs="+", default=[16, 64, 256])
    p.add_argument("--geometry_lib", default=None)
    p.add_argument("--gate", action="store_true")
    p.add_argument("--out", default=None)
    a = p.parse_args()
    if a.gate:
        return gate(a.out)
    import torch
    from curve_gaussian_amd import _lib as L
    from curve_gaussian_amd.ops import edge_occlusion as EO
    from curve_gaussian_amd.ops import edge_score as ES
    from edge_occlusion import sphere_mesh
    from edge_orient import sphere_cameras
    from edge_support import events_ms
    if not torch.cuda.is_available():
        raise SystemExit("surfel_depth: needs a GPU; nothing is measured without one")
    dev = torch.device("cuda", 0)
    H, W, V = a.height, a.width, a.views
    lib, stream = L.load(), L.raw_stream(dev)
    K, M = sphere_cameras(V, H, W)
    Kd, Md = ES.cameras_on(dev, K, np.ascontiguousarray(M.reshape(V, 12)))
    same = lambda x, y: bool(torch.equal(x.cpu().view(torch.int32), y.cpu().view(torch.int32)))

    rng = np.random.default_rng(7)
    pa, na = fibonacci_sphere(a.points)
    ra = EO.surfel_radii(pa, device=dev)
    pb = (0.5 + rng.uniform(-0.1, 0.1, (a.big, 3))).astype(np.float32)
    nb = rng.normal(0, 1, (a.big, 3)).astype(np.float32)
    rb = np.full((a.big,), 0.5, np.float32)
    where = np.sort(rng.choice(a.points, 100, replace=False))
    pc, nc, rc = (np.insert(x, where, y[:100], axis=0) for x, y in ((pa, pb), (na, nb), (ra, rb)))
    clouds = {"A": (pa, na, ra), "B": (pb, nb, rb), "C": (pc, nc, rc)}
    pixel = 1.8 / K[0, 0]   # world units a pixel spans at the cameras' distance from the cube's centre
    print(f"{V} views {W}x{H}; A: {len(pa)} surfels, median radius {float(np.median(ra)):.6f} = {float(np.median(ra)) / pixel:.2f} "
          f"pixels at the centre's distance; B: {len(pb)} of radius 0.5 = {0.5 / pixel:.0f} pixels; C: {len(pc)}", flush=True)

    # equality with the host first
    for name, n in (("A", 4000), ("B", 2)):
        part = EO.Surfels(*(x[:n] for x in clouds[name]))
        want = EO.surfel_depth(part, K[:1], M[:1], H, W, window=0, backend="host")
        assert same(EO.surfel_depth(part, K[:1], M[:1], H, W, window=0, device=dev), want), f"{name}: disagrees with the host"
    print("equal to the host back end on 4000 surfels of A and 2 of B x 1 view", flush=True)

    alt = None
    if a.geometry_lib:
        alt = ctypes.CDLL(os.path.abspath(a.geometry_lib)).surfel_depth_geometry
        alt.restype = ctypes.c_int
        alt.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p,
                        ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_uint, ctypes.c_void_p, ctypes.c_void_p]
    depth = torch.empty((V, H, W), dtype=torch.float32, device=dev)
    other = torch.empty_like(depth)
    result = {"views": V, "width": W, "height": H, "rounds": 3, "device": torch.cuda.get_device_name(dev), "ms": {},
              "surfels": {k: len(v[0]) for k, v in clouds.items()}, "median_radius_A": float(np.median(ra)), "reps": a.reps,
              "heavy_reps": a.heavy_reps, "covered_pixels": {}}

    def rounds(calls, reps):
        for call in calls.values():   # the warm-up
            call()
        torch.cuda.synchronize()
        ms = {name: [] for name in calls}
        for _ in range(3):
            for name, call in calls.items():
                ms[name].append(events_ms(torch, call, reps[name]))
        for name, t in ms.items():
            print(f"  {name}: {[round(x, 3) for x in t]} ms per call ({reps[name]} calls a round)", flush=True)
        result["ms"].update(ms)

    print("a +inf fill of the planes alone (torch's fill kernel):", flush=True)
    rounds({"fill": lambda: depth.fill_(float("inf"))}, {"fill": a.reps})
    for name, (pts, nrm, rad) in clouds.items():
        P = len(pts)
        pd, nd, rd = (torch.from_numpy(np.ascontiguousarray(x)).to(dev) for x in (pts, nrm, rad))
        shipped = f"surfel_depth_{name}_shipped"
        calls = {shipped: lambda: L.check(lib.cgs_surfel_depth(P, L.ptr(pd), L.ptr(nd), L.ptr(rd), V, L.ptr(Kd), L.ptr(Md), H, W,
                                                               L.ptr(depth), stream), "cgs_surfel_depth")}
        reps = {shipped: a.reps if name != "B" else a.heavy_reps}
        calls[shipped]()
        torch.cuda.synchronize()
        result["covered_pixels"][name] = int(torch.isfinite(depth).sum())
        if alt is not None:
            variants = [("thread", 0, 0), ("wave", 1, 0)] + [(f"hybrid_{t}", 2, t) for t in a.thresholds]
            for label, geometry, small_max in variants:
                def call(geometry=geometry, small_max=small_max):
                    other.fill_(float("inf"))
                    assert alt(geometry, P, L.ptr(pd), L.ptr(nd), L.ptr(rd), V, L.ptr(Kd), L.ptr(Md), H, W, small_max, L.ptr(other),
                               stream) == 0
                call()
                torch.cuda.synchronize()
                assert same(other, depth), f"{name}: the {label} geometry's planes differ from the library's"
                key = f"surfel_depth_{name}_{label}"
                calls[key] = call
                heavy = name == "B" or (label == "wave") or (label == "thread" and name == "C")
                reps[key] = a.heavy_reps if heavy else a.reps
            print(f"cgs_surfel_depth, {name}: every geometry's planes equal the library's bit for bit", flush=True)
        print(f"cgs_surfel_depth, {name}: {P} surfels, {result['covered_pixels'][name]} covered pixels of {V * H * W}", flush=True)
        rounds(calls, reps)
        if name == "A":
            tris = sphere_mesh(224)
            td = torch.from_numpy(tris).to(dev)
            print(f"cgs_mesh_depth on the {len(tris)} triangles of the same sphere:", flush=True)
            rounds({"mesh_depth_sphere": lambda: L.check(lib.cgs_mesh_depth(len(tris), L.ptr(td), V, L.ptr(Kd), L.ptr(Md), H, W,
                                                                             L.ptr(other), stream), "cgs_mesh_depth")},
                   {"mesh_depth_sphere": a.reps})
            torch.cuda.synchronize()
            both = torch.isfinite(other) & torch.isfinite(depth)
            result["sphere"] = {"faces": len(tris), "mesh_pixels": int(torch.isfinite(other).sum()),
                                "holes": int((torch.isfinite(other) & ~torch.isfinite(depth)).sum()),
                                "max_depth_difference": float((other[both] - depth[both]).abs().max())}
            print(f"  the mesh covers {result['sphere']['mesh_pixels']} pixels, the cloud leaves {result['sphere']['holes']} of them "
                  f"empty; largest depth difference {result['sphere']['max_depth_difference']:.6f}", flush=True)
    finish(result, a.out)


if __name__ == "__main__":
    main()
