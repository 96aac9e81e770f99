"""python profiles/probes/edge_occlusion.py [--views 100] [--width 1600] [--height 1200] [--grid 224] [--edges 4000]
                                             [--samples 100] [--reps 20] [--thread_lib FILE] [--check_faces 4000] [--out FILE]
                                             [--clip] [--only_clip] [--parent_lib FILE]

Times the three occlusion kernels (profiles/edge_occlusion.md), everything resident, raw calls between device events after
a warm-up, three rounds, the variants alternating within a round:

  cgs_mesh_depth on a FINE mesh: a sphere of 2 x grid x grid triangles (100 352 at the default, a few pixels each) and on a
      COARSE one: the 12 triangles of a box that fills every image; with ``--thread_lib`` (built from
      profiles/probes/edge_occlusion_thread.hip) the other geometry -- one thread per (triangle, view) -- on both, after its
      planes are compared with the library's bit for bit.  The library's call includes the +inf fill and the other
      geometry's is timed behind a fill of the same planes; the fill alone is timed too.
  cgs_depth_window_max at radius 1 and 4.
  cgs_point_mask_depth beside cgs_point_mask on the samples of profiles/probes/edge_dedupe.py (400 708 at the defaults),
      gated by the fine mesh's planes.

``--clip`` (profiles/edge_clip.md): cgs_mesh_depth_clipped beside cgs_mesh_depth on the two meshes above -- seen from
      outside, every vertex in front of the plane, so nothing is clipped and the planes must be equal bit for bit -- and, with
      ``--parent_lib`` (a ``libcurvegs.so`` built from the commit before the clipping), beside that library's cgs_mesh_depth
      in the same rounds; then the INDOOR case: the 24 coarse triangles of ``solid_scan``'s room with ``--views`` cameras
      inside it, clipped (first view compared with the host back end) and unclipped.  ``--only_clip`` skips the rest.

Before anything is timed the planes of the first ``--check_faces`` triangles of the fine mesh and of the coarse mesh in the
first view, and the gated masks of the first two views, are compared with the host back end bit for bit."""
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
from edge_orient import sphere_cameras  # noqa: E402
from edge_support import events_ms  # noqa: E402


def sphere_mesh(grid, radius=0.45, centre=0.5):
    """float32 [2 grid^2, 3, 3]: a latitude / longitude sphere (the caps' triangles are degenerate and skipped by the rule)."""
    th = np.linspace(0.0, np.pi, grid + 1)[:, None]
    ph = np.linspace(0.0, 2.0 * np.pi, grid + 1)[None, :]
    p = centre + radius * np.stack([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th) * np.ones_like(ph)], 2)
    a, b, c, d = p[:-1, :-1], p[1:, :-1], p[1:, 1:], p[:-1, 1:]
    return np.concatenate([np.stack([a, b, c], 2).reshape(-1, 3, 3), np.stack([a, c, d], 2).reshape(-1, 3, 3)]).astype(np.float32)


def box_mesh(lo=-0.2, hi=1.2):
    """float32 [12,3,3]: a cube around the cameras' target that fills every image."""
    from curve_gaussian_amd.scene.solid_scan import _prism
    tris, _ = _prism([(lo, lo), (hi, lo), (hi, hi), (lo, hi)], lo, hi)
    return np.asarray(tris, np.float32).reshape(-1, 3, 3)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--views", type=int, default=100)
    p.add_argument("--width", type=int, default=1600)
    p.add_argument("--height", type=int, default=1200)
    p.add_argument("--grid", type=int, default=224)
    p.add_argument("--edges", type=int, default=4000)
    p.add_argument("--samples", type=int, default=100)
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--thread_lib", default=None)
    p.add_argument("--check_faces", type=int, default=4000)
    p.add_argument("--out", default=None)
    p.add_argument("--clip", action="store_true")
    p.add_argument("--only_clip", action="store_true")
    p.add_argument("--parent_lib", default=None)
    a = p.parse_args()
    import torch
    from curve_gaussian_amd import _lib as L
    from curve_gaussian_amd.ops import edge_occlusion as EO
    from curve_gaussian_amd.ops import edge_score as ES
    if not torch.cuda.is_available():
        raise SystemExit("edge_occlusion: needs a GPU; nothing is measured without one")
    dev = torch.device("cuda", 0)
    H, W, V = a.height, a.width, a.views
    lib, stream = L.load(), L.raw_stream(dev)
    K, M = sphere_cameras(V, H, W)
    Kd, Md = ES.cameras_on(dev, K, np.ascontiguousarray(M.reshape(V, 12)))
    meshes = {"fine": sphere_mesh(a.grid), "coarse": box_mesh()}
    pts, _ = straight_edges(a.edges, a.samples, 0.001)
    P = len(pts)
    same = lambda x, y: bool(torch.equal(x.cpu().view(torch.int32), y.cpu().view(torch.int32)))

    # equality first
    for name, tris in meshes.items():
        part = tris[:a.check_faces]
        want = EO.mesh_depth(part, K[:1], M[:1], H, W, window=1, backend="host")
        assert same(EO.mesh_depth(part, K[:1], M[:1], H, W, window=1), want), f"{name}: cgs_mesh_depth disagrees with the host"
    planes = EO.mesh_depth(meshes["fine"], K, M, H, W, window=1)
    want = EO.point_masks_depth(pts, K[:2], M[:2], planes[:2].cpu(), EO.DEPTH_SLACK, backend="host", return_counts=True)
    got = EO.point_masks_depth(pts, K[:2], M[:2], planes[:2], EO.DEPTH_SLACK, return_counts=True)
    assert all(torch.equal(g.cpu(), w) for g, w in zip(got, want)), "cgs_point_mask_depth disagrees with the host"
    print(f"{V} views {W}x{H}: equal to the host back end on {min(a.check_faces, len(meshes['fine']))} + 12 triangles x 1 view "
          f"and on {P} samples x 2 views", flush=True)

    alt = None
    if a.thread_lib:
        alt = ctypes.CDLL(os.path.abspath(a.thread_lib)).mesh_depth_thread
        alt.restype = ctypes.c_int
        alt.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, ctypes.c_int,
                        ctypes.c_void_p, ctypes.c_void_p]
    depth = torch.empty((V, H, W), dtype=torch.float32, device=dev)
    other = torch.empty_like(depth)
    result = {"views": V, "width": W, "height": H, "rounds": 3, "device": torch.cuda.get_device_name(dev), "ms": {}}

    def rounds(calls, reps):
        for call in calls.values():   # the warm-up
            call()
        torch.cuda.synchronize()
        ms = {name: [] for name in calls}
        for _ in range(3):
            for name, call in calls.items():
                ms[name].append(events_ms(torch, call, reps[name] if isinstance(reps, dict) else reps))
        for name, t in ms.items():
            print(f"  {name}: {[round(x, 3) for x in t]} ms per call", flush=True)
        result["ms"].update(ms)

    def finish():
        line = json.dumps(result)
        print(line)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(line + "\n")

    if a.clip or a.only_clip:
        near = EO.NEAR_CLIP
        parent = None
        if a.parent_lib:
            parent = ctypes.CDLL(os.path.abspath(a.parent_lib))
            parent.cgs_mesh_depth.restype, parent.cgs_mesh_depth.argtypes = L.SIGNATURES["cgs_mesh_depth"]
        for name, tris in meshes.items():
            F = len(tris)
            t_d = torch.from_numpy(tris).to(dev)
            calls = {f"clip_{name}_unclipped": lambda: L.check(lib.cgs_mesh_depth(
                         F, L.ptr(t_d), V, L.ptr(Kd), L.ptr(Md), H, W, L.ptr(depth), stream), "cgs_mesh_depth"),
                     f"clip_{name}_clipped": lambda: L.check(lib.cgs_mesh_depth_clipped(
                         F, L.ptr(t_d), V, L.ptr(Kd), L.ptr(Md), H, W, near, L.ptr(other), stream), "cgs_mesh_depth_clipped")}
            if parent is not None:
                calls[f"clip_{name}_parent"] = lambda: L.check(parent.cgs_mesh_depth(
                    F, L.ptr(t_d), V, L.ptr(Kd), L.ptr(Md), H, W, L.ptr(depth), stream), "cgs_mesh_depth [parent]")
                calls[f"clip_{name}_parent"]()
                torch.cuda.synchronize()
                kept = depth.clone()
            calls[f"clip_{name}_unclipped"]()
            calls[f"clip_{name}_clipped"]()
            torch.cuda.synchronize()
            assert same(depth, other), f"{name}: the clipped entry's planes differ from the unclipped one's"
            if parent is not None:
                assert same(depth, kept), f"{name}: this build and the parent write different bits"
                del kept
            print(f"clipping, {name}: {F} triangles seen from outside, clipped == unclipped"
                  + (" == the parent build's" if parent is not None else "") + " bit for bit", flush=True)
            rounds(calls, a.reps)
        from curve_gaussian_amd.ops.view_chunks import camera_arrays
        from curve_gaussian_amd.scene import solid_scan as SS
        room, _ = SS.solid_geometry("room")
        Kr, Mr = camera_arrays(SS.emap_cameras_of(SS.room_cameras(V, H, W)))
        want = EO.mesh_depth(room, Kr[:1], Mr[:1], H, W, window=0, backend="host", near_clip=near)
        assert same(EO.mesh_depth(room, Kr[:1], Mr[:1], H, W, window=0, near_clip=near), want), "room: disagrees with the host"
        Krd, Mrd = ES.cameras_on(dev, Kr, np.ascontiguousarray(np.asarray(Mr).reshape(V, 12)))
        r_d = torch.from_numpy(room).to(dev)
        calls = {"clip_room_clipped": lambda: L.check(lib.cgs_mesh_depth_clipped(
                     len(room), L.ptr(r_d), V, L.ptr(Krd), L.ptr(Mrd), H, W, near, L.ptr(other), stream), "cgs_mesh_depth_clipped"),
                 "clip_room_unclipped": lambda: L.check(lib.cgs_mesh_depth(
                     len(room), L.ptr(r_d), V, L.ptr(Krd), L.ptr(Mrd), H, W, L.ptr(depth), stream), "cgs_mesh_depth")}
        calls["clip_room_clipped"]()
        calls["clip_room_unclipped"]()
        torch.cuda.synchronize()
        result["room"] = {"faces": len(room), "inf_pixels_clipped": int(torch.isinf(other).sum()),
                          "inf_pixels_unclipped": int(torch.isinf(depth).sum()), "pixels": V * H * W, "near": near}
        print(f"clipping, room: {len(room)} triangles, cameras inside, first view equal to the host; +inf pixels "
              f"{result['room']['inf_pixels_clipped']} clipped, {result['room']['inf_pixels_unclipped']} unclipped of {V * H * W}",
              flush=True)
        rounds(calls, a.reps)
        result.update({"faces": {k: len(v) for k, v in meshes.items()}, "reps": a.reps, "parent": bool(a.parent_lib)})
        if a.only_clip:
            finish()
            return

    print("a +inf fill of the planes alone (torch's fill kernel):", flush=True)
    rounds({"fill": lambda: depth.fill_(float("inf"))}, a.reps)
    for name, tris in meshes.items():
        F = len(tris)
        t_d = torch.from_numpy(tris).to(dev)
        calls = {f"mesh_depth_{name}_wave": lambda: L.check(lib.cgs_mesh_depth(
            F, L.ptr(t_d), V, L.ptr(Kd), L.ptr(Md), H, W, L.ptr(depth), stream), "cgs_mesh_depth")}
        reps = {f"mesh_depth_{name}_wave": a.reps}
        if alt is not None:
            other.fill_(float("inf"))
            assert alt(F, L.ptr(t_d), V, L.ptr(Kd), L.ptr(Md), H, W, L.ptr(other), stream) == 0
            calls[f"mesh_depth_{name}_wave"]()
            torch.cuda.synchronize()
            assert same(other, depth), f"{name}: the thread geometry's planes differ from the library's"
            # (its call does not fill: a fill of the same planes goes in front, as inside the library's call)
            calls[f"mesh_depth_{name}_thread"] = lambda: (other.fill_(float("inf")),
                                                          alt(F, L.ptr(t_d), V, L.ptr(Kd), L.ptr(Md), H, W, L.ptr(other), stream))
            reps[f"mesh_depth_{name}_thread"] = a.reps if name == "fine" else 2
        print(f"cgs_mesh_depth, {name}: {F} triangles, {int(torch.isfinite(depth).sum()) if alt else '-'} covered pixels", flush=True)
        rounds(calls, reps)
    fine_d = torch.from_numpy(meshes["fine"]).to(dev)
    L.check(lib.cgs_mesh_depth(len(meshes["fine"]), L.ptr(fine_d), V, L.ptr(Kd), L.ptr(Md), H, W, L.ptr(depth), stream),
            "cgs_mesh_depth")
    print("cgs_depth_window_max:", flush=True)
    rounds({f"window_max_r{r}": (lambda r=r: L.check(lib.cgs_depth_window_max(V, H, W, r, L.ptr(depth), L.ptr(other), stream),
                                                      "cgs_depth_window_max")) for r in (1, 4)}, a.reps)
    L.check(lib.cgs_depth_window_max(V, H, W, 1, L.ptr(depth), L.ptr(other), stream), "cgs_depth_window_max")
    pts_d = torch.from_numpy(pts).to(dev)
    mask = torch.empty((V, H, W), dtype=torch.uint8, device=dev)
    kept = torch.empty((V,), dtype=torch.int32, device=dev)
    hidden = torch.empty((V,), dtype=torch.int32, device=dev)
    print(f"the masks of {P} samples:", flush=True)
    rounds({"point_mask_depth": lambda: L.check(lib.cgs_point_mask_depth(
                P, L.ptr(pts_d), V, L.ptr(Kd), L.ptr(Md), H, W, L.ptr(other), EO.DEPTH_SLACK, L.ptr(mask), L.ptr(kept), L.ptr(hidden),
                stream), "cgs_point_mask_depth"),
            "point_mask": lambda: L.check(lib.cgs_point_mask(P, L.ptr(pts_d), V, L.ptr(Kd), L.ptr(Md), H, W, L.ptr(mask),
                                                             L.ptr(kept), stream), "cgs_point_mask")}, a.reps)
    result.update({"points": P, "faces": {k: len(v) for k, v in meshes.items()}, "reps": a.reps,
                   "hidden_sample_views": int(hidden.sum())})
    finish()


if __name__ == "__main__":
    main()
