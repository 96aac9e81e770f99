"""python profiles/probes/edge_support.py [--views 100] [--width 1600] [--height 1200] [--edges 2000] [--resolution 0.0005]
                                           [--drawn_every 10] [--reps 20] [--host_views 100] [--out FILE]

Times the per-edge 2D support of ``ops.edge_support`` on the GPU (profiles/edge_support.md).  The scan: ``--views`` cameras
on a sphere around the unit cube, ``--edges`` random edges in it (half lines, half Bezier curves) sampled at
``--resolution`` by ``sample_edges``, and edge maps that draw the samples of every ``--drawn_every``-th edge into every
view, so that those edges have support and the others only where they cross a drawn one.

  1. ``edt_squared`` of the detected masks of all views, one call between device events (three times)
  2. ``cgs_edge_support``: the result compared with the host back end on the first ``--host_views`` views FIRST, then
     ``--reps`` raw calls between device events after a warm-up, everything resident, at T = 3 and T = 1
  3. the host back end's time on the same inputs (``--host_views`` views; SCALED to the scan and said to be when fewer)
  4. ``edge_support`` end to end by the wall clock around a synchronise, three times."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def random_edges(n, seed=0):
    """{"curves_ctl_pts": [n/2,12], "lines_end_pts": [n - n/2,6]} in the unit cube; a curve's inner control points lie near
    its chord."""
    rng = np.random.default_rng(seed)
    a, b = rng.uniform(0.1, 0.9, (n, 3)), rng.uniform(0.1, 0.9, (n, 3))
    nc = n // 2
    bend = rng.normal(0.0, 0.05, (nc, 2, 3))
    ctl = np.stack([a[:nc], a[:nc] + (b[:nc] - a[:nc]) / 3 + bend[:, 0], a[:nc] + 2 * (b[:nc] - a[:nc]) / 3 + bend[:, 1], b[:nc]], 1)
    return {"curves_ctl_pts": ctl.reshape(nc, 12).tolist(), "lines_end_pts": np.concatenate([a[nc:], b[nc:]], 1).tolist()}


def draw_maps(pts, V, H, W):
    """(NovelViewCamera s, uint8 [V,H,W] PidiNet-style maps): every point sets its pixel in every view."""
    from curve_gaussian_amd import synthetic as S
    from curve_gaussian_amd.edge_extraction.novel_view import NovelViewCamera
    pts = pts.astype(np.float64)
    cams, maps = [], np.zeros((V, H, W), np.uint8)
    for k, c in enumerate(S.fibonacci_cameras(V, H, W)):
        w2c = c.world_view_transform.double().numpy().T
        fx, fy = W / (2 * math.tan(c.FoVx / 2)), H / (2 * math.tan(c.FoVy / 2))
        cam = pts @ w2c[:3, :3].T + w2c[:3, 3]
        u, v = fx * cam[:, 0] / cam[:, 2] + W / 2.0, fy * cam[:, 1] / cam[:, 2] + H / 2.0
        ok = (cam[:, 2] > 0) & (u >= 0) & (u < W) & (v >= 0) & (v < H)
        maps[k, np.floor(v[ok]).astype(int), np.floor(u[ok]).astype(int)] = 255
        cams.append(NovelViewCamera(f"v{k}", np.ascontiguousarray(w2c[:3, :3]), w2c[:3, 3].copy(), fx, fy, W / 2.0, H / 2.0, W, H))
    return cams, maps


def events_ms(torch, call, reps):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        call()
    stop.record()
    torch.cuda.synchronize()
    return start.elapsed_time(stop) / reps


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--views", type=int, default=100)
    p.add_argument("--width", type=int, default=1600)
    p.add_argument("--height", type=int, default=1200)
    p.add_argument("--edges", type=int, default=2000)
    p.add_argument("--resolution", type=float, default=0.0005)
    p.add_argument("--drawn_every", type=int, default=10)
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--host_views", type=int, default=100)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    import torch
    from curve_gaussian_amd import _lib as L
    from curve_gaussian_amd.edge_extraction.novel_view import camera_arrays
    from curve_gaussian_amd.ops import edge_score as ES
    from curve_gaussian_amd.ops import edge_support as SP
    if not torch.cuda.is_available():
        raise SystemExit("edge_support: needs a GPU; nothing is measured without one")
    dev = torch.device("cuda", 0)
    H, W, V = a.height, a.width, a.views
    edge_dict = random_edges(a.edges)
    t0 = time.perf_counter()
    pts, off = SP.sample_edges(edge_dict["curves_ctl_pts"], edge_dict["lines_end_pts"], a.resolution)
    t_sample = time.perf_counter() - t0
    E, P = len(off) - 1, len(pts)
    drawn = np.zeros(P, bool)
    is_drawn = np.arange(E) % a.drawn_every == 0
    for e in np.nonzero(is_drawn)[0]:
        drawn[off[e]:off[e + 1]] = True
    t0 = time.perf_counter()
    cams, maps = draw_maps(pts[drawn], V, H, W)
    print(f"{E} edges, {P} samples (sample_edges {t_sample:.2f} s); {V} views {W}x{H} drawn in {time.perf_counter() - t0:.1f} s; "
          f"detected pixels {(maps > 127).mean():.5f}", flush=True)
    result = {"views": V, "width": W, "height": H, "edges": E, "points": P, "resolution": a.resolution,
              "drawn_every": a.drawn_every, "sample_edges_seconds": t_sample, "device": torch.cuda.get_device_name(dev)}

    # 1. the distance transform of all views
    det = torch.from_numpy((maps > 127).astype(np.uint8)).to(dev)
    d2 = ES.edt_squared(det, backend="gpu", device=dev)
    torch.cuda.synchronize()
    edt_ms = [events_ms(torch, lambda: ES.edt_squared(det, backend="gpu", device=dev), 1) for _ in range(3)]
    print(f"edt_squared of {V} views: {[round(t, 3) for t in edt_ms]} ms per call (allocation of its outputs included)", flush=True)
    result["edt_squared_ms"] = edt_ms
    del det

    # 2. the kernel: equality first, then the time
    intr, w2c = camera_arrays(cams)
    lib, stream = L.load(), L.raw_stream(dev)
    pts_d, off_d = torch.from_numpy(pts).to(dev), torch.from_numpy(off).to(dev)
    Kd, Md = torch.from_numpy(intr).to(dev), torch.from_numpy(np.ascontiguousarray(w2c.reshape(V, 12))).to(dev)
    hv = max(1, min(a.host_views, V))
    tol = SP.TOLERANCES_PX
    d2_h = d2[:hv].cpu().numpy()
    t0 = time.perf_counter()
    want = SP.support_counts(pts, off, intr[:hv], w2c[:hv], d2_h, tol, backend="host")
    t_host = time.perf_counter() - t0
    del d2_h
    got = SP.support_counts(pts_d, off, intr, w2c, d2, tol, backend="gpu")
    assert torch.equal(got[:, :hv].cpu(), want), "cgs_edge_support disagrees with the host back end"
    seen = got[:, :, 0].sum().item()
    print(f"equal to the host back end on {hv} views; {seen} seen samples of {P * V}, "
          f"{got[:, :, 2].sum().item()} of them within {tol[1]} px", flush=True)
    scaled = t_host / hv * V
    print(f"backend=host: support_counts {t_host:.2f} s for {hv} views of the same points"
          + ("" if hv == V else f"; SCALED to {V} views: {scaled:.1f} s"), flush=True)
    result["host"] = {"views_timed": hv, "support_counts_seconds": t_host, "scaled_seconds": scaled}
    for T in (3, 1):
        tol_d = torch.tensor(ES.tolerances_squared(tol[:T]), dtype=torch.int32).to(dev)
        out = torch.empty((E, V, 1 + T), dtype=torch.int32, device=dev)
        call = lambda: L.check(lib.cgs_edge_support(E, P, L.ptr(pts_d), L.ptr(off_d), V, L.ptr(Kd), L.ptr(Md), H, W, L.ptr(d2), T,
                                                    L.ptr(tol_d), L.ptr(out), stream), "cgs_edge_support")
        call()
        torch.cuda.synchronize()
        ms = [events_ms(torch, call, a.reps) for _ in range(3)]
        assert torch.equal(out[:, :hv].cpu(), want[:, :, :1 + T])
        print(f"cgs_edge_support T={T}: {[round(t, 4) for t in ms]} ms per call over {a.reps} calls each; "
              f"{P * V / min(ms) / 1e6:.1f} G point-views per second", flush=True)
        result[f"edge_support_T{T}_ms"] = ms
    del got, out

    # 4. end to end
    runs = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = SP.edge_support(edge_dict, cams, maps, "PidiNet", resolution=a.resolution, backend="gpu", device=dev)
        torch.cuda.synchronize()
        runs.append(time.perf_counter() - t0)
    kept = res["kept"]
    print(f"edge_support end to end: {[round(r, 3) for r in runs]} s; kept {int(kept.sum())} of {E} edges "
          f"({int(kept[is_drawn].sum())} of the {int(is_drawn.sum())} drawn, {int(kept[~is_drawn].sum())} of the others)", flush=True)
    result.update({"edge_support_seconds": runs, "kept": int(kept.sum()), "drawn": int(is_drawn.sum()),
                   "kept_drawn": int(kept[is_drawn].sum()), "kept_not_drawn": int(kept[~is_drawn].sum())})
    lib.cgs_prof_reset()
    lib.cgs_prof_enable(1)
    SP.edge_support(edge_dict, cams, maps, "PidiNet", resolution=a.resolution, backend="gpu", device=dev)
    torch.cuda.synchronize()
    prof = L.prof_collect()
    lib.cgs_prof_enable(0)
    for name, (kms, n) in sorted(prof.items()):
        print(f"  {name}: {kms:.3f} ms in {n} launches", flush=True)
    result["kernels_ms"] = {k: v[0] for k, v in prof.items()}
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
