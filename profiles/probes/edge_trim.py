"""python profiles/probes/edge_trim.py [--views 100] [--width 1600] [--height 1200] [--edges 2000] [--resolution 0.0005]
                                        [--drawn_every 10] [--reps 20] [--host_views 100] [--atomic_lib FILE] [--out FILE]

Times the per-sample tally of ``ops.edge_trim`` on the GPU beside the per-edge counts of ``ops.edge_support`` on the same
inputs (profiles/edge_trim.md).  The scan is the one of profiles/probes/edge_support.py: ``--views`` cameras on a sphere
around the unit cube, ``--edges`` random edges sampled at ``--resolution``, every ``--drawn_every``-th edge drawn into every
view.

  1. ``cgs_sample_support``: the tally compared with the host back end on the first ``--host_views`` views FIRST, and its
     per-edge sums with ``cgs_edge_support``'s on all views; then ``--reps`` raw calls between device events after a
     warm-up, everything resident, at T = 3 and T = 1, and as many of ``cgs_edge_support`` in the same rounds
  2. with ``--atomic_lib`` (built from profiles/probes/edge_trim_atomic.hip): the other kernel shape -- views in blockIdx.y,
     integer atomicAdd -- checked against the first and timed in the same rounds
  3. ``trim_edges`` end to end by the wall clock around a synchronise, three times, and the library's own kernel timers."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from edge_support import draw_maps, events_ms, random_edges  # noqa: E402  (the sibling probe: the same scan)


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
    p.add_argument("--atomic_lib", default=None)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    import torch
    from curve_gaussian_amd import _lib as L
    from curve_gaussian_amd.edge_extraction.novel_view import camera_arrays
    from curve_gaussian_amd.ops import edge_score as ES
    from curve_gaussian_amd.ops import edge_support as SP
    from curve_gaussian_amd.ops import edge_trim as ET
    if not torch.cuda.is_available():
        raise SystemExit("edge_trim: needs a GPU; nothing is measured without one")
    dev = torch.device("cuda", 0)
    H, W, V = a.height, a.width, a.views
    edge_dict = random_edges(a.edges)
    pts, off = SP.sample_edges(edge_dict["curves_ctl_pts"], edge_dict["lines_end_pts"], a.resolution)
    E, P = len(off) - 1, len(pts)
    drawn = np.zeros(P, bool)
    is_drawn = np.arange(E) % a.drawn_every == 0
    for e in np.nonzero(is_drawn)[0]:
        drawn[off[e]:off[e + 1]] = True
    t0 = time.perf_counter()
    cams, maps = draw_maps(pts[drawn], V, H, W)
    print(f"{E} edges, {P} samples; {V} views {W}x{H} drawn in {time.perf_counter() - t0:.1f} s; "
          f"detected pixels {(maps > 127).mean():.5f}", flush=True)
    result = {"views": V, "width": W, "height": H, "edges": E, "points": P, "resolution": a.resolution,
              "drawn_every": a.drawn_every, "device": torch.cuda.get_device_name(dev)}
    d2 = ES.edt_squared(torch.from_numpy((maps > 127).astype(np.uint8)).to(dev), backend="gpu", device=dev)

    # 1. equality first
    intr, w2c = camera_arrays(cams)
    lib, stream = L.load(), L.raw_stream(dev)
    pts_d, off_d = torch.from_numpy(pts).to(dev), torch.from_numpy(off).to(dev)
    Kd, Md = torch.from_numpy(intr).to(dev), torch.from_numpy(np.ascontiguousarray(w2c.reshape(V, 12))).to(dev)
    hv = max(1, min(a.host_views, V))
    tol = SP.TOLERANCES_PX
    d2_h = d2[:hv].cpu().numpy()
    t0 = time.perf_counter()
    want = ET.sample_tally(pts, intr[:hv], w2c[:hv], d2_h, tol, backend="host")
    t_host = time.perf_counter() - t0
    del d2_h
    got = ET.sample_tally(pts_d, intr[:hv], w2c[:hv], d2[:hv], tol, backend="gpu")
    assert torch.equal(got.cpu(), want), "cgs_sample_support disagrees with the host back end"
    if hv < V:
        ET.sample_tally(pts_d, intr[hv:], w2c[hv:], d2[hv:], tol, backend="gpu", out=got)
    counts = SP.support_counts(pts_d, off, intr, w2c, d2, tol, backend="gpu")
    run = torch.cat([torch.zeros((1, 4), dtype=torch.int64, device=dev), torch.cumsum(got.long(), 0)])
    off_l = off_d.long()
    assert torch.equal(run[off_l[1:]] - run[off_l[:-1]], counts.long().sum(1)), "the edge sums disagree with cgs_edge_support"
    print(f"equal to the host back end on {hv} views and, summed per edge, to cgs_edge_support on {V}; "
          f"{got[:, 0].sum().item()} seen sample-views of {P * V}, {got[:, 2].sum().item()} of them within {tol[1]} px; "
          f"backend=host: sample_tally {t_host:.2f} s for {hv} views", flush=True)
    result["host"] = {"views_timed": hv, "sample_tally_seconds": t_host}
    whole = got
    del counts, run

    # 2. the times, the kernels of a round one after the other
    alt = None
    if a.atomic_lib:
        alt = ctypes.CDLL(os.path.abspath(a.atomic_lib)).sample_support_atomic
        alt.restype, alt.argtypes = L.SIGNATURES["cgs_sample_support"]
    for T in (3, 1):
        tol_d = torch.tensor(ES.tolerances_squared(tol[:T]), dtype=torch.int32).to(dev)
        tally = torch.zeros((P, 1 + T), dtype=torch.int32, device=dev)
        out = torch.empty((E, V, 1 + T), dtype=torch.int32, device=dev)
        calls = {
            "sample_support": lambda: L.check(lib.cgs_sample_support(P, L.ptr(pts_d), V, L.ptr(Kd), L.ptr(Md), H, W, L.ptr(d2), T,
                                                                     L.ptr(tol_d), L.ptr(tally), stream), "cgs_sample_support"),
            "edge_support": lambda: L.check(lib.cgs_edge_support(E, P, L.ptr(pts_d), L.ptr(off_d), V, L.ptr(Kd), L.ptr(Md), H, W,
                                                                 L.ptr(d2), T, L.ptr(tol_d), L.ptr(out), stream), "cgs_edge_support")}
        if alt is not None:
            calls["sample_support_atomic"] = lambda: L.check(alt(P, L.ptr(pts_d), V, L.ptr(Kd), L.ptr(Md), H, W, L.ptr(d2), T,
                                                                 L.ptr(tol_d), L.ptr(tally), stream), "sample_support_atomic")
        for name, call in calls.items():   # the warm-up; every tally kernel once from a zeroed tally: the same integers
            tally.zero_()
            call()
            assert name == "edge_support" or torch.equal(tally, whole[:, :1 + T]), f"{name} disagrees at T={T}"
        torch.cuda.synchronize()
        ms = {name: [] for name in calls}
        for _ in range(3):
            for name, call in calls.items():
                ms[name].append(events_ms(torch, call, a.reps))
        for name, t in ms.items():
            print(f"{name} T={T}: {[round(x, 4) for x in t]} ms per call over {a.reps} calls each; "
                  f"{P * V / min(t) / 1e6:.1f} G sample-views per second", flush=True)
            result[f"{name}_T{T}_ms"] = t
    del tally, out, whole, d2

    # 3. end to end
    runs = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = ET.trim_edges(edge_dict, cams, maps, "PidiNet", resolution=a.resolution, backend="gpu", device=dev)
        torch.cuda.synchronize()
        runs.append(time.perf_counter() - t0)
    n = np.diff(off.astype(np.int64))
    kept = np.array([sum(b - a_ + 1 for a_, b in s) for s in res["spans"]], np.int64)
    whole_edges = np.array([s == [(0, int(k) - 1)] for s, k in zip(res["spans"], n)])
    print(f"trim_edges end to end: {[round(r, 3) for r in runs]} s; {len(res['source'])} pieces of {E} edges, "
          f"{int(kept.sum())} of {P} samples kept ({int(kept[is_drawn].sum())} of {int(n[is_drawn].sum())} on the drawn edges, "
          f"{int(whole_edges[is_drawn].sum())} of the {int(is_drawn.sum())} drawn edges whole)", flush=True)
    result.update({"trim_edges_seconds": runs, "pieces": int(len(res["source"])), "kept_samples": int(kept.sum()),
                   "kept_samples_drawn": int(kept[is_drawn].sum()), "samples_drawn": int(n[is_drawn].sum()),
                   "drawn_whole": int(whole_edges[is_drawn].sum())})
    lib.cgs_prof_reset()
    lib.cgs_prof_enable(1)
    ET.trim_edges(edge_dict, cams, maps, "PidiNet", resolution=a.resolution, backend="gpu", device=dev)
    torch.cuda.synchronize()
    prof = L.prof_collect()
    lib.cgs_prof_enable(0)
    for name, (kms, k) in sorted(prof.items()):
        print(f"  {name}: {kms:.3f} ms in {k} launches", flush=True)
    result["kernels_ms"] = {k: v[0] for k, v in prof.items()}
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
