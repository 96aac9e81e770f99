"""python profiles/probes/edge_snap.py [--views 100] [--width 1600] [--height 1200] [--distinct 10] [--segments 150]
                                        [--edges 4000] [--samples 100] [--capture 3] [--reps 50] [--host_views 2]
                                        [--check_samples 20000] [--out FILE]

Times ``cgs_sample_snap_terms`` beside ``cgs_sample_support`` (profiles/edge_snap.md) on the tally workload of
profiles/probes/edge_orient.py: the samples of profiles/probes/edge_dedupe.py (400 708 at the defaults) in ``--views``
cameras on a sphere around the unit cube, against the distance transform of three-pixel strokes.  Everything resident, raw
calls between device events after a warm-up, the two kernels alternating within each of three rounds.

Before anything is timed the terms of the first ``--check_samples`` samples in the first ``--host_views`` views are compared
with the host back end bit for bit, and two calls over halves of the views with one call over all of them.  The words a
kernel gathers from the transform are counted from the shapes and the tallies and printed."""
import argparse
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
from edge_thin import dilate, segment_views  # noqa: E402


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--views", type=int, default=100)
    p.add_argument("--width", type=int, default=1600)
    p.add_argument("--height", type=int, default=1200)
    p.add_argument("--distinct", type=int, default=10)
    p.add_argument("--segments", type=int, default=150)
    p.add_argument("--edges", type=int, default=4000)
    p.add_argument("--samples", type=int, default=100)
    p.add_argument("--capture", type=float, default=3.0)
    p.add_argument("--reps", type=int, default=50)
    p.add_argument("--host_views", type=int, default=2)
    p.add_argument("--check_samples", type=int, default=20000)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    import torch
    from curve_gaussian_amd import _lib as L
    from curve_gaussian_amd.ops import edge_score as ES
    from curve_gaussian_amd.ops import edge_snap as SN
    if not torch.cuda.is_available():
        raise SystemExit("edge_snap: needs a GPU; nothing is measured without one")
    dev = torch.device("cuda", 0)
    H, W, V = a.height, a.width, a.views
    lib, stream = L.load(), L.raw_stream(dev)
    cap2 = SN.capture_squared(a.capture)
    hv = max(1, min(a.host_views, a.distinct, V))
    thick = dilate(segment_views(min(a.distinct, V), H, W, a.segments), 1)
    d2 = ES.edt_squared(torch.from_numpy(np.tile(thick, (-(-V // thick.shape[0]), 1, 1))[:V]).to(dev), backend="gpu", device=dev)
    pts, off = straight_edges(a.edges, a.samples, 0.001)
    P = len(pts)
    K, M = sphere_cameras(V, H, W)

    # equality first
    pc = min(P, a.check_samples)
    want = SN.snap_terms(pts[:pc], K[:hv], M[:hv], d2[:hv].cpu(), a.capture, backend="host")
    got = SN.snap_terms(pts[:pc], K[:hv], M[:hv], d2[:hv], a.capture)
    same = lambda x, y: bool(torch.equal(x[0].cpu().view(torch.int64), y[0].cpu().view(torch.int64)) and torch.equal(x[1].cpu(), y[1].cpu()))
    assert same(got, want), "cgs_sample_snap_terms disagrees with the host back end"
    pts_d = torch.from_numpy(pts).to(dev)
    whole = SN.snap_terms(pts_d, K, M, d2, a.capture)
    halves = SN.snap_terms(pts_d, K[:V // 2], M[:V // 2], d2[:V // 2], a.capture)
    SN.snap_terms(pts_d, K[V // 2:], M[V // 2:], d2[V // 2:], a.capture, out=halves)
    assert same(halves, whole), "two calls over halves of the views are not one call over all of them"
    captured = int(whole[1].sum())

    Kd, Md = ES.cameras_on(dev, K, np.ascontiguousarray(M.reshape(V, 12)))
    tol_d = torch.tensor([1], dtype=torch.int32).to(dev)
    lut_d = torch.from_numpy(SN.distance_table(cap2)).to(dev)
    tally = torch.zeros((P, 2), dtype=torch.int32, device=dev)
    terms = torch.zeros((P, SN.TERMS), dtype=torch.float64, device=dev)
    views = torch.zeros((P,), dtype=torch.int32, device=dev)
    calls = {
        "sample_snap_terms": lambda: L.check(lib.cgs_sample_snap_terms(
            P, L.ptr(pts_d), V, L.ptr(Kd), L.ptr(Md), H, W, L.ptr(d2), cap2, L.ptr(lut_d), L.ptr(terms), L.ptr(views), stream),
            "cgs_sample_snap_terms"),
        "sample_support": lambda: L.check(lib.cgs_sample_support(P, L.ptr(pts_d), V, L.ptr(Kd), L.ptr(Md), H, W, L.ptr(d2), 1,
                                                                 L.ptr(tol_d), L.ptr(tally), stream), "cgs_sample_support")}
    for call in calls.values():   # the warm-up, from zeroed sums
        call()
    torch.cuda.synchronize()
    assert same((terms, views), whole), "the raw call disagrees with snap_terms"
    seen = int(tally[:, 0].sum())
    print(f"{P} samples x {V} views {W}x{H}, capture {a.capture:g} px: equal to the host back end on {pc} samples x {hv} views, "
          f"chunk-invariant on all; {seen} seen sample-views, {captured} captured", flush=True)
    ms = {name: [] for name in calls}
    for _ in range(3):
        for name, call in calls.items():
            ms[name].append(events_ms(torch, call, a.reps))
    # every seen sample-view whose footprint lies inside the plane reads four words; the count of those lies between the
    # captured and the seen sample-views, so the bounds below bracket the words gathered
    words = {"sample_snap_terms": [4 * captured, 4 * seen], "sample_support": [seen, seen]}
    for name, t in ms.items():
        print(f"  {name}: {[round(x, 3) for x in t]} ms per call over {a.reps} calls each; {P * V / min(t) / 1e6:.1f} G "
              f"sample-views per second; between {words[name][0]} and {words[name][1]} words of 4 bytes gathered", flush=True)
    result = {"views": V, "width": W, "height": H, "points": P, "cap2": cap2, "reps": a.reps, "rounds": 3, "seen": seen,
              "captured": captured, "ms": ms, "gathered_words": words, "device": torch.cuda.get_device_name(dev)}
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
