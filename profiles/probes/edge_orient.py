"""python profiles/probes/edge_orient.py [--views 100] [--width 1600] [--height 1200] [--distinct 10] [--segments 150]
                                          [--edges 4000] [--samples 100] [--tolerance 1] [--reps 50] [--host_views 2]
                                          [--check_samples 20000] [--out FILE]

Times the three kernels of ``ops.edge_orient`` beside the path they stand in for (profiles/edge_orient.md), everything
resident, raw calls between device events after a warm-up, the rounds alternating:

  planes   ``--views`` views of drawn strokes -- the masks of profiles/probes/edge_thin.py, one pixel wide and dilated to
           three -- through ``cgs_mask_orientation`` + ``cgs_oriented_near``; the yardstick is ``cgs_edt_squared`` of the
           same masks into a preallocated transform
  tally    the samples of profiles/probes/edge_dedupe.py (400 708 at the defaults) in ``--views`` cameras on a sphere
           around the unit cube through ``cgs_sample_support_oriented``; the yardstick is ``cgs_sample_support`` at T = 1 on
           the distance transform of the same masks

Before anything is timed the planes of the first ``--host_views`` views and the tally of the first ``--check_samples``
samples in those views are compared with the host back end (``torch.equal``), and near != 0 with the transform <= tol2 on
all views.  The bytes a kernel must move are computed from the shapes and printed with the rate they make."""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from edge_dedupe import straight_edges  # noqa: E402  (the sibling probes: the same inputs)
from edge_support import events_ms  # noqa: E402
from edge_thin import dilate, segment_views  # noqa: E402


def sphere_cameras(V, H, W):
    """(intrinsics [V,4], w2c [V,3,4]) float64 of the cameras of profiles/probes/edge_support.py."""
    from curve_gaussian_amd import synthetic as S
    K, M = np.zeros((V, 4)), np.zeros((V, 3, 4))
    for k, c in enumerate(S.fibonacci_cameras(V, H, W)):
        K[k] = W / (2 * math.tan(c.FoVx / 2)), H / (2 * math.tan(c.FoVy / 2)), W / 2.0, H / 2.0
        M[k] = c.world_view_transform.double().numpy().T[:3]
    return K, M


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--views", type=int, default=100)
    p.add_argument("--width", type=int, default=1600)
    p.add_argument("--height", type=int, default=1200)
    p.add_argument("--distinct", type=int, default=10)
    p.add_argument("--segments", type=int, default=150)
    p.add_argument("--edges", type=int, default=4000)
    p.add_argument("--samples", type=int, default=100)
    p.add_argument("--tolerance", type=float, default=1.0)
    p.add_argument("--reps", type=int, default=50)
    p.add_argument("--host_views", type=int, default=2)
    p.add_argument("--check_samples", type=int, default=20000)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    import torch
    from curve_gaussian_amd import _lib as L
    from curve_gaussian_amd.ops import edge_orient as OR
    from curve_gaussian_amd.ops import edge_score as ES
    if not torch.cuda.is_available():
        raise SystemExit("edge_orient: needs a GPU; nothing is measured without one")
    dev = torch.device("cuda", 0)
    H, W, V = a.height, a.width, a.views
    lib, stream = L.load(), L.raw_stream(dev)
    tol2 = ES.tolerances_squared([a.tolerance])[0]
    hv = max(1, min(a.host_views, a.distinct, V))
    result = {"views": V, "width": W, "height": H, "tol2": tol2, "reps": a.reps, "rounds": 3,
              "tile": [L.ORIENT_TILE_HEIGHT, L.ORIENT_TILE_WIDTH], "device": torch.cuda.get_device_name(dev), "planes": {}}
    lines = segment_views(min(a.distinct, V), H, W, a.segments)
    plane_bytes = V * H * W

    # ---- the planes
    code, near = (torch.empty((V, H, W), dtype=torch.uint8, device=dev) for _ in range(2))
    d2 = torch.empty((V, H, W), dtype=torch.int32, device=dev)
    ws = torch.empty((lib.cgs_edt_workspace_bytes(V, H, W),), dtype=torch.uint8, device=dev)
    for r in (0, 1):
        thick = dilate(lines, r)
        src = torch.from_numpy(np.tile(thick, (-(-V // thick.shape[0]), 1, 1))[:V]).to(dev)
        t0 = time.perf_counter()
        want_code = OR.mask_orientation(thick[:hv], backend="host")
        want_near = OR.oriented_near(want_code, a.tolerance, backend="host")
        t_host = time.perf_counter() - t0
        calls = {
            "mask_orientation": lambda: L.check(lib.cgs_mask_orientation(V, H, W, L.ptr(src), L.ptr(code), stream),
                                                "cgs_mask_orientation"),
            "oriented_near": lambda: L.check(lib.cgs_oriented_near(V, H, W, L.ptr(code), tol2, L.ptr(near), stream),
                                             "cgs_oriented_near"),
            "edt_squared": lambda: L.check(lib.cgs_edt_squared(V, H, W, L.ptr(src), L.ptr(ws), L.ptr(d2), stream),
                                           "cgs_edt_squared")}
        for call in calls.values():   # the warm-up, and the equality
            call()
        torch.cuda.synchronize()
        assert torch.equal(code[:hv].cpu(), want_code), "cgs_mask_orientation disagrees with the host back end"
        assert torch.equal(near[:hv].cpu(), want_near), "cgs_oriented_near disagrees with the host back end"
        assert torch.equal(near != 0, d2 <= tol2), "near != 0 is not the distance transform within the tolerance"
        oriented = float(((code != 0) & (code != 0xFF)).sum()) / max(1.0, float((code != 0).sum()))
        print(f"stroke {2 * r + 1} px ({100 * thick.mean():.2f} % set, {100 * oriented:.1f} % of the set pixels oriented): equal "
              f"to the host back end on {hv} views, near != 0 equal to edt <= {tol2} on {V}; backend=host {t_host:.2f} s for "
              f"{hv} views", flush=True)
        ms = {name: [] for name in calls}
        for _ in range(3):
            for name, call in calls.items():
                ms[name].append(events_ms(torch, call, a.reps))
        moved = {"mask_orientation": 2 * plane_bytes, "oriented_near": 2 * plane_bytes, "edt_squared": 5 * plane_bytes}
        for name, t in ms.items():
            print(f"  {name}: {[round(x, 3) for x in t]} ms per call over {a.reps} calls each; at least {moved[name] / 1e6:.0f} MB "
                  f"in and out: {moved[name] / min(t) / 1e6:.0f} GB/s", flush=True)
        result["planes"][str(2 * r + 1)] = {"set_pixels": float(thick.mean()), "oriented_share": oriented, "ms": ms,
                                            "min_bytes": moved, "host_seconds": t_host, "host_views": hv}
    del ws

    # ---- the tally, on the three-pixel strokes' planes left in near and d2
    pts, off = straight_edges(a.edges, a.samples, 0.001)
    P = len(pts)
    partner = OR.sample_partners(off)
    K, M = sphere_cameras(V, H, W)
    e_check = int(np.searchsorted(off, a.check_samples, side="right")) - 1   # whole edges
    pc = int(off[e_check])
    want = OR.oriented_tally(pts[:pc], OR.sample_partners(off[:e_check + 1]), K[:hv], M[:hv], near[:hv].cpu(), backend="host")
    got = OR.oriented_tally(pts[:pc], partner[:pc], K[:hv], M[:hv], near[:hv])
    assert torch.equal(got.cpu(), want), "cgs_sample_support_oriented disagrees with the host back end"
    pts_d, par_d = torch.from_numpy(pts).to(dev), torch.from_numpy(partner).to(dev)
    Kd, Md = ES.cameras_on(dev, K, np.ascontiguousarray(M.reshape(V, 12)))
    tol_d = torch.tensor([tol2], dtype=torch.int32).to(dev)
    tally = torch.zeros((P, 2), dtype=torch.int32, device=dev)
    calls = {
        "sample_support_oriented": lambda: L.check(lib.cgs_sample_support_oriented(
            P, L.ptr(pts_d), L.ptr(par_d), V, L.ptr(Kd), L.ptr(Md), H, W, L.ptr(near), OR.SPREAD, L.ptr(tally), stream),
            "cgs_sample_support_oriented"),
        "sample_support": lambda: L.check(lib.cgs_sample_support(P, L.ptr(pts_d), V, L.ptr(Kd), L.ptr(Md), H, W, L.ptr(d2), 1,
                                                                 L.ptr(tol_d), L.ptr(tally), stream), "cgs_sample_support")}
    sums = {}
    for name, call in calls.items():   # the warm-up, from a zeroed tally
        tally.zero_()
        call()
        torch.cuda.synchronize()
        sums[name] = [int(x) for x in tally.sum(0).tolist()]
    assert sums["sample_support"][0] == sums["sample_support_oriented"][0] and \
        sums["sample_support_oriented"][1] <= sums["sample_support"][1], sums
    wide = torch.zeros((P, 2), dtype=torch.int32, device=dev)
    L.check(lib.cgs_sample_support_oriented(P, L.ptr(pts_d), L.ptr(par_d), V, L.ptr(Kd), L.ptr(Md), H, W, L.ptr(near), 4,
                                            L.ptr(wide), stream), "cgs_sample_support_oriented")
    assert torch.equal(wide, tally), "with every orientation accepted the tally is cgs_sample_support's"
    print(f"{P} samples x {V} views: equal to the host back end on {pc} samples x {hv} views; {sums['sample_support'][0]} seen "
          f"sample-views, {sums['sample_support'][1]} near, {sums['sample_support_oriented'][1]} near and agreeing", flush=True)
    ms = {name: [] for name in calls}
    for _ in range(3):
        for name, call in calls.items():
            ms[name].append(events_ms(torch, call, a.reps))
    seen = sums["sample_support"][0]
    for name, t in ms.items():
        print(f"  {name}: {[round(x, 3) for x in t]} ms per call over {a.reps} calls each; {P * V / min(t) / 1e6:.1f} G "
              f"sample-views per second; {seen} gathers of one {'byte' if 'oriented' in name else 'word'}", flush=True)
    result["tally"] = {"points": P, "seen": seen, "sums": sums, "ms": ms}
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
