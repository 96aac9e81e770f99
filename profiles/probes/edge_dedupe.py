"""python profiles/probes/edge_dedupe.py [--edges 4000] [--samples 100] [--resolution 0.001] [--check_samples 20000]
                                          [--reps 5] [--out FILE]

Times ``cgs_sample_cover`` (profiles/edge_dedupe.md) on two layouts of the same edges: ``--edges`` straight edges of
``--samples`` +- 20 % samples each, ``--resolution`` apart, every fourth edge a duplicate one resolution beside its predecessor,

  scattered   in the unit box, the tolerance 2 x the resolution: most tiles of candidates lie out of reach of a tile of
              queries and are culled by their boxes
  packed      the same points shrunk into one box whose diagonal is the tolerance: no box is out of reach, every pair passes
              the distance test, and only the rank cull is left

The same code runs both; the difference between the two inputs is the box cull's worth.  Before anything is timed the cover
of the first ``--check_samples`` samples (whole edges) is compared with the host back end on both layouts, and the host's
time for that subset is printed beside the kernel's for the whole set."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from edge_support import events_ms  # noqa: E402  (the sibling probe)


def straight_edges(E, samples, resolution, seed=0):
    """(points float32 [P,3], offsets int32 [E+1]): E straight edges in the unit box, every fourth a duplicate of its
    predecessor, so that the scattered layout has something to cover."""
    rng = np.random.default_rng(seed)
    n = rng.integers(int(0.8 * samples), int(1.2 * samples) + 1, E)
    d = rng.normal(size=(E, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    start = rng.uniform(0.0, 1.0, (E, 3)) - 0.5 * n[:, None] * resolution * d
    dup = np.flatnonzero(np.arange(E) % 4 == 3)   # every fourth edge runs beside the one before it, one resolution away
    side = np.cross(d[dup - 1], rng.normal(size=(len(dup), 3)))
    d[dup] = d[dup - 1]
    start[dup] = start[dup - 1] + resolution * side / np.linalg.norm(side, axis=1, keepdims=True)
    off = np.zeros(E + 1, np.int64)
    off[1:] = np.cumsum(n)
    k = np.arange(off[-1]) - np.repeat(off[:-1], n)
    pts = np.repeat(start, n, 0) + (k * resolution)[:, None] * np.repeat(d, n, 0)
    return pts.astype(np.float32), off.astype(np.int32)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--edges", type=int, default=4000)
    p.add_argument("--samples", type=int, default=100)
    p.add_argument("--resolution", type=float, default=0.001)
    p.add_argument("--check_samples", type=int, default=20000)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    import torch
    from curve_gaussian_amd import _lib as L
    from curve_gaussian_amd.ops import edge_dedupe as ED
    if not torch.cuda.is_available():
        raise SystemExit("edge_dedupe: needs a GPU; nothing is measured without one")
    dev = torch.device("cuda", 0)
    tolerance, cos_min = ED.TOLERANCE_RESOLUTIONS * a.resolution, ED.COS_MIN
    pts, off = straight_edges(a.edges, a.samples, a.resolution)
    P, E = len(pts), len(off) - 1
    lo = pts.min(0)
    span = float((pts.max(0) - lo).max())
    layouts = {"scattered": pts, "packed": ((pts - lo) * np.float32(tolerance / (np.sqrt(3.0) * span * 1.001))).astype(np.float32)}
    ranks = ED.edge_ranks(off)
    e_check = int(np.searchsorted(off, a.check_samples, side="right")) - 1   # whole edges
    p_check = int(off[e_check])
    result = {"edges": E, "points": P, "resolution": a.resolution, "tolerance": tolerance, "cos_min": cos_min,
              "check_points": p_check, "device": torch.cuda.get_device_name(dev)}
    print(f"{E} edges, {P} samples, tolerance {tolerance:g}; the check: the first {e_check} edges, {p_check} samples", flush=True)

    # 1. equality first
    sub_ranks = ED.edge_ranks(off[:e_check + 1])
    for name, x in layouts.items():
        t0 = time.perf_counter()
        want = ED.sample_cover(x[:p_check], off[:e_check + 1], sub_ranks, tolerance, cos_min, backend="host")
        t_host = time.perf_counter() - t0
        got = ED.sample_cover(x[:p_check], off[:e_check + 1], sub_ranks, tolerance, cos_min, backend="gpu", device=dev)
        assert torch.equal(got.cpu(), want), f"cgs_sample_cover disagrees with the host back end on the {name} layout"
        covered = int((want != ED.NO_COVER).sum())
        print(f"{name}: equal to the host back end on {p_check} samples ({covered} covered); backend=host: {t_host:.2f} s", flush=True)
        result[f"{name}_host_seconds_check"] = t_host
        result[f"{name}_covered_check"] = covered

    # 2. the times: raw calls between device events after a warm-up, everything resident, the layouts alternating
    lib, stream = L.load(), L.raw_stream(dev)
    off_d, rk_d = torch.from_numpy(off).to(dev), torch.from_numpy(ranks).to(dev)
    work = torch.empty(int(lib.cgs_sample_cover_workspace_bytes(P)), dtype=torch.uint8, device=dev)
    cover = torch.empty(P, dtype=torch.int32, device=dev)
    tol2 = float(np.float32(tolerance) * np.float32(tolerance))
    cos2 = float(np.float32(cos_min) * np.float32(cos_min))
    calls, ms = {}, {}
    for name, x in layouts.items():
        x_d = torch.from_numpy(x).to(dev)
        calls[name] = (lambda x_d=x_d: L.check(lib.cgs_sample_cover(P, L.ptr(x_d), E, L.ptr(off_d), L.ptr(rk_d), tol2, cos2,
                                                                    L.ptr(cover), L.ptr(work), stream), "cgs_sample_cover"))
        calls[name]()   # the warm-up
        torch.cuda.synchronize()
        result[f"{name}_covered"] = int((cover != ED.NO_COVER).sum())
        ms[name] = []
    for _ in range(3):
        for name, call in calls.items():
            ms[name].append(events_ms(torch, call, a.reps))
    for name, t in ms.items():
        print(f"cgs_sample_cover, {name}: {[round(v, 3) for v in t]} ms per call over {a.reps} calls each; "
              f"{result[name + '_covered']} of {P} samples covered; {P * P / min(t) / 1e6:.1f} G pairs per second, culled ones "
              "counted", flush=True)
        result[f"{name}_ms"] = t
    lib.cgs_prof_reset()
    lib.cgs_prof_enable(1)
    for call in calls.values():
        call()
        torch.cuda.synchronize()
        for kname, (kms, k) in sorted(L.prof_collect().items()):
            print(f"  {kname}: {kms:.3f} ms in {k} launches", flush=True)
        lib.cgs_prof_reset()
    lib.cgs_prof_enable(0)
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
