"""python profiles/probes/edge_join.py [--edges 4000] [--samples 100] [--resolution 0.001] [--check_samples 100000]
                                        [--reps 50] [--out FILE]

Times ``cgs_end_attach`` (profiles/edge_join.md) on the input of the dedupe probe (profiles/probes/edge_dedupe.py):
``--edges`` straight edges of ``--samples`` +- 20 % samples each, ``--resolution`` apart, scattered in the unit box, every
fourth edge a duplicate one resolution beside its predecessor; tolerance 2 x and reach 8 x the resolution, the defaults of
``join_edges``.  Before anything is timed the keys of the first ``--check_samples`` samples (whole edges) are compared with
the host back end, and the host's time for that subset is printed beside the kernel's for the whole set."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from edge_dedupe import straight_edges  # noqa: E402  (the sibling probes)
from edge_support import events_ms  # noqa: E402


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--edges", type=int, default=4000)
    p.add_argument("--samples", type=int, default=100)
    p.add_argument("--resolution", type=float, default=0.001)
    p.add_argument("--check_samples", type=int, default=100000)
    p.add_argument("--reps", type=int, default=50)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    import torch
    from curve_gaussian_amd import _lib as L
    from curve_gaussian_amd.ops import edge_join as EJ
    if not torch.cuda.is_available():
        raise SystemExit("edge_join: needs a GPU; nothing is measured without one")
    dev = torch.device("cuda", 0)
    tolerance, reach = EJ.TOLERANCE_RESOLUTIONS * a.resolution, EJ.REACH_RESOLUTIONS * a.resolution
    pts, off = straight_edges(a.edges, a.samples, a.resolution)
    P, E = len(pts), len(off) - 1
    e_check = int(np.searchsorted(off, a.check_samples, side="right")) - 1   # whole edges
    p_check = int(off[e_check])
    result = {"edges": E, "points": P, "resolution": a.resolution, "tolerance": tolerance, "reach": reach,
              "check_edges": e_check, "check_points": p_check, "device": torch.cuda.get_device_name(dev)}
    print(f"{E} edges, {P} samples, tolerance {tolerance:g}, reach {reach:g}; the check: the first {e_check} edges, "
          f"{p_check} samples", flush=True)

    # 1. equality first
    t0 = time.perf_counter()
    want = EJ.end_attach(pts[:p_check], off[:e_check + 1], tolerance, reach, backend="host")
    t_host = time.perf_counter() - t0
    got = EJ.end_attach(pts[:p_check], off[:e_check + 1], tolerance, reach, backend="gpu", device=dev)
    assert torch.equal(got.cpu(), want), "cgs_end_attach disagrees with the host back end"
    attached = int((want != EJ.NO_ATTACH).sum())
    print(f"equal to the host back end on {2 * e_check} ends x {p_check} samples ({attached} attached); backend=host: "
          f"{t_host:.2f} s", flush=True)
    result.update(host_seconds_check=t_host, attached_check=attached)

    # 2. the time: raw calls between device events after a warm-up, everything resident
    lib, stream = L.load(), L.raw_stream(dev)
    pts_d, off_d = torch.from_numpy(pts).to(dev), torch.from_numpy(off).to(dev)
    work = torch.empty(int(lib.cgs_end_attach_workspace_bytes(P, E)), dtype=torch.uint8, device=dev)
    keys = torch.empty(2 * E, dtype=torch.int64, device=dev)
    tol2 = float(np.float32(tolerance) * np.float32(tolerance))
    reach2 = float(np.float32(reach) * np.float32(reach))
    call = lambda: L.check(lib.cgs_end_attach(P, L.ptr(pts_d), E, L.ptr(off_d), tol2, reach2, L.ptr(keys), L.ptr(work), stream),
                           "cgs_end_attach")
    call()   # the warm-up
    torch.cuda.synchronize()
    result["attached"] = int((keys != EJ.NO_ATTACH).sum())
    ms = [events_ms(torch, call, a.reps) for _ in range(3)]
    print(f"cgs_end_attach: {[round(v, 3) for v in ms]} ms per call over {a.reps} calls each; {result['attached']} of {2 * E} "
          f"ends attached; {2 * E * P / min(ms) / 1e6:.1f} G pairs per second", flush=True)
    result["ms"] = ms
    lib.cgs_prof_reset()
    lib.cgs_prof_enable(1)
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
