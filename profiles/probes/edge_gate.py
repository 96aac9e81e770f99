"""python profiles/probes/edge_gate.py [--views 100] [--width 1600] [--height 1200] [--distinct 10] [--segments 150]
                                        [--edges 4000] [--samples 100] [--capture 3] [--reps 50] [--host_views 2]
                                        [--check_samples 20000] [--parent_lib FILE] [--out FILE]

Times the four depth-gated kernels beside their ungated siblings (profiles/edge_gate.md) -- ``cgs_edge_support``,
``cgs_sample_support``, ``cgs_sample_support_oriented``, ``cgs_sample_snap_terms`` and the ``_depth`` entry of each -- on the
tally workload of profiles/probes/edge_snap.py: the samples of profiles/probes/edge_dedupe.py (400 708 at the defaults) in
``--views`` cameras on a sphere around the unit cube, against the distance transform of three-pixel strokes.  The depth is
the z-buffer of the box of scene/solid_scan.py in the same cameras with the default window, so part of the samples is
hidden.  Everything resident, raw calls between device events after a warm-up, all entries alternating within each of three
rounds.

``--parent_lib``: a ``libcurvegs.so`` built from the commit before the gate.  Its four ungated entries are loaded beside this
build's, asserted to write the same bits, and timed in the same rounds: "the existing kernels did not get slower" is judged
against them.  Without it that comparison is NOT MEASURED and the output says so.

Before anything is timed the gated results of the first ``--check_samples`` samples in the first ``--host_views`` views are
compared with the host back end bit for bit."""
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
from edge_thin import dilate, segment_views  # noqa: E402

UNGATED = ("cgs_edge_support", "cgs_sample_support", "cgs_sample_support_oriented", "cgs_sample_snap_terms")


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
    p.add_argument("--parent_lib", default=None)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    import torch
    from curve_gaussian_amd import _lib as L
    from curve_gaussian_amd.ops import edge_occlusion as EO
    from curve_gaussian_amd.ops import edge_orient as OR
    from curve_gaussian_amd.ops import edge_score as ES
    from curve_gaussian_amd.ops import edge_snap as SN
    from curve_gaussian_amd.ops import edge_support as SP
    from curve_gaussian_amd.ops import edge_trim as ET
    from curve_gaussian_amd.scene.solid_scan import solid_geometry
    if not torch.cuda.is_available():
        raise SystemExit("edge_gate: needs a GPU; nothing is measured without one")
    dev = torch.device("cuda", 0)
    H, W, V = a.height, a.width, a.views
    lib, stream = L.load(), L.raw_stream(dev)
    cap2 = SN.capture_squared(a.capture)
    hv = max(1, min(a.host_views, a.distinct, V))
    thick = dilate(segment_views(min(a.distinct, V), H, W, a.segments), 1)
    masks = torch.from_numpy(np.tile(thick, (-(-V // thick.shape[0]), 1, 1))[:V]).to(dev)
    d2 = ES.edt_squared(masks, backend="gpu", device=dev)
    near = OR.oriented_near(OR.mask_orientation(masks, backend="gpu", device=dev), 1, backend="gpu", device=dev)
    del masks
    pts, off = straight_edges(a.edges, a.samples, 0.001)
    P, E = len(pts), len(off) - 1
    partner = OR.sample_partners(off)
    K, M = sphere_cameras(V, H, W)
    depth = EO.mesh_depth(solid_geometry("box")[0], K, M, H, W, EO.DEPTH_WINDOW, backend="gpu", device=dev)
    slack = EO.DEPTH_SLACK

    # equality with the host back end first
    pc = min(P, a.check_samples)
    oc = off[:int(np.searchsorted(off, pc, "right"))]
    pe = int(oc[-1])
    for backend in ("host", "gpu"):
        g = (lambda t: t[:hv].cpu()) if backend == "host" else (lambda t: t[:hv])
        kw = dict(backend=backend, depth=g(depth), slack=slack)
        hid = [torch.zeros(pc, dtype=torch.int32, device=None if backend == "host" else dev) for _ in range(3)]
        res = [SP.support_counts(pts[:pe], oc, K[:hv], M[:hv], g(d2), (1,), return_hidden=True, **kw),
               ET.sample_tally(pts[:pc], K[:hv], M[:hv], g(d2), (1,), hidden_out=hid[0], **kw),
               OR.oriented_tally(pts[:pc], partner[:pc].clip(max=pc - 1), K[:hv], M[:hv], g(near), 1, hidden_out=hid[1], **kw),
               SN.snap_terms(pts[:pc], K[:hv], M[:hv], g(d2), a.capture, hidden_out=hid[2], **kw)]
        flat = [t.cpu().numpy().tobytes() for r in res for t in (r if isinstance(r, tuple) else (r,))] + \
               [h.cpu().numpy().tobytes() for h in hid]
        if backend == "host":
            want = flat
    assert flat == want, "a gated kernel disagrees with its host back end"

    Kd, Md = ES.cameras_on(dev, K, np.ascontiguousarray(M.reshape(V, 12)))
    pts_d, off_d, partner_d = torch.from_numpy(pts).to(dev), torch.from_numpy(off).to(dev), torch.from_numpy(partner).to(dev)
    tol_d = torch.tensor([1], dtype=torch.int32).to(dev)
    lut_d = torch.from_numpy(SN.distance_table(cap2)).to(dev)
    z = lambda *shape, dtype=torch.int32: torch.zeros(shape, dtype=dtype, device=dev)

    def entries(lib, gated, tag):
        """name -> (call, outputs): the four entries of ``lib`` on buffers of their own."""
        sfx = "_depth" if gated else ""
        gate = (L.ptr(depth), slack) if gated else ()
        counts, tally, ot, terms, views = z(E, V, 2), z(P, 2), z(P, 2), z(P, SN.TERMS, dtype=torch.float64), z(P)
        hidden = [z(E, V), z(P), z(P), z(P)]   # (each returned with its entry's outputs: the pointers stay valid)
        ptr = L.ptr
        hid = [(ptr(h),) if gated else () for h in hidden]
        out = {
            "edge_support": (lambda: getattr(lib, "cgs_edge_support" + sfx)(
                E, P, ptr(pts_d), ptr(off_d), V, ptr(Kd), ptr(Md), H, W, ptr(d2), 1, ptr(tol_d), *gate, ptr(counts), *hid[0],
                stream), (counts, hidden[0])),
            "sample_support": (lambda: getattr(lib, "cgs_sample_support" + sfx)(
                P, ptr(pts_d), V, ptr(Kd), ptr(Md), H, W, ptr(d2), 1, ptr(tol_d), *gate, ptr(tally), *hid[1], stream), (tally, hidden[1])),
            "sample_support_oriented": (lambda: getattr(lib, "cgs_sample_support_oriented" + sfx)(
                P, ptr(pts_d), ptr(partner_d), V, ptr(Kd), ptr(Md), H, W, ptr(near), 1, *gate, ptr(ot), *hid[2], stream), (ot, hidden[2])),
            "sample_snap_terms": (lambda: getattr(lib, "cgs_sample_snap_terms" + sfx)(
                P, ptr(pts_d), V, ptr(Kd), ptr(Md), H, W, ptr(d2), cap2, ptr(lut_d), *gate, ptr(terms), ptr(views), *hid[3],
                stream), (terms, views, hidden[3]))}
        return {f"{name}{sfx} [{tag}]": v for name, v in out.items()}

    table = {**entries(lib, False, "this build"), **entries(lib, True, "this build")}
    if a.parent_lib:
        parent = ctypes.CDLL(os.path.abspath(a.parent_lib))
        for name in UNGATED:
            getattr(parent, name).restype, getattr(parent, name).argtypes = L.SIGNATURES[name]
        table.update(entries(parent, False, "parent"))
    for name, (call, _) in table.items():   # the warm-up, from zeroed outputs
        assert call() == 0, name
    torch.cuda.synchronize()
    bits = {name: [t.cpu().numpy().tobytes() for t in outs] for name, (_, outs) in table.items()}
    seen = int(table["sample_support [this build]"][1][0][:, 0].sum())
    visible = int(table["sample_support_depth [this build]"][1][0][:, 0].sum())
    if a.parent_lib:
        for name in UNGATED:
            k = name[4:]
            assert bits[f"{k} [parent]"] == bits[f"{k} [this build]"], f"{name}: this build and the parent write different bits"
    print(f"{P} samples of {E} edges x {V} views {W}x{H}: gated kernels equal to the host back end on {pc} samples x {hv} views; "
          f"{seen} seen sample-views, {seen - visible} of them hidden ({(seen - visible) / max(seen, 1):.1%}); ungated entries "
          + ("bit-equal to the parent build's" if a.parent_lib else "NOT compared with a parent build (no --parent_lib)"), flush=True)
    ms = {name: [] for name in table}
    for _ in range(3):
        for name, (call, _) in table.items():
            ms[name].append(events_ms(torch, call, a.reps))
    for name, t in ms.items():
        print(f"  {name}: {[round(x, 4) for x in t]} ms per call over {a.reps} calls each", flush=True)
    result = {"views": V, "width": W, "height": H, "points": P, "edges": E, "cap2": cap2, "reps": a.reps, "rounds": 3, "seen": seen,
              "hidden": seen - visible, "parent": bool(a.parent_lib), "ms": ms, "device": torch.cuda.get_device_name(dev)}
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
