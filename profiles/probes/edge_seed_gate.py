"""python profiles/probes/edge_seed_gate.py [--views 100] [--width 1600] [--height 1200] [--grid 256] [--shape box]
                                             [--reps 20] [--rounds 3] [--check_grid 64] [--host_views 2] [--parent_lib FILE]
                                             [--out FILE]

Times the three depth-gated kernels of the edge vote beside their ungated siblings (profiles/edge_seed_gate.md) --
``cgs_voxel_votes``, ``cgs_ray_claims`` (with its clear), ``cgs_ray_wins`` and the ``_depth`` entry of each -- on a solid scan
of scene/solid_scan.py: ``--views`` cameras of ``--width`` x ``--height`` around ``--shape`` with its hidden lines removed, a
grid of ``--grid`` voxels a side over the unit cube, the planes ``cgs_mesh_depth`` + ``cgs_depth_window_max`` of the solid's own
mesh with the default window and the vote's default slack (half the voxel diagonal).  The listed voxels of the claims are
what the GATED vote keeps at the default selection; both the gated and the ungated claims and wins walk that list.
Everything resident, raw calls between device events after a warm-up, all entries alternating within each round.

``--parent_lib``: a ``libcurvegs.so`` built from the commit before the gate.  Its three ungated entries are loaded beside this
build's, asserted to write the same bits, and timed in the same rounds: "the existing kernels did not get slower" is judged
against them.  Without it that comparison is NOT MEASURED and the output says so.

Before anything is timed the gated vote, claims and wins of a ``--check_grid`` grid on the first ``--host_views`` views are
compared with the host back end bit for bit."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from edge_seed_exclusive import events_ms  # noqa: E402  (the sibling probe's timer)

UNGATED = ("cgs_voxel_votes", "cgs_ray_claims", "cgs_ray_wins")
BOUNDS = ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--views", type=int, default=100)
    p.add_argument("--width", type=int, default=1600)
    p.add_argument("--height", type=int, default=1200)
    p.add_argument("--grid", type=int, default=256)
    p.add_argument("--shape", default="box")
    p.add_argument("--reps", type=int, default=20)
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--check_grid", type=int, default=64)
    p.add_argument("--host_views", type=int, default=2)
    p.add_argument("--parent_lib", default=None)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    import torch
    from curve_gaussian_amd import _lib as L
    from curve_gaussian_amd.ops import edge_occlusion as EO
    from curve_gaussian_amd.ops import edge_score as ES
    from curve_gaussian_amd.ops import edge_seed as SD
    from curve_gaussian_amd.ops.view_chunks import camera_arrays
    from curve_gaussian_amd.scene.solid_scan import solid_scan
    if not torch.cuda.is_available():
        raise SystemExit("edge_seed_gate: needs a GPU; nothing is measured without one")
    dev = torch.device("cuda", 0)
    H, W, V = a.height, a.width, a.views
    on = dict(backend="gpu", device=dev)
    scan = solid_scan(a.shape, V, H, W, **on)
    intr, w2c = camera_arrays(scan.cameras)
    depth = EO.mesh_depth(scan.tris, intr, w2c, H, W, EO.DEPTH_WINDOW, **on)
    per = max(1, SD.BYTE_BUDGET // (SD.BYTES_PER_PIXEL * H * W))
    parts = []
    for b in range(0, V, per):
        det = torch.from_numpy((scan.maps[b:b + per] > 127).astype(np.uint8))
        parts.append(SD.near_bits(ES.edt_squared(det, **on), 2, **on))
    bits = torch.cat(parts)
    del parts

    # equality with the host back end first, on a small grid and a few views
    hv = max(1, min(a.host_views, V))
    cd = SD.grid_dims(BOUNDS, a.check_grid)
    flat = {}
    for backend in ("host", "gpu"):
        g = (lambda t: t[:hv].cpu()) if backend == "host" else (lambda t: t[:hv])
        kw = dict(backend=backend, depth=g(depth))
        votes = SD.voxel_votes(BOUNDS, cd, intr[:hv], w2c[:hv], g(bits), H, W, return_hidden=True, **kw)
        seen, hit = (t.cpu().numpy() for t in votes[:2])
        index = np.nonzero(SD.select_voxels(seen, hit, 1, 0.5))[0].astype(np.int32)
        support = SD.voxel_support(seen, hit, index)
        args = (BOUNDS, cd, index, support, intr[:hv], w2c[:hv], g(bits))
        best = SD.ray_claims(*args, H, W, **kw)
        wins = SD.ray_wins(*args, best, H, W, **kw)
        flat[backend] = [t.cpu().numpy().tobytes() for t in (*votes, best, wins)]
    assert flat["gpu"] == flat["host"], "a gated kernel disagrees with its host back end"
    checked = int(index.size)

    # the timed workload: the full grid, all views, the list the gated vote keeps
    dims = SD.grid_dims(BOUNDS, a.grid)
    n = dims[0] * dims[1] * dims[2]
    slack = SD.default_slack(BOUNDS, dims)
    gated = SD.voxel_votes(BOUNDS, dims, intr, w2c, bits, H, W, depth=depth, slack=slack, return_hidden=True, **on)
    plain = SD.voxel_votes(BOUNDS, dims, intr, w2c, bits, H, W, **on)
    seen, hit, hidden = (t.cpu().numpy() for t in gated)
    seen_pairs, hidden_pairs = int(plain[0].cpu().numpy().astype(np.int64).sum()), int(hidden.astype(np.int64).sum())
    assert np.array_equal(seen.astype(np.int64) + hidden, plain[0].cpu().numpy()), "seen + hidden is not the ungated seen"
    index = np.nonzero(SD.select_voxels(seen, hit, 3, 0.8))[0].astype(np.int32)
    kept_plain = int(SD.select_voxels(*(t.cpu().numpy() for t in plain), 3, 0.8).sum())
    support = SD.voxel_support(seen, hit, index)
    M = int(index.size)
    del gated, plain

    lib, stream = L.load(), L.raw_stream(dev)
    lo, hi = (np.asarray(x, np.float64) for x in BOUNDS)
    lo_c, step_c = (C.c_double * 3)(*lo), (C.c_double * 3)(*((hi - lo) / np.array(dims, np.float64)))
    grid = (dims[0], dims[1], dims[2], C.cast(lo_c, C.c_void_p), C.cast(step_c, C.c_void_p))
    Kd, Md = torch.from_numpy(intr).to(dev), torch.from_numpy(np.ascontiguousarray(w2c.reshape(V, 12))).to(dev)
    idx_d, sup_d = torch.from_numpy(index).to(dev), support.to(dev)
    ptr = L.ptr
    views = (V, ptr(Kd), ptr(Md), H, W, ptr(bits))
    listed = (M, ptr(idx_d), ptr(sup_d))

    def entries(lib, gate, tag):
        """name -> (call, outputs): the three entries of ``lib`` on buffers of their own."""
        sfx = "_depth" if gate else ""
        d = (ptr(depth), slack) if gate else ()
        z16 = lambda m: torch.zeros(m, dtype=torch.uint16, device=dev)
        seen, hit, hid, wins = z16(n), z16(n), z16(n), z16(M)
        best = torch.zeros((V, H, W), dtype=torch.int32, device=dev)
        out = {
            "voxel_votes": (lambda: getattr(lib, "cgs_voxel_votes" + sfx)(
                *grid, *views, *d, 0, ptr(seen), ptr(hit), *((ptr(hid),) if gate else ()), stream), (seen, hit, hid)),
            "ray_claims": (lambda: getattr(lib, "cgs_ray_claims" + sfx)(*grid, *listed, *views, *d, 1, ptr(best), stream), (best,)),
            "ray_wins": (lambda: getattr(lib, "cgs_ray_wins" + sfx)(
                *grid, *listed, *views, ptr(best), *d, SD.EXCL_WINDOW, SD.EXCL_MARGIN, 0, ptr(wins), stream), (wins,))}
        return {f"{name}{sfx} [{tag}]": v for name, v in out.items()}   # (claims before wins: the wins read its best)

    table = {**entries(lib, False, "this build"), **entries(lib, True, "this build")}
    if a.parent_lib:
        parent = C.CDLL(os.path.abspath(a.parent_lib))
        for name in UNGATED:
            getattr(parent, name).restype, getattr(parent, name).argtypes = L.SIGNATURES[name]
        table.update(entries(parent, False, "parent"))
    for name, (call, _) in table.items():   # the warm-up, from zeroed outputs
        assert call() == 0, name
    torch.cuda.synchronize()
    out_bits = {name: [t.cpu().numpy().tobytes() for t in outs] for name, (_, outs) in table.items()}
    if a.parent_lib:
        for name in UNGATED:
            k = name[4:]
            assert out_bits[f"{k} [parent]"] == out_bits[f"{k} [this build]"], f"{name}: this build and the parent write different bits"
    hits = {k: int(table[f"ray_wins{s} [this build]"][1][0].cpu().numpy().astype(np.int64).sum()) for k, s in (("plain", ""), ("gated", "_depth"))}
    print(f"{a.shape}: grid {dims} x {V} views {W}x{H}; gated kernels equal to the host back end on a {cd} grid x {hv} views "
          f"({checked} listed voxels); {seen_pairs} seen pairs, {hidden_pairs} of them hidden ({hidden_pairs / max(seen_pairs, 1):.1%}); "
          f"kept voxels {M} gated, {kept_plain} ungated; wins {hits}; ungated entries "
          + ("bit-equal to the parent build's" if a.parent_lib else "NOT compared with a parent build (no --parent_lib)"), flush=True)
    ms = {name: [] for name in table}
    for _ in range(a.rounds):
        for name, (call, _) in table.items():
            ms[name].append(events_ms(torch, call, a.reps))
    for name, t in ms.items():
        print(f"  {name}: {[round(x, 4) for x in t]} ms per call over {a.reps} calls each", flush=True)
    result = {"shape": a.shape, "views": V, "width": W, "height": H, "dims": list(dims), "reps": a.reps, "rounds": a.rounds,
              "seen_pairs": seen_pairs, "hidden_pairs": hidden_pairs, "listed": M, "kept_ungated": kept_plain, "slack": slack,
              "parent": bool(a.parent_lib), "ms": ms, "device": torch.cuda.get_device_name(dev)}
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
