"""python -m curve_gaussian_amd.tsdf_mesh --scan DIR --depth_dir NAME [--detector PidiNet] [--grid N] [--bounds ...]
                                          [--trunc T] [--min_weight K] [--out FILE] [--backend gpu|host] [--overwrite]

A mesh occluder from a scan's depth maps (``ops.tsdf``: a truncated signed distance field over a voxel lattice, its zero
surface by marching tetrahedra).  For a scan whose only depth source is per-view maps -- ``stereo_depth``'s, fused or
not, or a sensor's -- and whose user wants what only a mesh gives: ``--ignore_contours`` and ``--near_clip`` are rejected
with ``--depth_dir``, and every view of the maps is a separate estimate while the mesh is one surface.  The chain:

    python -m curve_gaussian_amd.edge_detect --scan SCAN
    python -m curve_gaussian_amd.stereo_depth --scan SCAN --fuse
    python -m curve_gaussian_amd.tsdf_mesh --scan SCAN --depth_dir depth_stereo_fused
    ... --occluder SCAN/tsdf_mesh.ply --depth_slack <recommended_slack of SCAN/tsdf_mesh.json> [--ignore_contours] [--near_clip N]

``--depth_dir`` (inside the scan unless absolute) holds one ``<image stem>.npy`` per view as ``--depth_dir`` reads them
elsewhere; an entry that is not a positive finite number says nothing.  The cameras are those that
``edge_extraction.reprojection`` forms for the scan (through its ``--detector`` edge maps: run ``edge_detect`` first), as
``stereo_depth``'s tool takes them.

Output: ``<out>`` (default ``<scan>/tsdf_mesh.ply``), a triangle soup by ``write_triangle_ply`` that ``read_occluder``
classifies as a mesh, and beside it ``<out stem>.json`` with every parameter, ``ops.tsdf.tsdf_mesh``'s ``info`` and
``recommended_slack`` = 2 x the voxel diagonal.  An existing file is left alone without ``--overwrite``.  OFF BY DEFAULT:
no other tool calls this.  EVERY DEFAULT IS UNTUNED (grid 128, trunc 4 x the longest step, min_weight 2, the slack)."""
import argparse
import json
import os
import sys

import numpy as np

from .ops import edge_occlusion as EO
from .ops import tsdf as TS

OUT_FILE = "tsdf_mesh.ply"
SLACK_NOTE = ("the depth gate's default slack (0.001) is far below what the lattice resolves: pass recommended_slack as "
              "--depth_slack with this mesh")


def mesh_scan(scan_dir, depth_dir, detector="PidiNet", out=None, overwrite=False, backend="gpu", grid=TS.GRID, bounds=TS.BOUNDS,
              trunc=None, min_weight=TS.MIN_WEIGHT):
    """Writes the TSDF mesh of the scan's depth maps and its JSON record (see the module's text); returns the two paths."""
    from .edge_extraction import reprojection as RP
    out_file = os.path.join(scan_dir, OUT_FILE) if out is None else out
    record = os.path.splitext(out_file)[0] + ".json"
    if os.path.exists(out_file) and not overwrite:
        raise FileExistsError(f"tsdf_mesh: {out_file} exists and is left untouched; pass --overwrite (overwrite=True) to "
                              "replace it")
    if os.path.exists(os.path.join(scan_dir, "sparse")):
        cams, _ = RP.colmap_scan_cameras(scan_dir, detector)
    else:
        cams, _ = RP.emap_cameras(scan_dir, detector)
    maps = RP.scan_depth_maps(os.path.join(scan_dir, depth_dir), cams)
    tris, info = TS.tsdf_mesh(maps, cams, grid=grid, bounds=bounds, trunc=trunc, min_weight=min_weight, backend=backend)
    os.makedirs(os.path.dirname(os.path.abspath(out_file)), exist_ok=True)
    EO.write_triangle_ply(out_file, tris)
    report = {"method": "tsdf_marching_tetrahedra", "backend": backend, "detector": detector, "depth_dir": depth_dir,
              "grid": (int(grid) if np.ndim(grid) == 0 else [int(g) for g in grid]),
              "bounds": np.asarray(bounds, np.float64).tolist(), "trunc": info["trunc"], "min_weight": info["min_weight"],
              "info": info, "recommended_slack": info["recommended_slack"], "note": SLACK_NOTE}
    with open(record, "w") as f:
        json.dump(report, f, indent=1)
    return out_file, record


def main(argv=None):
    p = argparse.ArgumentParser(prog="python -m curve_gaussian_amd.tsdf_mesh",
                                description="A triangle-mesh occluder from a scan's depth maps (TSDF + marching tetrahedra), "
                                            "in the format --occluder reads.  Every default is untuned.")
    p.add_argument("--scan", required=True, help="the scan: a COLMAP folder (sparse/0 + images) or an EMAP one (meta_data.json + color)")
    p.add_argument("--depth_dir", required=True, help="the folder of <image stem>.npy depth maps (inside the scan unless absolute)")
    p.add_argument("--detector", default="PidiNet", help="the edge maps through which the scan's cameras are read")
    p.add_argument("--grid", type=int, default=TS.GRID, help="lattice points along the longest side of the bounds (untuned)")
    p.add_argument("--bounds", type=float, nargs=6, default=None, metavar=("X0", "Y0", "Z0", "X1", "Y1", "Z1"),
                   help="the box the lattice fills (default: the unit cube)")
    p.add_argument("--trunc", type=float, default=None, help="the truncation distance, world units (default: 4 x the longest step; untuned)")
    p.add_argument("--min_weight", type=int, default=TS.MIN_WEIGHT, help="the observing views every corner of a cell needs (untuned)")
    p.add_argument("--out", default=None, help=f"the file to write (default: <scan>/{OUT_FILE})")
    p.add_argument("--backend", choices=("gpu", "host"), default="gpu")
    p.add_argument("--overwrite", action="store_true", help="replace an existing output file")
    a = p.parse_args(argv)
    bounds = TS.BOUNDS if a.bounds is None else (tuple(a.bounds[:3]), tuple(a.bounds[3:]))
    out_file, record = mesh_scan(a.scan, a.depth_dir, detector=a.detector, out=a.out, overwrite=a.overwrite, backend=a.backend,
                                 grid=a.grid, bounds=bounds, trunc=a.trunc, min_weight=a.min_weight)
    print(f"tsdf_mesh: wrote {out_file} and {record}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
