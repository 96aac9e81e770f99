"""Seed points of a scan from its edge maps, without training: the multi-view voxel vote of ``ops.edge_seed`` as a tool.

    python -m curve_gaussian_amd.edge_seed_cli --scan DIR [--layout emap|colmap] [--backend gpu|host] [--directions]
                                               [--exclusive] [--occluder FILE | --depth_dir DIR] [--depth_slack S]
                                               [--depth_window R] [--near_clip [VALUE]] --out seeds.ply

The cameras and maps are those ``edge_extraction.reprojection`` scores against: ``emap_cameras`` (meta_data.json) or
``read_colmap`` (sparse/0; ``--undistort`` as there).  The box is ``--bounds``, or ``scene.default_seed_bounds``.  The seeds
are written as the ASCII PLY of ``edge_points.ply``; the counts are printed.  ``--directions`` also seeds the curves'
directions: they are written as the PLY's normals (zero for an undirected seed) and the directed count is printed.
``--exclusive`` keeps only the voted voxels that win the pixels they claim (``--excl_window``, ``--excl_margin``,
``--excl_win_ratio``), which suppresses the ghosts of a scan with few views; the voxels that remain are printed.
``--occluder`` (a mesh file inside the scan directory) or ``--depth_dir`` (a directory inside it with one
``<image stem>.npy`` depth map per camera), at most one, gate the vote and the claims: a view whose depth plane has a surface
more than ``--depth_slack`` (default: half the voxel diagonal) in front of a voxel's centre does not see the voxel
(``--depth_window``: the window maximum over the planes); the hidden (voxel, view) pairs are printed.  On a scan of a solid
the ungated vote keeps next to nothing at the default ``--min_ratio``.  The defaults are untuned, and without a depth source
there is no occlusion reasoning, with or without ``--exclusive`` (ops/edge_seed.py); the gate's own limits -- no near-plane
clipping unless ``--near_clip`` (with ``--occluder``, for cameras inside the mesh) asks for it, drawn solids only -- are
those of ops/edge_occlusion.py."""
import argparse
import os
import sys

import numpy as np

from .edge_extraction import reprojection as RP
from .ops import edge_seed as SD
from .scene import dataset_io as IO


def parser():
    ap = argparse.ArgumentParser(description="Seed points from a scan's edge maps by a multi-view voxel vote.")
    ap.add_argument("--scan", required=True, help="the scan directory")
    ap.add_argument("--layout", choices=RP.LAYOUTS, default="emap")
    ap.add_argument("--detector", default="DexiNed")
    ap.add_argument("--backend", choices=SD.SEED_BACKENDS, default="gpu")
    ap.add_argument("--undistort", action="store_true", help="colmap layout: resample the edge maps through the lens model")
    ap.add_argument("--out", required=True, help="the PLY file to write")
    ap.add_argument("--bounds", nargs=6, type=float, default=None, metavar=("X0", "Y0", "Z0", "X1", "Y1", "Z1"))
    ap.add_argument("--grid", type=int, default=128)
    ap.add_argument("--tol_px", type=float, default=2.0)
    ap.add_argument("--min_views", type=int, default=3)
    ap.add_argument("--min_ratio", type=float, default=0.8)
    ap.add_argument("--cell", type=int, default=4)
    ap.add_argument("--max_seeds", type=int, default=20000)
    ap.add_argument("--edge_threshold", type=float, default=SD.EDGE_MAX_THRESHOLD)
    ap.add_argument("--directions", action="store_true", help="seed the curves' directions too (the PLY's normals)")
    ap.add_argument("--dir_radius", type=int, default=SD.DIR_RADIUS)
    ap.add_argument("--dir_min_support", type=int, default=SD.DIR_MIN_SUPPORT)
    ap.add_argument("--dir_min_linearity", type=float, default=SD.DIR_MIN_LINEARITY)
    ap.add_argument("--exclusive", action="store_true", help="keep only the voted voxels that win the pixels they claim")
    ap.add_argument("--excl_window", type=int, default=SD.EXCL_WINDOW)
    ap.add_argument("--excl_margin", type=int, default=SD.EXCL_MARGIN)
    ap.add_argument("--excl_win_ratio", type=float, default=SD.EXCL_WIN_RATIO)
    ap.add_argument("--thin", action="store_true", help="thin the detected masks first (a thick detector response; untuned)")
    RP.add_depth_arguments(ap)   # --occluder / --depth_dir, --depth_slack, --depth_window: gate the vote and the claims
    ap.set_defaults(depth_slack=None)   # None: half the voxel diagonal (ops.edge_seed.default_slack), not a sample's slack
    return ap


def seed_options(args):
    """seed_points' keywords of a parsed command line."""
    opts = dict(grid=args.grid, tol_px=args.tol_px, min_views=args.min_views, min_ratio=args.min_ratio, cell=args.cell,
                max_seeds=args.max_seeds, edge_threshold=args.edge_threshold, directions=args.directions,
                dir_radius=args.dir_radius, dir_min_support=args.dir_min_support, dir_min_linearity=args.dir_min_linearity,
                exclusive=args.exclusive, excl_window=args.excl_window, excl_margin=args.excl_margin,
                excl_win_ratio=args.excl_win_ratio)
    if args.thin:
        opts["thin"] = True
    if args.occluder is not None or args.depth_dir is not None:
        opts.update(occluder=args.occluder, depth_dir=args.depth_dir, depth_slack=args.depth_slack,
                    depth_window=args.depth_window)
    if args.near_clip is not None:   # (seed_points rejects it without an occluder)
        opts["near_clip"] = args.near_clip
    return opts


def seed_scan(scan_dir, layout="emap", detector="DexiNed", undistort=False, bounds=None, backend="gpu", occluder=None,
              depth_dir=None, **options):
    """(seeds float64 [N,3], info) of the scan at ``scan_dir``; ``options``: seed_points' keywords.  ``occluder``: the name of
    a mesh file inside the scan directory; ``depth_dir``: the name of a directory inside it with one ``<image stem>.npy``
    depth map per camera (``reprojection.scan_depth_maps``); at most one, with ``depth_slack`` / ``depth_window`` among the
    options."""
    if layout not in RP.LAYOUTS:
        raise ValueError(f"unknown layout {layout!r}: expected one of {RP.LAYOUTS}")
    points = None
    if layout == "emap":
        if undistort:
            raise ValueError("undistort applies to the colmap layout only")
        cams, maps = RP.emap_cameras(scan_dir, detector)
    else:
        from .scene.colmap_io import read_colmap
        train, _, pcd, _ = read_colmap(scan_dir, detector=detector, undistort=undistort, undistort_backend=backend)
        cams, maps = RP.scene_cameras(train)
        points = pcd.points
    if bounds is None:
        bounds = IO.default_seed_bounds(layout, points)
    if occluder is not None and depth_dir is not None:
        raise ValueError("seed_scan: give an occluder or a depth_dir, not both")
    if occluder is not None:
        options["occluder"] = os.path.join(scan_dir, occluder)
    elif depth_dir is not None:
        options["depth_maps"] = RP.scan_depth_maps(os.path.join(scan_dir, depth_dir), cams)
    seeds, info = SD.seed_points(cams, maps, detector, bounds, backend=backend, **options)
    info["bounds"] = [np.asarray(b, np.float64).tolist() for b in bounds]
    return seeds, info


def main(argv=None):
    args = parser().parse_args(argv)
    bounds = (args.bounds[:3], args.bounds[3:]) if args.bounds is not None else None
    seeds, info = seed_scan(args.scan, args.layout, args.detector, args.undistort, bounds, args.backend, **seed_options(args))
    IO.write_points_ply(args.out, seeds, info["directions"] if args.directions else None)
    print(f"views {info['views']}, grid {info['dims'][0]}x{info['dims'][1]}x{info['dims'][2]}, kept voxels "
          f"{info['kept_voxels']}, cells {info['cells']}, seeds {info['seeds']}{' (capped)' if info['capped'] else ''}, "
          f"bounds {info['bounds']}" + (f", after the claims {info['exclusive_voxels']} voxels" if args.exclusive else "")
          + (f", directed {info['directed']}" if args.directions else "") + (", detected masks thinned" if args.thin else "")
          + (f", depth gate hid {info['hidden_pairs']} (voxel, view) pairs at slack {info['depth_slack']:g}"
             if "hidden_pairs" in info else ""))
    print(f"Wrote {args.out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
