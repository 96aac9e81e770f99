"""``python -m curve_gaussian_amd.surfel_cloud IN.ply OUT.ply [--factor F | --radius R]``: a point cloud (a PLY without
faces, such as COLMAP's fused.ply) rewritten with a ``radius`` property, the file ``--occluder`` takes as disks
(ops/edge_occlusion.py, ``read_occluder``).  Normals are kept when the input has ``nx ny nz``.  The radii are derived from
the 3 nearest neighbours (``surfel_radii``, ``--factor``), or the constant ``--radius``; this is where a command-line user
sets them."""
import argparse
import sys

import numpy as np

from .ops import edge_occlusion as EO


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m curve_gaussian_amd.surfel_cloud", description=__doc__.split("\n\n")[0])
    ap.add_argument("input", help="a PLY with a vertex element (x y z, optionally nx ny nz) and no faces")
    ap.add_argument("output", help="the PLY to write: x y z, nx ny nz when the input has them, radius")
    ap.add_argument("--factor", type=float, default=None,
                    help=f"radius = factor * sqrt(mean squared distance to the 3 nearest neighbours), capped at "
                         f"{EO.SURFEL_RADIUS_CAP} median radii (default {EO.SURFEL_RADIUS_FACTOR}; untuned)")
    ap.add_argument("--radius", type=float, default=None, help="one constant radius in world units instead")
    ap.add_argument("--backend", choices=("gpu", "host"), default="gpu", help="where the neighbours are searched")
    args = ap.parse_args(argv)
    if args.factor is not None and args.radius is not None:
        ap.error("give --factor or --radius, not both")
    if args.radius is not None and not (args.radius > 0.0 and np.isfinite(args.radius)):
        ap.error("--radius must be finite and > 0")
    cloud = EO.read_occluder(args.input, derive_radii=False)
    if not isinstance(cloud, EO.Surfels):
        ap.error(f"{args.input} is a mesh (it has faces): it is an occluder as it is")
    if args.radius is not None:
        radii = np.full((len(cloud.points),), args.radius, np.float32)
    else:
        factor = EO.SURFEL_RADIUS_FACTOR if args.factor is None else args.factor
        radii = EO.surfel_radii(cloud.points, factor, backend=args.backend)
    EO.write_surfel_ply(args.output, cloud._replace(radii=radii))
    finite = radii[np.isfinite(radii)]
    print(f"{len(radii)} surfels, {'with' if cloud.normals is not None else 'without'} normals, radii "
          + (f"{float(finite.min()):.6g} .. {float(finite.max()):.6g} (median {float(np.median(finite)):.6g})" if finite.size
             else "none finite") + f" -> {args.output}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
