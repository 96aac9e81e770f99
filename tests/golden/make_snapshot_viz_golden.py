#!/usr/bin/env python
"""Generates tests/golden/snapshot_viz.npz by IMPORTING the reference's scene/gaussian_curve_model.py and running its
GaussianCurveModel.draw_curve (:712-727) and draw_ellipsoids (:634-709) unmodified, on CPU (runs only where the reference
checkout exists; the fixture, numbers only, travels).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_snapshot_viz_golden.py

How it is run:
  1. Imports go through make_model_golden.import_reference (placeholders for the absent packages, poisoned before
     anything is called).  seaborn is make_novel_view_golden's restatement of color_palette('hls', n).
  2. open3d is a RECORDING stand-in.  It records what the reference passes to it: the arrays given to Vector3dVector for
     the point cloud (points, colours) and for every sphere (the scaled vertices), the quaternion given to
     get_rotation_matrix_from_quaternion, the centre given to translate, the colour given to paint_uniform_color, and the
     file names given to write_point_cloud / write_triangle_mesh.  create_sphere returns the PRODUCT's template
     (curve_gaussian_amd.scene.snapshot_viz.sphere_template, a restatement of Open3D's): the scaled vertices pin the
     reference's scaling of that template, not Open3D's own sphere.  rotate / translate / += are restated only so that
     the reference's code runs to its end; their results are not recorded.
  3. The reference places tensors on 'cuda' (torch.linspace(..., device='cuda'), .cuda()); a TorchFunctionMode maps
     them to the CPU for the duration of the run.  The reference's source is not modified.
  4. The model is made with object.__new__ as in make_model_golden; its per-splat tensors come from the reference's own
     prepare_scaling_rot on the CPU.  torch.manual_seed(0) runs right before each draw, so the reference's global
     torch.randperm(n) equals the product's permutation drawn from a generator seeded with 0.

The model: five curves of twelve splats, two of them lines, sh_degree 0, mask logits well away from the 0.01 threshold
(sigmoid = 0.01 at logit -4.595), seven splats masked off, two of them on a line."""
import math
import os
import sys
import tempfile
import types

import numpy as np
import torch

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.append(os.path.dirname(os.path.dirname(HERE)))   # the project (the sphere template)
from make_model_golden import _ARMED, import_reference  # noqa: E402
from make_novel_view_golden import _seaborn  # noqa: E402

from curve_gaussian_amd.scene.snapshot_viz import sphere_template  # noqa: E402

SEED = 20261016
B, M, NUM_SAMPLE, STEP = 5, 12, 200, 7000
REC = {"scaled_vertices": [], "quaternions": [], "centers": [], "colors": [], "files": []}


def _open3d():
    o3d = types.ModuleType("open3d")
    o3d.__path__ = []
    utility, geometry, io = (types.ModuleType(f"open3d.{n}") for n in ("utility", "geometry", "io"))

    class Vector3dVector:
        def __init__(self, a):
            self.raw = np.array(a)                       # as passed (a copy)
            self.data = self.raw.astype(np.float64)

    class PointCloud:
        def __init__(self):
            self.points = self.colors = None

    class TriangleMesh:
        def __init__(self):
            self._v = np.zeros((0, 3))
            self.triangles = np.zeros((0, 3), np.int64)
            self.vertex_colors = np.zeros((0, 3))

        @staticmethod
        def create_sphere(radius=1.0, resolution=20):
            m = TriangleMesh()
            m._v, m.triangles = sphere_template(radius, resolution)
            m.triangles = m.triangles.astype(np.int64)
            return m

        @property
        def vertices(self):
            return self._v

        @vertices.setter
        def vertices(self, vec):
            REC["scaled_vertices"].append(vec.raw)
            self._v = vec.data

        def rotate(self, R, center=(0.0, 0.0, 0.0)):
            c = np.asarray(center, np.float64)
            self._v = (self._v - c) @ np.asarray(R, np.float64).T + c

        def translate(self, t, relative=True):
            REC["centers"].append(np.array(t))
            self._v = self._v + np.asarray(t, np.float64)
            return self

        def paint_uniform_color(self, c):
            REC["colors"].append(np.array(c))
            self.vertex_colors = np.tile(np.asarray(c, np.float64), (self._v.shape[0], 1))
            return self

        def __iadd__(self, o):
            self.triangles = np.concatenate([self.triangles, o.triangles + self._v.shape[0]])
            self._v = np.concatenate([self._v, o._v])
            self.vertex_colors = np.concatenate([self.vertex_colors, o.vertex_colors])
            return self

    def get_rotation_matrix_from_quaternion(q):
        REC["quaternions"].append(np.array(q))
        w, x, y, z = (float(v) for v in q)
        tx, ty, tz = 2 * x, 2 * y, 2 * z
        return np.array([[1 - (ty * y + tz * z), ty * x - tz * w, tz * x + ty * w],
                         [ty * x + tz * w, 1 - (tx * x + tz * z), tz * y - tx * w],
                         [tz * x - ty * w, tz * y + tx * w, 1 - (tx * x + ty * y)]])

    def write_point_cloud(path, pcd, write_ascii=False, **k):
        REC["files"].append(os.path.basename(path))
        REC["cloud"] = (pcd.points.raw, pcd.colors.raw, bool(write_ascii))
        return True

    def write_triangle_mesh(path, mesh, **k):
        REC["files"].append(os.path.basename(path))
        REC["mesh"] = (mesh._v.shape[0], mesh.triangles.shape[0])
        return True

    utility.Vector3dVector = Vector3dVector
    geometry.PointCloud, geometry.TriangleMesh = PointCloud, TriangleMesh
    geometry.get_rotation_matrix_from_quaternion = get_rotation_matrix_from_quaternion
    io.write_point_cloud, io.write_triangle_mesh = write_point_cloud, write_triangle_mesh
    o3d.utility, o3d.geometry, o3d.io = utility, geometry, io
    for m in (o3d, utility, geometry, io):
        sys.modules[m.__name__] = m


class OnCpu(torch.overrides.TorchFunctionMode):
    """'cuda' -> the CPU: Tensor.cuda() returns the tensor, a device='cuda' argument becomes 'cpu'."""

    def __torch_function__(self, func, types, args=(), kwargs=None):
        kwargs = dict(kwargs or {})
        if func is torch.Tensor.cuda:
            return args[0]
        dev = kwargs.get("device")
        if dev is not None and torch.device(dev).type == "cuda":
            kwargs["device"] = "cpu"
        return func(*args, **kwargs)


def main():
    sys.modules["seaborn"] = _seaborn()
    _open3d()
    GCM = import_reference("scene.gaussian_curve_model")
    _ARMED[0] = True
    torch.set_num_threads(1)
    gen = torch.Generator().manual_seed(SEED)

    p0 = torch.rand(B, 1, 3, generator=gen)
    steps = 0.08 * torch.randn(B, 3, 3, generator=gen) + torch.tensor([0.0, 0.05, 0.0])
    cp = torch.cat([p0, p0 + torch.cumsum(steps, dim=1)], dim=1).contiguous()
    width = (math.log(5e-3) + 0.4 * torch.randn(B, 1, generator=gen)).contiguous()
    opacity = (0.405 + torch.randn(B, 1, generator=gen)).contiguous()
    is_bezier = torch.tensor([True, False, True, True, False])
    mask = (0.5 + torch.rand(B, M, 1, generator=gen) * 2.5)          # logits in [0.5, 3]: on
    for b, i in ((0, 0), (0, 7), (1, 3), (2, 11), (3, 5), (3, 6), (4, 0)):
        mask[b, i, 0] = -6.0                                           # sigmoid(-6) = 0.0025: off
    mask = mask.contiguous()

    g = object.__new__(GCM.GaussianCurveModel)
    g.n_gaussians = M
    g.max_sh_degree = 0
    g.active_sh_degree = 0
    g.setup_functions()
    t = torch.linspace(0.5 / M, 1 - 0.5 / M, M)                        # gaussian_curve_model.py:58-60, on the CPU
    g.sample_t = t[:, None, None]
    g._curve_points, g._width, g._opacity, g._mask, g.is_bezier = cp, width, opacity, mask, is_bezier
    g._features_dc = torch.zeros(B, M, 1, 3)
    g._features_rest = torch.zeros(B, M, 0, 3)
    g.xyz_gradient_accum = torch.zeros(B * M, 1)
    g.denom = torch.zeros(B * M, 1)
    out = {}
    with OnCpu(), tempfile.TemporaryDirectory() as tmp, torch.no_grad():
        g.prepare_scaling_rot()
        out.update(xyz=g.get_xyz.numpy().copy(), rotation=g.get_rotation.numpy().copy(),
                   scaling=g.get_scaling.numpy().copy())
        torch.manual_seed(0)
        g.draw_curve(tmp, STEP, num_sample=NUM_SAMPLE)
        torch.manual_seed(0)
        g.draw_ellipsoids(tmp, STEP)

    pts, cols, ascii_ = REC["cloud"]
    assert ascii_
    P = B * M
    assert len(REC["scaled_vertices"]) == len(REC["quaternions"]) == len(REC["centers"]) == len(REC["colors"]) == P
    out.update(curve_points=cp.numpy(), width=width.numpy(), opacity=opacity.numpy(), mask=mask.numpy(),
               is_bezier=is_bezier.numpy(), n_gaussians=np.int64(M), num_sample=np.int64(NUM_SAMPLE),
               step=np.int64(STEP), radius=np.float64(1.2), resolution=np.int64(10),
               curve_sample_points=pts, curve_point_colors=cols, files=np.array(REC["files"]),
               splat_scaled_vertices=np.stack(REC["scaled_vertices"]), splat_quaternion=np.stack(REC["quaternions"]),
               splat_center=np.stack(REC["centers"]), splat_color=np.stack(REC["colors"]),
               mesh_counts=np.array(REC["mesh"], np.int64))
    for k, v in sorted(out.items()):
        print(f"{k:24s} {v.dtype} {v.shape}")
    np.savez_compressed(os.path.join(HERE, "snapshot_viz.npz"), **out)


if __name__ == "__main__":
    main()
