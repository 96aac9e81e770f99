"""The depth gate of the TRAINING render: one resident stack of depth planes, one per training camera, that the fused view
forward holds every splat's centre against (``cgs_view_forward_depth`` / ``cgs_view_forward_render_depth``, the rule in
include/curvegs.h: a splat whose centre the view's plane hides gets radius 0 and is treated like a frustum-culled one).

``TrainGate`` is built once from the training cameras and ONE depth source -- ``occluder=`` (triangles, a ``Surfels`` or the
path of a mesh / cloud file) or ``depth_maps=`` (one array of camera z per camera) -- through the chain's own operators:
``ChunkDepth`` draws the planes (``mesh_depth`` / ``surfel_depth`` / the caller's maps, then the window maximum) chunk by
chunk and the chunks are copied into one float32 [V,H,W] stack.  Unlike the scan-level operators, which rebuild a chunk's
planes per call, training visits a random view every iteration, so all V planes stay resident: ``planes_bytes`` says what
that costs, and a stack beyond ``max_bytes`` is refused.

OFF BY DEFAULT, UNTUNED: ``depth_slack`` defaults to the chain's ``DEPTH_SLACK``.  The gate is piecewise constant: it has no
derivative of its own, a hidden splat simply receives no gradient from that view."""
import ctypes as C

import numpy as np
import torch

from .. import _lib as L
from . import edge_occlusion as EO
from . import edge_score as ES
from .view_chunks import camera_arrays, view_chunks

PLANES_BUDGET = 1 << 30          # bytes of resident planes a TrainGate accepts by default (24 views of 1600 x 1600 are 246 MB)
CHUNK_BUDGET = 256 << 20         # working set of one ChunkDepth chunk while the stack is built


def gate_cameras(cameras):
    """NovelViewCamera s of the cameras a gate is built for: NovelViewCamera s as they are; the cameras a Scene trains on
    (``R``, ``T``, ``original_image``) through ``reprojection.scene_cameras``; anything else that the renderer takes
    (``world_view_transform`` = the transposed world-to-view matrix, ``FoVx``, ``FoVy``: ``synthetic.SynthCamera``) with the
    focal lengths of the field of view at the image's size and the principal point at its centre, like ``scene_cameras``."""
    from ..edge_extraction.novel_view import NovelViewCamera
    from ..scene.dataset_io import fov2focal
    cameras = list(cameras)
    if all(isinstance(c, NovelViewCamera) for c in cameras):
        return cameras
    if all(hasattr(c, "R") and hasattr(c, "T") and hasattr(c, "original_image") for c in cameras):
        from ..edge_extraction.reprojection import scene_cameras
        return scene_cameras(cameras)[0]
    out = []
    for i, c in enumerate(cameras):
        H, W = int(c.image_height), int(c.image_width)
        w2c = c.world_view_transform.detach().cpu().double().numpy().T
        out.append(NovelViewCamera(str(getattr(c, "image_name", i)), np.ascontiguousarray(w2c[:3, :3]), w2c[:3, 3].copy(),
                                   float(fov2focal(c.FoVx, W)), float(fov2focal(c.FoVy, H)), W / 2.0, H / 2.0, W, H))
    return out


class TrainGate:
    """The resident gate of a training run.

      V, height, width   the stack's shape; every camera must have the same image size (ValueError otherwise)
      planes             float32 [V,H,W]: camera z after the window maximum, +inf where there is no surface -- a tensor on
                         ``device`` for ``backend="gpu"``, a CPU tensor for ``backend="host"`` (``to(device)`` uploads it)
      intr, w2c          float64 [V,4] and [V,12] on the planes' device: the cameras the planes were drawn with
      slack, window      the checked settings; ``near`` the near plane or None
      planes_bytes       4 V H W
      settings()         what a result records: ChunkDepth's keys and "planes_bytes"
    """

    def __init__(self, cameras, occluder=None, depth_maps=None, depth_slack=EO.DEPTH_SLACK, depth_window=EO.DEPTH_WINDOW,
                 near_clip=None, backend="gpu", device=None, max_bytes=PLANES_BUDGET):
        ES._check_backend(backend)
        if (occluder is None) == (depth_maps is None):
            raise ValueError("TrainGate: give exactly one depth source, occluder= or depth_maps=")
        cams = gate_cameras(cameras)
        if not cams:
            raise ValueError("TrainGate: no cameras")
        sizes = sorted({(int(c.height), int(c.width)) for c in cams})
        if len(sizes) != 1:
            raise ValueError(f"TrainGate: the cameras have mixed image sizes {sizes} (height, width); the gate keeps one "
                             "[V,H,W] stack of planes")
        self.V, (self.height, self.width) = len(cams), sizes[0]
        self.planes_bytes = 4 * self.V * self.height * self.width
        if self.planes_bytes > int(max_bytes):
            raise ValueError(f"TrainGate: {self.V} planes of {self.width}x{self.height} need {self.planes_bytes} bytes, over "
                             f"the budget of {int(max_bytes)} (max_bytes)")
        src = EO.ChunkDepth("TrainGate", cams, occluder=occluder, depth_maps=depth_maps, depth_slack=depth_slack,
                            depth_window=depth_window, near_clip=near_clip)
        self.slack, self.window, self.near = src.slack, src.window, src.near
        self._settings = src.settings()
        dev = None
        if backend == "gpu":
            dev = ES._device_for([], "TrainGate", device)
        src.to(backend, dev)
        stack = torch.empty((self.V, self.height, self.width), dtype=torch.float32, device=dev if dev is not None else "cpu")
        for H, W, sel, intr, w2c in view_chunks(cams, src.bytes_per_pixel, CHUNK_BUDGET):
            p = src.planes(H, W, sel, intr, w2c)
            p = p if torch.is_tensor(p) else torch.from_numpy(np.ascontiguousarray(p))
            stack[torch.as_tensor(sel, device=stack.device)] = p.to(stack.device)
        self.planes = stack
        K, M = camera_arrays(cams)
        self.intr = torch.from_numpy(np.ascontiguousarray(K)).to(stack.device)
        self.w2c = torch.from_numpy(np.ascontiguousarray(M.reshape(self.V, 12))).to(stack.device)
        self.cameras = cams

    @property
    def device(self):
        return self.planes.device

    def to(self, device):
        """The same gate with its planes and cameras on ``device`` (a gate built on the host, uploaded once)."""
        self.planes, self.intr, self.w2c = (t.to(device) for t in (self.planes, self.intr, self.w2c))
        return self

    def settings(self):
        return dict(self._settings, planes_bytes=self.planes_bytes)

    def check(self, H, W, dev):
        """ValueError unless the gate serves a render of H x W pixels on ``dev``."""
        if (int(H), int(W)) != (self.height, self.width):
            raise ValueError(f"depth_gate: the planes are {self.width}x{self.height}, the view is {int(W)}x{int(H)}")
        dev, mine = torch.device(dev), self.planes.device
        if mine.type != "cuda" or dev.type != "cuda" or (dev.index is not None and mine.index != dev.index):
            raise ValueError(f"depth_gate: the planes are on {self.planes.device}, the model on {dev} (TrainGate.to)")

    def view_args(self, view):
        """(host view number, device int32 view index or None) of a ``depth_gate=(gate, view)`` argument: an int is checked
        against [0, V) here; a one-element int32 tensor on the planes' device is read by the kernel (a captured graph picks
        the step's plane that way)."""
        if torch.is_tensor(view):
            if view.dtype != torch.int32 or view.numel() != 1 or view.device != self.planes.device:
                raise ValueError("depth_gate: a device view index is a one-element int32 tensor on the planes' device")
            return 0, view
        v = int(view)
        if not 0 <= v < self.V:
            raise ValueError(f"depth_gate: view {v} is outside [0, {self.V})")
        return v, None

    def struct(self, view):
        """``cgs_view_gate`` of this gate for one view (the tensors it points into must outlive the call)."""
        v, idx = self.view_args(view)
        return L.ViewGate(self.planes.data_ptr(), self.intr.data_ptr(), self.w2c.data_ptr(),
                          idx.data_ptr() if idx is not None else None, float(self.slack), self.V, v, self.height, self.width)

    def tensors(self, view):
        """(planes, intr, w2c, slack, host view, device view index or None): the compiled shim's form of ``struct``."""
        v, idx = self.view_args(view)
        return self.planes, self.intr, self.w2c, float(self.slack), v, idx


def splat_visibility(points, gate):
    """Per splat centre, over the gate's views: (seen, hidden, dead) -- int32 [P] the views whose image the centre falls into,
    int32 [P] those of them whose plane hides it, bool [P] the centres hidden in EVERY view that sees them (at least one):
    no gradient of a gated run can reach such a splat.  No new kernel: ``point_masks_depth`` tallies per VIEW, so the
    per-splat tally is taken per view from ``gate_view_host``, the host statement of the same rule that operator is tested
    against (a report written once, at the end of training)."""
    pts = np.ascontiguousarray(ES._host(points), np.float32).reshape(-1, 3)
    planes, K, M = ES._host(gate.planes), ES._host(gate.intr), ES._host(gate.w2c)
    seen = np.zeros((pts.shape[0],), np.int32)
    hidden = np.zeros((pts.shape[0],), np.int32)
    for v in range(gate.V):
        _u, _v, vis, hid = EO.gate_view_host(pts, K[v], M[v], planes[v], gate.slack)
        seen += (vis | hid)
        hidden += hid
    return seen, hidden, (seen > 0) & (hidden == seen)
