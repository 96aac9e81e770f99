"""ctypes front-end of oracle/_ref/libref_raster.so: the REFERENCE rasterizer's own kernels (cuda_rasterizer/*.cu built for
gfx950 against our shims by oracle/ref_raster/Makefile) behind the C ABI of oracle/ref_raster/ref_raster_api.cpp.

The functions take CUDA tensors and return tensors shaped like the reference binding's (rasterize_points.cu):
``forward`` -> color [1,H,W], radii [P], invdepth [1,H,W], out_all_map [4,H,W] plus the saved state; ``backward`` -> the nine
gradients (dL_dsh [P,M,3]) plus dL_dconic [P,2,2] and dL_dinvdepths ([P,1] with an upstream inverse-depth gradient, else
[0,1]); ``mark_visible`` -> bool [P].  Argument order and meaning follow ``oracle.raster.forward`` / ``backward``.

Test infrastructure only.  A missing library is an error, never a skip: a silently skipped pin is no pin.
"""
import ctypes as C
import os

import numpy as np
import torch  # before the library: torch's bundled HIP runtime must be the only one in the process

from . import GLM_CHECK_SO, REF_RASTER_SO

_LIB = None
_vp, _i, _f = C.c_void_p, C.c_int, C.c_float


def lib() -> C.CDLL:
    global _LIB
    if _LIB is not None:
        return _LIB
    so = os.environ.get("REF_RASTER_LIB", REF_RASTER_SO)   # REF_RASTER_LIB: an experiment build of the same recipe
    if not os.path.exists(so):
        raise FileNotFoundError(
            f"{so} is missing: the reference rasterizer is built by oracle.build() where the reference checkout "
            "and hipcc are present (REF_RASTER_SRC names the checkout's cuda_rasterizer/ directory)")
    L = C.CDLL(so)
    L.ref_last_error.restype = C.c_char_p
    L.ref_forward.restype = _i
    L.ref_forward.argtypes = [C.POINTER(_vp), _i, _i, _i, _vp, _i, _i, _vp, _vp, _vp, _vp, _vp, _f, _vp, _vp, _vp, _vp, _vp,
                              _vp, _f, _f, _i, _vp, _vp, _vp, _i, _i, _vp]
    L.ref_backward.restype = _i
    L.ref_backward.argtypes = [_vp, _i, _i] + [_vp] * 8 + [_f] + [_vp] * 5 + [_f, _f] + [_vp] * 15 + [_i, _i]
    L.ref_mark_visible.restype = _i
    L.ref_mark_visible.argtypes = [_i, _vp, _vp, _vp, _vp]
    L.ref_num_rendered.restype = _i
    L.ref_num_rendered.argtypes = [_vp]
    L.ref_copy_state.restype = _i
    L.ref_copy_state.argtypes = [_vp, C.c_char_p, _vp]
    L.ref_free.restype = None
    L.ref_free.argtypes = [_vp]
    _LIB = L
    return L


def glm_check_lib() -> C.CDLL:
    """oracle/_ref/libglm_check.so: the GLM shim's operators on caller-given arrays (host only, no reference source)."""
    if not os.path.exists(GLM_CHECK_SO):
        raise FileNotFoundError(f"{GLM_CHECK_SO} is missing: oracle.build() builds it wherever hipcc is")
    return C.CDLL(GLM_CHECK_SO)


def _check(rc, what):
    if rc != 0:
        raise RuntimeError(f"reference {what}: {lib().ref_last_error().decode()}")


def _dev(t):
    """None or an empty tensor -> no pointer (the binding's torch::Tensor([]).data<float>()); else contiguous float32 CUDA."""
    if t is None or t.numel() == 0:
        return None
    t = t.detach()
    assert t.is_cuda, "the reference rasterizer takes CUDA tensors"
    return t.to(torch.float32).contiguous()


def _ptr(t):
    return None if t is None else t.data_ptr()


class RefForward:
    """Outputs and saved state of one reference forward; ``free()`` (or __del__) releases the reference's buffers."""

    def __init__(self, ctx, P, H, W, color, radii, invdepth, out_all_map, inputs):
        self._ctx = ctx
        self.P, self.H, self.W = P, H, W
        self.color, self.radii, self.invdepth, self.out_all_map = color, radii, invdepth, out_all_map
        self.inputs = inputs
        self.num_rendered = int(lib().ref_num_rendered(ctx))

    def _state(self, which, n, dtype):
        out = np.zeros(n, dtype)
        if n:
            _check(lib().ref_copy_state(self._ctx, which.encode(), out.ctypes.data), "state " + which)
        return out

    @property
    def tiles(self):
        return ((self.W + 15) // 16) * ((self.H + 15) // 16)

    @property
    def ranges(self): return self._state("ranges", 2 * self.tiles if self.P else 0, np.uint32).reshape(-1, 2)
    @property
    def point_list(self): return self._state("point_list", self.num_rendered, np.uint32)
    @property
    def point_keys(self): return self._state("point_keys", self.num_rendered, np.uint64)
    @property
    def n_contrib(self): return self._state("n_contrib", self.H * self.W if self.P else 0, np.uint32).reshape(-1, self.W)
    @property
    def final_T(self): return self._state("final_T", self.H * self.W if self.P else 0, np.float32).reshape(-1, self.W)
    @property
    def means2D(self): return self._state("means2D", 2 * self.P, np.float32).reshape(-1, 2)
    @property
    def depths(self): return self._state("depths", self.P, np.float32)
    @property
    def conic_opacity(self): return self._state("conic_opacity", 4 * self.P, np.float32).reshape(-1, 4)
    @property
    def tiles_touched(self): return self._state("tiles_touched", self.P, np.uint32)

    def free(self):
        if self._ctx:
            lib().ref_free(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def forward(bg, means3D, colors_precomp, opacities, scales, rotations, scale_modifier, cov3D_precomp, all_map,
            viewmatrix, projmatrix, tan_fovx, tan_fovy, H, W, sh, degree, campos, prefiltered=False,
            antialiasing=False, render_geo=True) -> RefForward:
    L = lib()
    m = _dev(means3D)
    dev = m.device if m is not None else torch.device("cuda")
    P = 0 if m is None else m.shape[0]
    sh_d = _dev(sh)
    M = 0 if sh_d is None else sh_d.shape[1]
    a = dict(bg=_dev(bg), means3D=m, sh=sh_d, colors=_dev(colors_precomp), opac=_dev(opacities), scales=_dev(scales),
             rots=_dev(rotations), cov3D=_dev(cov3D_precomp), all_map=_dev(all_map), view=_dev(viewmatrix),
             proj=_dev(projmatrix), campos=_dev(campos), scale_modifier=float(scale_modifier), tan_fovx=float(tan_fovx),
             tan_fovy=float(tan_fovy), degree=int(degree), M=M, antialiasing=bool(antialiasing), render_geo=bool(render_geo))
    color = torch.zeros(1, H, W, device=dev)
    invd = torch.zeros(1, H, W, device=dev)
    amap = torch.zeros(4, H, W, device=dev)
    radii = torch.zeros(P, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    ctx = _vp()
    rc = L.ref_forward(C.byref(ctx), P, int(degree), M, _ptr(a["bg"]), W, H, _ptr(m), _ptr(sh_d), _ptr(a["colors"]),
                       _ptr(a["opac"]), _ptr(a["scales"]), a["scale_modifier"], _ptr(a["rots"]), _ptr(a["cov3D"]),
                       _ptr(a["all_map"]), _ptr(a["view"]), _ptr(a["proj"]), _ptr(a["campos"]), a["tan_fovx"], a["tan_fovy"],
                       int(prefiltered), color.data_ptr(), invd.data_ptr(), amap.data_ptr(), int(antialiasing),
                       int(render_geo), _ptr(radii) if P else None)
    if rc != 0:
        if ctx.value:
            L.ref_free(ctx)
        _check(rc, "forward")
    return RefForward(ctx.value, P, H, W, color, radii, invd, amap, a)


def backward(fw: RefForward, dL_dcolor, dL_dinvdepth, dL_dall_map):
    """dL_dinvdepth None -> no inverse-depth gradient (the binding's empty tensor); dL_dcolor / dL_dall_map None -> zeros
    (autograd materialises them)."""
    L = lib()
    a = fw.inputs
    P, M, H, W = fw.P, a["M"], fw.H, fw.W
    dev = fw.color.device
    z = lambda *s: torch.zeros(*s, device=dev)
    g = dict(dL_dmeans2D=z(P, 3), dL_dcolors=z(P, 1), dL_dopacity=z(P, 1), dL_dmeans3D=z(P, 3), dL_dcov3D=z(P, 6),
             dL_dsh=z(P, M, 3), dL_dscales=z(P, 3), dL_drotations=z(P, 4), dL_dall_map=z(P, 4), dL_dconic=z(P, 2, 2))
    dcol = _dev(dL_dcolor.to(dev)) if dL_dcolor is not None else z(1, H, W)
    damap = _dev(dL_dall_map.to(dev)) if dL_dall_map is not None else z(4, H, W)
    dinv = _dev(dL_dinvdepth.to(dev)) if dL_dinvdepth is not None else None
    g["dL_dinvdepths"] = z(P, 1) if dinv is not None else z(0, 1)
    torch.cuda.synchronize(dev)
    p = lambda k: g[k].data_ptr() if g[k].numel() else None
    rc = L.ref_backward(fw._ctx, a["degree"], M, _ptr(a["bg"]), _ptr(fw.out_all_map), _ptr(a["means3D"]), _ptr(a["sh"]),
                        _ptr(a["colors"]), _ptr(a["all_map"]), _ptr(a["opac"]), _ptr(a["scales"]), a["scale_modifier"],
                        _ptr(a["rots"]), _ptr(a["cov3D"]), _ptr(a["view"]), _ptr(a["proj"]), _ptr(a["campos"]),
                        a["tan_fovx"], a["tan_fovy"], _ptr(fw.radii) if P else None, _ptr(dcol), _ptr(dinv), _ptr(damap),
                        p("dL_dmeans2D"), p("dL_dconic"), p("dL_dopacity"), p("dL_dcolors"), p("dL_dinvdepths"),
                        p("dL_dmeans3D"), p("dL_dcov3D"), p("dL_dsh"), p("dL_dscales"), p("dL_drotations"), p("dL_dall_map"),
                        int(a["antialiasing"]), int(a["render_geo"]))
    _check(rc, "backward")
    return g


def mark_visible(means3D, viewmatrix, projmatrix):
    L = lib()
    m = _dev(means3D)
    P = 0 if m is None else m.shape[0]
    present = torch.zeros(P, dtype=torch.bool, device=m.device if m is not None else "cuda")
    if P:
        v, pr = _dev(viewmatrix), _dev(projmatrix)
        torch.cuda.synchronize(m.device)
        _check(L.ref_mark_visible(P, _ptr(m), _ptr(v), _ptr(pr), present.data_ptr()), "markVisible")
    return present
