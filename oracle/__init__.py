"""CPU oracle for the curve-Gaussian hot path.

``oracle/_ref/libref_raster.so`` (``oracle.ref_raster``) is the reference rasterizer itself, built from the reference's
sources by ``oracle/ref_raster/Makefile``.

TEST INFRASTRUCTURE ONLY: only ``tests/``, ``__graft_entry__.smoke()`` and ``bench.py``'s
``cpu_baseline`` leg may import this package.  The product (``curve_gaussian_amd``) never does.
"""
import ctypes
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB = None

# The reference rasterizer built from the reference's own sources (oracle/ref_raster/Makefile) -- see build_ref_raster() --
# and the GLM shim's host-only checks, which need no reference source.
REF_RASTER_SO = os.path.join(_HERE, "_ref", "libref_raster.so")
GLM_CHECK_SO = os.path.join(_HERE, "_ref", "libglm_check.so")
_REF_RASTER_RECIPE = os.path.join(_HERE, "ref_raster")
# where the reference checkout's cuda_rasterizer/ is looked for: REF_RASTER_SRC, else the checkout's location
# (/root/reference, like tests/golden/make_*golden.py), else a checkout named `reference` next to this repository
_REF_RASTER_SUBDIR = os.path.join("submodules", "diff-cur-rasterization", "cuda_rasterizer")
_REF_RASTER_SRC_CANDIDATES = (os.path.join("/root/reference", _REF_RASTER_SUBDIR),
                              os.path.join(os.path.dirname(os.path.dirname(_HERE)), "reference", _REF_RASTER_SUBDIR))
_HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def build(force: bool = False) -> str:
    """Compile oracle/*.c into oracle/liboracle.so with gcc (seconds), and the reference rasterizer where it can be built."""
    so = os.path.join(_HERE, "liboracle.so")
    srcs = [os.path.join(_HERE, f) for f in ("raster_ref.c",)]
    if force or not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.check_call(["make", "-C", _HERE, "-B", "liboracle.so"], stdout=subprocess.DEVNULL)
    build_ref_raster(force)
    return so


def _ref_raster_inputs():
    out = []
    for d, _, files in os.walk(_REF_RASTER_RECIPE):
        out += [os.path.join(d, f) for f in files if not f.endswith((".pyc", ".o", ".so"))]
    return out


def ref_raster_src():
    """The reference checkout's cuda_rasterizer/ directory if this machine has a readable one, else None."""
    env = os.environ.get("REF_RASTER_SRC")
    for src in ([env] if env else list(_REF_RASTER_SRC_CANDIDATES)):
        if all(os.access(os.path.join(src, f), os.R_OK) for f in ("forward.cu", "backward.cu", "rasterizer_impl.cu")):
            return src
    return None


def _newer_than_recipe(so):
    return os.path.exists(so) and all(os.path.getmtime(f) <= os.path.getmtime(so) for f in _ref_raster_inputs())


def build_ref_raster(force: bool = False):
    """oracle/_ref/libglm_check.so (the GLM shim's host-only checks, our sources only) wherever hipcc is, and
    oracle/_ref/libref_raster.so from the reference checkout's cuda_rasterizer/ where one is readable (about 20 s of hipcc).

    Each is skipped when it is newer than the shim, the wrapper and the recipe.  Where the checkout or hipcc is absent
    (a machine that only runs the tests), an existing oracle/_ref/ is left as it is and nothing is raised; the tests that
    need the library then fail with a clear message if it never arrived.  Returns the library's path, or None."""
    if not os.access(_HIPCC, os.X_OK):
        return REF_RASTER_SO if os.path.exists(REF_RASTER_SO) else None
    make = ["make", "-C", _REF_RASTER_RECIPE, f"HIPCC={_HIPCC}"] + (["-B"] if force else [])
    if force or not _newer_than_recipe(GLM_CHECK_SO):
        subprocess.check_call(make + ["glm"], stdout=subprocess.DEVNULL)
    src = ref_raster_src()
    if src is None:
        return REF_RASTER_SO if os.path.exists(REF_RASTER_SO) else None
    if force or not _newer_than_recipe(REF_RASTER_SO):
        subprocess.check_call(make + ["-j4", f"REF_RASTER_SRC={src}"], stdout=subprocess.DEVNULL)
    return REF_RASTER_SO


def lib() -> ctypes.CDLL:
    global _LIB
    if _LIB is None:
        so = os.path.join(_HERE, "liboracle.so")
        if not os.path.exists(so):
            build()
        _LIB = ctypes.CDLL(so)
    return _LIB
