"""The two headline compositors must fit seven workgroups on a compute unit (seven waves per SIMD): at most 72 vector
registers (512 per SIMD lane, allocated in eights), at most floor(163,840 / 7) = 23,405 bytes of LDS, and no more spill /
scratch than the six-wave build they replace had (2 spilled registers, 12 bytes).

render.hip and render_unit_bwd.hip are compiled to assembly for the device only, with the Makefile's HIPFLAGS, into a temporary
directory, and the kernels' metadata records (.amdgpu_metadata: one YAML-like record per kernel) are read -- the four fields
below and the kernel's name, nothing else of the listing."""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "curve_gaussian_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

MAX_VGPRS = 72
MAX_LDS = 163840 // 7          # 23,405
MAX_SPILLS = 2                 # the six-wave parent's figures
MAX_SCRATCH = 12

# (source file, itanium-mangled prefix of the instance) of every kernel shipped at seven waves per SIMD
#   k_render_fwd3<GEO = true, SORT = true, UNIT = true, TAG = true>,  k_render_bwd_unit<STRIDE = 8, GATED = false>
SHIPPED_AT_SEVEN = {
    "k_render_fwd3<true,true,true,true>": ("render.hip", "_ZN3cgs13k_render_fwd3ILb1ELb1ELb1ELb1EEE"),
    "k_render_bwd_unit<8,false>": ("render_unit_bwd.hip", "_ZN3cgs17k_render_bwd_unitILi8ELb0EEE"),
}


def _makefile_hipflags():
    text = open(os.path.join(CSRC, "Makefile")).read()
    arch = re.search(r"^ARCH \?= (\S+)", text, re.M).group(1)
    flags = re.search(r"^HIPFLAGS \?= (.*)$", text, re.M).group(1)
    return flags.replace("$(ARCH)", arch).split()


def _metadata(asm_text):
    """{kernel symbol: {field: int}} from the metadata records of a device assembly listing."""
    out = {}
    for rec in asm_text.split("  - .agpr_count:")[1:]:
        name = re.search(r"^\s+\.name:\s+(\S+)", rec, re.M)
        if not name:
            continue
        fields = {}
        for f in ("vgpr_count", "group_segment_fixed_size", "vgpr_spill_count", "private_segment_fixed_size"):
            m = re.search(r"^\s+\." + f + r":\s+(\d+)", rec, re.M)
            if m:
                fields[f] = int(m.group(1))
        out[name.group(1)] = fields
    return out


@pytest.fixture(scope="module")
def resources(tmp_path_factory):
    if not (os.path.exists(HIPCC) or shutil.which(HIPCC)):
        pytest.skip("hipcc is not installed here")
    tmp = tmp_path_factory.mktemp("compositor_asm")
    found = {}
    for src in sorted({s for s, _ in SHIPPED_AT_SEVEN.values()}):
        asm = os.path.join(str(tmp), src.replace(".hip", ".s"))
        subprocess.run([HIPCC, *_makefile_hipflags(), "-S", "--cuda-device-only", "-w", os.path.join(CSRC, src), "-o", asm],
                       check=True, cwd=str(tmp), capture_output=True)
        found.update(_metadata(open(asm).read()))
    return found


@pytest.mark.parametrize("kernel", list(SHIPPED_AT_SEVEN))
def test_kernel_fits_seven_workgroups_per_compute_unit(resources, kernel):
    prefix = SHIPPED_AT_SEVEN[kernel][1]
    match = [v for k, v in resources.items() if k.startswith(prefix)]
    assert len(match) == 1, f"{kernel}: {len(match)} metadata records start with {prefix}"
    r = match[0]
    print(f"\n   {kernel}: {r}")
    assert r["vgpr_count"] <= MAX_VGPRS, r
    assert r["group_segment_fixed_size"] <= MAX_LDS, r
    assert r["vgpr_spill_count"] <= MAX_SPILLS, r
    assert r["private_segment_fixed_size"] <= MAX_SCRATCH, r
