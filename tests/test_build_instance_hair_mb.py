"""The eight kernels of the HAIRMB form of the two-level kernel (embree-compressed_amd/csrc/trace_instance_hair_mb.hip) are in the library,
free of scratch and of VGPR spills, and within the register cap of the wave bound each is compiled for; moving LineMBLeaf and
CurveMBLeaf into their headers and adding the form left the kernel families of the line, curve and instance units what they were.  Read
from the built library's code objects (tools/kernel_metadata.py), no GPU."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from kernel_metadata import kernel_metadata  # noqa: E402

import test_build_instance_hair as tbh  # noqa: E402  (FAMILY: the family sizes before the HAIR form; CAP)

LIB = os.path.join(ROOT, "embree-compressed_amd", "lib", "libembree3.so")
# waves per SIMD asked of trace_instance_hair_mb_kernel<PLUECKER, OCCLUDED, *> (trace_instance.hip.h TRACE_INST_HAIRMB_MIN_WAVES_*) and the
# registers (VGPR + AGPR) a wave may use at that bound on gfx950: 512 / waves, in units of 8
WAVES = {("true", "false"): 2, ("false", "false"): 2, ("true", "true"): 3, ("false", "true"): 3}
CAP = {2: 256, 3: 168, 4: 128}
assert CAP == tbh.CAP


@pytest.fixture(scope="module")
def meta():
    return kernel_metadata(LIB)


def test_the_eight_moving_hair_kernels_have_no_scratch_and_no_vgpr_spills(meta):
    hair = {n: r for n, r in meta.items() if n.startswith("trace_instance_hair_mb_kernel<")}
    assert len(hair) == 8, sorted(hair)
    for n, r in sorted(hair.items()):
        pl, occ, vec = re.match(r"trace_instance_hair_mb_kernel<(\w+), (\w+), (\w+)>", n).groups()
        cap = CAP[WAVES[(pl, occ)]]
        print(f"{n}: {r['vgpr']} VGPRs + {r['agpr']} AGPRs of {cap} at {WAVES[(pl, occ)]} waves per SIMD, scratch {r['scratch']}, spills s{r['sgpr_spills']} / v{r['vgpr_spills']}")
        assert r["scratch"] == 0 and r["vgpr_spills"] == 0, (n, r)
        assert r["vgpr"] + r["agpr"] <= cap, (n, r)
        assert r["max_wg"] == 256, (n, r)


def test_the_family_sizes_of_the_line_curve_and_instance_units_are_what_they_were(meta):
    for prefix, n in dict(tbh.FAMILY, **{"trace_instance_hair_kernel<": 8}).items():
        got = sum(1 for name in meta if name.startswith(prefix))
        assert got == n, (prefix, got, n)
