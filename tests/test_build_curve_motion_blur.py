"""CPU-side build check (no GPU): the kernels of the motion-blur ribbon leaf (trace_curve_mb.hip, accel kinds 44..47) are in the library -
CurveMBLeaf and CurveMBLeafLinear, robust and fast, closest hit and occluded, plain and counted twins, aligned and unaligned records: what
launch_leaf instantiates per (leaf, ROBUST) pair, times two per leaf.  None uses scratch or spills a vector register; the plain kernels
stay within the three waves per SIMD they are compiled for (at most 168 VGPRs, no spilled scalar register either), the counted twins
within their two (256).  There is no pool and no service kernel for them.  The families of the static curve leaf and of the motion-blur
line leaf are what they were."""
import itertools
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from kernel_metadata import kernel_metadata  # noqa: E402

LIB = os.path.join(ROOT, "embree-compressed_amd", "lib", "libembree3.so")


def _family(md, leaf):
    return {n: r for n, r in md.items() if n.startswith("trace_kernel<%s, " % leaf)}


def test_the_motion_blur_curve_kernels_are_present_without_scratch_and_within_their_wave_bounds():
    md = kernel_metadata(LIB)
    bad = []
    for leaf in ("CurveMBLeaf", "CurveMBLeafLinear"):
        fam = _family(md, leaf)
        want = ["trace_kernel<%s, %s>" % (leaf, ", ".join(str(b).lower() for b in bits)) for bits in itertools.product((False, True), repeat=4)]
        assert sorted(fam) == sorted(want) and len(fam) == 16, sorted(fam)
        for n, r in fam.items():
            counted = n[n.index("<") + 1: n.rindex(">")].rsplit(",", 4)[-2].strip() == "true"
            cap = 256 if counted else 168
            if r["scratch"] != 0 or r["vgpr_spills"] != 0 or r["vgpr"] + r["agpr"] > cap or (not counted and r["sgpr_spills"] != 0):
                bad.append((n, r["vgpr"], r["agpr"], r["scratch"], r["sgpr_spills"], r["vgpr_spills"]))
    assert not bad, bad
    assert not any("CurveMB" in n and not n.startswith("trace_kernel<CurveMBLeaf") for n in md)  # lane kernel only: no pool, no service kernel


def test_the_existing_curve_and_motion_blur_line_families_are_unchanged():
    md = kernel_metadata(LIB)
    assert len(_family(md, "CurveLeaf")) == 16 and not any(n.startswith("trace_pool_kernel<CurveLeaf") or n.startswith("service_kernel<CurveLeaf") for n in md)
    for leaf in ("LineMBLeaf", "LineMBLeafLinear"):
        assert len(_family(md, leaf)) == 16, leaf
    assert not any(n.startswith("trace_pool_kernel<LineMB") or n.startswith("service_kernel<LineMB") for n in md)
