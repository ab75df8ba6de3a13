"""CPU-side build check (no GPU): the kernels of the motion-blur line leaf (trace_line_mb.hip, accel kinds 38..41) are in the library -
LineMBLeaf and LineMBLeafLinear, robust and fast, closest hit and occluded, plain and counted twins, aligned and unaligned records: what
launch_leaf instantiates per (leaf, ROBUST) pair, the number the library holds for TriMBLeaf<false>, times two per leaf.  None uses
scratch or spills a vector register; the plain kernels stay within the three waves per SIMD they are compiled for (at most 168 VGPRs,
no spilled scalar register either), the counted twins within their two (256).  The families of the static line leaf and of the
motion-blur triangle leaf are what they were."""
import itertools
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from kernel_metadata import kernel_metadata  # noqa: E402

LIB = os.path.join(ROOT, "embree-compressed_amd", "lib", "libembree3.so")


def _family(md, leaf):
    return {n: r for n, r in md.items() if n.startswith("trace_kernel<%s, " % leaf)}


def test_the_motion_blur_line_kernels_are_present_without_scratch_and_within_their_wave_bounds():
    md = kernel_metadata(LIB)
    per_pair = len(_family(md, "TriMBLeaf<false>"))  # launch_leaf<TriMBLeaf<false>, false>: occluded x counted x aligned
    assert per_pair == 8
    bad = []
    for leaf in ("LineMBLeaf", "LineMBLeafLinear"):
        fam = _family(md, leaf)
        want = ["trace_kernel<%s, %s>" % (leaf, ", ".join(str(b).lower() for b in bits)) for bits in itertools.product((False, True), repeat=4)]
        assert sorted(fam) == sorted(want) and len(fam) == 2 * per_pair, sorted(fam)
        for n, r in fam.items():
            counted = n[n.index("<") + 1: n.rindex(">")].rsplit(",", 4)[-2].strip() == "true"
            cap = 256 if counted else 168
            if r["scratch"] != 0 or r["vgpr_spills"] != 0 or r["vgpr"] + r["agpr"] > cap or (not counted and r["sgpr_spills"] != 0):
                bad.append((n, r["vgpr"], r["agpr"], r["scratch"], r["sgpr_spills"], r["vgpr_spills"]))
    assert not bad, bad
    assert not any(n.startswith("trace_pool_kernel<LineMB") or n.startswith("service_kernel<LineMB") for n in md)  # lane kernel only


def test_the_existing_line_and_motion_blur_triangle_families_are_unchanged():
    md = kernel_metadata(LIB)
    assert len(_family(md, "LineLeaf")) == 16 and sum(n.startswith("trace_pool_kernel<LineLeaf, ") for n in md) == 16
    for leaf in ("TriMBLeaf<true>", "TriMBLeaf<false>", "TriMBLeafLinear<true>", "TriMBLeafLinear<false>"):
        assert len(_family(md, leaf)) == 8, leaf
