"""CPU-side build check (no GPU): the kernels of the ribbon leaf (trace_curve.hip, accel kinds 42 / 43) are in the library - CurveLeaf,
robust and fast, closest hit and occluded, plain and counted twins, aligned and unaligned records: what launch_leaf instantiates per
(leaf, ROBUST) pair, the number the library holds for LineMBLeaf.  None uses scratch or spills a vector register; the plain kernels stay
within the three waves per SIMD they are compiled for (at most 168 VGPRs), the counted twins within their two (256).  The leaf has no
ray-pool and no service form.  The families of the line leaves are what they were."""
import itertools
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from kernel_metadata import kernel_metadata  # noqa: E402

LIB = os.path.join(ROOT, "embree-compressed_amd", "lib", "libembree3.so")
VGPR_CAP = {3: 168, 2: 256}  # allocated VGPRs + AGPRs per lane that still admit this many waves per SIMD
CURVE_MIN_WAVES = 3          # CurveLeaf::MIN_WAVES


def _family(md, leaf):
    return {n: r for n, r in md.items() if n.startswith("trace_kernel<%s, " % leaf)}


def test_the_curve_kernels_are_present_without_scratch_and_within_their_wave_bounds():
    md = kernel_metadata(LIB)
    fam = _family(md, "CurveLeaf")
    want = ["trace_kernel<CurveLeaf, %s>" % ", ".join(str(b).lower() for b in bits) for bits in itertools.product((False, True), repeat=4)]
    assert sorted(fam) == sorted(want) and len(fam) == len(_family(md, "LineMBLeaf")), sorted(fam)
    bad = []
    for n, r in fam.items():
        counted = n[n.index("<") + 1: n.rindex(">")].rsplit(",", 4)[-2].strip() == "true"
        cap = VGPR_CAP[2] if counted else VGPR_CAP[CURVE_MIN_WAVES]
        if r["scratch"] != 0 or r["vgpr_spills"] != 0 or r["vgpr"] + r["agpr"] > cap:
            bad.append((n, r["vgpr"], r["agpr"], r["scratch"], r["vgpr_spills"]))
    assert not bad, bad
    assert not any(n.startswith("trace_pool_kernel<Curve") or n.startswith("service_kernel<Curve") for n in md)  # lane kernel only


def test_the_line_families_are_unchanged():
    md = kernel_metadata(LIB)
    assert len(_family(md, "LineLeaf")) == 16 and sum(n.startswith("trace_pool_kernel<LineLeaf, ") for n in md) == 16
    for leaf in ("LineMBLeaf", "LineMBLeafLinear"):
        assert len(_family(md, leaf)) == 16, leaf
        assert not any(n.startswith("trace_pool_kernel<%s, " % leaf) for n in md)
