"""CPU-side build check (no GPU): the kernels of the tube leaf (trace_round_curve.hip, accel kinds 42 / 43 with Accel::roundCurves) are in
the library - RoundCurveLeaf, robust and fast, closest hit and occluded, plain and counted twins, aligned and unaligned records: the 16
instantiations launch_leaf gives a (leaf, ROBUST) pair.  None uses scratch or spills a vector register; the plain kernels stay within the
waves per SIMD the leaf declares (RoundCurveLeaf::MIN_WAVES, read from the header; 2: at most 256 VGPRs) and within the figures measured for
this leaf (209 closest hit, 179 any hit: profiles/round_curve_kernel_resources.txt), the counted twins within 256.  The leaf has no ray-pool and no service form.  The families of the ribbon and line leaves count what they counted."""
import itertools
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from kernel_metadata import kernel_metadata  # noqa: E402

LIB = os.path.join(ROOT, "embree-compressed_amd", "lib", "libembree3.so")
VGPR_CAP = {3: 168, 2: 256}  # allocated VGPRs + AGPRs per lane that still admit this many waves per SIMD
HEADER = os.path.join(ROOT, "embree-compressed_amd", "csrc", "trace_round_curve.hip.h")
MEASURED = {"closest hit": 209, "any hit": 179}  # VGPRs of the plain kernels as built (profiles/round_curve_kernel_resources.txt): an upper bound


def _min_waves():
    """RoundCurveLeaf::MIN_WAVES as the header declares it"""
    text = open(HEADER).read()
    leaf = text[text.index("struct RoundCurveLeaf"):]
    return int(re.search(r"static constexpr int MIN_WAVES = (\d+);", leaf).group(1))


def _family(md, leaf):
    return {n: r for n, r in md.items() if n.startswith("trace_kernel<%s, " % leaf)}


def test_the_round_curve_kernels_are_present_without_scratch_and_within_their_wave_bounds():
    md = kernel_metadata(LIB)
    fam = _family(md, "RoundCurveLeaf")
    want = ["trace_kernel<RoundCurveLeaf, %s>" % ", ".join(str(b).lower() for b in bits) for bits in itertools.product((False, True), repeat=4)]
    assert sorted(fam) == sorted(want), sorted(fam)
    bad = []
    for n, r in fam.items():
        counted = n[n.index("<") + 1: n.rindex(">")].rsplit(",", 4)[-2].strip() == "true"
        occluded = n[n.index("<") + 1: n.rindex(">")].rsplit(",", 4)[-3].strip() == "true"
        cap = VGPR_CAP[2] if counted else min(VGPR_CAP[_min_waves()], MEASURED["any hit" if occluded else "closest hit"])
        if r["scratch"] != 0 or r["vgpr_spills"] != 0 or r["vgpr"] + r["agpr"] > cap:
            bad.append((n, r["vgpr"], r["agpr"], r["scratch"], r["vgpr_spills"]))
    assert not bad, bad
    assert not any(n.startswith("trace_pool_kernel<RoundCurve") or n.startswith("service_kernel<RoundCurve") for n in md)  # lane kernel only


def test_the_ribbon_and_line_families_are_unchanged():
    md = kernel_metadata(LIB)
    assert len(_family(md, "CurveLeaf")) == 16 and not any(n.startswith("trace_pool_kernel<Curve") or n.startswith("service_kernel<Curve") for n in md)
    assert len(_family(md, "LineLeaf")) == 16 and sum(n.startswith("trace_pool_kernel<LineLeaf, ") for n in md) == 16
    for leaf in ("LineMBLeaf", "LineMBLeafLinear", "CurveMBLeaf", "CurveMBLeafLinear"):
        assert len(_family(md, leaf)) == 16, leaf
        assert not any(n.startswith("trace_pool_kernel<%s, " % leaf) for n in md)
