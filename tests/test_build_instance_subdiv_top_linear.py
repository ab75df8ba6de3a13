"""CPU-side build check (no GPU): the 24 instantiations of the TOPMB form of the subdivision two-level kernel
(trace_instance_subdiv_top_linear.hip, accel kinds 34 / 35) - the eager leaf and bvh4.compressed.leaf at C = 1..5 x closest hit /
occluded x aligned / unaligned records - are in the library, none needs scratch or spills vector registers that its swept twin does
not, and each stays within the registers of the wave bound it is asked for, which is its twin's (instance_min_waves).  The library
exports the new launch symbol, and the 24 kernels of the swept form are still there under their names."""
import itertools
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from kernel_metadata import kernel_metadata  # noqa: E402

LIB = os.path.join(ROOT, "embree-compressed_amd", "lib", "libembree3.so")
LEAVES = ["GridCellLeaf"] + ["CbvhLeaf<1, %d, false>" % c for c in range(1, 6)]
# VGPRs of a wave bound on gfx950 (512 per SIMD lane, in blocks of 8): 2 waves 256, 3 waves 168, 4 waves 128
CAP = {2: 256, 3: 168, 4: 128}


def _waves(leaf, occluded):
    """instance_min_waves (trace_instance.hip.h): the leaf's top-level bound (3; cBVH from C = 4 on 2), one less for the eager
    closest-hit kernel"""
    if leaf == "GridCellLeaf":
        return 3 if occluded else 2
    return 2 if int(leaf.split(",")[1]) >= 4 else 3


def _name(base, leaf, *flags):
    return "%s<%s, %s>" % (base, leaf, ", ".join(str(b).lower() for b in flags))


def test_the_24_topmb_instantiations_are_present_and_need_no_more_scratch_than_their_twins():
    all_md = kernel_metadata(LIB)
    md = {n: r for n, r in all_md.items() if n.startswith("trace_instance_subdiv_top_linear_kernel<")}
    want = [(leaf, occ, vec) for leaf in LEAVES for occ, vec in itertools.product((False, True), repeat=2)]
    assert sorted(md) == sorted(_name("trace_instance_subdiv_top_linear_kernel", *w) for w in want) and len(md) == 24
    bad = []
    for leaf, occ, vec in want:
        r, twin = md[_name("trace_instance_subdiv_top_linear_kernel", leaf, occ, vec)], all_md[_name("trace_instance_subdiv_kernel", leaf, occ, vec)]
        print("%-24s occluded %-5s vec %-5s vgpr %3d (twin %3d) sgpr %3d scratch %d (twin %d) sgpr spills %d (twin %d)"
              % (leaf, occ, vec, r["vgpr"], twin["vgpr"], r["sgpr"], r["scratch"], twin["scratch"], r["sgpr_spills"], twin["sgpr_spills"]))
        if r["scratch"] > twin["scratch"] or r["vgpr_spills"] > twin["vgpr_spills"] or r["vgpr"] + r["agpr"] > CAP[_waves(leaf, occ)] or r["lds"] != twin["lds"]:
            bad.append((leaf, occ, vec, r, twin))
    assert not bad, bad


def test_the_swept_form_keeps_its_24_kernels_and_the_launch_symbol_is_exported():
    names = list(kernel_metadata(LIB))
    assert sum(n.startswith("trace_instance_subdiv_kernel<") for n in names) == 24
    src = open(os.path.join(ROOT, "embree-compressed_amd", "csrc", "trace_instance_subdiv_top_linear.hip")).read()
    assert "launch_trace_instance_subdiv_top_linear" in src
    with open(LIB, "rb") as f:
        text = f.read()
    for fn in ("launch_trace_instance_subdiv_top_linear", "launch_trace_instance_subdiv"):  # the Itanium-mangled names in the symbol table
        assert ("_ZN5rtamd%d%sERKNS_12LaunchParamsE" % (len(fn), fn)).encode() in text, fn
