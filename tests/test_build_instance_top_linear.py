"""CPU-side build check (no GPU): the 8 instantiations of the TOPMB form of the two-level kernel (trace_instance_top_linear.hip, accel
kinds 32 / 33) - Pluecker / Moeller x closest hit / occluded x aligned / unaligned records - and the 4 of its EXCL form for the
re-traces of the host filter loop are in the library, none uses scratch or spills, and each stays within the registers of the wave
bound it is asked for, which is the bound of its NODEMB twin: any hit four waves per SIMD (at most 128 VGPRs), closest-hit Moeller
three (168), closest-hit Pluecker two (256); the filter kernels are closest-hit kernels.  The kernels of the four existing families are
still there under their names, as many as before."""
import itertools
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from kernel_metadata import kernel_metadata  # noqa: E402

LIB = os.path.join(ROOT, "embree-compressed_amd", "lib", "libembree3.so")


def _name(base, *flags):
    return "%s<%s>" % (base, ", ".join(str(b).lower() for b in flags))


def test_the_twelve_topmb_instantiations_are_present_without_scratch_and_within_their_wave_bound():
    all_md = kernel_metadata(LIB)
    md = {n: r for n, r in all_md.items() if n.startswith("trace_instance_top_linear_")}
    caps = {}
    for pluecker, occluded, vec in itertools.product((False, True), repeat=3):
        caps[_name("trace_instance_top_linear_kernel", pluecker, occluded, vec)] = 128 if occluded else (256 if pluecker else 168)
    for pluecker, vec in itertools.product((False, True), repeat=2):
        caps[_name("trace_instance_top_linear_filter_kernel", pluecker, vec)] = 256 if pluecker else 168
    assert sorted(md) == sorted(caps) and len(md) == 12
    bad = [(n, md[n]) for n, cap in caps.items()
           if md[n]["scratch"] != 0 or md[n]["sgpr_spills"] != 0 or md[n]["vgpr_spills"] != 0 or md[n]["vgpr"] + md[n]["agpr"] > cap]
    assert not bad, bad
    for n in md:
        print("%-70s vgpr %3d agpr %3d sgpr %3d scratch %d" % (n, md[n]["vgpr"], md[n]["agpr"], md[n]["sgpr"], md[n]["scratch"]))


def test_the_existing_families_keep_their_counts():
    names = list(kernel_metadata(LIB))
    count = lambda prefix: sum(n.startswith(prefix) for n in names)  # noqa: E731
    assert count("trace_instance_kernel<") == 32
    assert count("trace_instance_mesh_mb_kernel<") == 8
    assert count("trace_instance_mesh_mb_linear_kernel<") == 8
    assert count("trace_instance_filter_kernel<") == 24
