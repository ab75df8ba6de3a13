"""CPU-side build check (no GPU): the 8 instantiations of the NODEMB form of the two-level kernel (trace_instance_mesh_mb_linear.hip,
accel kinds 30 / 31) - Pluecker / Moeller x closest hit / occluded x aligned / unaligned records - are in the library, none uses
scratch, and each stays within the registers of the wave bound it is asked for, which is the bound of its twin in
trace_instance_mesh_mb.hip: any hit four waves per SIMD (at most 128 VGPRs), closest-hit Moeller three (168), closest-hit Pluecker
two (256).  The 40 kernels of the other forms are still there under their names."""
import itertools
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from kernel_metadata import kernel_metadata  # noqa: E402

LIB = os.path.join(ROOT, "embree-compressed_amd", "lib", "libembree3.so")


def test_the_eight_nodemb_instantiations_are_present_without_scratch_and_within_their_wave_bound():
    all_md = kernel_metadata(LIB)
    md = {n: r for n, r in all_md.items() if n.startswith("trace_instance_mesh_mb_linear_kernel<")}
    caps = {}
    for pluecker, occluded, vec in itertools.product((False, True), repeat=3):
        n = "trace_instance_mesh_mb_linear_kernel<%s>" % ", ".join(str(b).lower() for b in (pluecker, occluded, vec))
        caps[n] = 128 if occluded else (256 if pluecker else 168)
    assert sorted(md) == sorted(caps) and len(md) == 8
    bad = [(n, md[n]["vgpr"], md[n]["agpr"], md[n]["scratch"]) for n, cap in caps.items() if md[n]["scratch"] != 0 or md[n]["vgpr"] + md[n]["agpr"] > cap]
    assert not bad, bad
    assert sum(n.startswith("trace_instance_kernel<") for n in all_md) == 32 and sum(n.startswith("trace_instance_mesh_mb_kernel<") for n in all_md) == 8
