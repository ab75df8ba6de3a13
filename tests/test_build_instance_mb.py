"""CPU-side build check (no GPU): the 32 instantiations of the two-level instance kernel (trace_instance.hip) - Pluecker / Moeller x
closest hit / occluded x aligned / unaligned records x triangles / triangles and quads x static / moving instances (XFMB) - are all in
the library, none uses scratch, and each stays within the registers of the wave bound documented for it: four waves per SIMD (at most
128 VGPRs), three (at most 168) for closest-hit Pluecker with quads."""
import itertools
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from kernel_metadata import kernel_metadata  # noqa: E402

LIB = os.path.join(ROOT, "embree-compressed_amd", "lib", "libembree3.so")


def test_all_instance_kernel_instantiations_are_present_without_scratch_and_within_their_wave_bound():
    md = {n: r for n, r in kernel_metadata(LIB).items() if n.startswith("trace_instance_kernel<")}
    names = {}
    for pluecker, occluded, vec, quads, xfmb in itertools.product((False, True), repeat=5):
        n = "trace_instance_kernel<%s>" % ", ".join(str(b).lower() for b in (pluecker, occluded, vec, quads, xfmb))
        names[n] = 168 if (quads and pluecker and not occluded) else 128
    assert sorted(md) == sorted(names) and len(md) == 32
    bad = [(n, md[n]["vgpr"], md[n]["agpr"], md[n]["scratch"]) for n, cap in names.items()
           if md[n]["scratch"] != 0 or md[n]["vgpr"] + md[n]["agpr"] > cap]
    assert not bad, bad
