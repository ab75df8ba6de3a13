"""CPU-side build check (no GPU): the 24 instantiations of the EXCL form of the two-level instance kernel (trace_instance_filter.hip, the
re-traces of the host filter loop below an instance: 8 forms of the kinds 14..21, the MESHMB and the NODEMB form, Pluecker / Moeller,
aligned / general records, closest hit only) are all in the library, none uses scratch or spills, and each stays within the registers of
the wave bound it is asked for: the bound of its unfiltered twin, one wave less for the Pluecker triangle-only forms (docs/experiments.md,
"Filters below an instance").  The unfiltered kernels keep their numbers."""
import itertools
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from kernel_metadata import kernel_metadata  # noqa: E402

LIB = os.path.join(ROOT, "embree-compressed_amd", "lib", "libembree3.so")
VGPRS_AT = {4: 128, 3: 168, 2: 256}  # waves per SIMD -> registers a wave may have (512 per SIMD lane, allocated in blocks of 8)


def _waves(pluecker, meshmb):
    if meshmb:
        return 2 if pluecker else 3
    # with quads: the twin's bound; triangles only: the Pluecker twin runs at 4 and has no register to spare for the scan
    return 3 if pluecker else 4


def test_all_filter_kernel_instantiations_are_present_without_scratch_and_within_their_wave_bound():
    all_md = kernel_metadata(LIB)
    md = {n: r for n, r in all_md.items() if n.startswith("trace_instance_filter_kernel<")}
    forms = [(q, x, False, False) for q, x in itertools.product((False, True), repeat=2)] + [(True, True, True, False), (True, True, True, True)]
    names = {}
    for pluecker, vec in itertools.product((False, True), repeat=2):
        for quads, xfmb, meshmb, nodemb in forms:
            n = "trace_instance_filter_kernel<%s>" % ", ".join(str(b).lower() for b in (pluecker, vec, quads, xfmb, meshmb, nodemb))
            names[n] = VGPRS_AT[_waves(pluecker, meshmb)]
    assert sorted(md) == sorted(names) and len(md) == 24
    bad = [(n, md[n]["vgpr"], md[n]["agpr"], md[n]["scratch"], md[n]["sgpr_spills"], md[n]["vgpr_spills"]) for n, cap in names.items()
           if md[n]["scratch"] != 0 or md[n]["sgpr_spills"] or md[n]["vgpr_spills"] or md[n]["vgpr"] + md[n]["agpr"] > cap]
    assert not bad, bad
    # the unfiltered two-level kernels are all still there (their own build checks hold their registers)
    assert sum(n.startswith("trace_instance_kernel<") for n in all_md) == 32
    assert sum(n.startswith("trace_instance_mesh_mb_kernel<") for n in all_md) == 8
    assert sum(n.startswith("trace_instance_mesh_mb_linear_kernel<") for n in all_md) == 8
