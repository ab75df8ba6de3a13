// Filter callbacks below an instance (device config inst_filters=1): the EXCL form of the two-level kernel of trace_instance.hip, for the
// re-traces of the host filter loop (rt_filter.cpp).  The loop traces closest candidates, the host runs the callbacks, a rejected
// candidate goes on its ray's exclusion list and the ray is traced again: a launch on the mesh instance accel that carries such a list
// (LaunchParams::exclOffsets != nullptr; trace.h describes the entries) is handed over by launch_trace_instance, launch_trace_instance_mesh_mb
// and launch_trace_instance_mesh_mb_linear to this unit (the kinds 32 / 33 keep theirs beside their kernel, trace_instance_top_linear.hip).  Its kernels are the text of trace_instance_body.hip.h with EXCL = true: in the
// triangle, quad, motion-blur triangle and motion-blur quad leaf loops a candidate that passed its test is dropped BEFORE the block's
// minimum selection when the list names (instance geomID, geomID, primID, bits of t) - so the block's next best candidate is found, and
// everything else (traversal order, tfar at block entry, ties) is the unfiltered kernel's.  The loop always asks for the closest
// candidate, any-hit queries included, so only OCCLUDED = false exists:
//   kinds 14..21   PLUECKER x QUADS x XFMB                     8 forms
//   kinds 22 / 23  MESHMB (QUADS and XFMB present)             2 forms
//   kinds 30 / 31  NODEMB (MESHMB over time-dependent nodes)   2 forms
// each for 16-byte aligned records (VEC) and for any others: 24 instantiations.  They serve latency-bound filter rounds of a few rays,
// not the metric: each is asked for the waves per SIMD of its unfiltered twin, or for one less where the scan's registers would
// otherwise spill (trace_instance.hip.h instance_min_waves) - none may use scratch (tools/kernel_resources.sh, docs/experiments.md
// "Filters below an instance").
#include "trace_instance.hip.h"

namespace rtamd {
namespace dev {

// the EXCL twin of a closest-hit form (the one over a time-dependent top level is trace_instance_top_linear.hip's filter kernel)
constexpr InstanceForm instance_filter_form(bool pluecker, bool vec, bool quads, bool xfmb, bool meshmb, bool nodemb)
{
  InstanceForm f = instance_form(pluecker, false, vec, quads, xfmb);
  f.MESHMB = meshmb; f.NODEMB = nodemb;
  f.EXCL = true;
  return f;
}

template <bool Pluecker, bool Vec, bool Quads, bool Xfmb, bool MeshMb, bool NodeMb>
__global__ __launch_bounds__(TRACE_BLOCK, instance_min_waves(instance_filter_form(Pluecker, Vec, Quads, Xfmb, MeshMb, NodeMb))) void trace_instance_filter_kernel(LaunchParams P)
{
  constexpr InstanceForm FORM = instance_filter_form(Pluecker, Vec, Quads, Xfmb, MeshMb, NodeMb);
  using Leaf = MeshLeaves;
#include "trace_instance_body.hip.h"
}

template <bool PLUECKER, bool QUADS, bool XFMB, bool MESHMB, bool NODEMB>
inline hipError_t launch_instance_filter_vec(const LaunchParams& p, hipStream_t stream)
{
  return launch_instance_pair<trace_instance_filter_kernel<PLUECKER, true, QUADS, XFMB, MESHMB, NODEMB>, trace_instance_filter_kernel<PLUECKER, false, QUADS, XFMB, MESHMB, NODEMB>>(p, stream);
}

} // namespace dev

hipError_t launch_trace_instance_filter(const LaunchParams& p, hipStream_t stream)
{
  // a list, its two-word keys, and a closest-hit launch: anything else is a caller's mistake, not a kernel to fall back to
  if (p.counters || p.occluded || !p.exclOffsets || !p.exclPairs || !p.exclT) return hipErrorInvalidValue;
  switch (p.accel.kind) {
  case ACCEL_INST_TRI_PLUECKER: return dev::launch_instance_filter_vec<true, false, false, false, false>(p, stream);
  case ACCEL_INST_TRI_MOELLER: return dev::launch_instance_filter_vec<false, false, false, false, false>(p, stream);
  case ACCEL_INST_PLUECKER: return dev::launch_instance_filter_vec<true, true, false, false, false>(p, stream);
  case ACCEL_INST_MOELLER: return dev::launch_instance_filter_vec<false, true, false, false, false>(p, stream);
  case ACCEL_INSTMB_TRI_PLUECKER: return dev::launch_instance_filter_vec<true, false, true, false, false>(p, stream);
  case ACCEL_INSTMB_TRI_MOELLER: return dev::launch_instance_filter_vec<false, false, true, false, false>(p, stream);
  case ACCEL_INSTMB_PLUECKER: return dev::launch_instance_filter_vec<true, true, true, false, false>(p, stream);
  case ACCEL_INSTMB_MOELLER: return dev::launch_instance_filter_vec<false, true, true, false, false>(p, stream);
  case ACCEL_INSTMESHMB_PLUECKER: return dev::launch_instance_filter_vec<true, true, true, true, false>(p, stream);
  case ACCEL_INSTMESHMB_MOELLER: return dev::launch_instance_filter_vec<false, true, true, true, false>(p, stream);
  case ACCEL_INSTMESHMB_LINEAR_PLUECKER: return dev::launch_instance_filter_vec<true, true, true, true, true>(p, stream);
  case ACCEL_INSTMESHMB_LINEAR_MOELLER: return dev::launch_instance_filter_vec<false, true, true, true, true>(p, stream);
  default: return hipErrorInvalidValue;
  }
}

} // namespace rtamd
