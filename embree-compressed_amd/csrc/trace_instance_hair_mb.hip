// Line segments and flat curves with time steps below an instance (device config inst_hair=1,inst_hair_mb=1; accel kinds
// ACCEL_INSTMESHMB_PLUECKER / ACCEL_INSTMESHMB_MOELLER with LaunchParams::instHair == 2): the HAIRMB form of the two-level kernel of
// trace_instance.hip, in a unit of its own so that its eight instantiations compile beside the others.  It is the HAIR form of
// trace_instance_hair.hip with two more trees per instanced scene:
//   2"". the scene's InstanceSceneRecord holds eight roots.  Visiting order is the slot order of Scene - triangles, motion-blur triangles,
//        quads, motion-blur quads, curves, motion-blur curves, lines, motion-blur lines; the record keeps the static hair roots in words 4
//        and 5 and the moving ones in words 6 and 7, all in the second dwordx4 the HAIR form loads already.  Up to seven pending trees wait
//        as markers REF_INST_TREE(code) above the exit marker; the three state bits of the HAIR form hold the codes 6 and 7 too;
//   3"". a leaf of the two new trees is CurveMBLeaf::intersect / LineMBLeaf::intersect (trace_curve_mb.hip.h, trace_line_mb.hip.h) on the
//        LOCAL ray at the ray's time, which is the same in both spaces and read through the ray's index.  The CurveMBRecords and
//        LineMBRecords lie in sections of `blobs` that start at multiples of 160 and 80 bytes behind the LineRecords, the leaf references
//        rebased so that `blobs` is indexed as one array of that record type.  The trees' nodes are swept QNode8s: moving hair built under
//        mb_bounds=linear is refused at commit.
// Each tree is traced against the tfar the one before it left; a later tree wins a bit-identical t.  No exclusion scan, like the HAIR form.
#include "trace_instance.hip.h"

namespace rtamd {
namespace dev {

constexpr InstanceForm instance_hair_mb_form(bool pluecker, bool occluded, bool vec)
{
  InstanceForm f = instance_hair_form(pluecker, occluded, vec);
  f.HAIRMB = true;
  return f;
}

template <bool Pluecker, bool Occluded, bool Vec>
__global__ __launch_bounds__(TRACE_BLOCK, instance_min_waves(instance_hair_mb_form(Pluecker, Occluded, Vec))) void trace_instance_hair_mb_kernel(LaunchParams P)
{
  constexpr InstanceForm FORM = instance_hair_mb_form(Pluecker, Occluded, Vec);
  using Leaf = MeshLeaves;
#include "trace_instance_body.hip.h"
}

template <bool PLUECKER, bool OCCLUDED>
inline hipError_t launch_instance_hair_mb_vec(const LaunchParams& p, hipStream_t stream)
{
  return launch_instance_pair<trace_instance_hair_mb_kernel<PLUECKER, OCCLUDED, true>, trace_instance_hair_mb_kernel<PLUECKER, OCCLUDED, false>>(p, stream);
}

} // namespace dev

hipError_t launch_trace_instance_hair_mb(const LaunchParams& p, hipStream_t stream)
{
  if (p.counters || p.exclOffsets || p.instHair != 2u) return hipErrorInvalidValue; // no instrumented twin, no EXCL form
  switch (p.accel.kind) {
  case ACCEL_INSTMESHMB_PLUECKER: return p.occluded ? dev::launch_instance_hair_mb_vec<true, true>(p, stream) : dev::launch_instance_hair_mb_vec<true, false>(p, stream);
  case ACCEL_INSTMESHMB_MOELLER: return p.occluded ? dev::launch_instance_hair_mb_vec<false, true>(p, stream) : dev::launch_instance_hair_mb_vec<false, false>(p, stream);
  default: return hipErrorInvalidValue;
  }
}

} // namespace rtamd
