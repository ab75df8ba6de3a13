// Line segments and flat curves below an instance (device config inst_hair=1; accel kinds ACCEL_INSTMESHMB_PLUECKER / ACCEL_INSTMESHMB_MOELLER
// with LaunchParams::instHair set): the HAIR form of the two-level kernel of trace_instance.hip, in a unit of its own so that its eight
// instantiations compile beside the others.  It is the MESHMB form of trace_instance_mesh_mb.hip with two more trees per instanced scene:
//   2"'. the scene's InstanceSceneRecord holds six roots - triangles, motion-blur triangles, quads, motion-blur quads, curves, lines, in
//        Scene::commit's order; the curve and the line root lead its second dwordx4.  The pending trees wait as markers REF_INST_TREE(code)
//        above the exit marker, as in the MESHMB form; three state bits hold the code of the tree the lane is in;
//   3"'. a leaf of the curve or the line tree is CurveLeaf::intersect / LineLeaf::intersect (trace_curve.hip.h, trace_line.hip.h) on the
//        LOCAL ray: the ray's own space (line_space) is built from the local direction, whose length the instance's scale changes, as the
//        reference hands the transformed ray to the instanced scene's intersectors unchanged (instance_intersector.cpp:51-62).  The
//        CurveRecords and LineRecords lie in sections of `blobs` that start at multiples of 80 and 48 bytes behind the QuadMBRecords; the
//        leaf references are rebased so that `blobs` is indexed as one array of that record type, which is how the two leaves index
//        P.accel.blobs.  A hit below the instance sets instID; any-hit ends the ray;
//   4"'. the exit marker clears the three bits and the world ray is read again.
// The leaf-batching rule (leafBatch / nodeWork) runs over all six leaf kinds together.  Swept node boxes only, and no exclusion scan:
// hair below a top scene of a linear kind, and filters beside instanced hair, are refused at commit / at the call.
#include "trace_instance.hip.h"

namespace rtamd {
namespace dev {

// (its form, instance_hair_form, is in trace_instance.hip.h: the HAIRMB form starts from it)
template <bool Pluecker, bool Occluded, bool Vec>
__global__ __launch_bounds__(TRACE_BLOCK, instance_min_waves(instance_hair_form(Pluecker, Occluded, Vec))) void trace_instance_hair_kernel(LaunchParams P)
{
  constexpr InstanceForm FORM = instance_hair_form(Pluecker, Occluded, Vec);
  using Leaf = MeshLeaves;
#include "trace_instance_body.hip.h"
}

template <bool PLUECKER, bool OCCLUDED>
inline hipError_t launch_instance_hair_vec(const LaunchParams& p, hipStream_t stream)
{
  return launch_instance_pair<trace_instance_hair_kernel<PLUECKER, OCCLUDED, true>, trace_instance_hair_kernel<PLUECKER, OCCLUDED, false>>(p, stream);
}

} // namespace dev

hipError_t launch_trace_instance_hair(const LaunchParams& p, hipStream_t stream)
{
  if (p.counters || p.exclOffsets || p.instHair != 1u) return hipErrorInvalidValue; // no instrumented twin, no EXCL form
  switch (p.accel.kind) {
  case ACCEL_INSTMESHMB_PLUECKER: return p.occluded ? dev::launch_instance_hair_vec<true, true>(p, stream) : dev::launch_instance_hair_vec<true, false>(p, stream);
  case ACCEL_INSTMESHMB_MOELLER: return p.occluded ? dev::launch_instance_hair_vec<false, true>(p, stream) : dev::launch_instance_hair_vec<false, false>(p, stream);
  default: return hipErrorInvalidValue;
  }
}

} // namespace rtamd
