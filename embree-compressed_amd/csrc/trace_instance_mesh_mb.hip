// Motion-blur triangle and quad meshes below an instance (accel kinds ACCEL_INSTMESHMB_PLUECKER / ACCEL_INSTMESHMB_MOELLER): the MESHMB
// form of the two-level kernel of trace_instance.hip, in a unit of its own so that its eight instantiations compile beside the others.
// An instanced scene may hold up to four trees - static triangles, motion-blur triangles, static quads, motion-blur quads - which the
// local ray traverses completely, one after the other, in Scene::commit's order, each against the tfar the one before left (the
// instanced scene's AccelN, scene.cpp:650-654; instance_intersector.cpp:51-62 passes ray.time on unchanged), so a later tree's hit at a
// bit-identical t replaces the earlier one:
//   2". the instance's record names the scene's InstanceSceneRecord (accel.h) with the four roots.  Above the exit marker the lane
//       stacks one marker per pending tree, REF_INST_TREE(code) with the tree's root in the distance word, in reverse visiting order,
//       and continues at the root of the first tree the scene has; two state bits hold the code of the tree it is in;
//   3". popping such a marker - recognised before the distance cull - sets the two bits to its code and continues at its root.  A
//       leaf is then, by the code, TriLeaf / QuadLeaf::intersect (as in the QUADS form) or the block loop of TriMBLeaf::intersect /
//       QuadMBLeaf::intersect (trace_tri_mb.hip, trace_quad_mb.hip) written out in the body over time_segment, lerp_vertex and the static
//       tests (called, these two cost rate or registers: the body gives the figures): the
//       ray's time is read from the ray record through the ray's index (the same value in world and local space), a record is tested
//       only when its segment is the ray's itime, blocks are 4 records, all candidates of a block see the tfar at block entry, the
//       lowest lane wins ties, a later block replaces an equal t, quads split into A = (v0, v1, v3) and B = (v2, v1, v3).  The
//       TriMBRecords and QuadMBRecords lie in sections of `blobs` that start at multiples of their sizes; the leaf references are
//       rebased so that `blobs` is indexed as one array of that record type;
//   4". the exit marker clears the bits.
// Instance steps (XFMB) and the leaf-batching rule (leafBatch / nodeWork, over all four leaf kinds together) are those of the other forms.
// Node boxes of the motion-blur trees are the swept boxes of the motion-blur accels (time-dependent ones: trace_instance_mesh_mb_linear.hip).
#include "trace_instance.hip.h"

namespace rtamd {
namespace dev {

template <bool Pluecker, bool Occluded, bool Vec>
__global__ __launch_bounds__(TRACE_BLOCK, instance_min_waves(instance_mesh_mb_form(Pluecker, Occluded, Vec))) void trace_instance_mesh_mb_kernel(LaunchParams P)
{
  constexpr InstanceForm FORM = instance_mesh_mb_form(Pluecker, Occluded, Vec);
  using Leaf = MeshLeaves;
#include "trace_instance_body.hip.h"
}

template <bool PLUECKER, bool OCCLUDED>
inline hipError_t launch_instance_mesh_mb_vec(const LaunchParams& p, hipStream_t stream)
{
  return launch_instance_pair<trace_instance_mesh_mb_kernel<PLUECKER, OCCLUDED, true>, trace_instance_mesh_mb_kernel<PLUECKER, OCCLUDED, false>>(p, stream);
}

} // namespace dev

hipError_t launch_trace_instance_mesh_mb(const LaunchParams& p, hipStream_t stream)
{
  if (p.counters) return hipErrorInvalidValue; // no instrumented twin (rt_trace.cpp refuses counted batches on scenes with instances)
  if (p.instHair == 2u) return p.exclOffsets ? hipErrorInvalidValue : launch_trace_instance_hair_mb(p, stream); // moving line or curve trees below the instances: the HAIRMB form, no EXCL twin either
  if (p.instHair) return p.exclOffsets ? hipErrorInvalidValue : launch_trace_instance_hair(p, stream); // line and curve trees below the instances: the HAIR form, which has no EXCL twin
  if (p.exclOffsets) return launch_trace_instance_filter(p, stream); // a re-trace of the host filter loop: the EXCL form (trace_instance_filter.hip)
  switch (p.accel.kind) {
  case ACCEL_INSTMESHMB_PLUECKER: return p.occluded ? dev::launch_instance_mesh_mb_vec<true, true>(p, stream) : dev::launch_instance_mesh_mb_vec<true, false>(p, stream);
  case ACCEL_INSTMESHMB_MOELLER: return p.occluded ? dev::launch_instance_mesh_mb_vec<false, true>(p, stream) : dev::launch_instance_mesh_mb_vec<false, false>(p, stream);
  default: return hipErrorInvalidValue;
  }
}

} // namespace rtamd
