// Single-level instancing (RTC_GEOMETRY_TYPE_INSTANCE, one time step): a two-level traversal kernel of its own, one ray per lane.
// This file describes the kernel and launches its 32 instantiations; the kernel template is in trace_instance.hip.h, beside the list of the
// other forms' units, and its body, one text for all of them, in trace_instance_body.hip.h.
// The accel (accel.h InstanceRecord, rt_scene.cpp build_instance_accel) is ONE node array: a top-level BVH8 over the instances' world
// bounds with one instance per leaf, and behind it the triangle trees of the instanced scenes, rebased, over one TriRecord array.
// Per ray:
//   1. the top-level tree is traversed in world space (the loop of bvh_intersector1.cpp:40-126 / :128-209, as trace_loop.hip.h);
//   2. at an instance leaf the ray enters the instance (instance_intersector.cpp:51-59): org' = xfmPoint(world2local, org)
//      (affinespace.h:110), dir' = xfmVector(world2local, dir) (linearspace3.h:169), tnear and tfar unchanged - t is common to both
//      spaces; the node-test constants are re-derived from the local ray, an exit marker (REF_INST_EXIT) goes on the stack and the
//      traversal continues at the instanced scene's root with the same stack;
//   3. triangle leaves below are TriLeaf::intersect (trace_tri.hip.h), the top-level leaf, on the local ray (written out in the body for
//      the triangle-only forms, which says why): all records of a block of 4 see the tfar at block entry, the lowest lane wins ties, a
//      later block replaces an equal t.  A hit the leaf commits is this instance's; it keeps the instanced scene's geomID / primID and
//      Ng, u, v as computed in LOCAL space (the reference does not transform Ng), and the instance's geomID as instID
//      (instance_intersector.cpp:57), whatever the context's instID[0] holds;
//   4. popping the marker restores the world-space ray (read again through the ray's index) and its node-test constants
//      (instance_intersector.cpp:61-62).
// What a world-space entry below the marker was stacked with - its entry distance - is compared with the ray's tfar as ever: t is common.
// From the shared headers: LaunchParams, the 64 work queues with chunked grabs, the stack[entry][lane] LDS layout with its HBM overflow
// columns and the `overflow` word, TravRay, the QNode8 decode and slab test with the reference's child order, pluecker / moeller /
// commit_hit, load_ray / store_hit.  No octet form, no ray-pool form, no root cull pre-pass, no service kernel, no instrumented twin
// (rt_trace.cpp launch_on, rt_service.cpp; counted batches on scenes with instances are refused).
//
// QUADS (accel kinds ACCEL_INST_PLUECKER / ACCEL_INST_MOELLER): an instanced scene may hold a quad tree next to, or instead of, its
// triangle tree.  Inside an instance the local ray traverses the triangle tree completely and then the quad tree, against the tfar the
// triangles left (the instanced scene's AccelN, scene.cpp:650-654) - so a quad at a bit-identical t replaces the triangle:
//   2'. entering an instance whose record has a quad root stacks a second marker (REF_INST_QUADS, the quad root in the entry's
//       distance word) above the exit marker and continues at the triangle root; without a triangle tree it starts in the quad tree;
//   3'. popping that marker sets the lane's ST_QUADS bit and continues at the quad root; with the bit set a leaf is
//       QuadLeaf::intersect (trace_quad.hip.h), the top-level leaf: 8 candidates per block of 4 records (A =
//       (v0, v1, v3) in lanes 0-3, B = (v2, v1, v3) in lanes 4-7), all against the tfar at block entry, one minimum, the lowest lane
//       wins ties, a later block replaces an equal t.  The QuadRecords lie behind the InstanceRecords in `blobs`, one 64-byte array;
//   4'. the exit marker clears the bit.
//
// XFMB (accel kinds ACCEL_INSTMB_*): instances may have time steps (instance motion blur, scene_instance.h:58-63,
// instance_intersector.cpp:51-56).  Entering an instance whose record names InstanceSteps (pad[1] != 0) the lane reads its ray's time
// through the ray's index, loads the two steps around it and computes world2local = inverse(lerp(step[itime], step[itime + 1], ftime))
// with the function the host exports (instance_xfm.h), in place of the record's matrix; everything after that - the transform of org
// and dir, the markers, the trees, leaving - is the static form.  A singular interpolated transform (det == 0 or a matrix that is
// not finite) is not entered: the lane pops instead and pushes nothing, where the reference would trace NaNs.  An instance with one
// time step in such a scene (pad[1] == 0) is entered through its record.
#include "trace_instance.hip.h"

namespace rtamd {

hipError_t launch_trace_instance(const LaunchParams& p, hipStream_t stream)
{
  if (p.counters) return hipErrorInvalidValue; // no instrumented twin (rt_trace.cpp refuses counted batches on scenes with instances)
  if (p.exclOffsets) return launch_trace_instance_filter(p, stream); // a re-trace of the host filter loop: the EXCL form (trace_instance_filter.hip)
  switch (p.accel.kind) {
  case ACCEL_INST_TRI_PLUECKER: return p.occluded ? dev::launch_instance_vec<true, true, false, false>(p, stream) : dev::launch_instance_vec<true, false, false, false>(p, stream);
  case ACCEL_INST_TRI_MOELLER: return p.occluded ? dev::launch_instance_vec<false, true, false, false>(p, stream) : dev::launch_instance_vec<false, false, false, false>(p, stream);
  case ACCEL_INST_PLUECKER: return p.occluded ? dev::launch_instance_vec<true, true, true, false>(p, stream) : dev::launch_instance_vec<true, false, true, false>(p, stream);
  case ACCEL_INST_MOELLER: return p.occluded ? dev::launch_instance_vec<false, true, true, false>(p, stream) : dev::launch_instance_vec<false, false, true, false>(p, stream);
  case ACCEL_INSTMB_TRI_PLUECKER: return p.occluded ? dev::launch_instance_vec<true, true, false, true>(p, stream) : dev::launch_instance_vec<true, false, false, true>(p, stream);
  case ACCEL_INSTMB_TRI_MOELLER: return p.occluded ? dev::launch_instance_vec<false, true, false, true>(p, stream) : dev::launch_instance_vec<false, false, false, true>(p, stream);
  case ACCEL_INSTMB_PLUECKER: return p.occluded ? dev::launch_instance_vec<true, true, true, true>(p, stream) : dev::launch_instance_vec<true, false, true, true>(p, stream);
  case ACCEL_INSTMB_MOELLER: return p.occluded ? dev::launch_instance_vec<false, true, true, true>(p, stream) : dev::launch_instance_vec<false, false, true, true>(p, stream);
  default: return hipErrorInvalidValue;
  }
}

} // namespace rtamd
