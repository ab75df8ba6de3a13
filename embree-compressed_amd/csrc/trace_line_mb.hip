// Motion-blur line segment leaves of the quantized BVH8: flat linear curves with time steps, Line4i with a time (LineMiMBIntersector1<4>,
// kernels/geometry/linei_intersector.h -> LineMi::gather(..., time), linei.h:258-278 -> LineIntersector1<4>::intersect).
// 80-byte records (LineMBRecord, accel.h) fetched as five dwordx4: the two end points, radii in w, at both ends of ONE time segment of
// the geometry, and the ids.
//   time segment     as for the motion-blur triangles (trace_mb.hip.h time_segment, geometry.h:28-34); a record is tested only when the
//                    ray's itime equals the record's segment, checked before any arithmetic
//   interpolation    lerp(p0, p1, f) = madd(1 - f, p0, f * p1) on Vec4vf (linei.h:276-277, vec4.h:179): ALL FOUR components, so the
//                    radius is interpolated like a coordinate: lerp_vertex4 of trace_mb.hip.h (lerp_vertex zeroes w and cannot serve)
//   test             line_test of the static leaf on the interpolated end points (trace_line.hip.h); the ray space is recomputed per
//                    leaf visit, as there
// Blocks are groups of 4 RECORDS from the leaf start with the static leaf's rules: all tested records of a block see the tfar at block
// entry, the lowest lane wins ties, a later block wins an equal t (`t <= tfar`); any-hit returns at the first valid candidate.
// The ray's time is read from the ray record, word 7, through the ray's index (trace_mb.hip.h ray_time).  No pool form and no service
// kernel, like the other motion-blur leaves.
#include "trace_leaf.hip.h"
#include "trace_line_mb.hip.h"

namespace rtamd {
hipError_t launch_trace_line_mb(const LaunchParams& p, hipStream_t stream)
{
  // one leaf arithmetic; robust / fast traversal by the kind, swept / time-dependent nodes by the kind; lane kernel only (rt_trace.cpp
  // launch_on never asks for the ray-pool skeleton on this accel)
  if (p.accel.kind == ACCEL_LINEMB_LINEAR_ROBUST) return dev::launch_leaf<dev::LineMBLeafLinear, true>(p, stream);
  if (p.accel.kind == ACCEL_LINEMB_LINEAR_FAST) return dev::launch_leaf<dev::LineMBLeafLinear, false>(p, stream);
  if (p.accel.kind == ACCEL_LINEMB_ROBUST) return dev::launch_leaf<dev::LineMBLeaf, true>(p, stream);
  return dev::launch_leaf<dev::LineMBLeaf, false>(p, stream);
}

} // namespace rtamd
