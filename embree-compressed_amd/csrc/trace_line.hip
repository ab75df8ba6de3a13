// Line segment leaves of the quantized BVH8: flat linear curves (RTC_GEOMETRY_TYPE_FLAT_LINEAR_CURVE), Line4i.
// 48-byte records (LineRecord, accel.h) fetched as three dwordx4; every group of 4 records from the leaf start is one block with the
// reference's 4-wide SIMD semantics (LineMiIntersector1<4>, kernels/geometry/linei_intersector.h -> LineIntersector1<4>::intersect,
// line_intersector.h:64-98): all 4 tested against the tfar at block entry, one select_min, the lowest lane wins equal t
// (Intersect1EpilogM<4,4>); a later block sees the tfar the earlier one left and wins an equal t (`t <= tfar`).
// The test works in the ray's own space (Precalculations, line_intersector.h:53-58): s = rsqrt(dot(dir, dir)) and the transposed
// frame of s * dir - nine floats and s that depend on the ray only.  RayState and the octet exchange rows have no room for them and
// every other leaf shares those, so they are recomputed at each leaf visit (about 40 VALU operations, one division per rsqrt).
// One arithmetic serves the robust and the fast accel; only the node test differs.
// A ray exactly parallel to a segment's axis has d1 == 0 and takes its u from 0 * inf, as in the reference.
#include "trace_leaf.hip.h"
#include "trace_line.hip.h"

namespace rtamd {

hipError_t launch_trace_line(const LaunchParams& p, hipStream_t stream)
{
  // one leaf; robust traversal for RTC_SCENE_FLAG_ROBUST scenes, fast traversal otherwise
  const bool robust = p.accel.kind == ACCEL_LINE_ROBUST;
  if (p.poolKernel) return robust ? dev::launch_leaf_pool<dev::LineLeaf, true>(p, stream) : dev::launch_leaf_pool<dev::LineLeaf, false>(p, stream);
  return robust ? dev::launch_leaf<dev::LineLeaf, true>(p, stream) : dev::launch_leaf<dev::LineLeaf, false>(p, stream);
}

} // namespace rtamd
