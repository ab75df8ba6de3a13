// Motion-blur ribbon leaves of the quantized BVH8: flat Bezier and B-spline curves with time steps (Bezier1iIntersector1MB,
// kernels/geometry/bezier1i_intersector.h:126-162 -> NativeCurves::gather(..., float time), scene_bezier_curves.h:138-158 -> the ribbon
// intersector of the static path).
// 160-byte records (CurveMBRecord, accel.h) fetched as dwordx4: the four native (Bezier) control points, radii in w, at both ends of ONE
// time segment of the geometry, the id row (geomID, primID, segment, numSegments) and the tessellation rate N.
//   time segment     as for the other motion-blur leaves (trace_mb.hip.h time_segment, geometry.h:28-34); the id row is read first and a
//                    record is tested only when the ray's itime equals the record's segment, checked before any arithmetic.  Times outside
//                    [0, 1] extrapolate the first / last segment; a NaN time selects segment 0 with a NaN ftime, every control point
//                    becomes NaN and no quad is hit (max(U, V) is NaN, trace_curve.hip)
//   interpolation    each of the four control points is lerp(a, b, f) = madd(1 - f, a, f * b) on ALL FOUR components (lerp_vertex4 of
//                    trace_mb.hip.h): the radius goes through the same madd as the coordinates
//   test             from there on the static ribbon leaf on the interpolated points (trace_curve.hip, trace_curve.hip.h): ray space,
//                    the N segments in passes of 8, ribbon_end, ribbon_quad_test with `T <= absDen * tfar` and the self-hit rule, the
//                    record, pass and tie rules of that header; Ng = eval_du(u) of the interpolated WORLD control points
// The ray's time is read from the ray record, word 7, through the ray's index (trace_mb.hip.h ray_time).  Forms: lane-per-ray and octet.
// No pool form and no service kernel, like the other motion-blur leaves.  One arithmetic serves the robust and the fast accel.
#undef CURVE_BASIS_TABLE // (the table build of trace_curve.hip is a measurement of the static leaf alone)
#include "trace_curve_mb.hip.h"

namespace rtamd {
hipError_t launch_trace_curve_mb(const LaunchParams& p, hipStream_t stream)
{
  // one leaf arithmetic; robust / fast traversal by the kind, swept / time-dependent nodes by the kind; lane kernel only (rt_trace.cpp
  // launch_on never asks for the ray-pool skeleton on this accel)
  if (p.accel.kind == ACCEL_CURVEMB_LINEAR_ROBUST) return dev::launch_leaf<dev::CurveMBLeafLinear, true>(p, stream);
  if (p.accel.kind == ACCEL_CURVEMB_LINEAR_FAST) return dev::launch_leaf<dev::CurveMBLeafLinear, false>(p, stream);
  if (p.accel.kind == ACCEL_CURVEMB_ROBUST) return dev::launch_leaf<dev::CurveMBLeaf, true>(p, stream);
  return dev::launch_leaf<dev::CurveMBLeaf, false>(p, stream);
}

} // namespace rtamd
