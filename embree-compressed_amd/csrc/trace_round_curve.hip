// Tube leaves of the quantized BVH8: round Bezier and B-spline curves (device config round_curves=1; Scene::roundCurveAccel, the kinds
// ACCEL_CURVE_ROBUST / ACCEL_CURVE_FAST with LaunchParams::roundCurves set).  The leaf and its arithmetic are described in
// trace_round_curve.hip.h; this unit holds its launcher and with it the kernels: the lane kernel only, octet form only
// (RoundCurveLeaf::OCTET_ONLY), robust traversal for RTC_SCENE_FLAG_ROBUST scenes and fast traversal otherwise.
#include "trace_round_curve.hip.h"

namespace rtamd {

hipError_t launch_trace_round_curve(const LaunchParams& p, hipStream_t stream)
{
  return p.accel.kind == ACCEL_CURVE_ROBUST ? dev::launch_leaf<dev::RoundCurveLeaf, true>(p, stream) : dev::launch_leaf<dev::RoundCurveLeaf, false>(p, stream);
}

} // namespace rtamd
