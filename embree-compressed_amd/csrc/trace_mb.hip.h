// What the motion-blur leaves share (trace_tri_mb.hip, trace_quad_mb.hip, trace_line_mb.hip, trace_curve_mb.hip): the ray's time, the time segment of a record, the
// interpolation of a vertex.  Stateless __forceinline__ helpers, under the rule of trace_leaf.hip.h: a leaf uses a helper only where
// its kernels stay the same instructions as with the helper in its own unit (tools/kernel_metadata.py --digest).
#pragma once
#include "trace_leaf.hip.h"

namespace rtamd {
namespace dev {

__device__ __forceinline__ float ray_time(const LaunchParams& P, uint32_t rayIdx)
{
  return ((const float*)((const char*)P.rays + (size_t)rayIdx * P.stride))[7];
}

// lerp(p0, p1, f) of the reference (math.h): madd(1 - f, p0, f * p1); w is not interpolated
__device__ __forceinline__ float4 lerp_vertex(const float4 p0, const float4 p1, float f)
{
  const float g = 1.0f - f;
  return make_float4(madd(g, p0.x, f * p1.x), madd(g, p0.y, f * p1.y), madd(g, p0.z, f * p1.z), 0.0f);
}

// lerp of a Vec4vf (the line and curve leaves, linei.h:276-277, scene_bezier_curves.h:138-158): the radius in w goes through the same
// madd as the coordinates
__device__ __forceinline__ float4 lerp_vertex4(const float4 p0, const float4 p1, float f)
{
  const float g = 1.0f - f;
  return make_float4(madd(g, p0.x, f * p1.x), madd(g, p0.y, f * p1.y), madd(g, p0.z, f * p1.z), madd(g, p0.w, f * p1.w));
}

// does the record with `segment` of a mesh with `numSegments` serve a ray at `time`?  f = ftime of the ray in that mesh
__device__ __forceinline__ bool time_segment(float time, uint32_t segment, uint32_t numSegments, float& f)
{
  const float S = (float)numSegments;
  const float ts = time * S;
  const float itimef = fminf(fmaxf(floorf(ts), 0.0f), S - 1.0f);
  f = ts - itimef;
  return (uint32_t)(int)itimef == segment;
}

} // namespace dev
} // namespace rtamd
