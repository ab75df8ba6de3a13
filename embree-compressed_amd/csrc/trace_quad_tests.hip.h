// The triangle tests of the quad leaves (trace_quad.hip, trace_quad_mb.hip): Pluecker / Moeller-Trumbore on one triangle of a quad,
// with the u / v mapping and the negated normal of triangle B.  Under the rule of trace_leaf.hip.h (same instructions as with the
// functions in the leaf's own unit).
#pragma once
#include "trace_leaf.hip.h"

namespace rtamd {
namespace dev {

// Moeller-Trumbore on the triangle (a, b, c) of a quad, edges formed as the reference's vertex form does (e1 = a - b, e2 = c - a,
// MoellerTrumboreIntersector1::intersect(ray, v0, v1, v2), triangle_intersector_moeller.h); the test itself is moeller()'s.
// flip: triangle B of the quad - U / V are mapped before the division and the normal is negated.
__device__ __forceinline__ bool moeller_quad(const RayState& r, const float4 a, const float4 b, const float4 c, float tfarBlock, bool flip, TriHit& h)
{
  const float e1x = a.x - b.x, e1y = a.y - b.y, e1z = a.z - b.z;
  const float e2x = c.x - a.x, e2y = c.y - a.y, e2z = c.z - a.z;
  const float ngx = msub(e2y, e1z, e2z * e1y), ngy = msub(e2z, e1x, e2x * e1z), ngz = msub(e2x, e1y, e2y * e1x);
  const float cx = a.x - r.ox, cy = a.y - r.oy, cz = a.z - r.oz;
  const float rx = msub(cy, r.dz, cz * r.dy), ry = msub(cz, r.dx, cx * r.dz), rz = msub(cx, r.dy, cy * r.dx);
  const float den = dot3(ngx, ngy, ngz, r.dx, r.dy, r.dz);
  const float absDen = fabsf(den);
  const uint32_t sgnDen = __float_as_uint(den) & 0x80000000u;
  const float U = xorf(dot3(rx, ry, rz, e2x, e2y, e2z), sgnDen);
  const float V = xorf(dot3(rx, ry, rz, e1x, e1y, e1z), sgnDen);
  if (!((den != 0.0f) & (U >= 0.0f) & (V >= 0.0f) & (U + V <= absDen))) return false;
  const float T = xorf(dot3(ngx, ngy, ngz, cx, cy, cz), sgnDen);
  h.Ts = T; h.absDen = absDen;
  if (!((absDen * r.tnear < T) & (T <= absDen * tfarBlock))) return false;
  const float rcpAbsDen = 1.0f / absDen;
  h.t = T * rcpAbsDen;
  h.u = (flip ? absDen - V : U) * rcpAbsDen;
  h.v = (flip ? absDen - U : V) * rcpAbsDen;
  const uint32_t s = flip ? 0x80000000u : 0u;
  h.ngx = xorf(ngx, s); h.ngy = xorf(ngy, s); h.ngz = xorf(ngz, s);
  return true;
}

// Pluecker on the triangle (a, b, c) of a quad: pluecker() unchanged, then the B mapping after the division.
__device__ __forceinline__ bool pluecker_quad(const RayState& r, const float4 a, const float4 b, const float4 c, float tfarBlock, bool flip, TriHit& h)
{
  if (!pluecker(r, a, b, c, tfarBlock, h)) return false;
  const float u = h.u, v = h.v;
  h.u = flip ? 1.0f - v : u;
  h.v = flip ? 1.0f - u : v;
  const uint32_t s = flip ? 0x80000000u : 0u;
  h.ngx = xorf(h.ngx, s); h.ngy = xorf(h.ngy, s); h.ngz = xorf(h.ngz, s);
  return true;
}

} // namespace dev
} // namespace rtamd
