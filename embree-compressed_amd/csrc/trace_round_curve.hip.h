// The tube leaf: round Bezier and B-spline curves (RTC_GEOMETRY_TYPE_ROUND_BEZIER_CURVE / _ROUND_BSPLINE_CURVE, device config
// round_curves=1) on the records of the flat curves (CurveRecord, accel.h: the four native control points with their radii in w, geomID,
// primID; N = 0).  The surface of a curve P(u), r(u) is the set of points Q with dot(Q - P(u), P'(u)) = 0 and |Q - P(u)| = r(u) for a u
// in [0, 1]: no end caps, and the inside counts (a ray that starts in the tube hits where it leaves).  The leaf restates
// BezierCurve1Intersector1 + intersect_bezier_recursive_jacobian + intersect_bezier_iterative_jacobian
// (kernels/geometry/bezier_curve_intersector.h:68-247) in its 8-wide build (numBezierSubdivisions = 2), with CylinderN::intersect
// (cylinder.h:161-225) and HalfPlaneN::intersect (plane.h:56-67).  The eight lanes of an octet are that build's vector; every lane holds
// the ray and the current record.
//   moving the ray  dt = dot(0.25 (v0 + v1 + v2 + v3) - org, dir) / dot(dir, dir); the control points relative to org + dt dir, the ray
//                   parameters below relative to dt
//   one level       over [u0, u1]: lane k evaluates point and derivative at lerp(u0, u1, k / 7) (de Casteljau, evalN) and - lanes 0..6 -
//                   owns the sub-segment to the point of lane k + 1, which it fetches from that lane.  The sub-segment as a Bezier
//                   curve P0, P0 + dP0 s, P3 - dP3 s, P3 with s = (u1 - u0) / 21; its distance from the chord P0 P3 is at most the
//                   larger sqr_point_to_line_distance of the two scaled derivatives.  Outer cylinder around the chord (max w + that)
//                   (1 + 2 ulp), inner cylinder max(0, (1 - 2 ulp) (min w - that)); the half planes at P0 and P3 cut the outer
//                   cylinder's interval, inside [tnear - dt, tfar - dt]; what the inner cylinder leaves of it are the two candidates
//                   tp0 = [lo, min(hi, inner.lower)] and tp1 = [max(lo, inner.upper), hi].  A candidate is unstable where the inner
//                   cylinder is missed or |cos| of the ray and the inner normal is below 0.3
//   depths          the top level is depth 1; a candidate of depth d is refined by a level over its sub-segment while d < (unstable ? 3 : 2)
//                   and goes to Newton from that depth on: three levels at most, unrolled at compile time (level<DEPTH>), so that each
//                   level's per-lane state lives in named registers
//   Newton          at most five iterations of the 2x2 system in (u, t): f = dot(R, T), g = sqrt(dot(R, R) - f^2) - r(u) with R = Q(t) -
//                   P(u), T = normalize(P'(u)); from (u of the outer cylinder's hit, tp0.lower) for a front and (..., tp1.upper) for a back
//                   candidate.  Converged when |f| < 16 ulp max|P'| and |g| < 16 ulp max(|dir|, cmax), cmax the largest |component| of the
//                   relative control points (the reference: 16 ulp |dir|, which a short dir puts below g's own rounding); accepted when tnear < t + dt < tfar and
//                   0 <= u <= 1.  Hit: t + dt, u, v = 0, Ng = cross(cross(P', Rn), P'.w Rn + P') with Rn = normalize(R), not normalised,
//                   evaluated at the (u, t) that is reported (the reference: at the iterate before the last update)
// Order.  The reference walks a level's candidates one at a time, front to back (all tp0, then all tp1), each against the tfar the
// previous one left, and runs Newton per candidate.  HERE the lanes of a level whose candidates are ready for Newton iterate AT ONCE,
// each against the tfar at that point, followed by one 8-lane minimum (the lowest lane wins an equal t); the candidates that need a deeper
// level follow one by one, nearest first, through the one call site of level<DEPTH + 1>.  Chosen, not measured: it keeps Newton - the
// longest dependent chain of the leaf - on up to seven lanes instead of one.  A candidate that the reference skips because its interval
// starts behind a hit found meanwhile cannot hold a nearer root, so in exact arithmetic the nearest hit is the same; a filter re-trace
// finds the same bits, since nothing a candidate computes depends on another candidate's hit except the test against tfar.
// The records of a leaf one after the other in stored order, each against the tfar the previous one left.  Any-hit ends at the first
// accepted candidate.  A converged candidate listed for the ray in the exclusion list (keyed by t: entry and exit of a tube share geomID
// and primID) is dropped before it may shorten tfar, as in the ribbon leaf.
// Every loop is wave-uniform (__ballot): the lane exchange and the 8-lane minimum need all lanes of an octet present; an octet that has
// nothing to do at a level runs it masked.
// Forms: octet only (OCTET_ONLY, as the grid-cell leaf): no lane-per-ray form, no ray-pool kernel, no service kernel.  One arithmetic
// serves the robust and the fast accel; only the node test differs.
#pragma once
#include "trace_curve.hip.h"

namespace rtamd {
namespace dev {

#define RC_ULP 1.1920928955078125e-07f // float(ulp): std::numeric_limits<float>::epsilon()

// lerp(v0, v1, t) = madd(1 - t, v0, t * v1) (math.h:273-276)
__device__ __forceinline__ float rc_lerp(float a, float b, float t) { return madd(1.0f - t, a, t * b); }
__device__ __forceinline__ float4 rc_lerp4(const float4 a, const float4 b, float t)
{
  return make_float4(rc_lerp(a.x, b.x, t), rc_lerp(a.y, b.y, t), rc_lerp(a.z, b.z, t), rc_lerp(a.w, b.w, t));
}
__device__ __forceinline__ float rc_rsqrt(float v) { return 1.0f / sqrtf(v); }

// what a pass keeps per octet while it works on one record: every lane of the octet holds the same values
struct RoundCtx
{
  float dx, dy, dz;      // ray direction
  float tnear, tfar, dt; // the ray's interval (tfar shrinks with every hit) and the shift of the ray parameter
  const float4* lp;      // the record: its four control points are read again by every evaluation (sixteen registers less across the levels)
  float qx, qy, qz;      // org + dt * dir: the control points are taken relative to it
  bool alive;            // the octet still works on this record (any-hit: false once a candidate is accepted)
};

// BezierCurve3fa::evalN (bezier_curve.h:177-193): point and derivative at t, all four components
__device__ __forceinline__ void rc_points(const RoundCtx& c, float4& p0, float4& p1, float4& p2, float4& p3)
{
  const float4* lp = c.lp;
  asm volatile("" : "+v"(lp)); // opaque: otherwise the loads of two evaluations are merged and the points stay live in between
  p0 = lp[0]; p1 = lp[1]; p2 = lp[2]; p3 = lp[3];
  p0.x -= c.qx; p0.y -= c.qy; p0.z -= c.qz;
  p1.x -= c.qx; p1.y -= c.qy; p1.z -= c.qz;
  p2.x -= c.qx; p2.y -= c.qy; p2.z -= c.qz;
  p3.x -= c.qx; p3.y -= c.qy; p3.z -= c.qz;
}
__device__ __forceinline__ void rc_eval(const float4 c_p0, const float4 c_p1, const float4 c_p2, const float4 c_p3, float t, float4& p, float4& dp)
{
  const float4 p10 = rc_lerp4(c_p0, c_p1, t), p11 = rc_lerp4(c_p1, c_p2, t), p12 = rc_lerp4(c_p2, c_p3, t);
  const float4 p20 = rc_lerp4(p10, p11, t), p21 = rc_lerp4(p11, p12, t);
  p = rc_lerp4(p20, p21, t);
  dp = make_float4(3.0f * (p21.x - p20.x), 3.0f * (p21.y - p20.y), 3.0f * (p21.z - p20.z), 3.0f * (p21.w - p20.w));
}

// CylinderN::intersect around the chord from P0 (P3 - P0 = d, rl = 1 / |d|) with squared radius rr, for a ray from the origin: the
// interval [lo, hi] (empty = [+inf, -inf]), the parallel special case included; u and Ng of the near (FAR = false) or far hit
struct RoundCyl
{
  float A, B, C0, dOz, Oz, eps; // the quadratic without the radius: C = C0 - rr
};
__device__ __forceinline__ RoundCyl rc_cylinder_setup(const RoundCtx& c, const float4 P0, float dx, float dy, float dz, float rl)
{
  const float ax = dx * rl, ay = dy * rl, az = dz * rl; // dP = (p1 - p0) * rl
  const float ox = 0.0f - P0.x, oy = 0.0f - P0.y, oz = 0.0f - P0.z; // O = org - P0
  const float dOdO = dot3(c.dx, c.dy, c.dz, c.dx, c.dy, c.dz);
  const float OdO = dot3(c.dx, c.dy, c.dz, ox, oy, oz);
  const float OO = dot3(ox, oy, oz, ox, oy, oz);
  RoundCyl q;
  q.dOz = dot3(ax, ay, az, c.dx, c.dy, c.dz);
  q.Oz = dot3(ax, ay, az, ox, oy, oz);
  q.A = dOdO - q.dOz * q.dOz;
  q.B = 2.0f * (OdO - q.dOz * q.Oz);
  q.C0 = OO - q.Oz * q.Oz;
  q.eps = 16.0f * RC_ULP * fmaxf(fabsf(dOdO), fabsf(q.dOz * q.dOz));
  return q;
}
__device__ __forceinline__ bool rc_cylinder(const RoundCyl& q, float rr, float& lo, float& hi)
{
  const float C = q.C0 - rr;
  const float D = q.B * q.B - 4.0f * q.A * C;
  bool valid = D >= 0.0f;
  const float Q = sqrtf(D);
  const float rcp2A = 1.0f / (2.0f * q.A);
  lo = valid ? (-q.B - Q) * rcp2A : RT_INF;
  hi = valid ? (-q.B + Q) * rcp2A : -RT_INF;
  if (valid && fabsf(q.A) < q.eps) { // rays parallel to the cylinder
    const bool inside = C <= 0.0f;
    lo = inside ? -RT_INF : RT_INF;
    hi = inside ? RT_INF : -RT_INF;
    valid = inside;
  }
  return valid;
}

// HalfPlaneN::intersect for a ray from the origin: the half line on the side of the plane through Pp that N points away from... as the
// reference has it: lower = (eps | DN < 0) ? -inf : t, upper = (eps | DN > 0) ? +inf : t with t = -ON / DN
__device__ __forceinline__ void rc_half_plane(const RoundCtx& c, float px, float py, float pz, float nx, float ny, float nz, float& lo, float& hi)
{
  const float ON = dot3(0.0f - px, 0.0f - py, 0.0f - pz, nx, ny, nz);
  const float DN = dot3(c.dx, c.dy, c.dz, nx, ny, nz);
  const bool eps = fabsf(DN) < 1e-18f; // min_rcp_input
  const float t = -ON * (1.0f / DN);
  lo = (eps || DN < 0.0f) ? -RT_INF : t;
  hi = (eps || DN > 0.0f) ? RT_INF : t;
}

// sqr_point_to_line_distance(PmQ0, Q1mQ0) (vec3.h:230-235)
__device__ __forceinline__ float rc_sqr_dist(float px, float py, float pz, float dx, float dy, float dz)
{
  const float nx = msub(py, dz, pz * dy), ny = msub(pz, dx, px * dz), nz = msub(px, dy, py * dx);
  return dot3(nx, ny, nz, nx, ny, nz) * (1.0f / dot3(dx, dy, dz, dx, dy, dz));
}

// intersect_bezier_iterative_jacobian from (u, t), on this lane alone.  true: converged and accepted, h holds the hit (t with dt added)
__device__ __forceinline__ bool rc_newton(const RoundCtx& c, float u, float t, TriHit& h)
{
  // The scale of the bound on g.  The reference has |dir| alone; g is a distance in world units, and its float32 error is a few ulp of
  // what enters R = Q - P: the control points relative to the ray's reference point.  Under a short unnormalised direction (|dir| below
  // the curve's extent) 16 ulp |dir| drops below that error, Newton never "converges", and the front hit is lost to the back of the tube,
  // to another curve or to a miss.  HERE the scale is max(|dir|, cmax) with cmax the largest |x|, |y|, |z|, |w| of the four relative
  // control points: the same bits as the reference's bound wherever |dir| >= cmax, a bound the arithmetic can meet everywhere else
  float gScale = sqrtf(dot3(c.dx, c.dy, c.dz, c.dx, c.dy, c.dz));
  {
    float4 c0, c1, c2, c3;
    rc_points(c, c0, c1, c2, c3);
    const float m0 = fmaxf(fmaxf(fabsf(c0.x), fabsf(c0.y)), fmaxf(fabsf(c0.z), fabsf(c0.w)));
    const float m1 = fmaxf(fmaxf(fabsf(c1.x), fabsf(c1.y)), fmaxf(fabsf(c1.z), fabsf(c1.w)));
    const float m2 = fmaxf(fmaxf(fabsf(c2.x), fabsf(c2.y)), fmaxf(fabsf(c2.z), fabsf(c2.w)));
    const float m3 = fmaxf(fmaxf(fabsf(c3.x), fabsf(c3.y)), fmaxf(fabsf(c3.z), fabsf(c3.w)));
    gScale = fmaxf(gScale, fmaxf(fmaxf(m0, m1), fmaxf(m2, m3)));
  }
#pragma nounroll
  for (int i = 0; i < 5; i++) {
    const float qx = t * c.dx, qy = t * c.dy, qz = t * c.dz; // Q = madd(t, dir, org) with org = 0
    float4 c0, c1, c2, c3, p, dp;
    rc_points(c, c0, c1, c2, c3);
    rc_eval(c0, c1, c2, c3, u, p, dp);
    // eval_dudu: BezierBasis::derivative2 (bezier_curve.h:51-61)
    const float t1 = u, t0 = 1.0f - t1;
    const float b0 = 6.0f * t0, b1 = 6.0f * madd(-2.0f, t0, t1), b2 = 6.0f * madd(-2.0f, t1, t0), b3 = 6.0f * t1;
    const float ddx = bezier_combine(b0, b1, b2, b3, c0.x, c1.x, c2.x, c3.x);
    const float ddy = bezier_combine(b0, b1, b2, b3, c0.y, c1.y, c2.y, c3.y);
    const float ddz = bezier_combine(b0, b1, b2, b3, c0.z, c1.z, c2.z, c3.z);
    const float rx = qx - p.x, ry = qy - p.y, rz = qz - p.z; // R = Q - P; dRdu = -dPdu, dRdt = dir
    const float pp = dot3(dp.x, dp.y, dp.z, dp.x, dp.y, dp.z);
    const float rsPP = rc_rsqrt(pp);
    const float Tx = dp.x * rsPP, Ty = dp.y * rsPP, Tz = dp.z * rsPP; // T = normalize(dPdu)
    // dTdu = dnormalize(dPdu, ddPdu) = (pp * ddp - pdp * dp) * rcp(pp) * rsqrt(pp) (vec3fa.h:321-326)
    const float pdp = dot3(dp.x, dp.y, dp.z, ddx, ddy, ddz);
    const float sc = (1.0f / pp) * rsPP;
    const float dTx = (pp * ddx - pdp * dp.x) * sc, dTy = (pp * ddy - pdp * dp.y) * sc, dTz = (pp * ddz - pdp * dp.z) * sc;
    const float f = dot3(rx, ry, rz, Tx, Ty, Tz);
    const float dfdu = dot3(-dp.x, -dp.y, -dp.z, Tx, Ty, Tz) + dot3(rx, ry, rz, dTx, dTy, dTz);
    const float dfdt = dot3(c.dx, c.dy, c.dz, Tx, Ty, Tz);
    const float K = dot3(rx, ry, rz, rx, ry, rz) - f * f;
    const float dKdu = dot3(rx, ry, rz, -dp.x, -dp.y, -dp.z) - f * dfdu;
    const float dKdt = dot3(rx, ry, rz, c.dx, c.dy, c.dz) - f * dfdt;
    const float rsK = rc_rsqrt(K);
    const float g = sqrtf(K) - p.w;
    const float dgdu = dKdu * rsK - dp.w;
    const float dgdt = dKdt * rsK;
    // dut = rcp(J) * (f, g) with J = (dfdu, dfdt; dgdu, dgdt)
    const float rdet = 1.0f / (dfdu * dgdt - dfdt * dgdu);
    u -= (dgdt * f - dfdt * g) * rdet;
    t -= (dfdu * g - dgdu * f) * rdet;
    const bool convU = fabsf(f) < 16.0f * RC_ULP * fmaxf(fmaxf(fabsf(dp.x), fabsf(dp.y)), fabsf(dp.z));
    const bool convT = fabsf(g) < 16.0f * RC_ULP * gScale;
    if (convU && convT) {
      const float th = t + c.dt;
      if (!(th > c.tnear && th < c.tfar)) return false; // rejects NaNs
      if (!(u >= 0.0f && u <= 1.0f)) return false;
      // The normal at the hit that is reported: point, derivative and R once more at the updated (u, t).  The reference takes them from
      // the iterate before the update, up to 16 ulp |dir| off the surface - on a thin tube (radius 1e-3 |dir|) a turn of the normal by 1e-2
      rc_points(c, c0, c1, c2, c3);
      rc_eval(c0, c1, c2, c3, u, p, dp);
      const float sx = t * c.dx - p.x, sy = t * c.dy - p.y, sz = t * c.dz - p.z;
      const float rs = rc_rsqrt(dot3(sx, sy, sz, sx, sy, sz));
      const float nx = sx * rs, ny = sy * rs, nz = sz * rs;                                  // R = normalize(Q - P)
      const float ux = madd(dp.w, nx, dp.x), uy = madd(dp.w, ny, dp.y), uz = madd(dp.w, nz, dp.z); // U = madd(dPdu.w, R, dPdu)
      const float vx = msub(dp.y, nz, dp.z * ny), vy = msub(dp.z, nx, dp.x * nz), vz = msub(dp.x, ny, dp.y * nx); // V = cross(dPdu, R)
      h.t = th;
      h.u = u;
      h.v = 0.0f;
      h.ngx = msub(vy, uz, vz * uy); h.ngy = msub(vz, ux, vx * uz); h.ngz = msub(vx, uy, vy * ux); // cross(V, U)
      return true;
    }
  }
  return false;
}

struct RoundCurveLeaf : LeafTraits
{
  static constexpr bool OCTET_ONLY = true; // the lane kernel tests these leaves eight lanes per ray, always
  // Two waves per SIMD (at most 256 VGPRs): bounded at three (168) the closest-hit kernels spill 35 registers (128 bytes of scratch per lane) - the three
  // levels fit, Newton below the third does not (profiles/round_curve_kernel_resources.txt)
  static constexpr int MIN_WAVES = 2;

  // One level of intersect_bezier_recursive_jacobian over [u0, u1] for the octets with `active` set; the others run it masked.
  template <int DEPTH, bool OCCLUDED>
  static __device__ __forceinline__ void level(const LaunchParams& P, float* x, uint32_t lid, RoundCtx& c, float u0, float u1, bool active)
  {
    const uint32_t k = lid & 7u;
    // subdivide curve: this lane's point, the next lane's as the end of this lane's sub-segment
    const float dscale = (u1 - u0) * (1.0f / (3.0f * 7.0f));
    const float vu = rc_lerp(u0, u1, (float)k * (1.0f / 7.0f));
    float4 P0, dP0;
    {
      float4 c0, c1, c2, c3;
      rc_points(c, c0, c1, c2, c3);
      rc_eval(c0, c1, c2, c3, vu, P0, dP0);
    }
    dP0.x *= dscale; dP0.y *= dscale; dP0.z *= dscale; dP0.w *= dscale;
    float4 P3, dP3; // shift_right_1: lane k + 1 of the octet (lane 7 reads outside it and is masked)
    P3.x = __shfl_down(P0.x, 1); P3.y = __shfl_down(P0.y, 1); P3.z = __shfl_down(P0.z, 1); P3.w = __shfl_down(P0.w, 1);
    dP3.x = __shfl_down(dP0.x, 1); dP3.y = __shfl_down(dP0.y, 1); dP3.z = __shfl_down(dP0.z, 1); dP3.w = __shfl_down(dP0.w, 1);
    bool valid = active && c.alive && k < 7u;
    const float P1w = P0.w + dP0.w, P2w = P3.w - dP3.w;
    const float ex = P3.x - P0.x, ey = P3.y - P0.y, ez = P3.z - P0.z;
    // bounding cylinders
    const float rr1 = rc_sqr_dist(dP0.x, dP0.y, dP0.z, ex, ey, ez), rr2 = rc_sqr_dist(dP3.x, dP3.y, dP3.z, ex, ey, ez);
    const float maxr12 = sqrtf(fmaxf(rr1, rr2));
    float rOuter = fmaxf(fmaxf(P0.w, P1w), fmaxf(P2w, P3.w)) + maxr12;
    float rInner = fminf(fminf(P0.w, P1w), fminf(P2w, P3.w)) - maxr12;
    rOuter = (1.0f + 2.0f * RC_ULP) * rOuter;
    rInner = fmaxf(0.0f, (1.0f - 2.0f * RC_ULP) * rInner);
    const float rl = rc_rsqrt(dot3(ex, ey, ez, ex, ey, ez));
    const RoundCyl cyl = rc_cylinder_setup(c, P0, ex, ey, ez, rl);
    float oLo, oHi;
    valid &= rc_cylinder(cyl, rOuter * rOuter, oLo, oHi);
    // cap planes
    float tpLo = fmaxf(c.tnear - c.dt, oLo), tpHi = fminf(c.tfar - c.dt, oHi);
    float hLo, hHi;
    rc_half_plane(c, P0.x, P0.y, P0.z, dP0.x, dP0.y, dP0.z, hLo, hHi);
    tpLo = fmaxf(tpLo, hLo); tpHi = fminf(tpHi, hHi);
    rc_half_plane(c, P3.x, P3.y, P3.z, -dP3.x, -dP3.y, -dP3.z, hLo, hHi);
    tpLo = fmaxf(tpLo, hLo); tpHi = fminf(tpHi, hHi);
    valid &= tpLo <= tpHi;
    // inner cylinder and the unstable areas
    float iLo, iHi;
    const bool validInner = rc_cylinder(cyl, rInner * rInner, iLo, iHi);
    const float rsDir = rc_rsqrt(dot3(c.dx, c.dy, c.dz, c.dx, c.dy, c.dz));
    const float ndx = c.dx * rsDir, ndy = c.dy * rsDir, ndz = c.dz * rsDir;
    // u and Ng of a cylinder hit at t (cylinder.h:195-209): u = madd(t, dOz, Oz) * rl, Ng = t * dir - madd(u, p1 - p0, p0)
    auto cyl_u = [&](float t) { return madd(t, cyl.dOz, cyl.Oz) * rl; };
    auto unstable_at = [&](float t) {
      const float uc = cyl_u(t);
      const float nx = t * c.dx - madd(uc, ex, P0.x), ny = t * c.dy - madd(uc, ey, P0.y), nz = t * c.dz - madd(uc, ez, P0.z);
      const float rs = rc_rsqrt(dot3(nx, ny, nz, nx, ny, nz));
      return !validInner || fabsf(dot3(ndx, ndy, ndz, nx * rs, ny * rs, nz * rs)) < 0.3f;
    };
    const bool unstable0 = unstable_at(iLo), unstable1 = unstable_at(iHi);
    // subtract the inner interval: the front and the back candidate
    const float t0Hi = fminf(tpHi, iLo), t1Lo = fmaxf(tpLo, iHi);
    bool valid0 = valid && tpLo <= t0Hi, valid1 = valid && t1Lo <= tpHi;
    // the Newton start parameters: the outer cylinder's u, clamped, in the curve's parameter (the reference divides by VSIZEX here)
    const float uo0 = rc_lerp(u0, u1, ((float)k + fminf(fmaxf(cyl_u(oLo), 0.0f), 1.0f)) * (1.0f / 8.0f));
    const float uo1 = rc_lerp(u0, u1, ((float)k + fminf(fmaxf(cyl_u(oHi), 0.0f), 1.0f)) * (1.0f / 8.0f));

#pragma nounroll
    for (int phase = 0; phase < 2; phase++) { // all front candidates, then all back candidates
      const float tlo = phase ? t1Lo : tpLo;
      const bool unstable = phase ? unstable1 : unstable0;
      bool cand = (phase ? valid1 : valid0) && c.alive && tlo + c.dt <= c.tfar;
      if constexpr (DEPTH >= 2) { // candidates that have reached their depth: Newton on all their lanes at once
        const bool ready = cand && (DEPTH >= 3 || !unstable);
        if (__ballot(ready) != 0ull) {
          TriHit h;
          h.t = RT_INF;
          bool ok = ready && rc_newton(c, phase ? uo1 : uo0, phase ? tpHi : tpLo, h);
          // (geomID, primID of the record and the ray's index are read again here: three registers less across the levels)
          const uint2 ids = *(const uint2*)(c.lp + 4);
          if (ok && P.exclOffsets) ok = !candidate_excluded(P, __float_as_uint(x[10]), ids.x, ids.y, h.t);
          if (OCCLUDED) {
            if (octet_ballot(ok, lid) != 0u) {
              if (k == 0u) x[9] = __uint_as_float(1u);
              c.alive = false;
            }
          } else {
            const float tmin = octet_min8(ok ? h.t : RT_INF);
            const uint32_t w = octet_ballot(ok && h.t == tmin, lid);
            if (w != 0u && k == (uint32_t)__ffs(w) - 1u) row_write_hit(x, h, ids.x, ids.y); // the lowest lane wins an equal t
            c.tfar = w != 0u ? tmin : c.tfar;
          }
        }
        cand = cand && !ready;
      }
      if constexpr (DEPTH < 3) { // the others one level deeper, nearest first
        cand = cand && c.alive;
        while (__ballot(cand) != 0ull) {
          const float tmin = octet_min8(cand ? tlo : RT_INF);
          const uint32_t w = octet_ballot(cand && tlo == tmin, lid); // select_min: the lowest lane among equal minima
          const uint32_t sel = w != 0u ? (uint32_t)__ffs(w) - 1u : 0u;
          if (k == sel) cand = false;
          // vu0[i], vu0[i + 1] of the selected sub-segment, as its lanes computed them
          const float a = rc_lerp(u0, u1, (float)sel * (1.0f / 7.0f)), b = rc_lerp(u0, u1, (float)(sel + 1u) * (1.0f / 7.0f));
          level<DEPTH + 1, OCCLUDED>(P, x, lid, c, a, b, w != 0u);
          cand = cand && c.alive && tlo + c.dt <= c.tfar;
        }
      }
    }
  }

  // Child-parallel form (trace_loop.hip.h): the records of the leaf of the ray in exchange row `x` one after the other (words 0..7 = org,
  // tnear, dir, tfar; word 8 = leaf ref; word 10 = the ray's index).  A hit goes into the row (words 0..7 = t, Ng, u, v, geomID, primID;
  // word 9 = 1), written by the lane that found it.
  template <bool OCCLUDED, bool COUNT>
  static __device__ __forceinline__ void octet_pass(const LaunchParams& P, float* x, bool valid, uint32_t lid, WorkCounters& wc)
  {
    const CurveRecord* __restrict__ recs = (const CurveRecord*)P.accel.blobs;
    const RayState r = row_ray(x);
    const uint32_t ref = __float_as_uint(x[8]);
    uint32_t first, cnt;
    leaf_range(ref, first, cnt);
    cnt = valid ? cnt : 0u;
    RoundCtx c;
    c.dx = r.dx; c.dy = r.dy; c.dz = r.dz;
    c.tnear = r.tnear; c.tfar = r.tfar;
    bool occludedDone = false;
    for (uint32_t i = 0; __ballot(i < cnt) != 0ull; i++) {
      const bool present = i < cnt && !occludedDone;
      const float4* lp = (const float4*)(recs + first + (i < cnt ? i : 0u));
      const float4 V0 = lp[0], V1 = lp[1], V2 = lp[2], V3 = lp[3];
      if (COUNT && present && (lid & 7u) == 0u) wc.prims++;
      // move ray closer to make intersection stable
      const float cx = 0.25f * (((V0.x + V1.x) + V2.x) + V3.x) - r.ox, cy = 0.25f * (((V0.y + V1.y) + V2.y) + V3.y) - r.oy,
                  cz = 0.25f * (((V0.z + V1.z) + V2.z) + V3.z) - r.oz;
      c.dt = dot3(cx, cy, cz, r.dx, r.dy, r.dz) * (1.0f / dot3(r.dx, r.dy, r.dz, r.dx, r.dy, r.dz));
      const float qx = madd(c.dt, r.dx, r.ox), qy = madd(c.dt, r.dy, r.oy), qz = madd(c.dt, r.dz, r.oz);
      c.lp = lp;
      c.qx = qx; c.qy = qy; c.qz = qz;
      c.alive = present;
      level<1, OCCLUDED>(P, x, lid, c, 0.0f, 1.0f, present);
      if (OCCLUDED && present && !c.alive) occludedDone = true; // Occluded1Epilog1: any accepted candidate
    }
  }
};

} // namespace dev
} // namespace rtamd
